"""Host check of the workspace layout helper (``_hip/csrc/ws_layout.h``).

The header is plain C++17, so a stand-alone program (``tests/cpp/
ws_layout_check.cpp``) is compiled against it with the host compiler and run:
mixed double/int32/int64/uint8 slots are disjoint, in order, 8-aligned and
inside ``bytes()``; odd int32/uint8 counts (1, 3, 257) do not reach the next
slot; zero-length slots work; an all-double layout is exactly ``8 * sum(n)``
bytes; overflow throws.
"""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest


_ROOT = Path(__file__).resolve().parent.parent
_CSRC = _ROOT / "optuna_amd" / "_hip" / "csrc"
_PROGRAM = Path(__file__).resolve().parent / "cpp" / "ws_layout_check.cpp"


def test_ws_layout_program(tmp_path) -> None:
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "ws_layout_check"
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{_CSRC}",
         str(_PROGRAM), "-o", str(exe)],
        check=True,
    )
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
