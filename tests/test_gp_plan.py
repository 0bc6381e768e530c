"""Host check of the GP sessions' chunk and split arithmetic
(``_hip/csrc/gp_plan.h``).

The header is plain C++17, so a stand-alone program (``tests/cpp/
gp_plan_check.cpp``) is compiled against it with the host compiler and run: for
every chunk of 1..70000 candidates and a maximum of 1, 2, 3, 40 and 4096
workgroups per candidate the split count lies in ``[1, max]`` and the chunk
writes fewer than ``GP_TARGET_BLOCKS + bc`` partial records, which is what the
partial buffer holds; a budget below one candidate gives chunks of one, a huge
one stops at the grid's 65535; the chunks cover the batch and one fewer would
not; and the chunk counts that the GPU tests pin (7 and 3) hold.
"""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest


_ROOT = Path(__file__).resolve().parent.parent
_CSRC = _ROOT / "optuna_amd" / "_hip" / "csrc"
_PROGRAM = Path(__file__).resolve().parent / "cpp" / "gp_plan_check.cpp"


def test_gp_plan_program(tmp_path) -> None:
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "gp_plan_check"
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{_CSRC}",
         str(_PROGRAM), "-o", str(exe)],
        check=True,
    )
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
