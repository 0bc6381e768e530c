"""The benchmark's command line: --steps, the result line, --dump-outputs, --full.

Runs ``bench.py`` on a small history (300 trials, 4 dims) so that each run takes
a few seconds with or without a GPU.
"""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest


REPO = Path(__file__).resolve().parent.parent
STEPS, WARMUP, DIMS = 3, 1, 4


def _run_bench(out_dir: Path, *extra: str) -> dict:
    proc = subprocess.run(
        [
            sys.executable, str(REPO / "bench.py"),
            "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
            "--history", "300", "--dims", str(DIMS),
            "--dump-outputs", str(out_dir), *extra,
        ],  # fmt: skip
        cwd=REPO,
        capture_output=True,
        text=True,
        timeout=300,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, proc.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("bench")
    plain = _run_bench(root / "plain")
    full = _run_bench(root / "full", "--full")
    return root, plain, full


def test_result_line(runs) -> None:
    _, plain, full = runs
    for result in (plain, full):
        assert result["metric"] == "sampler suggest()/sec at 10k-trial history, 20-dim space"
        assert result["unit"] == "suggest/s"
        assert result["higher_is_better"] is True
        assert result["dtype"] == "fp64"
        assert result["steps"] == STEPS and result["warmup"] == WARMUP
        assert result["ms_per_step"] > 0
        # value and ms_per_step describe the same timed region
        assert result["value"] == pytest.approx(1000.0 / result["ms_per_step"], rel=1e-9)


def test_dump_outputs_hold_the_last_timed_step(runs) -> None:
    root, _, _ = runs
    params = np.load(root / "plain" / "params.npy")
    values = np.load(root / "plain" / "values.npy")
    assert params.dtype == np.float64 and params.shape == (DIMS,)
    assert values.dtype == np.float64 and values.shape == (1,)
    assert np.all((params >= -5.0) & (params <= 5.0))
    # The objective is a shifted sphere plus seeded noise, one draw per step:
    # the dumped value must be the one told in step WARMUP + STEPS.
    noise = np.random.RandomState(1234).randn(WARMUP + STEPS)[-1]
    assert values[0] == pytest.approx(np.sum((params - 1.0) ** 2) + 0.01 * noise, rel=1e-12)


def test_same_arguments_give_the_same_outputs(runs) -> None:
    root, _, _ = runs
    for name in ("params.npy", "values.npy"):
        assert np.array_equal(np.load(root / "plain" / name), np.load(root / "full" / name))
