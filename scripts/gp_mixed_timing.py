"""Time per suggest of a single-objective ``GPSampler`` study over a mixed
search space: 20 dimensions of which ``--categorical`` (default 5) are
categorical with 4 choices, on a history of ``--history`` trials.

Prints one line: the first ask + suggest + tell apart (cold fit, code-object
loads), then the median and minimum of ``--steps`` further ones, and where the
cached regressor lives. ``--categorical 0`` is the all-continuous study of the
same size, which shows what the categorical axes still cost.

It imports ``optuna_amd`` from the current directory and uses nothing the
categorical device path added, so it also runs from an export of an older
commit; that is how two builds are compared (alternate the two trees in one
job, each run under its own time limit).

A GPU is required; nothing here falls back.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.getcwd())
warnings.simplefilter("ignore")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import optuna_amd  # noqa: E402
from optuna_amd.distributions import CategoricalDistribution, FloatDistribution  # noqa: E402


D = 20
CHOICES = ["a", "b", "c", "d"]
# What a choice adds to the loss, per categorical axis: the best choice differs.
PENALTY = np.array([[0.0, 0.3, 0.6, 0.9], [0.5, 0.0, 0.2, 0.7], [0.4, 0.8, 0.0, 0.1],
                    [0.9, 0.3, 0.5, 0.0], [0.2, 0.0, 0.6, 0.4]])


def _loss(x: np.ndarray, codes: np.ndarray, rng: np.random.RandomState) -> float:
    """A smooth bowl in the continuous axes plus a per-choice penalty, and noise."""
    centre = np.where(np.arange(len(x)) % 2 == 0, 0.3, 0.7)
    out = float(np.sum((x - centre) ** 2))
    for k, c in enumerate(codes):
        out += float(PENALTY[k % len(PENALTY), c])
    return out + 0.02 * float(rng.randn())


def study_line(history: int, steps: int, n_cat: int) -> None:
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    floats = [f"x{i:02d}" for i in range(D - n_cat)]
    cats = [f"c{i:02d}" for i in range(n_cat)]
    dists = {n: FloatDistribution(0.0, 1.0) for n in floats}
    dists.update({n: CategoricalDistribution(CHOICES) for n in cats})
    sampler = optuna_amd.samplers.GPSampler(seed=0, n_startup_trials=10)
    study = optuna_amd.create_study(sampler=sampler)
    rng = np.random.RandomState(history)
    trials = []
    for _ in range(history):
        x = rng.rand(len(floats))
        codes = rng.randint(len(CHOICES), size=n_cat)
        params = {n: float(v) for n, v in zip(floats, x)}
        params.update({n: CHOICES[c] for n, c in zip(cats, codes)})
        trials.append(
            optuna_amd.create_trial(
                params=params, distributions=dists, value=_loss(x, codes, rng)
            )
        )
    study.add_trials(trials)

    def step() -> None:
        t = study.ask()
        x = np.array([t.suggest_float(n, 0.0, 1.0) for n in floats])
        codes = np.array(
            [CHOICES.index(t.suggest_categorical(n, CHOICES)) for n in cats], dtype=int
        )
        study.tell(t, _loss(x, codes, rng))

    t0 = time.perf_counter()
    step()  # cold fit, code-object loads
    first = time.perf_counter() - t0
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t0)
    gpr = sampler._gprs_cache_list[0]
    print(f"study history={history} dims={D} categorical={n_cat} "
          f"gp_device={gpr.device.type} dense_sqdiff={gpr._squared_X_diff is not None} "
          f"first_ms={1e3 * first:.0f} median_ms={1e3 * statistics.median(times):.1f} "
          f"min_ms={1e3 * min(times):.1f} max_ms={1e3 * max(times):.1f} steps={steps}",
          flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--history", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--categorical", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_mixed_timing: a GPU is required")
    if not 0 <= args.categorical <= D:
        raise SystemExit(f"gp_mixed_timing: need 0 <= --categorical <= {D}")
    study_line(args.history, args.steps, args.categorical)


if __name__ == "__main__":
    main()
