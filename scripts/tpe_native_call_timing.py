"""Wall time of the fused TPE suggest's native calls on the headline workload.

Runs the configuration of ``bench.py`` defaults (TPE, single objective, 10k
history, 20 float dims, 24 candidates) and takes ``time.perf_counter`` around
every ``TpeDeviceHistory.fused_score`` call and, separately, around every
``fused_prepare`` call (a build without the early fit has none), every
``tpe_below_kernels`` call (the native fit of the below estimator; a build
without it has none) and the whole of ``TPESampler._sample_locked``. Prints one
JSON line with the median, the 10th/90th percentiles and min/max in
microseconds, plus the suggest+tell rate of the timed steps.

    python scripts/tpe_native_call_timing.py [--steps 300] [--warmup 16]
        [--history 10000] [--dims 20] [--label NAME]

Run it once per build under comparison, in the same job, from that build's
tree (the script imports whatever ``optuna_amd`` is first on ``sys.path``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np


sys.path.insert(0, os.getcwd())


class _TimedHistory:
    """Forwards to a ``TpeDeviceHistory``; times the two fused entry points."""

    def __init__(self, hist, times: dict[str, list[float]]) -> None:
        self._hist = hist
        self._times = times

    def __getattr__(self, name):
        attr = getattr(self._hist, name)
        if name not in self._times:
            return attr
        bucket = self._times[name]

        def timed(*args, **kwargs):
            t0 = time.perf_counter()
            out = attr(*args, **kwargs)
            bucket.append(time.perf_counter() - t0)
            return out

        return timed


def _stats(samples: list[float]) -> dict | None:
    if not samples:
        return None
    us = np.asarray(samples) * 1e6
    return {
        "n": int(len(us)),
        "median_us": round(float(np.median(us)), 2),
        "p10_us": round(float(np.percentile(us, 10)), 2),
        "p90_us": round(float(np.percentile(us, 90)), 2),
        "min_us": round(float(us.min()), 2),
        "max_us": round(float(us.max()), 2),
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--history", type=int, default=10000)
    ap.add_argument("--dims", type=int, default=20)
    ap.add_argument("--label", default="")
    args = ap.parse_args()

    import optuna_amd
    from optuna_amd.samplers._tpe import _device

    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    times: dict[str, list[float]] = {
        "fused_score": [], "fused_prepare": [], "tpe_below_kernels": [], "sample_locked": [],
        "fused_draw_score": [], "draw_below_native": [], "ppf": [], "score_fused": [],
        "best_candidate": [],
    }

    def timed(fn, bucket: list[float]):
        def wrapper(*args, **kwargs):
            t0 = time.perf_counter()
            out = fn(*args, **kwargs)
            bucket.append(time.perf_counter() - t0)
            return out

        return wrapper

    orig_init = _device._SpaceDeviceMirror.__init__

    def init(self, space):
        orig_init(self, space)
        self._hist = _TimedHistory(self._hist, times)

    _device._SpaceDeviceMirror.__init__ = init
    sampler_cls = optuna_amd.samplers.TPESampler
    sampler_cls._sample_locked = timed(sampler_cls._sample_locked, times["sample_locked"])
    sampler_cls._best_candidate = staticmethod(
        timed(sampler_cls._best_candidate, times["best_candidate"])
    )
    mirror_cls = _device._SpaceDeviceMirror
    mirror_cls.score_fused = timed(mirror_cls.score_fused, times["score_fused"])
    if hasattr(_device, "draw_below_native"):
        _device._tn.ppf = timed(_device._tn.ppf, times["ppf"])
        _device.draw_below_native = timed(
            _device.draw_below_native, times["draw_below_native"]
        )
    # A build from before the native below route has no such entry.
    orig_native = getattr(_device, "native_below", None)
    if orig_native is not None:
        wrapped: dict = {}

        def native_below(cache):
            fn = orig_native(cache)
            if fn is None or getattr(fn, "__name__", "") != "tpe_below_kernels":
                return fn  # none, or the draw route's entry (timed as fused_draw_score)
            if fn not in wrapped:
                wrapped[fn] = timed(fn, times["tpe_below_kernels"])
            return wrapped[fn]

        _device.native_below = native_below

    names = [f"x{i}" for i in range(args.dims)]
    dists = {n: optuna_amd.distributions.FloatDistribution(-5.0, 5.0) for n in names}
    study = optuna_amd.create_study(
        sampler=optuna_amd.samplers.TPESampler(seed=42, n_startup_trials=10)
    )
    rng0 = np.random.RandomState(0)
    params = rng0.uniform(-5.0, 5.0, size=(args.history, args.dims))
    values = rng0.rand(args.history)
    study.add_trials(
        [
            optuna_amd.create_trial(
                params={n: float(params[r, i]) for i, n in enumerate(names)},
                distributions=dists,
                value=float(values[r]),
            )
            for r in range(args.history)
        ]
    )
    rng = np.random.RandomState(1234)

    def one_step() -> None:
        trial = study.ask()
        x = np.array([trial.suggest_float(n, -5.0, 5.0) for n in names])
        study.tell(trial, float(np.sum((x - 1.0) ** 2) + 0.01 * rng.randn()))

    for _ in range(args.warmup):
        one_step()
    for bucket in times.values():
        del bucket[:]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    wall = time.perf_counter() - t0
    n_scored = len(times["fused_score"]) + len(times["fused_draw_score"])
    assert n_scored == args.steps, "the fused path was not taken"

    print(
        json.dumps(
            {
                "label": args.label,
                "steps": args.steps,
                "history": args.history,
                "dims": args.dims,
                "steps_per_s": round(args.steps / wall, 1),
                "fused_score": _stats(times["fused_score"]),
                "fused_prepare": _stats(times["fused_prepare"]),
                "tpe_below_kernels": _stats(times["tpe_below_kernels"]),
                "sample_locked": _stats(times["sample_locked"]),
                "fused_draw_score": _stats(times["fused_draw_score"]),
                "draw_below_native": _stats(times["draw_below_native"]),
                "ppf": _stats(times["ppf"]),
                "score_fused": _stats(times["score_fused"]),
                "best_candidate": _stats(times["best_candidate"]),
            }
        ),
        flush=True,
    )


if __name__ == "__main__":
    main()
