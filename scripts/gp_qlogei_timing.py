"""Timing of the fused qLogEI session against the torch path.

On one fitted device GP with R running trials, in one process, alternating:
the fused path and the torch evaluation forced through ``BaseAcquisitionFunc``
on the same object (the op chain every qLogEI call took before the session
existed), at the two shapes the sampler uses: B = 2048 without gradient for
the pre-sample evaluation and B = 10 with gradient for a local-search step.
Prints the table of docs/PERF.md's qLogEI section.

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

from optuna_amd._gp import acqf as acqf_mod  # noqa: E402
from optuna_amd._gp import gp as gp_mod  # noqa: E402
from optuna_amd._gp import prior  # noqa: E402
from optuna_amd._gp import search_space as gp_ss  # noqa: E402
from optuna_amd.distributions import FloatDistribution  # noqa: E402


def _timed_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()  # both paths end in a copy to the host
    return 1e3 * (time.perf_counter() - t0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--dims", type=int, default=20)
    ap.add_argument("--running", type=int, default=8)
    ap.add_argument("--qmc", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_qlogei_timing: a GPU is required")

    n, d = args.n, args.dims
    rng = np.random.RandomState(n)
    X = rng.rand(n, d)
    y = -np.sum((X - 0.6) ** 2, axis=1) + 0.02 * rng.randn(n)
    y = (y - y.mean()) / y.std()
    t0 = time.perf_counter()
    gpr = gp_mod.fit_kernel_params(
        X, y, np.zeros(d, dtype=bool), prior.default_log_prior, 1e-6, False
    )
    print(f"<!-- N={n} D={d}: fit in {time.perf_counter() - t0:.1f} s on {gpr.device} -->",
          flush=True)
    space = gp_ss.SearchSpace({f"x{i}": FloatDistribution(0.0, 1.0) for i in range(d)})
    acqf = acqf_mod.qLogEI(
        gpr, space, float(np.median(y)), 0.3 * rng.rand(args.running, d),
        n_qmc_samples=args.qmc, qmc_seed=1,
    )
    if acqf._fused_session() is None:
        raise SystemExit("gp_qlogei_timing: the fused path is not eligible here")
    base = acqf_mod.BaseAcquisitionFunc
    # Candidates around the optimum and running trials away from it, so that
    # part of the draws beat the fantasies and the last column compares more
    # than the fantasies' own mean.
    pre, loc = 0.4 + 0.4 * rng.rand(2048, d), 0.4 + 0.4 * rng.rand(10, d)

    print("| N | R | Q | shape | fused ms (median, min..max) | torch ms (median, min..max) | "
          "torch / fused | max rel diff f |")
    print("|---|---|---|---|---|---|---|---|")
    for shape, fused, forced in (
        ("B=2048 no grad", lambda: acqf.eval_acqf_no_grad(pre),
         lambda: base.eval_acqf_no_grad(acqf, pre)),
        ("B=10 with grad", lambda: acqf.eval_acqf_batched_with_grad(loc),
         lambda: base.eval_acqf_batched_with_grad(acqf, loc)),
    ):
        a, b = fused(), forced()
        a, b = (a[0], b[0]) if isinstance(a, tuple) else (a, b)
        diff = np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
        for _ in range(3):
            fused(), forced()
        tf, tt = [], []
        for _ in range(args.rounds):  # alternating: both see the same machine
            tf.append(_timed_ms(fused))
            tt.append(_timed_ms(forced))
        mf, mt = statistics.median(tf), statistics.median(tt)
        print(f"| {n} | {args.running} | {args.qmc} | {shape} | "
              f"{mf:.2f} ({min(tf):.2f}..{max(tf):.2f}) | {mt:.2f} ({min(tt):.2f}..{max(tt):.2f}) | "
              f"{mt / mf:.1f} | {diff:.1e} |", flush=True)


if __name__ == "__main__":
    main()
