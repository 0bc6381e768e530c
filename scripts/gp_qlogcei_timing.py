"""Timing of the fused qLogCEI session against the torch path.

On one fitted device objective GP and C fitted constraint GPs with R running
trials, in one process, alternating: the fused path and the torch evaluation
forced through ``BaseAcquisitionFunc`` on the same object (the op chain every
qLogCEI call took before the session existed), at the two shapes the sampler
uses: B = 2048 without gradient for the pre-sample evaluation and B = 10 with
gradient for a local-search step. Prints the table of docs/PERF.md's qLogCEI
section.

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
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--dims", type=int, default=20)
    ap.add_argument("--constraints", type=int, default=4)
    ap.add_argument("--running", type=int, default=8)
    ap.add_argument("--qmc", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_qlogcei_timing: a GPU is required")

    n, d, n_con = args.n, args.dims, args.constraints
    rng = np.random.RandomState(n)
    X = rng.rand(n, d)
    t0 = time.perf_counter()
    gprs = []
    for centre in np.linspace(0.6, 0.4, 1 + n_con):  # the objective, then the constraints
        y = -np.sum((X - centre) ** 2, axis=1) + 0.02 * rng.randn(n)
        y = (y - y.mean()) / y.std()
        gprs.append(gp_mod.fit_kernel_params(
            X, y, np.zeros(d, dtype=bool), prior.default_log_prior, 1e-6, False
        ))
    print(f"<!-- N={n} D={d}: {1 + n_con} fits in {time.perf_counter() - t0:.1f} s on "
          f"{gprs[0].device} -->", flush=True)
    space = gp_ss.SearchSpace({f"x{i}": FloatDistribution(0.0, 1.0) for i in range(d)})
    acqf = acqf_mod.qLogCEI(
        gprs[0], space, 0.0, 0.3 * rng.rand(args.running, d), n_qmc_samples=args.qmc,
        qmc_seed=1, constraints_gpr_list=gprs[1:], constraints_threshold_list=[0.0] * n_con,
    )
    if acqf._fused_session() is None:
        raise SystemExit("gp_qlogcei_timing: the fused path is not eligible here")
    base = acqf_mod.BaseAcquisitionFunc
    pre, loc = 0.4 + 0.4 * rng.rand(2048, d), 0.4 + 0.4 * rng.rand(10, d)

    print("| N | C | R | Q | shape | fused ms (median, min..max) | torch ms (median, min..max) | "
          "torch / fused | max rel diff f |")
    print("|---|---|---|---|---|---|---|---|---|")
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
        print(f"| {n} | {n_con} | {args.running} | {args.qmc} | {shape} | "
              f"{mf:.2f} ({min(tf):.2f}..{max(tf):.2f}) | {mt:.2f} ({min(tt):.2f}..{max(tt):.2f}) | "
              f"{mt / mf:.1f} | {diff:.1e} |", flush=True)


if __name__ == "__main__":
    main()
