"""Timing of the fused qLogEHVI session against the torch path.

On M fitted device GPs with R running trials, in one process, alternating:
the fused path and the torch evaluation forced through ``BaseAcquisitionFunc``
on the same object (the op chain every qLogEHVI call took before the session
existed), at the two shapes the sampler uses: B = 2048 without gradient for
the pre-sample evaluation and B = 10 with gradient for a local-search step.
Prints the table of docs/PERF.md's qLogEHVI section and the box counts of the
problem.

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
    ap.add_argument("--objectives", type=int, default=3)
    ap.add_argument("--running", type=int, default=8)
    ap.add_argument("--qmc", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--few-boxes", action="store_true",
                    help="uniform history, optima on a line: a dozen boxes per draw")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_qlogehvi_timing: a GPU is required")

    n, d, n_obj = args.n, args.dims, args.objectives
    rng = np.random.RandomState(n)
    # The history of scripts/gp_ehvi_timing.py: conflicting quadratic losses with
    # optima at corners of {0.2, 0.8}^D, half of the points uniform and half near
    # the Pareto set (the hull of the optima), which is what gives a study its
    # hundreds to thousands of boxes. The running trials lie near that set too.
    centres = np.stack(
        [np.random.RandomState(100 + m).choice([0.2, 0.8], d) for m in range(n_obj)]
    )

    def near_front(k: int) -> np.ndarray:
        pts = rng.dirichlet(np.ones(n_obj), k) @ centres + 0.03 * rng.randn(k, d)
        return np.clip(pts, 0.0, 1.0)

    if args.few_boxes:
        centres = np.linspace(0.3, 0.7, n_obj)[:, None] * np.ones(d)

        def near_front(k: int) -> np.ndarray:  # noqa: F811
            return 0.3 + 0.4 * rng.rand(k, d)

    if args.few_boxes:
        X = rng.rand(n, d)
    else:
        X = np.concatenate([rng.rand(n - n // 2, d), near_front(n // 2)])
    Y = -np.stack([np.sum((X - c) ** 2, axis=1) for c in centres], axis=-1)
    Y = Y + 0.02 * rng.randn(*Y.shape)
    Y = (Y - Y.mean(axis=0)) / Y.std(axis=0)
    t0 = time.perf_counter()
    gprs = [
        gp_mod.fit_kernel_params(
            X, Y[:, m], np.zeros(d, dtype=bool), prior.default_log_prior, 1e-6, False
        )
        for m in range(n_obj)
    ]
    print(f"<!-- N={n} D={d} M={n_obj}: fits in {time.perf_counter() - t0:.1f} s on "
          f"{gprs[0].device} -->", flush=True)
    space = gp_ss.SearchSpace({f"x{i}": FloatDistribution(0.0, 1.0) for i in range(d)})
    running = near_front(args.running)
    t0 = time.perf_counter()
    acqf = acqf_mod.qLogEHVI(
        gprs, space, torch.from_numpy(Y), running,
        n_qmc_samples=args.qmc, qmc_seed=1,
    )
    counts = acqf._box_counts
    print(f"<!-- boxes per draw: min {min(counts)}, median {int(np.median(counts))}, "
          f"max {max(counts)}, {sum(counts)} in all; built in "
          f"{time.perf_counter() - t0:.1f} s -->", flush=True)
    if acqf._fused_session() is None:
        raise SystemExit("gp_qlogehvi_timing: the fused path is not eligible here")
    base = acqf_mod.BaseAcquisitionFunc
    pre = near_front(2048) if args.few_boxes else rng.rand(2048, d)
    loc = near_front(10)

    print("| N | M | R | Q | shape | fused ms (median, min..max) | "
          "torch ms (median, min..max) | torch / fused | max rel diff f |")
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
        print(f"| {n} | {n_obj} | {args.running} | {args.qmc} | {shape} | "
              f"{mf:.2f} ({min(tf):.2f}..{max(tf):.2f}) | "
              f"{mt:.2f} ({min(tt):.2f}..{max(tt):.2f}) | "
              f"{mt / mf:.1f} | {diff:.1e} |", flush=True)

    _order_check(acqf, gprs, X, Y, running, args.qmc, {"B=2048": pre, "B=10": loc})


def _order_check(acqf, gprs, X, Y, running, n_qmc, batches) -> None:
    """How far the torch chain is from itself with the observations in another
    order (same hyperparameters, draws and boxes), next to fused against torch:
    the draws s differ in their last bits, and the acquisition subtracts box
    corners from them, which near the front are observed values."""
    perm = np.random.RandomState(1).permutation(len(X))
    conds = []
    for m, g in enumerate(gprs):
        other = gp_mod.GPRegressor(
            g._is_categorical.cpu(), torch.from_numpy(X[perm]), torch.from_numpy(Y[perm, m]),
            g.inverse_squared_lengthscales.cpu().clone(), g.kernel_scale.cpu().clone(),
            g.noise_var.cpu().clone(),
        )
        other.to(g.device)
        other._cache_matrix()
        conds.append(acqf_mod._fantasize(other, running, n_qmc, 1 + m, 1e-12))
    print("\n| shape | max abs diff s, torch vs permuted torch | max rel diff f, torch vs "
          "permuted torch | max rel diff f, fused vs torch |")
    print("|---|---|---|---|")
    for shape, x in batches.items():
        with torch.no_grad():
            xt = acqf._up(x)
            s0, s1 = (
                torch.stack([c.sample_joint_posterior(xt, return_fantasy=False) for c in cs], -1)
                for cs in (acqf._cond_gpr_list, conds)
            )
            f0, f1 = (
                (torch.special.logsumexp(acqf_mod._per_sample_log_hvi(
                    s, acqf._box_lower, acqf._box_intervals), dim=-1) - np.log(n_qmc)).cpu().numpy()
                for s in (s0, s1)
            )
        fused = acqf.eval_acqf_no_grad(x)
        rel = lambda a, b: np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))  # noqa: E731
        print(f"| {shape} | {float((s0 - s1).abs().max()):.1e} | {rel(f1, f0):.1e} | "
              f"{rel(fused, f0):.1e} |", flush=True)


if __name__ == "__main__":
    main()
