"""Timing of the fused LogEHVI session against the torch path.

Default mode prints the per-call table of docs/PERF.md's LogEHVI section: on
the same fitted device GPs, in one process, the fused session and the torch
evaluation forced on the same ``LogEHVI`` object, at the two shapes the sampler
uses (B = 2048 without gradient for the pre-sample evaluation, B = 10 with
gradient for a local-search step), with the box count and the torch path's
peak device memory.

``--study`` prints the time per suggest of a 3-objective ``GPSampler`` study.
It imports ``optuna_amd`` from the current directory and uses nothing this
change added, so it also runs from an export of an older commit; that is how
two builds are compared (alternate the two trees in one job).

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
from optuna_amd._gp import acqf as acqf_mod  # noqa: E402
from optuna_amd._gp import gp as gp_mod  # noqa: E402
from optuna_amd._gp import prior  # noqa: E402
from optuna_amd._gp import search_space as gp_ss  # noqa: E402
from optuna_amd.distributions import FloatDistribution  # noqa: E402


D = 20


def _centres(n_obj: int) -> np.ndarray:
    return np.stack(
        [np.random.RandomState(100 + m).choice([0.2, 0.8], D) for m in range(n_obj)]
    )


def _history(n: int, rng: np.random.RandomState) -> np.ndarray:
    """A study that has partly converged: half of the points uniform in
    [0, 1]^D, half near the Pareto set (the hull of the three centres)."""
    near = rng.dirichlet(np.ones(3), n // 2) @ _centres(3) + 0.03 * rng.randn(n // 2, D)
    return np.concatenate([rng.rand(n - n // 2, D), np.clip(near, 0.0, 1.0)])


def _objectives(X: np.ndarray, n_obj: int, rng: np.random.RandomState) -> np.ndarray:
    """n_obj conflicting smooth losses of X in [0, 1]^D (squared distance to
    n_obj fixed points of {0.2, 0.8}^D) plus a little noise."""
    cols = []
    for centre in _centres(n_obj):
        cols.append(np.sum((X - centre) ** 2, axis=1))
    Y = np.stack(cols, axis=1)
    return Y + 0.02 * rng.randn(*Y.shape)


def _median_ms(fn, warmup: int, repeats: int) -> float:
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()  # both paths end in a copy to the host
        times.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(times)


def per_call_table(sizes: list[int], n_objs: list[int]) -> None:
    base = acqf_mod.BaseAcquisitionFunc
    print("| N | M | boxes J | shape | fused ms | torch ms | torch / fused | "
          "torch peak MiB | max rel diff f |")
    print("|---|---|---|---|---|---|---|---|---|")
    for n in sizes:
        rng = np.random.RandomState(n)
        X = _history(n, rng)
        losses = _objectives(X, max(n_objs), rng)
        scores = -(losses - losses.mean(0)) / losses.std(0)  # maximised, standardised
        t0 = time.perf_counter()
        gprs = [
            gp_mod.fit_kernel_params(
                X, scores[:, m], np.zeros(D, dtype=bool), prior.default_log_prior, 1e-6, False
            )
            for m in range(max(n_objs))
        ]
        print(f"<!-- N={n}: {max(n_objs)} fits in {time.perf_counter() - t0:.1f} s -->",
              flush=True)
        space = gp_ss.SearchSpace({f"x{i}": FloatDistribution(0.0, 1.0) for i in range(D)})
        for M in n_objs:
            acqf = acqf_mod.LogEHVI(
                gpr_list=gprs[:M], search_space=space,
                Y_train=torch.from_numpy(scores[:, :M].copy()), n_qmc_samples=128, qmc_seed=1,
            )
            if acqf._fused_session() is None:
                raise SystemExit("gp_ehvi_timing: the fused session is not eligible here")
            J = int(acqf._box_lower.shape[0])
            pre = rng.rand(2048, D)
            loc = rng.rand(10, D)
            for shape, fused, forced, reps in (
                ("B=2048 no grad", lambda: acqf.eval_acqf_no_grad(pre),
                 lambda: base.eval_acqf_no_grad(acqf, pre), 5),
                ("B=10 with grad", lambda: acqf.eval_acqf_batched_with_grad(loc),
                 lambda: base.eval_acqf_batched_with_grad(acqf, loc), 20),
            ):
                f_fused = fused()
                fused_ms = _median_ms(fused, 2, 2 * reps)
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                try:
                    f_torch = forced()
                    torch_ms = _median_ms(forced, 1, reps)
                    peak = torch.cuda.max_memory_allocated() / 2**20
                    a = f_fused[0] if isinstance(f_fused, tuple) else f_fused
                    b = f_torch[0] if isinstance(f_torch, tuple) else f_torch
                    diff = f"{np.max(np.abs(a - b) / np.abs(b)):.1e}"
                    row = f"{torch_ms:.2f} | {torch_ms / fused_ms:.1f} | {peak:.0f} | {diff}"
                except torch.cuda.OutOfMemoryError:
                    row = "out of memory | - | - | -"
                print(f"| {n} | {M} | {J} | {shape} | {fused_ms:.2f} | {row} |", flush=True)
                torch.cuda.empty_cache()


def study_line(history: int, steps: int) -> None:
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    names = [f"x{i}" for i in range(D)]
    dists = {n: FloatDistribution(0.0, 1.0) for n in names}
    study = optuna_amd.create_study(
        directions=["minimize"] * 3,
        sampler=optuna_amd.samplers.GPSampler(seed=0, n_startup_trials=10),
    )
    rng = np.random.RandomState(history)
    X = _history(history, rng)
    Y = _objectives(X, 3, rng)
    study.add_trials(
        [
            optuna_amd.create_trial(
                params={n: float(X[r, i]) for i, n in enumerate(names)},
                distributions=dists,
                values=[float(v) for v in Y[r]],
            )
            for r in range(history)
        ]
    )

    def step() -> None:
        t = study.ask()
        x = np.array([[t.suggest_float(n, 0.0, 1.0) for n in names]])
        study.tell(t, [float(v) for v in _objectives(x, 3, rng)[0]])

    t0 = time.perf_counter()
    step()  # cold fits, code-object loads
    first = time.perf_counter() - t0
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t0)
    fused = os.environ.get("OPTUNA_AMD_GP_FUSED_EHVI", "1") != "0" and hasattr(
        acqf_mod.LogEHVI, "_fused_session"
    )
    print(f"study history={history} objectives=3 dims={D} fused_ehvi={fused} "
          f"first_ms={1e3 * first:.0f} median_ms={1e3 * statistics.median(times):.1f} "
          f"min_ms={1e3 * min(times):.1f} steps={steps}", flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--study", action="store_true")
    ap.add_argument("--history", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 5000])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_ehvi_timing: a GPU is required")
    if args.study:
        study_line(args.history, args.steps)
    else:
        per_call_table(args.sizes, [2, 3])


if __name__ == "__main__":
    main()
