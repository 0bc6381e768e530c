"""Timing of the fused GP fit evaluation against the torch op chain.

One loss-and-gradient call of the hyperparameter fit on one regressor, in one
process, alternating: the ``GpFitSession`` route (build_cov, torch's
factorisation, grad) and ``_loss_and_grad_closed_form_torch``, from a device
synchronise to the returned host values, at N in {512, 1024, 2048, 5000}, D = 20,
all-continuous and with three categorical columns. The fused call is also
split into its two native calls and the factorisation between them.

``--fit`` instead times a cold fit and a warm refit through
``fit_kernel_params`` under both settings of OPTUNA_AMD_GP_FUSED_FIT and
counts their evaluations. ``--suggest`` runs GPSampler suggests on bench.py's
GP history (5000 observations, 20 dimensions, random values) on two studies,
one per setting, alternating step by step, and splits a step into the fit, the
acquisition optimisation and the rest, with the optimiser's evaluation counts.
Each mode prints one table of docs/PERF.md's GP fit section.

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

from optuna_amd import _hip  # noqa: E402
from optuna_amd._gp import gp as gp_mod  # noqa: E402

MIN_NOISE = 1e-6


def _timed_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()  # ends in a copy to the host, or in the synchronise of the split
    return 1e3 * (time.perf_counter() - t0)


def _stats(ts: list[float]) -> str:
    return f"{statistics.median(ts):.2f} ({min(ts):.2f}..{max(ts):.2f})"


def evaluation_table(rounds: int) -> None:
    core = _hip.require()
    print("| N | D | categorical | fused ms (median, min..max) | torch ms (median, min..max) | "
          "torch / fused | build_cov ms | factorisation ms | grad ms | max rel diff grad |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    d = 20
    for n in (512, 1024, 2048, 5000):
        for cat in ([], [3, 9, 19]):
            rng = np.random.RandomState(n + len(cat))
            X = rng.rand(n, d)
            X[:, cat] = rng.randint(0, 3, size=(n, len(cat)))
            y = np.sum((X - 0.3) ** 2, axis=1) + 0.05 * rng.randn(n)
            y = (y - y.mean()) / y.std()
            is_cat = np.zeros(d, dtype=bool)
            is_cat[cat] = True
            ones = torch.ones(d + 2, dtype=torch.float64)
            gpr = gp_mod.GPRegressor(
                torch.from_numpy(is_cat), torch.from_numpy(X), torch.from_numpy(y),
                ones[:d], ones[d], ones[d + 1],
            ).to(torch.device("cuda"))
            Xd, yd = gpr._X_train, gpr._y_train.squeeze(-1)
            raw = rng.uniform(-0.5, 0.5, d + 2)
            fused = gpr._fused_fit_evaluator(Xd, yd, MIN_NOISE, False)
            if fused is None:
                raise SystemExit("gp_fit_timing: the fused route is not eligible here")

            def forced():
                return gpr._loss_and_grad_closed_form_torch(raw, Xd, yd, MIN_NOISE, False)

            # The fused call in its three parts, each ended by a synchronise.
            session = core.GpFitSession(
                Xd.data_ptr(), yd.data_ptr(), n, d, cat_mask=sum(1 << c for c in cat)
            )
            C = torch.empty((n, n), dtype=torch.float64, device="cuda")
            parts: dict = {}

            def p_cov():
                session.build_cov(raw, MIN_NOISE, False, C.data_ptr())

            def p_fact():
                L = torch.linalg.cholesky(C)
                parts["L"] = L
                parts["a"] = torch.cholesky_solve(yd.unsqueeze(-1), L)[:, 0].contiguous()
                parts["I"] = torch.cholesky_inverse(L)
                torch.cuda.current_stream().synchronize()

            def p_grad():
                session.grad(raw, MIN_NOISE, False, parts["L"].data_ptr(),
                             parts["a"].data_ptr(), parts["I"].data_ptr())

            (_, ga), (_, gb) = fused(raw), forced()
            diff = np.max(np.abs(ga - gb) / np.maximum(np.abs(gb), 1e-300))
            for _ in range(3):
                fused(raw), forced(), p_cov(), p_fact(), p_grad()
            tf, tt, tc, tl, tg = [], [], [], [], []
            for _ in range(rounds):  # alternating: both see the same machine
                tf.append(_timed_ms(lambda: fused(raw)))
                tt.append(_timed_ms(forced))
                tc.append(_timed_ms(p_cov))
                tl.append(_timed_ms(p_fact))
                tg.append(_timed_ms(p_grad))
            med = statistics.median
            print(f"| {n} | {d} | {len(cat)} | {_stats(tf)} | {_stats(tt)} | "
                  f"{med(tt) / med(tf):.2f} | {med(tc):.2f} | {med(tl):.2f} | {med(tg):.2f} | "
                  f"{diff:.1e} |", flush=True)
            del gpr, fused, session, C, parts
            torch.cuda.empty_cache()


def _bench_history(n: int, d: int):
    rng = np.random.RandomState(0)
    return rng.uniform(-5.0, 5.0, size=(n, d)), rng.rand(n)


def fit_table() -> None:
    """A cold fit at 5000 rows, then a warm refit (16 iterations at most) at 5125."""
    from optuna_amd._gp import prior

    n, d = 5125, 20
    P, v = _bench_history(n, d)
    X = (P + 5.0) / 10.0
    is_cat = np.zeros(d, dtype=bool)
    evals = {"n": 0}
    cls = gp_mod.GPRegressor
    torch_eval, fused_factory = cls._loss_and_grad_closed_form_torch, cls._fused_fit_evaluator

    def counted_torch(self, *a, **k):
        evals["n"] += 1
        return torch_eval(self, *a, **k)

    def counted_fused(self, *a, **k):
        evaluate = fused_factory(self, *a, **k)
        if evaluate is None:
            return None

        def counted(raw):
            evals["n"] += 1
            return evaluate(raw)

        return counted

    cls._loss_and_grad_closed_form_torch, cls._fused_fit_evaluator = counted_torch, counted_fused

    def fit(rows, cache):
        y = v[:rows]
        evals["n"] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gpr = gp_mod.fit_kernel_params(
            X[:rows], (y - y.mean()) / y.std(), is_cat, prior.default_log_prior, MIN_NOISE,
            False, gpr_cache=cache,
        )
        torch.cuda.synchronize()
        return gpr, 1e3 * (time.perf_counter() - t0), evals["n"]

    print("| repetition | route | cold fit ms | evaluations | warm refit ms | evaluations | "
          "noise variance | kernel scale |")
    print("|---|---|---|---|---|---|---|---|")
    for rep in (1, 2):
        for switch in ("0", "1"):
            os.environ["OPTUNA_AMD_GP_FUSED_FIT"] = switch
            g0, t_cold, n_cold = fit(5000, None)
            g1, t_warm, n_warm = fit(n, g0)
            print(f"| {rep} | {'fused' if switch == '1' else 'torch chain'} | {t_cold:.0f} | "
                  f"{n_cold} | {t_warm:.0f} | {n_warm} | {g1.noise_var.item():.6g} | "
                  f"{g1.kernel_scale.item():.6g} |", flush=True)
            del g0, g1
            torch.cuda.empty_cache()


def suggest_table(steps: int, warmup: int) -> None:
    """Where a suggest at bench.py's GP configuration spends its time, per route."""
    import optuna_amd
    from optuna_amd._gp import acqf as acqf_mod
    from optuna_amd._gp import optim_mixed

    optuna_amd.logging.set_verbosity(optuna_amd.logging.ERROR)
    n, d = 5000, 20
    names = [f"x{i}" for i in range(d)]
    dists = {k: optuna_amd.distributions.FloatDistribution(-5.0, 5.0) for k in names}
    P, v = _bench_history(n, d)
    trials = [
        optuna_amd.create_trial(
            params=dict(zip(names, map(float, p))), distributions=dists, value=float(val)
        )
        for p, val in zip(P, v)
    ]
    studies = {}
    for switch in ("0", "1"):
        studies[switch] = optuna_amd.create_study(
            sampler=optuna_amd.samplers.GPSampler(seed=0, n_startup_trials=10)
        )
        studies[switch].add_trials(trials)

    now = {"fit": 0.0, "opt": 0.0, "grad": 0, "nograd": 0}

    def timed(module, name, key):
        inner = getattr(module, name)

        def wrapper(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = inner(*a, **k)
            torch.cuda.synchronize()
            now[key] += 1e3 * (time.perf_counter() - t0)
            return out

        setattr(module, name, wrapper)

    def counted(name, key):
        inner = getattr(acqf_mod._FusedEntryPoints, name)

        def wrapper(self, *a, **k):
            now[key] += 1
            return inner(self, *a, **k)

        setattr(acqf_mod._FusedEntryPoints, name, wrapper)

    timed(gp_mod, "fit_kernel_params", "fit")
    timed(optim_mixed, "optimize_acqf_mixed", "opt")
    counted("eval_acqf_batched_with_grad", "grad")
    counted("eval_acqf_no_grad", "nograd")

    rows = {"0": [], "1": []}
    for _ in range(warmup + steps):
        for switch in ("0", "1"):
            os.environ["OPTUNA_AMD_GP_FUSED_FIT"] = switch
            for key in now:
                now[key] = 0
            study = studies[switch]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t = study.ask()
            x = np.array([t.suggest_float(k, -5, 5) for k in names])
            study.tell(t, float(np.sum((x - 1) ** 2)))
            rows[switch].append((1e3 * (time.perf_counter() - t0), dict(now)))
    os.environ.pop("OPTUNA_AMD_GP_FUSED_FIT", None)

    print("| route | ms per step | fit | acquisition optimisation | rest | "
          "gradient calls per step | no-gradient calls per step | refits |")
    print("|---|---|---|---|---|---|---|---|")
    for switch, name in (("0", "torch chain"), ("1", "fused")):
        r = rows[switch][warmup:]

        def mean(f):
            return statistics.mean(f(total, parts) for total, parts in r)

        total, fit = mean(lambda t, p: t), mean(lambda t, p: p["fit"])
        opt = mean(lambda t, p: p["opt"])
        refits = sum(1 for _, p in r if p["fit"] > 100.0)
        print(f"| {name} | {total:.2f} | {fit:.2f} | {opt:.2f} | {total - fit - opt:.2f} | "
              f"{mean(lambda t, p: p['grad']):.1f} | {mean(lambda t, p: p['nograd']):.1f} | "
              f"{refits} |", flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--suggest", action="store_true")
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_fit_timing: a GPU is required")
    if args.fit:
        fit_table()
    elif args.suggest:
        suggest_table(args.steps, args.warmup)
    else:
        evaluation_table(args.rounds)


if __name__ == "__main__":
    main()
