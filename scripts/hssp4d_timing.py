"""Host-against-device timing of the 4-objective hypervolume and greedy HSSP.

Prints one table per measurement of docs/PERF.md's 4-objective section: the
hypervolume and HSSP gate sweeps (host and device in the same process, on the
same tie-free sphere fronts, ref = 1.2), the device-only HSSP sizes, and the
suggests per second of a 4-objective MO-TPE study. A GPU is required; nothing
here falls back. ``--quick`` drops the sizes whose host side takes tens of
seconds.
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

import optuna_amd  # noqa: E402
from optuna_amd import _hip  # noqa: E402
from optuna_amd._hypervolume import hssp, wfg  # noqa: E402
from optuna_amd.testing.hv_reference import sphere_front  # noqa: E402


REF = np.full(4, 1.2)
OFF = 10**12


def _median_ms(fn, repeats: int) -> float:
    fn()  # warm-up: code-object load, workspace growth
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()  # every timed call ends in a device synchronise (or is host-only)
        times.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(times)


def _host_ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def hv_table(sizes: list[int]) -> None:
    print("\n## hypervolume, 4-D: host WFG against k_hv4d (through compute_hypervolume)")
    print("| n | host ms | device ms | host/device | rel diff |")
    print("|---|---|---|---|---|")
    for n in sizes:
        pts = sphere_front(n, 4, 100 + n)
        wfg._DEVICE_HV4D_MIN_ROWS = OFF
        host_val = wfg.compute_hypervolume(pts, REF)
        host = _host_ms(lambda: wfg.compute_hypervolume(pts, REF))
        if host < 200:
            host = _median_ms(lambda: wfg.compute_hypervolume(pts, REF), 5)
        wfg._DEVICE_HV4D_MIN_ROWS = 0
        dev_val = wfg.compute_hypervolume(pts, REF)
        dev = _median_ms(lambda: wfg.compute_hypervolume(pts, REF), 20)
        print(f"| {n} | {host:.3f} | {dev:.3f} | {host / dev:.1f} | "
              f"{abs(dev_val - host_val) / host_val:.1e} |", flush=True)


def hssp_table(cases: list[tuple[int, int]], with_host: bool) -> None:
    title = "host lazy greedy against Hssp4dSession" if with_host else "Hssp4dSession only"
    print(f"\n## HSSP, 4-D: {title} (through _solve_hssp)")
    print("| n | k | n*k | host ms | device ms | host/device | same picks |")
    print("|---|---|---|---|---|---|---|")
    for n, k in cases:
        cand = sphere_front(n, 4, 200 + n)
        idx = np.arange(n)
        hssp._DEVICE_HSSP4D_MIN_WORK = 0
        dev_pick = hssp._solve_hssp(cand, idx, k, REF)
        dev = _median_ms(lambda: hssp._solve_hssp(cand, idx, k, REF), 5 if n * k > 20000 else 20)
        host_s, ratio, same = "-", "-", "-"
        if with_host:
            # the reference host path: both device gates off
            hssp._DEVICE_HSSP4D_MIN_WORK = OFF
            wfg._DEVICE_HV4D_MIN_ROWS = OFF
            t0 = time.perf_counter()
            host_pick = hssp._solve_hssp(cand, idx, k, REF)
            host = 1e3 * (time.perf_counter() - t0)
            host_s, ratio = f"{host:.1f}", f"{host / dev:.1f}"
            same = str(bool((host_pick == dev_pick).all()))
        print(f"| {n} | {k} | {n * k} | {host_s} | {dev:.2f} | {ratio} | {same} |", flush=True)


def study_table(histories: list[int], steps: int) -> None:
    print("\n## 4-objective MO-TPE study (10 float params, sphere-front history)")
    print("| history | ms / suggest+tell (median) | suggests / s | Hssp4dSession runs |")
    print("|---|---|---|---|")
    for n_hist in histories:
        optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
        names = [f"x{i}" for i in range(10)]
        dists = {n: optuna_amd.distributions.FloatDistribution(0.0, 1.0) for n in names}
        study = optuna_amd.create_study(
            directions=["minimize"] * 4,
            sampler=optuna_amd.samplers.TPESampler(seed=0, n_startup_trials=10),
        )
        r = np.random.RandomState(n_hist)
        vals = np.abs(r.randn(n_hist, 4)) + 1e-3
        vals /= np.linalg.norm(vals, axis=1, keepdims=True)
        # half of the history sits behind the front, as in a real study
        vals[::2] *= r.uniform(1.0, 1.5, (len(vals[::2]), 1))
        params = r.uniform(0, 1, (n_hist, 10))
        study.add_trials(
            [
                optuna_amd.create_trial(
                    params={n: float(params[j, i]) for i, n in enumerate(names)},
                    distributions=dists,
                    values=[float(v) for v in vals[j]],
                )
                for j in range(n_hist)
            ]
        )
        def step() -> None:
            t = study.ask()
            for n in names:
                t.suggest_float(n, 0.0, 1.0)
            v = np.abs(r.randn(4)) + 1e-3
            study.tell(t, list(v / np.linalg.norm(v)))

        step()
        before = _session_runs()
        times = []
        for _ in range(steps):
            t0 = time.perf_counter()
            step()
            times.append(time.perf_counter() - t0)
        med = statistics.median(times)
        print(f"| {n_hist} | {1e3 * med:.1f} | {1.0 / med:.1f} | {_session_runs() - before} |",
              flush=True)


_RUNS = 0


def _session_runs() -> int:
    return _RUNS


def _count_session_runs() -> None:
    """Count device HSSP runs by wrapping the dispatch function."""
    global _RUNS
    inner = hssp._solve_hssp_4d_device

    def counted(*args):
        global _RUNS
        out = inner(*args)
        if out is not None:
            _RUNS += 1
        return out

    hssp._solve_hssp_4d_device = counted


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    core = _hip.require()
    if core is None or not core.available():
        raise SystemExit("hssp4d_timing: a GPU and the built extension are required")
    default_gates = (wfg._DEVICE_HV4D_MIN_ROWS, hssp._DEVICE_HSSP4D_MIN_WORK)
    print(f"shipped gates: hv rows >= {default_gates[0]}, hssp n*k >= {default_gates[1]}")

    hv_table([4, 6, 8, 12, 16, 24, 32, 64] + ([] if args.quick else [400]))
    hssp_table(
        [(8, 2), (10, 3), (12, 4), (16, 4), (16, 8), (24, 8), (32, 8), (40, 20)]
        + ([] if args.quick else [(70, 33), (120, 60)]),
        with_host=True,
    )
    hssp_table([(350, 100), (350, 200), (1000, 300)], with_host=False)

    wfg._DEVICE_HV4D_MIN_ROWS, hssp._DEVICE_HSSP4D_MIN_WORK = default_gates
    _count_session_runs()
    study_table([1000, 2000], steps=10)


if __name__ == "__main__":
    main()
