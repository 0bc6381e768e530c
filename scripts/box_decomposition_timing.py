"""Timing of the device box decomposition against the host one.

Both routes of ``get_non_dominated_boxes_batched`` on the same inputs in one
process, the size gate forced each way: tie-free sphere fronts of 2, 3 and 4
objectives over a size sweep, Q = 1 and Q = 128 draws of R = 8 rows each near
the front. Prints the tables of docs/PERF.md's "Box decomposition on the
device": median wall clock (the device route ends in copies to the host),
whether the two routes gave the same set of boxes for every draw, and the LDS
the device reports with the active-list capacity that follows from it.

The host column of a Q = 128 row is one draw's median times 128 where the
draws would take more than ``--host-budget`` seconds; such rows are marked.

A GPU is required; nothing here falls back.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402

from optuna_amd import _hip  # noqa: E402
from optuna_amd._hypervolume import box_decomposition as bd  # noqa: E402
from optuna_amd.testing.hv_reference import sphere_front  # noqa: E402

OFF = 10**9
SIZES = {2: (16, 64, 256, 1024, 4096), 3: (4, 8, 16, 32, 64, 256, 1000), 4: (4, 8, 16, 50, 100, 200)}


def _route(gate: int, base, extra, ref):
    bd._DEVICE_BOXES_MIN_ROWS = {m: gate for m in (2, 3, 4)}
    return bd.get_non_dominated_boxes_batched(base, extra, ref)


def _median_ms(fn, reps: int) -> float:
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def _same_sets(a, b) -> bool:
    if not np.array_equal(a[2], b[2]):
        return False
    for lo, hi in zip(a[2][:-1], a[2][1:]):
        rows = [np.concatenate([r[0][lo:hi], r[1][lo:hi]], axis=1) for r in (a, b)]
        if not np.array_equal(*(r[np.lexsort(r.T[::-1])] for r in rows)):
            return False
    return True


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-budget", type=float, default=6.0)
    args = ap.parse_args()
    core = _hip.require()
    if core is None or not core.available():
        raise SystemExit("box_decomposition_timing: a GPU is required")
    default_gate = dict(bd._DEVICE_BOXES_MIN_ROWS)
    for m in (2, 3, 4):
        lds, cap = core.box_decompose_limits(m)
        print(f"<!-- M={m}: the device reports {lds} bytes of LDS per workgroup, "
              f"active list of {cap} entries; gate {default_gate[m]} -->")
    print("| M | n0 | R | Q | boxes per draw | host ms | device ms | host / device | same sets |")
    print("|---|---|---|---|---|---|---|---|---|")
    for m, sizes in SIZES.items():
        ref = np.full(m, 1.1)
        for n0 in sizes:
            base = sphere_front(n0, m, n0)
            rng = np.random.RandomState(n0 + m)
            for q in (1, 128):
                extra = sphere_front(8 * q, m, 7).reshape(q, 8, m) * rng.uniform(0.9, 1.1, (q, 8, 1))
                _route(0, base, extra, ref)  # warm-up: code objects, workspace
                dev = _route(0, base, extra, ref)
                t_dev = _median_ms(lambda: _route(0, base, extra, ref), args.reps)
                t_one = _median_ms(lambda: _route(OFF, base, extra[:1], ref), 1)
                if q == 1 or t_one * q <= 1e3 * args.host_budget:
                    host = _route(OFF, base, extra, ref)
                    t_host = _median_ms(lambda: _route(OFF, base, extra, ref), 1 if q > 1 else 3)
                    same, mark = _same_sets(dev, host), ""
                else:  # one draw checked, the host time scaled
                    same = _same_sets(_route(0, base, extra[:1], ref), _route(OFF, base, extra[:1], ref))
                    t_host, mark = t_one * q, " (one draw x Q)"
                print(f"| {m} | {n0} | 8 | {q} | {int(np.median(np.diff(dev[2])))} | "
                      f"{t_host:.2f}{mark} | {t_dev:.2f} | {t_host / t_dev:.1f} | {same} |",
                      flush=True)
    bd._DEVICE_BOXES_MIN_ROWS = default_gate


if __name__ == "__main__":
    main()
