"""Host references for the hypervolume kernels, shared by the CPU and GPU tests.

``hv_grid`` shares nothing with the production code: it marks the dominated
cells of the compressed coordinate grid and adds their volumes, for any number
of objectives. ``hv4d_nested_sweep`` is the numpy transcription of the 4-D
kernel's dataflow (``k_hv4d``): agreement between the two, and with the host
WFG, is evidence that the nested-sweep formula is right before any device code
runs. ``hssp_views4`` builds the six pre-sorted views of a selected set that
``hssp4d_contrib`` takes.
"""
from __future__ import annotations

import numpy as np


def hv_grid(pts: np.ndarray, ref: np.ndarray) -> float:
    """Exact union volume on the compressed coordinate grid (minimisation).

    Memory is the product of the per-axis unique-coordinate counts, so this is
    for small inputs only.
    """
    pts = np.asarray(pts, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if pts.shape[0] == 0:
        return 0.0
    m = pts.shape[1]
    axes = [np.unique(np.append(pts[:, d], ref[d])) for d in range(m)]
    lows = [a[:-1] for a in axes]
    widths = [np.diff(a) for a in axes]

    def along(v: np.ndarray, d: int) -> np.ndarray:
        shape = [1] * m
        shape[d] = len(v)
        return v.reshape(shape)

    covered = np.zeros([len(a) for a in lows], dtype=bool)
    for p in pts:
        box = along(lows[0] >= p[0], 0)
        for d in range(1, m):
            box = box & along(lows[d] >= p[d], d)
        covered |= box
    vol = along(widths[0], 0)
    for d in range(1, m):
        vol = vol * along(widths[d], d)
    return float(np.sum(np.broadcast_to(vol, covered.shape)[covered]))


def hv4d_nested_sweep(pts: np.ndarray, ref: np.ndarray) -> float:
    """``sum_t sum_u slab_w(t) * slab_x(u) * A(t, u)`` over stable w- and x-ranks.

    ``A(t, u)`` is the (y, z) staircase area of the points with w-rank <= t and
    x-rank <= u, swept in y-ascending order with a running min of z. Zero-width
    slabs (tied coordinates) are skipped.
    """
    pts = np.asarray(pts, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    n = len(pts)
    if n == 0:
        return 0.0
    assert pts.shape[1] == 4
    ow = np.argsort(pts[:, 0], kind="stable")
    ox = np.argsort(pts[:, 1], kind="stable")
    oy = np.argsort(pts[:, 2], kind="stable")
    rank_w = np.empty(n, dtype=np.int64)
    rank_x = np.empty(n, dtype=np.int64)
    rank_w[ow] = np.arange(n)
    rank_x[ox] = np.arange(n)
    slab_w = np.diff(np.append(pts[ow, 0], ref[0]))
    slab_x = np.diff(np.append(pts[ox, 1], ref[1]))
    dy = np.diff(np.append(pts[oy, 2], ref[2]))
    z = pts[oy, 3]
    rw, rx = rank_w[oy], rank_x[oy]
    u = np.arange(n)
    total = 0.0
    for t in range(n):
        if slab_w[t] <= 0.0:
            continue
        passes = (rw <= t)[None, :] & (rx[None, :] <= u[:, None])  # (u, q)
        minz = np.minimum.accumulate(np.where(passes, z[None, :], ref[3]), axis=1)
        area = np.sum(dy[None, :] * (ref[3] - minz), axis=1)
        live = slab_x > 0.0
        total += slab_w[t] * float(np.sum(slab_x[live] * area[live]))
    return total


def hssp_views4(
    sel: np.ndarray,
) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``(sw, sx, sy, syz, syrw, syrx)`` of a (k, 4) selected set, by stable argsort:
    w ascending, x ascending, and the y-ascending stream (y, z, w-rank, x-rank)."""
    sel = np.asarray(sel, dtype=np.float64).reshape(-1, 4)
    k = len(sel)
    ow = np.argsort(sel[:, 0], kind="stable")
    ox = np.argsort(sel[:, 1], kind="stable")
    oy = np.argsort(sel[:, 2], kind="stable")
    rank_w = np.empty(k, dtype=np.int32)
    rank_x = np.empty(k, dtype=np.int32)
    rank_w[ow] = np.arange(k, dtype=np.int32)
    rank_x[ox] = np.arange(k, dtype=np.int32)
    c = np.ascontiguousarray
    return (
        c(sel[ow, 0]),
        c(sel[ox, 1]),
        c(sel[oy, 2]),
        c(sel[oy, 3]),
        c(rank_w[oy]),
        c(rank_x[oy]),
    )


# ---------------------------------------------------------------------------
# Shared edge-case inputs
# ---------------------------------------------------------------------------


def sphere_front(n: int, m: int, seed: int) -> np.ndarray:
    """n mutually non-dominated, tie-free points on the unit-sphere orthant, lexsorted."""
    r = np.random.RandomState(seed)
    p = np.abs(r.randn(n, m)) + 1e-3
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    p = np.unique(p, axis=0)
    assert len(p) == n
    return p


def lattice_points(n: int, m: int, seed: int) -> np.ndarray:
    """n points on the 0.1-lattice: ties in every axis, dominated and duplicate rows."""
    r = np.random.RandomState(seed)
    p = np.round(r.uniform(0.1, 0.9, (n, m)), 1)
    if n >= 6:
        p[n - n // 6 :] = p[: n // 6]  # guaranteed duplicates
    return p


def tied_front4(axis: int) -> np.ndarray:
    """40 4-D points in two groups of 20 that each share one value on ``axis``;
    within a group two of the other axes trade off and the third is scattered."""
    i = np.arange(20)
    t = i / 20.0
    others = [d for d in range(4) if d != axis]
    pts = np.empty((40, 4))
    pts[:20, axis] = 0.25
    pts[:20, others[0]] = t
    pts[:20, others[1]] = 0.95 - t
    pts[:20, others[2]] = 0.1 + 0.8 * ((7 * i) % 20) / 20.0
    pts[20:, axis] = 0.5
    pts[20:, others[0]] = t - 0.03
    pts[20:, others[1]] = 0.9 - t
    pts[20:, others[2]] = 0.1 + 0.8 * ((3 * i + 5) % 20) / 20.0
    return np.unique(pts, axis=0)
