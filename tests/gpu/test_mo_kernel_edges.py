"""Edge-shape differential tests for the multi-objective HIP kernels
(non-domination rank, 3-D hypervolume, greedy-HSSP contributions and session).

The extension is called directly, below the host dispatch thresholds, and
compared with references written here: an O(N²M) numpy peel, a slice-in-x
staircase sweep and an exact coordinate-compression grid.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from optuna_amd import _hip


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


# ---------------------------------------------------------------------------
# Non-domination rank
# ---------------------------------------------------------------------------


def _peel(vals: np.ndarray) -> np.ndarray:
    """Reference ranks: repeatedly strip the rows no remaining row dominates."""
    n = len(vals)
    with np.errstate(invalid="ignore"):
        leq = (vals[:, None, :] <= vals[None, :, :]).all(axis=2)  # [j, i]: j <= i everywhere
        lt = (vals[:, None, :] < vals[None, :, :]).any(axis=2)
    dom = leq & lt  # dom[j, i]: j dominates i
    ranks = np.full(n, -1, dtype=np.int64)
    left = np.ones(n, dtype=bool)
    r = 0
    while left.any():
        front = left & ~(dom & left[:, None]).any(axis=0)
        ranks[front] = r
        left &= ~front
        r += 1
    return ranks


def _rank_data(pattern: str, n: int, m: int) -> np.ndarray:
    r = np.random.RandomState(1000 * n + 10 * m + len(pattern))
    if pattern == "small-ints":
        return r.randint(0, 4, (n, m)).astype(np.float64)
    if pattern == "identical":
        return np.full((n, m), 2.5)
    if pattern == "chain":
        return np.tile(np.arange(n, dtype=np.float64)[r.permutation(n), None], (1, m))
    if pattern == "antichain":
        v = np.zeros((n, m))
        if m >= 2:
            i = r.permutation(n).astype(np.float64)
            v[:, 0], v[:, 1] = i, n - i
        return v
    if pattern == "inf-rows":
        v = r.randint(0, 4, (n, m)).astype(np.float64)
        v[r.rand(n, m) < 0.15] = np.inf
        v[r.rand(n, m) < 0.15] = -np.inf
        v[0] = np.inf
        v[n - 1] = -np.inf
        return v
    raise ValueError(pattern)


_PATTERNS = ["small-ints", "identical", "chain", "antichain", "inf-rows"]


@pytest.mark.parametrize("pattern", _PATTERNS)
@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 257])
def test_nondomination_rank_edges(core, n, m, pattern) -> None:
    vals = _rank_data(pattern, n, m)
    want = _peel(vals)
    if pattern == "chain":
        assert want.max() == n - 1
    if pattern in ("antichain", "identical"):
        assert want.max() == 0
    for n_below in sorted({0, 1, n // 2, n}):
        got = np.asarray(core.nondomination_rank(np.ascontiguousarray(vals), n_below))
        assert got.shape == (n,)
        ranked = got >= 0
        np.testing.assert_array_equal(got[~ranked], -1)
        np.testing.assert_array_equal(got[ranked], want[ranked])
        if n_below == 0:
            assert not ranked.any()
        assert ranked.sum() >= n_below
        # fronts are assigned whole
        np.testing.assert_array_equal(ranked, np.isin(want, np.unique(got[ranked])))
        if n_below == n:
            np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------
# 3-D hypervolume
# ---------------------------------------------------------------------------


def _hv_slices(pts: np.ndarray, ref: np.ndarray) -> float:
    """Slice along x; each slab's cross-section is a 2-D staircase area."""
    xs = np.unique(pts[:, 0])
    total = 0.0
    for i, x in enumerate(xs):
        width = (xs[i + 1] if i + 1 < len(xs) else ref[0]) - x
        sub = pts[pts[:, 0] <= x][:, 1:]
        sub = sub[np.lexsort((sub[:, 1], sub[:, 0]))]  # y ascending
        zmin = np.minimum.accumulate(sub[:, 1])
        y_next = np.append(sub[1:, 0], ref[1])
        total += width * float(np.sum((y_next - sub[:, 0]) * (ref[2] - zmin)))
    return total


def _hv_grid(pts: np.ndarray, ref: np.ndarray) -> float:
    """Exact union volume on the compressed coordinate grid."""
    axes = [np.unique(np.append(pts[:, d], ref[d])) for d in range(3)]
    lows = [a[:-1] for a in axes]
    widths = [np.diff(a) for a in axes]
    covered = np.zeros([len(a) for a in lows], dtype=bool)
    for p in pts:
        covered |= (
            (lows[0] >= p[0])[:, None, None]
            & (lows[1] >= p[1])[None, :, None]
            & (lows[2] >= p[2])[None, None, :]
        )
    vol = widths[0][:, None, None] * widths[1][None, :, None] * widths[2][None, None, :]
    return float(np.sum(vol[covered]))


def _sphere_front(n: int, seed: int) -> np.ndarray:
    """n mutually non-dominated, tie-free points (unit-sphere octant), lexsorted."""
    r = np.random.RandomState(seed)
    p = np.abs(r.randn(n, 3)) + 1e-3
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    p = np.unique(p, axis=0)
    assert len(p) == n
    return p


_REF = np.array([1.2, 1.3, 1.4])


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_hv3d_lds_tile_edges(core, n) -> None:
    pts = _sphere_front(n, 70 + n)
    want = _hv_slices(pts, _REF)
    if n <= 64:
        np.testing.assert_allclose(_hv_grid(pts, _REF), want, rtol=1e-12)
    got = core.hv3d(np.ascontiguousarray(pts), *map(float, _REF))
    print(f"hv3d n={n}: got {got!r} want {want!r}")
    np.testing.assert_allclose(got, want, rtol=1e-10)


def _tied_front(kind: str) -> np.ndarray:
    if kind == "lattice":  # i + j + k = 9: an antichain tied in every coordinate
        pts = [(i, j, 9 - i - j) for i in range(10) for j in range(10 - i)]
        return np.unique(np.array(pts, dtype=np.float64) / 10.0, axis=0)
    # one shared coordinate, the other two trading off
    t = np.arange(20, dtype=np.float64) / 20.0
    cols = {"tied-x": (0, 1, 2), "tied-y": (1, 0, 2), "tied-z": (2, 0, 1)}[kind]
    pts = np.empty((40, 3))
    pts[:20, cols[0]], pts[:20, cols[1]], pts[:20, cols[2]] = 0.25, t, 0.95 - t
    pts[20:, cols[0]], pts[20:, cols[1]], pts[20:, cols[2]] = 0.5, t - 0.03, 0.9 - t
    return np.unique(pts, axis=0)


@pytest.mark.parametrize("kind", ["lattice", "tied-x", "tied-y", "tied-z"])
def test_hv3d_tied_coordinates(core, kind) -> None:
    from optuna_amd.study._multi_objective import _is_pareto_front

    pts = _tied_front(kind)
    pts = pts[_is_pareto_front(pts, assume_unique_lexsorted=True)]
    assert len(pts) >= 20
    tied = {"lattice": (0, 1, 2), "tied-x": (0,), "tied-y": (1,), "tied-z": (2,)}[kind]
    for d in tied:
        assert len(np.unique(pts[:, d])) <= len(pts) // 2  # ties present in the tested set
    want = _hv_grid(pts, _REF)
    np.testing.assert_allclose(_hv_slices(pts, _REF), want, rtol=1e-12)
    got = core.hv3d(np.ascontiguousarray(pts), *map(float, _REF))
    np.testing.assert_allclose(got, want, rtol=1e-10)


# ---------------------------------------------------------------------------
# Greedy-HSSP contributions
# ---------------------------------------------------------------------------


def _views(sel: np.ndarray):
    """Pre-sorted views of the selected set, built by stable argsort."""
    k = len(sel)
    ox = np.argsort(sel[:, 0], kind="stable")
    oy = np.argsort(sel[:, 1], kind="stable")
    rank_x = np.empty(k, dtype=np.int32)
    rank_x[ox] = np.arange(k, dtype=np.int32)
    c = np.ascontiguousarray
    return (c(sel[ox, 0]), c(sel[ox, 2]), c(sel[oy, 1]), c(sel[oy, 2]), c(rank_x[oy]))


@functools.lru_cache(maxsize=None)
def _contrib_case(k: int) -> tuple[np.ndarray, np.ndarray]:
    r = np.random.RandomState(300 + k)
    # Selected points on a coarse lattice (ties among themselves) plus free ones.
    sel = np.round(r.uniform(0.1, 0.9, (k, 3)), 1)
    sel[k // 2:] = r.uniform(0.1, 0.9, (k - k // 2, 3))
    cand = r.uniform(0.05, 0.95, (20, 3))
    cand[0] = 0.01  # dominates every selected point
    if k:
        cand[1] = sel[0]  # equal to a selected point
        cand[2] = sel[k - 1] + [0.02, 0.03, 0.0]  # dominated by one selected point
        cand[3] = [sel[0, 0], 0.07, 0.9]  # shares x with a selected point
        cand[4] = [0.9, sel[k - 1, 1], 0.06]  # shares y
        cand[5] = [0.08, 0.85, sel[k // 2, 2]]  # shares z
        cand[6] = [sel[0, 0], sel[k - 1, 1], sel[k // 2, 2]]  # shares all three
    sel.setflags(write=False)
    cand.setflags(write=False)
    return sel, cand


@pytest.mark.parametrize("k", [0, 1, 2, 33, 129])
def test_hssp3d_contrib_edges(core, k) -> None:
    from optuna_amd._hypervolume import wfg

    sel, cand = _contrib_case(k)
    ref = np.array([1.0, 1.1, 1.2])
    if k <= 33:
        def hv(p):
            return _hv_grid(p, ref) if len(p) else 0.0
    else:
        assert k + 1 < wfg._DEVICE_HV3D_MIN_ROWS  # host path

        def hv(p):
            return wfg.compute_hypervolume(p, ref)

    base = hv(sel)
    want = np.array([hv(np.vstack([sel, c[None, :]])) - base for c in cand])
    if k:
        assert abs(want[1]) <= 1e-12 and abs(want[2]) <= 1e-12
    got = np.asarray(
        core.hssp3d_contrib(np.ascontiguousarray(cand), *_views(sel), *map(float, ref))
    )
    incl = np.prod(ref[None, :] - cand, axis=1)
    print("max |got - want| / incl:", np.max(np.abs(got - want) / incl))
    assert (np.abs(got - want) <= 1e-10 * incl).all(), (got, want)


# ---------------------------------------------------------------------------
# Greedy-HSSP session
# ---------------------------------------------------------------------------

_HSSP_REF = np.array([1.2, 1.2, 1.2])


@functools.lru_cache(maxsize=None)
def _host_greedy(subset_size: int) -> np.ndarray:
    """Host lazy-greedy order over the 100 tie-free candidates."""
    from optuna_amd._hypervolume import hssp

    cand = _sphere_front(100, 21)
    old = hssp._DEVICE_HSSP_MIN_WORK
    hssp._DEVICE_HSSP_MIN_WORK = 10**12
    try:
        out = hssp._solve_hssp(cand, np.arange(100), subset_size, _HSSP_REF)
    finally:
        hssp._DEVICE_HSSP_MIN_WORK = old
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("subset_size", [1, 2, 65, 99, 100, 150])
def test_hssp3d_session_matches_host_order(core, subset_size) -> None:
    cand = _sphere_front(100, 21)
    session = core.Hssp3dSession(np.ascontiguousarray(cand), *map(float, _HSSP_REF))
    got = np.asarray(session.run(subset_size))
    if subset_size < 100:
        want = _host_greedy(subset_size)
    else:
        # The host returns every index unordered once nothing is left to
        # choose; the greedy order of all 100 is the 99-prefix plus the one
        # remaining candidate. 150 clamps to n.
        first = _host_greedy(99)
        want = np.append(first, np.setdiff1d(np.arange(100), first))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("subset_size", [20, 65, 80])
def test_hssp3d_session_with_duplicates(core, subset_size) -> None:
    from optuna_amd._hypervolume import hssp, wfg

    cand = _sphere_front(100, 22).copy()
    cand[70:] = cand[np.random.RandomState(5).choice(70, 30, replace=False)]
    session = core.Hssp3dSession(np.ascontiguousarray(cand), *map(float, _HSSP_REF))
    got = np.asarray(session.run(subset_size))
    assert got.shape == (subset_size,)
    assert ((got >= 0) & (got < 100)).all()
    assert len(np.unique(got)) == subset_size
    old = hssp._DEVICE_HSSP_MIN_WORK
    hssp._DEVICE_HSSP_MIN_WORK = 10**12
    try:
        host = hssp._solve_hssp(cand, np.arange(100), subset_size, _HSSP_REF)
    finally:
        hssp._DEVICE_HSSP_MIN_WORK = old
    np.testing.assert_allclose(
        wfg.compute_hypervolume(cand[got], _HSSP_REF),
        wfg.compute_hypervolume(cand[host], _HSSP_REF),
        rtol=1e-9,
    )
