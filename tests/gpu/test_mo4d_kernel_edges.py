"""Edge-shape differential tests for the 4-objective HIP kernels (k_hv4d,
k_hssp4d_contrib, k_hssp4d_insert and the Hssp4dSession launch train).

The extension is called directly. References are the exact grid
(``hv_grid``), a recursive slice-by-slice sweep written here, the host WFG and
the host lazy greedy, all with the device gates patched off.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np
import pytest

import optuna_amd
from optuna_amd import _hip
from optuna_amd._hypervolume import hssp, wfg
from optuna_amd.testing.hv_reference import (
    hssp_views4,
    hv_grid,
    lattice_points,
    sphere_front,
    tied_front4,
)


pytestmark = pytest.mark.gpu

_REF = np.array([1.2, 1.3, 1.4, 1.25])
_HSSP_REF = np.full(4, 1.2)
_OFF = 10**12


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


@contextlib.contextmanager
def _host_only():
    """Both 4-D device gates off: the host WFG / lazy greedy as reference."""
    old = (wfg._DEVICE_HV4D_MIN_ROWS, hssp._DEVICE_HSSP4D_MIN_WORK)
    wfg._DEVICE_HV4D_MIN_ROWS, hssp._DEVICE_HSSP4D_MIN_WORK = _OFF, _OFF
    try:
        yield
    finally:
        wfg._DEVICE_HV4D_MIN_ROWS, hssp._DEVICE_HSSP4D_MIN_WORK = old


def _c(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------
# hv4d
# ---------------------------------------------------------------------------


def _hv_slices(pts: np.ndarray, ref: np.ndarray) -> float:
    """Slice along the first axis; each slab's cross-section is the same
    problem one dimension down, ending in a 2-D staircase area."""
    if pts.shape[1] == 2:
        sub = pts[np.lexsort((pts[:, 1], pts[:, 0]))]
        zmin = np.minimum.accumulate(sub[:, 1])
        nxt = np.append(sub[1:, 0], ref[0])
        return float(np.sum((nxt - sub[:, 0]) * (ref[1] - zmin)))
    vs = np.unique(pts[:, 0])
    total = 0.0
    for i, v in enumerate(vs):
        width = (vs[i + 1] if i + 1 < len(vs) else ref[0]) - v
        total += width * _hv_slices(pts[pts[:, 0] <= v][:, 1:], ref[1:])
    return total


def _hv_rtol(n: int) -> float:
    # 1e-10 is the 3-D suite's bound; the second term is the worst-case
    # rounding of a sum of n^3 non-negative terms (3.8e-9 at n = 257).
    return max(1e-10, 2.0 * n**3 * 2.0**-53)


# The pair tile is 16 x 16 and the y-stream tile 256 entries.
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 255, 256, 257])
def test_hv4d_tile_edges(core, n) -> None:
    pts = sphere_front(n, 4, 70 + n)
    if n <= 17:
        want = hv_grid(pts, _REF)
        np.testing.assert_allclose(_hv_slices(pts, _REF), want, rtol=1e-12)
    else:
        want = _hv_slices(pts, _REF)
    got = core.hv4d(_c(pts), *map(float, _REF))
    print(f"hv4d n={n}: got {got!r} want {want!r} rel err {abs(got - want) / want:.3e}")
    np.testing.assert_allclose(got, want, rtol=_hv_rtol(n))
    # row order must not matter (host prep sorts), and runs are bit-identical
    shuffled = pts[np.random.RandomState(n).permutation(n)]
    assert core.hv4d(_c(shuffled), *map(float, _REF)) == got


@pytest.mark.parametrize("kind", ["lattice", "tied-w", "tied-x", "tied-y", "tied-z"])
def test_hv4d_tied_coordinates(core, kind) -> None:
    pts = lattice_points(30, 4, 7) if kind == "lattice" else tied_front4("wxyz".index(kind[-1]))
    want = hv_grid(pts, _REF)
    got = core.hv4d(_c(pts), *map(float, _REF))
    print(f"hv4d {kind}: got {got!r} want {want!r} rel err {abs(got - want) / want:.3e}")
    np.testing.assert_allclose(got, want, rtol=_hv_rtol(len(pts)))


def test_hv4d_rejects_malformed(core) -> None:
    assert core.hv4d(np.empty((0, 4)), 1.0, 1.0, 1.0, 1.0) == 0.0
    with pytest.raises(RuntimeError):
        core.hv4d(np.zeros((3, 3)), 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(RuntimeError):
        core.hssp4d_contrib(np.zeros((3, 3)), *hssp_views4(np.empty((0, 4))), 1.0, 1.0, 1.0, 1.0)
    views = list(hssp_views4(np.full((2, 4), 0.5)))
    views[3] = views[3][:1]
    with pytest.raises(RuntimeError):
        core.hssp4d_contrib(np.zeros((3, 4)), *views, 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(RuntimeError):
        core.Hssp4dSession(np.zeros((3, 3)), 1.0, 1.0, 1.0, 1.0)
    assert core.HSSP4D_MAX_SUBSET == hssp._DEVICE_HSSP4D_MAX_SUBSET


# ---------------------------------------------------------------------------
# hssp4d_contrib
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _contrib_case(k: int) -> tuple[np.ndarray, np.ndarray]:
    r = np.random.RandomState(400 + k)
    # Selected points: half on a coarse lattice (ties among themselves), half free.
    sel = np.round(r.uniform(0.1, 0.9, (k, 4)), 1)
    sel[k // 2 :] = r.uniform(0.1, 0.9, (k - k // 2, 4))
    cand = r.uniform(0.05, 0.95, (20, 4))
    cand[0] = 0.01  # dominates every selected point
    if k:
        a, b, m = sel[0], sel[k - 1], sel[k // 2]
        cand[1] = a  # equal to a selected point
        cand[2] = b + [0.02, 0.03, 0.0, 0.01]  # dominated by a selected point
        cand[3] = [a[0], 0.07, 0.9, 0.5]  # shares w
        cand[4] = [0.9, b[1], 0.06, 0.5]  # shares x
        cand[5] = [0.08, 0.85, m[2], 0.5]  # shares y
        cand[6] = [0.5, 0.08, 0.85, a[3]]  # shares z
        cand[7] = [a[0], b[1], m[2], a[3]]  # shares all four
    sel.setflags(write=False)
    cand.setflags(write=False)
    return sel, cand


def _contribs(core, cand: np.ndarray, sel: np.ndarray, ref: np.ndarray) -> np.ndarray:
    return np.asarray(core.hssp4d_contrib(_c(cand), *hssp_views4(sel), *map(float, ref)))


@pytest.mark.parametrize("k", [0, 1, 2, 33, 65])
def test_hssp4d_contrib_edges(core, k) -> None:
    sel, cand = _contrib_case(k)
    ref = np.array([1.0, 1.1, 1.2, 1.05])
    if k <= 17:
        def hv(p):
            return hv_grid(p, ref)
    else:
        def hv(p):
            return wfg.compute_hypervolume(p, ref)

    with _host_only():
        base = hv(sel)
        want = np.array([hv(np.vstack([sel, c[None, :]])) - base for c in cand])
    incl = np.prod(ref[None, :] - cand, axis=1)
    if k:
        assert abs(want[1]) <= 1e-12 and abs(want[2]) <= 1e-12
    else:
        np.testing.assert_allclose(want, incl, rtol=1e-12)
    got = _contribs(core, cand, sel, ref)
    print(f"k={k}: max |got - want| / incl = {np.max(np.abs(got - want) / incl):.3e}")
    assert (np.abs(got - want) <= 1e-10 * incl).all(), (got, want)
    if k:
        assert abs(got[1]) <= 1e-12 and abs(got[2]) <= 1e-12
    # no floating-point atomics: a second run is bit-identical
    np.testing.assert_array_equal(_contribs(core, cand, sel, ref), got)


# ---------------------------------------------------------------------------
# Session
# ---------------------------------------------------------------------------


def _front40() -> np.ndarray:
    return sphere_front(40, 4, 21)


@functools.lru_cache(maxsize=None)
def _host_greedy39() -> np.ndarray:
    """Host lazy-greedy order of 39 of the 40 tie-free candidates. Exact greedy
    equals this order here: the smallest relative gap between the top two
    contributions over all rounds is 6.5e-3, far above rounding."""
    with _host_only():
        out = hssp._solve_hssp(_front40(), np.arange(40), 39, _HSSP_REF)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("subset_size", [1, 2, 20, 39, 40, 60])
def test_hssp4d_session_matches_host_order(core, subset_size) -> None:
    session = core.Hssp4dSession(_c(_front40()), *map(float, _HSSP_REF))
    got = np.asarray(session.run(subset_size))
    first = _host_greedy39()
    if subset_size < 40:
        want = first[:subset_size]
    else:  # the last pick is whatever is left; 60 clamps to n
        want = np.append(first, np.setdiff1d(np.arange(40), first))
    np.testing.assert_array_equal(got, want)


def test_hssp4d_session_matches_stateless_kernel_past_one_wavefront(core) -> None:
    cand = sphere_front(70, 4, 23)
    got = np.asarray(core.Hssp4dSession(_c(cand), *map(float, _HSSP_REF)).run(69))
    picked: list[int] = []
    for _ in range(69):
        vals = _contribs(core, cand, cand[picked], _HSSP_REF)
        vals[picked] = -np.inf
        picked.append(int(np.argmax(vals)))  # lowest index on ties
    np.testing.assert_array_equal(got, np.array(picked))


@pytest.mark.parametrize("subset_size", [20, 65])
def test_hssp4d_session_with_duplicates(core, subset_size) -> None:
    cand = sphere_front(100, 4, 22).copy()
    cand[70:] = cand[np.random.RandomState(5).choice(70, 30, replace=False)]
    got = np.asarray(core.Hssp4dSession(_c(cand), *map(float, _HSSP_REF)).run(subset_size))
    assert got.shape == (subset_size,)
    assert ((got >= 0) & (got < 100)).all()
    assert len(np.unique(got)) == subset_size
    incl = np.prod(_HSSP_REF[None, :] - cand, axis=1)
    worst = 0.0
    for r in range(subset_size):
        vals = _contribs(core, cand, cand[got[:r]], _HSSP_REF)
        rest = np.setdiff1d(np.arange(100), got[:r])
        slack = (vals[rest] - vals[got[r]]) / incl[rest]
        worst = max(worst, float(slack.max()))
        assert (slack <= 1e-10).all(), (r, got[r], slack.max())
    print(f"largest (other - picked) / incl over {subset_size} rounds: {worst:.3e}")


# ---------------------------------------------------------------------------
# Python level
# ---------------------------------------------------------------------------


def test_solve_hssp_device_equals_host(core, monkeypatch) -> None:
    cand = _front40()
    idx = np.arange(40)
    monkeypatch.setattr(hssp, "_DEVICE_HSSP4D_MIN_WORK", 0)
    dev = hssp._solve_hssp(cand, idx, 20, _HSSP_REF)
    monkeypatch.setattr(hssp, "_DEVICE_HSSP4D_MIN_WORK", _OFF)
    monkeypatch.setattr(wfg, "_DEVICE_HV4D_MIN_ROWS", _OFF)
    host = hssp._solve_hssp(cand, idx, 20, _HSSP_REF)
    np.testing.assert_array_equal(dev, host)
    np.testing.assert_array_equal(host, _host_greedy39()[:20])


def test_compute_hypervolume_device_equals_host(core, monkeypatch) -> None:
    pts = sphere_front(64, 4, 31)
    monkeypatch.setattr(wfg, "_DEVICE_HV4D_MIN_ROWS", 0)
    dev = wfg.compute_hypervolume(pts, _REF)
    monkeypatch.setattr(wfg, "_DEVICE_HV4D_MIN_ROWS", _OFF)
    host = wfg.compute_hypervolume(pts, _REF)
    print(f"hv 64 x 4: device {dev!r} host {host!r} rel err {abs(dev - host) / host:.3e}")
    np.testing.assert_allclose(dev, host, rtol=1e-10)


# ---------------------------------------------------------------------------
# End to end
# ---------------------------------------------------------------------------


def test_four_objective_tpe_study_uses_the_session(core, monkeypatch) -> None:
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    dims = 4
    dists = {f"x{i}": optuna_amd.distributions.FloatDistribution(0.0, 1.0) for i in range(dims)}
    study = optuna_amd.create_study(
        directions=["minimize"] * 4,
        sampler=optuna_amd.samplers.TPESampler(seed=0, n_startup_trials=10),
    )
    r = np.random.RandomState(0)
    front = sphere_front(400, 4, 33)
    study.add_trials(
        [
            optuna_amd.create_trial(
                params={f"x{i}": float(r.uniform(0, 1)) for i in range(dims)},
                distributions=dists,
                values=[float(v) for v in row],
            )
            for row in front
        ]
    )

    runs: list[int] = []
    real = core.Hssp4dSession

    class Spy:
        def __init__(self, *args) -> None:
            self._inner = real(*args)

        def run(self, subset_size: int):
            runs.append(subset_size)
            return self._inner.run(subset_size)

    class SpyCore:
        Hssp4dSession = Spy

        def __getattr__(self, name):
            return getattr(core, name)

    spy_core = SpyCore()
    monkeypatch.setattr(_hip, "get", lambda: spy_core)
    for step in range(3):
        trial = study.ask()
        params = {f"x{i}": trial.suggest_float(f"x{i}", 0.0, 1.0) for i in range(dims)}
        assert all(0.0 <= v <= 1.0 for v in params.values())
        assert len(runs) >= step + 1, "Hssp4dSession.run was not used on this suggest"
        v = np.abs(r.randn(4)) + 1e-3
        study.tell(trial, list(v / np.linalg.norm(v)))
