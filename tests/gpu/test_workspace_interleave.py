"""Every entry point lays its own regions over the one shared device workspace.
This suite calls them in two different orders and requires bit-identical
results per call: a region that is sized or placed wrongly shows up as a result
that depends on what the previous call left behind. (The library uses no
floating-point atomics, so equal inputs give equal bits.)

Order A runs each entry point at its small shape, then at its large one.
Order B runs large calls to *other* entry points before each small call, so
the small call's regions lie over their stale contents in a workspace that
those calls have grown.

Each result is also checked against a host reference: ``_truncnorm_np``, the
host non-domination peel, the exact hypervolume grid of
``optuna_amd.testing.hv_reference`` (contributions and greedy orders are
derived from it) and the numpy Parzen estimator. Tolerances are the ones the
edge suites already use for the same entry points.

Shapes are the smallest that reach the carving edges: odd int32 / uint8 counts
(1, 3, 257 rows, odd ``kcap``), one and two bitmask words, zero-length regions
(k = 0, no extras, no stepped edges), odd exclusion lists.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Callable

import numpy as np
import pytest

from optuna_amd import _hip
from optuna_amd.distributions import FloatDistribution
from optuna_amd.samplers._tpe import _truncnorm_np as tn
from optuna_amd.samplers._tpe._device import default_weight_ramp
from optuna_amd.samplers._tpe.parzen import _ParzenEstimator, _ParzenEstimatorParameters
from optuna_amd.samplers._tpe.sampler import default_weights
from optuna_amd.study import _multi_objective as mo
from optuna_amd.testing import tpe_reference as ref_mod
from optuna_amd.testing.hv_reference import hssp_views4, hv_grid, sphere_front
from optuna_amd.testing.tpe_reference import EdgeCase


pytestmark = pytest.mark.gpu

_REF3 = np.array([1.2, 1.3, 1.4])
_REF4 = np.array([1.2, 1.3, 1.4, 1.25])


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


def _c(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


@dataclasses.dataclass(frozen=True)
class _Call:
    name: str
    run: Callable[[object], np.ndarray]  # core -> result
    check: Callable[[np.ndarray], None]  # result against the host reference


@dataclasses.dataclass(frozen=True)
class _Entry:
    name: str
    small: tuple[_Call, ...]
    large: tuple[_Call, ...]


# ---------------------------------------------------------------------------
# Elementwise truncnorm, non-domination rank
# ---------------------------------------------------------------------------


def _log_gauss_mass(n: int) -> _Call:
    r = np.random.RandomState(100 + n)
    a = r.uniform(-6.0, 4.0, n)
    b = a + r.uniform(0.01, 5.0, n)

    def check(got: np.ndarray) -> None:
        assert got.shape == (n,)
        np.testing.assert_allclose(got, tn._log_gauss_mass(a, b), rtol=1e-10, atol=1e-12)

    return _Call(f"log_gauss_mass[n={n}]", lambda core: np.asarray(core.log_gauss_mass(a, b)),
                 check)


def _rank(n: int) -> _Call:
    vals = np.random.RandomState(200 + n).randint(0, 6, (n, 2)).astype(np.float64)
    assert n < mo._DEVICE_RANK_MIN_ROWS  # the reference below is the host peel

    def check(got: np.ndarray) -> None:
        want, _ = mo._calculate_nondomination_rank(vals)
        np.testing.assert_array_equal(got, want)

    return _Call(f"nondomination_rank[N={n}]",
                 lambda core: np.asarray(core.nondomination_rank(_c(vals), n)), check)


# ---------------------------------------------------------------------------
# Hypervolume and greedy HSSP, three and four objectives
# ---------------------------------------------------------------------------


def _lattice_front3(n: int) -> np.ndarray:
    """n points of the antichain i + j + k = 22 on a 1/23 lattice, x-lexsorted:
    ties in every coordinate, and a grid small enough for ``hv_grid``."""
    pts = [(i, j, 22 - i - j) for i in range(23) for j in range(23 - i)]
    out = np.unique(np.array(pts, dtype=np.float64) / 23.0, axis=0)[:n]
    assert len(out) == n
    return out


def _hv(dims: int, n: int) -> _Call:
    if dims == 3:
        pts = _lattice_front3(n)
        ref = _REF3
    else:
        pts = sphere_front(n, 4, 300 + n)
        ref = _REF4

    def run(core) -> np.ndarray:
        fn = core.hv3d if dims == 3 else core.hv4d
        return np.array([fn(_c(pts), *map(float, ref))])

    def check(got: np.ndarray) -> None:
        # 1e-10 is the bound of both hypervolume edge suites at these sizes.
        np.testing.assert_allclose(got[0], hv_grid(pts, ref), rtol=1e-10)

    return _Call(f"hv{dims}d[N={n}]", run, check)


def _views3(sel: np.ndarray):
    """(sx, sxz, sy, syz, syr) of a (k, 3) selected set, by stable argsort."""
    k = len(sel)
    ox = np.argsort(sel[:, 0], kind="stable")
    oy = np.argsort(sel[:, 1], kind="stable")
    rank_x = np.empty(k, dtype=np.int32)
    rank_x[ox] = np.arange(k, dtype=np.int32)
    return (_c(sel[ox, 0]), _c(sel[ox, 2]), _c(sel[oy, 1]), _c(sel[oy, 2]),
            np.ascontiguousarray(rank_x[oy]))


def _gains(cand: np.ndarray, picked: list[int], ref: np.ndarray) -> np.ndarray:
    """Exact contribution of every candidate to the picked set, from the grid."""
    sel = cand[np.array(picked, dtype=np.int64)]
    base = hv_grid(sel, ref)
    return np.array([hv_grid(np.vstack([sel, c[None, :]]), ref) - base for c in cand])


def _hssp3d_contrib(k: int) -> _Call:
    cand = sphere_front(5, 3, 41)
    sel = sphere_front(3, 3, 42)[:k]

    def check(got: np.ndarray) -> None:
        both = np.vstack([sel, cand])
        want = _gains(both, list(range(k)), _REF3)[k:]
        incl = np.prod(_REF3[None, :] - cand, axis=1)
        assert (np.abs(got - want) <= 1e-10 * incl).all(), (got, want)

    def run(core) -> np.ndarray:
        return np.asarray(core.hssp3d_contrib(_c(cand), *_views3(sel), *map(float, _REF3)))

    return _Call(f"hssp3d_contrib[k={k}]", run, check)


def _session(dims: int, n: int, subset_size: int) -> _Call:
    cand = sphere_front(n, dims, 50 + dims)
    ref = np.full(dims, 1.2)

    def run(core) -> np.ndarray:
        cls = core.Hssp3dSession if dims == 3 else core.Hssp4dSession
        return np.asarray(cls(_c(cand), *map(float, ref)).run(subset_size))

    def check(got: np.ndarray) -> None:
        picked: list[int] = []
        for _ in range(subset_size):
            g = _gains(cand, picked, ref)
            g[picked] = -np.inf
            top = np.sort(g)[::-1]
            # The exact greedy order is unambiguous: no near-tie for the lead.
            assert len(top) < 2 or top[0] - top[1] > 1e-6 * top[0]
            picked.append(int(np.argmax(g)))
        np.testing.assert_array_equal(got, np.array(picked))

    return _Call(f"Hssp{dims}dSession.run[n={n}, subset={subset_size}]", run, check)


# ---------------------------------------------------------------------------
# TPE: resident score and fused score, against the numpy Parzen estimator
# ---------------------------------------------------------------------------


def _parzen(space, obs: np.ndarray, weights: np.ndarray | None) -> _ParzenEstimator:
    params = _ParzenEstimatorParameters(
        prior_weight=1.0, consider_magic_clip=True, consider_endpoints=False,
        weights=default_weights, multivariate=True,
    )
    observations = {name: obs[:, d] for d, name in enumerate(space)}
    return _ParzenEstimator(observations, space, params, predetermined_weights=weights)


def _check_logpdf(got: np.ndarray, want: np.ndarray) -> None:
    assert got.shape == want.shape
    assert np.isfinite(want).all() and not np.isnan(got).any()
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9)


def _score(D: int, L: int, per_dim: bool) -> _Call:
    """257 table rows (odd), 2 of them invalid (255 sorted positions, odd), every
    other valid row in the subset, L constant-liar rows, one candidate."""
    space = {f"x{d}": FloatDistribution(-5.0, 5.0) for d in range(D)}
    r = np.random.RandomState(600 + 10 * D + L)
    n = 257
    obs = r.uniform(-5.0, 5.0, (n, D))
    invalid = np.array([17, 200])
    obs[invalid] = 0.0
    valid = np.setdiff1d(np.arange(n), invalid)
    sel = valid[::2]
    extras = r.uniform(-5.0, 5.0, (L, D))
    x = r.uniform(-5.0, 5.0, (1, D))
    pos = np.full(n, -1, dtype=np.int32)
    pos[sel] = np.arange(len(sel), dtype=np.int32)
    cols = [
        np.ascontiguousarray(valid[np.argsort(obs[valid, d], kind="stable")].astype(np.int32))
        for d in range(D)
    ]
    raw_w = np.linspace(0.5, 1.5, len(sel) + L)
    w = np.append(raw_w, [1.0])
    logw = np.log(w / w.sum())
    order = np.argsort(extras, axis=0, kind="stable")
    kw = {}
    if L:
        kw = dict(
            extras_raw=_c(extras),
            extras_sorted=_c(np.take_along_axis(extras, order, axis=0).T),
            extras_sorted_idx=np.ascontiguousarray(order.T.astype(np.int32)),
        )

    def run(core) -> np.ndarray:
        hist = core.TpeDeviceHistory(D)
        hist.append(_c(obs))
        return np.asarray(hist.score(
            cols, pos, len(sel), logw, np.full(D, -5.0), np.full(D, 5.0), np.zeros(D),
            np.zeros(D), 1.0, _c(x), np.zeros((1, 2 * D)), False, True, per_dim=per_dim, **kw,
        ))

    def check(got: np.ndarray) -> None:
        pe = _parzen(space, np.concatenate([obs[sel], extras]), raw_w)
        xs = {name: x[:, d] for d, name in enumerate(space)}
        _check_logpdf(got, pe.log_pdf_per_dim(xs) if per_dim else pe.log_pdf(xs))

    return _Call(f"score[D={D}, L={L}, per_dim={per_dim}]", run, check)


def _fused_score(E: int) -> _Call:
    """70 above rows and E excluded ones, a prior-only below mixture (Kb = 1),
    one candidate, the last dim stepped so that ``xedges`` is packed."""
    space = {
        "x0": FloatDistribution(-5.0, 5.0),
        "x1": FloatDistribution(-5.0, 5.0),
        "s2": FloatDistribution(0.0, 10.0, step=0.5),
    }
    r = np.random.RandomState(700 + E)
    n = 70 + E
    raw_x = ref_mod._draw(r, space, 1)
    a = EdgeCase("t", space, ref_mod._draw(r, space, n), np.ones(n), 1.0, raw_x).kde_args()
    obs = a["obs"]  # no log dims: the KDE domain is the raw one
    excl = np.sort(r.choice(n, E, replace=False)).astype(np.int32)
    members = np.setdiff1d(np.arange(n), excl)
    mid = 0.5 * (a["alow"] + a["ahigh"])
    width = a["ahigh"] - a["alow"]
    tail = (np.empty(0), *default_weight_ramp(len(members), 1.0), 1.0, False, True)

    def run(core) -> np.ndarray:
        hist = core.TpeDeviceHistory(3)
        hist.append(_c(obs))
        hist.upload_sorted([
            np.ascontiguousarray(np.argsort(obs[:, d], kind="stable").astype(np.int32))
            for d in range(3)
        ])
        hist.set_domain(a["alow"], a["ahigh"], a["steps"], a["n_choices"])
        return np.asarray(hist.fused_score(
            excl, len(members), _c(a["x"]), _c(a["xedges"]), _c(mid[None, :]),
            _c(width[None, :]), np.array([1.0]), *tail, False,
        ))

    def check(got: np.ndarray) -> None:
        xs = {name: raw_x[:, d] for d, name in enumerate(space)}
        log_g = _parzen(space, obs[members], None).log_pdf(xs)
        log_l = _parzen(space, np.empty((0, 3)), None).log_pdf(xs)
        _check_logpdf(got, log_l - log_g)

    return _Call(f"fused_score[E={E}]", run, check)


# ---------------------------------------------------------------------------
# The two orders
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _entries() -> tuple[_Entry, ...]:
    flags = (False, True)
    return (
        _Entry("log_gauss_mass", (_log_gauss_mass(1),), (_log_gauss_mass(257),)),
        _Entry("nondomination_rank", (_rank(1),), (_rank(65),)),
        _Entry("hv3d", (_hv(3, 1),), (_hv(3, 257),)),
        _Entry("hssp3d_contrib", (_hssp3d_contrib(0),), (_hssp3d_contrib(3),)),
        _Entry("Hssp3dSession.run", (_session(3, 5, 1),), (_session(3, 5, 4),)),
        _Entry("hv4d", (_hv(4, 1),), (_hv(4, 7),)),
        _Entry("Hssp4dSession.run", (_session(4, 6, 1),), (_session(4, 6, 4),)),
        _Entry("score",
               tuple(_score(1, L, pd) for L in (0, 3) for pd in flags),
               tuple(_score(3, L, pd) for L in (0, 3) for pd in flags)),
        _Entry("fused_score", (_fused_score(1),), (_fused_score(3),)),
    )


def _order_a() -> list[_Call]:
    return [c for e in _entries() for c in e.small + e.large]


def _order_b() -> list[_Call]:
    entries = _entries()
    out: list[_Call] = []
    for i, e in enumerate(entries):
        others = [entries[(i + j) % len(entries)] for j in (1, 2, 4)]
        for j, call in enumerate(e.small):
            out += [o.large[j % len(o.large)] for o in others]
            out.append(call)
        out += e.large
    return out


def test_orders_cover_every_call() -> None:
    a, b = _order_a(), _order_b()
    assert len({c.name for c in a}) == len(a)
    assert {c.name for c in b} == {c.name for c in a}
    assert [c.name for c in a] != [c.name for c in b]


def test_results_do_not_depend_on_call_order(core) -> None:
    # B first: where this module is the first user of the workspace, B's large
    # calls are also the ones that make it grow.
    interleaved = [(c.name, c.run(core)) for c in _order_b()]
    plain = {c.name: c.run(core) for c in _order_a()}
    for name, got in interleaved:
        assert got.dtype == plain[name].dtype
        # Bit for bit, in whatever order and however often the call is made.
        np.testing.assert_array_equal(got, plain[name], err_msg=name)


def test_results_match_host_references(core) -> None:
    for call in _order_a():
        got = call.run(core)
        print(call.name, np.asarray(got).ravel()[:4])
        call.check(got)
