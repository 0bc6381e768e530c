"""Edge-shape differential tests for the TPE HIP kernels.

Every case calls the extension directly (below the sampler's dispatch
thresholds) and compares against ``optuna_amd.testing.tpe_reference``, an
independent fp64 reference that shares no formula with the kernels; the CPU
suite pins that reference against the host estimator.

Tolerance: rtol = atol = 1e-9 (the project's device-vs-host bound); ``-inf``
must match exactly and NaN is never allowed.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from optuna_amd import _hip
from optuna_amd.distributions import FloatDistribution
from optuna_amd.samplers._tpe.sampler import default_weights
from optuna_amd.testing import tpe_reference as ref_mod
from optuna_amd.testing.tpe_reference import default_ramp, edge_cases, mixture_logpdf


pytestmark = pytest.mark.gpu

RTOL = 1e-9
ATOL = 1e-9


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


def _check(got: np.ndarray, ref: np.ndarray) -> None:
    got = np.asarray(got)
    assert got.shape == ref.shape
    print("max |got - ref| over finite:",
          np.max(np.abs(got - ref)[np.isfinite(ref) & np.isfinite(got)], initial=0.0))
    assert not np.isnan(got).any(), got
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
    finite = np.isfinite(ref)
    np.testing.assert_allclose(got[finite], ref[finite], rtol=RTOL, atol=ATOL)


def _logw(weights: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore"):
        return np.log(weights)


def _sorted_cols(obs: np.ndarray, rows: np.ndarray | None = None) -> list[np.ndarray]:
    """Per-dim stable sorted order of the given table rows (default: all)."""
    if rows is None:
        rows = np.arange(obs.shape[0])
    return [
        np.ascontiguousarray(rows[np.argsort(obs[rows, d], kind="stable")].astype(np.int32))
        for d in range(obs.shape[1])
    ]


def _table(core, obs: np.ndarray):
    hist = core.TpeDeviceHistory(obs.shape[1])
    if len(obs):
        hist.append(np.ascontiguousarray(obs))
    return hist


def _score(hist, cols, pos, n_above, a, per_dim=False, **extras):
    return hist.score(
        cols, pos, n_above, _logw(a["weights"]), a["alow"], a["ahigh"], a["steps"],
        a["n_choices"], a["prior_weight"], np.ascontiguousarray(a["x"]),
        np.ascontiguousarray(a["xedges"]), a["consider_endpoints"], a["magic_clip"],
        per_dim=per_dim, **extras,
    )


# ---------------------------------------------------------------------------
# Scoring routes over the shared case table
# ---------------------------------------------------------------------------

_CASES = {c.name: c for c in edge_cases()}


@functools.lru_cache(maxsize=None)
def _case_ref(name: str, per_dim: bool) -> np.ndarray:
    out = _CASES[name].reference(per_dim=per_dim)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(_CASES))
def test_kde_logpdf_edge(core, name) -> None:
    case = _CASES[name]
    a = case.kde_args()
    obs = a["obs"]
    sorted_pos = np.ascontiguousarray(
        np.argsort(obs, axis=0, kind="stable").astype(np.int64)
    ).reshape(obs.shape)
    got = core.kde_logpdf(
        np.ascontiguousarray(obs), sorted_pos, _logw(a["weights"]), a["alow"], a["ahigh"],
        a["steps"], a["n_choices"], a["prior_weight"], np.ascontiguousarray(a["x"]),
        np.ascontiguousarray(a["xedges"]), a["consider_endpoints"], a["magic_clip"],
    )
    _check(got, _case_ref(name, False))
    if case.expect_all_neginf:
        assert np.isneginf(got).all()


@pytest.mark.parametrize("per_dim", [False, True], ids=["joint", "perdim"])
@pytest.mark.parametrize("name", list(_CASES))
def test_resident_score_edge(core, name, per_dim) -> None:
    """All rows appended, explicit sorted columns, identity position map."""
    case = _CASES[name]
    a = case.kde_args()
    obs = a["obs"]
    n = obs.shape[0]
    hist = _table(core, obs)
    got = _score(hist, _sorted_cols(obs) if n else [], np.arange(n, dtype=np.int32), n, a,
                 per_dim=per_dim)
    _check(got, _case_ref(name, per_dim))
    if case.expect_all_neginf and not per_dim:
        assert np.isneginf(got).all()


# ---------------------------------------------------------------------------
# Resident table: subset compaction
# ---------------------------------------------------------------------------

_FLOAT2 = dict(
    alow=np.full(2, -5.0), ahigh=np.full(2, 5.0), steps=np.zeros(2), n_choices=np.zeros(2),
    prior_weight=1.0, consider_endpoints=False, magic_clip=True,
)


def _float2_args(weights: np.ndarray, x: np.ndarray) -> dict:
    return dict(_FLOAT2, weights=weights, x=x, xedges=np.zeros((len(x), 4)))


def _mix_weights(raw: np.ndarray) -> np.ndarray:
    w = np.append(raw, [1.0]) if len(raw) else np.array([1.0])
    return w / w.sum()


@functools.lru_cache(maxsize=None)
def _compaction_table(n: int) -> tuple[np.ndarray, np.ndarray]:
    r = np.random.RandomState(500 + n)
    obs, x = r.uniform(-5, 5, (n, 2)), r.uniform(-5, 5, (5, 2))
    obs.setflags(write=False)
    x.setflags(write=False)
    return obs, x


def _subset(kind: str, obs: np.ndarray) -> np.ndarray | None:
    n = len(obs)
    order0 = np.argsort(obs[:, 0], kind="stable")
    if kind == "empty":
        sel = np.empty(0, dtype=np.int64)
    elif kind == "all":
        sel = np.arange(n)
    elif kind == "first":
        sel = np.array([0])
    elif kind == "last":
        sel = np.array([n - 1])
    elif kind == "every-other":
        sel = np.arange(0, n, 2)
    elif kind == "tile0-empty":  # no member among dim 0's first 256 sorted positions
        sel = order0[256:] if n > 256 else None
    elif kind == "last-tile-only":
        sel = order0[(n - 1) // 256 * 256:] if n > 256 else None
    else:
        raise ValueError(kind)
    return None if sel is None else np.sort(sel)


_SUBSETS = ["empty", "all", "first", "last", "every-other", "tile0-empty", "last-tile-only"]
_COMPACTION = [
    (n, kind)
    for n in (1, 256, 257, 513)
    for kind in _SUBSETS
    if n > 256 or kind not in ("tile0-empty", "last-tile-only")
]


@pytest.mark.parametrize("n,kind", _COMPACTION)
def test_compaction_subsets(core, n, kind) -> None:
    obs, x = _compaction_table(n)
    sel = _subset(kind, obs)
    hist = _table(core, obs)
    pos = np.full(n, -1, dtype=np.int32)
    pos[sel] = np.arange(len(sel), dtype=np.int32)
    a = _float2_args(_mix_weights(default_ramp(len(sel))), x)
    want = {pd: mixture_logpdf(obs=obs[sel], **a, per_dim=pd) for pd in (False, True)}
    for pd in (False, True):
        _check(_score(hist, _sorted_cols(obs), pos, len(sel), a, per_dim=pd), want[pd])


def test_compaction_with_invalid_rows(core) -> None:
    """Invalid rows are -1 in ``pos`` and absent from the sorted columns, so
    the sorted length Nv is smaller than the table."""
    r = np.random.RandomState(9)
    n = 300
    obs, x = r.uniform(-5, 5, (n, 2)), r.uniform(-5, 5, (5, 2))
    invalid = np.sort(r.choice(n, 40, replace=False))
    valid = np.setdiff1d(np.arange(n), invalid)
    obs[invalid] = 0.0
    sel = valid[::3]
    hist = _table(core, obs)
    pos = np.full(n, -1, dtype=np.int32)
    pos[sel] = np.arange(len(sel), dtype=np.int32)
    cols = _sorted_cols(obs, valid)
    assert len(cols[0]) == n - 40
    a = _float2_args(_mix_weights(default_ramp(len(sel))), x)
    for pd in (False, True):
        _check(_score(hist, cols, pos, len(sel), a, per_dim=pd),
               mixture_logpdf(obs=obs[sel], **a, per_dim=pd))


# ---------------------------------------------------------------------------
# Resident sorted index
# ---------------------------------------------------------------------------


def _trials(space, block: np.ndarray, offset: int):
    from optuna_amd.testing.trials import _create_frozen_trial

    names = list(space)
    return [
        _create_frozen_trial(
            number=offset + j, values=(0.0,),
            params={n: float(v) for n, v in zip(names, row) if not np.isnan(v)},
            distributions={n: space[n] for n, v in zip(names, row) if not np.isnan(v)},
        )
        for j, row in enumerate(block)
    ]


@pytest.mark.parametrize("kind", ["positions", "growth"])
def test_resident_sorted_index(core, kind) -> None:
    from optuna_amd.samplers._tpe._history import _SpaceCache

    space = {"a": FloatDistribution(-5.0, 5.0), "b": FloatDistribution(-5.0, 5.0)}
    cache = _SpaceCache(space)
    hist = core.TpeDeviceHistory(2)
    x = np.random.RandomState(3).uniform(-5, 5, (5, 2))
    n_rows = 0
    for step, block in enumerate(ref_mod.sorted_index_batches(kind)):
        cache.append(_trials(space, block, n_rows))
        table = np.array(cache.params[n_rows:], dtype=np.float64)
        table[np.isnan(block).any(axis=1)] = 0.0  # never indexed: not in the sorted order
        hist.append(np.ascontiguousarray(table))
        if step == 0:
            hist.upload_sorted(list(cache.sorted_rows))
        else:
            # One insert per run of valid rows, as the sampler's mirror does.
            ok = np.concatenate([[False], cache.valid[n_rows:], [False]])
            edges = np.flatnonzero(ok[1:] != ok[:-1])
            for first, end in zip(edges[::2], edges[1::2]):
                hist.insert_sorted_by_value(n_rows + int(first), int(end - first))
        n_rows += len(block)
        valid = np.nonzero(cache.valid)[0]
        assert hist.n_sorted == len(valid) == cache._n_sorted

        pos = np.full(n_rows, -1, dtype=np.int32)
        pos[valid] = np.arange(len(valid), dtype=np.int32)
        a = _float2_args(_mix_weights(default_weights(len(valid))), x)
        resident = _score(hist, [], pos, len(valid), a)
        explicit = _score(hist, [np.ascontiguousarray(c) for c in cache.sorted_rows], pos,
                          len(valid), a)
        np.testing.assert_array_equal(resident, explicit)
        _check(resident, mixture_logpdf(obs=np.array(cache.params)[valid], **a))


def test_score_refuses_n_above_beyond_the_index(core) -> None:
    """A host-side argument check: it throws before anything is launched, and
    a correct call on the same history then scores as usual."""
    obs = np.array([[-1.0, 2.0], [3.0, -4.0], [0.5, 0.25]])
    x = np.random.RandomState(5).uniform(-5, 5, (4, 2))
    pos = np.arange(3, dtype=np.int32)
    hist = _table(core, obs)
    hist.upload_sorted(_sorted_cols(obs))
    bad = _float2_args(_mix_weights(default_ramp(4)), x)
    with pytest.raises(RuntimeError, match="n_above"):
        _score(hist, [], pos, 4, bad)
    a = _float2_args(_mix_weights(default_ramp(3)), x)
    _check(_score(hist, [], pos, 3, a), mixture_logpdf(obs=obs, **a))


# ---------------------------------------------------------------------------
# Extras (constant-liar rows merged into the compacted subset on device)
# ---------------------------------------------------------------------------

# dim 0 sorted: -4, -3.5, -2.5, -0.5, 1, 2, 3, 4.5 — the neighbour gaps around
# -0.5 (2.0 left, 1.5 right) differ and exceed the magic-clip floor, so which of
# two tied kernels sorts first changes their bandwidths.
_FIN = np.array(
    [[-4.0, 0.3], [-2.5, -4.2], [-0.5, 2.2], [1.0, -1.1], [3.0, 4.4], [4.5, -2.9],
     [-3.5, 1.4], [2.0, -0.2], [0.2, 3.1], [-1.7, -3.6]]
)
_SEL = np.arange(8)  # rows 8, 9 stay outside the subset


def _extras_case(name: str) -> tuple[np.ndarray, np.ndarray]:
    r = np.random.RandomState(41)
    sel = _SEL
    if name == "L1-equal-finished":
        ex = np.array([[-0.5, 0.9]])
    elif name == "L2-duplicates-equal-finished":
        ex = np.array([[1.9, -1.1], [1.9, -1.1]])
    elif name == "L2-below-and-above-all":
        ex = np.array([[-4.9, -4.8], [4.9, 4.8]])
    elif name == "L2-both-below-all":
        ex = np.array([[-4.9, -4.8], [-4.7, -4.6]])
    elif name == "L2-both-above-all":
        ex = np.array([[4.9, 4.8], [4.7, 4.6]])
    elif name == "L300-ties-and-duplicates":
        ex = r.uniform(-5, 5, (300, 2))
        ex[10] = _FIN[2]
        ex[11, 0] = _FIN[4, 0]
        ex[200] = ex[20]
        ex[299, 1] = ex[0, 1]
    elif name == "Na0-L3":
        ex = np.array([[0.5, -0.5], [-2.0, 3.0], [0.5, 1.0]])
        sel = np.empty(0, dtype=np.int64)
    else:
        raise ValueError(name)
    return sel, ex


@pytest.mark.parametrize(
    "name",
    ["L1-equal-finished", "L2-duplicates-equal-finished", "L2-below-and-above-all",
     "L2-both-below-all", "L2-both-above-all", "L300-ties-and-duplicates", "Na0-L3"],
)
def test_extras_merge(core, name) -> None:
    sel, ex = _extras_case(name)
    x = np.random.RandomState(8).uniform(-5, 5, (5, 2))
    x[0] = [-0.5, 2.2]
    hist = _table(core, _FIN)
    pos = np.full(len(_FIN), -1, dtype=np.int32)
    pos[sel] = np.arange(len(sel), dtype=np.int32)
    order = np.argsort(ex, axis=0, kind="stable")
    extras = dict(
        extras_raw=np.ascontiguousarray(ex),
        extras_sorted=np.ascontiguousarray(np.take_along_axis(ex, order, axis=0).T),
        extras_sorted_idx=np.ascontiguousarray(order.T.astype(np.int32)),
    )
    combined = np.concatenate([_FIN[sel], ex])
    a = _float2_args(_mix_weights(default_ramp(len(combined))), x)
    for pd in (False, True):
        got = _score(hist, _sorted_cols(_FIN), pos, len(sel), a, per_dim=pd, **extras)
        _check(got, mixture_logpdf(obs=combined, **a, per_dim=pd))
