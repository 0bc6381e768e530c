"""Differential tests for the fused TPE suggest entry point and the
insert-by-value kernel of the resident sorted index.

The extension is called directly. ``fused_score(..., return_parts=True)``
returns ``((3, S) [ei | log g | log l], (K,) above log-weights)``; log g and
log l are compared against ``optuna_amd.testing.tpe_reference`` (an independent
fp64 reference that shares no formula with the kernels) and against the unfused
``score()`` on the same inputs with an explicit position map.

Tolerance: rtol = atol = 1e-9 (the project's device-vs-host bound); ``-inf``
must match exactly and NaN is never allowed. The default weight ramp written on
device is compared with ``np.log(w / w.sum())`` at 1e-12 absolute.

Shapes are the smallest at which each mechanism can go wrong: table rows at the
endpoint rules (1, 2, 3), the 256-position tile edge (255, 256, 257) and the
512-kernel single-phase/two-phase edge (K = 512, 513, 514 out of 513 rows).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from optuna_amd import _hip
from optuna_amd.distributions import FloatDistribution
from optuna_amd.samplers._tpe.sampler import default_weights
from optuna_amd.testing import tpe_reference as ref_mod
from optuna_amd.testing.tpe_reference import EdgeCase, kernel_sigmas, mixture_logpdf


pytestmark = pytest.mark.gpu

RTOL = 1e-9
ATOL = 1e-9

_CONT3 = {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(3)}
_CONT1 = {"x0": FloatDistribution(-5.0, 5.0)}
# One log dim and one stepped dim (the stepped one exercises xedges).
_MIXED3 = {
    "f": FloatDistribution(-5.0, 5.0),
    "lf": FloatDistribution(1e-3, 1e3, log=True),
    "sf": FloatDistribution(0.0, 10.0, step=0.5),
}


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


def _check(got: np.ndarray, ref: np.ndarray, what: str) -> None:
    got = np.asarray(got)
    assert got.shape == ref.shape
    both = np.isfinite(ref) & np.isfinite(got)
    print(f"{what}: max |got - ref| over finite:", np.max(np.abs(got - ref)[both], initial=0.0))
    assert not np.isnan(got).any(), (what, got)
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
    finite = np.isfinite(ref)
    np.testing.assert_allclose(got[finite], ref[finite], rtol=RTOL, atol=ATOL)


def _logw(weights: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore"):
        return np.log(weights)


def _mix(w: np.ndarray, prior_weight: float) -> np.ndarray:
    if len(w) == 0:
        return np.array([1.0])
    w = np.append(w, [prior_weight])
    return w / w.sum()


@functools.lru_cache(maxsize=None)
def _inputs(space_tag: str, n: int, S: int, data: str, seed: int):
    """KDE-domain table, domain arrays and candidates (read-only, shared)."""
    space = {"cont1": _CONT1, "cont3": _CONT3, "mixed3": _MIXED3}[space_tag]
    r = np.random.RandomState(seed)
    obs_raw = ref_mod._draw(r, space, n)
    D = obs_raw.shape[1]
    if data == "dups":
        # A constant column and a column over five distinct values.
        obs_raw[:, 0] = 1.25
        if D > 1:
            obs_raw[:, 1] = r.choice([-4.0, -1.0, 0.0, 2.5, 4.0], n)
    elif data == "lattice":
        # Tie-free jittered lattice, min gap >= range / (4 n): keeps the
        # bandwidths large enough for the 1e-9 bound with the magic clip off.
        cell = 10.0 / n
        for d in range(D):
            lat = -5.0 + cell * (np.arange(n) + 0.5) + r.uniform(-0.25, 0.25, n) * cell
            obs_raw[:, d] = r.permutation(lat)
    case = EdgeCase("fused", space, obs_raw, np.ones(n), 1.0, ref_mod._draw(r, space, S))
    a = case.kde_args()
    out = {k: a[k] for k in ("obs", "alow", "ahigh", "steps", "n_choices", "x", "xedges")}
    for v in out.values():
        v.setflags(write=False)
    return out


def _sorted_cols(obs: np.ndarray) -> list[np.ndarray]:
    return [
        np.ascontiguousarray(np.argsort(obs[:, d], kind="stable").astype(np.int32))
        for d in range(obs.shape[1])
    ]


def _resident(core, a):
    obs = a["obs"]
    hist = core.TpeDeviceHistory(obs.shape[1])
    hist.append(np.ascontiguousarray(obs))
    hist.upload_sorted(_sorted_cols(obs))
    hist.set_domain(a["alow"], a["ahigh"], a["steps"], a["n_choices"])
    return hist


def _excl(kind: str, obs: np.ndarray) -> np.ndarray:
    """Exclusion lists named by their place in dim 0's sorted order."""
    n = len(obs)
    order0 = np.argsort(obs[:, 0], kind="stable")
    if kind == "empty":
        rows = order0[:0]
    elif kind == "first":
        rows = order0[:1]
    elif kind == "last":
        rows = order0[-1:]
    elif kind == "first+last":
        rows = order0[[0, -1]] if n >= 2 else order0[:1]
    elif kind == "straddle-tile":
        rows = order0[255:257]
    elif kind == "whole-tile":
        rows = order0[256:512]
    elif kind == "whole-first-tile":
        rows = order0[:256]
    elif kind == "1024":
        rows = np.random.RandomState(5).choice(n, 1024, replace=False)
    else:
        raise ValueError(kind)
    return np.sort(rows).astype(np.int32)


def _below(a, rows: np.ndarray, ce: bool, mc: bool, prior_weight: float):
    """Below estimator over the given table rows: kernels and reference inputs."""
    obs = a["obs"][rows]
    D = obs.shape[1]
    mid = 0.5 * (a["alow"] + a["ahigh"])
    rng_ = a["ahigh"] - a["alow"]
    if len(rows) == 0:
        mus, sigmas = mid[None, :].copy(), rng_[None, :].copy()
    else:
        sig = np.column_stack(
            [kernel_sigmas(obs[:, d], a["alow"][d], a["ahigh"][d], ce, mc) for d in range(D)]
        )
        mus = np.vstack([obs, mid])
        sigmas = np.vstack([sig, rng_])
    w = _mix(default_weights(len(rows)), prior_weight)
    return obs, np.ascontiguousarray(mus), np.ascontiguousarray(sigmas), w


def _run_case(core, a, excl, ce, mc, prior_weight=1.0, custom_weights=None, hist=None,
              below_rows=None):
    """One fused call checked against the reference and against score()."""
    from optuna_amd.samplers._tpe._device import default_weight_ramp

    obs = a["obs"]
    n, D = obs.shape
    if hist is None:
        hist = _resident(core, a)
    members = np.setdiff1d(np.arange(n), excl)
    Na = len(members)
    # The below estimator needs no relation to excl on device; unless told
    # otherwise use the excluded rows (at most 40 keeps the reference small).
    if below_rows is None:
        below_rows = excl[:40]
    bobs, bmu, bsig, bw = _below(a, below_rows, ce, mc, prior_weight)
    kw = dict(alow=a["alow"], ahigh=a["ahigh"], steps=a["steps"], n_choices=a["n_choices"],
              prior_weight=prior_weight, x=a["x"], xedges=a["xedges"],
              consider_endpoints=ce, magic_clip=mc)
    if custom_weights is None:
        w_above = _mix(default_weights(Na), prior_weight)
        logw_arg = np.empty(0)
        w_num, w_start, w_step, log_total = default_weight_ramp(Na, prior_weight)
    else:
        w_above = _mix(custom_weights, prior_weight)
        logw_arg = _logw(w_above)
        w_num, w_start, w_step, log_total = 0, 1.0, 0.0, 0.0
    has_steps = bool((a["steps"] > 0).any())
    parts, logw_dev = hist.fused_score(
        excl, Na, np.ascontiguousarray(a["x"]),
        np.ascontiguousarray(a["xedges"]) if has_steps else np.empty(0),
        bmu, bsig, bw, logw_arg, w_num, w_start, w_step, log_total, prior_weight,
        ce, mc, True,
    )
    ei, log_g, log_l = parts

    # Above log-weights as the scoring kernels read them.
    ref_logw = _logw(w_above)
    assert logw_dev.shape == ref_logw.shape
    if custom_weights is None:
        np.testing.assert_array_equal(np.isneginf(logw_dev), np.isneginf(ref_logw))
        fin = np.isfinite(ref_logw)
        print("max |logw - ref|:", np.max(np.abs(logw_dev - ref_logw)[fin], initial=0.0))
        np.testing.assert_allclose(logw_dev[fin], ref_logw[fin], rtol=0.0, atol=1e-12)
    else:
        np.testing.assert_array_equal(logw_dev, ref_logw)

    ref_g = mixture_logpdf(obs=obs[members], weights=w_above, **kw)
    ref_l = mixture_logpdf(obs=bobs, weights=bw, **kw)
    _check(log_g, ref_g, "log_g")
    _check(log_l, ref_l, "log_l")
    _check(ei, ref_l - ref_g, "ei")

    pos = np.full(n, -1, dtype=np.int32)
    pos[members] = np.arange(Na, dtype=np.int32)
    unfused = hist.score(
        [], pos, Na, _logw(w_above), a["alow"], a["ahigh"], a["steps"], a["n_choices"],
        prior_weight, np.ascontiguousarray(a["x"]), np.ascontiguousarray(a["xedges"]), ce, mc,
    )
    _check(log_g, np.asarray(unfused), "log_g vs score()")

    # The production form returns the (S,) acquisition values only.
    plain = hist.fused_score(
        excl, Na, np.ascontiguousarray(a["x"]),
        np.ascontiguousarray(a["xedges"]) if has_steps else np.empty(0),
        bmu, bsig, bw, logw_arg, w_num, w_start, w_step, log_total, prior_weight,
        ce, mc, False,
    )
    np.testing.assert_array_equal(plain, ei)
    return hist


@pytest.mark.parametrize("excl_kind", ["empty", "first", "last", "first+last"])
@pytest.mark.parametrize("dims", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 513, 1025])
def test_fused_table_sizes(core, n, dims, excl_kind) -> None:
    """Endpoint rules, tile edge and the single-/two-phase edge (513 rows give
    K = 514, 513 and 512 with 0, 1 and 2 rows excluded)."""
    S = 24 if dims == 3 else 1
    a = _inputs("cont3" if dims == 3 else "cont1", n, S, "random", 100 + n)
    ce = (n + dims) % 2 == 0
    _run_case(core, a, _excl(excl_kind, a["obs"]), ce, True)


@pytest.mark.parametrize("ce", [False, True], ids=["ce0", "ce1"])
@pytest.mark.parametrize(
    "n,excl_kind",
    [
        (1025, "straddle-tile"),
        (1025, "whole-tile"),
        (1025, "whole-first-tile"),
        (1025, "1024"),
        (2049, "1024"),
    ],
)
def test_fused_exclusion_patterns(core, n, excl_kind, ce) -> None:
    """Excluded rows at a tile edge, a whole excluded tile (the fit must walk
    the sorted column past it, also to the low endpoint) and a full list."""
    a = _inputs("cont3", n, 24, "random", 200 + n)
    _run_case(core, a, _excl(excl_kind, a["obs"]), ce, True)


@pytest.mark.parametrize("ce", [False, True], ids=["ce0", "ce1"])
def test_fused_magic_clip_off(core, ce) -> None:
    a = _inputs("cont3", 257, 24, "lattice", 301)
    obs = a["obs"]
    order0 = np.argsort(obs[:, 0], kind="stable")
    excl = np.sort(order0[[0, 100, 101, 256]]).astype(np.int32)
    _run_case(core, a, excl, ce, False)


@pytest.mark.parametrize("ce", [False, True], ids=["ce0", "ce1"])
def test_fused_duplicate_values(core, ce) -> None:
    a = _inputs("cont3", 257, 24, "dups", 302)
    excl = np.array([0, 5, 6, 7, 130, 256], dtype=np.int32)
    _run_case(core, a, excl, ce, True)


@pytest.mark.parametrize("n", [3, 257, 513])
def test_fused_log_and_stepped_dims(core, n) -> None:
    a = _inputs("mixed3", n, 24, "random", 400 + n)
    _run_case(core, a, _excl("first+last", a["obs"]), False, True)
    _run_case(core, a, _excl("empty", a["obs"]), True, True, prior_weight=2.5)


@pytest.mark.parametrize("n_above", [1, 24, 25, 26, 27, 60])
def test_fused_default_weight_ramp(core, n_above) -> None:
    """The ramp lengths 0, 1 and 2 around the 25 flat weights (checked at
    1e-12 absolute inside _run_case), with a prior weight other than 1."""
    a = _inputs("cont1", n_above + 2, 1, "random", 500 + n_above)
    _run_case(core, a, np.array([0, n_above + 1], dtype=np.int32), False, True, prior_weight=0.5)


@pytest.mark.parametrize("n", [3, 513, 1025])
def test_fused_custom_weights_upload(core, n) -> None:
    a = _inputs("cont3", n, 24, "random", 600 + n)
    excl = _excl("first", a["obs"])
    w = np.random.RandomState(n).uniform(0.1, 2.0, n - 1)
    w[0] = 0.0  # a zero weight uploads as -inf
    _run_case(core, a, excl, False, True, prior_weight=2.5, custom_weights=w)


def test_fused_rejects_bad_inputs(core) -> None:
    a = _inputs("cont3", 257, 24, "random", 700)
    hist = _resident(core, a)
    _, bmu, bsig, bw = _below(a, np.arange(3), False, True, 1.0)
    x = np.ascontiguousarray(a["x"])

    def call(excl, n_above):
        return hist.fused_score(np.asarray(excl, dtype=np.int32), n_above, x, np.empty(0),
                                bmu, bsig, bw)

    with pytest.raises(RuntimeError):
        call([5, 5], 255)  # not strictly ascending
    with pytest.raises(RuntimeError):
        call([257], 256)  # not a table row
    with pytest.raises(RuntimeError):
        call([3], 258)  # more kernels than indexed rows
    with pytest.raises(RuntimeError):
        call(np.arange(1025), 0)  # list longer than the LDS cache


# ---------------------------------------------------------------------------
# Insert by value
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


def _insert_batches(kind: str) -> list[np.ndarray]:
    if kind in ("positions", "growth"):
        # Front / middle / back single rows, a 5-row batch with ties and an
        # invalid row in the first block; growth across the 1024 capacity.
        return ref_mod.sorted_index_batches(kind)
    r = np.random.RandomState(9)
    if kind == "batches":
        first = r.uniform(-5, 5, (300, 2))
        b64 = r.uniform(-5, 5, (64, 2))
        b64[10] = first[3]  # ties with an existing row and inside the batch
        b64[11] = first[3]
        b64[40, 0] = np.nan  # an invalid row splits the batch into two runs
        return [first, r.uniform(-5, 5, (2, 2)), b64]
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["positions", "growth", "batches"])
def test_insert_sorted_by_value(core, kind) -> None:
    from optuna_amd.samplers._tpe._history import _SpaceCache

    space = {"a": FloatDistribution(-5.0, 5.0), "b": FloatDistribution(-5.0, 5.0)}
    cache = _SpaceCache(space)
    hist = core.TpeDeviceHistory(2)
    n_rows = 0
    for step, block in enumerate(_insert_batches(kind)):
        cache.append(_trials(space, block, n_rows))
        bad = np.isnan(block).any(axis=1)
        table = np.array(cache.params[n_rows:], dtype=np.float64)
        table[bad] = 0.0  # never indexed
        hist.append(np.ascontiguousarray(table))
        if step == 0:
            hist.upload_sorted(list(cache.sorted_rows))
        else:
            # One call per run of valid rows, as the device mirror does.
            r = 0
            while r < len(block):
                if bad[r]:
                    r += 1
                    continue
                e = r
                while e < len(block) and not bad[e]:
                    e += 1
                hist.insert_sorted_by_value(n_rows + r, e - r)
                r = e
        n_rows += len(block)
        assert hist.n_sorted == cache.n_valid == cache._n_sorted
        got = hist.sorted_index()
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, np.stack(cache.sorted_rows))

    # A fused score over the index the inserts produced.
    valid = np.nonzero(cache.valid)[0]
    invalid = np.nonzero(~cache.valid)[0]
    below = valid[::50][:20]
    excl = cache.excluded_rows(below)
    np.testing.assert_array_equal(excl, np.union1d(below, invalid).astype(np.int32))
    obs = np.array(cache.params, dtype=np.float64)
    obs[invalid] = 0.0
    a = dict(obs=obs, alow=np.full(2, -5.0), ahigh=np.full(2, 5.0), steps=np.zeros(2),
             n_choices=np.zeros(2), x=np.random.RandomState(3).uniform(-5, 5, (5, 2)),
             xedges=np.zeros((5, 4)))
    hist.set_domain(a["alow"], a["ahigh"], a["steps"], a["n_choices"])
    _run_case(core, a, excl, False, True, hist=hist, below_rows=below)


# ---------------------------------------------------------------------------
# Sampler level
# ---------------------------------------------------------------------------

# Seed for which the unfused path's own top-two acquisition gap is >= 1e-6 on
# all 16 steps (checked on the CPU by tests/test_tpe_fused_dispatch.py).
SAMPLER_SEED = 0


def _seeded_study(seed: int):
    import optuna_amd

    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    rng = np.random.RandomState(seed)
    dists = {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(4)}
    study = optuna_amd.create_study(
        sampler=optuna_amd.samplers.TPESampler(seed=seed, n_startup_trials=5)
    )
    # Built exactly like the study of the CPU seed check.
    trials = []
    for _ in range(600):
        params = {f"x{i}": float(rng.uniform(-5.0, 5.0)) for i in range(4)}
        value = float(sum(v**2 for v in params.values()))
        trials.append(optuna_amd.create_trial(params=params, distributions=dists, value=value))
    study.add_trials(trials)
    return study


def _suggest_sequence(monkeypatch, seed: int, n_steps: int = 16):
    """(params per step, top-two acquisition gap per step) of a seeded run.
    Every step tells the same objective, so two runs that agree on a step see
    the same history on the next one."""
    from optuna_amd.samplers import TPESampler

    study = _seeded_study(seed)
    gaps: list[float] = []
    orig = TPESampler._compare

    def spy(samples, vals):
        top = np.sort(np.asarray(vals))[-2:]
        gaps.append(float(top[1] - top[0]))
        return orig(samples, vals)

    out = []
    with monkeypatch.context() as m:
        m.setattr(TPESampler, "_compare", staticmethod(spy))
        for _ in range(n_steps):
            t = study.ask()
            p = [t.suggest_float(f"x{i}", -5.0, 5.0) for i in range(4)]
            study.tell(t, float(sum(v**2 for v in p)))
            out.append(p)
    return np.array(out), np.array(gaps)


def test_sampler_fused_matches_unfused(core, monkeypatch) -> None:
    from optuna_amd.samplers._tpe import _device as device_mod

    fused_calls = {"n": 0}
    orig = device_mod.score_above_resident

    def spy(*args, **kwargs):
        if kwargs.get("fused") is not None:
            fused_calls["n"] += 1
        return orig(*args, **kwargs)

    monkeypatch.setattr(device_mod, "score_above_resident", spy)
    monkeypatch.setenv("OPTUNA_AMD_TPE_FUSED", "0")
    ref_params, ref_gaps = _suggest_sequence(monkeypatch, SAMPLER_SEED)
    assert fused_calls["n"] == 0
    monkeypatch.setenv("OPTUNA_AMD_TPE_FUSED", "1")
    got_params, _ = _suggest_sequence(monkeypatch, SAMPLER_SEED)
    assert fused_calls["n"] == 16

    print("unfused top-two gaps:", ref_gaps)
    skipped = 0
    for step in range(16):
        if ref_gaps[step] < 1e-6:
            # Near-tie on the unfused path itself: the argmax may legitimately
            # flip, and if it does the two histories differ from here on.
            skipped += 1
            if not np.array_equal(got_params[step], ref_params[step]):
                break
            continue
        np.testing.assert_array_equal(got_params[step], ref_params[step])
    assert skipped <= 1
