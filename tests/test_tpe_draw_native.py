"""Native draw of the fused TPE suggest (``_hip/csrc/tpe_draw_host.h`` and its
binding ``tpe_draw_bind.h``).

The header and the binding code are compiled into a host-only pybind11 module
(``tests/cpp/tpe_draw_module.cpp``) with the host compiler, and its pieces are
compared bit for bit with what they replace: ``_truncnorm_np.ppf``,
``RandomState.choice``, ``_device.draw_below_native`` with the scoring inputs
``score_fused`` derives, and ``np.argmax``. A stand-alone program
(``tests/cpp/tpe_draw_check.cpp``) runs the header with libm stand-ins, plain
and under the address and undefined-behaviour sanitizers.

The routing tests replace the extension by a stub whose ``fused_draw_score``
runs the host module, and check when the sampler takes the native draw route
and that it returns and leaves behind the same as the two-call route.
"""
from __future__ import annotations

import importlib.util
import shutil
import subprocess
import sysconfig
import types
from pathlib import Path

import numpy as np
import pytest

from optuna_amd import _hip
from optuna_amd.distributions import FloatDistribution, IntDistribution
from optuna_amd.samplers._tpe import _device
from optuna_amd.samplers._tpe import _truncnorm_np as _tn
from optuna_amd.samplers._tpe.parzen import (
    _NumericalSpace,
    _ParzenEstimator,
    _ParzenEstimatorParameters,
)
from optuna_amd.samplers._tpe.sampler import default_weights
from optuna_amd.testing import tpe_below_cases as tc


_ROOT = Path(__file__).resolve().parent.parent
_CSRC = _ROOT / "optuna_amd" / "_hip" / "csrc"
_CPP = Path(__file__).resolve().parent / "cpp"


def _compiler() -> str | None:
    return next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)


@pytest.fixture(scope="module")
def mod(tmp_path_factory):
    """The host-only module, built once and bound to scipy's scalars."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    pybind11 = pytest.importorskip("pybind11")
    out = tmp_path_factory.mktemp("tpe_draw") / (
        "_tpe_draw_host" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so")
    )
    subprocess.run(
        [cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared",
         "-fvisibility=hidden", f"-I{_CSRC}", f"-I{pybind11.get_include()}",
         f"-I{sysconfig.get_paths()['include']}", str(_CPP / "tpe_draw_module.cpp"),
         "-o", str(out)],
        check=True,
    )
    spec = importlib.util.spec_from_file_location("_tpe_draw_host", out)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    capsules = _device._draw_capsules()
    assert capsules is not None, "this scipy exports no scalar capsules"
    assert module.tpe_draw_bind(*capsules) is True and module.tpe_draw_bound()
    return module


def _bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _assert_same(got: np.ndarray, want: np.ndarray, what) -> None:
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), what
    # Stricter than the line above: the bit patterns, signed zeros included.
    diff = np.nonzero(_bits(got) != _bits(want))
    assert len(diff[0]) == 0, (what, len(diff[0]), got[diff][:4], want[diff][:4])


# ---------------------------------------------------------------------------
# Quantile
# ---------------------------------------------------------------------------

_PPF_SHAPES = ((1, 1), (1, 20), (24, 1), (7, 3), (24, 20), (13, 37))  # 13 * 37 = 481


def _ppf_inputs(shape, seed):
    """Intervals of every regime over one domain: kernels left of, right of
    and inside [-5, 5] (a, b both negative, both positive, straddling zero,
    a on zero), sigmas from 1e-3 to 20 times the range, far tails, q on 0 and
    1, a == b and a > b."""
    r = np.random.RandomState(seed)
    mu = r.uniform(-8.0, 8.0, shape)
    mu[r.rand(*shape) < 0.1] = -5.0  # a == 0 exactly
    sigma = 10.0 * 10 ** r.uniform(-4.0, np.log10(20.0), shape)
    a = (-5.0 - mu) / sigma
    b = (5.0 - mu) / sigma
    far = r.rand(*shape) < 0.1
    a[far] = np.where(r.rand(far.sum()) < 0.5, -38.0, 37.5) - r.rand(far.sum())
    b[far] = a[far] + r.uniform(0.01, 3.0, far.sum())
    q = r.uniform(0.0, 1.0, shape)
    q[r.rand(*shape) < 0.08] = 0.0
    q[r.rand(*shape) < 0.08] = 1.0
    same = r.rand(*shape) < 0.05
    b[same] = a[same]
    swap = r.rand(*shape) < 0.05
    a[swap], b[swap] = b[swap] + 0.5, a[swap]
    return q, a, b


@pytest.mark.parametrize("shape", _PPF_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantile_equals_truncnorm_np(mod, shape) -> None:
    seen = dict(left=False, right=False, central=False, a_neg=False, a_nonneg=False,
                far=False, q0=False, q1=False, same=False, swapped=False)
    for seed in range(12):
        q, a, b = _ppf_inputs(shape, 100 * seed + shape[0])
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            want = _tn.ppf(q, a, b)
            got = mod.tpe_draw_ppf(q, a, b)
        _assert_same(got, want, (shape, seed))
        proper = a < b
        seen["left"] |= bool((proper & (b <= 0)).any())
        seen["right"] |= bool((proper & (a > 0)).any())
        seen["central"] |= bool((proper & (a <= 0) & (b > 0)).any())
        seen["a_neg"] |= bool((a < 0).any())
        seen["a_nonneg"] |= bool((a >= 0).any())
        seen["far"] |= bool((np.abs(a) > 37).any())
        seen["q0"] |= bool((q == 0).any())
        seen["q1"] |= bool((q == 1).any())
        seen["same"] |= bool((a == b).any())
        seen["swapped"] |= bool((a > b).any())
    if shape[0] * shape[1] >= 400:  # enough elements to meet every kind
        assert all(seen.values()), seen


def test_quantile_sigma_extremes(mod) -> None:
    """Sigmas of 1e-3 and of 20 times the range, every kernel position."""
    mu = np.repeat(np.linspace(-5.0, 5.0, 11), 2)
    sigma = np.tile([1e-3 * 10.0, 20.0 * 10.0], 11)
    a, b = (-5.0 - mu) / sigma, (5.0 - mu) / sigma
    for qv in (0.0, 1e-300, 0.25, 0.5, 1.0 - 2.0**-53, 1.0):
        q = np.full_like(a, qv)
        with np.errstate(divide="ignore", invalid="ignore"):
            _assert_same(mod.tpe_draw_ppf(q, a, b), _tn.ppf(q, a, b), qv)


# ---------------------------------------------------------------------------
# Kernel choice
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 2, 26, 1025])
def test_choice_equals_randomstate_choice(mod, n) -> None:
    for seed in range(6):
        r = np.random.RandomState(seed)
        w = r.rand(n)
        if n > 1:
            w[r.rand(n) < 0.3] = 0.0
            w[seed % n] = 0.5  # never all zero
        w /= w.sum()
        for S in (1, 24):
            a, b = np.random.RandomState(1000 + seed), np.random.RandomState(1000 + seed)
            want = a.choice(n, p=w, size=S)
            got = mod.tpe_draw_choice(w, b.random_sample(S))
            assert got.dtype == np.int64 and np.array_equal(got, want), (n, seed, S)
            assert a.random_sample() == b.random_sample()  # the streams stay in step


# ---------------------------------------------------------------------------
# Whole draw
# ---------------------------------------------------------------------------


def _numpy_below_kernels(obs, alow, ahigh, consider_endpoints, consider_magic_clip, active):
    """``tpe_below_kernels`` through the estimator's per-dim numpy fit."""
    parameters = _ParzenEstimatorParameters(
        prior_weight=1.0, consider_magic_clip=consider_magic_clip,
        consider_endpoints=consider_endpoints, weights=default_weights, multivariate=True,
    )
    cols = [
        _ParzenEstimator._numerical_kernels(None, obs[:, d], alow[d], ahigh[d], parameters)
        for d in range(obs.shape[1])
    ]
    mus = np.column_stack([m for m, _ in cols])
    sigmas = np.column_stack([s for _, s in cols])
    loc, scale = mus[active, :], sigmas[active, :]
    return mus, sigmas, (alow[None, :] - loc) / scale, (ahigh[None, :] - loc) / scale, loc, scale


def _below_weights(n: int) -> np.ndarray:
    w = np.append(default_weights(n), [1.0]) if n else np.array([1.0])
    return w / w.sum()


def _cache_of(space, raw: np.ndarray, n_invalid: int = 0):
    """What ``draw_below_native`` reads of a ``_SpaceCache``; ``n_invalid``
    rows in between are marked invalid."""
    n, D = raw.shape
    params = np.zeros((n + n_invalid, D))
    valid = np.ones(n + n_invalid, dtype=bool)
    bad = np.linspace(0, n + n_invalid - 1, n_invalid).astype(int)  # spread out
    valid[bad] = False
    params[valid] = raw
    params[~valid] = np.nan
    return types.SimpleNamespace(
        params=params, valid=valid, dists=list(space.values()), names=list(space)
    )


def _check_whole_draw(mod, space, raw, ce, mc, seed, what, S=24, n_invalid=0) -> None:
    cache = _cache_of(space, raw, n_invalid)
    rows = np.arange(len(cache.valid), dtype=np.int64)
    ns = _NumericalSpace.of(cache.dists)
    w = _below_weights(len(raw))
    rng = np.random.RandomState(seed)
    with np.errstate(divide="ignore", invalid="ignore"):
        x_want, mus_want, sig_want = _device.draw_below_native(
            _numpy_below_kernels, cache, rows, w, rng, S, ce, mc
        )
    rng2 = np.random.RandomState(seed)
    u = rng2.random_sample(S)
    q = rng2.uniform(low=0, high=1, size=(S, len(space)))
    with np.errstate(divide="ignore", invalid="ignore"):
        x_raw, mus, sigmas, x_kde, xedges = mod.tpe_draw_candidates(
            cache.params, cache.valid, rows, w, u, q, ns.adapted_lows, ns.adapted_highs,
            ns.kinds, ns.lows, ns.highs, ns.steps, ce, mc,
        )
    _assert_same(x_raw, x_want, (what, "x_raw"))
    _assert_same(mus, mus_want, (what, "mus"))
    _assert_same(sigmas, sig_want, (what, "sigmas"))
    assert rng.random_sample() == rng2.random_sample()
    # The scoring inputs score_fused derives from the candidates.
    is_log, _, _, steps, _ = _device._space_domains(space)
    x_log = x_want.copy()
    if is_log.any():
        x_log[:, is_log] = np.log(x_log[:, is_log])
    _assert_same(x_kde, x_log, (what, "x_kde"))
    _assert_same(xedges, _device._cell_edges(x_want, is_log, steps), (what, "xedges"))


_KINDS5 = {
    "lin": FloatDistribution(-5.0, 5.0),
    "log": FloatDistribution(1e-3, 10.0, log=True),
    "step": FloatDistribution(-5.0, 5.0, step=0.5),
    "logint": IntDistribution(1, 64, log=True),
    "int": IntDistribution(0, 20),
}


def _raw_for(space, n: int, seed: int) -> np.ndarray:
    r = np.random.RandomState(seed)
    cols = []
    for dist in space.values():
        vals = [tc._draw_param(r, dist) for _ in range(n)]
        cols.append(np.asarray(vals, dtype=np.float64))
    return np.column_stack(cols).reshape(n, len(space))


@pytest.mark.parametrize("n", [0, 1, 2, 25])
@pytest.mark.parametrize("ce,mc", [(False, True), (True, False)])
def test_whole_draw_every_dim_kind(mod, n, ce, mc) -> None:
    for seed in range(4):
        raw = _raw_for(_KINDS5, n, 50 + seed)
        _check_whole_draw(mod, _KINDS5, raw, ce, mc, seed, (n, ce, mc, seed),
                          n_invalid=seed % 3)
    _check_whole_draw(mod, _KINDS5, _raw_for(_KINDS5, n, 7), ce, mc, 9, "S=1", S=1)


def test_whole_draw_on_the_below_cases(mod) -> None:
    """The edge columns of tpe_below_cases (ties, all-equal columns, values
    on both bounds), every case whose kernels fit the fused entry."""
    used = 0
    for i, case in enumerate(tc.cases()):
        if len(case.raw) + 1 > _device.FUSED_MAX_BELOW:
            continue
        _check_whole_draw(mod, case.space, case.raw, case.consider_endpoints,
                          case.consider_magic_clip, i, case.name)
        used += 1
    assert used == len(tc.cases())


def test_candidates_reject_wrong_arrays(mod) -> None:
    space = {"x": FloatDistribution(-5.0, 5.0)}
    ns = _NumericalSpace.of(list(space.values()))
    table, valid = np.zeros((3, 1)), np.ones(3, dtype=bool)
    rows, w = np.arange(3, dtype=np.int64), _below_weights(3)
    u, q = np.full(2, 0.5), np.full((2, 1), 0.5)
    consts = (ns.adapted_lows, ns.adapted_highs, ns.kinds, ns.lows, ns.highs, ns.steps)
    mod.tpe_draw_candidates(table, valid, rows, w, u, q, *consts, False, True)
    with pytest.raises(RuntimeError, match="out of range"):
        mod.tpe_draw_candidates(table, valid, rows + 1, w, u, q, *consts, False, True)
    with pytest.raises(RuntimeError, match="weight"):
        mod.tpe_draw_candidates(table, valid, rows, w[:3], u, q, *consts, False, True)
    with pytest.raises(RuntimeError, match="dtype"):
        mod.tpe_draw_candidates(table, valid, rows.astype(np.int32), w, u, q, *consts,
                                False, True)
    with pytest.raises(RuntimeError, match="shape"):
        mod.tpe_draw_candidates(table, valid, rows, w, u, q[:, :0], *consts, False, True)
    with pytest.raises(RuntimeError, match="layout"):
        mod.tpe_draw_candidates(np.zeros((3, 2))[:, :1], valid, rows, w, u, q, *consts,
                                False, True)


# ---------------------------------------------------------------------------
# Arg-max
# ---------------------------------------------------------------------------


@pytest.mark.parametrize(
    "vals",
    [
        [1.0, 3.0, 3.0, 2.0],
        [-np.inf, -np.inf, -np.inf],
        [1.0, 5.0, np.nan, 9.0, np.nan],
        [np.nan],
        [-0.0, 0.0],
        [2.0],
        [-np.inf, np.inf, np.inf],
    ],
    ids=["ties", "all-ninf", "nan-middle", "nan-only", "zeros", "single", "inf-ties"],
)
def test_argmax_equals_numpy(mod, vals) -> None:
    v = np.asarray(vals, dtype=np.float64)
    assert mod.tpe_draw_argmax(v) == int(np.argmax(v))


# ---------------------------------------------------------------------------
# Binding
# ---------------------------------------------------------------------------


def test_bind_rejects_other_capsules(mod) -> None:
    from scipy.special import cython_special

    capi = cython_special.__pyx_capi__
    good = _device._draw_capsules()
    try:
        # The float variant of ndtr carries another signature string.
        assert mod.tpe_draw_bind(capi["__pyx_fuse_0ndtr"], good[1], good[2]) is False
        assert mod.tpe_draw_bound() is False
        assert mod.tpe_draw_bind(good[0], object(), good[2]) is False
        with pytest.raises(RuntimeError, match="not bound"):
            mod.tpe_draw_ppf(np.zeros(1), np.zeros(1), np.ones(1))
    finally:
        assert mod.tpe_draw_bind(*good) is True


# ---------------------------------------------------------------------------
# Stand-alone program
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_standalone_program(tmp_path, sanitize) -> None:
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "tpe_draw_check"
    flags = []
    if sanitize:
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
        # The runtimes go into the program itself (clang's default, asked of
        # gcc): a dynamic runtime refuses to start behind any preloaded library.
        version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        if "clang" not in version:
            flags += ["-static-libasan", "-static-libubsan"]
    subprocess.run(
        [cxx, "-std=c++17", "-O1" if sanitize else "-O2", "-Wall", "-Wextra", "-Werror", *flags,
         f"-I{_CSRC}", str(_CPP / "tpe_draw_check.cpp"), "-o", str(exe)],
        check=True,
    )
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "tpe_draw: ok" in run.stdout


# ---------------------------------------------------------------------------
# Sampler routing (the extension replaced by a recording stub)
# ---------------------------------------------------------------------------

_CONT4 = {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(4)}
_MIXED4 = tc.MIXED4


def _fake_acq(x_kde: np.ndarray) -> np.ndarray:
    return -np.sum(np.asarray(x_kde) ** 2, axis=1)


class _StubHistory:
    """Stands in for ``TpeDeviceHistory``: the host half of each entry runs
    (through the host module), the device half is ``_fake_acq``."""

    def __init__(self, core, dims: int) -> None:
        self._core = core

    def set_domain(self, *args) -> None: ...
    def append(self, block) -> None: ...
    def upload_sorted(self, cols) -> None: ...
    def insert_sorted_by_value(self, first_row, n_new) -> None: ...

    def fused_prepare(self, *args) -> None:
        self._core.log.append("fused_prepare")

    def fused_score(self, excl, n_above, x, xedges, bmu, bsig, bw, *rest):
        self._core.log.append("fused_score")
        self._core.x_kde.append(np.array(x))
        return _fake_acq(x)

    def score(self, sorted_cols, pos, n_above, logw, alow, ahigh, steps, n_choices,
              prior_weight, x, xedges, ce, mc, per_dim=False, **kwargs):
        self._core.log.append("score")
        return np.zeros(x.shape if per_dim else len(x))


class _StubHistoryWithDraw(_StubHistory):
    def fused_draw_score(self, excl, n_above, table, valid, below_rows, bw, u, q, alow, ahigh,
                         kinds, lows, highs, steps, logw, w_num, w_start, w_step, log_total,
                         prior_weight, ce, mc):
        self._core.log.append("fused_draw_score")
        x_raw, _, _, x_kde, _ = self._core.mod.tpe_draw_candidates(
            table, valid, below_rows, bw, u, q, alow, ahigh, kinds, lows, highs, steps, ce, mc
        )
        self._core.x_kde.append(x_kde)
        acq = _fake_acq(x_kde)
        return int(np.argmax(acq)), x_raw, acq


class _StubCore:
    def __init__(self, mod, with_draw: bool = True, bind_ok: bool = True) -> None:
        self.mod, self.log, self.x_kde = mod, [], []
        self._hist_cls = _StubHistoryWithDraw if with_draw else _StubHistory
        self._bind_ok = bind_ok

    def available(self) -> bool:
        return True

    def TpeDeviceHistory(self, dims: int):  # noqa: N802
        return self._hist_cls(self, dims)

    def tpe_below_kernels(self, *args):
        self.log.append("tpe_below_kernels")
        return _numpy_below_kernels(*args)

    def tpe_draw_bind(self, *capsules) -> bool:
        self.log.append("tpe_draw_bind")
        return self._bind_ok and self.mod.tpe_draw_bind(*capsules)


@pytest.fixture
def install(monkeypatch, mod):
    def _install(**kwargs) -> _StubCore:
        core = _StubCore(mod, **kwargs)
        monkeypatch.setattr(_hip, "get", lambda: core)
        monkeypatch.setattr(_hip, "is_available", lambda: True)
        monkeypatch.setattr(_device, "device_ready", lambda n_kernels: n_kernels >= 512)
        for name in ("OPTUNA_AMD_TPE_FUSED", "OPTUNA_AMD_TPE_NATIVE_BELOW",
                     "OPTUNA_AMD_TPE_NATIVE_DRAW"):
            monkeypatch.delenv(name, raising=False)
        return core

    return _install


def _steps(log: list) -> list:
    return [e for e in log if e != "tpe_draw_bind"]


def test_draw_route_taken_when_eligible(install) -> None:
    core = install()
    study = tc.seeded_study(1, _CONT4)
    for step in range(2):
        t = tc.suggest_all(study, _CONT4)
        study.tell(t, float(step))
    assert _steps(core.log) == ["fused_prepare", "fused_draw_score"] * 2
    assert core.log.count("tpe_draw_bind") == 1  # bound once per space
    assert core.x_kde[0].shape == (24, 4)


def test_env_switch_keeps_the_two_call_route(monkeypatch, install) -> None:
    core = install()
    monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_DRAW", "0")
    study = tc.seeded_study(1, _CONT4)
    tc.suggest_all(study, _CONT4)
    assert core.log == ["fused_prepare", "tpe_below_kernels", "fused_score"]
    monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_DRAW", "1")
    tc.suggest_all(study, _CONT4)
    assert _steps(core.log)[3:] == ["fused_prepare", "fused_draw_score"]


def test_failed_binding_keeps_the_two_call_route(monkeypatch, install) -> None:
    core = install(bind_ok=False)
    study = tc.seeded_study(1, _CONT4)
    tc.suggest_all(study, _CONT4)
    tc.suggest_all(study, _CONT4)
    assert _steps(core.log) == ["fused_prepare", "tpe_below_kernels", "fused_score"] * 2
    assert core.log.count("tpe_draw_bind") == 1
    # No capsules to hand over at all.
    core = install()
    monkeypatch.setattr(_device, "_draw_capsules", lambda: None)
    study = tc.seeded_study(1, _CONT4)
    tc.suggest_all(study, _CONT4)
    assert core.log == ["fused_prepare", "tpe_below_kernels", "fused_score"]


def test_extension_without_the_entry_keeps_the_two_call_route(install) -> None:
    core = install(with_draw=False)
    study = tc.seeded_study(1, _CONT4)
    tc.suggest_all(study, _CONT4)
    assert core.log == ["fused_prepare", "tpe_below_kernels", "fused_score"]


@pytest.mark.parametrize(
    "kwargs,expect",
    [
        (dict(weights=lambda n: np.linspace(0.5, 1.5, n)), ["fused_prepare", "fused_score"]),
        (dict(n_objectives=2), ["score"]),  # per-dim batch, unfused
    ],
    ids=["custom-weights", "per-dim"],
)
def test_ineligible_suggests_stay_where_they_are(install, kwargs, expect) -> None:
    core = install()
    study = tc.seeded_study(1, _CONT4, **kwargs)
    tc.suggest_all(study, _CONT4)
    assert sorted(set(core.log)) == sorted(expect)


def test_without_native_below_no_draw_route(monkeypatch, install) -> None:
    core = install()
    monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_BELOW", "0")
    study = tc.seeded_study(1, _CONT4)
    tc.suggest_all(study, _CONT4)
    assert core.log == ["fused_prepare", "fused_score"]


@pytest.mark.parametrize(
    "space,kwargs",
    [
        (_CONT4, {}),
        (_MIXED4, {}),
        (_MIXED4, dict(consider_endpoints=True, consider_magic_clip=False, prior_weight=0.3)),
    ],
    ids=["cont4", "mixed4", "mixed4-flags"],
)
def test_routes_agree(monkeypatch, install, space, kwargs) -> None:
    """Same parameters, same scoring inputs and the same RNG state after
    three suggests with the history growing in between."""
    runs = []
    for env in ("1", "0"):
        core = install()
        monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_DRAW", env)
        study = tc.seeded_study(3, space, **kwargs)
        params = []
        for step in range(3):
            t = tc.suggest_all(study, space)
            params.append(list(t.params.values()))
            study.tell(t, float(step))
        assert core.log.count("fused_draw_score") == (3 if env == "1" else 0)
        assert core.log.count("fused_score") == (0 if env == "1" else 3)
        runs.append((params, core.x_kde, study.sampler._rng.rng.get_state()))
    (p_on, x_on, s_on), (p_off, x_off, s_off) = runs
    assert p_on == p_off
    assert [type(v) for v in p_on[0]] == [type(v) for v in p_off[0]]
    for a, b in zip(x_on, x_off):
        _assert_same(a, b, "x_kde")
    assert s_on[0] == s_off[0] and s_on[2:] == s_off[2:]
    np.testing.assert_array_equal(s_on[1], s_off[1])
