"""Host-side pieces of the fused TPE suggest: when the sampler takes it, how the
exclusion list is built, the lazily maintained host sorted index, and the
device's default-weight formula (transcribed in numpy)."""
from __future__ import annotations

import math

import numpy as np
import pytest

import optuna_amd
from optuna_amd.distributions import CategoricalDistribution, FloatDistribution
from optuna_amd.samplers import TPESampler
from optuna_amd.samplers._tpe import _device
from optuna_amd.samplers._tpe._history import _SpaceCache
from optuna_amd.samplers._tpe.parzen import _ParzenEstimator
from optuna_amd.samplers._tpe.sampler import default_weights
from optuna_amd.testing.trials import _create_frozen_trial


_SPACE = {"a": FloatDistribution(-5.0, 5.0), "b": FloatDistribution(-5.0, 5.0)}
_OK = dict(per_dim=False, n_liar=0, default_estimator=True, rows_ascending=True,
           n_excl=25, n_below_kernels=26)


# ---------------------------------------------------------------------------
# Eligibility
# ---------------------------------------------------------------------------


def test_fused_eligible_default(monkeypatch) -> None:
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    assert _device.fused_eligible(_SPACE, **_OK)


@pytest.mark.parametrize(
    "change",
    [
        dict(per_dim=True),
        dict(n_liar=1),
        dict(default_estimator=False),
        dict(rows_ascending=False),
        dict(n_excl=1025),
        dict(n_below_kernels=1025),
    ],
    ids=lambda c: next(iter(c)),
)
def test_fused_ineligible(monkeypatch, change) -> None:
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    assert not _device.fused_eligible(_SPACE, **{**_OK, **change})


def test_fused_limits_inclusive(monkeypatch) -> None:
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    assert _device.fused_eligible(_SPACE, **{**_OK, "n_excl": 1024, "n_below_kernels": 1024})


def test_fused_ineligible_categorical_and_env(monkeypatch) -> None:
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    space = dict(_SPACE, c=CategoricalDistribution(["u", "v"]))
    assert not _device.fused_eligible(space, **_OK)
    assert not _device.fused_eligible({}, **_OK)
    monkeypatch.setenv("OPTUNA_AMD_TPE_FUSED", "0")
    assert not _device.fused_eligible(_SPACE, **_OK)
    monkeypatch.setenv("OPTUNA_AMD_TPE_FUSED", "1")
    assert _device.fused_eligible(_SPACE, **_OK)


# ---------------------------------------------------------------------------
# Sampler routing (device calls replaced by a recorder)
# ---------------------------------------------------------------------------


def _study(seed: int, space=None, n: int = 600, **sampler_kwargs):
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    space = space or {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(4)}
    rng = np.random.RandomState(seed)
    study = optuna_amd.create_study(
        sampler=TPESampler(seed=seed, n_startup_trials=5, **sampler_kwargs)
    )
    trials = []
    for _ in range(n):
        params = {}
        for name, dist in space.items():
            if isinstance(dist, CategoricalDistribution):
                params[name] = dist.choices[rng.randint(len(dist.choices))]
            else:
                params[name] = float(rng.uniform(dist.low, dist.high))
        value = float(sum(v**2 for v in params.values() if isinstance(v, float)))
        trials.append(optuna_amd.create_trial(params=params, distributions=space, value=value))
    study.add_trials(trials)
    return study, space


def _suggest(study, space):
    t = study.ask()
    for name, dist in space.items():
        if isinstance(dist, CategoricalDistribution):
            t.suggest_categorical(name, dist.choices)
        else:
            t.suggest_float(name, dist.low, dist.high)
    return t


@pytest.fixture
def recorder(monkeypatch):
    """Pretend a device is there; record how the sampler calls it."""
    calls: list[dict] = []

    def fake(cache, sel, weights, samples, ce, mc, prior_weight=1.0, extras=None,
             per_dim=False, fused=None):
        calls.append(dict(cache=cache, sel=sel, weights=weights, samples=samples,
                          fused=fused, extras=extras))
        S = len(fused.x_raw) if fused is not None else len(next(iter(samples.values())))
        return np.zeros(S)

    monkeypatch.setattr(_device, "device_ready", lambda n_kernels: n_kernels >= 512)
    monkeypatch.setattr(_device, "score_above_resident", fake)
    coeff = {"n": 0}
    orig = _ParzenEstimator._precompute_logpdf_coefficients

    def counting(self):
        coeff["n"] += 1
        return orig(self)

    monkeypatch.setattr(_ParzenEstimator, "_precompute_logpdf_coefficients", counting)
    return calls, coeff


def test_sampler_takes_fused_path(monkeypatch, recorder) -> None:
    calls, coeff = recorder
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    study, space = _study(1)
    _suggest(study, space)
    assert len(calls) == 1
    req = calls[0]["fused"]
    assert req is not None and calls[0]["weights"] is None and calls[0]["sel"] is None
    assert req.n_above == 600 - len(req.below_rows) == 575
    assert req.x_raw.shape == (24, 4)
    assert req.below_mus.shape == req.below_sigmas.shape == (26, 4)
    assert req.below_weights.shape == (26,)
    # The below estimator only drew candidates: nothing forced its scoring
    # coefficients or its log_pdf.
    assert coeff["n"] == 0


def test_sampler_env_forces_unfused(monkeypatch, recorder) -> None:
    calls, coeff = recorder
    monkeypatch.setenv("OPTUNA_AMD_TPE_FUSED", "0")
    study, space = _study(1)
    _suggest(study, space)
    assert len(calls) == 1 and calls[0]["fused"] is None
    assert len(calls[0]["sel"]) == 575 and len(calls[0]["weights"]) == 576
    assert coeff["n"] == 1  # below log_pdf on the host


def test_sampler_custom_weights_are_uploaded(monkeypatch, recorder) -> None:
    calls, _ = recorder
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    study, space = _study(1, weights=lambda n: np.linspace(0.5, 1.5, n))
    _suggest(study, space)
    w = calls[0]["weights"]
    assert calls[0]["fused"] is not None and w.shape == (576,)
    expect = np.append(np.linspace(0.5, 1.5, 575), [1.0])
    np.testing.assert_array_equal(w, expect / expect.sum())


def test_sampler_categorical_space_stays_unfused(monkeypatch, recorder) -> None:
    calls, _ = recorder
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    space = {"x": FloatDistribution(-5.0, 5.0), "k": CategoricalDistribution(["a", "b", "c"])}
    study, space = _study(2, space=space)
    _suggest(study, space)
    assert len(calls) == 1 and calls[0]["fused"] is None


def test_sampler_same_candidates_either_way(monkeypatch, recorder) -> None:
    """The fused path draws the candidates with the same RNG calls."""
    calls, _ = recorder
    monkeypatch.setenv("OPTUNA_AMD_TPE_FUSED", "0")
    study, space = _study(3)
    _suggest(study, space)
    monkeypatch.setenv("OPTUNA_AMD_TPE_FUSED", "1")
    study, space = _study(3)
    _suggest(study, space)
    unfused, fused = calls
    x = np.column_stack([unfused["samples"][n] for n in space])
    np.testing.assert_array_equal(fused["fused"].x_raw, x)


# ---------------------------------------------------------------------------
# Exclusion list and lazy host index
# ---------------------------------------------------------------------------


def _trials(block: np.ndarray, offset: int):
    names = list(_SPACE)
    return [
        _create_frozen_trial(
            number=offset + j, values=(0.0,),
            params={n: float(v) for n, v in zip(names, row) if not np.isnan(v)},
            distributions={n: _SPACE[n] for n, v in zip(names, row) if not np.isnan(v)},
        )
        for j, row in enumerate(block)
    ]


def _random_blocks(seed: int) -> list[np.ndarray]:
    r = np.random.RandomState(seed)
    blocks = []
    for size in [70, 1, 1, 5, 1, 130, 1, 1, 1, 3, 64, 1]:
        b = np.round(r.uniform(-5, 5, (size, 2)), 1)  # coarse grid: many ties
        b[r.rand(size) < 0.1, r.randint(2)] = np.nan
        blocks.append(b)
    return blocks


def test_excluded_rows() -> None:
    cache = _SpaceCache(_SPACE)
    n = 0
    for b in _random_blocks(0):
        cache.append(_trials(b, n))
        n += len(b)
    invalid = np.nonzero(~cache.valid)[0]
    assert len(invalid) > 0 and cache.n_invalid == len(invalid)
    assert cache.n_valid == n - len(invalid)
    valid = np.nonzero(cache.valid)[0]
    below = valid[[40, 3, 17, 200, 5]]  # any order
    excl = cache.excluded_rows(below)
    assert excl.dtype == np.int32
    np.testing.assert_array_equal(excl, np.union1d(below, invalid))
    # Above rows are the ascending complement; k = row - lower_bound(excl, row).
    above = np.setdiff1d(np.arange(n), excl)
    np.testing.assert_array_equal(above - np.searchsorted(excl, above), np.arange(len(above)))
    # No invalid rows: just the sorted below rows.
    clean = _SpaceCache(_SPACE)
    clean.append(_trials(np.zeros((10, 2)), 0))
    np.testing.assert_array_equal(clean.excluded_rows(np.array([7, 2])), [2, 7])


def test_lazy_index_equals_eager() -> None:
    eager, lazy = _SpaceCache(_SPACE), _SpaceCache(_SPACE)
    n = 0
    for b in _random_blocks(1):
        eager.append(_trials(b, n))
        eager._n_sorted  # noqa: B018 - reading it brings the index up to date
        lazy.append(_trials(b, n))
        assert lazy.n_valid == eager._n_sorted_host
        n += len(b)
    assert lazy._n_sorted_host == 0 and len(lazy._pending) > 0  # nothing flushed yet
    assert lazy._n_sorted == eager._n_sorted == lazy.n_valid
    for c in range(2):
        np.testing.assert_array_equal(lazy.sorted_rows[c], eager.sorted_rows[c])
        np.testing.assert_array_equal(lazy.sorted_vals[c], eager.sorted_vals[c])
        # And both equal a stable argsort over the valid rows.
        valid = np.nonzero(lazy.valid)[0]
        order = valid[np.argsort(lazy.params[valid, c], kind="stable")]
        np.testing.assert_array_equal(lazy.sorted_rows[c], order)


# ---------------------------------------------------------------------------
# Default weights as the device writes them
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("prior_weight", [1.0, 0.5, 0.0])
def test_device_weight_formula(prior_weight) -> None:
    for n in list(range(0, 80)) + [575, 9975, 99975]:
        w = _device.expand_weight_ramp(n, prior_weight)
        ref = default_weights(n)
        assert w.shape == (n + 1,)
        if n:
            np.testing.assert_array_max_ulp(w[:n], ref, maxulp=1)
            assert w[n] == prior_weight
            total = np.append(ref, [prior_weight]).sum()
            if total > 0:
                log_total = _device.default_weight_ramp(n, prior_weight)[3]
                assert abs(log_total - math.log(total)) < 1e-12
        else:
            assert w[0] == 1.0 and _device.default_weight_ramp(0, prior_weight)[3] == 0.0


# ---------------------------------------------------------------------------
# Seed of the sampler-level GPU equivalence test
# ---------------------------------------------------------------------------


def test_gpu_equivalence_seed_has_no_near_ties(monkeypatch) -> None:
    """tests/gpu/test_tpe_fused_suggest.py compares fused and unfused suggests
    bit for bit and may skip a step whose unfused top-two acquisition gap is
    below 1e-6; its seed must not lean on that allowance."""
    seed = 0  # SAMPLER_SEED of the GPU test
    study, space = _study(seed)
    gaps: list[float] = []
    orig = TPESampler._compare

    def spy(samples, vals):
        top = np.sort(np.asarray(vals))[-2:]
        gaps.append(float(top[1] - top[0]))
        return orig(samples, vals)

    monkeypatch.setattr(TPESampler, "_compare", staticmethod(spy))
    for _ in range(16):
        t = _suggest(study, space)
        study.tell(t, float(sum(v**2 for v in t.params.values())))
    assert len(gaps) == 16
    print("top-two gaps:", gaps)
    assert min(gaps) >= 1e-6
