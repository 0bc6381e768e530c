"""Pins the independent TPE reference (``optuna_amd.testing.tpe_reference``)
against the host estimator without a GPU, so that a later device-vs-reference
mismatch can only be the device's."""
from __future__ import annotations

import numpy as np
import pytest

from optuna_amd.samplers._tpe.parzen import _ParzenEstimator, _ParzenEstimatorParameters
from optuna_amd.testing.tpe_reference import edge_cases


_CASES = list(edge_cases())


def _host(case, per_dim: bool) -> np.ndarray:
    w = np.asarray(case.weights_raw, dtype=np.float64)
    params = _ParzenEstimatorParameters(
        case.prior_weight, case.magic_clip, case.consider_endpoints, lambda n: w[:n], True
    )
    obs = {name: case.obs_raw[:, c] for c, name in enumerate(case.names)}
    mpe = _ParzenEstimator(obs, case.space, params)
    samples = {name: case.x_raw[:, c] for c, name in enumerate(case.names)}
    return mpe.log_pdf_per_dim(samples) if per_dim else mpe.log_pdf(samples)


def test_edge_case_names_are_unique_and_seeded() -> None:
    names = [c.name for c in _CASES]
    assert len(set(names)) == len(names)
    again = list(edge_cases())
    for a, b in zip(_CASES, again):
        np.testing.assert_array_equal(a.obs_raw, b.obs_raw)
        np.testing.assert_array_equal(a.x_raw, b.x_raw)


@pytest.mark.parametrize("per_dim", [False, True], ids=["joint", "perdim"])
@pytest.mark.parametrize("case", _CASES, ids=lambda c: c.name)
def test_reference_matches_host_estimator(case, per_dim) -> None:
    ref = case.reference(per_dim=per_dim)
    with np.errstate(divide="ignore"):
        host = _host(case, per_dim)
    assert ref.shape == host.shape
    assert not np.isnan(ref).any() and not np.isnan(host).any()
    np.testing.assert_array_equal(np.isneginf(ref), np.isneginf(host))
    finite = np.isfinite(host)
    assert np.isfinite(ref[finite]).all()
    # Also covers the magic_clip=False lattices, whose documented guard is the
    # looser 1e-10.
    np.testing.assert_allclose(ref[finite], host[finite], rtol=1e-12, atol=0.0)
    if case.expect_all_neginf and not per_dim:
        assert np.isneginf(ref).all()


def test_magic_clip_off_cases_are_tie_free_lattices() -> None:
    """The clip-off cases stay inside the documented limit: N <= 64 and every
    neighbour gap >= range / (4 N), so sigma never collapses to 1e-12."""
    off = [c for c in _CASES if not c.magic_clip]
    assert off
    for case in off:
        n = len(case.obs_raw)
        assert n <= 64
        for d in range(case.obs_raw.shape[1]):
            gaps = np.diff(np.sort(case.obs_raw[:, d]))
            assert gaps.min() >= 10.0 / (4 * n)


@pytest.mark.parametrize("kind", ["positions", "growth"])
def test_space_cache_sorted_rows_match_stable_argsort(kind) -> None:
    """The incrementally maintained per-dim index equals a stable argsort over
    the valid rows after every append."""
    from optuna_amd.distributions import FloatDistribution
    from optuna_amd.samplers._tpe._history import _SpaceCache
    from optuna_amd.testing.tpe_reference import sorted_index_batches
    from optuna_amd.testing.trials import _create_frozen_trial

    space = {"a": FloatDistribution(-5.0, 5.0), "b": FloatDistribution(-5.0, 5.0)}
    cache = _SpaceCache(space)
    n_rows = 0
    for block in sorted_index_batches(kind):
        trials = [
            _create_frozen_trial(
                number=n_rows + j, values=(0.0,),
                params={n: float(v) for n, v in zip(space, row) if not np.isnan(v)},
                distributions={n: space[n] for n, v in zip(space, row) if not np.isnan(v)},
            )
            for j, row in enumerate(block)
        ]
        cache.append(trials)
        n_rows += len(block)
        valid = np.nonzero(cache.valid)[0]
        np.testing.assert_array_equal(valid, np.nonzero(~np.isnan(np.vstack(
            sorted_index_batches(kind))[:n_rows]).any(axis=1))[0])
        for c in range(2):
            want = valid[np.argsort(cache.params[valid, c], kind="stable")]
            np.testing.assert_array_equal(cache.sorted_rows[c], want)
