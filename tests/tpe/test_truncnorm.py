"""Golden tests: host truncnorm vs scipy.stats.truncnorm (and later the HIP K3 lib)."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
from scipy import stats

from optuna_amd.samplers._tpe import _truncnorm_np as tn


RANGES = [
    (-2.0, 2.0),
    (0.5, 3.0),
    (-3.0, -0.5),
    (-10.0, -9.0),
    (9.0, 10.0),
    (-30.0, -29.0),
    (29.0, 30.0),
    (-1e10, 1e10),
]


@pytest.mark.parametrize("a,b", RANGES)
def test_ppf_matches_scipy(a: float, b: float) -> None:
    q = np.linspace(1e-10, 1 - 1e-10, 101)
    ours = tn.ppf(q, np.full_like(q, a), np.full_like(q, b))
    ref = stats.truncnorm.ppf(q, a, b)
    np.testing.assert_allclose(ours, ref, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("a,b", RANGES)
def test_logpdf_matches_scipy(a: float, b: float) -> None:
    x = np.linspace(a, b, 51)
    ours = tn.logpdf(x, np.full_like(x, a), np.full_like(x, b))
    ref = stats.truncnorm.logpdf(x, a, b)
    np.testing.assert_allclose(ours, ref, rtol=1e-10, atol=1e-10)


def test_logpdf_outside_support() -> None:
    assert tn.logpdf(np.array([5.0]), np.array([-1.0]), np.array([1.0]))[0] == -np.inf


def test_log_gauss_mass_extreme_tails() -> None:
    # Far left tail: mass is tiny but must stay finite in log space.
    a = np.array([-40.0, 35.0])
    b = np.array([-39.0, 36.0])
    out = tn._log_gauss_mass(a, b)
    assert np.all(np.isfinite(out))
    ref = stats.truncnorm.logpdf(0, a, b)  # just check ours is finite/consistent sign
    assert np.all(out < 0)


def test_ppf_endpoints() -> None:
    assert tn.ppf(np.array([0.0]), np.array([-2.0]), np.array([3.0]))[0] == -2.0
    assert tn.ppf(np.array([1.0]), np.array([-2.0]), np.array([3.0]))[0] == 3.0


def test_rvs_seeded_within_bounds() -> None:
    rng = np.random.RandomState(0)
    a = np.full(1000, -1.0)
    b = np.full(1000, 2.0)
    draws = tn.rvs(a, b, loc=1.0, scale=0.5, random_state=rng)
    assert np.all(draws >= 1.0 - 0.5) and np.all(draws <= 1.0 + 1.0)
    rng2 = np.random.RandomState(0)
    draws2 = tn.rvs(a, b, loc=1.0, scale=0.5, random_state=rng2)
    np.testing.assert_array_equal(draws, draws2)


# ---- mpmath golden points (tests/golden/truncnorm_edges.json) -----------------------

_GOLDEN_PATH = Path(__file__).resolve().parent.parent / "golden" / "truncnorm_edges.json"
_GOLDEN = json.loads(_GOLDEN_PATH.read_text())


def _col(section: str, key: str) -> np.ndarray:
    return np.array([p[key] for p in _GOLDEN[section]], dtype=np.float64)


def test_log_gauss_mass_matches_mpmath_golden() -> None:
    with np.errstate(all="ignore"):
        ours = tn._log_gauss_mass(_col("log_gauss_mass", "a"), _col("log_gauss_mass", "b"))
    np.testing.assert_allclose(ours, _col("log_gauss_mass", "expected"), rtol=1e-10, atol=1e-12)


def test_ppf_matches_mpmath_golden() -> None:
    with np.errstate(all="ignore"):
        ours = tn.ppf(_col("ppf", "q"), _col("ppf", "a"), _col("ppf", "b"))
    np.testing.assert_allclose(ours, _col("ppf", "expected"), rtol=1e-8, atol=1e-10)


def test_logpdf_matches_mpmath_golden() -> None:
    with np.errstate(all="ignore"):
        ours = tn.logpdf(
            _col("logpdf", "x"), _col("logpdf", "a"), _col("logpdf", "b"),
            _col("logpdf", "loc"), _col("logpdf", "scale"),
        )
    expected = _col("logpdf", "expected")
    assert np.isneginf(expected).sum() >= 10  # the one-ulp-outside points are present
    np.testing.assert_allclose(ours, expected, rtol=1e-9, atol=1e-10)


def test_golden_file_is_what_the_generator_writes() -> None:
    import importlib.util

    if importlib.util.find_spec("mpmath") is None:
        return  # the committed values stand on their own; nothing to regenerate with

    script = _GOLDEN_PATH.parent.parent.parent / "scripts" / "gen_truncnorm_golden.py"
    spec = importlib.util.spec_from_file_location("gen_truncnorm_golden", script)
    assert spec is not None and spec.loader is not None
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert json.loads(json.dumps(mod.generate())) == _GOLDEN
