"""Device truncnorm library vs mpmath golden points.

``tests/golden/truncnorm_edges.json`` holds 50-digit mpmath values rounded to
float64 (``scripts/gen_truncnorm_golden.py``): deep-tail intervals that reach
the ``ndtri_exp`` asymptotic branch (a < -37.2), q in {0, 1}, narrow central
intervals and one-ulp-outside points. Tolerances are the project's existing
device bounds.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

from optuna_amd import _hip


pytestmark = pytest.mark.gpu

_GOLDEN = json.loads(
    (Path(__file__).resolve().parent.parent / "golden" / "truncnorm_edges.json").read_text()
)


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


def _col(section: str, key: str) -> np.ndarray:
    return np.array([p[key] for p in _GOLDEN[section]], dtype=np.float64)


def _report(section: str, got: np.ndarray, expected: np.ndarray) -> None:
    with np.errstate(all="ignore"):
        err = np.abs(got - expected)
        rel = err / np.abs(expected)
    ok = np.isfinite(expected) & (expected != 0)
    i = int(np.argmax(np.where(ok, rel, 0.0)))
    print(f"{section}: worst rel {rel[i]:.3e} at {_GOLDEN[section][i]} got {got[i]!r}")


def test_log_gauss_mass_device_matches_golden(core) -> None:
    got = core.log_gauss_mass(_col("log_gauss_mass", "a"), _col("log_gauss_mass", "b"))
    expected = _col("log_gauss_mass", "expected")
    _report("log_gauss_mass", got, expected)
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got, expected, rtol=1e-10, atol=1e-12)


def test_ppf_device_matches_golden(core) -> None:
    got = core.truncnorm_ppf(_col("ppf", "q"), _col("ppf", "a"), _col("ppf", "b"))
    expected = _col("ppf", "expected")
    _report("ppf", got, expected)
    assert not np.isnan(got).any()
    assert (got >= _col("ppf", "a")).all() and (got <= _col("ppf", "b")).all()
    np.testing.assert_allclose(got, expected, rtol=1e-8, atol=1e-10)


def test_logpdf_device_matches_golden(core) -> None:
    got = core.truncnorm_logpdf(
        _col("logpdf", "x"), _col("logpdf", "a"), _col("logpdf", "b"),
        _col("logpdf", "loc"), _col("logpdf", "scale"),
    )
    expected = _col("logpdf", "expected")
    _report("logpdf", got, expected)
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(expected))
    np.testing.assert_allclose(got, expected, rtol=1e-9, atol=1e-10)
