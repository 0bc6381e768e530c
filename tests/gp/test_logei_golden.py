"""The host log-EI (``acqf.standard_logei``, ``acqf.logei``) and its autograd
derivatives against the mpmath golden points of ``tests/golden/gp_logei_edges.json``
(``scripts/gen_gp_logei_golden.py``), which depend on neither the host formula
nor the device kernel that mirrors it.

Tolerances are the project's: rtol 1e-8 / atol 1e-10 on a value, rtol 1e-6 /
atol 1e-8 on a derivative. Every session case of the file is admissible at these
tolerances by construction (the generator refuses a case whose expected values
move by a tenth of them under the rounding of ``mean`` and ``raw``).
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch

from optuna_amd._gp import acqf as acqf_mod
from optuna_amd._gp import gp as gp_mod


F_TOL = dict(rtol=1e-8, atol=1e-10)
G_TOL = dict(rtol=1e-6, atol=1e-8)

_GOLDEN_PATH = Path(__file__).resolve().parent.parent / "golden" / "gp_logei_edges.json"
_GOLDEN = json.loads(_GOLDEN_PATH.read_text())
_STANDARD = _GOLDEN["standard"]
_SESSION = _GOLDEN["session"]


def _col(key: str) -> np.ndarray:
    return np.array([row[key] for row in _STANDARD], dtype=np.float64)


def test_golden_file_covers_the_edges() -> None:
    z = _col("z")
    for point in (-1.0, -1.5, -0.5, 0.0, 1e-300, -1e-300, 3.0, 8.0, 40.0, -5.0, -20.0, -38.0,
                  -39.0, -100.0, -1e3, -1e4, -1e5, -1e6, -1e7, -1e8, -1e10):
        assert point in z
    for cut in (acqf_mod._TAIL_Z, acqf_mod._SERIES_Z):
        assert np.nextafter(cut, -np.inf) in z and np.nextafter(cut, np.inf) in z
    zs = np.array([c["z"] for c in _SESSION])
    clamped = np.array([c["raw"] < 0 for c in _SESSION])
    assert zs[clamped].min() <= -1e8 and zs[clamped].max() > 3.9
    assert (zs[~clamped] < acqf_mod._SERIES_Z).any() and (zs[~clamped] > 4.0).any()
    assert sum(c["cat_mask"] != 0 for c in _SESSION) >= 1


def test_standard_logei_value_matches_mpmath_golden() -> None:
    got = acqf_mod.standard_logei(torch.from_numpy(_col("z"))).numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, _col("log_h"), **F_TOL)


def test_standard_logei_derivative_matches_mpmath_golden() -> None:
    z = torch.from_numpy(_col("z")).requires_grad_(True)
    acqf_mod.standard_logei(z).sum().backward()
    got = z.grad.numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, _col("r_m"), **G_TOL)


def test_logei_variance_derivative_matches_mpmath_golden() -> None:
    """d/dvar of logei(mean=z, var, f0=0) at var = 1 is r_v / 2."""
    mean = torch.from_numpy(_col("z"))
    var = torch.ones_like(mean).requires_grad_(True)
    acqf_mod.logei(mean=mean, var=var, f0=0.0).sum().backward()
    got = var.grad.numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, 0.5 * _col("r_v"), **G_TOL)


def _host_session(case: dict) -> tuple[float, np.ndarray, float]:
    """(f, grad, raw) of ``acqf.logei`` over the posterior of ``case``, by autograd."""
    X = torch.tensor(case["X"], dtype=torch.float64)
    eta = torch.tensor(case["eta"], dtype=torch.float64)
    alpha = torch.tensor(case["alpha"], dtype=torch.float64)
    cinv = torch.tensor(case["cinv"], dtype=torch.float64)
    cat = [d for d in range(case["D"]) if (case["cat_mask"] >> d) & 1]
    x = torch.tensor(case["x"], dtype=torch.float64).requires_grad_(True)
    sqd = (x.unsqueeze(-2) - X).square()
    if cat:
        sqd[..., cat] = (sqd[..., cat] > 0.0).double()
    k = gp_mod.matern52_of_sqdist((sqd * eta).sum(-1)) * case["scale"]
    mean = torch.linalg.vecdot(k, alpha)
    raw = case["scale"] - torch.linalg.vecdot(k, cinv.matmul(k))
    f = acqf_mod.logei(mean=mean, var=raw.clamp_min(0.0) + case["stab"], f0=case["threshold"])
    f.backward()
    return float(f.detach()), x.grad.numpy(), float(raw.detach())


@pytest.mark.parametrize("case", _SESSION, ids=[c["name"] for c in _SESSION])
def test_host_logei_matches_mpmath_golden_session(case: dict) -> None:
    assert case["N"] in (1, 2, 3) and case["D"] in (1, 2, 3)
    f, grad, raw = _host_session(case)
    assert (raw < 0) == (case["raw"] < 0)
    assert np.isfinite(f) and np.isfinite(grad).all()
    np.testing.assert_allclose(f, case["f"], **F_TOL)
    np.testing.assert_allclose(grad, np.array(case["grad"]), **G_TOL)
    for d in range(case["D"]):
        if (case["cat_mask"] >> d) & 1:
            assert grad[d] == 0.0 and case["grad"][d] == 0.0


def test_golden_file_is_what_the_generator_writes() -> None:
    import importlib.util

    if importlib.util.find_spec("mpmath") is None:
        return  # the committed values stand on their own; nothing to regenerate with

    script = _GOLDEN_PATH.parent.parent.parent / "scripts" / "gen_gp_logei_golden.py"
    spec = importlib.util.spec_from_file_location("gen_gp_logei_golden", script)
    assert spec is not None and spec.loader is not None
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import mpmath

    names = {c["name"]: c for c in _SESSION}
    with mpmath.workdps(mod.DPS):
        # A handful of rows of each section, to equal float64.
        for row in _STANDARD[::5]:
            assert mod.standard_row(row["z"]) == row
        for case in mod.CASES[::6]:
            assert json.loads(json.dumps(mod.session_case(*case))) == names[case[0]]
    assert [c[0] for c in mod.CASES] == [c["name"] for c in _SESSION]
    assert mod.SERIES_Z == acqf_mod._SERIES_Z
