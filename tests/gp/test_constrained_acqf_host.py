"""On a CPU GP the constrained acquisitions have no fused session, and their
numpy entry points are exactly the ones of ``BaseAcquisitionFunc``."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from optuna_amd._gp import acqf as acqf_mod
from optuna_amd._gp import gp, prior
from optuna_amd._gp import search_space as gp_ss
from optuna_amd.distributions import FloatDistribution


D = 3


@pytest.fixture(scope="module")
def fitted():
    rng = np.random.RandomState(0)
    X = rng.rand(30, D)
    Y = np.stack([-np.sum(np.square(X), axis=1), -np.sum(np.square(X - 1.0), axis=1)], axis=1)
    Y = (Y - Y.mean(0)) / Y.std(0)
    cons = np.stack([X[:, 0] + X[:, 1] - 1.25, 0.2 - X[:, 2]], axis=1)
    feasible = (cons <= 0).all(axis=1)
    assert 5 < feasible.sum() < 25
    c_std = (-cons - (-cons).mean(0)) / (-cons).std(0)
    gprs = [
        gp.fit_kernel_params(
            X, col, np.zeros(D, dtype=bool), prior.default_log_prior, 1e-6, False
        )
        for col in (Y[:, 0], Y[:, 1], c_std[:, 0], c_std[:, 1])
    ]
    assert all(g.device.type == "cpu" for g in gprs)
    return dict(
        Y=Y, feasible=feasible, objectives=gprs[:2],
        common=dict(
            search_space=gp_ss.SearchSpace(
                {f"x{i}": FloatDistribution(0.0, 1.0) for i in range(D)}
            ),
            constraints_gpr_list=gprs[2:],
            constraints_threshold_list=(-(-cons).mean(0) / (-cons).std(0)).tolist(),
        ),
    )


def _make(fitted, kind: str):
    if kind.startswith("LogCEI"):
        best = float(fitted["Y"][fitted["feasible"], 0].max())
        threshold = -np.inf if kind == "LogCEI no feasible" else best
        return acqf_mod.LogCEI(
            gpr=fitted["objectives"][0], threshold=threshold, **fitted["common"]
        )
    y_feasible = (
        None
        if kind == "LogCEHVI no feasible"
        else torch.from_numpy(fitted["Y"][fitted["feasible"]])
    )
    return acqf_mod.LogCEHVI(
        gpr_list=fitted["objectives"], Y_feasible=y_feasible, n_qmc_samples=32, qmc_seed=5,
        **fitted["common"],
    )


@pytest.mark.parametrize(
    "kind", ["LogCEI", "LogCEI no feasible", "LogCEHVI", "LogCEHVI no feasible"]
)
def test_cpu_gp_keeps_the_torch_entry_points(fitted, kind: str) -> None:
    acqf = _make(fitted, kind)
    assert acqf._fused_session() is None
    base = acqf_mod.BaseAcquisitionFunc
    cands = np.random.RandomState(1).rand(8, D)

    np.testing.assert_array_equal(
        acqf.eval_acqf_no_grad(cands), base.eval_acqf_no_grad(acqf, cands)
    )
    one = acqf.eval_acqf_no_grad(cands[3])
    assert np.ndim(one) == 0
    np.testing.assert_array_equal(one, base.eval_acqf_no_grad(acqf, cands[3]))

    fb, gb = acqf.eval_acqf_batched_with_grad(cands[:4].copy())
    rf, rg = base.eval_acqf_batched_with_grad(acqf, cands[:4].copy())
    assert fb.shape == (4,) and gb.shape == (4, D) and np.abs(rg).max() > 0
    np.testing.assert_array_equal(fb, rf)
    np.testing.assert_array_equal(gb, rg)

    f1, g1 = acqf.eval_acqf_with_grad(cands[5].copy())
    r1, rg1 = base.eval_acqf_with_grad(acqf, cands[5].copy())
    assert isinstance(f1, float) and g1.shape == (D,)
    assert f1 == r1
    np.testing.assert_array_equal(g1, rg1)
