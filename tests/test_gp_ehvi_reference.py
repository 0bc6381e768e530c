"""The numpy LogEHVI reference of ``optuna_amd.testing.gp_reference`` against
``acqf.logehvi`` and torch autograd on CPU tensors.

The reference is what the fused device kernel is specified by (value, df/dmean
and df/dvar per objective), so it has to agree with the torch formulation the
sampler used so far. Inputs are continuous random draws: no ``y - lo`` lands
exactly on EPS or on a box interval, where torch's gradient splits in halves
and is not the target.
"""
from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch

from optuna_amd._gp import acqf as acqf_mod
from optuna_amd.testing.gp_reference import EPS, logehvi_reference


def _torch_side(mean, var, eps, lo, iv):
    """(f, df/dmean, df/dvar) the way LogEHVI.eval_acqf composes them."""
    mean_t = torch.from_numpy(mean).requires_grad_(True)
    var_t = torch.from_numpy(var).requires_grad_(True)
    y_post = mean_t[None, :] + torch.sqrt(var_t)[None, :] * torch.from_numpy(eps)
    f = acqf_mod.logehvi(y_post, torch.from_numpy(lo), torch.from_numpy(iv))
    f.backward()
    return f.item(), mean_t.grad.numpy(), var_t.grad.numpy()


def _draw(rng: np.random.RandomState, M: int, Q: int, J: int):
    mean = rng.randn(M)
    var = rng.uniform(0.01, 1.0, M)
    eps = rng.randn(Q, M)
    lo = rng.randn(J, M)
    # Narrow and wide boxes: some terms end on the interval, some on EPS, some
    # in between.
    iv = rng.uniform(0.05, 2.0, (J, M))
    return mean, var, eps, lo, iv


@pytest.mark.parametrize(
    "M, Q, J", list(itertools.product((2, 3, 4), (1, 5), (1, 7)))
)
def test_reference_matches_torch(M: int, Q: int, J: int) -> None:
    rng = np.random.RandomState(1000 + 100 * M + 10 * Q + J)
    seen = set()
    for _ in range(4):
        mean, var, eps, lo, iv = _draw(rng, M, Q, J)
        diff = (mean + np.sqrt(var) * eps)[:, None, :] - lo[None, :, :]
        assert not np.any(diff == EPS) and not np.any(diff == iv[None])
        seen |= {"eps"} if (diff < EPS).any() else set()
        seen |= {"iv"} if (diff > iv[None]).any() else set()
        seen |= {"free"} if ((diff > EPS) & (diff < iv[None])).any() else set()

        f, wm, wv = logehvi_reference(mean, np.sqrt(var), eps, lo, iv)
        f_t, gm_t, gv_t = _torch_side(mean, var, eps, lo, iv)
        np.testing.assert_allclose(f, f_t, rtol=1e-12, atol=0.0)
        np.testing.assert_allclose(wm, gm_t, rtol=1e-9, atol=0.0)
        np.testing.assert_allclose(wv, gv_t, rtol=1e-9, atol=0.0)
    # At the larger shape the four draws take every branch of the double clamp.
    if (Q, J) == (5, 7):
        assert seen == {"eps", "iv", "free"}


@pytest.mark.parametrize("M", (2, 3, 4))
def test_every_term_on_the_eps_clamp(M: int) -> None:
    """A candidate dominated in every sample: all d sit on EPS, f is finite
    (M log EPS + log J) and no gradient passes, on either side."""
    rng = np.random.RandomState(7 + M)
    Q, J = 5, 7
    mean, var, eps, lo, iv = _draw(rng, M, Q, J)
    mean = mean - 50.0  # far below every lower bound
    f, wm, wv = logehvi_reference(mean, np.sqrt(var), eps, lo, iv)
    f_t, gm_t, gv_t = _torch_side(mean, var, eps, lo, iv)
    assert np.isfinite(f)
    np.testing.assert_allclose(f, M * np.log(EPS) + np.log(J), rtol=1e-12)
    np.testing.assert_allclose(f, f_t, rtol=1e-12, atol=0.0)
    for grad in (wm, wv, gm_t, gv_t):
        assert grad.shape == (M,) and np.all(grad == 0.0)
