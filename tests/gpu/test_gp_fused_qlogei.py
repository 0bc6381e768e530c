"""``GpQLogEiSession`` against the torch formulation of ``sample_joint_posterior``
+ ``qLogEI.eval_acqf``, at the fused sessions' tolerances. The synthetic cases fit
no GP: targets peak at 0.75, running points beside the peak, candidates around it,
so that a draw beats the best fantasy for 10% to 90% of the (candidate, draw) pairs."""
from functools import partial

import numpy as np
import pytest
import torch

from optuna_amd import _hip
from optuna_amd._gp import acqf as acqf_mod, gp as gp_mod, prior, search_space as gp_ss
from optuna_amd.distributions import FloatDistribution


pytestmark = pytest.mark.gpu

F_TOL = dict(rtol=1e-8, atol=1e-10)
G_TOL = dict(rtol=1e-6, atol=1e-8)
STAB = EPS = 1e-12


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    assert c is not None and c.available(), "the HIP extension must run here: no fallback"
    return c


class _Problem:
    """One synthetic GP, R running points in ``xr_box``, Q draws, categorical columns ``cat``."""

    def __init__(self, N, D, R, Q, seed, xr_box=(0.35, 0.75), cat=(), dev="cuda"):
        g = torch.Generator().manual_seed(seed)
        rand = partial(torch.rand, generator=g, dtype=torch.float64)
        self.cat, self.seed = list(cat), seed
        X, Xr = rand(N, D), xr_box[0] + (xr_box[1] - xr_box[0]) * rand(R, D)
        X[:, self.cat], Xr[:, self.cat] = (3.0 * X[:, self.cat]).floor(), rand(R, len(cat)).round()
        self.X, self.Xr = X.to(dev), Xr.to(dev)
        self.eta = ((0.5 + rand(D)) * (2.0 / D)).to(dev)
        self.scale = float(0.5 + rand(1))
        cont = [d for d in range(D) if d not in cat]
        y = torch.exp(-4.0 * (X[:, cont] - 0.75).square().mean(-1)) + 0.05 * rand(N)
        C = self.kernel(self.X, self.X) + 0.1 * torch.eye(N, dtype=torch.float64, device=dev)
        self.cinv = torch.linalg.inv(C).contiguous()
        self.alpha = self.cinv.mv(y.to(dev)).contiguous()
        self.threshold = float(y.min()) - 1.0
        # ConditionalGPRegressor.__init__ on these tensors.
        k_r = self.kernel(self.Xr, self.X)
        self.Vr_t = k_r.matmul(self.cinv).contiguous()  # (R, N): column-major (N, R)
        mean_r = k_r.mv(self.alpha)
        cov_rr = self.kernel(self.Xr, self.Xr) - self.Vr_t.matmul(k_r.T)
        cov_rr.diagonal().clamp_min_(0.0).add_(STAB)
        self.L = torch.linalg.cholesky(cov_rr).contiguous()
        normals = torch.randn(Q, R + 1, generator=g, dtype=torch.float64).to(dev)
        self.z = normals[:, -1].contiguous()
        self.fantasy = mean_r + normals[:, :-1].matmul(self.L.T)
        self.W = gp_mod._solve_cholesky(self.L, (self.fantasy - mean_r).T).contiguous()
        self.m = (self.fantasy.amax(-1) - self.threshold).clamp_min(EPS)

    def kernel(self, a, b):
        # scale * Matern-5/2, Hamming term on the categorical columns; differentiable in a
        sq = (a.unsqueeze(-2) - b.unsqueeze(-3)).square()
        if self.cat:
            sq = sq.clone()
            sq[..., self.cat] = (sq.detach()[..., self.cat] > 0.0).double()
        return gp_mod.matern52_of_sqdist((sq * self.eta).sum(-1)) * self.scale

    def reference(self, x_np):
        # f, gradient (autograd), share of active pairs, smallest unclamped variance.
        x = torch.from_numpy(x_np).to(self.X.device).requires_grad_(True)
        K = self.kernel(x, self.X)
        raw = self.scale - torch.linalg.vecdot(K, K.matmul(self.cinv))
        c = self.kernel(x, self.Xr) - K.matmul(self.Vr_t.T)
        V = gp_mod._solve_cholesky(self.L, c, left=False)
        cv_raw = raw.clamp_min(0.0) + STAB - torch.linalg.vecdot(V, c)
        samples = (torch.linalg.vecdot(K, self.alpha).unsqueeze(-1) + c.matmul(self.W)
                   + cv_raw.clamp_min(0.0).sqrt().unsqueeze(-1) * self.z)
        y_post = torch.cat([self.fantasy.expand(len(x), -1, -1), samples.unsqueeze(-1)], dim=-1)
        f = acqf_mod._mean_max_log_utility((y_post - self.threshold).clamp_min(EPS).log())
        f.sum().backward()
        share = float((samples.detach() - self.threshold > self.m).double().mean())
        slack = float(torch.minimum(raw, cv_raw).min().detach())
        return f.detach().cpu().numpy(), x.grad.cpu().numpy(), share, slack


# Each N, D, R, Q, B once; then chunks of two, B = 10 at N = 513 (S = 3), a categorical column.
CASES = [
    (1, 1, 1, 1, 1, {}, {}),
    (255, 64, 64, 128, 7, {}, {}),
    (256, 3, 2, 130, 7, {}, {}),
    (257, 64, 1, 128, 1, {}, {}),
    (513, 6, 64, 130, 7, {}, {}),
    (257, 5, 2, 128, 13, dict(xr_box=(0.5, 0.95)), dict(scratch_budget_bytes=2 * 3 * 257 * 8)),
    (513, 4, 2, 128, 10, dict(xr_box=(0.5, 0.95)), {}),
    (257, 4, 2, 128, 7, dict(cat=(1,)), {}),
]


@pytest.mark.parametrize("N, D, R, Q, B, problem_kw, session_kw", CASES)
def test_session_matches_torch(core, N, D, R, Q, B, problem_kw, session_kw) -> None:
    prob = _Problem(N, D, R, Q, seed=7 * N + D + R + Q, **problem_kw)
    torch.cuda.synchronize()
    x = 0.55 + 0.4 * np.random.RandomState(prob.seed + 17).rand(B, D)
    x[:, prob.cat] = np.floor(5.0 * x[:, prob.cat] - 2.0)  # 0, 1, 2
    want_f, want_g, share, slack = prob.reference(x)
    assert np.isfinite(want_f).all() and np.isfinite(want_g).all() and slack > 0.0
    assert Q == 1 or (0.1 <= share <= 0.9 and np.abs(want_g).max() > 1e-3)
    tensors = (prob.X, prob.alpha, prob.cinv, prob.eta, prob.Xr, prob.Vr_t, prob.L, prob.W)
    ptrs = [t.data_ptr() for t in tensors]
    sess = core.GpQLogEiSession(
        *ptrs[:4], N, D, prob.scale, STAB, prob.threshold, *ptrs[4:], R, prob.z.cpu().numpy(),
        prob.m.cpu().numpy(), cat_mask=sum(1 << d for d in prob.cat), **session_kw,
    )
    f0, g0 = sess.eval(x, with_grad=False)
    f1, g1 = sess.eval(x, with_grad=True)
    assert np.asarray(g0).size == 0 and np.asarray(g1).shape == (B, D)
    np.testing.assert_allclose(f0, want_f, **F_TOL)
    np.testing.assert_array_equal(f1, f0)
    np.testing.assert_allclose(g1, want_g, **G_TOL)
    assert np.all(np.asarray(g1)[:, prob.cat] == 0.0)
    assert sess.n_chunks(B) == (7 if session_kw else 1)
    assert sess.n_splits(B) == -(-N // 256) and sess.n_splits(2048) == 1
    f, g = sess.eval(np.empty((0, D)), with_grad=True)  # no candidates: empty arrays
    assert np.asarray(f).shape == (0,) and np.asarray(g).shape == (0, D)


@pytest.mark.parametrize("R, Q", [(0, 4), (65, 4), (2, 1025)])
def test_out_of_range_shapes_are_refused(core, R: int, Q: int) -> None:
    with pytest.raises(RuntimeError, match="GpQLogEiSession"):  # before any pointer is read
        core.GpQLogEiSession(*[0] * 4, 8, 2, 1.0, STAB, 0.0, *[0] * 4, R, np.zeros(Q), np.zeros(Q))


def test_qlogei_entry_points_use_the_session(core, monkeypatch) -> None:
    monkeypatch.setattr(gp_mod.GPRegressor, "_DEVICE_FIT_MIN_OBS", 32)
    n, d, rng = 40, 3, np.random.RandomState(3)
    X = rng.rand(n, d)
    # Noisy targets and running points off the optimum, for a mixed active share.
    y = -np.sum(np.square(X - 0.6), axis=1) + 0.1 * rng.randn(n)
    y = (y - y.mean()) / y.std()
    gpr = gp_mod.fit_kernel_params(X, y, np.zeros(d, bool), prior.default_log_prior, 1e-6, False)
    space = gp_ss.SearchSpace({f"x{i}": FloatDistribution(0.0, 1.0) for i in range(d)})
    running, t = 0.3 * rng.rand(2, d), float(np.median(y))
    acqf = acqf_mod.qLogEI(gpr, space, t, running, n_qmc_samples=128, qmc_seed=5)
    assert isinstance(acqf._fused_session(), core.GpQLogEiSession)
    base, cands = acqf_mod.BaseAcquisitionFunc, rng.rand(24, d)
    with torch.no_grad():  # active share of the candidates whose gradient is compared
        draws = acqf._cond_gpr.sample_joint_posterior(acqf._up(cands[:8]), return_fantasy=False)
        best = acqf._cond_gpr.get_fantasy_samples().amax(-1).clamp_min(acqf._threshold + EPS)
        share = (draws > best).double().mean(-1).cpu().numpy()
    assert 0.1 <= share[:6].mean() <= 0.9 and 0.1 <= share[7] <= 0.9
    f0, r0 = acqf.eval_acqf_no_grad(cands), base.eval_acqf_no_grad(acqf, cands)
    np.testing.assert_allclose(f0, r0, **F_TOL)
    fb, gb = acqf.eval_acqf_batched_with_grad(cands[:6].copy())
    rf, rg = base.eval_acqf_batched_with_grad(acqf, cands[:6].copy())
    np.testing.assert_allclose(fb, rf, **F_TOL)
    np.testing.assert_allclose(gb, rg, **G_TOL)
    f1, g1 = acqf.eval_acqf_with_grad(cands[7].copy())
    r1, rg1 = base.eval_acqf_with_grad(acqf, cands[7].copy())
    assert isinstance(f1, float) and g1.shape == (d,)
    np.testing.assert_allclose(f1, r1, **F_TOL)
    np.testing.assert_allclose(g1, rg1, **G_TOL)
