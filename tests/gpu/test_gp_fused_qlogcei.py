"""``GpQLogCeiSession`` against the torch formulation of ``qLogCEI.eval_acqf`` over
``sample_joint_posterior``, at the fused sessions' tolerances. The synthetic cases
fit no GP: G = [objective] + C GPs as in ``test_gp_fused_qlogei.py`` (seeds
``seed + 101 g``) share the running points, and constraint c's threshold is a
quantile of its own candidate-column samples over the batch."""
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
TAU = 1e-2


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    assert c is not None and c.available(), "the HIP extension must run here: no fallback"
    return c


class _Gp:
    """One synthetic GP, Q fantasy draws at R running points: ``Xr``, or its own in ``xr_box``."""

    def __init__(self, N, D, R, Q, seed, Xr=None, xr_box=(0.35, 0.75), cat=(), dev="cuda"):
        g = torch.Generator().manual_seed(seed)
        rand = partial(torch.rand, generator=g, dtype=torch.float64)
        self.cat = list(cat)
        X, own = rand(N, D), xr_box[0] + (xr_box[1] - xr_box[0]) * rand(R, D)
        X[:, self.cat] = (3.0 * X[:, self.cat]).floor()
        own[:, self.cat] = rand(R, len(cat)).round()
        self.X, self.Xr = X.to(dev), (own.to(dev) if Xr is None else Xr)
        self.eta = ((0.5 + rand(D)) * (2.0 / D)).to(dev)
        self.scale = float(0.5 + rand(1))
        cont = [d for d in range(D) if d not in cat]
        y = torch.exp(-4.0 * (X[:, cont] - 0.75).square().mean(-1)) + 0.05 * rand(N)
        C = self.kernel(self.X, self.X) + 0.1 * torch.eye(N, dtype=torch.float64, device=dev)
        self.cinv = torch.linalg.inv(C).contiguous()
        self.alpha = self.cinv.mv(y.to(dev)).contiguous()
        self.threshold = float(y.min()) - 1.0  # of the objective; a constraint gets a quantile
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

    def kernel(self, a, b):
        # scale * Matern-5/2, Hamming term on the categorical columns; differentiable in a
        sq = (a.unsqueeze(-2) - b.unsqueeze(-3)).square()
        if self.cat:
            sq = sq.clone()
            sq[..., self.cat] = (sq.detach()[..., self.cat] > 0.0).double()
        return gp_mod.matern52_of_sqdist((sq * self.eta).sum(-1)) * self.scale

    def y_post(self, x):
        # sample_joint_posterior: (B, Q, R + 1), and the smallest unclamped variance
        K = self.kernel(x, self.X)
        raw = self.scale - torch.linalg.vecdot(K, K.matmul(self.cinv))
        c = self.kernel(x, self.Xr) - K.matmul(self.Vr_t.T)
        V = gp_mod._solve_cholesky(self.L, c, left=False)
        cv_raw = raw.clamp_min(0.0) + STAB - torch.linalg.vecdot(V, c)
        samples = (torch.linalg.vecdot(K, self.alpha).unsqueeze(-1) + c.matmul(self.W)
                   + cv_raw.clamp_min(0.0).sqrt().unsqueeze(-1) * self.z)
        y = torch.cat([self.fantasy.expand(len(x), -1, -1), samples.unsqueeze(-1)], dim=-1)
        return y, float(torch.minimum(raw, cv_raw).min().detach())


def _reference(gps, n_obj, x_np, quantile):
    """Thresholds, F (Q), then per use of the constraint terms (with, without): f and
    its autograd gradient; the share of pairs the candidate column wins; the slack."""
    x = torch.from_numpy(x_np).to(gps[0].X.device).requires_grad_(True)
    posts = [gp.y_post(x) for gp in gps]
    thr = [gp.threshold if g < n_obj else float(y.detach()[..., -1].quantile(quantile))
           for g, (gp, (y, _)) in enumerate(zip(gps, posts))]
    terms = [(y - t).clamp_min(EPS).log() if g < n_obj
             else torch.nn.functional.logsigmoid((y - t) / TAU)
             for g, ((y, _), t) in enumerate(zip(posts, thr))]
    out = []
    for kept in (terms, terms[:n_obj] or [torch.zeros_like(terms[0])]):
        f = acqf_mod._mean_max_log_utility(sum(kept))
        grad = torch.zeros_like(x)  # no term at all: f = 0
        if f.requires_grad:
            (grad,) = torch.autograd.grad(f.sum(), x, retain_graph=True)
        out.append((f.detach().cpu().numpy(), grad.cpu().numpy()))
    u = sum(terms).detach()
    F = u[0, :, :-1].amax(-1)
    share = float((u[..., -1] > F).double().mean())
    return thr, F.cpu().numpy(), out[0], out[1], share, min(s for _, s in posts)


# N, D, R, Q, B, C, quantile, then the problem's and the session's extras. S = 3 at N = 513;
# the budget of the sixth row holds two candidates' K / MP / V and per-draw buffers. With 16
# constraints and running points off the candidates some fantasy is nearly always infeasible
# and the candidate column wins 96% of the pairs at any quantile: that row moves them closer.
CASES = [
    (1, 1, 1, 1, 1, 1, 0.5, {}, {}),
    (255, 64, 64, 128, 7, 1, 0.3, {}, {}),
    (256, 3, 2, 130, 7, 16, 0.05, dict(xr_box=(0.5, 0.95)), {}),
    (257, 64, 1, 128, 1, 2, 0.5, {}, {}),
    (513, 6, 64, 130, 7, 3, 0.3, {}, {}),
    (257, 5, 2, 128, 13, 2, 0.5, dict(xr_box=(0.5, 0.95)),
     dict(scratch_budget_bytes=2 * 3 * (3 * 257 + 128 + 30) * 8)),
    (257, 4, 2, 128, 7, 0, None, {}, {}),
    (257, 4, 2, 128, 7, 2, 0.5, dict(cat=(1,)), {}),
    (256, 3, 2, 130, 7, 2, 0.5, dict(has_objective=False), {}),
]


def _problem(N, D, R, Q, C, has_objective=True, dev="cuda", **gp_kw):
    seed, n_obj = 7 * N + D + R + Q, 1 if has_objective else 0
    gps = [_Gp(N, D, R, Q, seed, dev=dev, **gp_kw)]  # its running points are everyone's
    gps += [_Gp(N, D, R, Q, seed + 101 * i, gps[0].Xr, dev=dev, **gp_kw)
            for i in range(1, n_obj + C)]
    return gps, n_obj, seed


def _candidates(B, D, seed, cat):
    x = 0.55 + 0.4 * np.random.RandomState(seed + 17).rand(B, D)
    x[:, list(cat)] = np.floor(5.0 * x[:, list(cat)] - 2.0)  # 0, 1, 2
    return x


@pytest.mark.parametrize("N, D, R, Q, B, C, quantile, problem_kw, session_kw", CASES)
def test_session_matches_torch(core, N, D, R, Q, B, C, quantile, problem_kw, session_kw) -> None:
    gps, n_obj, seed = _problem(N, D, R, Q, C, **problem_kw)
    cat = list(problem_kw.get("cat", ()))
    x = _candidates(B, D, seed, cat)
    thr, F, (want_f, want_g), (bare_f, bare_g), share, slack = _reference(gps, n_obj, x, quantile)
    torch.cuda.synchronize()
    assert np.isfinite(want_f).all() and np.isfinite(want_g).all()
    if Q > 1:  # the case exercises both sides of the max, no clamp and its constraints
        assert 0.1 <= share <= 0.9 and slack > 0.0
        assert C == 0 or np.abs(want_f - bare_f).min() > 1e-4
        assert C == 0 or np.abs(want_g - bare_g).max(axis=1).min() > 1e-4
    names = ("X", "alpha", "cinv", "eta", "Vr_t", "L", "W")
    ptrs = {n: [getattr(gp, n).data_ptr() for gp in gps] for n in names}
    sess = core.GpQLogCeiSession(
        ptrs["X"], ptrs["alpha"], ptrs["cinv"], ptrs["eta"], [gp.scale for gp in gps], N, D,
        STAB, gps[0].Xr.data_ptr(), ptrs["Vr_t"], ptrs["L"], ptrs["W"], R, thr, n_obj == 1,
        torch.stack([gp.z for gp in gps], dim=-1).cpu().numpy(), F, TAU,
        cat_mask=sum(1 << d for d in cat), **session_kw,
    )
    f0, g0 = sess.eval(x, with_grad=False)
    f1, g1 = sess.eval(x, with_grad=True)
    assert np.asarray(g0).size == 0 and np.asarray(g1).shape == (B, D)
    np.testing.assert_allclose(f0, want_f, **F_TOL)
    np.testing.assert_array_equal(f1, f0)
    np.testing.assert_allclose(g1, want_g, **G_TOL)
    assert np.all(np.asarray(g1)[:, cat] == 0.0)
    chunks = 7 if session_kw else 1
    assert sess.n_chunks(B, False) == chunks and sess.n_chunks(B, True) == chunks
    assert sess.n_splits(B) == -(-N // 256) and sess.n_splits(2048) == 1
    f, g = sess.eval(np.empty((0, D)), with_grad=True)  # no candidates: empty arrays
    assert np.asarray(f).shape == (0,) and np.asarray(g).shape == (0, D)


@pytest.mark.parametrize("R, Q, G, has_objective", [
    (0, 4, 2, True), (65, 4, 2, True), (2, 1025, 2, True), (2, 4, 18, True), (2, 4, 17, False),
    (2, 4, 0, False),
])
def test_out_of_range_shapes_are_refused(core, R, Q, G, has_objective) -> None:
    with pytest.raises(RuntimeError, match="GpQLogCeiSession"):  # before any pointer is read
        core.GpQLogCeiSession(
            *[[0] * G] * 4, [1.0] * G, 8, 2, STAB, 0, *[[0] * G] * 3, R, [0.0] * G,
            has_objective, np.zeros((Q, G)), np.zeros(Q), TAU,
        )


@pytest.mark.parametrize("threshold", [None, -np.inf])
def test_qlogcei_entry_points_use_the_session(core, monkeypatch, threshold) -> None:
    monkeypatch.setattr(gp_mod.GPRegressor, "_DEVICE_FIT_MIN_OBS", 32)
    n, d, rng = 40, 3, np.random.RandomState(3)
    X = rng.rand(n, d)
    ys = [-np.sum(np.square(X - c), axis=1) + 0.1 * rng.randn(n) for c in (0.6, 0.4, 0.7)]
    ys = [(y - y.mean()) / y.std() for y in ys]
    gprs = [
        gp_mod.fit_kernel_params(X, y, np.zeros(d, bool), prior.default_log_prior, 1e-6, False)
        for y in ys
    ]
    space = gp_ss.SearchSpace({f"x{i}": FloatDistribution(0.0, 1.0) for i in range(d)})
    running = 0.3 * rng.rand(2, d)
    t = float(np.median(ys[0])) if threshold is None else threshold
    acqf = acqf_mod.qLogCEI(
        gprs[0], space, t, running, n_qmc_samples=128, qmc_seed=5,
        constraints_gpr_list=gprs[1:], constraints_threshold_list=[0.0, -0.3],
    )
    assert isinstance(acqf._fused_session(), core.GpQLogCeiSession)
    base, cands = acqf_mod.BaseAcquisitionFunc, rng.rand(24, d)
    f0, r0 = acqf.eval_acqf_no_grad(cands), base.eval_acqf_no_grad(acqf, cands)
    np.testing.assert_allclose(f0, r0, **F_TOL)
    fb, gb = acqf.eval_acqf_batched_with_grad(cands[:6].copy())
    rf, rg = base.eval_acqf_batched_with_grad(acqf, cands[:6].copy())
    assert np.abs(rg).max() > 1e-3
    np.testing.assert_allclose(fb, rf, **F_TOL)
    np.testing.assert_allclose(gb, rg, **G_TOL)
    f1, g1 = acqf.eval_acqf_with_grad(cands[7].copy())
    r1, rg1 = base.eval_acqf_with_grad(acqf, cands[7].copy())
    assert isinstance(f1, float) and g1.shape == (d,)
    np.testing.assert_allclose(f1, r1, **F_TOL)
    np.testing.assert_allclose(g1, rg1, **G_TOL)
