"""The fused LogEHVI session (``GpLogEhviSession``) against the torch
formulation of ``optuna_amd/_gp/acqf.py``.

Both sides do the same fp64 math in a different summation order, so the
tolerances are the ones of ``test_fused_logei_matches_torch_path``: rtol 1e-8 /
atol 1e-10 on the value, rtol 1e-6 / atol 1e-8 on the gradient.

The synthetic cases fit no GP: the session only sees raw device pointers, so a
random ``X``, an explicit inverse of an SPD matrix and a random ``alpha`` are a
complete input. Shapes are the smallest that reach another code path: N on both
sides of the 256-thread block, D = 1 and the maximum 64, every supported M, one
QMC sample and the sampler's 128, box counts of 1, one LDS tile and one more,
one candidate and a few, and a scratch budget lowered until the candidates are
evaluated in several chunks.
"""
from __future__ import annotations

import itertools
import warnings

import numpy as np
import pytest

import optuna_amd
from optuna_amd import _hip
from optuna_amd.distributions import FloatDistribution


pytestmark = pytest.mark.gpu

F_TOL = dict(rtol=1e-8, atol=1e-10)
G_TOL = dict(rtol=1e-6, atol=1e-8)
STAB = 1e-12


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


def _matern(x, X, eta, scale):
    """scale * Matern-5/2 of the ARD distance, (B, N); differentiable in x."""
    from optuna_amd._gp import gp as gp_mod

    r2 = ((x.unsqueeze(-2) - X.unsqueeze(-3)).square() * eta).sum(-1)
    return gp_mod.matern52_of_sqdist(r2) * scale


class _Problem:
    """M synthetic GPs over one X, plus QMC normals and boxes, on the device."""

    def __init__(self, N, D, M, Q, J, seed, lo_shift=0.0, jitter=0.1):
        import torch

        dev = torch.device("cuda")
        g = torch.Generator().manual_seed(seed)

        def rand(*shape):
            return torch.rand(*shape, generator=g, dtype=torch.float64)

        def randn(*shape):
            return torch.randn(*shape, generator=g, dtype=torch.float64)

        self.N, self.D, self.M, self.Q, self.J = N, D, M, Q, J
        self.X = rand(N, D).to(dev)
        self.eta = [((0.5 + rand(D)) * (2.0 / D)).to(dev) for _ in range(M)]
        self.scale = [float(0.5 + rand(1)) for _ in range(M)]
        # 1 / sqrt(N) keeps the posterior mean of order one, among the boxes.
        self.alpha = [(randn(N) / np.sqrt(N)).to(dev) for _ in range(M)]
        self.cinv = []
        for m in range(M):
            # The GP's own covariance plus jitter: SPD, and the posterior
            # variance it implies is positive. A small `jitter` with a large
            # identity instead drives the variance onto its clamp.
            C = _matern(self.X, self.X, self.eta[m], self.scale[m])
            C = C + jitter * torch.eye(N, dtype=torch.float64, device=dev)
            self.cinv.append(torch.linalg.inv(C).contiguous())
        self.eps = randn(Q, M).to(dev)
        self.lo = (0.7 * randn(J, M) + lo_shift).to(dev)
        self.iv = (0.05 + 1.95 * rand(J, M)).to(dev)
        if J > 2:
            self.iv[J // 2, 0] = float("inf")  # unbounded boxes occur in practice
        self._seed = seed
        torch.cuda.synchronize()

    def candidates(self, B):
        return np.random.RandomState(self._seed + 17).rand(B, self.D)

    def session(self, core, **kw):
        return core.GpLogEhviSession(
            [self.X.data_ptr()] * self.M,
            [a.data_ptr() for a in self.alpha],
            [c.data_ptr() for c in self.cinv],
            [e.data_ptr() for e in self.eta],
            self.scale, self.N, self.D, STAB,
            self.eps.cpu().numpy(), self.lo.cpu().numpy(), self.iv.cpu().numpy(), **kw,
        )

    def torch_value_and_grad(self, x_np):
        """LogEHVI.eval_acqf's formulas on these tensors, with autograd."""
        import torch

        from optuna_amd._gp import acqf as acqf_mod

        x = torch.from_numpy(x_np).to(self.X.device).requires_grad_(True)
        cols = []
        for m in range(self.M):
            K = _matern(x, self.X, self.eta[m], self.scale[m])
            mean = torch.linalg.vecdot(K, self.alpha[m])
            var = (self.scale[m] - torch.linalg.vecdot(K, K.matmul(self.cinv[m]))).clamp_min(0.0)
            sd = torch.sqrt(var + STAB)
            cols.append(mean[..., None] + sd[..., None] * self.eps[..., m])
        f = acqf_mod.logehvi(torch.stack(cols, dim=-1), self.lo, self.iv)
        f.sum().backward()
        return f.detach().cpu().numpy(), x.grad.cpu().numpy()


def _check(core, prob: _Problem, B: int, **session_kw):
    x = prob.candidates(B)
    want_f, want_g = prob.torch_value_and_grad(x)
    sess = prob.session(core, **session_kw)
    f0, g0 = sess.eval(x, with_grad=False)
    f1, g1 = sess.eval(x, with_grad=True)
    label = f"N={prob.N} D={prob.D} M={prob.M} Q={prob.Q} J={prob.J} B={B}"
    assert np.asarray(f0).shape == (B,) and np.asarray(g0).size == 0
    assert np.asarray(g1).shape == (B, prob.D)
    assert np.isfinite(want_f).all() and np.isfinite(want_g).all(), label
    np.testing.assert_allclose(f0, want_f, err_msg=label, **F_TOL)
    np.testing.assert_allclose(f1, want_f, err_msg=label, **F_TOL)
    np.testing.assert_allclose(g1, want_g, err_msg=label, **G_TOL)
    return sess, np.asarray(f1), np.asarray(g1)


@pytest.mark.parametrize("N, D", [(1, 1), (1, 64), (257, 1), (257, 64)])
@pytest.mark.parametrize("M", [2, 3, 4])
def test_session_matches_torch_on_synthetic_inputs(core, M: int, N: int, D: int) -> None:
    tile = core.GP_EHVI_BOX_TILE
    moved = 0
    for Q, J, B in itertools.product((1, 128), (1, tile, tile + 1), (1, 7)):
        prob = _Problem(N, D, M, Q, J, seed=1000 * M + 10 * N + D + Q + J)
        _, _, g = _check(core, prob, B)
        moved += int(np.abs(g).max() > 1e-6)
    # The gradient check is not a comparison of zeros.
    assert moved >= 6


@pytest.mark.parametrize("M", [2, 3, 4])
def test_lowered_scratch_budget_forces_candidate_chunks(core, M: int) -> None:
    N, D, B = 257, 5, 13
    prob = _Problem(N, D, M, Q=5, J=9, seed=50 + M)
    budget = 2 * M * 3 * N * 8  # two candidates with the gradient, 2 M without
    sess, _, _ = _check(core, prob, B, scratch_budget_bytes=budget)
    assert sess.n_chunks(B, True) == 7
    assert sess.n_chunks(B, False) == (B + 2 * M - 1) // (2 * M) >= 2
    # Less than one candidate's worth still evaluates, one candidate at a time.
    sess, _, _ = _check(core, prob, 3, scratch_budget_bytes=8)
    assert sess.n_chunks(3, True) == 3
    # The default budget keeps a pre-sample batch at 5000 observations and 4
    # objectives far from gigabytes.
    assert core.GP_EHVI_SCRATCH_BUDGET_BYTES <= 512 << 20


@pytest.mark.parametrize("M", [2, 4])
def test_clamped_variance_passes_no_gradient(core, M: int) -> None:
    """An inverse that overshoots drives scale - K Cinv K below zero: the
    variance sits on its clamp, and like autograd the closed form sends
    nothing through it."""
    import torch

    prob = _Problem(64, 3, M, Q=5, J=9, seed=90 + M)
    for m in range(M):
        prob.cinv[m] = (50.0 * torch.eye(64, dtype=torch.float64, device="cuda")).contiguous()
    torch.cuda.synchronize()
    x = prob.candidates(4)
    K = _matern(torch.from_numpy(x).cuda(), prob.X, prob.eta[0], prob.scale[0])
    assert bool((prob.scale[0] - 50.0 * (K * K).sum(-1) < 0).all())
    _check(core, prob, 4)


@pytest.mark.parametrize("M", [2, 3, 4])
def test_all_dominated_candidate(core, M: int) -> None:
    """Every box lies far above every sample: each term sits on the EPS clamp.
    f is finite (M log EPS + log J) and the gradient is exactly zero."""
    tile = core.GP_EHVI_BOX_TILE
    prob = _Problem(257, 6, M, Q=128, J=tile + 1, seed=70 + M, lo_shift=1e3)
    _, f, g = _check(core, prob, 7)
    np.testing.assert_allclose(f, M * np.log(1e-12) + np.log(tile + 1), rtol=1e-12)
    assert np.all(g == 0.0)


def _sphere_study_data(n: int, seed: int):
    """n observations in [0, 1]^3 whose three (maximised, standardised)
    objectives lie near a sphere front, so most of them are non-dominated."""
    rng = np.random.RandomState(seed)
    X = rng.rand(n, 3)
    a, b = X[:, 0] * np.pi / 2, X[:, 1] * np.pi / 2
    r = 1.0 + 0.2 * (X[:, 2] - 0.5) + 0.02 * rng.randn(n)
    Y = -np.stack([r * np.cos(a) * np.cos(b), r * np.sin(a) * np.cos(b), r * np.sin(b)], axis=1)
    return X, (Y - Y.mean(0)) / Y.std(0)


def test_logehvi_entry_points_use_the_session(core, monkeypatch) -> None:
    import torch

    from optuna_amd._gp import acqf as acqf_mod
    from optuna_amd._gp import gp as gp_mod
    from optuna_amd._gp import prior
    from optuna_amd._gp import search_space as gp_ss

    monkeypatch.setattr(gp_mod.GPRegressor, "_DEVICE_FIT_MIN_OBS", 100)
    n, d, M = 200, 3, 3
    X, Y = _sphere_study_data(n, 21)
    gprs = [
        gp_mod.fit_kernel_params(
            X, Y[:, i], np.zeros(d, dtype=bool), prior.default_log_prior, 1e-6, False
        )
        for i in range(M)
    ]
    assert all(g.device.type == "cuda" and g._cov_Y_Y_inv is not None for g in gprs)
    space = gp_ss.SearchSpace({f"x{i}": FloatDistribution(0.0, 1.0) for i in range(d)})

    def make():
        return acqf_mod.LogEHVI(
            gpr_list=gprs, search_space=space, Y_train=torch.from_numpy(Y),
            n_qmc_samples=128, qmc_seed=5,
        )

    acqf = make()
    assert acqf._box_lower.shape[0] > core.GP_EHVI_BOX_TILE
    assert acqf._fused_session() is not None

    base = acqf_mod.BaseAcquisitionFunc
    cands = np.random.RandomState(22).rand(24, d)
    np.testing.assert_allclose(
        acqf.eval_acqf_no_grad(cands), base.eval_acqf_no_grad(acqf, cands), **F_TOL
    )
    one = acqf.eval_acqf_no_grad(cands[3])
    assert np.ndim(one) == 0
    np.testing.assert_allclose(one, base.eval_acqf_no_grad(acqf, cands[3]), **F_TOL)

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

    monkeypatch.setenv("OPTUNA_AMD_GP_FUSED_EHVI", "0")
    forced = make()
    assert forced._fused_session() is None
    np.testing.assert_allclose(
        forced.eval_acqf_no_grad(cands), base.eval_acqf_no_grad(acqf, cands), **F_TOL
    )


def test_workspace_shared_with_logei_session_in_both_orders(core) -> None:
    """The LogEI session and the new one lay their regions over the same
    workspace. Whatever the other left behind, and in whichever order the
    workspace grew, each call returns the same bits."""
    small = _Problem(1, 1, 2, Q=1, J=1, seed=301)
    large = _Problem(257, 7, 3, Q=128, J=core.GP_EHVI_BOX_TILE + 1, seed=302)

    def ehvi(prob, B, grad):
        x = prob.candidates(B)

        def run():
            f, g = prob.session(core).eval(x, with_grad=grad)
            return np.concatenate([np.asarray(f).ravel(), np.asarray(g).ravel()])

        return run

    def logei(prob, B, grad):
        x = prob.candidates(B)

        def run():
            sess = core.GpLogEiSession(
                prob.X.data_ptr(), prob.alpha[0].data_ptr(), prob.cinv[0].data_ptr(),
                prob.eta[0].data_ptr(), prob.N, prob.D, prob.scale[0], STAB, 0.1,
            )
            f, g = sess.eval(x, with_grad=grad)
            return np.concatenate([np.asarray(f).ravel(), np.asarray(g).ravel()])

        return run

    calls = {
        "ehvi small": ehvi(small, 1, True),
        "ehvi large": ehvi(large, 7, True),
        "ehvi large no grad": ehvi(large, 7, False),
        "logei small": logei(small, 1, True),
        "logei large": logei(large, 9, True),
    }
    order_a = ["logei small", "ehvi small", "logei large", "ehvi large", "ehvi large no grad"]
    order_b = ["ehvi large", "logei small", "ehvi large no grad", "ehvi small", "logei large",
               "ehvi small", "logei small", "ehvi large"]
    assert set(order_a) == set(order_b) == set(calls)
    got_b = [(name, calls[name]()) for name in order_b]
    got_a = {name: calls[name]() for name in order_a}
    for name, got in got_b:
        assert np.isfinite(got).all(), name
        np.testing.assert_array_equal(got, got_a[name], err_msg=name)


def test_gp_sampler_uses_fused_logehvi(core, monkeypatch) -> None:
    """A two-objective GPSampler study on a device-sized history must run its
    acquisition through the fused session."""
    from optuna_amd._gp import acqf as acqf_mod
    from optuna_amd._gp import gp as gp_mod

    monkeypatch.setattr(gp_mod.GPRegressor, "_DEVICE_FIT_MIN_OBS", 100)
    counts = {"fused": 0}
    orig = acqf_mod.LogEHVI._fused_session

    def spy(self):
        out = orig(self)
        if out is not None:
            counts["fused"] += 1
        return out

    monkeypatch.setattr(acqf_mod.LogEHVI, "_fused_session", spy)
    warnings.simplefilter("ignore")
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    rng = np.random.RandomState(4)
    names = [f"x{i}" for i in range(4)]
    dists = {n: FloatDistribution(0.0, 1.0) for n in names}
    study = optuna_amd.create_study(
        directions=["minimize", "minimize"],
        sampler=optuna_amd.samplers.GPSampler(seed=0, n_startup_trials=5),
    )
    pm = rng.rand(300, 4)

    def values(x):
        return float(np.sum(np.square(x))), float(np.sum(np.square(np.asarray(x) - 1.0)))

    study.add_trials(
        [
            optuna_amd.create_trial(
                params={n: float(pm[r, i]) for i, n in enumerate(names)},
                distributions=dists,
                values=list(values(pm[r])),
            )
            for r in range(300)
        ]
    )

    def objective(trial):
        return values([trial.suggest_float(n, 0.0, 1.0) for n in names])

    study.optimize(objective, n_trials=2)
    assert len(study.trials) == 302
    assert counts["fused"] >= 1
