"""The fused feasibility term (``GpConstraintSet``), alone and added to the
LogEI / LogEHVI sessions, against the torch formulation of
``optuna_amd/_gp/acqf.py`` with autograd.

Both sides do the same fp64 math in a different summation order, so the
tolerances are the ones of ``test_gp_fused_ehvi.py``: rtol 1e-8 / atol 1e-10 on
the value, rtol 1e-6 / atol 1e-8 on the gradient.

The synthetic cases fit no GP: the native classes only see raw device pointers,
so a random ``X``, the GP's own Matern covariance plus 0.1 I inverted and
``alpha ~ N(0, 1/N)`` are a complete input. Thresholds are placed from the
reference posterior of the batch, ``t = median(mean) + k median(sigma)`` with
k = -6, 0, +30, so that z sits in the right tail, the centre and the deep left
tail. Shapes are the smallest that reach another code path: N on both sides of
the 256-thread block, D = 1 and the maximum 64, one constraint and several, one
candidate and a few, an N that splits one candidate over several workgroups,
and a scratch budget lowered until the candidates are evaluated in chunks.
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
KS = (-6.0, 0.0, 30.0)  # right tail, centre, deep left tail


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


class _Gps:
    """n synthetic GPs over one X on the device: the first n_obj are objectives,
    the rest constraints."""

    def __init__(self, N, D, n_obj, n_con, seed, jitter=0.1):
        import torch

        dev = torch.device("cuda")
        self._gen = torch.Generator().manual_seed(seed)
        n = n_obj + n_con
        self.N, self.D, self.n_obj, self.n_con = N, D, n_obj, n_con
        self.X = self.rand(N, D).to(dev)
        self.eta = [((0.5 + self.rand(D)) * (2.0 / D)).to(dev) for _ in range(n)]
        self.scale = [float(0.5 + self.rand(1)) for _ in range(n)]
        # 1 / sqrt(N) keeps the posterior mean of order one.
        self.alpha = [(self.randn(N) / np.sqrt(N)).to(dev) for _ in range(n)]
        self.cinv = []
        for i in range(n):
            C = _matern(self.X, self.X, self.eta[i], self.scale[i])
            C = C + jitter * torch.eye(N, dtype=torch.float64, device=dev)
            self.cinv.append(torch.linalg.inv(C).contiguous())
        self.thresholds = [0.0] * n_con
        self._seed = seed
        torch.cuda.synchronize()

    def rand(self, *shape):
        import torch

        return torch.rand(*shape, generator=self._gen, dtype=torch.float64)

    def randn(self, *shape):
        import torch

        return torch.randn(*shape, generator=self._gen, dtype=torch.float64)

    def candidates(self, B):
        return np.random.RandomState(self._seed + 17).rand(B, self.D)

    def posterior(self, i, x):
        """(mean, raw variance before the clamp) of GP i, as GPRegressor.posterior."""
        import torch

        K = _matern(x, self.X, self.eta[i], self.scale[i])
        mean = torch.linalg.vecdot(K, self.alpha[i])
        raw = self.scale[i] - torch.linalg.vecdot(K, K.matmul(self.cinv[i]))
        return mean, raw

    def z(self, c, x):
        import torch

        mean, raw = self.posterior(self.n_obj + c, x)
        return (mean - self.thresholds[c]) / torch.sqrt(raw.clamp_min(0.0) + STAB)

    def place_thresholds(self, x_np, ks):
        """t_c = median(mean_c) + k_c median(sigma_c) over the batch x_np."""
        import torch

        x = torch.from_numpy(x_np).to(self.X.device)
        for c, k in enumerate(ks):
            mean, raw = self.posterior(self.n_obj + c, x)
            sigma = torch.sqrt(raw.clamp_min(0.0) + STAB)
            self.thresholds[c] = float(mean.median() + k * sigma.median())

    def feasibility(self, x):
        """LogPI.eval_acqf's formula summed over the constraints."""
        import torch

        return sum(torch.special.log_ndtr(self.z(c, x)) for c in range(self.n_con))

    def reference(self, x_np, objective=None):
        """(f, grad, z of every constraint) by torch autograd."""
        import torch

        x = torch.from_numpy(x_np).to(self.X.device).requires_grad_(True)
        f = self.feasibility(x)
        if objective is not None:
            f = f + objective(x)
        f.sum().backward()
        with torch.no_grad():
            zs = torch.stack([self.z(c, x) for c in range(self.n_con)])
        return f.detach().cpu().numpy(), x.grad.cpu().numpy(), zs.cpu().numpy()

    def _ptrs(self, tensors, lo, hi):
        return [t.data_ptr() for t in tensors[lo:hi]]

    def constraint_set(self, core, **kw):
        lo, hi = self.n_obj, self.n_obj + self.n_con
        return core.GpConstraintSet(
            [self.X.data_ptr()] * self.n_con,
            self._ptrs(self.alpha, lo, hi), self._ptrs(self.cinv, lo, hi),
            self._ptrs(self.eta, lo, hi), self.scale[lo:hi], self.thresholds,
            self.N, self.D, STAB, **kw,
        )


def _check(evaluate, want_f, want_g, B, D, label):
    """Both gradient settings of evaluate(with_grad) against the reference."""
    f0, g0 = evaluate(False)
    f1, g1 = evaluate(True)
    assert np.asarray(f0).shape == (B,) and np.asarray(g0).size == 0, label
    assert np.asarray(g1).shape == (B, D), label
    assert np.isfinite(want_f).all() and np.isfinite(want_g).all(), label
    np.testing.assert_allclose(f0, want_f, err_msg=label, **F_TOL)
    np.testing.assert_allclose(f1, want_f, err_msg=label, **F_TOL)
    np.testing.assert_allclose(g1, want_g, err_msg=label, **G_TOL)
    return np.asarray(f1), np.asarray(g1)


def _check_set(core, gps: _Gps, x, label, **kw):
    want_f, want_g, zs = gps.reference(x)
    cs = gps.constraint_set(core, **kw)
    _check(lambda grad: cs.eval(x, with_grad=grad), want_f, want_g, len(x), gps.D, label)
    return cs, want_g, zs


# ---- 1. the constraint set alone ------------------------------------------------------


@pytest.mark.parametrize("N, D", [(1, 1), (1, 64), (257, 1), (257, 64)])
@pytest.mark.parametrize("C", [1, 3])
def test_constraint_set_matches_torch_on_synthetic_inputs(core, C: int, N: int, D: int) -> None:
    # One constraint takes each placement in turn; three take one each.
    placements = [KS] if C == 3 else [(k,) for k in KS]
    z_min, z_max = np.inf, -np.inf
    moved = expected_to_move = 0
    for B, ks in itertools.product((1, 7), placements):
        gps = _Gps(N, D, 0, C, seed=1000 * C + 10 * N + D + B)
        x = gps.candidates(B)
        gps.place_thresholds(x, ks)
        label = f"N={N} D={D} C={C} B={B} k={ks}"
        _, want_g, zs = _check_set(core, gps, x, label)
        assert np.isfinite(zs).all(), label
        z_min, z_max = min(z_min, zs.min()), max(z_max, zs.max())
        if ks != (-6.0,):  # a centre or a left-tail constraint is present
            expected_to_move += 1
            moved += int(np.abs(want_g).max() > 1e-6)
    assert z_min < -20.0 and z_max > 4.0
    # The gradient check is not a comparison of zeros.
    assert moved == expected_to_move >= 2


# ---- 2. splits and chunks --------------------------------------------------------------


def test_splits_over_workgroups_and_candidate_chunks(core) -> None:
    N, D = 1031, 5
    gps = _Gps(N, D, 0, 3, seed=41)
    x1 = gps.candidates(1)
    gps.place_thresholds(x1, KS)
    cs, _, _ = _check_set(core, gps, x1, "one candidate over several workgroups")
    assert cs.n_splits(1) > 1
    assert cs.n_splits(100000) == 1

    x13 = gps.candidates(13)
    gps.place_thresholds(x13, KS)
    cs, _, _ = _check_set(core, gps, x13, "chunks of two", scratch_budget_bytes=2 * 3 * N * 8)
    assert cs.n_chunks(13, True) == 7
    # Less than one candidate's worth still evaluates, one candidate at a time.
    cs, _, _ = _check_set(core, gps, x13[:3].copy(), "budget 8", scratch_budget_bytes=8)
    assert cs.n_chunks(3, True) == 3


# ---- 3. clamped variance ---------------------------------------------------------------


def test_clamped_variance_passes_no_gradient(core) -> None:
    """An inverse that overshoots drives scale - K Cinv K below zero: sigma sits
    on sqrt(stab), and like autograd the closed form sends nothing through the
    variance (w_v = 0; a w_v taken from the formula would be of order
    rho z / stab and swamp the gradient).

    With sigma = 1e-6 the z of a batch spread by (mean_b - t) / 1e-6. The means
    are scaled down to that order so that |z| stays below 1e3: autograd's
    log_ndtr backward is exp(-(log Phi + z^2 / 2)), whose rounding error grows
    as 1e-16 z^2 / 2 and would pass the gradient tolerance near |z| = 1e5, where
    the comparison would measure the reference."""
    import torch

    gps = _Gps(64, 3, 0, 3, seed=93)
    for c in range(3):
        gps.cinv[c] = (50.0 * torch.eye(64, dtype=torch.float64, device="cuda")).contiguous()
        gps.alpha[c] = (1e-5 * gps.alpha[c]).contiguous()
    torch.cuda.synchronize()
    x = gps.candidates(4)
    xt = torch.from_numpy(x).cuda()
    for c in range(3):
        assert bool((gps.posterior(c, xt)[1] < 0).all())
    gps.place_thresholds(x, KS)
    _, want_g, zs = _check_set(core, gps, x, "clamped")
    assert np.abs(zs).max() < 1e3 and zs.min() < -20.0 and zs.max() > 4.0
    assert np.abs(want_g).max() > 1e-6


# ---- 4. composition with the objective sessions ----------------------------------------


def _logei_session(core, gps: _Gps, f0: float):
    return core.GpLogEiSession(
        gps.X.data_ptr(), gps.alpha[0].data_ptr(), gps.cinv[0].data_ptr(),
        gps.eta[0].data_ptr(), gps.N, gps.D, gps.scale[0], STAB, f0,
    )


def _torch_logei(gps: _Gps, f0: float):
    from optuna_amd._gp import acqf as acqf_mod

    def objective(x):
        mean, raw = gps.posterior(0, x)
        return acqf_mod.logei(mean=mean, var=raw.clamp_min(0.0) + STAB, f0=f0)

    return objective


class _Boxes:
    """QMC normals and boxes for M objectives, as in test_gp_fused_ehvi.py."""

    def __init__(self, gps: _Gps, Q, J):
        M = gps.n_obj
        dev = gps.X.device
        self.eps = gps.randn(Q, M).to(dev)
        self.lo = (0.7 * gps.randn(J, M)).to(dev)
        self.iv = (0.05 + 1.95 * gps.rand(J, M)).to(dev)
        self.iv[J // 2, 0] = float("inf")  # unbounded boxes occur in practice

    def session(self, core, gps: _Gps):
        M = gps.n_obj
        return core.GpLogEhviSession(
            [gps.X.data_ptr()] * M,
            [a.data_ptr() for a in gps.alpha[:M]], [c.data_ptr() for c in gps.cinv[:M]],
            [e.data_ptr() for e in gps.eta[:M]], gps.scale[:M], gps.N, gps.D, STAB,
            self.eps.cpu().numpy(), self.lo.cpu().numpy(), self.iv.cpu().numpy(),
        )

    def torch_objective(self, gps: _Gps):
        import torch

        from optuna_amd._gp import acqf as acqf_mod

        def objective(x):
            cols = []
            for m in range(gps.n_obj):
                mean, raw = gps.posterior(m, x)
                sd = torch.sqrt(raw.clamp_min(0.0) + STAB)
                cols.append(mean[..., None] + sd[..., None] * self.eps[..., m])
            return acqf_mod.logehvi(torch.stack(cols, dim=-1), self.lo, self.iv)

        return objective


def _same_bits(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(np.asarray(u), np.asarray(v))


@pytest.mark.parametrize("B", [1, 9])
def test_logei_session_adds_the_feasibility_term(core, B: int) -> None:
    gps = _Gps(257, 7, 1, 3, seed=500 + B)
    x = gps.candidates(B)
    gps.place_thresholds(x, KS)
    f0 = 0.1
    want_f, want_g, _ = gps.reference(x, _torch_logei(gps, f0))
    cs = gps.constraint_set(core)
    sess = _logei_session(core, gps, f0)
    _check(lambda grad: sess.eval(x, grad, constraints=cs), want_f, want_g, B, gps.D, f"B={B}")
    # The feasibility term is not negligible next to log-EI here.
    plain = np.asarray(sess.eval(x, True)[0])
    assert np.abs(want_f - plain).min() > 1.0
    for grad in (False, True):
        _same_bits(sess.eval(x, grad, constraints=None), sess.eval(x, grad))


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("M", [2, 4])
def test_logehvi_session_adds_the_feasibility_term(core, M: int, B: int) -> None:
    gps = _Gps(257, 7, M, 3, seed=600 + 10 * M + B)
    boxes = _Boxes(gps, Q=128, J=core.GP_EHVI_BOX_TILE + 1)
    x = gps.candidates(B)
    gps.place_thresholds(x, KS)
    want_f, want_g, _ = gps.reference(x, boxes.torch_objective(gps))
    cs = gps.constraint_set(core)
    sess = boxes.session(core, gps)
    _check(
        lambda grad: sess.eval(x, grad, constraints=cs), want_f, want_g, B, gps.D, f"M={M} B={B}"
    )
    plain = np.asarray(sess.eval(x, True)[0])
    assert np.abs(want_f - plain).min() > 1.0
    for grad in (False, True):
        _same_bits(sess.eval(x, grad, constraints=None), sess.eval(x, grad))


def test_constraint_set_of_another_shape_is_refused(core) -> None:
    gps = _Gps(33, 3, 1, 1, seed=7)
    other = _Gps(34, 3, 0, 1, seed=8)
    with pytest.raises(RuntimeError):
        _logei_session(core, gps, 0.1).eval(
            gps.candidates(2), True, constraints=other.constraint_set(core)
        )
    with pytest.raises(RuntimeError):
        core.GpConstraintSet([], [], [], [], [], [], 33, 3, STAB)
    n = core.GP_FEAS_MAX_C + 1
    with pytest.raises(RuntimeError):
        core.GpConstraintSet(
            [gps.X.data_ptr()] * n, [gps.alpha[0].data_ptr()] * n, [gps.cinv[0].data_ptr()] * n,
            [gps.eta[0].data_ptr()] * n, [1.0] * n, [0.0] * n, 33, 3, STAB,
        )


# ---- 5. the acquisition functions' entry points ----------------------------------------


@pytest.fixture(scope="module")
def fitted(core):
    """Two objective GPs and two constraint GPs fitted on 200 observations of
    smooth functions of X; about half of the rows are feasible.

    The observations carry noise of 0.3 standard deviations. Fitted to exact
    values of such smooth functions the GPs take a noise near the 1e-6 floor,
    scale - K Cinv K is then all cancellation, and two fp64 summation orders of
    it share few digits: the comparison would be one of rounding noise. The
    torch formulation evaluated in fp64 and in extended precision on the host
    differs by 1e-6 relative in log Phi with noise-free observations, by 7e-9
    at 0.1 standard deviations and by 2e-10 at 0.3, which leaves the 1e-8
    tolerance to the code under test."""
    from optuna_amd._gp import gp as gp_mod
    from optuna_amd._gp import prior
    from optuna_amd._gp import search_space as gp_ss

    n, d = 200, 3
    rng = np.random.RandomState(31)
    X = rng.rand(n, d)
    Y = np.stack([-np.sum(np.square(X), axis=1), -np.sum(np.square(X - 1.0), axis=1)], axis=1)
    Y = (Y - Y.mean(0)) / Y.std(0) + 0.3 * rng.randn(n, 2)
    # Feasible where c <= 0, as the sampler has it: x0 + x1 <= 1.25 and x2 >= 0.2.
    cons = np.stack([X[:, 0] + X[:, 1] - 1.25, 0.2 - X[:, 2]], axis=1)
    cons = cons + 0.3 * cons.std(0) * rng.randn(n, 2)
    feasible = (cons <= 0).all(axis=1)
    assert 0.35 < feasible.mean() < 0.65
    c_std = (-cons - (-cons).mean(0)) / (-cons).std(0)
    thresholds = (-(-cons).mean(0) / (-cons).std(0)).tolist()

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(gp_mod.GPRegressor, "_DEVICE_FIT_MIN_OBS", 100)
        gprs = [
            gp_mod.fit_kernel_params(
                X, col, np.zeros(d, dtype=bool), prior.default_log_prior, 1e-6, False
            )
            for col in (Y[:, 0], Y[:, 1], c_std[:, 0], c_std[:, 1])
        ]
    assert all(g.device.type == "cuda" and g._cov_Y_Y_inv is not None for g in gprs)
    space = gp_ss.SearchSpace({f"x{i}": FloatDistribution(0.0, 1.0) for i in range(d)})
    return dict(
        d=d, Y=Y, feasible=feasible, objectives=gprs[:2], constraints=gprs[2:],
        thresholds=thresholds, space=space,
    )


def _make_acqf(fitted, kind: str, **kw):
    import torch

    from optuna_amd._gp import acqf as acqf_mod

    common = dict(
        search_space=fitted["space"],
        constraints_gpr_list=fitted["constraints"],
        constraints_threshold_list=fitted["thresholds"],
    )
    if kind.startswith("LogCEI"):
        best = float(fitted["Y"][fitted["feasible"], 0].max())
        threshold = -np.inf if kind == "LogCEI no feasible" else best
        return acqf_mod.LogCEI(gpr=fitted["objectives"][0], threshold=threshold, **common)
    y_feasible = (
        None
        if kind == "LogCEHVI no feasible"
        else torch.from_numpy(fitted["Y"][fitted["feasible"]])
    )
    return acqf_mod.LogCEHVI(
        gpr_list=fitted["objectives"], Y_feasible=y_feasible, n_qmc_samples=128, qmc_seed=5,
        **common, **kw,
    )


KINDS = ["LogCEI", "LogCEI no feasible", "LogCEHVI", "LogCEHVI no feasible"]


@pytest.mark.parametrize("kind", KINDS)
def test_constrained_entry_points_use_the_session(core, fitted, monkeypatch, kind: str) -> None:
    from optuna_amd._gp import acqf as acqf_mod

    d = fitted["d"]
    acqf = _make_acqf(fitted, kind)
    session = acqf._fused_session()
    assert session is not None
    assert (session._objective is None) == kind.endswith("no feasible")

    base = acqf_mod.BaseAcquisitionFunc
    cands = np.random.RandomState(22).rand(24, d)
    many = acqf.eval_acqf_no_grad(cands)
    assert many.shape == (24,)
    np.testing.assert_allclose(many, base.eval_acqf_no_grad(acqf, cands), **F_TOL)
    one = acqf.eval_acqf_no_grad(cands[3])
    assert np.ndim(one) == 0
    np.testing.assert_allclose(one, base.eval_acqf_no_grad(acqf, cands[3]), **F_TOL)

    fb, gb = acqf.eval_acqf_batched_with_grad(cands[:6].copy())
    rf, rg = base.eval_acqf_batched_with_grad(acqf, cands[:6].copy())
    assert fb.shape == (6,) and gb.shape == (6, d)
    assert np.abs(rg).max() > 1e-3
    np.testing.assert_allclose(fb, rf, **F_TOL)
    np.testing.assert_allclose(gb, rg, **G_TOL)

    f1, g1 = acqf.eval_acqf_with_grad(cands[7].copy())
    r1, rg1 = base.eval_acqf_with_grad(acqf, cands[7].copy())
    assert isinstance(f1, float) and g1.shape == (d,)
    np.testing.assert_allclose(f1, r1, **F_TOL)
    np.testing.assert_allclose(g1, rg1, **G_TOL)

    monkeypatch.setenv("OPTUNA_AMD_GP_FUSED_CONSTRAINED", "0")
    forced = _make_acqf(fitted, kind)
    assert forced._fused_session() is None
    np.testing.assert_allclose(forced.eval_acqf_no_grad(cands), many, **F_TOL)


def test_constrained_cases_that_stay_on_torch(core, fitted, monkeypatch) -> None:
    running = np.random.RandomState(23).rand(2, fitted["d"])
    with_running = _make_acqf(fitted, "LogCEHVI", normalized_params_of_running_trials=running)
    assert with_running._fused_session() is None
    # An objective term without a session keeps the whole acquisition on torch.
    monkeypatch.setenv("OPTUNA_AMD_GP_FUSED_EHVI", "0")
    assert _make_acqf(fitted, "LogCEHVI")._fused_session() is None
    assert _make_acqf(fitted, "LogCEHVI no feasible")._fused_session() is not None


# ---- 6. the shared workspace -----------------------------------------------------------


def test_workspace_shared_between_all_gp_sessions_in_both_orders(core) -> None:
    """The constraint set and both objective sessions, with and without
    constraints, lay their regions over the same workspace. Whatever the other
    left behind, and in whichever order the workspace grew, each call returns
    the same bits."""
    small = _Gps(1, 1, 2, 1, seed=301)
    large = _Gps(257, 7, 3, 3, seed=302)
    small_boxes = _Boxes(small, Q=1, J=1)
    large_boxes = _Boxes(large, Q=128, J=core.GP_EHVI_BOX_TILE + 1)
    small.place_thresholds(small.candidates(1), (0.0,))
    large.place_thresholds(large.candidates(9), KS)

    def call(gps, boxes, what, B, grad):
        x = gps.candidates(B)

        def run():
            cs = gps.constraint_set(core)
            if what == "set":
                f, g = cs.eval(x, with_grad=grad)
            else:
                sess = (
                    _logei_session(core, gps, 0.1) if what.startswith("logei")
                    else boxes.session(core, gps)
                )
                f, g = sess.eval(x, grad, constraints=cs if what.endswith("+c") else None)
            return np.concatenate([np.asarray(f).ravel(), np.asarray(g).ravel()])

        return run

    calls = {}
    for what in ("set", "logei+c", "ehvi+c", "logei", "ehvi"):
        calls[f"{what} small"] = call(small, small_boxes, what, 1, True)
        calls[f"{what} large"] = call(large, large_boxes, what, 9, True)
    calls["set large no grad"] = call(large, large_boxes, "set", 9, False)
    calls["ehvi+c large no grad"] = call(large, large_boxes, "ehvi+c", 9, False)

    order_a = sorted(calls, key=lambda name: (name.split()[1] != "small", name))
    order_b = sorted(calls, reverse=True) + ["set small", "ehvi+c large", "logei+c small"]
    assert order_a != order_b[: len(order_a)] and set(order_a) == set(order_b) == set(calls)
    got_b = [(name, calls[name]()) for name in order_b]
    got_a = {name: calls[name]() for name in order_a}
    for name, got in got_b:
        assert np.isfinite(got).all(), name
        np.testing.assert_array_equal(got, got_a[name], err_msg=name)


# ---- 7. the sampler end to end ---------------------------------------------------------


@pytest.mark.parametrize(
    "n_objectives, any_feasible", [(1, True), (2, True), (1, False), (2, False)],
    ids=["LogCEI", "LogCEHVI", "LogCEI no feasible", "LogCEHVI no feasible"],
)
def test_gp_sampler_uses_fused_constrained_path(
    core, monkeypatch, n_objectives: int, any_feasible: bool
) -> None:
    """A constrained GPSampler study on a device-sized history must run its
    acquisition through the fused session: objective session plus constraint
    set, or the constraint set alone while no trial is feasible."""
    from optuna_amd._gp import acqf as acqf_mod
    from optuna_amd._gp import gp as gp_mod

    monkeypatch.setattr(gp_mod.GPRegressor, "_DEVICE_FIT_MIN_OBS", 100)
    cls = acqf_mod.LogCEI if n_objectives == 1 else acqf_mod.LogCEHVI
    seen = {"fused": 0, "alone": 0}
    orig = cls._fused_session

    def spy(self):
        out = orig(self)
        if out is not None:
            seen["fused"] += 1
            seen["alone"] += int(out._objective is None)
        return out

    monkeypatch.setattr(cls, "_fused_session", spy)
    warnings.simplefilter("ignore")
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    rng = np.random.RandomState(4)
    names = [f"x{i}" for i in range(4)]
    dists = {n: FloatDistribution(0.0, 1.0) for n in names}

    def values(x):
        x = np.asarray(x)
        both = [float(np.sum(np.square(x))), float(np.sum(np.square(x - 1.0)))]
        return both[:n_objectives]

    def constraints_of(x):
        # Feasible (<= 0) for about half of the unit cube, or nowhere in it.
        if any_feasible:
            return [float(x[0] + x[1] - 1.0), float(0.1 - x[2])]
        return [float(x[0] + x[1] + 0.1), float(1.1 - x[2])]

    study = optuna_amd.create_study(
        directions=["minimize"] * n_objectives,
        sampler=optuna_amd.samplers.GPSampler(
            seed=0, n_startup_trials=5,
            constraints_func=lambda t: constraints_of([t.params[n] for n in names]),
        ),
    )
    pm = rng.rand(300, 4)
    study.add_trials(
        [
            optuna_amd.create_trial(
                params={n: float(pm[r, i]) for i, n in enumerate(names)},
                distributions=dists,
                values=values(pm[r]),
                system_attrs={"constraints": constraints_of(pm[r])},
            )
            for r in range(300)
        ]
    )
    n_feasible = sum(max(t.system_attrs["constraints"]) <= 0 for t in study.trials)
    assert (50 < n_feasible < 250) if any_feasible else n_feasible == 0

    def objective(trial):
        out = values([trial.suggest_float(n, 0.0, 1.0) for n in names])
        return out[0] if n_objectives == 1 else out

    study.optimize(objective, n_trials=2)
    assert len(study.trials) == 302
    assert seen["fused"] >= 1
    assert (seen["alone"] == 0) if any_feasible else (seen["alone"] == seen["fused"])
