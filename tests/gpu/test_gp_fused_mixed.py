"""The fused GP sessions on search spaces with categorical columns (``cat_mask``)
against the torch formulas of ``optuna_amd/_gp/acqf.py`` with the Hamming
overwrite of ``GPRegressor.kernel`` and autograd.

On a categorical column the kernel's distance term is ``eta_d * [x_d != X_id]``
and the input gradient is exactly zero. Both sides do the same fp64 math in a
different summation order, so the tolerances are the project's: rtol 1e-8 /
atol 1e-10 on the value, rtol 1e-6 / atol 1e-8 on the gradient of the continuous
columns; the gradient of a categorical column must equal 0.0.

The synthetic problems fit no GP (random ``X`` with integer codes on the
categorical columns, the inverse of the mixed Matern matrix plus jitter, random
``alpha``). Shapes are the smallest that reach another path: N = 1 and both sides
of the 256-thread block, D = 1 (all categorical), a middle column of 3, both end
columns of the maximum 64, one candidate and ten (more than one workgroup per
candidate), and a scratch budget lowered until the batch takes several chunks.
Among ten candidates half take codes that occur in ``X``, one takes a code no row
has, and one copies a training row exactly (r2 = 0).
"""
from __future__ import annotations

import functools
import warnings

import numpy as np
import pytest

import optuna_amd
from optuna_amd import _hip
from optuna_amd.distributions import (
    CategoricalDistribution,
    FloatDistribution,
    IntDistribution,
)


pytestmark = pytest.mark.gpu

F_TOL = dict(rtol=1e-8, atol=1e-10)
G_TOL = dict(rtol=1e-6, atol=1e-8)
STAB = 1e-12
N_CODES = 3
ABSENT_CODE = 7.0
THRESHOLD = 0.1
MAX_M, N_CONS = 4, 2

SHAPES = [
    pytest.param(N, D, mask, id=f"N{N}-D{D}-mask{mask:#x}")
    for N in (1, 255, 257)
    for D, mask in ((1, 0b1), (3, 0b010), (64, (1 << 63) | 1))
]


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


def _columns(mask: int, D: int) -> list[int]:
    return [d for d in range(D) if (mask >> d) & 1]


def _matern(x, X, eta, scale, cat):
    """scale * Matern-5/2 of the mixed ARD distance, (B, N); differentiable in x."""
    from optuna_amd._gp import gp as gp_mod

    sqd = (x.unsqueeze(-2) - X.unsqueeze(-3)).square()
    if cat:
        sqd[..., cat] = (sqd[..., cat] > 0.0).double()
    return gp_mod.matern52_of_sqdist((sqd * eta).sum(-1)) * scale


class _Problem:
    """MAX_M objective GPs and N_CONS constraint GPs over one mixed X, plus QMC
    normals and boxes for every M, on the device."""

    Q, J = 5, 9

    def __init__(self, N: int, D: int, mask: int, seed: int) -> None:
        import torch

        dev = torch.device("cuda")
        g = torch.Generator().manual_seed(seed)

        def rand(*shape):
            return torch.rand(*shape, generator=g, dtype=torch.float64)

        def randn(*shape):
            return torch.randn(*shape, generator=g, dtype=torch.float64)

        self.N, self.D, self.mask = N, D, mask
        self.cat = _columns(mask, D)
        X = rand(N, D)
        for d in self.cat:
            X[:, d] = torch.randint(N_CODES, (N,), generator=g).double()
        self.X = X.to(dev)
        n_gps = MAX_M + N_CONS
        self.eta = [((0.5 + rand(D)) * (2.0 / D)).to(dev) for _ in range(n_gps)]
        self.scale = [float(0.5 + rand(1)) for _ in range(n_gps)]
        # 1 / sqrt(N) keeps the posterior mean of order one.
        self.alpha = [(randn(N) / np.sqrt(N)).to(dev) for _ in range(n_gps)]
        self.cinv = []
        for i in range(n_gps):
            C = _matern(self.X, self.X, self.eta[i], self.scale[i], self.cat)
            C = C + 0.1 * torch.eye(N, dtype=torch.float64, device=dev)
            self.cinv.append(torch.linalg.inv(C).contiguous())
        self.con_thresholds = [-0.2, 0.3]
        self.eps = {M: randn(self.Q, M).to(dev) for M in (2, MAX_M)}
        self.lo = {M: (0.7 * randn(self.J, M)).to(dev) for M in (2, MAX_M)}
        self.iv = {M: (0.05 + 1.95 * rand(self.J, M)).to(dev) for M in (2, MAX_M)}
        self._rng_seed = seed
        self._want: dict = {}
        torch.cuda.synchronize()

    def candidates(self, B: int) -> np.ndarray:
        rng = np.random.RandomState(self._rng_seed + 17 + B)
        X = self.X.cpu().numpy()
        x = rng.rand(B, self.D)
        for d in self.cat:
            x[:, d] = rng.randint(N_CODES, size=B)
            half = (B + 1) // 2
            x[:half, d] = X[rng.randint(self.N, size=half), d]  # codes X has
        if B >= 3:
            x[B - 2, self.cat] = ABSENT_CODE  # a code no row has
            x[B - 1] = X[rng.randint(self.N)]  # a training row: r2 = 0
        return x

    # ---- sessions ----------------------------------------------------------------

    def _ptrs(self, idx):
        return (
            [self.X.data_ptr()] * len(idx),
            [self.alpha[i].data_ptr() for i in idx],
            [self.cinv[i].data_ptr() for i in idx],
            [self.eta[i].data_ptr() for i in idx],
            [self.scale[i] for i in idx],
        )

    def logei(self, core, **kw):
        kw.setdefault("cat_mask", self.mask)
        return core.GpLogEiSession(
            self.X.data_ptr(), self.alpha[0].data_ptr(), self.cinv[0].data_ptr(),
            self.eta[0].data_ptr(), self.N, self.D, self.scale[0], STAB, THRESHOLD, **kw,
        )

    def logehvi(self, core, M: int, **kw):
        kw.setdefault("cat_mask", self.mask)
        return core.GpLogEhviSession(
            *self._ptrs(range(M)), self.N, self.D, STAB,
            self.eps[M].cpu().numpy(), self.lo[M].cpu().numpy(), self.iv[M].cpu().numpy(),
            **kw,
        )

    def constraint_set(self, core, **kw):
        kw.setdefault("cat_mask", self.mask)
        return core.GpConstraintSet(
            *self._ptrs(range(MAX_M, MAX_M + N_CONS)), self.con_thresholds,
            self.N, self.D, STAB, **kw,
        )

    # ---- the torch side ----------------------------------------------------------

    def _posterior(self, x, i):
        import torch

        K = _matern(x, self.X, self.eta[i], self.scale[i], self.cat)
        mean = torch.linalg.vecdot(K, self.alpha[i])
        var = (self.scale[i] - torch.linalg.vecdot(K, K.matmul(self.cinv[i]))).clamp_min(0.0)
        return mean, var

    def want(self, kind: str, B: int):
        """(f, g) of acqf.py's formulas for ``kind`` in {"ei", "ehvi2", "ehvi4",
        "con"}, computed once per (kind, B)."""
        import torch

        from optuna_amd._gp import acqf as acqf_mod

        if (kind, B) not in self._want:
            x = torch.from_numpy(self.candidates(B)).to(self.X.device).requires_grad_(True)
            if kind == "ei":
                mean, var = self._posterior(x, 0)
                f = acqf_mod.logei(mean=mean, var=var + STAB, f0=THRESHOLD)
            elif kind == "con":
                f = 0.0
                for c in range(N_CONS):
                    mean, var = self._posterior(x, MAX_M + c)
                    f = f + torch.special.log_ndtr(
                        (mean - self.con_thresholds[c]) / torch.sqrt(var + STAB)
                    )
            else:
                M = int(kind[-1])
                cols = []
                for m in range(M):
                    mean, var = self._posterior(x, m)
                    sd = torch.sqrt(var + STAB)
                    cols.append(mean[..., None] + sd[..., None] * self.eps[M][..., m])
                f = acqf_mod.logehvi(torch.stack(cols, dim=-1), self.lo[M], self.iv[M])
            f.sum().backward()
            got = f.detach().cpu().numpy(), x.grad.cpu().numpy()
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
            self._want[kind, B] = got
        return self._want[kind, B]


@functools.lru_cache(maxsize=None)
def _problem(N: int, D: int, mask: int) -> _Problem:
    return _Problem(N, D, mask, seed=100 * N + D)


def _check(prob: _Problem, evaluate, kinds: list[str], B: int, label: str) -> np.ndarray:
    """``evaluate(x, with_grad)`` against the sum of the torch terms ``kinds``."""
    x = prob.candidates(B)
    want_f = sum(prob.want(k, B)[0] for k in kinds)
    want_g = sum(prob.want(k, B)[1] for k in kinds)
    label = f"{label} N={prob.N} D={prob.D} mask={prob.mask:#x} B={B}"
    f0, g0 = evaluate(x, False)
    f1, g1 = evaluate(x, True)
    f0, f1, g1 = np.asarray(f0), np.asarray(f1), np.asarray(g1)
    assert f0.shape == (B,) and np.asarray(g0).size == 0, label
    assert g1.shape == (B, prob.D), label
    np.testing.assert_allclose(f0, want_f, err_msg=label, **F_TOL)
    np.testing.assert_allclose(f1, want_f, err_msg=label, **F_TOL)
    cont = [d for d in range(prob.D) if d not in prob.cat]
    np.testing.assert_allclose(g1[:, cont], want_g[:, cont], err_msg=label, **G_TOL)
    assert np.all(g1[:, prob.cat] == 0.0), label
    assert np.all(want_g[:, prob.cat] == 0.0), label  # autograd agrees
    return g1


@pytest.mark.parametrize("N, D, mask", SHAPES)
def test_logei_session_on_a_mixed_space(core, N: int, D: int, mask: int) -> None:
    prob = _problem(N, D, mask)
    sess = prob.logei(core)
    cset = prob.constraint_set(core)
    moved = 0.0
    for B in (1, 10):
        g = _check(prob, lambda x, wg: sess.eval(x, with_grad=wg), ["ei"], B, "LogEI")
        moved = max(moved, float(np.abs(g).max()))
        _check(
            prob,
            lambda x, wg: sess.eval(x, with_grad=wg, constraints=cset),
            ["ei", "con"], B, "LogEI + constraints",
        )
    # With a continuous column the gradient check is not a comparison of zeros.
    assert (moved > 1e-6) == (D > len(prob.cat))


@pytest.mark.parametrize("N, D, mask", SHAPES)
def test_logehvi_session_on_a_mixed_space(core, N: int, D: int, mask: int) -> None:
    prob = _problem(N, D, mask)
    sess = prob.logehvi(core, 2)
    cset = prob.constraint_set(core)
    for B in (1, 10):
        _check(prob, lambda x, wg: sess.eval(x, with_grad=wg), ["ehvi2"], B, "LogEHVI")
        _check(
            prob,
            lambda x, wg: sess.eval(x, with_grad=wg, constraints=cset),
            ["ehvi2", "con"], B, "LogEHVI + constraints",
        )


def test_logehvi_session_with_four_objectives(core) -> None:
    prob = _problem(257, 3, 0b010)
    sess = prob.logehvi(core, 4)
    _check(prob, lambda x, wg: sess.eval(x, with_grad=wg), ["ehvi4"], 10, "LogEHVI M=4")


@pytest.mark.parametrize("N, D, mask", SHAPES)
def test_constraint_set_alone_on_a_mixed_space(core, N: int, D: int, mask: int) -> None:
    prob = _problem(N, D, mask)
    cset = prob.constraint_set(core)
    for B in (1, 10):
        _check(prob, lambda x, wg: cset.eval(x, with_grad=wg), ["con"], B, "constraints")
    if N > 256:
        assert cset.n_splits(10) > 1  # more than one workgroup per candidate


def test_lowered_scratch_budget_takes_several_chunks(core) -> None:
    N, D, mask, B, M = 257, 3, 0b010, 10, 2
    prob = _problem(N, D, mask)
    budget = 2 * M * 3 * N * 8  # two candidates with the gradient, 2 M without
    sess = prob.logehvi(core, M, scratch_budget_bytes=budget)
    cset = prob.constraint_set(core, scratch_budget_bytes=2 * 3 * N * 8)
    assert sess.n_chunks(B, True) == 5 and sess.n_chunks(B, False) >= 2
    assert cset.n_chunks(B, True) == 5
    _check(prob, lambda x, wg: sess.eval(x, with_grad=wg), ["ehvi2"], B, "chunked LogEHVI")
    _check(
        prob,
        lambda x, wg: sess.eval(x, with_grad=wg, constraints=cset),
        ["ehvi2", "con"], B, "chunked LogEHVI + constraints",
    )
    _check(prob, lambda x, wg: cset.eval(x, with_grad=wg), ["con"], B, "chunked constraints")


def test_mask_zero_is_the_argument_left_out(core) -> None:
    """On an all-continuous problem ``cat_mask=0`` and no ``cat_mask`` run the
    same code: equal bits."""
    prob = _problem(257, 3, 0)
    x = prob.candidates(10)
    pairs = {
        "LogEI": (prob.logei(core, cat_mask=0), core.GpLogEiSession(
            prob.X.data_ptr(), prob.alpha[0].data_ptr(), prob.cinv[0].data_ptr(),
            prob.eta[0].data_ptr(), prob.N, prob.D, prob.scale[0], STAB, THRESHOLD,
        )),
        "LogEHVI": (prob.logehvi(core, 2, cat_mask=0), core.GpLogEhviSession(
            *prob._ptrs(range(2)), prob.N, prob.D, STAB, prob.eps[2].cpu().numpy(),
            prob.lo[2].cpu().numpy(), prob.iv[2].cpu().numpy(),
        )),
        "constraints": (prob.constraint_set(core, cat_mask=0), core.GpConstraintSet(
            *prob._ptrs(range(MAX_M, MAX_M + N_CONS)), prob.con_thresholds,
            prob.N, prob.D, STAB,
        )),
    }
    for name, (with_zero, without) in pairs.items():
        for with_grad in (False, True):
            f_a, g_a = with_zero.eval(x, with_grad=with_grad)
            f_b, g_b = without.eval(x, with_grad=with_grad)
            np.testing.assert_array_equal(np.asarray(f_a), np.asarray(f_b), err_msg=name)
            np.testing.assert_array_equal(np.asarray(g_a), np.asarray(g_b), err_msg=name)
            assert np.isfinite(np.asarray(f_a)).all(), name
    # The continuous problem is a real one for the sessions: it matches torch.
    _check(prob, lambda x, wg: pairs["LogEI"][0].eval(x, with_grad=wg), ["ei"], 10, "mask 0")


def test_mask_checks(core) -> None:
    prob = _problem(257, 3, 0b010)
    for build in (
        lambda m: prob.logei(core, cat_mask=m),
        lambda m: prob.logehvi(core, 2, cat_mask=m),
        lambda m: prob.constraint_set(core, cat_mask=m),
    ):
        build(0b100)  # the last column is within D
        with pytest.raises(RuntimeError, match="cat_mask"):
            build(0b1000)
        with pytest.raises(RuntimeError, match="cat_mask"):
            build(1 << 63)
    # A set over another search space than the session's.
    x = prob.candidates(10)
    other = prob.constraint_set(core, cat_mask=0b001)
    for sess in (prob.logei(core), prob.logehvi(core, 2)):
        with pytest.raises(RuntimeError, match="cat_mask"):
            sess.eval(x, with_grad=False, constraints=other)
        sess.eval(x, with_grad=False, constraints=prob.constraint_set(core))


def test_no_per_dimension_tensor_for_a_mixed_space(core) -> None:
    """A condition, not a measurement: neither the fit's loss nor a cross
    covariance of a device-resident mixed regressor may allocate half of the
    (N, N, D) / (B, N, D) tensor that the dense formulation needs. The
    legitimate (N, N) and (B, N) temporaries are 8 MiB and 4 MiB each."""
    import torch

    from optuna_amd._gp import gp as gp_mod

    N, D, B = 1024, 64, 512
    rng = np.random.RandomState(5)
    is_cat = np.zeros(D, dtype=bool)
    is_cat[::8] = True
    assert is_cat.sum() == 8
    X = rng.rand(N, D)
    X[:, is_cat] = rng.randint(4, size=(N, 8))
    dev = torch.device("cuda")
    gpr = gp_mod.GPRegressor(
        is_categorical=torch.from_numpy(is_cat).to(dev),
        X_train=torch.from_numpy(X).to(dev),
        y_train=torch.from_numpy(rng.randn(N)).to(dev),
        inverse_squared_lengthscales=torch.ones(D, dtype=torch.float64, device=dev),
        kernel_scale=torch.tensor(1.0, dtype=torch.float64, device=dev),
        noise_var=torch.tensor(0.1, dtype=torch.float64, device=dev),
    )
    assert gpr._squared_X_diff is None
    X1 = torch.from_numpy(X[:B] + 0.0).to(dev)
    raw = np.zeros(D + 2)

    def peak_rise(call) -> int:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        del out
        return torch.cuda.max_memory_allocated() - before

    rise = peak_rise(
        lambda: gpr._loss_and_grad_closed_form_torch(
            raw, gpr._X_train, gpr._y_train.squeeze(-1), 1e-6, False
        )
    )
    assert rise < 8 * N * N * D // 2, f"loss: {rise / 2**20:.1f} MiB"
    rise = peak_rise(lambda: gpr.kernel(X1, gpr._X_train))
    assert rise < 8 * B * N * D // 2, f"kernel: {rise / 2**20:.1f} MiB"


def test_gp_sampler_stays_on_the_device_with_a_categorical_parameter(
    core, monkeypatch
) -> None:
    """Two suggests of a GPSampler study over 2 floats, 1 int and 1 categorical:
    the regressor lives in HBM without a dense tensor, the acquisition runs
    through a fused session that carries the categorical column, and the second
    suggest absorbs the new trial without a refit.

    The history is 80 trials: the refit cadence (``_incremental_update_applicable``)
    lets a regressor absorb fewer than max(1, n_fit // 40) new rows, which at 40
    observations is none, so no history of 40 could ever reach ``update_data``.
    """
    from optuna_amd._gp import acqf as acqf_mod
    from optuna_amd._gp import gp as gp_mod

    monkeypatch.setattr(gp_mod.GPRegressor, "_DEVICE_FIT_MIN_OBS", 32)
    constructed: list[int] = []
    real_session = core.GpLogEiSession

    def recording_session(*args, **kwargs):
        constructed.append(kwargs.get("cat_mask", 0))
        return real_session(*args, **kwargs)

    monkeypatch.setattr(core, "GpLogEiSession", recording_session)
    sessions: list[object] = []
    real_fused = acqf_mod.LogEI._fused_session

    def fused_spy(self):
        out = real_fused(self)
        sessions.append(out)
        return out

    monkeypatch.setattr(acqf_mod.LogEI, "_fused_session", fused_spy)
    absorbed: list[bool] = []
    real_update = gp_mod.GPRegressor.update_data

    def update_spy(self, X_full, y_full):
        out = real_update(self, X_full, y_full)
        absorbed.append(out)
        return out

    monkeypatch.setattr(gp_mod.GPRegressor, "update_data", update_spy)

    warnings.simplefilter("ignore")
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    choices = ["adam", "sgd", "rmsprop"]
    dists = {
        "x0": FloatDistribution(0.0, 1.0),
        "x1": FloatDistribution(0.0, 1.0),
        "layers": IntDistribution(1, 8),
        "opt": CategoricalDistribution(choices),
    }

    def value(p) -> float:
        return (
            (p["x0"] - 0.3) ** 2 + (p["x1"] - 0.7) ** 2 + 0.05 * (p["layers"] - 4) ** 2
            + 0.2 * choices.index(p["opt"])
        )

    rng = np.random.RandomState(4)
    sampler = optuna_amd.samplers.GPSampler(seed=0)
    study = optuna_amd.create_study(sampler=sampler)
    history = [
        {
            "x0": float(rng.rand()), "x1": float(rng.rand()),
            "layers": int(rng.randint(1, 9)), "opt": choices[rng.randint(3)],
        }
        for _ in range(80)
    ]
    study.add_trials(
        [optuna_amd.create_trial(params=p, distributions=dists, value=value(p)) for p in history]
    )

    def step() -> dict:
        trial = study.ask()
        p = {
            "x0": trial.suggest_float("x0", 0.0, 1.0),
            "x1": trial.suggest_float("x1", 0.0, 1.0),
            "layers": trial.suggest_int("layers", 1, 8),
            "opt": trial.suggest_categorical("opt", choices),
        }
        study.tell(trial, value(p))
        return p

    suggestions = [step()]
    gpr = sampler._gprs_cache_list[0]
    assert gpr.device.type == "cuda" and gpr._squared_X_diff is None
    mask = acqf_mod._cat_mask(gpr._is_categorical)
    assert bin(mask).count("1") == 1
    assert sessions and all(s is not None for s in sessions)
    assert constructed and all(m == mask for m in constructed)
    assert absorbed == []

    suggestions.append(step())
    assert absorbed == [True]
    assert len(study.trials) == 82
    for p in suggestions:
        assert 0.0 <= p["x0"] <= 1.0 and 0.0 <= p["x1"] <= 1.0
        assert isinstance(p["layers"], int) and 1 <= p["layers"] <= 8
        assert p["opt"] in choices
