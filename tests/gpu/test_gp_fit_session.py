"""``GpFitSession`` (build_cov, torch's factorisation, grad) against
``GPRegressor._loss_and_grad_numpy`` on the explicit (N, N, D) squared-difference
tensor (Hamming indicator on the categorical columns), at the tolerances of
``tests/gp/test_gp.py``: the loss to rel 1e-8, the gradient to rtol 1e-6 / atol 1e-8,
the covariance to 1e-12. The deterministic cases (noise = 1e-6) sit at D >= 16: at
D = 1 the 129 x 129 covariance has a condition number near 1e8 there and LAPACK's
own inverse is not good to 1e-6."""
import numpy as np
import pytest
import torch

from optuna_amd import _hip
from optuna_amd._gp import gp as gp_mod, prior


pytestmark = pytest.mark.gpu

MIN_NOISE = 1e-6
MASKS = {"none": lambda D: [], "mid": lambda D: [D // 2], "ends": lambda D: sorted({0, D - 1})}
# Every N at D = 17 unmixed; every D and mask at N = 129; the noise-free objective
# alternates through the D >= 16 cases.
CASES = [(N, 17, "none", N in (2, 64, 200)) for N in (1, 2, 63, 64, 65, 200)] + [
    (129, D, mask, D >= 16 and k % 2 == 0)
    for D in (1, 16, 17, 64)
    for k, mask in enumerate(MASKS)
]


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    assert c is not None and c.available(), "the HIP extension must run here: no fallback"
    return c


def _problem(N, D, mask):
    rng = np.random.RandomState(1000 * N + 10 * D + len(mask))
    cat = MASKS[mask](D)
    X = rng.rand(N, D)
    X[:, cat] = rng.randint(0, 3, size=(N, len(cat)))
    y = np.sum((X - 0.3) ** 2, axis=1) + 0.05 * rng.randn(N)
    y = (y - y.mean()) / y.std() if N > 1 else y
    raw = np.concatenate([np.zeros(D + 1), [np.log(1.0 - 0.99 * MIN_NOISE)]])
    raw = raw + rng.uniform(-0.5, 0.5, D + 2)
    sqd = (X[:, None, :] - X[None, :, :]) ** 2
    sqd[..., cat] = sqd[..., cat] > 0.0
    is_cat = np.zeros(D, dtype=bool)
    is_cat[cat] = True
    ones = torch.ones(D + 2, dtype=torch.float64)
    gpr = gp_mod.GPRegressor(
        torch.from_numpy(is_cat), torch.from_numpy(X), torch.from_numpy(y),
        ones[:D], ones[D], ones[D + 1],
    )
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    session = _hip.require().GpFitSession(
        Xd.data_ptr(), yd.data_ptr(), N, D, cat_mask=sum(1 << d for d in cat)
    )
    return gpr, session, Xd, yd, raw, sqd, y


def _evaluate(session, Xd, yd, raw, det, calls=1):
    C = torch.empty((len(yd), len(yd)), dtype=torch.float64, device="cuda")
    session.build_cov(raw, MIN_NOISE, det, C.data_ptr())
    L = torch.linalg.cholesky(C)
    alpha = torch.cholesky_solve(yd.unsqueeze(-1), L)[:, 0].contiguous()
    Cinv = torch.cholesky_inverse(L)
    torch.cuda.current_stream().synchronize()
    ptrs = (L.data_ptr(), alpha.data_ptr(), Cinv.data_ptr())
    return C, [session.grad(raw, MIN_NOISE, det, *ptrs) for _ in range(calls)]


def _deviation(loss, grad, loss_ref, grad_ref):
    """(relative loss error, largest gradient error over its allowance 1e-8 + 1e-6 |ref|)."""
    return (
        abs(loss - loss_ref) / abs(loss_ref),
        float(np.max(np.abs(grad - grad_ref) / (1e-8 + 1e-6 * np.abs(grad_ref)))),
    )


@pytest.mark.parametrize("N,D,mask,det", CASES)
def test_loss_and_gradient_match_numpy(core, N, D, mask, det):
    gpr, session, Xd, yd, raw, sqd, y = _problem(N, D, mask)
    loss_ref, grad_ref = gpr._loss_and_grad_numpy(raw, sqd, y, MIN_NOISE, det)
    _, [(loss, grad)] = _evaluate(session, Xd, yd, raw, det)
    torch_dev = _deviation(
        *gpr._loss_and_grad_closed_form_torch(raw, Xd, yd, MIN_NOISE, det), loss_ref, grad_ref
    )
    fused_dev = _deviation(loss, grad, loss_ref, grad_ref)
    print(f"\nDEV N={N} D={D} {mask} det={det}: fused loss {fused_dev[0]:.1e} grad "
          f"{fused_dev[1]:.1e} | torch loss {torch_dev[0]:.1e} grad {torch_dev[1]:.1e}")
    assert loss == pytest.approx(loss_ref, rel=1e-8)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-6, atol=1e-8)
    if det:
        assert grad[-1] == 0.0


@pytest.mark.parametrize("mask", ["none", "ends"])
def test_build_cov_matches_closed_form_and_is_symmetric(core, mask):
    N, D = 65, 17
    _, session, Xd, yd, raw, sqd, _ = _problem(N, D, mask)
    C, _ = _evaluate(session, Xd, yd, raw, False)
    C = C.cpu().numpy()
    r2 = sqd @ np.exp(raw[:D])
    u = np.sqrt(5.0 * r2)
    ref = np.exp(raw[D]) * np.exp(-u) * ((5.0 / 3.0) * r2 + u + 1.0)
    ref += (np.exp(raw[D + 1]) + MIN_NOISE) * np.eye(N)
    np.testing.assert_allclose(C, ref, rtol=1e-12, atol=1e-12)
    assert np.array_equal(C, C.T)


def test_grad_is_deterministic(core):
    _, session, Xd, yd, raw, _, _ = _problem(129, 17, "mid")
    _, [(loss_a, grad_a), (loss_b, grad_b)] = _evaluate(session, Xd, yd, raw, False, calls=2)
    assert np.float64(loss_a).tobytes() == np.float64(loss_b).tobytes()
    assert grad_a.tobytes() == grad_b.tobytes()


@pytest.mark.parametrize("order", ["C", "F"])
def test_fit_routes_through_the_session(core, monkeypatch, order):
    """A Fortran-ordered X reaches the device strided: the session reads a copy."""
    rng = np.random.RandomState(5)
    n, d = 600, 5
    X = np.asarray(rng.rand(n, d), order=order)
    Y = np.sum((X - 0.3) ** 2, axis=1) + 0.05 * rng.randn(n)
    Y = (Y - Y.mean()) / Y.std()
    calls = {"build_cov": 0, "grad": 0}

    class Counting:
        def __init__(self, *args, **kwargs):
            self._inner = core.GpFitSession(*args, **kwargs)

        def build_cov(self, *args):
            calls["build_cov"] += 1
            return self._inner.build_cov(*args)

        def grad(self, *args):
            calls["grad"] += 1
            return self._inner.grad(*args)

    class Core:
        GpFitSession = Counting

        def __getattr__(self, name):
            return getattr(core, name)

    monkeypatch.setattr(_hip, "get", lambda: Core())

    def fit():
        return gp_mod.fit_kernel_params(
            X, Y, np.zeros(d, dtype=bool), prior.default_log_prior, MIN_NOISE, False
        )

    fused = fit()
    assert calls["build_cov"] == calls["grad"] > 0
    seen = dict(calls)
    monkeypatch.setenv("OPTUNA_AMD_GP_FUSED_FIT", "0")
    plain = fit()
    assert calls == seen
    np.testing.assert_allclose(
        fused.inverse_squared_lengthscales.cpu().numpy(),
        plain.inverse_squared_lengthscales.cpu().numpy(),
        rtol=1e-4,
    )
    np.testing.assert_allclose(fused.kernel_scale.item(), plain.kernel_scale.item(), rtol=1e-4)
    np.testing.assert_allclose(fused.noise_var.item(), plain.noise_var.item(), rtol=1e-3)
