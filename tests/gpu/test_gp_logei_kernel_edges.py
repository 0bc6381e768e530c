"""``GpLogEiSession`` (``k_gp_cross_cov<false>``, the dgemm, ``k_gp_logei_final``)
at its edges, against two references:

* the mpmath golden problems of ``tests/golden/gp_logei_edges.json``
  (``scripts/gen_gp_logei_golden.py``), which depend on neither the kernel nor
  the host formula it mirrors: z on both sides of -1 and of the series cut, a
  candidate on a training row, cross-covariances that underflow, a masked
  column, a clamped variance (``raw < 0``) and the left tail down to z = -1e8;
* the torch formulation of ``optuna_amd/_gp/acqf.py`` with autograd, at kernel
  scale: N on both sides of the 256-thread block and two blocks, D = 1 and the
  maximum 64, one candidate and seven, and a clamped variance at N = 64.

Tolerances are the project's: rtol 1e-8 / atol 1e-10 on the value, rtol 1e-6 /
atol 1e-8 on the gradient. The golden cases are admissible at them by
construction (see the generator); the synthetic ones fit no GP and take the
inverse of the Matern matrix plus 0.1 I, as the sibling suites do.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

from optuna_amd import _hip


pytestmark = pytest.mark.gpu

F_TOL = dict(rtol=1e-8, atol=1e-10)
G_TOL = dict(rtol=1e-6, atol=1e-8)
STAB = 1e-12

_GOLDEN_PATH = Path(__file__).resolve().parent.parent / "golden" / "gp_logei_edges.json"
_SESSION = json.loads(_GOLDEN_PATH.read_text())["session"]
_GP_NAMES = sorted({c["gp"] for c in _SESSION})


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


# ---- 1. the golden problems ------------------------------------------------------------


class _GoldenGp:
    """The GP of a golden case as small device tensors, and sessions over it."""

    def __init__(self, case: dict) -> None:
        import torch

        def up(values):
            return torch.tensor(values, dtype=torch.float64).cuda().contiguous()

        self.case = case
        self.X, self.alpha = up(case["X"]), up(case["alpha"])
        self.cinv, self.eta = up(case["cinv"]), up(case["eta"])
        torch.cuda.synchronize()

    def session(self, core, threshold: float):
        c = self.case
        return core.GpLogEiSession(
            self.X.data_ptr(), self.alpha.data_ptr(), self.cinv.data_ptr(),
            self.eta.data_ptr(), c["N"], c["D"], c["scale"], c["stab"], threshold,
            cat_mask=c["cat_mask"],
        )


def _check_golden_rows(f0, g0, f1, g1, cases: list[dict], rows: list[int], B: int) -> None:
    """Rows ``rows`` of both evaluations of a batch of B against their cases."""
    f0, f1, g1 = np.asarray(f0), np.asarray(f1), np.asarray(g1)
    D = cases[0]["D"]
    assert f0.shape == (B,) and f1.shape == (B,) and np.asarray(g0).size == 0
    assert g1.shape == (B, D)
    np.testing.assert_array_equal(f0, f1)
    for row, case in zip(rows, cases):
        label = case["name"]
        assert np.isfinite(f1[row]) and np.isfinite(g1[row]).all(), label
        np.testing.assert_allclose(f1[row], case["f"], err_msg=label, **F_TOL)
        np.testing.assert_allclose(g1[row], np.array(case["grad"]), err_msg=label, **G_TOL)
        for d in range(D):
            if (case["cat_mask"] >> d) & 1:
                assert g1[row, d] == 0.0 and case["grad"][d] == 0.0, label


@pytest.mark.parametrize("case", _SESSION, ids=[c["name"] for c in _SESSION])
def test_golden_case(core, case: dict) -> None:
    gp = _GoldenGp(case)
    sess = gp.session(core, case["threshold"])
    x = np.array([case["x"]], dtype=np.float64)
    f0, g0 = sess.eval(x, with_grad=False)
    f1, g1 = sess.eval(x, with_grad=True)
    _check_golden_rows(f0, g0, f1, g1, [case], [0], 1)


@pytest.mark.parametrize("gp_name", _GP_NAMES)
def test_golden_cases_of_one_gp_as_one_batch(core, gp_name: str) -> None:
    """All candidates of the cases that share a GP go through as one batch, once
    per threshold among them; the rows whose case has that threshold are checked.
    The other rows are valid inputs that only travel along."""
    cases = [c for c in _SESSION if c["gp"] == gp_name]
    gp = _GoldenGp(cases[0])
    x = np.array([c["x"] for c in cases], dtype=np.float64)
    B = len(cases)
    assert B >= 2
    for threshold in sorted({c["threshold"] for c in cases}):
        rows = [i for i, c in enumerate(cases) if c["threshold"] == threshold]
        sess = gp.session(core, threshold)
        f0, g0 = sess.eval(x, with_grad=False)
        f1, g1 = sess.eval(x, with_grad=True)
        _check_golden_rows(f0, g0, f1, g1, [cases[i] for i in rows], rows, B)


# ---- 2. kernel-scale shapes against torch ----------------------------------------------


def _matern(x, X, eta, scale):
    """scale * Matern-5/2 of the ARD distance, (B, N); differentiable in x."""
    from optuna_amd._gp import gp as gp_mod

    r2 = ((x.unsqueeze(-2) - X.unsqueeze(-3)).square() * eta).sum(-1)
    return gp_mod.matern52_of_sqdist(r2) * scale


class _Gp:
    """One synthetic GP: random X, alpha ~ N(0, 1/N), the inverse of Matern + 0.1 I."""

    def __init__(self, N: int, D: int, seed: int, device: str = "cuda") -> None:
        import torch

        dev = torch.device(device)
        g = torch.Generator().manual_seed(seed)
        self.N, self.D, self._seed = N, D, seed
        self.X = torch.rand(N, D, generator=g, dtype=torch.float64).to(dev)
        self.eta = ((0.5 + torch.rand(D, generator=g, dtype=torch.float64)) * (2.0 / D)).to(dev)
        self.scale = float(0.5 + torch.rand(1, generator=g, dtype=torch.float64))
        # 1 / sqrt(N) keeps the posterior mean of order one.
        self.alpha = (torch.randn(N, generator=g, dtype=torch.float64) / np.sqrt(N)).to(dev)
        C = _matern(self.X, self.X, self.eta, self.scale)
        C = C + 0.1 * torch.eye(N, dtype=torch.float64, device=dev)
        self.cinv = torch.linalg.inv(C).contiguous()
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def candidates(self, B: int) -> np.ndarray:
        rng = np.random.RandomState(self._seed + 17)
        x = rng.rand(B, self.D)
        if B > 1:
            x[B - 1] = self.X[rng.randint(self.N)].cpu().numpy()  # a training row: r2 = 0
        return x

    def posterior(self, x):
        """(mean, raw variance before the clamp), as GPRegressor.posterior."""
        import torch

        K = _matern(x, self.X, self.eta, self.scale)
        mean = torch.linalg.vecdot(K, self.alpha)
        raw = self.scale - torch.linalg.vecdot(K, K.matmul(self.cinv))
        return mean, raw

    def place_threshold(self, x_np: np.ndarray, k: float) -> float:
        """median(mean) + k median(sigma) over the batch: z is about -k."""
        import torch

        with torch.no_grad():
            mean, raw = self.posterior(torch.from_numpy(x_np).to(self.X.device))
            sigma = torch.sqrt(raw.clamp_min(0.0) + STAB)
            return float(mean.median() + k * sigma.median())

    def reference(self, x_np: np.ndarray, threshold: float):
        """(f, grad, z, raw) of acqf.logei over the clamped posterior, by autograd."""
        import torch

        from optuna_amd._gp import acqf as acqf_mod

        x = torch.from_numpy(x_np).to(self.X.device).requires_grad_(True)
        mean, raw = self.posterior(x)
        var = raw.clamp_min(0.0) + STAB
        f = acqf_mod.logei(mean=mean, var=var, f0=threshold)
        f.sum().backward()
        z = ((mean - threshold) / torch.sqrt(var)).detach()
        return (
            f.detach().cpu().numpy(), x.grad.cpu().numpy(), z.cpu().numpy(),
            raw.detach().cpu().numpy(),
        )

    def session(self, core, threshold: float):
        # cat_mask left out: the unmixed cross-covariance instantiation.
        return core.GpLogEiSession(
            self.X.data_ptr(), self.alpha.data_ptr(), self.cinv.data_ptr(),
            self.eta.data_ptr(), self.N, self.D, self.scale, STAB, threshold,
        )


def _check_against_torch(core, gp: _Gp, x: np.ndarray, threshold: float, label: str):
    want_f, want_g, z, raw = gp.reference(x, threshold)
    sess = gp.session(core, threshold)
    f0, g0 = sess.eval(x, with_grad=False)
    f1, g1 = sess.eval(x, with_grad=True)
    f0, f1, g1 = np.asarray(f0), np.asarray(f1), np.asarray(g1)
    B = len(x)
    assert f0.shape == (B,) and np.asarray(g0).size == 0, label
    assert g1.shape == (B, gp.D), label
    assert np.isfinite(want_f).all() and np.isfinite(want_g).all(), label
    np.testing.assert_array_equal(f0, f1, err_msg=label)
    np.testing.assert_allclose(f1, want_f, err_msg=label, **F_TOL)
    np.testing.assert_allclose(g1, want_g, err_msg=label, **G_TOL)
    return want_g, z, raw


@pytest.mark.parametrize("D", [1, 64])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_session_matches_torch_on_synthetic_inputs(core, N: int, D: int) -> None:
    for B in (1, 7):
        gp = _Gp(N, D, seed=10 * N + D + B)
        x = gp.candidates(B)
        zs = []
        for k in (-2.0, 3.0):  # z about +2 and about -3: both branches
            label = f"N={N} D={D} B={B} k={k}"
            threshold = gp.place_threshold(x, k)
            want_g, z, _ = _check_against_torch(core, gp, x, threshold, label)
            # The gradient check is not a comparison of zeros.
            assert np.abs(want_g).max() > 1e-6, label
            zs.append(z)
        zs = np.concatenate(zs)
        assert zs.min() < -1.0 < zs.max()


# ---- 3. clamped variance at kernel scale -----------------------------------------------


def test_clamped_variance_passes_no_gradient(core) -> None:
    """An inverse that overshoots drives scale - K Cinv K below zero: sigma sits
    on sqrt(stab), and like autograd through clamp_min(0) the closed form sends
    nothing through the variance (a w_v taken from the formula is phi/h / (2 stab),
    1e11 and more times the true gradient).

    With sigma = 1e-6 the z of a batch spread by (mean_b - t) / 1e-6. The means
    are scaled down to that order so that |z| stays below 1e3 and the rounding
    of the reference's own mean (1e-16 relative, times 1e6) stays out of the
    comparison."""
    import torch

    gp = _Gp(64, 3, seed=93)
    gp.cinv = (50.0 * torch.eye(64, dtype=torch.float64, device="cuda")).contiguous()
    gp.alpha = (1e-5 * gp.alpha).contiguous()
    torch.cuda.synchronize()
    x = gp.candidates(4)
    zs, moved = [], 0.0
    for k in (-6.0, 0.0, 30.0):
        threshold = gp.place_threshold(x, k)
        want_g, z, raw = _check_against_torch(core, gp, x, threshold, f"clamped k={k}")
        assert (raw < 0).all()
        zs.append(z)
        moved = max(moved, float(np.abs(want_g).max()))
    zs = np.concatenate(zs)
    assert np.abs(zs).max() < 1e3 and zs.min() < -20.0 and zs.max() > 4.0
    assert moved > 1e-6
