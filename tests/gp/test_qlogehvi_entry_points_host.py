"""On CPU GPs ``qLogEHVI`` has no session and its numpy entry points are the base class's."""
import numpy as np
import torch

from optuna_amd._gp import acqf as acqf_mod, gp, prior, search_space as gp_ss
from optuna_amd.distributions import FloatDistribution


def test_cpu_gps_keep_the_torch_path() -> None:
    d, rng = 3, np.random.RandomState(0)
    X = rng.rand(30, d)
    Y = np.stack([-np.sum(np.square(X - c), axis=1) + 0.1 * rng.randn(30) for c in (0.3, 0.7)], -1)
    gprs = [
        gp.fit_kernel_params(X, y, np.zeros(d, bool), prior.default_log_prior, 1e-6, False)
        for y in Y.T
    ]
    space = gp_ss.SearchSpace({f"x{i}": FloatDistribution(0.0, 1.0) for i in range(d)})
    acqf = acqf_mod.qLogEHVI(
        gprs, space, torch.from_numpy(Y), rng.rand(2, d), n_qmc_samples=16, qmc_seed=5
    )
    assert acqf._fused_session() is None
    assert len(acqf._box_counts) == 16 and max(acqf._box_counts) == acqf._box_lower.shape[1]
    base, cands = acqf_mod.BaseAcquisitionFunc, rng.rand(5, d)
    np.testing.assert_array_equal(acqf.eval_acqf_no_grad(cands), base.eval_acqf_no_grad(acqf, cands))
    for got, want in zip(
        acqf.eval_acqf_batched_with_grad(cands) + acqf.eval_acqf_with_grad(cands[1]),
        base.eval_acqf_batched_with_grad(acqf, cands) + base.eval_acqf_with_grad(acqf, cands[1]),
    ):
        np.testing.assert_array_equal(got, want)
