"""Batch sizes at the ends of what ``GpLogEiSession.eval`` takes.

The session evaluates the whole batch as one chunk, one candidate per ``y`` of
``k_gp_cross_cov``'s grid, so it takes 1..65535 candidates. No candidates give
empty arrays without a launch, and one more than the grid holds is refused on
the host, with or without ``constraints=``, as the two chunking sessions have
always done for an empty batch.
"""
from __future__ import annotations

import numpy as np
import pytest

from optuna_amd import _hip


pytestmark = pytest.mark.gpu

N, D = 1, 2


def test_logei_session_empty_and_oversized_batches() -> None:
    import torch

    core = _hip.require()
    if core is None or not core.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    dev = torch.device("cuda")
    X = torch.full((N, D), 0.5, dtype=torch.float64, device=dev)
    eta = torch.ones(D, dtype=torch.float64, device=dev)
    alpha = torch.ones(N, dtype=torch.float64, device=dev)
    cinv = torch.full((N, N), 0.5, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    sess = core.GpLogEiSession(
        X.data_ptr(), alpha.data_ptr(), cinv.data_ptr(), eta.data_ptr(), N, D, 1.0, 1e-12, 0.1
    )
    ptrs = ([X.data_ptr()], [alpha.data_ptr()], [cinv.data_ptr()], [eta.data_ptr()])
    cs = core.GpConstraintSet(*ptrs, [1.0], [0.0], N, D, 1e-12)

    for constraints in (None, cs):
        f, g = sess.eval(np.empty((0, D)), True, constraints=constraints)
        assert np.asarray(f).shape == (0,) and np.asarray(g).shape == (0, D)
        f, g = sess.eval(np.empty((0, D)), False, constraints=constraints)
        assert np.asarray(f).shape == (0,) and np.asarray(g).size == 0
        with pytest.raises(RuntimeError, match="65535"):
            sess.eval(np.zeros((65536, D)), False, constraints=constraints)

    # The largest batch is taken, and every row of it is the single-row result.
    x = np.tile(np.array([[0.25, 0.75]]), (65535, 1))
    f, g = sess.eval(x, True)
    f1, g1 = sess.eval(x[:1].copy(), True)
    assert np.asarray(f).shape == (65535,) and np.asarray(g).shape == (65535, D)
    assert np.isfinite(f1).all() and np.isfinite(g1).all()
    np.testing.assert_array_equal(f, np.repeat(f1, 65535))
    np.testing.assert_array_equal(g, np.repeat(g1, 65535, axis=0))
