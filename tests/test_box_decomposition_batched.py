"""The host route of ``get_non_dominated_boxes_batched`` against the acquisition's
per-draw ``_get_boxes`` loop."""
import numpy as np
import pytest
import torch

from optuna_amd._gp import acqf as acqf_mod
from optuna_amd._hypervolume.box_decomposition import get_non_dominated_boxes_batched


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("R", [0, 2])
def test_host_route_equals_the_per_draw_loop(monkeypatch, M: int, R: int) -> None:
    monkeypatch.setenv("OPTUNA_AMD_GP_BOXES_DEVICE", "0")
    rng = np.random.RandomState(10 * M + R)
    base = np.round(rng.uniform(0.1, 1.2, (30, M)), 2)  # ties, dominated rows, rows past ref
    base[25:] = base[:5]
    extra = rng.uniform(0.05, 1.2, (3, R, M))
    ref = np.ones(M)
    lo, iv, offsets = get_non_dominated_boxes_batched(base, extra, ref)
    assert offsets[0] == 0 and offsets[-1] == len(lo) == len(iv)
    for q in range(3):
        Y = torch.from_numpy(-np.concatenate([base, extra[q]]))
        want_lo, want_up = acqf_mod._get_boxes(Y, ref)
        part = slice(offsets[q], offsets[q + 1])
        np.testing.assert_array_equal(lo[part], want_lo.numpy())
        np.testing.assert_array_equal(iv[part], (want_up - want_lo).clamp_min_(1e-12).numpy())
