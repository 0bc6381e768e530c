"""Box decomposition of the non-dominated region for (q)LogEHVI.

Implements Lacour-Klamroth-Fonseca "A Box Decomposition Algorithm to Compute the
Hypervolume Indicator" (arXiv:1510.01963): Algorithm 2 maintains the upper-bound
set U(N) with its defining points; applying it twice (once on the sign-flipped
upper-bound set) yields a partition of the *non-dominated* region into boxes,
which is what EHVI integrates over.

Parity: reference ``optuna/_hypervolume/box_decomposition.py`` (BoTorch-derived:
_get_upper_bound_set :30, _get_box_bounds :96, get_non_dominated_box_bounds
:138). Minimization convention throughout.
"""
from __future__ import annotations

import os
import warnings

import numpy as np

from optuna_amd.study._multi_objective import _is_pareto_front


def _update_upper_bounds(
    sol: np.ndarray,
    ubs: np.ndarray,
    dps: np.ndarray,
    first_dim_always_updates: np.ndarray,
) -> tuple[np.ndarray, np.ndarray]:
    """One Alg.-2 insertion: replace the bounds strictly dominated by ``sol``.

    ubs: (n_bounds, k) current upper-bound set; dps: (n_bounds, k, k) defining
    points (dps[i, j] is z^j of ubs[i]).
    """
    k = sol.shape[0]
    strictly_below = np.all(sol < ubs, axis=-1)
    if not strictly_below.any():
        return ubs, dps

    kept_ubs = ubs[~strictly_below]
    kept_dps = dps[~strictly_below]
    hit_ubs = ubs[strictly_below]
    hit_dps = dps[strictly_below]

    new_ubs_list = []
    new_dps_list = []
    # max over defining points z^i (i != j) of their j-th coordinate; the first
    # objective always passes because solutions arrive sorted by it (Alg. 2 line 2).
    masked = np.where(first_dim_always_updates, -np.inf, hit_dps)
    thresholds = masked.max(axis=-2)  # (n_hit, k)
    for u_idx in range(len(hit_ubs)):
        for j in range(k):
            if sol[j] >= thresholds[u_idx, j]:
                u_new = hit_ubs[u_idx].copy()
                u_new[j] = sol[j]
                d_new = hit_dps[u_idx].copy()
                d_new[j] = sol
                new_ubs_list.append(u_new)
                new_dps_list.append(d_new)

    if new_ubs_list:
        ubs_out = np.vstack([kept_ubs, np.asarray(new_ubs_list)])
        dps_out = np.vstack([kept_dps, np.asarray(new_dps_list).reshape(-1, k, k)])
    else:
        ubs_out, dps_out = kept_ubs, kept_dps
    return ubs_out, dps_out


def _get_upper_bound_set(
    sorted_pareto_sols: np.ndarray, ref_point: np.ndarray
) -> tuple[np.ndarray, np.ndarray]:
    """U(N) and its defining points for pareto solutions sorted by objective 0."""
    _, k = sorted_pareto_sols.shape
    # mask[i, j] True → skip the inequality for defining-point row i, column j.
    mask = np.eye(k, dtype=bool)
    mask[:, 0] = True

    ubs = np.asarray([ref_point])
    dps = np.full((1, k, k), -np.inf)
    dps[0, np.arange(k), np.arange(k)] = ref_point  # dummy points \hat{z}^k
    for sol in sorted_pareto_sols:
        ubs, dps = _update_upper_bounds(sol, ubs, dps, mask)
    return ubs, dps


def _get_box_bounds(
    upper_bound_set: np.ndarray, def_points: np.ndarray, ref_point: np.ndarray
) -> np.ndarray:
    """Eq. (2) of Lacour17: per-bound boxes [l, u]; empty boxes dropped."""
    k = upper_bound_set.shape[-1]
    assert k > 1, "box decomposition requires n_objectives > 1"
    lower = np.empty_like(upper_bound_set)
    upper = np.empty_like(upper_bound_set)
    lower[:, 0] = def_points[:, 0, 0]
    upper[:, 0] = ref_point[0]
    running_max = np.maximum.accumulate(def_points, axis=-2)
    for j in range(1, k):
        lower[:, j] = running_max[:, j - 1, j]
        upper[:, j] = upper_bound_set[:, j]
    keep = ~np.any(upper <= lower, axis=-1)
    return np.stack([lower[keep], upper[keep]])


def get_non_dominated_box_bounds(
    loss_vals: np.ndarray, ref_point: np.ndarray
) -> tuple[np.ndarray, np.ndarray]:
    """Partition the non-dominated region below ``ref_point`` into boxes.

    Returns (lower_bounds, upper_bounds), each (n_boxes, n_objectives).
    """
    assert np.all(np.isfinite(loss_vals)), "loss_vals must be clipped before box decomposition."
    uniq = np.unique(loss_vals, axis=0)
    sorted_pareto_sols = uniq[_is_pareto_front(uniq, assume_unique_lexsorted=True)]
    k = loss_vals.shape[-1]
    assert k > 1, "box decomposition requires n_objectives > 1"
    if k > 4:
        warnings.warn(
            "Box decomposition (typically used by `GPSampler`) might be significantly "
            "slow for n_objectives > 4. Please consider using another sampler instead."
        )

    # Dual trick: the sign-flipped upper-bound set of U(N) partitions the
    # non-dominated region (see Lacour17 §3 / the reference's derivation).
    neg_ubs = -_get_upper_bound_set(sorted_pareto_sols, ref_point)[0]
    neg_ubs_sorted = np.unique(neg_ubs, axis=0)
    inf_point = np.full_like(ref_point, np.inf)
    neg_lower_set, neg_dps = _get_upper_bound_set(
        neg_ubs_sorted[_is_pareto_front(neg_ubs_sorted, assume_unique_lexsorted=True)],
        inf_point,
    )
    box_upper, box_lower = -_get_box_bounds(neg_lower_set, neg_dps, inf_point)
    return box_lower, box_upper


_INTERVAL_EPS = 1e-12  # the acquisition's clamp: a zero interval has a NaN gradient

# Fewest rows (base rows below the reference point plus a draw's own rows) per
# number of objectives from which the device decomposes: the smallest sizes of
# scripts/box_decomposition_timing.py (docs/PERF.md, "Box decomposition on the
# device"), 16 + 8 rows for two objectives and 4 + 8 for three and four. The
# device won there by 4.8x, 4.3x and 6.8x with one draw, and by more at every
# larger size and with 128 draws; nothing smaller was measured.
_DEVICE_BOXES_MIN_ROWS = {2: 24, 3: 12, 4: 12}


def _boxes_host(
    base_losses: np.ndarray, extra_rows: np.ndarray, ref_point: np.ndarray
) -> tuple[np.ndarray, np.ndarray]:
    """Max-space (lower, intervals) of one draw: the acquisition's ``_get_boxes``."""
    losses = np.concatenate([base_losses, extra_rows], axis=0)
    kept = losses[(losses < ref_point).all(axis=-1)]
    front = kept[_is_pareto_front(kept, assume_unique_lexsorted=False)]
    box_lo, box_hi = get_non_dominated_box_bounds(front, ref_point)
    # Negating swaps the roles of the bounds.
    lower, upper = -box_hi, -box_lo
    return lower, np.maximum(upper - lower, _INTERVAL_EPS)


def _boxes_device(
    base_losses: np.ndarray, extra_losses: np.ndarray, ref_point: np.ndarray
) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray] | None:
    """K6e HIP path: every draw's boxes in one launch train (or None)."""
    n_objectives = ref_point.shape[0]
    n_rows = base_losses.shape[0] + extra_losses.shape[1]
    if (
        os.environ.get("OPTUNA_AMD_GP_BOXES_DEVICE", "1") == "0"
        or n_objectives not in _DEVICE_BOXES_MIN_ROWS
        or n_rows < _DEVICE_BOXES_MIN_ROWS[n_objectives]
        or not (np.isfinite(base_losses).all() and np.isfinite(extra_losses).all())
        or not np.isfinite(ref_point).all()
    ):
        return None
    from optuna_amd import _hip

    core = _hip.get()
    if core is None or not core.available():
        return None
    return core.box_decompose(base_losses, extra_losses, ref_point)


def get_non_dominated_boxes_batched(
    base_losses: np.ndarray, extra_losses: np.ndarray, ref_point: np.ndarray
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Boxes of the non-dominated region of ``base | extra[q]`` for every draw q.

    base_losses: (n0, k) rows shared by the draws; extra_losses: (Q, R, k), the
    rows of each draw (R may be 0); all in loss (minimization) space. Returns
    packed max-space ``(lower, intervals, offsets)``: the boxes of draw q are
    rows ``offsets[q]:offsets[q + 1]``, the same set as the acquisition's
    per-draw decomposition of ``concatenate([base, extra[q]])`` with the
    intervals clamped to 1e-12. The order of a draw's boxes depends on the
    route (host or device) and is the same from run to run.
    """
    base_losses = np.ascontiguousarray(base_losses, dtype=np.float64)
    extra_losses = np.ascontiguousarray(extra_losses, dtype=np.float64)
    ref_point = np.ascontiguousarray(ref_point, dtype=np.float64)
    n_draws, _, k = extra_losses.shape
    assert base_losses.ndim == 2 and base_losses.shape[1] == k == ref_point.shape[0]

    kept = base_losses[(base_losses < ref_point).all(axis=-1)]
    # The device reduces the rows to their front itself, per draw.
    device = _boxes_device(kept, extra_losses, ref_point)
    if device is not None and len(device[3]) == 0:
        return device[:3]
    # The front of base | extra[q] is the front of front(base) | extra[q]: the
    # host reduces the base once for all draws.
    base_front = kept[_is_pareto_front(kept, assume_unique_lexsorted=False)]
    if device is None:
        per_draw = [_boxes_host(base_front, extra_losses[q], ref_point) for q in range(n_draws)]
    else:
        lower, intervals, offsets, host_needed = device
        per_draw = [
            (lower[offsets[q] : offsets[q + 1]], intervals[offsets[q] : offsets[q + 1]])
            for q in range(n_draws)
        ]
        for q in host_needed:
            per_draw[q] = _boxes_host(base_front, extra_losses[q], ref_point)
    offsets = np.concatenate([[0], np.cumsum([len(lo) for lo, _ in per_draw])]).astype(np.int64)
    return (
        np.concatenate([lo for lo, _ in per_draw], axis=0).reshape(-1, k),
        np.concatenate([iv for _, iv in per_draw], axis=0).reshape(-1, k),
        offsets,
    )
