"""Host reference for the fused LogEHVI kernel: the value and the two
posterior-side gradient weights, from the posterior moments alone.

Plain numpy broadcasts over the full (Q, J, M) tensor, so it is only meant for
test-sized inputs. It shares no code with the device kernel (which streams the
pairs with an online log-sum-exp) and none with ``acqf.logehvi`` (torch).
"""
from __future__ import annotations

import numpy as np


EPS = 1e-12


def logehvi_reference(
    mean: np.ndarray,  # (M,) posterior mean per objective
    sd: np.ndarray,  # (M,) posterior standard deviation, sqrt(var + stab)
    eps: np.ndarray,  # (Q, M) fixed QMC normals
    lo: np.ndarray,  # (J, M) box lower bounds
    iv: np.ndarray,  # (J, M) box intervals
) -> tuple[float, np.ndarray, np.ndarray]:
    """Return ``(f, wm, wv)`` for one candidate.

    ``f = logsumexp_{q,j} sum_m log d[q,j,m] - log Q`` with
    ``d = min(max(y - lo, EPS), iv)`` and ``y[q,m] = mean_m + sd_m eps[q,m]``;
    ``wm_m = df/dmean_m`` and ``wv_m = df/dvar_m`` where ``var_m = sd_m**2``.
    Clamped terms carry no gradient; at an exact tie (``y - lo`` equal to EPS or
    to ``iv``) the one-sided choice made here is not meaningful.
    """
    mean = np.asarray(mean, dtype=np.float64)
    sd = np.asarray(sd, dtype=np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    lo = np.asarray(lo, dtype=np.float64)
    iv = np.asarray(iv, dtype=np.float64)
    n_q = eps.shape[0]

    y = mean[None, :] + sd[None, :] * eps  # (Q, M)
    diff = y[:, None, :] - lo[None, :, :]  # (Q, J, M)
    d = np.minimum(np.maximum(diff, EPS), iv[None, :, :])
    t = np.log(d).sum(axis=-1)  # (Q, J)
    t_max = t.max()
    total = np.exp(t - t_max).sum()
    f = float(t_max + np.log(total) - np.log(n_q))

    w = np.exp(t - t_max) / total  # (Q, J), sums to 1
    free = (diff > EPS) & (diff < iv[None, :, :])
    inv = np.zeros_like(diff)
    inv[free] = 1.0 / diff[free]
    df_dy = (w[:, :, None] * inv).sum(axis=1)  # (Q, M)
    wm = df_dy.sum(axis=0)
    wv = (eps * df_dy).sum(axis=0) / (2.0 * sd)
    return f, wm, wv
