"""Independent fp64 reference for the TPE mixture log-pdf, plus the shared
edge-case table used by the CPU and GPU differential tests.

This module deliberately shares no code with the production estimator
(``samplers/_tpe/parzen*.py``) or with the HIP kernels: it forms the full
(S, K, D) tensor of per-(candidate, kernel, dim) log terms from the *centered*
truncated-normal density and reduces it with ``scipy.special.logsumexp``. The
production host path and the device kernels both use the expanded quadratic
form ``x²·c1 + x·c2 + c3``; agreement with this module is therefore evidence
about the math, not about a shared formula.
"""
from __future__ import annotations

from dataclasses import dataclass
import math
from typing import Iterator

import numpy as np
from scipy import special

from optuna_amd.distributions import (
    BaseDistribution,
    CategoricalDistribution,
    FloatDistribution,
    IntDistribution,
)


_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def log_gauss_mass(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """log(Phi(b) - Phi(a)) elementwise; -inf where a >= b."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    out = np.full(a.shape, -np.inf)
    ok = a < b
    left = ok & (b <= 0)
    right = ok & (a > 0)
    central = ok & ~left & ~right
    with np.errstate(all="ignore"):
        if left.any():
            lb = special.log_ndtr(b[left])
            out[left] = lb + np.log1p(-np.exp(special.log_ndtr(a[left]) - lb))
        if right.any():
            la = special.log_ndtr(-a[right])
            out[right] = la + np.log1p(-np.exp(special.log_ndtr(-b[right]) - la))
        if central.any():
            out[central] = np.log1p(-special.ndtr(a[central]) - special.ndtr(-b[central]))
    return out


def kernel_sigmas(
    col: np.ndarray, low: float, high: float, consider_endpoints: bool, magic_clip: bool
) -> np.ndarray:
    """Per-observation bandwidths of one numerical dim (observation order)."""
    n = len(col)
    order = np.argsort(col, kind="stable")
    sv = col[order]
    sig_sorted = np.empty(n)
    for r in range(n):
        prev = low if r == 0 else sv[r - 1]
        nxt = high if r == n - 1 else sv[r + 1]
        sig_sorted[r] = max(sv[r] - prev, nxt - sv[r])
    if not consider_endpoints and n >= 2:
        sig_sorted[0] = sv[1] - sv[0]
        sig_sorted[n - 1] = sv[n - 1] - sv[n - 2]
    rng_ = high - low
    minsigma = rng_ / min(100.0, n + 2.0) if magic_clip else 1e-12
    sig_sorted = np.minimum(np.maximum(sig_sorted, minsigma), rng_)
    sig = np.empty(n)
    sig[order] = sig_sorted
    return sig


def mixture_terms(
    obs: np.ndarray,
    alow: np.ndarray,
    ahigh: np.ndarray,
    steps: np.ndarray,
    n_choices: np.ndarray,
    prior_weight: float,
    x: np.ndarray,
    xedges: np.ndarray,
    consider_endpoints: bool,
    magic_clip: bool,
) -> np.ndarray:
    """(S, K, D) log density of candidate s under kernel k in dim d (K = N + 1)."""
    obs = np.asarray(obs, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    N, D = obs.shape
    S = x.shape[0]
    K = N + 1
    terms = np.empty((S, K, D))
    for d in range(D):
        C = int(n_choices[d])
        if C > 0:
            if N == 0:
                w = np.full((1, C), 1.0 / C)
            else:
                w = np.full((K, C), prior_weight / K)
                w[np.arange(N), obs[:, d].astype(np.int64)] += 1.0
                rs = w.sum(axis=1, keepdims=True)
                w = w / np.where(rs == 0.0, 1.0, rs)
            with np.errstate(divide="ignore"):
                terms[:, :, d] = np.log(w[:, x[:, d].astype(np.int64)]).T
            continue
        low, high = float(alow[d]), float(ahigh[d])
        mu = np.append(obs[:, d], 0.5 * (low + high))
        sigma = np.append(
            kernel_sigmas(obs[:, d], low, high, consider_endpoints, magic_clip), high - low
        )
        log_z = log_gauss_mass((low - mu) / sigma, (high - mu) / sigma)  # (K,)
        if steps[d] > 0:
            xl = xedges[:, d][:, None]
            xr = xedges[:, D + d][:, None]
            terms[:, :, d] = log_gauss_mass((xl - mu) / sigma, (xr - mu) / sigma) - log_z
        else:
            diff = x[:, d][:, None] - mu[None, :]
            terms[:, :, d] = (
                -(diff * diff) / (2.0 * sigma * sigma) - np.log(sigma) - _HALF_LOG_2PI - log_z
            )
    return terms


def mixture_logpdf(
    obs: np.ndarray,
    weights: np.ndarray,
    alow: np.ndarray,
    ahigh: np.ndarray,
    steps: np.ndarray,
    n_choices: np.ndarray,
    prior_weight: float,
    x: np.ndarray,
    xedges: np.ndarray,
    consider_endpoints: bool,
    magic_clip: bool,
    per_dim: bool = False,
) -> np.ndarray:
    """Mixture log-pdf of ``x`` under the Parzen estimator fitted to ``obs``.

    Arguments are in the KDE domain (log already applied), exactly those of
    the extension's ``kde_logpdf`` except that ``weights`` ((N+1,), normalized,
    prior last) replaces ``logw``. Returns (S,), or (S, D) of independent 1-D
    mixtures with ``per_dim=True``.
    """
    terms = mixture_terms(
        obs, alow, ahigh, steps, n_choices, prior_weight, x, xedges,
        consider_endpoints, magic_clip,
    )
    w = np.asarray(weights, dtype=np.float64)
    if per_dim:
        return special.logsumexp(terms, axis=1, b=w[None, :, None])
    return special.logsumexp(terms.sum(axis=2), axis=1, b=w[None, :])


# ---------------------------------------------------------------------------
# Shared edge-case table
# ---------------------------------------------------------------------------


@dataclass
class EdgeCase:
    name: str
    space: dict[str, BaseDistribution]
    obs_raw: np.ndarray  # (N, D) internal representation (categorical = index)
    weights_raw: np.ndarray  # (N,) unnormalized kernel weights
    prior_weight: float
    x_raw: np.ndarray  # (S, D)
    consider_endpoints: bool = False
    magic_clip: bool = True
    expect_all_neginf: bool = False

    @property
    def names(self) -> list[str]:
        return list(self.space.keys())

    def mixture_weights(self) -> np.ndarray:
        if len(self.obs_raw) == 0:
            return np.array([1.0])
        w = np.append(np.asarray(self.weights_raw, dtype=np.float64), [self.prior_weight])
        return w / w.sum()

    def kde_args(self) -> dict:
        """KDE-domain arrays: the extension's arguments, ``weights`` for ``logw``."""
        dists = list(self.space.values())
        D = len(dists)
        alow, ahigh = np.zeros(D), np.ones(D)
        steps, n_choices = np.zeros(D), np.zeros(D)
        obs = np.array(self.obs_raw, dtype=np.float64).reshape(-1, D)
        x = np.array(self.x_raw, dtype=np.float64)
        xedges = np.zeros((x.shape[0], 2 * D))
        for d, dist in enumerate(dists):
            if isinstance(dist, CategoricalDistribution):
                n_choices[d] = len(dist.choices)
                continue
            step = float(dist.step) if dist.step is not None else 0.0
            lo, hi = float(dist.low) - step / 2, float(dist.high) + step / 2
            steps[d] = step
            if step:
                xedges[:, d] = x[:, d] - step / 2
                xedges[:, D + d] = x[:, d] + step / 2
            if dist.log:
                lo, hi = math.log(lo), math.log(hi)
                obs[:, d] = np.log(obs[:, d])
                xedges[:, [d, D + d]] = np.log(xedges[:, [d, D + d]]) if step else 0.0
                x[:, d] = np.log(x[:, d])
            alow[d], ahigh[d] = lo, hi
        return dict(
            obs=obs, weights=self.mixture_weights(), alow=alow, ahigh=ahigh, steps=steps,
            n_choices=n_choices, prior_weight=float(self.prior_weight), x=x, xedges=xedges,
            consider_endpoints=self.consider_endpoints, magic_clip=self.magic_clip,
        )

    def reference(self, per_dim: bool = False) -> np.ndarray:
        return mixture_logpdf(**self.kde_args(), per_dim=per_dim)


def default_ramp(n: int) -> np.ndarray:
    """Tie-free positive weights (every kernel distinguishable)."""
    return np.linspace(0.5, 1.5, n) if n else np.empty(0)


_MIXED6 = {
    "f": FloatDistribution(-5.0, 5.0),
    "i": IntDistribution(1, 10),
    "lf": FloatDistribution(1e-3, 1e3, log=True),
    "c": CategoricalDistribution([0, 1, 2, 3]),
    "sf": FloatDistribution(0.0, 1.0, step=0.1),
    "li": IntDistribution(1, 64, log=True),
}

_MIXED3 = {
    "f": FloatDistribution(-5.0, 5.0),
    "i": IntDistribution(1, 10),
    "c": CategoricalDistribution([0, 1, 2, 3]),
}


def _draw(rng: np.random.RandomState, space: dict[str, BaseDistribution], n: int) -> np.ndarray:
    """(n, D) random points of ``space`` in internal representation."""
    out = np.empty((n, len(space)))
    for d, dist in enumerate(space.values()):
        if isinstance(dist, CategoricalDistribution):
            out[:, d] = rng.randint(0, len(dist.choices), n)
        elif isinstance(dist, IntDistribution):
            if dist.log:
                out[:, d] = np.clip(
                    np.round(np.exp(rng.uniform(math.log(dist.low), math.log(dist.high), n))),
                    dist.low, dist.high,
                )
            else:
                out[:, d] = rng.randint(dist.low, dist.high + 1, n)
        elif dist.step is not None:
            n_cells = int(round((dist.high - dist.low) / dist.step))
            out[:, d] = dist.low + dist.step * rng.randint(0, n_cells + 1, n)
        elif dist.log:
            out[:, d] = np.exp(rng.uniform(math.log(dist.low), math.log(dist.high), n))
        else:
            out[:, d] = rng.uniform(dist.low, dist.high, n)
    return out


def _floats(d: int) -> dict[str, BaseDistribution]:
    return {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(d)}


def edge_cases() -> Iterator[EdgeCase]:
    """Named, seeded cases at the sizes and values where the kernels branch."""
    S = 5
    seed = 0

    def rs() -> np.random.RandomState:
        nonlocal seed
        seed += 1
        return np.random.RandomState(1000 + seed)

    # Small N: empty / single / first sizes at which the endpoint rule applies.
    for n in (0, 1, 2, 3):
        for tag, space in (("d1", _floats(1)), ("mixed6", _MIXED6)):
            for ce in (False, True):
                r = rs()
                yield EdgeCase(
                    f"small-n{n}-{tag}-ce{int(ce)}", space, _draw(r, space, n),
                    default_ramp(n), 1.0, _draw(r, space, S), consider_endpoints=ce,
                )

    # Block (256) and logsumexp chunk (512) boundaries: K = N + 1.
    for n in (255, 256, 511, 512, 1023, 1024):
        for tag, space in (("cont2", _floats(2)), ("mixed3", _MIXED3)):
            r = rs()
            yield EdgeCase(
                f"boundary-n{n}-{tag}", space, _draw(r, space, n), default_ramp(n), 1.0,
                _draw(r, space, S),
            )

    # More dims than block lanes (strided candidate staging).
    for d in (257, 300):
        r = rs()
        space = _floats(d)
        yield EdgeCase(
            f"wide-d{d}", space, _draw(r, space, 5), default_ramp(5), 1.0, _draw(r, space, S)
        )
    r = rs()
    space = _floats(256)
    space["last_int"] = IntDistribution(1, 10)
    yield EdgeCase(
        "wide-d257-int-last", space, _draw(r, space, 5), default_ramp(5), 1.0,
        _draw(r, space, S),
    )

    # Ties (magic clip on).
    r = rs()
    space = _floats(2)
    obs = _draw(r, space, 8)
    obs[:, 0] = 1.25
    yield EdgeCase("ties-identical-column", space, obs, default_ramp(8), 1.0, _draw(r, space, S))
    obs = _draw(r, space, 9)
    obs[0, 0], obs[1, 0], obs[2, 0], obs[3, 0] = -5.0, 5.0, -5.0, 5.0
    obs[4, 1], obs[5, 1] = 5.0, -5.0
    for ce in (False, True):
        yield EdgeCase(
            f"ties-obs-on-bounds-ce{int(ce)}", space, obs.copy(), default_ramp(9), 1.0,
            _draw(r, space, S), consider_endpoints=ce,
        )
    obs = _draw(r, space, 7)
    x = np.array([obs[0], obs[3], [-5.0, 5.0], [5.0, -5.0], [obs[2, 0], -5.0]])
    yield EdgeCase("cand-on-obs-and-bounds", space, obs, default_ramp(7), 1.0, x)

    # Magic clip off: tie-free jittered lattice, min gap >= range / (4 N).
    for n in (5, 64):
        r = rs()
        space = _floats(2)
        cell = 10.0 / n
        obs = np.empty((n, 2))
        for d in range(2):
            lattice = -5.0 + cell * (np.arange(n) + 0.5) + r.uniform(-0.25, 0.25, n) * cell
            obs[:, d] = r.permutation(lattice)
        for ce in (False, True):
            yield EdgeCase(
                f"clip-off-lattice-n{n}-ce{int(ce)}", space, obs.copy(), default_ramp(n), 1.0,
                _draw(r, space, S), consider_endpoints=ce, magic_clip=False,
            )

    # Zero mixture weights.
    r = rs()
    space = _floats(2)
    n = 300
    obs, x = _draw(r, space, n), _draw(r, space, S)
    w = default_ramp(n)
    w0 = w.copy()
    w0[0] = 0.0
    yield EdgeCase("zero-w-k0", space, obs, w0, 1.0, x)
    w0 = w.copy()
    w0[:256] = 0.0
    yield EdgeCase("zero-w-first-block", space, obs, w0, 1.0, x)
    w0 = w.copy()
    w0[::3] = 0.0
    yield EdgeCase("zero-w-every-third", space, obs, w0, 1.0, x)
    r = rs()
    n = 600
    obs, x = _draw(r, _MIXED3, n), _draw(r, _MIXED3, S)
    w0 = default_ramp(n)
    w0[:256] = 0.0
    w0[512:] = 0.0
    yield EdgeCase("zero-w-first-block-mixed3", _MIXED3, obs, w0, 1.0, x)
    for n in (256, 512):
        for tag, space in (("cont2", _floats(2)), ("mixed3", _MIXED3)):
            r = rs()
            yield EdgeCase(
                f"zero-prior-k{n + 1}-{tag}", space, _draw(r, space, n), default_ramp(n), 0.0,
                _draw(r, space, S),
            )
    # prior_weight = 0 and a candidate category that only zero-weight kernels
    # (or none) observed: the density is exactly zero.
    r = rs()
    n = 40
    obs, x = _draw(r, _MIXED3, n), _draw(r, _MIXED3, S)
    obs[:, 2] = r.randint(0, 3, n)
    obs[:4, 2] = 3
    x[:, 2] = 3
    w0 = default_ramp(n)
    w0[:4] = 0.0
    yield EdgeCase(
        "zero-prior-unobserved-category", _MIXED3, obs, w0, 0.0, x, expect_all_neginf=True
    )

    # Categorical smoothing.
    for pw in (0.5, 2.5):
        for c in (2, 7):
            r = rs()
            space = {
                "f": FloatDistribution(-5.0, 5.0),
                "c": CategoricalDistribution(list(range(c))),
            }
            n = 12
            obs, x = _draw(r, space, n), _draw(r, space, S)
            obs[:, 1] = r.randint(0, c - 1, n)  # category c-1 never observed
            x[0, 1] = c - 1
            x[1, 1] = c - 1
            yield EdgeCase(f"categorical-pw{pw}-c{c}", space, obs, default_ramp(n), pw, x)

    # Weights other than the ramp with the prior weight off 1.
    for n, pw in ((7, 2.5), (513, 2.5), (255, 0.0)):
        for ce in (False, True):
            r = rs()
            yield EdgeCase(
                f"prior-weight-n{n}-pw{pw}-ce{int(ce)}", _MIXED6, _draw(r, _MIXED6, n),
                r.uniform(0.1, 2.0, n), pw, _draw(r, _MIXED6, S), consider_endpoints=ce,
            )


def sorted_index_batches(kind: str) -> list[np.ndarray]:
    """Append batches ((n, 2) parameter rows in [-5, 5]) that drive the
    incrementally sorted per-dim index through its edge positions. A NaN marks
    a parameter the trial does not have (an invalid row of the space).

    ``"positions"``: 600 rows, then single rows landing at position 0, in the
    middle and at the end, then a 5-row batch with duplicates and values equal
    to existing ones. ``"growth"``: 500 rows, then batches taking the index to
    1020, 1023 and 1026 rows (across the 1024-row device capacity).
    """
    r = np.random.RandomState(77)
    if kind == "positions":
        first = r.uniform(-4.9, 4.9, (600, 2))
        first[17, 1] = np.nan
        first[300, 0] = np.nan
        dup = np.array(
            [
                [first[0, 0], first[1, 1]],
                [first[0, 0], 1.5],
                [1.5, 1.5],
                [2.5, first[7, 1]],
                [2.5, first[7, 1]],
            ]
        )
        return [
            first,
            np.array([[-4.999, 4.999]]),
            np.array([[0.123, -0.321]]),
            np.array([[4.9995, -4.9995]]),
            dup,
        ]
    if kind == "growth":
        return [
            r.uniform(-5, 5, (500, 2)),
            r.uniform(-5, 5, (520, 2)),
            r.uniform(-5, 5, (3, 2)),
            r.uniform(-5, 5, (3, 2)),
        ]
    raise ValueError(kind)
