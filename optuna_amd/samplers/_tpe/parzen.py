"""Parzen-window KDE for TPE, in SoA (structure-of-arrays) layout.

Unlike the reference's per-dimension NamedTuple list
(reference ``optuna/samplers/_tpe/parzen_estimator.py`` :34 and
``probability_distributions.py`` :139), the estimator here packs all numerical
dimensions into dense ``(K, D)`` mu/sigma matrices plus a per-dimension descriptor
table (kind / low / high / step / adapted bounds). That layout is what the K1/K2
HIP kernels consume directly — fitting and the S×K×D log-pdf reduction run on
device with no repacking — and the numpy host path below is the golden reference
for them.

Behavioral parity with the reference estimator (same kernels, same magic clip,
same prior kernel, same discrete/log handling):
 * per-point sigma = max gap to sorted neighbors incl. domain endpoints
   (endpoints excluded from first/last gap unless consider_endpoints)
 * magic clip: sigma ∈ [(high-low)/min(100, 1+K), high-low], K = n_obs+1
 * +1 prior kernel: mu = domain midpoint, sigma = domain width
 * categorical: prior-smoothed one-hot weight matrix
 * discrete dims integrate the kernel over [x-step/2, x+step/2]
 * log dims model the density in log space (no Jacobian; it cancels in the
   below/above EI ratio)
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from optuna_amd.distributions import (
    BaseDistribution,
    CategoricalDistribution,
    FloatDistribution,
    IntDistribution,
)
from optuna_amd.samplers._tpe import _truncnorm_np as _tn


EPS = 1e-12

# Descriptor "kind" codes, shared with the HIP kernels (see _hip/kernels/tpe.hip).
KIND_CONT = 0  # continuous
KIND_LOG = 1  # continuous, log domain
KIND_DISC = 2  # discretized (step)
KIND_LOG_DISC = 3  # discretized, log domain
KIND_CAT = 4  # categorical


class _ParzenEstimatorParameters(NamedTuple):
    # Field order matches the reference (which keeps the prior always-on and
    # has no consider_prior field); ours stays as a trailing default.
    prior_weight: float
    consider_magic_clip: bool
    consider_endpoints: bool
    weights: Callable[[int], np.ndarray]
    multivariate: bool
    consider_prior: bool = True


class _NumericalDims(NamedTuple):
    """SoA view of all numerical dimensions of the KDE."""

    dim_indices: np.ndarray  # (Dn,) int — position in the search-space order
    kinds: np.ndarray  # (Dn,) int8 — KIND_* codes (non-categorical)
    lows: np.ndarray  # (Dn,) original domain low
    highs: np.ndarray  # (Dn,) original domain high
    steps: np.ndarray  # (Dn,) step or 0
    adapted_lows: np.ndarray  # (Dn,) KDE-domain low  (step-widened, logged)
    adapted_highs: np.ndarray  # (Dn,) KDE-domain high
    mus: np.ndarray  # (K, Dn)
    sigmas: np.ndarray  # (K, Dn)


class _CategoricalDim(NamedTuple):
    dim_index: int
    weights: np.ndarray  # (K, C)


class _NumericalSpace(NamedTuple):
    """Per-space constants of an all-numerical search space (no kernels)."""

    kinds: np.ndarray  # (D,) int8 — KIND_* codes
    lows: np.ndarray  # (D,) original domain low
    highs: np.ndarray  # (D,) original domain high
    steps: np.ndarray  # (D,) step or 0
    adapted_lows: np.ndarray  # (D,) KDE-domain low  (step-widened, logged)
    adapted_highs: np.ndarray  # (D,) KDE-domain high
    is_log: np.ndarray  # (D,) bool

    @classmethod
    def of(cls, dists: list[BaseDistribution]) -> "_NumericalSpace":
        steps = np.array(
            [float(d.step) if d.step is not None else 0.0 for d in dists]
        )
        is_log = np.array([bool(d.log) for d in dists])
        lows = np.array([float(d.low) for d in dists])
        highs = np.array([float(d.high) for d in dists])
        a_lows = np.where(steps != 0.0, lows - steps / 2, lows)
        a_highs = np.where(steps != 0.0, highs + steps / 2, highs)
        if is_log.any():
            a_lows[is_log] = np.log(a_lows[is_log])
            a_highs[is_log] = np.log(a_highs[is_log])
        kinds = np.where(
            is_log,
            np.where(steps != 0.0, KIND_LOG_DISC, KIND_LOG),
            np.where(steps != 0.0, KIND_DISC, KIND_CONT),
        ).astype(np.int8)
        return cls(kinds, lows, highs, steps, a_lows, a_highs, is_log)


def _to_param_domain(
    vals: np.ndarray, kinds: np.ndarray, lows: np.ndarray, highs: np.ndarray, steps: np.ndarray
) -> None:
    """KDE-domain draws (S, Dn) to parameter values, in place: log dims are
    exponentiated, stepped dims rounded to their grid and clipped."""
    is_log = (kinds == KIND_LOG) | (kinds == KIND_LOG_DISC)
    vals[:, is_log] = np.exp(vals[:, is_log])
    has_step = steps > 0
    if np.any(has_step):
        lo = lows[has_step]
        st = steps[has_step]
        hi = highs[has_step]
        vals[:, has_step] = np.clip(
            lo + np.round((vals[:, has_step] - lo) / st) * st, lo, hi
        )


def _mixture_weights(
    parameters: _ParzenEstimatorParameters,
    n_obs: int,
    predetermined_weights: np.ndarray | None = None,
) -> np.ndarray:
    """Normalized (n_obs + 1,) kernel weights of an estimator, prior last."""
    weights = (
        predetermined_weights
        if predetermined_weights is not None
        else _ParzenEstimator._call_weights_func(parameters.weights, n_obs)
    )
    if n_obs == 0:
        weights = np.array([1.0])
    else:
        weights = np.append(weights, [parameters.prior_weight])
    return weights / weights.sum()


class _ParzenEstimator:
    """Mixture of K product kernels over the search space (see module docstring)."""

    def __init__(
        self,
        observations: dict[str, np.ndarray],
        search_space: dict[str, BaseDistribution],
        parameters: _ParzenEstimatorParameters,
        predetermined_weights: np.ndarray | None = None,
        sorted_orders: dict[str, np.ndarray] | None = None,
    ) -> None:
        # sorted_orders: optional per-param argsort of the observations, supplied by
        # the incremental history mirror so the fit avoids per-suggest O(N log N).
        self._sorted_orders = sorted_orders or {}
        if parameters.prior_weight < 0:
            raise ValueError(
                "A non-negative value must be specified for prior_weight, but got "
                f"{parameters.prior_weight}."
            )
        self._search_space = search_space
        self._param_names = list(search_space.keys())

        n_obs = len(next(iter(observations.values()))) if observations else 0
        for name in self._param_names:
            assert len(observations[name]) == n_obs

        if predetermined_weights is not None:
            assert n_obs == len(predetermined_weights)
        self._weights = _mixture_weights(parameters, n_obs, predetermined_weights)
        self._n_kernels = n_obs + 1

        # ---- build per-dimension model, packing numerical dims into SoA ------------
        dists = [search_space[n] for n in self._param_names]
        if dists and all(
            not isinstance(d, CategoricalDistribution) for d in dists
        ):
            # All-numerical space: one vectorized fit over the (n, D) matrix
            # instead of D small per-dim numpy calls (the per-call overhead
            # dominates for the "below" estimator's ~25 observations).
            self._numerical = self._numerical_kernels_batched(
                observations, dists, parameters, n_obs
            )
            self._categoricals = []
            return

        num_idx: list[int] = []
        kinds: list[int] = []
        lows: list[float] = []
        highs: list[float] = []
        steps: list[float] = []
        alows: list[float] = []
        ahighs: list[float] = []
        mus_cols: list[np.ndarray] = []
        sigmas_cols: list[np.ndarray] = []
        categoricals: list[_CategoricalDim] = []

        for i, name in enumerate(self._param_names):
            dist = search_space[name]
            obs = np.asarray(observations[name], dtype=np.float64)
            if isinstance(dist, CategoricalDistribution):
                categoricals.append(
                    _CategoricalDim(i, self._categorical_weights(obs, len(dist.choices), parameters))
                )
                continue
            assert isinstance(dist, (FloatDistribution, IntDistribution))
            step = float(dist.step) if dist.step is not None else 0.0
            is_log = dist.log
            low = float(dist.low)
            high = float(dist.high)
            a_low = low - step / 2 if step else low
            a_high = high + step / 2 if step else high
            if is_log:
                a_low, a_high = np.log(a_low), np.log(a_high)
            mu, sigma = self._numerical_kernels(
                np.log(obs) if is_log else obs,
                a_low,
                a_high,
                parameters,
                order=self._sorted_orders.get(name),
            )
            num_idx.append(i)
            if is_log and step:
                kinds.append(KIND_LOG_DISC)
            elif is_log:
                kinds.append(KIND_LOG)
            elif step:
                kinds.append(KIND_DISC)
            else:
                kinds.append(KIND_CONT)
            lows.append(low)
            highs.append(high)
            steps.append(step)
            alows.append(a_low)
            ahighs.append(a_high)
            mus_cols.append(mu)
            sigmas_cols.append(sigma)

        self._numerical = _NumericalDims(
            dim_indices=np.asarray(num_idx, dtype=np.int64),
            kinds=np.asarray(kinds, dtype=np.int8),
            lows=np.asarray(lows, dtype=np.float64),
            highs=np.asarray(highs, dtype=np.float64),
            steps=np.asarray(steps, dtype=np.float64),
            adapted_lows=np.asarray(alows, dtype=np.float64),
            adapted_highs=np.asarray(ahighs, dtype=np.float64),
            mus=(
                np.stack(mus_cols, axis=1)
                if mus_cols
                else np.empty((self._n_kernels if n_obs else 1, 0))
            ),
            sigmas=(
                np.stack(sigmas_cols, axis=1)
                if sigmas_cols
                else np.empty((self._n_kernels if n_obs else 1, 0))
            ),
        )
        self._categoricals = categoricals

    # Scoring coefficients are derived on first use: an estimator that only
    # draws candidates (its kernels are scored on device) never pays for them.
    _LAZY_COEFFICIENTS = frozenset(
        ("_cont_mask", "_log_total_mass", "_c1", "_c2", "_c3", "_c3_rowsum")
    )

    def __getattr__(self, name: str):
        if name in _ParzenEstimator._LAZY_COEFFICIENTS and "_numerical" in self.__dict__:
            self._precompute_logpdf_coefficients()
            return self.__dict__[name]
        raise AttributeError(name)

    def _precompute_logpdf_coefficients(self) -> None:
        """Expand -((x-mu)/sigma)^2/2 - log sigma - log Z into x^2*c1 + x*c2 + c3.

        This reduces the S×K×D mixture log-pdf to two (S,D)@(D,K) GEMMs plus a
        per-kernel constant — the exact dataflow of the K2 HIP kernel, and ~50×
        faster than broadcast temporaries on host, with identical math.
        Only continuous (non-discrete) dims participate; discrete dims keep the
        integrated-cell path but get their total-mass normalization cached here.
        """
        num = self._numerical
        is_disc = num.steps > 0
        self._cont_mask = ~is_disc
        mus = num.mus
        sigmas = num.sigmas
        if num.mus.shape[1]:
            # Total truncation mass per (kernel, dim), cached for both paths.
            a = (num.adapted_lows[np.newaxis, :] - mus) / sigmas
            b = (num.adapted_highs[np.newaxis, :] - mus) / sigmas
            self._log_total_mass = _tn._log_gauss_mass(a, b)  # (K, Dn)
        else:
            self._log_total_mass = np.empty((len(self._weights), 0))

        cont = self._cont_mask
        if np.any(cont):
            m = mus[:, cont]
            s = sigmas[:, cont]
            inv_var = 1.0 / (s * s)
            self._c1 = -0.5 * inv_var  # (K, Dc)
            self._c2 = m * inv_var
            c3 = (
                -0.5 * m * m * inv_var
                - np.log(s)
                - 0.5 * np.log(2 * np.pi)
                - self._log_total_mass[:, cont]
            )
            self._c3 = c3  # (K, Dc) — per-dim scoring (independent mode)
            self._c3_rowsum = c3.sum(axis=1)  # (K,)
        else:
            self._c1 = np.empty((len(self._weights), 0))
            self._c2 = np.empty((len(self._weights), 0))
            self._c3 = np.empty((len(self._weights), 0))
            self._c3_rowsum = np.zeros(len(self._weights))

    # ---- fitting helpers ------------------------------------------------------------

    @staticmethod
    def _call_weights_func(weights_func: Callable[[int], np.ndarray], n: int) -> np.ndarray:
        w = np.asarray(weights_func(n), dtype=np.float64)[:n]
        if np.any(w < 0):
            raise ValueError(
                f"The `weights` function is not allowed to return negative values {w}. "
                f"The argument of the `weights` function is {n}."
            )
        if len(w) > 0 and np.sum(w) <= 0:
            raise ValueError(
                f"The `weights` function is not allowed to return all-zero values {w}. "
                f"The argument of the `weights` function is {n}."
            )
        if not np.all(np.isfinite(w)):
            raise ValueError(
                f"The `weights` function is not allowed to return infinite or NaN values {w}. "
                f"The argument of the `weights` function is {n}."
            )
        return w

    def _categorical_weights(
        self, observations: np.ndarray, n_choices: int, parameters: _ParzenEstimatorParameters
    ) -> np.ndarray:
        n_obs = len(observations)
        if n_obs == 0:
            return np.full((1, n_choices), 1.0 / n_choices)
        n_kernels = n_obs + 1
        w = np.full((n_kernels, n_choices), parameters.prior_weight / n_kernels)
        idx = observations.astype(int)
        w[np.arange(n_obs), idx] += 1.0
        row_sums = w.sum(axis=1, keepdims=True)
        return w / np.where(row_sums == 0, 1.0, row_sums)

    def _numerical_kernels_batched(
        self,
        observations: dict[str, np.ndarray],
        dists: list[BaseDistribution],
        parameters: _ParzenEstimatorParameters,
        n_obs: int,
    ) -> _NumericalDims:
        """Vectorized equivalent of the per-dim `_numerical_kernels` loop."""
        D = len(dists)
        kinds, lows, highs, steps, a_lows, a_highs, is_log = _NumericalSpace.of(dists)

        ranges = a_highs - a_lows
        if n_obs == 0:
            mus_full = (0.5 * (a_lows + a_highs))[None, :]
            sig_full = ranges[None, :]
        else:
            mus_mat = np.column_stack(
                [np.asarray(observations[n], dtype=np.float64) for n in self._param_names]
            )
            if is_log.any():
                mus_mat[:, is_log] = np.log(mus_mat[:, is_log])
            order_cols = [
                self._sorted_orders.get(name) for name in self._param_names
            ]
            if all(o is not None for o in order_cols):
                order_mat = np.column_stack(order_cols)
            else:
                order_mat = np.column_stack(
                    [
                        o
                        if o is not None
                        else np.argsort(mus_mat[:, c], kind="stable")
                        for c, o in enumerate(order_cols)
                    ]
                )
            padded = np.empty((n_obs + 2, D), dtype=np.float64)
            padded[0] = a_lows
            padded[-1] = a_highs
            padded[1:-1] = np.take_along_axis(mus_mat, order_mat, axis=0)
            gaps_left = padded[1:-1] - padded[:-2]
            gaps_right = padded[2:] - padded[1:-1]
            sorted_sigmas = np.maximum(gaps_left, gaps_right)
            if not parameters.consider_endpoints and n_obs >= 2:
                sorted_sigmas[0] = padded[2] - padded[1]
                sorted_sigmas[-1] = padded[-2] - padded[-3]
            inverse = np.empty_like(order_mat)
            np.put_along_axis(
                inverse, order_mat, np.arange(n_obs, dtype=order_mat.dtype)[:, None], axis=0
            )
            sigmas_mat = np.take_along_axis(sorted_sigmas, inverse, axis=0)
            if parameters.consider_magic_clip:
                minsig = ranges / min(100.0, 1.0 + (n_obs + 1))
            else:
                minsig = np.full(D, EPS)
            sigmas_mat = np.clip(sigmas_mat, minsig, ranges)
            mus_full = np.vstack([mus_mat, 0.5 * (a_lows + a_highs)])
            sig_full = np.vstack([sigmas_mat, ranges])

        return _NumericalDims(
            dim_indices=np.arange(D, dtype=np.int64),
            kinds=kinds,
            lows=lows,
            highs=highs,
            steps=steps,
            adapted_lows=a_lows,
            adapted_highs=a_highs,
            mus=mus_full,
            sigmas=sig_full,
        )

    def _numerical_kernels(
        self,
        mus: np.ndarray,
        low: float,
        high: float,
        parameters: _ParzenEstimatorParameters,
        order: np.ndarray | None = None,
    ) -> tuple[np.ndarray, np.ndarray]:
        """Per-point sigma = max gap to sorted neighbors; +1 prior kernel appended."""
        n = len(mus)
        if n == 0:
            return np.array([0.5 * (low + high)]), np.array([high - low])

        if order is None:
            # Stable: tied observations keep index order, so sigma assignment is
            # deterministic and matches the incrementally-sorted device orders.
            order = np.argsort(mus, kind="stable")
        padded = np.empty(n + 2, dtype=np.float64)
        padded[0] = low
        padded[1:-1] = mus[order]
        padded[-1] = high
        gaps_left = padded[1:-1] - padded[:-2]
        gaps_right = padded[2:] - padded[1:-1]
        sorted_sigmas = np.maximum(gaps_left, gaps_right)
        if not parameters.consider_endpoints and n >= 2:
            sorted_sigmas[0] = padded[2] - padded[1]
            sorted_sigmas[-1] = padded[-2] - padded[-3]
        # Scatter back to observation order (O(N), not an argsort of the argsort).
        inverse = np.empty_like(order)
        inverse[order] = np.arange(n)
        sigmas = sorted_sigmas[inverse]

        maxsigma = high - low
        if parameters.consider_magic_clip:
            minsigma = (high - low) / min(100.0, 1.0 + (n + 1))
        else:
            minsigma = EPS
        sigmas = np.clip(sigmas, minsigma, maxsigma)

        mus_out = np.append(mus, [0.5 * (low + high)])
        sigmas_out = np.append(sigmas, [high - low])
        return mus_out, sigmas_out

    # ---- sampling / scoring ---------------------------------------------------------

    @property
    def weights(self) -> np.ndarray:
        return self._weights

    @property
    def n_dims(self) -> int:
        return len(self._param_names)

    @property
    def _mixture_distribution(self):
        """The KDE as the reference's explicit object form (see
        ``probability_distributions.py``); converts from the SoA layout."""
        from optuna_amd.samplers._tpe import probability_distributions as _pd

        num = self._numerical
        per_dim: dict[int, object] = {}
        for j in range(len(num.dim_indices)):
            kind = int(num.kinds[j])
            mu = num.mus[:, j].copy()
            sigma = num.sigmas[:, j].copy()
            low = float(num.lows[j])
            high = float(num.highs[j])
            step = float(num.steps[j])
            if kind == KIND_CONT:
                d: object = _pd._BatchedTruncNormDistributions(mu, sigma, low, high)
            elif kind == KIND_LOG:
                d = _pd._BatchedTruncLogNormDistributions(mu, sigma, low, high)
            elif kind == KIND_DISC:
                d = _pd._BatchedDiscreteTruncNormDistributions(mu, sigma, low, high, step)
            else:
                d = _pd._BatchedDiscreteTruncLogNormDistributions(mu, sigma, low, high, step)
            per_dim[int(num.dim_indices[j])] = d
        for cat in self._categoricals:
            per_dim[int(cat.dim_index)] = _pd._BatchedCategoricalDistributions(
                cat.weights.copy()
            )
        dists = [per_dim[i] for i in range(len(self._param_names))]
        return _pd._MixtureOfProductDistribution(
            weights=self._weights.copy(), distributions=dists
        )

    def sample(self, rng: np.random.RandomState, size: int) -> dict[str, np.ndarray]:
        samples = self._sample_array(rng, size)
        return {name: samples[:, i] for i, name in enumerate(self._param_names)}

    def log_pdf(self, samples_dict: dict[str, np.ndarray]) -> np.ndarray:
        x = np.column_stack([samples_dict[name] for name in self._param_names]) if (
            self._param_names
        ) else np.empty((0, 0))
        return self._log_pdf_array(x)

    def sample_per_dim(
        self, rng: np.random.RandomState, size: int
    ) -> dict[str, np.ndarray]:
        """Independent-mode draws: each dim picks its own mixture component.

        The joint ``sample`` picks ONE component per draw shared by all dims (a
        product-mixture draw); independent-mode TPE treats every dim as its own
        1-D mixture, which is exactly a per-(draw, dim) component choice.
        """
        D = self.n_dims
        active = np.column_stack(
            [rng.choice(len(self._weights), p=self._weights, size=size) for _ in range(D)]
        )
        out = np.empty((size, D), dtype=np.float64)
        num = self._numerical
        Dn = num.mus.shape[1]
        if Dn:
            act_n = active[:, num.dim_indices]  # (S, Dn)
            cols = np.arange(Dn)[np.newaxis, :]
            mus = num.mus[act_n, cols]
            sigmas = num.sigmas[act_n, cols]
            a = (num.adapted_lows[np.newaxis, :] - mus) / sigmas
            b = (num.adapted_highs[np.newaxis, :] - mus) / sigmas
            vals = _tn.rvs(a, b, loc=mus, scale=sigmas, random_state=rng)
            _to_param_domain(vals, num.kinds, num.lows, num.highs, num.steps)
            out[:, num.dim_indices] = vals
        for cat in self._categoricals:
            active_w = cat.weights[active[:, cat.dim_index], :]
            q = rng.rand(size)
            cum = np.cumsum(active_w, axis=-1)
            cum[:, -1] = 1.0
            out[:, cat.dim_index] = np.sum(cum < q[:, np.newaxis], axis=-1)
        return {name: out[:, i] for i, name in enumerate(self._param_names)}

    def log_pdf_per_dim(self, samples_dict: dict[str, np.ndarray]) -> np.ndarray:
        """(S, D) of per-dim 1-D mixture log densities (independent mode)."""
        x = np.column_stack([samples_dict[name] for name in self._param_names])
        S = x.shape[0]
        K = len(self._weights)
        D = self.n_dims
        out = np.empty((S, D), dtype=np.float64)
        logw = np.log(self._weights)[np.newaxis, :]

        def lse(lt: np.ndarray) -> np.ndarray:  # (S, K) -> (S,)
            m = lt.max(axis=1)
            m[np.isneginf(m)] = 0.0
            with np.errstate(divide="ignore"):
                return np.log(np.exp(lt - m[:, None]).sum(axis=1)) + m

        num = self._numerical
        Dn = num.mus.shape[1]
        if Dn:
            xv = x[:, num.dim_indices]
            is_log = (num.kinds == KIND_LOG) | (num.kinds == KIND_LOG_DISC)
            xv = np.where(is_log[np.newaxis, :], np.log(np.maximum(xv, EPS)), xv)
            is_disc = num.steps > 0
            cont = self._cont_mask
            cont_cols = np.nonzero(cont)[0]
            if len(cont_cols):
                # All continuous dims at once: (S, K, Dc) of per-dim kernel
                # log-densities, logsumexp over K per (sample, dim).
                xc = xv[:, cont_cols]  # (S, Dc)
                lt = (
                    xc[:, None, :] * xc[:, None, :] * self._c1[None, :, :]
                    + xc[:, None, :] * self._c2[None, :, :]
                    + self._c3[None, :, :]
                    + logw[:, :, None]
                )
                m = lt.max(axis=1)  # (S, Dc)
                m[np.isneginf(m)] = 0.0
                with np.errstate(divide="ignore"):
                    vals = np.log(np.exp(lt - m[:, None, :]).sum(axis=1)) + m
                outside = (xc < num.adapted_lows[cont_cols]) | (
                    xc > num.adapted_highs[cont_cols]
                )
                vals[outside] = -np.inf
                out[:, num.dim_indices[cont_cols]] = vals
            for j in np.nonzero(is_disc)[0]:
                half = num.steps[j] / 2
                xj_raw = x[:, num.dim_indices[j]]
                if is_log[j]:
                    left = np.log(xj_raw - half)
                    right = np.log(xj_raw + half)
                else:
                    left = xj_raw - half
                    right = xj_raw + half
                m = num.mus[:, j]
                sg = num.sigmas[:, j]
                cell = _tn._log_gauss_mass(
                    (left[:, np.newaxis] - m) / sg, (right[:, np.newaxis] - m) / sg
                )
                out[:, num.dim_indices[j]] = lse(
                    cell - self._log_total_mass[:, j][np.newaxis, :] + logw
                )
        for cat in self._categoricals:
            xi = x[:, cat.dim_index].astype(np.int64)
            with np.errstate(divide="ignore"):
                out[:, cat.dim_index] = lse(np.log(cat.weights.T[xi, :]) + logw)
        return out

    # Array-level interfaces (used by the HIP dispatch and bench harness).

    def _sample_array(self, rng: np.random.RandomState, size: int) -> np.ndarray:
        active = rng.choice(len(self._weights), p=self._weights, size=size)
        out = np.empty((size, self.n_dims), dtype=np.float64)

        num = self._numerical
        if num.mus.shape[1]:
            mus = num.mus[active, :]  # (S, Dn)
            sigmas = num.sigmas[active, :]
            a = (num.adapted_lows[np.newaxis, :] - mus) / sigmas
            b = (num.adapted_highs[np.newaxis, :] - mus) / sigmas
            vals = _tn.rvs(a, b, loc=mus, scale=sigmas, random_state=rng)
            _to_param_domain(vals, num.kinds, num.lows, num.highs, num.steps)
            out[:, num.dim_indices] = vals

        for cat in self._categoricals:
            active_w = cat.weights[active, :]  # (S, C)
            q = rng.rand(size)
            cum = np.cumsum(active_w, axis=-1)
            cum[:, -1] = 1.0
            out[:, cat.dim_index] = np.sum(cum < q[:, np.newaxis], axis=-1)
        return out

    def _log_pdf_array(self, x: np.ndarray) -> np.ndarray:
        """(S, D) samples → (S,) log of the mixture density."""
        S = x.shape[0]
        K = len(self._weights)
        if S == 0:
            return np.empty(0)
        log_terms = np.zeros((S, K), dtype=np.float64)  # per-kernel product over dims

        num = self._numerical
        Dn = num.mus.shape[1]
        if Dn:
            xv = x[:, num.dim_indices]  # (S, Dn)
            is_log = (num.kinds == KIND_LOG) | (num.kinds == KIND_LOG_DISC)
            xv = np.where(is_log[np.newaxis, :], np.log(np.maximum(xv, EPS)), xv)
            is_disc = num.steps > 0
            cont = self._cont_mask

            # Continuous dims: quadratic-form expansion → two GEMMs + constants
            # (identical math to truncnorm logpdf; see _precompute_logpdf_coefficients).
            if np.any(cont):
                xc = xv[:, cont]  # (S, Dc)
                log_terms += (xc * xc) @ self._c1.T + xc @ self._c2.T
                log_terms += self._c3_rowsum[np.newaxis, :]
                # Outside the truncation box the density is exactly zero.
                outside = np.any(
                    (xc < num.adapted_lows[cont]) | (xc > num.adapted_highs[cont]), axis=1
                )
                if np.any(outside):
                    log_terms[outside, :] = -np.inf

            # Discrete dims: integrated kernel mass over the step cell.
            for j in np.nonzero(is_disc)[0]:
                half = num.steps[j] / 2
                xj_raw = x[:, num.dim_indices[j]]
                if is_log[j]:
                    left = np.log(xj_raw - half)
                    right = np.log(xj_raw + half)
                else:
                    left = xj_raw - half
                    right = xj_raw + half
                m = num.mus[:, j]
                s = num.sigmas[:, j]
                cell = _tn._log_gauss_mass(
                    (left[:, np.newaxis] - m) / s, (right[:, np.newaxis] - m) / s
                )
                log_terms += cell - self._log_total_mass[:, j][np.newaxis, :]

        for cat in self._categoricals:
            xi = x[:, cat.dim_index].astype(np.int64)
            with np.errstate(divide="ignore"):
                log_terms += np.log(cat.weights.T[xi, :])

        log_terms += np.log(self._weights)[np.newaxis, :]
        m = log_terms.max(axis=1)
        m[np.isneginf(m)] = 0.0
        with np.errstate(divide="ignore"):
            return np.log(np.exp(log_terms - m[:, None]).sum(axis=1)) + m
