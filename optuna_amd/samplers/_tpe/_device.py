"""Device dispatch for the TPE hot path (K1 fit + K2 mixture log-pdf on gfx950).

Device modes:

* **Resident history** (the fast path): each (study, search-space) keeps a
  ``TpeDeviceHistory`` whose parameter table lives in HBM and grows append-only
  in lockstep with the host mirror (``_history.py``). The per-dim sorted order
  (i32) is resident too and grows on the device with each tell. A suggest
  uploads only a subset position map, the domain, the mixture weights and the
  24 candidates — the fp64 observation matrix never crosses PCIe again. Subset
  compaction, the K1 fit and the K2 scoring all run on device.
* **Fused suggest** (`fused_eligible`): for joint scoring over numerical dims the
  suggest is two native calls on one stream, and no O(N) array is built or
  uploaded. `prepare_fused_resident` runs right after the below/above split:
  it uploads the short list of excluded rows and launches the above-set fit
  straight from the resident sorted index, into a coefficient buffer the
  history owns, and returns without waiting — the fit runs while the host
  builds the below estimator and draws the candidates. The scoring call then
  makes one packed upload (candidates, the below estimator's kernels), scores
  the above slices and the below mixture side by side in one launch, and a
  small merge launch writes `log l - log g`. The native side checks that the
  prepared fit still matches its arguments and otherwise fits by itself.
  Between the two calls the below estimator is fitted by a third, host-only
  native call (`draw_below_native` -> `tpe_below_kernels`) that repeats the
  numpy arithmetic of `parzen.py` bit for bit; the truncated-normal quantile
  and the RNG calls stay in Python. Custom weights functions and
  `OPTUNA_AMD_TPE_NATIVE_BELOW=0` keep the Python estimator.
* **Native draw route** (`native_draw`, the default on the fused path with the
  native below route): everything behind `prepare_fused_resident` is one native
  call, `TpeDeviceHistory.fused_draw_score`. The sampler makes the two RNG
  calls of the draw (`random_sample(S)` for the kernel choice, `uniform` for
  the (S, D) quantiles) and passes them on in a `DrawRequest`; the call gathers
  the below rows from the host table, fits the below estimator, turns the
  first draw into kernel indices as `RandomState.choice` does, evaluates the
  truncated-normal quantile, maps the draws to the parameter domain, derives
  the scoring inputs, runs the device half of the scoring call and returns the
  index of the best candidate with the candidates. The quantile repeats
  `_truncnorm_np.ppf` bit for bit: scipy's scalar `ndtr`, `log_ndtr` and
  `ndtri_exp` are taken from the capsules of `scipy.special.cython_special`
  and called per element, numpy's `log`, `log1p`, `exp` and `logaddexp` are
  numpy's own ufuncs, called on packed arrays (`csrc/tpe_draw_host.h`,
  `csrc/tpe_draw_bind.h`). `OPTUNA_AMD_TPE_NATIVE_DRAW=0`, an extension without
  the entry or a scipy without those capsules keep the three-call route.
* **Stateless scoring** (`kde_logpdf`): used by golden tests and the
  constant-liar path (whose observation set includes rows not in the table).

Eligibility: any numerical dimensions — continuous, log, int, or
step-discretized (the scoring kernel integrates the step cell). Categorical
dimensions keep the (already vectorized) host path.
"""
from __future__ import annotations

import math
import os
from typing import TYPE_CHECKING, NamedTuple

import numpy as np

from optuna_amd import _hip
from optuna_amd.distributions import (
    BaseDistribution,
    CategoricalDistribution,
    FloatDistribution,
    IntDistribution,
)
from optuna_amd.samplers._tpe import _truncnorm_np as _tn
from optuna_amd.samplers._tpe.parzen import _NumericalSpace, _to_param_domain


if TYPE_CHECKING:
    from optuna_amd.samplers._tpe._history import _SpaceCache

# Below this kernel count the host fit is cheaper than a kernel launch round trip.
DEVICE_MIN_KERNELS = 512


def space_is_device_eligible(space: dict[str, BaseDistribution]) -> bool:
    # Float / int / discrete dims use the (possibly cell-integrated) truncnorm
    # kernels; categorical dims use the closed-form smoothed one-hot weights.
    return bool(space)


def device_ready(n_kernels: int) -> bool:
    return n_kernels >= DEVICE_MIN_KERNELS and _hip.is_available()


# Limits of the fused entry point (LDS-cached exclusion list, below kernels
# fitted inside the scoring launch); mirrored in tpe_fused_kernels.h.
FUSED_MAX_EXCL = 1024
FUSED_MAX_BELOW = 1024

_EMPTY_F64 = np.empty(0, dtype=np.float64)


def fused_enabled() -> bool:
    """``OPTUNA_AMD_TPE_FUSED=0`` forces the unfused path (A/B runs)."""
    return os.environ.get("OPTUNA_AMD_TPE_FUSED", "1") != "0"


def fused_eligible(
    space: dict[str, BaseDistribution],
    *,
    per_dim: bool,
    n_liar: int,
    default_estimator: bool,
    rows_ascending: bool,
    n_excl: int,
    n_below_kernels: int,
) -> bool:
    """Whether a suggest may take the fused device entry point.

    The fused kernels address the "above" set as the ascending-row complement
    of a short exclusion list, score jointly, and evaluate the below mixture
    inside the scoring launch; every other case keeps the unfused path.
    """
    return (
        fused_enabled()
        and not per_dim
        and n_liar == 0
        and default_estimator
        and rows_ascending
        and n_excl <= FUSED_MAX_EXCL
        and n_below_kernels <= FUSED_MAX_BELOW
        and bool(space)
        and not any(isinstance(d, CategoricalDistribution) for d in space.values())
    )


def default_weight_ramp(n: int, prior_weight: float) -> tuple[int, float, float, float]:
    """(w_num, w_start, w_step, log_total) describing ``default_weights(n)``
    plus the prior weight, for the device to expand: kernel k < w_num has
    weight ``k * w_step + w_start`` (numpy ``linspace`` arithmetic, last ramp
    element exactly 1), every later kernel 1, the prior ``prior_weight``;
    ``log_total`` is the log of their sum (arithmetic series, O(1))."""
    if n < 25:
        return 0, 1.0, 0.0, math.log(n + prior_weight) if n else 0.0
    num = n - 25
    start = 1.0 / n
    step = (1.0 - start) / (num - 1) if num > 1 else 0.0
    if num > 1:
        ramp_sum = num * (start + 1.0) / 2.0
    else:
        ramp_sum = start * num
    return num, start, step, math.log(ramp_sum + 25.0 + prior_weight)


def expand_weight_ramp(n: int, prior_weight: float) -> np.ndarray:
    """Host transcription of the device's expansion of ``default_weight_ramp``:
    the (n + 1,) unnormalized mixture weights, prior last (the device then
    writes ``log(w) - log_total``). Used by the tests."""
    num, start, step, _ = default_weight_ramp(n, prior_weight)
    w = np.ones(n + 1, dtype=np.float64)
    k = np.arange(num, dtype=np.float64)
    w[:num] = k * step + start
    if num > 1:
        w[num - 1] = 1.0
    w[n] = prior_weight if n else 1.0
    return w


def native_below_enabled() -> bool:
    """``OPTUNA_AMD_TPE_NATIVE_BELOW=0`` keeps the below estimator of a fused
    suggest in Python (A/B runs)."""
    return os.environ.get("OPTUNA_AMD_TPE_NATIVE_BELOW", "1") != "0"


_UNRESOLVED = object()


def native_below(cache: "_SpaceCache"):
    """The extension's entry that fits the below estimator of a fused suggest
    natively, or None (switched off, or no extension loaded): on the native
    draw route (``native_draw``) the ``fused_draw_score`` of the space's
    device history, which also draws and scores in the same call, otherwise
    the host-only ``tpe_below_kernels``. Resolved once per space cache."""
    if not native_below_enabled():
        return None
    if native_draw(cache):
        return cache._native_draw_entry  # type: ignore[attr-defined]
    fn = getattr(cache, "_native_below", _UNRESOLVED)
    if fn is _UNRESOLVED:
        fn = getattr(_hip.get(), "tpe_below_kernels", None)
        cache._native_below = fn  # type: ignore[attr-defined]
    return fn


def draw_below_native(
    fn,
    cache: "_SpaceCache",
    below_rows: np.ndarray,
    weights: np.ndarray,
    rng: np.random.RandomState,
    size: int,
    consider_endpoints: bool,
    consider_magic_clip: bool,
) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Candidates of a fused suggest with the below estimator fitted by ``fn``
    (``tpe_below_kernels``): returns ``(x_raw (S, D), mus, sigmas (Kb, D))``.

    Equal bit for bit to ``_ParzenEstimator(below observations)`` followed by
    its ``_sample_array``: the same RNG calls in the same order, the same
    truncated-normal quantile, and a fit that repeats numpy's arithmetic.
    ``weights`` are that estimator's normalized mixture weights."""
    ns = _numerical_space_of(cache)
    obs = cache.params[below_rows[cache.valid[below_rows]]]  # a fresh (n, D) copy
    if ns.is_log.any():
        obs[:, ns.is_log] = np.log(obs[:, ns.is_log])
    active = rng.choice(len(weights), p=weights, size=size)
    mus, sigmas, a, b, loc, scale = fn(
        obs, ns.adapted_lows, ns.adapted_highs, consider_endpoints, consider_magic_clip, active
    )
    q = rng.uniform(low=0, high=1, size=a.shape)
    x = _tn.ppf(q, a, b) * scale + loc
    _to_param_domain(x, ns.kinds, ns.lows, ns.highs, ns.steps)
    return x, mus, sigmas


def native_draw_enabled() -> bool:
    """``OPTUNA_AMD_TPE_NATIVE_DRAW=0`` keeps the draw, the scoring call and
    the arg-max of a fused suggest as separate Python steps (A/B runs)."""
    return os.environ.get("OPTUNA_AMD_TPE_NATIVE_DRAW", "1") != "0"


def _draw_capsules() -> tuple | None:
    """scipy's scalar ``ndtr``, ``log_ndtr`` and ``ndtri_exp`` on doubles, as
    the capsules ``scipy.special.cython_special`` exports to other extension
    modules; None when this scipy does not export them."""
    try:
        from scipy.special import cython_special

        capi = cython_special.__pyx_capi__
        return capi["__pyx_fuse_1ndtr"], capi["__pyx_fuse_1log_ndtr"], capi["ndtri_exp"]
    except (ImportError, AttributeError, KeyError):
        return None


def _bind_native_draw(core) -> bool:
    """Hands the capsules to the extension, which checks their signature
    strings before it takes the pointers."""
    bind = getattr(core, "tpe_draw_bind", None)
    capsules = _draw_capsules() if bind is not None else None
    return capsules is not None and bool(bind(*capsules))


def native_draw(cache: "_SpaceCache") -> bool:
    """Whether the native draw route is on for this space: ``native_below``
    then gives the one-call entry, to be passed on in a ``DrawRequest``. Off
    when switched off, while the space has no device mirror yet
    (``prepare_fused_resident`` makes it), with an extension without
    ``fused_draw_score``, or with a scipy whose scalar functions could not be
    bound. Resolved once per space cache."""
    if not native_draw_enabled():
        return False
    entry = getattr(cache, "_native_draw_entry", _UNRESOLVED)
    if entry is _UNRESOLVED:
        mirror = getattr(cache, "_device_mirror", None)
        if mirror is None:
            return False
        entry = getattr(mirror._hist, "fused_draw_score", None)
        if entry is not None and not _bind_native_draw(_hip.get()):
            entry = None
        cache._native_draw_entry = entry  # type: ignore[attr-defined]
    return entry is not None


def _numerical_space_of(cache: "_SpaceCache") -> _NumericalSpace:
    ns = getattr(cache, "_numerical_space", None)
    if ns is None:
        ns = cache._numerical_space = _NumericalSpace.of(cache.dists)  # type: ignore[attr-defined]
    return ns


class DrawRequest(NamedTuple):
    """Inputs of a fused suggest on the native draw route (``native_draw``)."""

    below_rows: np.ndarray  # table rows of the below set
    n_above: int  # valid rows outside the below set
    below_weights: np.ndarray  # (Kb,) normalized, as for draw_below_native
    u: np.ndarray  # (S,) random_sample draw of the kernel choice
    q: np.ndarray  # (S, D) uniform draw of the quantile
    entry: object  # what native_below gave: the history's fused_draw_score


class FusedRequest(NamedTuple):
    """Inputs of a fused suggest beyond those of ``score_above_resident``."""

    below_rows: np.ndarray  # table rows of the below set
    n_above: int  # valid rows outside the below set
    x_raw: np.ndarray  # (S, D) candidates, as drawn
    below_mus: np.ndarray  # (Kb, D) below estimator kernels, KDE domain
    below_sigmas: np.ndarray  # (Kb, D)
    below_weights: np.ndarray  # (Kb,)


def _space_domains(
    space: dict[str, BaseDistribution],
) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(is_log, alow, ahigh, steps, n_choices) per dim, KDE domain.

    Step-discretized dims widen the domain by half a step on each side before
    the log transform — identical to the host estimator's adapted bounds
    (parzen.py `_numerical_kernels_batched`).
    """
    dists = list(space.values())
    is_cat = np.array([isinstance(d, CategoricalDistribution) for d in dists])
    is_log = np.array(
        [False if c else bool(d.log) for c, d in zip(is_cat, dists)]
    )
    steps = np.array(
        [
            0.0 if c else (float(d.step) if d.step is not None else 0.0)
            for c, d in zip(is_cat, dists)
        ],
        dtype=np.float64,
    )
    n_choices = np.array(
        [float(len(d.choices)) if c else 0.0 for c, d in zip(is_cat, dists)],
        dtype=np.float64,
    )
    alow = np.zeros(len(dists))
    ahigh = np.ones(len(dists))
    for c, d in enumerate(dists):
        if is_cat[c]:
            continue  # unused by the categorical branch
        lo = float(d.low) - steps[c] / 2 if steps[c] else float(d.low)
        hi = float(d.high) + steps[c] / 2 if steps[c] else float(d.high)
        if d.log:
            lo, hi = math.log(lo), math.log(hi)
        alow[c] = lo
        ahigh[c] = hi
    return is_log, alow, ahigh, steps, n_choices


def _cell_edges(
    x_raw: np.ndarray, is_log: np.ndarray, steps: np.ndarray
) -> np.ndarray:
    """(S, 2D) per-candidate step-cell edges [lo | hi] in KDE domain.

    Continuous dims get zeros (the kernel never reads them); discrete dims get
    x ∓ step/2, logged for log-discrete dims — exactly the host integration
    cell (parzen.py `_log_pdf_array`).
    """
    S, D = x_raw.shape
    edges = np.zeros((S, 2 * D), dtype=np.float64)
    disc = steps > 0
    if disc.any():
        half = steps[disc] / 2
        lo = x_raw[:, disc] - half
        hi = x_raw[:, disc] + half
        log_disc = is_log[disc]
        if log_disc.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                lo[:, log_disc] = np.log(lo[:, log_disc])
                hi[:, log_disc] = np.log(hi[:, log_disc])
        idx = np.nonzero(disc)[0]
        edges[:, idx] = lo
        edges[:, D + idx] = hi
    return edges


class _SpaceDeviceMirror:
    """HBM-resident copy of one space's parameter table (KDE domain)."""

    def __init__(self, space: dict[str, BaseDistribution]) -> None:
        core = _hip.get()
        assert core is not None
        (
            self._is_log,
            self._alow,
            self._ahigh,
            self._steps,
            self._n_choices,
        ) = _space_domains(space)
        self._hist = core.TpeDeviceHistory(len(space))
        self._hist.set_domain(self._alow, self._ahigh, self._steps, self._n_choices)
        self._has_steps = bool((self._steps > 0).any())
        self._n_appended = 0
        # Device-resident sorted index bookkeeping: table rows the resident
        # index already covers (-1: never uploaded).
        self._rows_sorted_synced = -1
        # (key, native fit arguments) of a prepare_fused not yet scored.
        self._prepared: tuple | None = None

    def sync(self, cache: "_SpaceCache") -> None:
        n_total = len(cache.valid)
        if n_total > self._n_appended:
            block = np.array(cache.params[self._n_appended :], dtype=np.float64)
            if self._is_log.any():
                with np.errstate(invalid="ignore", divide="ignore"):
                    block[:, self._is_log] = np.log(block[:, self._is_log])
            self._hist.append(np.ascontiguousarray(block))
            self._n_appended = n_total
        self._sync_sorted(cache)

    def _sync_sorted(self, cache: "_SpaceCache") -> None:
        n_rows = len(cache.valid)
        done = self._rows_sorted_synced
        if done == n_rows:
            return
        # Bulk (re-)upload when starting fresh or when a large batch arrived
        # (the sequential device insert is O(batch · N)); per-tell rows are
        # inserted by value on device, which needs neither the host index nor
        # an upload. (Log dims compare log values there: two rows a few ulps
        # apart may tie after the log and then keep row order.)
        if done < 0 or n_rows - done > 64:
            self._hist.upload_sorted(list(cache.sorted_rows))
        else:
            valid = cache.valid[done:n_rows]
            r = 0
            while r < len(valid):
                if not valid[r]:
                    r += 1
                    continue
                e = r
                while e < len(valid) and valid[e]:
                    e += 1
                self._hist.insert_sorted_by_value(done + r, e - r)
                r = e
        self._rows_sorted_synced = n_rows

    def score(
        self,
        cache: "_SpaceCache",
        sel: np.ndarray,
        weights: np.ndarray,
        samples: dict[str, np.ndarray],
        consider_endpoints: bool,
        consider_magic_clip: bool,
        prior_weight: float = 1.0,
        extras: np.ndarray | None = None,
        per_dim: bool = False,
    ) -> np.ndarray:
        """Score candidates against the resident table.

        ``extras`` ((L, D), internal repr) are constant-liar rows from other
        workers' RUNNING trials: they are appended to the mixture after the
        ``sel`` kernels (matching the host estimator's observation order) and
        merged into the per-dim sorted subsets on device.
        """
        self.sync(cache)
        n_total = len(cache.valid)
        pos = np.full(n_total, -1, dtype=np.int32)
        pos[sel] = np.arange(len(sel), dtype=np.int32)
        # The per-dim sorted index is device-resident (kept current by
        # _sync_sorted), so no columns are passed.
        sorted_cols: list = []
        x_raw = np.column_stack(
            [np.asarray(samples[n], dtype=np.float64) for n in cache.names]
        )
        xedges = _cell_edges(x_raw, self._is_log, self._steps)
        x = x_raw.copy()
        if self._is_log.any():
            x[:, self._is_log] = np.log(x[:, self._is_log])
        with np.errstate(divide="ignore"):
            logw = np.log(weights)
        kwargs = {}
        if extras is not None and len(extras):
            E = np.array(extras, dtype=np.float64)
            if self._is_log.any():
                E[:, self._is_log] = np.log(E[:, self._is_log])
            order = np.argsort(E, axis=0, kind="stable")  # (L, D) per column
            kwargs = dict(
                extras_raw=np.ascontiguousarray(E),
                extras_sorted=np.ascontiguousarray(
                    np.take_along_axis(E, order, axis=0).T  # (D, L)
                ),
                extras_sorted_idx=np.ascontiguousarray(
                    order.T.astype(np.int32)  # (D, L)
                ),
            )
        return self._hist.score(
            sorted_cols,
            pos,
            int(len(sel)),
            logw,
            self._alow,
            self._ahigh,
            self._steps,
            self._n_choices,
            float(prior_weight),
            np.ascontiguousarray(x),
            np.ascontiguousarray(xedges),
            consider_endpoints,
            consider_magic_clip,
            per_dim=per_dim,
            **kwargs,
        )


    def prepare_fused(
        self,
        cache: "_SpaceCache",
        below_rows: np.ndarray,
        n_above: int,
        weights: np.ndarray | None,
        consider_endpoints: bool,
        consider_magic_clip: bool,
        prior_weight: float,
    ) -> None:
        """First half of a fused suggest: bring the mirror up to date, build
        the exclusion list and launch the above-set fit, without waiting for
        it. Everything it needs is known right after the below/above split, so
        the fit runs on the GPU while the host builds the below estimator and
        draws the candidates. ``weights`` as in ``score_fused``."""
        self.sync(cache)
        excl = cache.excluded_rows(below_rows)
        if weights is None:
            logw = _EMPTY_F64
            ramp = default_weight_ramp(n_above, prior_weight)
        else:
            with np.errstate(divide="ignore"):
                logw = np.log(weights)
            ramp = (0, 1.0, 0.0, 0.0)
        fit_args = (
            excl,
            int(n_above),
            logw,
            *ramp,
            float(prior_weight),
            consider_endpoints,
            consider_magic_clip,
        )
        self._hist.fused_prepare(*fit_args)
        # score_fused takes these arguments over as they are when it is asked
        # for the same suggest (same split of the same table); the arrays are
        # held so that their identities stay theirs.
        key = self._suggest_key(
            cache, below_rows, n_above, weights, consider_endpoints, consider_magic_clip,
            prior_weight,
        )
        self._prepared = (key, fit_args, below_rows, weights)

    @staticmethod
    def _suggest_key(
        cache, below_rows, n_above, weights, consider_endpoints, consider_magic_clip, prior_weight
    ) -> tuple:
        return (
            len(cache.valid), id(below_rows), int(n_above), id(weights),
            consider_endpoints, consider_magic_clip, float(prior_weight),
        )

    def score_fused(
        self,
        cache: "_SpaceCache",
        req: FusedRequest,
        weights: np.ndarray | None,
        consider_endpoints: bool,
        consider_magic_clip: bool,
        prior_weight: float,
        return_parts: bool = False,
    ) -> np.ndarray:
        """Acquisition values through the fused entry point: one packed
        upload, no O(N) host arrays. ``weights`` is the normalized (n_above+1,)
        mixture weight vector of a custom weights function, or None for the
        default ramp. A ``prepare_fused`` for the same suggest has normally
        run already; if not, it runs here (the native side then still finds
        its fit prepared, just not early)."""
        args = (
            cache, req.below_rows, req.n_above, weights, consider_endpoints,
            consider_magic_clip, prior_weight,
        )
        if self._prepared is None or self._prepared[0] != self._suggest_key(*args):
            self.prepare_fused(*args)
        assert self._prepared is not None
        fit_args, self._prepared = self._prepared[1], None
        excl, n_above, logw, w_num, w_start, w_step, log_total = fit_args[:7]
        x = req.x_raw
        xedges = _cell_edges(x, self._is_log, self._steps) if self._has_steps else _EMPTY_F64
        if self._is_log.any():
            x = x.copy()
            x[:, self._is_log] = np.log(x[:, self._is_log])
        return self._hist.fused_score(
            excl,
            n_above,
            x,
            xedges,
            req.below_mus,
            req.below_sigmas,
            req.below_weights,
            logw,
            w_num,
            w_start,
            w_step,
            log_total,
            float(prior_weight),
            consider_endpoints,
            consider_magic_clip,
            return_parts,
        )


    def draw_score_fused(
        self,
        cache: "_SpaceCache",
        req: DrawRequest,
        consider_endpoints: bool,
        consider_magic_clip: bool,
        prior_weight: float,
    ) -> tuple[int, np.ndarray, np.ndarray]:
        """Second half of a fused suggest on the native draw route, in one
        native call: what ``draw_below_native`` (given its two RNG draws),
        ``score_fused`` and the arg-max compute. Default weight ramp only.
        Returns (best index, x_raw (S, D), (S,) acquisition values)."""
        args = (
            cache, req.below_rows, req.n_above, None, consider_endpoints,
            consider_magic_clip, prior_weight,
        )
        if self._prepared is None or self._prepared[0] != self._suggest_key(*args):
            self.prepare_fused(*args)
        assert self._prepared is not None
        fit_args, self._prepared = self._prepared[1], None
        excl, n_above, logw, w_num, w_start, w_step, log_total = fit_args[:7]
        ns = _numerical_space_of(cache)
        # numpy's ufuncs run inside the call: log(0) and inf - inf of the
        # quantile's edge cases are expected there, as in _truncnorm_np.
        with np.errstate(divide="ignore", invalid="ignore"):
            return req.entry(  # type: ignore[operator]
                excl,
                n_above,
                cache.params,
                cache.valid,
                np.ascontiguousarray(req.below_rows, dtype=np.int64),
                req.below_weights,
                req.u,
                req.q,
                ns.adapted_lows,
                ns.adapted_highs,
                ns.kinds,
                ns.lows,
                ns.highs,
                ns.steps,
                logw,
                w_num,
                w_start,
                w_step,
                log_total,
                float(prior_weight),
                consider_endpoints,
                consider_magic_clip,
            )


def _mirror_of(cache: "_SpaceCache") -> _SpaceDeviceMirror:
    mirror = getattr(cache, "_device_mirror", None)
    if mirror is None:
        mirror = _SpaceDeviceMirror(cache.space)
        cache._device_mirror = mirror  # type: ignore[attr-defined]
    return mirror


def prepare_fused_resident(
    cache: "_SpaceCache",
    below_rows: np.ndarray,
    n_above: int,
    weights: np.ndarray | None,
    consider_endpoints: bool,
    consider_magic_clip: bool,
    prior_weight: float = 1.0,
) -> None:
    """Launch the above-set fit of a fused suggest ahead of its scoring call
    (``score_above_resident(..., fused=...)`` with the same ``below_rows``
    object, ``n_above`` and ``weights``). Purely an early start: scoring
    without it, or after the table changed, fits by itself."""
    if not _hip.is_available():
        return
    _mirror_of(cache).prepare_fused(
        cache, below_rows, n_above, weights, consider_endpoints, consider_magic_clip,
        prior_weight,
    )


def score_above_resident(
    cache: "_SpaceCache",
    sel: np.ndarray | None,
    weights: np.ndarray | None,
    samples: dict[str, np.ndarray] | None,
    consider_endpoints: bool,
    consider_magic_clip: bool,
    prior_weight: float = 1.0,
    extras: np.ndarray | None = None,
    per_dim: bool = False,
    fused: FusedRequest | DrawRequest | None = None,
) -> np.ndarray | tuple[int, np.ndarray, np.ndarray]:
    """log g(x) for candidates via the device-resident table (creates the mirror
    on first use; attached to the host space cache so lifetimes match).
    ``per_dim=True`` returns the (S, D) per-dimension 1-D mixture log-pdfs
    (independent-mode TPE) instead of the joint (S,) product score.

    With ``fused`` (see ``fused_eligible``) the call returns the acquisition
    values ``log l(x) - log g(x)`` instead; ``sel`` and ``samples`` are unused
    and ``weights=None`` selects the default weight ramp, written on device.

    With a ``DrawRequest`` as ``fused`` (see ``native_draw``) the candidates
    are drawn inside the same native call as well, and the call returns (index
    of the best candidate, x_raw (S, D), (S,) acquisition values); default
    ramp only."""
    mirror = _mirror_of(cache)
    if isinstance(fused, DrawRequest):
        return mirror.draw_score_fused(
            cache, fused, consider_endpoints, consider_magic_clip, prior_weight
        )
    if fused is not None:
        return mirror.score_fused(
            cache, fused, weights, consider_endpoints, consider_magic_clip, prior_weight
        )
    return mirror.score(
        cache, sel, weights, samples, consider_endpoints, consider_magic_clip,
        prior_weight=prior_weight, extras=extras, per_dim=per_dim,
    )


def kde_logpdf(
    space: dict[str, BaseDistribution],
    observations: dict[str, np.ndarray],
    orders: dict[str, np.ndarray] | None,
    weights: np.ndarray,
    samples: dict[str, np.ndarray],
    consider_endpoints: bool,
    consider_magic_clip: bool,
    prior_weight: float = 1.0,
) -> np.ndarray:
    """Stateless device scoring (observation matrix uploaded per call)."""
    core = _hip.get()
    assert core is not None
    names = list(space.keys())
    D = len(names)
    N = len(observations[names[0]])

    is_log, alow, ahigh, steps, n_choices = _space_domains(space)
    obs = np.empty((N, D), dtype=np.float64)
    x_raw = np.column_stack(
        [np.asarray(samples[n], dtype=np.float64) for n in names]
    )
    sorted_pos = np.empty((N, D), dtype=np.int64)
    for c, name in enumerate(names):
        col = np.asarray(observations[name], dtype=np.float64)
        obs[:, c] = np.log(col) if is_log[c] else col
        if orders is not None:
            sorted_pos[:, c] = orders[name]
        else:
            sorted_pos[:, c] = np.argsort(col, kind="stable")

    xedges = _cell_edges(x_raw, is_log, steps)
    x = x_raw.copy()
    if is_log.any():
        x[:, is_log] = np.log(x[:, is_log])

    with np.errstate(divide="ignore"):
        logw = np.log(weights)
    return core.kde_logpdf(
        obs,
        sorted_pos,
        logw,
        alow,
        ahigh,
        steps,
        n_choices,
        float(prior_weight),
        x,
        np.ascontiguousarray(xedges),
        consider_endpoints,
        consider_magic_clip,
    )
