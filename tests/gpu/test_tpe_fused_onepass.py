"""Differential tests for the two-call fused TPE suggest: ``fused_prepare``
(early above-set fit into the history's own coefficient buffer) and the
one-pass scoring launch, in which a block owns a slice of C = 64 mixture
kernels, walks all candidates, and the below mixture is scored by extra blocks
of the same launch.

The extension is called directly with ``return_parts=True``; log g, log l and
their difference are compared against ``optuna_amd.testing.tpe_reference`` at
rtol = atol = 1e-9 (the project's device-vs-host bound), ``-inf`` positions
exactly, NaN never. Where two runs execute the same kernels on the same inputs
(prepared against unprepared fits) the comparison is bit for bit.

Shapes follow the constants of the scoring kernel: slices of C = 64 kernels
(K = n_above + 1 of 1, 2, C - 1, C, C + 1, 2C + 1, and 601 for many slices),
24 candidates per block in wavefront groups of 6 (S of 1, 24, 25), dims in
passes of 24 (D of 1, 20, 33: one partial pass, one full-size headline pass,
two passes), below estimators of 1, 2, 257 and 1024 kernels. Below slices hold
min(64, 256 // min(D, 24)) kernels, so the below sizes are run at D = 3 (full
64-kernel slices, 1024 = 16 of them) and D = 20 (12-kernel slices, the last
one partial).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from optuna_amd import _hip
from optuna_amd.distributions import FloatDistribution
from optuna_amd.samplers._tpe._device import default_weight_ramp
from optuna_amd.samplers._tpe.sampler import default_weights
from optuna_amd.testing import tpe_reference as ref_mod
from optuna_amd.testing.tpe_reference import EdgeCase, kernel_sigmas, mixture_logpdf


pytestmark = pytest.mark.gpu

RTOL = 1e-9
ATOL = 1e-9
C = 64  # SCORE_SLICE of tpe_fused_kernels.h


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


def _space(kind: str, D: int):
    """D float dims; every third one log-scaled and/or stepped by ``kind``."""
    space = {}
    for d in range(D):
        if kind in ("log", "mixed") and d % 3 == 1:
            space[f"l{d}"] = FloatDistribution(1e-3, 1e3, log=True)
        elif kind in ("step", "mixed") and d % 3 == 2:
            space[f"s{d}"] = FloatDistribution(0.0, 10.0, step=0.5)
        else:
            space[f"x{d}"] = FloatDistribution(-5.0, 5.0)
    return space


@functools.lru_cache(maxsize=None)
def _inputs(kind: str, D: int, n: int, n_below: int, S: int, seed: int):
    """KDE-domain table, below observations, domain arrays and candidates
    (read-only, shared between tests)."""
    space = _space(kind, D)
    r = np.random.RandomState(seed)
    x_raw = ref_mod._draw(r, space, S)
    a = EdgeCase("t", space, ref_mod._draw(r, space, n), np.ones(n), 1.0, x_raw).kde_args()
    b = EdgeCase("b", space, ref_mod._draw(r, space, n_below), np.ones(n_below), 1.0,
                 x_raw).kde_args()
    out = {k: a[k] for k in ("obs", "alow", "ahigh", "steps", "n_choices", "x", "xedges")}
    out["bobs"] = b["obs"]
    for v in out.values():
        v.setflags(write=False)
    return out


def _check(got: np.ndarray, ref: np.ndarray, what: str) -> None:
    got = np.asarray(got)
    assert got.shape == ref.shape
    both = np.isfinite(ref) & np.isfinite(got)
    print(f"{what}: max |got - ref| over finite:", np.max(np.abs(got - ref)[both], initial=0.0))
    assert not np.isnan(got).any(), (what, got)
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
    finite = np.isfinite(ref)
    np.testing.assert_allclose(got[finite], ref[finite], rtol=RTOL, atol=ATOL)


def _mix(w: np.ndarray, prior_weight: float) -> np.ndarray:
    if len(w) == 0:
        return np.array([1.0])
    w = np.append(w, [prior_weight])
    return w / w.sum()


def _resident(core, obs: np.ndarray, a):
    hist = core.TpeDeviceHistory(obs.shape[1])
    hist.append(np.ascontiguousarray(obs))
    hist.upload_sorted([
        np.ascontiguousarray(np.argsort(obs[:, d], kind="stable").astype(np.int32))
        for d in range(obs.shape[1])
    ])
    hist.set_domain(a["alow"], a["ahigh"], a["steps"], a["n_choices"])
    return hist


def _below(a, ce: bool, mc: bool, prior_weight: float):
    """Below estimator kernels over ``a['bobs']`` as the host builds them."""
    bobs = a["bobs"]
    D = bobs.shape[1]
    mid = 0.5 * (a["alow"] + a["ahigh"])
    rng_ = a["ahigh"] - a["alow"]
    if len(bobs) == 0:
        mus, sigmas = mid[None, :].copy(), rng_[None, :].copy()
    else:
        sig = np.column_stack(
            [kernel_sigmas(bobs[:, d], a["alow"][d], a["ahigh"][d], ce, mc) for d in range(D)]
        )
        mus = np.vstack([bobs, mid])
        sigmas = np.vstack([sig, rng_])
    w = _mix(default_weights(len(bobs)), prior_weight)
    return np.ascontiguousarray(mus), np.ascontiguousarray(sigmas), w


def _excl_rows(n: int, n_excl: int, seed: int = 11) -> np.ndarray:
    return np.sort(np.random.RandomState(seed).choice(n, n_excl, replace=False)).astype(np.int32)


class _Call:
    """Arguments of one fused suggest over table ``obs``, split for the two
    native entry points."""

    def __init__(self, a, obs, excl, ce, mc, prior_weight=1.0, custom_weights=None):
        self.a, self.obs, self.excl = a, obs, excl
        self.ce, self.mc, self.prior_weight = ce, mc, prior_weight
        self.members = np.setdiff1d(np.arange(len(obs)), excl)
        self.Na = len(self.members)
        if custom_weights is None:
            self.w_above = _mix(default_weights(self.Na), prior_weight)
            logw = np.empty(0)
            ramp = default_weight_ramp(self.Na, prior_weight)
        else:
            self.w_above = _mix(custom_weights, prior_weight)
            with np.errstate(divide="ignore"):
                logw = np.log(self.w_above)
            ramp = (0, 1.0, 0.0, 0.0)
        self.fit_tail = (logw, *ramp, prior_weight, ce, mc)
        self.bmu, self.bsig, self.bw = _below(a, ce, mc, prior_weight)
        has_steps = bool((a["steps"] > 0).any())
        self.x = np.ascontiguousarray(a["x"])
        self.xedges = np.ascontiguousarray(a["xedges"]) if has_steps else np.empty(0)

    def prepare(self, hist) -> None:
        hist.fused_prepare(self.excl, self.Na, *self.fit_tail)

    def score(self, hist, parts: bool = True):
        out = hist.fused_score(self.excl, self.Na, self.x, self.xedges, self.bmu, self.bsig,
                               self.bw, *self.fit_tail, parts)
        return out[0] if parts else out

    def check(self, parts) -> None:
        a = self.a
        kw = dict(alow=a["alow"], ahigh=a["ahigh"], steps=a["steps"], n_choices=a["n_choices"],
                  prior_weight=self.prior_weight, x=a["x"], xedges=a["xedges"],
                  consider_endpoints=self.ce, magic_clip=self.mc)
        ref_g = mixture_logpdf(obs=self.obs[self.members], weights=self.w_above, **kw)
        ref_l = mixture_logpdf(obs=a["bobs"], weights=self.bw, **kw)
        ei, log_g, log_l = parts
        _check(log_g, ref_g, "log_g")
        _check(log_l, ref_l, "log_l")
        both = np.isfinite(ref_g) & np.isfinite(ref_l)
        _check(ei[both], (ref_l - ref_g)[both], "ei")


def _run(core, kind, D, n_above, n_excl, Kb, S, seed, ce=False, custom_weights=None,
         prepare=True):
    a = _inputs(kind, D, n_above + n_excl, Kb - 1, S, seed)
    call = _Call(a, a["obs"], _excl_rows(n_above + n_excl, n_excl), ce, True,
                 custom_weights=custom_weights)
    assert call.Na == n_above
    hist = _resident(core, a["obs"], a)
    if prepare:
        call.prepare(hist)
    parts = call.score(hist)
    call.check(parts)
    # The production form returns the (S,) acquisition values only.
    np.testing.assert_array_equal(call.score(hist, parts=False), parts[0])
    return call, parts


# ---------------------------------------------------------------------------
# Shapes
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("prepare", [False, True], ids=["alone", "prepared"])
@pytest.mark.parametrize("K", [1, 2, C - 1, C, C + 1, 2 * C + 1, 601])
def test_slice_edges(core, K, prepare) -> None:
    """Above mixtures of one lane, a slice short of one lane, a full slice,
    one lane into the next slice, two slices and a lane, and ten slices."""
    _run(core, "cont", 3, K - 1, 2, 3, 24, 1000 + K, ce=K % 2 == 0, prepare=prepare)


@pytest.mark.parametrize("D", [3, 20])
@pytest.mark.parametrize("Kb", [1, 2, 257, 1024])
def test_below_sizes(core, Kb, D) -> None:
    """Prior-only below mixture, one observation, several slices with a
    partial last one, and the entry point's limit."""
    _run(core, "cont", D, C + 1, 3, Kb, 24, 2000 + Kb + D, ce=Kb % 2 == 0)


@pytest.mark.parametrize("D", [1, 20, 33])
@pytest.mark.parametrize("S", [1, 24, 25])
def test_candidates_and_dims(core, S, D) -> None:
    """One candidate, a full block of 24, one candidate into a second block;
    a single dim, the headline 20, and 33 (a second pass over the dims)."""
    _run(core, "cont", D, 2 * C + 1, 2, C + 1, S, 3000 + 10 * S + D, ce=S % 2 == 0)


@pytest.mark.parametrize("D", [3, 33])
@pytest.mark.parametrize("kind", ["log", "step", "mixed"])
def test_log_and_stepped_dims(core, kind, D) -> None:
    _run(core, kind, D, 2 * C + 1, 2, C + 1, 25, 4000 + D)
    _run(core, kind, D, C - 1, 0, 2, 24, 4100 + D, ce=True, prepare=False)


@pytest.mark.parametrize("pattern", ["scattered", "whole-slice", "all-but-prior"])
def test_zero_weights(core, pattern) -> None:
    """Zero weights upload as -inf log-weights. A slice whose kernels all have
    zero weight must contribute (-inf, 0) and never NaN."""
    n_above = 3 * C + 5
    w = np.random.RandomState(7).uniform(0.1, 2.0, n_above)
    if pattern == "scattered":
        w[[0, 5, C - 1, C, 2 * C + 3, n_above - 1]] = 0.0
    elif pattern == "whole-slice":
        w[C:2 * C] = 0.0
    else:
        w[:] = 0.0
    _, parts = _run(core, "cont", 3, n_above, 2, 3, 24, 5000, custom_weights=w)
    assert np.isfinite(parts).all()  # the prior keeps every mixture positive


def test_zero_weights_everywhere(core) -> None:
    """A prior weight of zero on top: log g is -inf for every candidate."""
    n_above = C + 3
    a = _inputs("cont", 3, n_above + 2, 2, 24, 5001)
    call = _Call(a, a["obs"], _excl_rows(n_above + 2, 2), False, True)
    call.w_above = np.zeros(n_above + 1)
    call.fit_tail = (np.full(n_above + 1, -np.inf), 0, 1.0, 0.0, 0.0, 1.0, False, True)
    ei, log_g, log_l = call.score(_resident(core, a["obs"], a))
    assert np.isneginf(log_g).all() and np.isfinite(log_l).all()
    assert (ei == np.inf).all()


# ---------------------------------------------------------------------------
# Prepared fits
# ---------------------------------------------------------------------------


def _fresh_parts(core, call: _Call):
    """The call on a new history, with no prepare."""
    return call.score(_resident(core, call.obs, call.a))


def test_prepare_then_score_equals_score_alone(core) -> None:
    a = _inputs("mixed", 20, 2 * C + 3, C, 25, 6000)
    call = _Call(a, a["obs"], _excl_rows(2 * C + 3, 2), False, True)
    alone = _fresh_parts(core, call)
    hist = _resident(core, a["obs"], a)
    call.prepare(hist)
    np.testing.assert_array_equal(call.score(hist), alone)
    # The prepared fit stays valid for a second identical suggest, and a
    # second prepare with the same arguments changes nothing either.
    np.testing.assert_array_equal(call.score(hist), alone)
    call.prepare(hist)
    call.prepare(hist)
    np.testing.assert_array_equal(call.score(hist), alone)
    call.check(alone)


def test_stale_prepare_after_append(core) -> None:
    a = _inputs("cont", 3, 2 * C + 4, 3, 24, 6001)
    obs = a["obs"]
    n = len(obs) - 1
    hist = _resident(core, obs[:n], a)
    old = _Call(a, obs[:n], _excl_rows(n, 2), False, True)
    old.prepare(hist)
    hist.append(np.ascontiguousarray(obs[n:]))
    hist.insert_sorted_by_value(n, 1)
    new = _Call(a, obs, _excl_rows(n, 2), False, True)
    assert new.Na == old.Na + 1
    got = new.score(hist)
    np.testing.assert_array_equal(got, _fresh_parts(core, new))
    new.check(got)


def test_stale_prepare_other_exclusion_list(core) -> None:
    a = _inputs("cont", 3, 2 * C + 4, 3, 24, 6002)
    n = len(a["obs"])
    hist = _resident(core, a["obs"], a)
    first = _Call(a, a["obs"], _excl_rows(n, 3, seed=1), False, True)
    second = _Call(a, a["obs"], _excl_rows(n, 3, seed=2), False, True)
    assert len(first.excl) == len(second.excl) and not np.array_equal(first.excl, second.excl)
    first.prepare(hist)
    got = second.score(hist)
    np.testing.assert_array_equal(got, _fresh_parts(core, second))
    second.check(got)


@pytest.mark.parametrize("other_call", ["score", "kde_logpdf"])
def test_prepare_survives_workspace_growth(core, other_call) -> None:
    """Between prepare and score another history scores through the shared
    workspace, with a table large enough to make it grow."""
    a = _inputs("cont", 3, 2 * C + 4, 3, 24, 6003)
    call = _Call(a, a["obs"], _excl_rows(len(a["obs"]), 2), False, True)
    hist = _resident(core, a["obs"], a)
    call.prepare(hist)

    big = _inputs("cont", 5, 70000 if other_call == "score" else 90000, 1, 24, 6004)
    n = len(big["obs"])
    w = np.full(n + 1, 1.0 / (n + 1))
    if other_call == "score":
        other = _resident(core, big["obs"], big)
        other.score([], np.arange(n, dtype=np.int32), n, np.log(w), big["alow"], big["ahigh"],
                    big["steps"], big["n_choices"], 1.0, np.ascontiguousarray(big["x"]),
                    np.ascontiguousarray(big["xedges"]), False, True)
    else:
        order = np.argsort(big["obs"], axis=0, kind="stable").astype(np.int64)
        core.kde_logpdf(np.ascontiguousarray(big["obs"]), np.ascontiguousarray(order),
                        np.log(w), big["alow"], big["ahigh"], big["steps"], big["n_choices"],
                        1.0, np.ascontiguousarray(big["x"]),
                        np.ascontiguousarray(big["xedges"]), False, True)

    got = call.score(hist)
    np.testing.assert_array_equal(got, _fresh_parts(core, call))
    call.check(got)


@pytest.mark.parametrize("order", ["ab", "ba"])
def test_two_histories_prepared_alternately(core, order) -> None:
    a = _inputs("cont", 3, 2 * C + 4, 3, 24, 6005)
    b = _inputs("mixed", 20, C + 9, C, 25, 6006)
    call_a = _Call(a, a["obs"], _excl_rows(len(a["obs"]), 2), False, True)
    call_b = _Call(b, b["obs"], _excl_rows(len(b["obs"]), 4), True, True)
    alone_a, alone_b = _fresh_parts(core, call_a), _fresh_parts(core, call_b)
    hist_a, hist_b = _resident(core, a["obs"], a), _resident(core, b["obs"], b)
    call_a.prepare(hist_a)
    call_b.prepare(hist_b)
    if order == "ab":
        got_a, got_b = call_a.score(hist_a), call_b.score(hist_b)
    else:
        got_b, got_a = call_b.score(hist_b), call_a.score(hist_a)
    np.testing.assert_array_equal(got_a, alone_a)
    np.testing.assert_array_equal(got_b, alone_b)
    call_a.check(got_a)
    call_b.check(got_b)
