"""The extension's ``fused_draw_score`` (the one-call second half of a fused
TPE suggest) against the two-call route it replaces, bit for bit: its
candidates against ``draw_below_native`` from the same seed, its acquisition
values against ``score_fused`` on those candidates (same kernels, same
inputs), its index against ``np.argmax``; and a seeded study with the native
draw route on and off.

Every case uses a table of 600 rows, just past the 512-kernel device
threshold; two of them are invalid for the space, one inside the below set.
"""
from __future__ import annotations

import functools
import types

import numpy as np
import pytest

from optuna_amd import _hip
from optuna_amd.distributions import FloatDistribution, IntDistribution
from optuna_amd.samplers._tpe import _device
from optuna_amd.samplers._tpe._history import _SpaceCache
from optuna_amd.samplers._tpe.sampler import default_weights
from optuna_amd.testing import tpe_below_cases as tc


pytestmark = pytest.mark.gpu

N_ROWS = 600
INVALID = (3, 377)  # row 3 lies in every non-empty below set


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


def _space(tag: str):
    if tag == "log":
        return {"a": FloatDistribution(-5.0, 5.0), "l": FloatDistribution(1e-3, 10.0, log=True),
                "b": FloatDistribution(0.0, 1.0)}
    if tag == "step":
        return {"a": FloatDistribution(-5.0, 5.0), "s": FloatDistribution(-5.0, 5.0, step=0.5),
                "li": IntDistribution(1, 64, log=True)}
    return {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(int(tag))}


@functools.lru_cache(maxsize=None)
def _cache(tag: str) -> _SpaceCache:
    """A space cache over 600 random rows with its device mirror, shared by
    the cases of one space (scoring leaves both unchanged)."""
    space = _space(tag)
    r = np.random.RandomState(len(space) + 17)
    trials = []
    for row in range(N_ROWS):
        params = {name: tc._draw_param(r, dist) for name, dist in space.items()}
        if row in INVALID:
            del params[next(iter(space))]
        trials.append(types.SimpleNamespace(params=params))
    cache = _SpaceCache(space)
    cache.append(trials)
    return cache


def _weights(n: int) -> np.ndarray:
    w = np.append(default_weights(n), [1.0]) if n else np.array([1.0])
    return w / w.sum()


def _bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _check_case(core, tag: str, S: int, n_below: int, ce: bool, mc: bool, seed: int) -> None:
    cache = _cache(tag)
    mirror = _device._mirror_of(cache)
    D = len(cache.names)
    # Below rows in trial order, the invalid row 3 among them when non-empty.
    below_rows = np.arange(1, 1 + 2 * n_below, 2, dtype=np.int64)
    n_valid_below = int(np.count_nonzero(cache.valid[below_rows]))
    assert n_valid_below == n_below - (1 if n_below >= 2 else 0)
    n_above = cache.n_valid - n_valid_below
    w = _weights(n_valid_below)

    rng = np.random.RandomState(seed)
    x_want, mus, sigmas = _device.draw_below_native(
        core.tpe_below_kernels, cache, below_rows, w, rng, S, ce, mc
    )
    acq_want = mirror.score_fused(
        cache, _device.FusedRequest(below_rows, n_above, x_want, mus, sigmas, w), None, ce, mc, 1.0
    )

    rng2 = np.random.RandomState(seed)
    u = rng2.random_sample(S)
    q = rng2.uniform(low=0, high=1, size=(S, D))
    assert _device.native_draw(cache), "the native draw route must bind on a GPU box"
    entry = _device.native_below(cache)
    best, x_raw, acq = mirror.draw_score_fused(
        cache, _device.DrawRequest(below_rows, n_above, w, u, q, entry), ce, mc, 1.0
    )
    assert x_raw.shape == (S, D) and acq.shape == (S,)
    np.testing.assert_array_equal(_bits(x_raw), _bits(x_want))
    np.testing.assert_array_equal(_bits(acq), _bits(acq_want))
    assert best == int(np.argmax(acq_want))
    assert rng.random_sample() == rng2.random_sample()


@pytest.mark.parametrize("n_below", [0, 2, 25])
@pytest.mark.parametrize("S", [1, 24])
@pytest.mark.parametrize("dims", [1, 3, 20])
def test_draw_score_equals_two_call_route(core, dims, S, n_below) -> None:
    ce = (dims + S + n_below) % 2 == 0
    _check_case(core, str(dims), S, n_below, ce, not ce or dims == 3, seed=dims * 100 + n_below)


@pytest.mark.parametrize("tag", ["log", "step"])
def test_draw_score_log_and_stepped_dims(core, tag) -> None:
    for n_below, ce in ((25, False), (2, True)):
        _check_case(core, tag, 24, n_below, ce, True, seed=5 + n_below)


def _run_study(monkeypatch, env: str):
    calls = {"draw": 0, "two_call": 0}
    orig = _device.score_above_resident

    def spy(*args, **kwargs):
        req = kwargs.get("fused")
        calls["draw" if isinstance(req, _device.DrawRequest) else "two_call"] += 1
        return orig(*args, **kwargs)

    with monkeypatch.context() as m:
        m.setenv("OPTUNA_AMD_TPE_NATIVE_DRAW", env)
        m.setattr(_device, "score_above_resident", spy)
        study = tc.seeded_study(0, tc.MIXED4)
        out = []
        for _ in range(30):
            t = tc.suggest_all(study, tc.MIXED4)
            study.tell(t, tc.mixed4_value(t.params))
            out.append([float(t.params[name]) for name in tc.MIXED4])
        state = study.sampler._rng.rng.get_state()
    return np.array(out), calls, state


def test_study_same_parameters_with_route_on_and_off(core, monkeypatch) -> None:
    p_on, calls_on, s_on = _run_study(monkeypatch, "1")
    assert calls_on == {"draw": 30, "two_call": 0}
    p_off, calls_off, s_off = _run_study(monkeypatch, "0")
    assert calls_off == {"draw": 0, "two_call": 30}
    assert p_on.shape == p_off.shape == (30, 4)
    np.testing.assert_array_equal(_bits(p_on), _bits(p_off))
    np.testing.assert_array_equal(s_on[1], s_off[1])
    assert s_on[2:] == s_off[2:]
