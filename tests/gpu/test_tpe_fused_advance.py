"""The native advance route of the fused TPE suggest (``fused_advance``: split
ledger, table append, index insert, exclusion list, ramp and fit launch in one
native call) against the separate host steps it replaces: two samplers with
one seed run the same ask/tell steps in one process, the route on and
``OPTUNA_AMD_TPE_NATIVE_HISTORY=0``, and must suggest the same bits, leave the
same resident sorted index and hand the same arguments to the fit.

Histories start just past the 512-kernel device threshold; the cases cover a
table and an index that grow past their capacity within the steps, rows
arriving several at once with invalid ones among them, tied values and tied
parameters, a log and a stepped dim, a maximize study, and an exclusion list
on and one past its limit.
"""
from __future__ import annotations

import warnings

import numpy as np
import pytest

import optuna_amd
from optuna_amd import _hip
from optuna_amd.distributions import FloatDistribution
from optuna_amd.samplers import TPESampler
from optuna_amd.samplers._tpe import _device


pytestmark = pytest.mark.gpu

N_STEPS = 30


@pytest.fixture(scope="module", autouse=True)
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    return c


class _Recorder:
    """Forwards to a ``TpeDeviceHistory`` and keeps what reached the fit."""

    def __init__(self, hist, log: list) -> None:
        self._hist = hist
        self._log = log

    def __getattr__(self, name):
        attr = getattr(self._hist, name)
        if name not in ("fused_advance", "fused_prepare", "fused_draw_score", "score"):
            return attr

        def recorded(*args, **kwargs):
            out = attr(*args, **kwargs)
            if name == "fused_advance":
                self._log.append((name, bool(out[8])))
            elif name == "fused_draw_score":
                # excl, n_above, below rows, the ramp
                self._log.append(
                    (name, np.array(args[0]), args[1], np.array(args[4]), tuple(args[15:19]))
                )
            else:
                self._log.append((name,))
            return out

        return recorded


def _value(params: dict) -> float:
    # One decimal: many tied objective values, so the ledger's tie order shows.
    return round(float(sum(v * v for v in params.values())) % 7.0, 1)


def _draw(r, space, lacking=()):
    params = {}
    for name, d in space.items():
        if name in lacking:
            continue
        if d.log:
            x = float(np.exp(r.uniform(np.log(d.low), np.log(d.high))))
        else:
            x = float(r.uniform(d.low, d.high))
        if d.step is not None:
            x = float(d.low + round((x - d.low) / d.step) * d.step)
        params[name] = min(max(x, d.low), d.high)
    return params


def _trials(r, space, n, lacking_rows=(), lacking=()):
    out = []
    lacking_rows = set(lacking_rows)
    for row in range(n):
        params = _draw(r, space, lacking if row in lacking_rows else ())
        if row % 9 == 4 and out and row not in lacking_rows and len(out[-1].params) == len(params):
            params = dict(out[-1].params)  # equal parameter values in two rows
        out.append(
            optuna_amd.create_trial(
                params=params,
                distributions={k: space[k] for k in params},
                # Rows lacking a parameter rank last, so no below set has one.
                value=_value(params) + (10.0 if row in lacking_rows else 0.0),
            )
        )
    return out


def _run(monkeypatch, route_on: bool, space, initial, arrivals, direction, multivariate):
    """One seeded study over ``initial``; ``arrivals`` maps a step to trials
    added ahead of it. Returns (suggested params, log, sorted indices)."""
    if route_on:
        monkeypatch.delenv("OPTUNA_AMD_TPE_NATIVE_HISTORY", raising=False)
    else:
        monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_HISTORY", "0")
    log: list = []
    orig_init = _device._SpaceDeviceMirror.__init__

    def init(self, sp):
        orig_init(self, sp)
        self._hist = _Recorder(self._hist, log)

    monkeypatch.setattr(_device._SpaceDeviceMirror, "__init__", init)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sampler = TPESampler(seed=7, n_startup_trials=5, multivariate=multivariate)
    study = optuna_amd.create_study(sampler=sampler, direction=direction)
    study.add_trials(initial)
    suggested = []
    for step in range(N_STEPS):
        if step in arrivals:
            study.add_trials(arrivals[step])
        log.append(("step", step))
        trial = study.ask()
        params = {
            name: trial.suggest_float(name, d.low, d.high, log=d.log, step=d.step)
            for name, d in space.items()
        }
        suggested.append([params[name] for name in space])
        study.tell(trial, _value(params))
    history = sampler._histories[study._study_id]
    assert (history._ledger is not None) == route_on
    indices = {
        tuple(cache.names): cache._device_mirror._hist.sorted_index()
        for cache in history._spaces.values()
        if getattr(cache, "_device_mirror", None) is not None
    }
    monkeypatch.setattr(_device._SpaceDeviceMirror, "__init__", orig_init)
    return np.array(suggested), log, indices


def _fits(log):
    return [e for e in log if e[0] == "fused_draw_score"]


def _compare(on, off) -> None:
    got, log_on, idx_on = on
    want, log_off, idx_off = off
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    assert idx_on.keys() == idx_off.keys() and idx_on
    for names in idx_on:
        np.testing.assert_array_equal(idx_on[names], idx_off[names])
    fits_on, fits_off = _fits(log_on), _fits(log_off)
    assert len(fits_on) == len(fits_off)
    for a, b in zip(fits_on, fits_off):
        np.testing.assert_array_equal(a[1], b[1])  # excl
        assert a[1].dtype == b[1].dtype == np.int32
        assert a[2] == b[2]  # n_above
        np.testing.assert_array_equal(a[3], b[3])  # below rows
        assert a[4][0] == b[4][0]
        assert np.array_equal(
            np.array(a[4][1:]).view(np.uint64), np.array(b[4][1:]).view(np.uint64)
        )
    assert not any(e[0] == "fused_advance" for e in log_off)


def _advances(log, first_step: int = 0):
    """`launched` of every fused_advance from ``first_step`` on."""
    out, step = [], -1
    for e in log:
        if e[0] == "step":
            step = e[1]
        elif e[0] == "fused_advance" and step >= first_step:
            out.append(e[1])
    return out


def _names_after(log, first_step: int):
    out, step = [], -1
    for e in log:
        if e[0] == "step":
            step = e[1]
        elif step >= first_step:
            out.append(e[0])
    return out


_D3 = {
    "a": FloatDistribution(-5.0, 5.0),
    "l": FloatDistribution(1e-3, 10.0, log=True),
    "s": FloatDistribution(-5.0, 5.0, step=0.5),
}


@pytest.mark.parametrize("direction", ["minimize", "maximize"])
@pytest.mark.parametrize(
    "tag,n0", [("d1", 600), ("d3", 600), ("d3", 1020)], ids=["d1-600", "d3-600", "d3-1020"]
)
def test_route_on_and_off_agree(monkeypatch, tag, n0, direction) -> None:
    space = {"a": FloatDistribution(-5.0, 5.0)} if tag == "d1" else _D3
    initial = _trials(np.random.RandomState(n0), space, n0)
    # Seven rows at once ahead of step 12: one call, one insert launch.
    arrivals = {12: _trials(np.random.RandomState(1), space, 7)}
    runs = [
        _run(monkeypatch, on, space, initial, arrivals, direction, multivariate=tag != "d1")
        for on in (True, False)
    ]
    _compare(*runs)
    log_on = runs[0][1]
    # The first suggest uploads the index in bulk; every later one advances.
    assert _advances(log_on) == [True] * (N_STEPS - 1)
    names = _names_after(log_on, 1)
    assert "fused_prepare" not in names and "score" not in names
    assert names.count("fused_draw_score") == N_STEPS - 1


def test_table_and_index_grow_within_the_steps(monkeypatch) -> None:
    """600 rows give both buffers a capacity of 1200; a bulk arrival of 585
    (past the 64 of one advance: the bulk upload) leaves them 14 short of it,
    and the single tells that follow grow both through the advance call."""
    space = _D3
    initial = _trials(np.random.RandomState(5), space, 600)
    arrivals = {1: _trials(np.random.RandomState(6), space, 585)}
    runs = [
        _run(monkeypatch, on, space, initial, arrivals, "minimize", multivariate=True)
        for on in (True, False)
    ]
    _compare(*runs)
    log_on = runs[0][1]
    assert len(_advances(log_on)) == N_STEPS - 2  # neither the first nor the bulk step
    assert all(_advances(log_on))
    (index,) = runs[0][2].values()
    # Every row but the last tell's, which no suggest has seen yet.
    assert index.shape == (3, 600 + 585 + N_STEPS - 1) and index.shape[1] > 1200


def test_invalid_rows_and_the_exclusion_limit(monkeypatch) -> None:
    """Two parameters sampled one by one, ``b`` missing from 997 of 1640
    trials: its space excludes 25 below rows and the invalid ones. Arrivals
    with invalid rows between valid ones take the list to exactly 1024 (route
    taken) and then to 1025 (no fit launched: the unfused route, same bits)."""
    space = {"a": FloatDistribution(-5.0, 5.0), "b": FloatDistribution(0.0, 1.0)}
    r = np.random.RandomState(3)
    lacking_rows = r.choice(1640, 997, replace=False)
    initial = _trials(r, space, 1640, lacking_rows, lacking=("b",))
    arrivals = {
        10: _trials(r, space, 6, lacking_rows=(1, 4), lacking=("b",)),  # 999 invalid: 1024
        20: _trials(r, space, 3, lacking_rows=(1,), lacking=("b",)),  # 1000 invalid: 1025
    }
    runs = [
        _run(monkeypatch, on, space, initial, arrivals, "minimize", multivariate=False)
        for on in (True, False)
    ]
    _compare(*runs)
    log_on = runs[0][1]
    excl_sizes = sorted({len(e[1]) for e in _fits(log_on)})
    assert excl_sizes[0] == 25 and 1024 in excl_sizes and max(excl_sizes) == 1024
    # Space a advances throughout, space b until the list is one too long.
    assert _advances(log_on, 20) == [True, False] * (N_STEPS - 20)
    assert _advances(log_on)[: 2 * 19] == [True] * (2 * 19)  # steps 1 to 19
    assert _names_after(log_on, 20).count("score") == N_STEPS - 20
    assert _names_after(runs[1][1], 20).count("score") == N_STEPS - 20
