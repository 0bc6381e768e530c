"""When the sampler takes the native step route of the fused suggest (one
``fused_step`` call from the tell to the chosen candidate) and when it keeps
the two calls ``fused_advance`` + ``fused_draw_score``; and that the RNG sees
the same calls in the same order on either route. The extension is replaced by
a stub core whose draw is a plain function of the two uniform draws, so equal
draws give equal suggestions."""
from __future__ import annotations

import bisect
import warnings

import numpy as np
import pytest

import optuna_amd
from optuna_amd import _hip
from optuna_amd.distributions import FloatDistribution
from optuna_amd.samplers import TPESampler
from optuna_amd.samplers._tpe import _device


class _StubLedger:
    def __init__(self) -> None:
        self._keys: list[float] = []
        self._rows: list[int] = []

    def __len__(self) -> int:
        return len(self._rows)

    def insert(self, row: int, key: float) -> None:
        i = bisect.bisect_right(self._keys, key)
        self._keys.insert(i, key)
        self._rows.insert(i, row)

    def insert_many(self, rows, keys) -> None:
        for row, key in zip(rows.tolist(), keys.tolist()):
            self.insert(row, key)

    def below(self, k: int) -> np.ndarray:
        return np.sort(np.asarray(self._rows[:k], dtype=np.int64))

    def export(self):
        return np.asarray(self._keys, dtype=np.float64), np.asarray(self._rows, dtype=np.int64)


def _fake_draw(u, q, lows, highs):
    """(best, x_raw) from the draws alone."""
    return int(np.argmax(u)), lows + q * (highs - lows)


class _StubHistory:
    """Stands in for ``TpeDeviceHistory``; every call lands in ``log``."""

    draws = True  # False: fused_step completes the advance half and does not draw

    def __init__(self, log: list, dims: int) -> None:
        self._log = log
        self._rows = 0

    def set_domain(self, *args) -> None: ...
    def upload_sorted(self, cols) -> None: ...
    def insert_sorted_by_value(self, first_row, n_new) -> None: ...

    def append(self, block) -> None:
        self._rows += len(block)

    def fused_prepare(self, *args) -> None:
        self._log.append(("fused_prepare",))

    def _advance(self, ledger, n_below, valid, invalid_rows, block, first_row, n_valid,
                 prior_weight):
        assert first_row == self._rows and len(valid) == first_row + len(block) == len(ledger)
        self._rows += len(block)
        below = ledger.below(n_below)
        excl = np.union1d(below.astype(np.int32), invalid_rows).astype(np.int32)
        n_below_valid = int(np.count_nonzero(valid[below]))
        n_above = n_valid - n_below_valid
        return (below, excl, n_below_valid, n_above,
                *_device.default_weight_ramp(n_above, prior_weight), True)

    def fused_advance(self, ledger, n_below, valid, invalid_rows, block, first_row, n_valid,
                      prior_weight, ce, mc):
        self._log.append(("fused_advance",))
        return self._advance(ledger, n_below, valid, invalid_rows, block, first_row, n_valid,
                             prior_weight)

    def fused_draw_score(self, excl, n_above, table, valid, below_rows, bw, u, q, alow, ahigh,
                         kinds, lows, highs, steps, *rest):
        self._log.append(("fused_draw_score", u, q, len(bw)))
        return (*_fake_draw(u, q, lows, highs), np.zeros(len(u)))

    def fused_step(self, ledger, n_below, valid, invalid_rows, block, first_row, n_valid,
                   table, bw, u, q, alow, ahigh, kinds, lows, highs, steps, prior_weight,
                   ce, mc):
        assert len(table) == len(valid)
        adv = self._advance(ledger, n_below, valid, invalid_rows, block, first_row, n_valid,
                            prior_weight)
        drawn = self.draws and len(bw) == adv[2] + 1
        self._log.append(("fused_step", u, q, len(bw), drawn))
        if not drawn:
            return None, adv
        return _fake_draw(u, q, lows, highs)

    def fused_score(self, *args):
        self._log.append(("fused_score",))
        return np.zeros(len(args[2]))

    def score(self, sorted_cols, pos, n_above, logw, alow, ahigh, steps, n_choices,
              prior_weight, x, xedges, ce, mc, **kwargs):
        self._log.append(("score",))
        return np.zeros(len(x))


class _StubHistoryWithoutStep(_StubHistory):
    fused_step = None  # an older extension: getattr(..., None) finds nothing


class _StubCore:
    TpeSplitLedger = _StubLedger

    def __init__(self, log: list, history_cls) -> None:
        self._log = log
        self._history_cls = history_cls

    def available(self) -> bool:
        return True

    def TpeDeviceHistory(self, dims: int):  # noqa: N802
        return self._history_cls(self._log, dims)

    def tpe_draw_bind(self, *capsules) -> bool:
        return True

    tpe_below_kernels = None  # without the draw route: the Python estimator


class _CountingRng:
    """Forwards to a ``RandomState`` and records every method called on it."""

    def __init__(self, rng, calls: list) -> None:
        self._rng = rng
        self._calls = calls

    def __getattr__(self, name):
        attr = getattr(self._rng, name)
        if not callable(attr):
            return attr

        def counted(*args, **kwargs):
            size = kwargs.get("size", args[0] if name == "random_sample" and args else None)
            self._calls.append((name, size))
            return attr(*args, **kwargs)

        return counted


def _install(monkeypatch, history_cls=_StubHistory) -> list:
    events: list = []
    core = _StubCore(events, history_cls)
    monkeypatch.setattr(_hip, "get", lambda: core)
    monkeypatch.setattr(_hip, "is_available", lambda: True)
    monkeypatch.setattr(_device, "device_ready", lambda n_kernels: n_kernels >= 512)
    monkeypatch.setattr(_device, "_draw_capsules", lambda: (object(), object(), object()))
    for name in ("OPTUNA_AMD_TPE_FUSED", "OPTUNA_AMD_TPE_NATIVE_HISTORY",
                 "OPTUNA_AMD_TPE_NATIVE_BELOW", "OPTUNA_AMD_TPE_NATIVE_DRAW",
                 "OPTUNA_AMD_TPE_NATIVE_STEP"):
        monkeypatch.delenv(name, raising=False)
    return events


@pytest.fixture
def log(monkeypatch):
    return _install(monkeypatch)


_SPACE = {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(4)}


def _study(seed: int, n: int = 600, lacking: int = 0, **sampler_kwargs):
    """A seeded study over ``n`` trials; the ``lacking`` best of them miss
    ``x3``, so they are in every below set and invalid for the joint space."""
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sampler = TPESampler(seed=seed, n_startup_trials=5, **sampler_kwargs)
    study = optuna_amd.create_study(sampler=sampler)
    rng = np.random.RandomState(seed)
    trials = []
    for row in range(n):
        names = list(_SPACE)[: 3 if row < lacking else 4]
        params = {name: float(rng.uniform(-5.0, 5.0)) for name in names}
        trials.append(
            optuna_amd.create_trial(
                params=params,
                distributions={name: _SPACE[name] for name in names},
                value=float(row) if row < lacking else 1000.0 + float(rng.rand()),
            )
        )
    study.add_trials(trials)
    calls: list = []
    sampler._rng._rng = _CountingRng(sampler._rng.rng, calls)
    return study, calls


def _step(study, log, calls, names=tuple(_SPACE)):
    """One suggest and its tell: (native calls, RNG calls, suggested params)."""
    del log[:], calls[:]
    t = study.ask()
    params = [t.suggest_float(name, -5.0, 5.0) for name in names]
    out = list(log), list(calls), params
    study.tell(t, 2000.0 + len(study.trials))
    return out


_DRAW_RNG = [("random_sample", 24), ("uniform", (24, 4))]


def test_one_step_call_from_the_second_suggest_on(log) -> None:
    study, calls = _study(1, multivariate=True)
    events, rng_calls, _ = _step(study, log, calls)  # makes the mirror, uploads the index
    assert [e[0] for e in events] == ["fused_prepare", "fused_draw_score"]
    assert rng_calls == _DRAW_RNG
    for _ in range(4):
        events, rng_calls, _ = _step(study, log, calls)
        assert [e[0] for e in events] == ["fused_step"] and events[0][4] is True
        assert events[0][3] == 26  # weights for the 25 below rows and the prior
        assert rng_calls == _DRAW_RNG
    mirror = next(iter(study.sampler._histories[study._study_id]._spaces.values()))._device_mirror
    assert mirror._prepared is None and mirror._n_appended == mirror._rows_sorted_synced == 604


def test_not_drawn_goes_on_with_the_same_draws(monkeypatch, log) -> None:
    study, calls = _study(2, multivariate=True)
    _step(study, log, calls)
    monkeypatch.setattr(_StubHistory, "draws", False)
    for _ in range(2):
        events, rng_calls, _ = _step(study, log, calls)
        assert [e[0] for e in events] == ["fused_step", "fused_draw_score"]
        step, draw = events
        assert step[4] is False
        assert draw[1] is step[1] and draw[2] is step[2]  # the very arrays, not new draws
        assert rng_calls == _DRAW_RNG


def test_below_rows_the_space_does_not_cover(log) -> None:
    """Two groups, (x0, x1, x2) and x3; three of the 25 below rows lack x3. In
    x3's space the weights built ahead of the call are for 26 kernels, the
    ledger gives 22 valid rows, the call does not draw and the suggest ends in
    fused_draw_score with 23 weights and the draws made once."""
    study, calls = _study(3, lacking=3, multivariate=True, group=True)
    _step(study, log, calls)
    events, rng_calls, _ = _step(study, log, calls)
    assert [e[0] for e in events] == ["fused_step"] * 2 + ["fused_draw_score"]
    assert events[0][4] is True and events[0][2].shape == (24, 3)
    step, draw = events[1:]
    assert (step[3], step[4], draw[3]) == (26, False, 23)
    assert draw[1] is step[1] and draw[2] is step[2]
    assert rng_calls == [("random_sample", 24), ("uniform", (24, 3)),
                         ("random_sample", 24), ("uniform", (24, 1))]


@pytest.mark.parametrize("how", ["switch", "no-entry", "no-draw", "no-below", "no-history"])
def test_switches_and_older_extensions_keep_the_two_calls(monkeypatch, how) -> None:
    log = _install(monkeypatch, _StubHistoryWithoutStep if how == "no-entry" else _StubHistory)
    env = {"switch": "OPTUNA_AMD_TPE_NATIVE_STEP", "no-draw": "OPTUNA_AMD_TPE_NATIVE_DRAW",
           "no-below": "OPTUNA_AMD_TPE_NATIVE_BELOW", "no-history": "OPTUNA_AMD_TPE_NATIVE_HISTORY"}
    if how in env:
        monkeypatch.setenv(env[how], "0")
    study, calls = _study(4, multivariate=True)
    _step(study, log, calls)
    for _ in range(2):
        events, rng_calls, _ = _step(study, log, calls)
        names = [e[0] for e in events]
        assert "fused_step" not in names
        if how in ("switch", "no-entry"):
            assert names == ["fused_advance", "fused_draw_score"]
            assert rng_calls == _DRAW_RNG
        elif how == "no-history":
            assert names == ["fused_prepare", "fused_draw_score"]
            assert rng_calls == _DRAW_RNG
        else:
            assert names[0] == "fused_advance" and names[-1] == "fused_score"
            assert [c[0] for c in rng_calls] != [c[0] for c in _DRAW_RNG]


@pytest.mark.parametrize(
    "kwargs,n",
    [
        (dict(multivariate=True, weights=lambda n: np.linspace(0.5, 1.5, n)), 600),
        (dict(multivariate=True, constant_liar=True), 600),
        (dict(multivariate=True), 530),  # above set below the device threshold
    ],
    ids=["custom-weights", "liar-row", "small-history"],
)
def test_ineligible_suggests_never_draw_early(monkeypatch, kwargs, n) -> None:
    """Where the suggest does not end on the native draw route, the step call
    is not made and the RNG calls are those of the same suggest with the step
    route switched off."""
    runs = []
    for switch in ("1", "0"):
        log = _install(monkeypatch)
        monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_STEP", switch)
        study, calls = _study(5, n=n, **kwargs)
        if kwargs.get("constant_liar"):
            running = study.ask()
            for name in _SPACE:
                running.suggest_float(name, -5.0, 5.0)
        seen = []
        for _ in range(3):
            events, rng_calls, params = _step(study, log, calls)
            assert "fused_step" not in [e[0] for e in events]
            seen.append(([e[0] for e in events], rng_calls, params))
        runs.append(seen)
    assert runs[0] == runs[1]


def test_routes_agree_on_suggestions_and_rng_state(monkeypatch) -> None:
    runs = []
    for switch in ("1", "0"):
        log = _install(monkeypatch)
        monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_STEP", switch)
        study, calls = _study(6, lacking=2, multivariate=True, group=True)
        seen = []
        for _ in range(4):
            events, rng_calls, params = _step(study, log, calls)
            seen.append((rng_calls, params))
        assert any(e[0] == "fused_step" for e in log) == (switch == "1")
        runs.append((seen, study.sampler._rng.rng.get_state()))
    (seen_on, s_on), (seen_off, s_off) = runs
    assert seen_on == seen_off
    assert s_on[0] == s_off[0] and s_on[2:] == s_off[2:]
    np.testing.assert_array_equal(s_on[1], s_off[1])


class _Proxy:
    """Stands in front of a history and forwards by name, as call recorders do."""

    def __init__(self, hist) -> None:
        self._hist = hist

    def __getattr__(self, name):
        return getattr(self._hist, name)


@pytest.mark.parametrize("how", ["proxied-history", "wrapped-entry"])
def test_observers_of_the_two_calls_keep_receiving_them(monkeypatch, log, how) -> None:
    """The step entry is looked up on the history's type and travels with the
    draw entry ``native_below`` gives: a forwarding proxy in front of the
    history, or a wrapper around that entry, keeps the two calls."""
    if how == "proxied-history":
        orig_init = _device._SpaceDeviceMirror.__init__

        def init(mirror, space):
            orig_init(mirror, space)
            mirror._hist = _Proxy(mirror._hist)

        monkeypatch.setattr(_device._SpaceDeviceMirror, "__init__", init)
    else:
        orig_native = _device.native_below

        def native_below(cache):
            fn = orig_native(cache)
            return None if fn is None else (lambda *args: fn(*args))

        monkeypatch.setattr(_device, "native_below", native_below)
    study, calls = _study(7, multivariate=True)
    _step(study, log, calls)
    for _ in range(2):
        events, rng_calls, _ = _step(study, log, calls)
        assert [e[0] for e in events] == ["fused_advance", "fused_draw_score"]
        assert rng_calls == _DRAW_RNG
