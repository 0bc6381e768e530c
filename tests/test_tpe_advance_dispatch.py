"""When the sampler takes the native advance route of the fused suggest (one
``fused_advance`` call in place of the split, the mirror sync, the exclusion
list and ``fused_prepare``) and when it keeps the separate steps. The
extension is replaced by a stub core that records its calls; its ledger and
its ``fused_advance`` are Python transcriptions of the native ones."""
from __future__ import annotations

import bisect
import warnings

import numpy as np
import pytest

import optuna_amd
from optuna_amd import _hip
from optuna_amd.distributions import CategoricalDistribution, FloatDistribution
from optuna_amd.samplers import TPESampler
from optuna_amd.samplers._tpe import _device
from optuna_amd.samplers._tpe._history import _SpaceCache, _TpeHistory
from optuna_amd.trial import FrozenTrial, TrialState


class _StubLedger:
    def __init__(self) -> None:
        self._keys: list[float] = []
        self._rows: list[int] = []

    def __len__(self) -> int:
        return len(self._rows)

    def insert(self, row: int, key: float) -> None:
        assert key == key
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


class _StubHistory:
    """Stands in for ``TpeDeviceHistory``; every call lands in ``log``."""

    fits = True  # False: fused_advance reports a fused limit that does not hold

    def __init__(self, log: list, dims: int) -> None:
        self._log = log
        self._dims = dims
        self._rows = 0
        log.append(("new", dims))

    def set_domain(self, alow, ahigh, steps, n_choices) -> None:
        self._log.append(("set_domain",))

    def append(self, block) -> None:
        self._rows += len(block)
        self._log.append(("append", len(block)))

    def upload_sorted(self, cols) -> None:
        self._log.append(("upload_sorted", len(cols[0]) if cols else 0))

    def insert_sorted_by_value(self, first_row, n_new) -> None:
        self._log.append(("insert_sorted_by_value", first_row, n_new))

    def fused_prepare(self, *args) -> None:
        self._log.append(("fused_prepare", args))

    def fused_advance(self, ledger, n_below, valid, invalid_rows, block, first_row, n_valid,
                      prior_weight, consider_endpoints, magic_clip):
        assert first_row == self._rows and block.shape[1] == self._dims
        assert len(valid) == first_row + len(block) == len(ledger)
        assert valid.dtype == bool and invalid_rows.dtype == np.int32
        self._rows += len(block)
        below = ledger.below(n_below)
        excl = np.union1d(below.astype(np.int32), invalid_rows).astype(np.int32)
        n_below_valid = int(np.count_nonzero(valid[below]))
        n_above = n_valid - n_below_valid
        out = (below, excl, n_below_valid, n_above,
               *_device.default_weight_ramp(n_above, prior_weight), self.fits)
        self._log.append(("fused_advance", (n_below, len(block), first_row, n_valid), out))
        return out

    def fused_score(self, *args):
        self._log.append(("fused_score", args))
        return np.zeros(len(args[2]))

    def score(self, sorted_cols, pos, n_above, logw, alow, ahigh, steps, n_choices,
              prior_weight, x, xedges, ce, mc, **kwargs):
        self._log.append(("score",))
        return np.zeros((len(x), self._dims) if kwargs.get("per_dim") else len(x))


class _StubHistoryWithoutAdvance(_StubHistory):
    fused_advance = None  # an older extension: getattr(..., None) finds nothing


class _StubCore:
    TpeSplitLedger = _StubLedger

    def __init__(self, log: list, history_cls=_StubHistory) -> None:
        self._log = log
        self._history_cls = history_cls

    def available(self) -> bool:
        return True

    def TpeDeviceHistory(self, dims: int):  # noqa: N802
        return self._history_cls(self._log, dims)


def _install(monkeypatch, history_cls=_StubHistory) -> list:
    events: list = []
    core = _StubCore(events, history_cls)
    monkeypatch.setattr(_hip, "get", lambda: core)
    monkeypatch.setattr(_hip, "is_available", lambda: True)
    monkeypatch.setattr(_device, "device_ready", lambda n_kernels: n_kernels >= 512)
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    monkeypatch.delenv("OPTUNA_AMD_TPE_NATIVE_HISTORY", raising=False)

    def wrap(cls, name, tag):
        orig = getattr(cls, name)

        def wrapped(self, *args, **kwargs):
            events.append((tag,))
            return orig(self, *args, **kwargs)

        monkeypatch.setattr(cls, name, wrapped)

    wrap(_device._SpaceDeviceMirror, "sync", "sync")
    wrap(_SpaceCache, "excluded_rows", "excluded_rows")
    wrap(_TpeHistory, "split", "split")
    return events


@pytest.fixture
def log(monkeypatch):
    return _install(monkeypatch)


_SPACE = {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(4)}


def _make_trials(rng, n, space=_SPACE, **kwargs):
    trials = []
    for _ in range(n):
        params = {
            name: (
                d.choices[rng.randint(len(d.choices))]
                if isinstance(d, CategoricalDistribution)
                else float(rng.uniform(d.low, d.high))
            )
            for name, d in space.items()
        }
        value = float(sum(v**2 for v in params.values() if isinstance(v, float)))
        trials.append(
            optuna_amd.create_trial(params=params, distributions=space, value=value, **kwargs)
        )
    return trials


def _study(seed: int, n: int = 600, space=_SPACE, directions=None, **sampler_kwargs):
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sampler = TPESampler(seed=seed, n_startup_trials=5, multivariate=True, **sampler_kwargs)
    study = optuna_amd.create_study(sampler=sampler, directions=directions or ["minimize"])
    rng = np.random.RandomState(seed)
    if len(study.directions) == 1:
        study.add_trials(_make_trials(rng, n, space))
    else:
        for t in _make_trials(rng, n, space):
            study.add_trial(
                optuna_amd.create_trial(
                    params=t.params, distributions=space, values=[t.value, -t.value]
                )
            )
    return study, rng


def _suggest(study, space=_SPACE):
    t = study.ask()
    for name, dist in space.items():
        if isinstance(dist, CategoricalDistribution):
            t.suggest_categorical(name, dist.choices)
        else:
            t.suggest_float(name, dist.low, dist.high)
    return t


def _step(study, log, space=_SPACE, value=1.0) -> list[str]:
    """One suggest and its tell; the names of the calls the suggest made."""
    del log[:]
    t = _suggest(study, space)
    names = [e[0] for e in log]
    study.tell(t, value if len(study.directions) == 1 else [value, value])
    return names


_REPLACED = ("split", "sync", "excluded_rows", "fused_prepare", "append", "insert_sorted_by_value",
             "upload_sorted")


def _assert_advanced(names) -> None:
    assert names.count("fused_advance") == 1, names
    assert not [n for n in names if n in _REPLACED], names
    assert names.count("fused_score") == 1 and "score" not in names


def _assert_todays_route(names, fused: bool = True) -> None:
    assert "fused_advance" not in names, names
    assert names.count("split") >= 1, names
    if fused:
        assert names.count("sync") == 1 and names.count("excluded_rows") == 1, names
        assert names.count("fused_prepare") == 1 and names.count("fused_score") == 1, names


def test_one_advance_call_from_the_second_suggest_on(log) -> None:
    study, _ = _study(1)
    _assert_todays_route(_step(study, log))  # makes the mirror, uploads the index
    assert ("upload_sorted", 600) in log
    for step in range(4):
        names = _step(study, log, value=float(step))
        _assert_advanced(names)
        (adv,) = [e for e in log if e[0] == "fused_advance"]
        n_rows = 600 + step + 1
        assert adv[1] == (25, 1, n_rows - 1, n_rows)
    # A suggest with no tell in between advances too, with an empty block.
    _suggest(study)
    del log[:]
    _suggest(study)
    (adv,) = [e for e in log if e[0] == "fused_advance"]
    assert adv[1] == (25, 0, 605, 605)
    _assert_advanced([e[0] for e in log])


def test_score_receives_what_the_advance_returned(log) -> None:
    study, _ = _study(2)
    _step(study, log)
    _step(study, log)
    (adv,) = [e[2] for e in log if e[0] == "fused_advance"]
    (score,) = [e[1] for e in log if e[0] == "fused_score"]
    # advance: below, excl, n_below_valid, n_above, w_num, w_start, w_step, log_total, ok
    # score:   excl, n_above, x, xedges, bmu, bsig, bw, logw, w_num, ..., mc, parts
    assert score[0] is adv[1] and score[1] == adv[3] == 601 - 25
    assert len(score[7]) == 0
    assert tuple(score[8:12]) == tuple(adv[4:8])
    assert score[12] == 1.0 and tuple(score[13:15]) == (False, True)
    assert score[4].shape == (26, 4)
    history = study.sampler._histories[study._study_id]
    mirror = history.space_cache(_SPACE)._device_mirror
    assert mirror._prepared is None  # taken over by the scoring call
    assert mirror._n_appended == mirror._rows_sorted_synced == 601
    assert history._split_memo is None or history._split_memo[0] == 600


def test_sixty_five_rows_at_once_take_the_bulk_route(log) -> None:
    study, rng = _study(3)
    _step(study, log)
    study.add_trials(_make_trials(rng, 64))  # with the tell above: 65 new rows
    names = _step(study, log)
    _assert_todays_route(names)
    assert ("upload_sorted", 665) in log
    _assert_advanced(_step(study, log))
    study.add_trials(_make_trials(rng, 63))  # 64 with the tell: one advance
    _assert_advanced(_step(study, log))
    assert [e[1] for e in log if e[0] == "fused_advance"] == [(25, 64, 666, 730)]


@pytest.mark.parametrize("kind", ["pruned", "infeasible", "nan"])
def test_an_uncovered_trial_ends_the_route_for_good(monkeypatch, log, kind) -> None:
    study, rng = _study(4)
    _step(study, log)
    _assert_advanced(_step(study, log))
    (trial,) = _make_trials(rng, 1)
    if kind == "pruned":
        trial.state = TrialState.PRUNED
    elif kind == "infeasible":
        trial.system_attrs["constraints"] = [1.0]
    else:
        # No public call stores a NaN value for a complete trial; the mirror
        # guards against one all the same.
        trial._values = [float("nan")]
        monkeypatch.setattr(FrozenTrial, "_validate", lambda self: None)
    study.add_trial(trial)
    history = study.sampler._histories[study._study_id]
    assert history._ledger is not None
    for _ in range(3):
        names = _step(study, log)
        _assert_todays_route(names)
        assert history._ledger is None


def test_two_objectives_keep_todays_route(log) -> None:
    study, _ = _study(5, directions=["minimize", "maximize"])
    for _ in range(3):
        names = _step(study, log)
        assert "fused_advance" not in names and "split" in names
    assert study.sampler._histories[study._study_id]._ledger is None


def test_constant_liar_row_keeps_todays_route(log) -> None:
    study, _ = _study(6, constant_liar=True)
    _step(study, log)
    _assert_advanced(_step(study, log))  # no running trial: no liar row
    running = _suggest(study)  # stays RUNNING, with all its parameters
    for _ in range(2):
        names = _step(study, log)
        assert "fused_advance" not in names and "split" in names and "score" in names
    # A failed trial never enters the history, so the order of the rows holds.
    study.tell(running, state=TrialState.FAIL)
    _assert_advanced(_step(study, log))
    (adv,) = [e for e in log if e[0] == "fused_advance"]
    assert adv[1][1] == 1 and adv[1][2] == 603  # the liar steps kept the mirror in step


def test_custom_weights_keep_todays_route(log) -> None:
    study, _ = _study(7, weights=lambda n: np.linspace(0.5, 1.5, n))
    for _ in range(3):
        _assert_todays_route(_step(study, log))


def test_categorical_dim_keeps_todays_route(log) -> None:
    space = dict(_SPACE, c=CategoricalDistribution(("u", "v", "w")))
    study, _ = _study(8, space=space)
    for _ in range(3):
        names = _step(study, log, space)
        assert "fused_advance" not in names and "split" in names and "score" in names


def test_history_below_the_device_threshold_stays_on_the_host(log) -> None:
    study, _ = _study(9, n=100)
    for _ in range(3):
        names = _step(study, log)
        assert "fused_advance" not in names and "new" not in names and "split" in names
    # 530 valid rows: the above set of the present route has 505 kernels and
    # stays on the host; the advance route's pre-check (530 - 25 < 512) agrees.
    study, _ = _study(9, n=530)
    for _ in range(3):
        names = _step(study, log)
        assert "fused_advance" not in names and "new" not in names and "split" in names


def test_environment_switch_keeps_todays_route(monkeypatch, log) -> None:
    monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_HISTORY", "0")
    study, _ = _study(10)
    for _ in range(3):
        _assert_todays_route(_step(study, log))
    assert study.sampler._histories[study._study_id]._ledger is None


def test_extension_without_the_entry_keeps_todays_route(monkeypatch) -> None:
    log = _install(monkeypatch, _StubHistoryWithoutAdvance)
    study, _ = _study(11)
    for _ in range(3):
        _assert_todays_route(_step(study, log))
    # The ledger alone still serves the split, through its export.
    assert study.sampler._histories[study._study_id]._ledger is not None


def test_failed_limit_goes_on_from_behind_the_split(monkeypatch, log) -> None:
    study, _ = _study(12)
    _step(study, log)
    monkeypatch.setattr(_StubHistory, "fits", False)
    for _ in range(2):
        names = _step(study, log)
        # The advance brought the mirror up to date and gave the below rows;
        # from there on the steps are the usual ones. (The stub's limit is
        # made up, so they end in the fused calls; the native limits are
        # those of fused_eligible, which then chooses the unfused scoring.)
        assert names.count("fused_advance") == 1 and "split" not in names
        assert "append" not in names and "insert_sorted_by_value" not in names
        assert names[1:] == ["sync", "excluded_rows", "fused_prepare", "fused_score"]
    monkeypatch.setattr(_StubHistory, "fits", True)
    _assert_advanced(_step(study, log))
