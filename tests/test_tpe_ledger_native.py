"""Native split ledger of the fused TPE suggest (``_hip/csrc/tpe_ledger_host.h``
and its binding ``tpe_ledger_bind.h``).

A stand-alone program (``tests/cpp/tpe_ledger_check.cpp``) runs the header
against a stable sort, plain and under the address and undefined-behaviour
sanitizers. The binding is compiled into a host-only pybind11 module
(``tests/cpp/tpe_ledger_module.cpp``) with the host compiler and compared with
``np.argsort(kind="stable")``, ``np.union1d`` and ``default_weight_ramp``; the
same class then stands behind ``_TpeHistory`` and its ``split`` is compared
with that of a history without a ledger over the same append sequences.
"""
from __future__ import annotations

import datetime
import importlib.util
import shutil
import subprocess
import sysconfig
import types
from pathlib import Path

import numpy as np
import pytest

from optuna_amd.distributions import FloatDistribution
from optuna_amd.samplers._tpe import _device, _history
from optuna_amd.samplers._tpe._history import _TpeHistory
from optuna_amd.study._study_direction import StudyDirection
from optuna_amd.trial import FrozenTrial, TrialState


_ROOT = Path(__file__).resolve().parent.parent
_CSRC = _ROOT / "optuna_amd" / "_hip" / "csrc"
_CPP = Path(__file__).resolve().parent / "cpp"


def _compiler() -> str | None:
    return next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)


@pytest.fixture(scope="module")
def mod(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    pybind11 = pytest.importorskip("pybind11")
    out = tmp_path_factory.mktemp("tpe_ledger") / (
        "_tpe_ledger_host" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so")
    )
    subprocess.run(
        [cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared",
         "-fvisibility=hidden", f"-I{_CSRC}", f"-I{pybind11.get_include()}",
         f"-I{sysconfig.get_paths()['include']}", str(_CPP / "tpe_ledger_module.cpp"),
         "-o", str(out)],
        check=True,
    )
    spec = importlib.util.spec_from_file_location("_tpe_ledger_host", out)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_standalone_program(tmp_path, sanitize) -> None:
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "tpe_ledger_check"
    flags = []
    if sanitize:
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
        # The runtimes go into the program itself (clang's default, asked of
        # gcc): a dynamic runtime refuses to start behind any preloaded library.
        version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        if "clang" not in version:
            flags += ["-static-libasan", "-static-libubsan"]
    subprocess.run(
        [cxx, "-std=c++17", "-O1" if sanitize else "-O2", "-Wall", "-Wextra", "-Werror", *flags,
         f"-I{_CSRC}", str(_CPP / "tpe_ledger_check.cpp"), "-o", str(exe)],
        check=True,
    )
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "tpe_ledger_check ok" in run.stdout


# ---------------------------------------------------------------------------
# The ledger against numpy
# ---------------------------------------------------------------------------


def _random_with_ties(n: int, seed: int) -> np.ndarray:
    r = np.random.RandomState(seed)
    keys = r.uniform(-1.0, 1.0, n)
    for i in range(1, n):
        if r.rand() < 0.1:
            keys[i] = keys[r.randint(i)]
    return keys


_KEY_CASES = {
    "empty": np.empty(0),
    "one": np.array([3.5]),
    "all_equal": np.full(100, 2.0),
    "ascending": np.arange(300) * 0.25,
    "descending": 1e3 - np.arange(300.0),
    "duplicates": np.array([1.0, 0.0, 1.0, 2.0, 0.0, 1.0, 2.0, 2.0, 0.0]),
    "signed_zeros": np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0, 1.0, -0.0]),
    "infinities": np.array([np.inf, 1.0, -np.inf, np.inf, 0.0, -np.inf, 1.0, np.inf, -np.inf]),
    "capacity_64": np.random.RandomState(1).randint(0, 50, 64).astype(float),
    "capacity_65": np.random.RandomState(2).randint(0, 50, 65).astype(float),
    "capacity_129": np.random.RandomState(3).randint(0, 50, 129).astype(float),
    "maximize": -_random_with_ties(500, 4),
    "random_2000": _random_with_ties(2000, 5),
}


def _check_against_argsort(ledger, keys: np.ndarray, name) -> None:
    n = len(keys)
    order = np.argsort(keys, kind="stable")
    got_keys, got_rows = ledger.export()
    assert len(ledger) == n, name
    assert got_rows.dtype == np.int64 and got_keys.dtype == np.float64
    assert np.array_equal(got_rows, order), name
    assert np.array_equal(got_keys.view(np.uint64), keys[order].view(np.uint64)), name
    for k in (0, 1, n // 10, n // 2, max(n - 1, 0), n, n + 1, n + 1000):
        want = np.sort(order[:k])
        got = ledger.below(k)
        assert got.dtype == np.int64 and np.array_equal(got, want), (name, k)


@pytest.mark.parametrize("name", list(_KEY_CASES))
def test_single_inserts_equal_stable_argsort(mod, name) -> None:
    keys = _KEY_CASES[name]
    ledger = mod.TpeSplitLedger()
    for row, key in enumerate(keys):
        ledger.insert(row, float(key))
        if name == "random_2000" and row % 250 == 0:
            _check_against_argsort(ledger, keys[: row + 1], (name, row))
    _check_against_argsort(ledger, keys, name)
    if name.startswith("capacity_"):
        assert ledger.capacity >= len(keys) > ledger.capacity // 2 or len(keys) == 64


@pytest.mark.parametrize("name", list(_KEY_CASES))
@pytest.mark.parametrize("batch", [3, 7, 300, 5000])
def test_batched_inserts_equal_stable_argsort(mod, name, batch) -> None:
    keys = _KEY_CASES[name]
    ledger = mod.TpeSplitLedger()
    for at in range(0, len(keys), batch):
        ledger.insert_many(np.arange(at, min(at + batch, len(keys))), keys[at : at + batch])
    _check_against_argsort(ledger, keys, (name, batch))


def test_nan_keys_are_refused(mod) -> None:
    ledger = mod.TpeSplitLedger()
    ledger.insert(0, 1.0)
    with pytest.raises(ValueError):
        ledger.insert(1, float("nan"))
    with pytest.raises(ValueError):
        ledger.insert_many(np.arange(1, 7), np.array([0.0, 1.0, np.nan, 2.0, 3.0, 4.0]))
    with pytest.raises(ValueError):
        ledger.below(-1)
    assert len(ledger) == 1


def test_exclusion_list_equals_union1d(mod) -> None:
    r = np.random.RandomState(0)
    for n_below, n_invalid in ((0, 0), (0, 5), (5, 0), (1, 1), (100, 37), (1000, 24), (3, 400)):
        below = np.sort(r.choice(5000, n_below, replace=False)).astype(np.int64)
        invalid = np.sort(r.choice(5000, n_invalid, replace=False)).astype(np.int32)
        if n_below and n_invalid:
            invalid[0] = min(invalid[0], below[0])  # some common rows
            invalid = np.unique(np.append(invalid, below[:: max(1, n_below // 3)])).astype(np.int32)
        want = np.union1d(below.astype(np.int32), invalid)
        got = mod.tpe_exclusion_list(below, invalid)
        assert got.dtype == np.int32 and np.array_equal(got, want), (n_below, n_invalid)


def test_weight_ramp_equals_python_bit_for_bit(mod) -> None:
    for prior_weight in (1.0, 0.0, 0.3, 7.5):
        for n in list(range(0, 60)) + [99, 100, 575, 1000, 9975, 10000, 123457]:
            if n == 0 and prior_weight == 0.0:
                continue
            want = _device.default_weight_ramp(n, prior_weight)
            got = mod.tpe_default_weight_ramp(n, prior_weight)
            assert got[0] == want[0]
            assert np.array_equal(
                np.array(got[1:]).view(np.uint64), np.array(want[1:]).view(np.uint64)
            ), (n, prior_weight)


# ---------------------------------------------------------------------------
# _TpeHistory with and without the ledger
# ---------------------------------------------------------------------------

_SPACE = {"x": FloatDistribution(-1.0, 1.0)}
_NOW = datetime.datetime(2024, 1, 1)


def _trial(
    number, value, state=TrialState.COMPLETE, constraints=None, intermediate=None, trial_id=None
):
    return FrozenTrial(
        number=number,
        state=state,
        value=value,
        datetime_start=_NOW,
        datetime_complete=_NOW,
        params={"x": 0.5},
        distributions=_SPACE,
        user_attrs={},
        system_attrs={} if constraints is None else {"constraints": constraints},
        intermediate_values=intermediate or {},
        trial_id=number if trial_id is None else trial_id,
    )


def _study(maximize: bool):
    direction = StudyDirection.MAXIMIZE if maximize else StudyDirection.MINIMIZE
    return types.SimpleNamespace(directions=[direction])


def _pair(monkeypatch, mod):
    """Two empty histories: one that will own a ledger, one that never does."""
    monkeypatch.setattr(_history, "_native_ledger_class", lambda: mod.TpeSplitLedger)
    with_ledger = _TpeHistory()
    monkeypatch.setattr(_history, "_native_ledger_class", lambda: None)
    return with_ledger, _TpeHistory()


def _same_state(a: _TpeHistory, b: _TpeHistory, study, what) -> None:
    n = len(a)
    assert n == len(b)
    assert a._rows_number_ascending == b._rows_number_ascending, what
    assert a._comp_cache_valid == b._comp_cache_valid, what
    for col in ("_numbers", "_states", "_values", "_violations", "_pruned_step",
                "_pruned_value", "_has_intermediate"):
        assert np.array_equal(getattr(a, col), getattr(b, col), equal_nan=True), (what, col)
    # The list is by value whatever the direction and is kept only while the
    # flag holds (without a ledger it goes stale afterwards, unread).
    if a._comp_cache_valid:
        assert np.array_equal(a._comp_rows, b._comp_rows), what
        assert np.array_equal(
            a._comp_vals.view(np.uint64), b._comp_vals.view(np.uint64)
        ), what
    for k in (0, 1, n // 10, n // 4, n, n + 3):
        a._split_memo = b._split_memo = None
        below_a, above_a = a.split(study, k)
        below_b, above_b = b.split(study, k)
        assert np.array_equal(below_a, below_b), (what, k)
        assert np.array_equal(above_a, above_b), (what, k)
        ledger = a.ledger_for(study)
        if ledger is not None:
            assert np.array_equal(ledger.below(k), below_b), (what, k)
            assert np.array_equal(a.complement_rows(below_b), above_b), (what, k)


def _values(n, seed):
    v = _random_with_ties(n, seed)
    v[::17] = 0.0
    v[5::17] = -0.0
    return v


@pytest.mark.parametrize("maximize", [False, True], ids=["minimize", "maximize"])
@pytest.mark.parametrize("first", [1, 40, 300])
def test_split_is_the_same_with_the_ledger(monkeypatch, mod, maximize, first) -> None:
    """A bulk first update, then single tells and a few small batches."""
    vals = _values(first + 150, 11)
    a, b = _pair(monkeypatch, mod)
    study = _study(maximize)
    trials = [_trial(i, float(v)) for i, v in enumerate(vals)]
    batches = [trials[:first]]
    at = first
    r = np.random.RandomState(first)
    while at < len(trials):
        m = 1 if r.rand() < 0.8 else int(r.randint(2, 9))
        batches.append(trials[at : at + m])
        at += m
    for i, batch in enumerate(batches):
        for h in (a, b):
            # The class is asked for at the first update only.
            monkeypatch.setattr(
                _history, "_native_ledger_class",
                (lambda: mod.TpeSplitLedger) if h is a else (lambda: None),
            )
            h.update(batch, 1, delta=True, maximize=maximize)
        if i % 10 == 0 or i == len(batches) - 1:
            _same_state(a, b, study, (first, i))
    assert a._ledger is not None and b._ledger is None
    assert len(a._ledger) == len(trials)
    assert a.ledger_for(study) is a._ledger
    assert a.ledger_for(_study(not maximize)) is None  # the other direction: numpy
    assert a.ledger_for(types.SimpleNamespace(directions=[study.directions[0]] * 2)) is None


def _uncovered(kind: str, number: int) -> FrozenTrial:
    if kind == "pruned":
        return _trial(number, 0.1, state=TrialState.PRUNED, intermediate={3: 0.4})
    if kind == "pruned_no_value":
        return _trial(number, None, state=TrialState.PRUNED)
    if kind == "infeasible":
        return _trial(number, 0.1, constraints=[0.5, -1.0])
    if kind == "nan":
        return _trial(number, float("nan"))
    assert kind == "out_of_order"
    return _trial(number - 30, 0.1, trial_id=number)


@pytest.mark.parametrize("maximize", [False, True], ids=["minimize", "maximize"])
@pytest.mark.parametrize("in_batch", [False, True], ids=["single", "batch"])
@pytest.mark.parametrize(
    "kind", ["pruned", "pruned_no_value", "infeasible", "nan", "out_of_order"]
)
def test_first_uncovered_trial_drops_the_ledger(monkeypatch, mod, kind, in_batch, maximize) -> None:
    vals = _values(140, 3)
    study = _study(maximize)
    a, b = _pair(monkeypatch, mod)
    trials = [_trial(i, float(v)) for i, v in enumerate(vals)]
    trials[100] = _uncovered(kind, 100)
    batches = [trials[:60]] + [[t] for t in trials[60:98]]
    batches += [trials[98:103]] if in_batch else [[t] for t in trials[98:103]]
    batches += [[t] for t in trials[103:120]] + [trials[120:]]
    for i, batch in enumerate(batches):
        for h in (a, b):
            monkeypatch.setattr(
                _history, "_native_ledger_class",
                (lambda: mod.TpeSplitLedger) if h is a else (lambda: None),
            )
            h.update(batch, 1, delta=True, maximize=maximize)
        covered = len(a) <= 100
        assert (a._ledger is not None) == covered, (i, len(a))
        assert (a.ledger_for(study) is not None) == covered
        _same_state(a, b, study, (kind, i))
    assert a._ledger is None and a._ledger_resolved  # for good


@pytest.mark.parametrize("flag", ["_comp_cache_valid", "_rows_number_ascending"])
def test_flipped_flags_force_the_python_paths(monkeypatch, mod, flag) -> None:
    """What tests/tpe/test_sampler_paths.py does by hand: the ledger steps
    aside and ``split`` gives what it gives without one."""
    study = _study(False)
    a, b = _pair(monkeypatch, mod)
    trials = [_trial(i, float(v)) for i, v in enumerate(_values(120, 9))]
    for h, cls in ((a, mod.TpeSplitLedger), (b, None)):
        monkeypatch.setattr(_history, "_native_ledger_class", lambda cls=cls: cls)
        h.update(trials[:80], 1, delta=True)
        for t in trials[80:100]:
            h.update([t], 1, delta=True)
        setattr(h, flag, False)
    assert a._ledger is not None and a.ledger_for(study) is None
    _same_state(a, b, study, flag)
    for t in trials[100:]:
        for h in (a, b):
            h.update([t], 1, delta=True)
            setattr(h, flag, False)
    _same_state(a, b, study, (flag, "after more tells"))


def test_no_ledger_when_switched_off_or_not_offered(monkeypatch, mod) -> None:
    trials = [_trial(i, float(i)) for i in range(5)]
    monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_HISTORY", "0")
    h = _TpeHistory()
    h.update(trials, 1, delta=True)
    assert h._ledger is None
    monkeypatch.delenv("OPTUNA_AMD_TPE_NATIVE_HISTORY")
    monkeypatch.setattr(_history, "_native_ledger_class", lambda: mod.TpeSplitLedger)
    h = _TpeHistory()
    h.update(trials, 2, delta=True)  # a study with two objectives
    assert h._ledger is None and not h._comp_cache_valid
