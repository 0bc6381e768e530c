"""Host-side order of the two-call fused suggest: the sampler launches the
above-set fit (``fused_prepare``) before it builds the below estimator, only on
the fused path, and the mirror sync and the exclusion list are done once per
suggest. The extension is replaced by a stub core that records its calls."""
from __future__ import annotations

import numpy as np
import pytest

import optuna_amd
from optuna_amd import _hip
from optuna_amd.distributions import FloatDistribution
from optuna_amd.samplers import TPESampler
from optuna_amd.samplers._tpe import _device
from optuna_amd.samplers._tpe._history import _SpaceCache


class _StubHistory:
    """Stands in for ``TpeDeviceHistory``; every call lands in ``log``."""

    def __init__(self, log: list, dims: int) -> None:
        self._log = log
        self._dims = dims
        self._rows = 0
        log.append(("new", dims))

    def set_domain(self, alow, ahigh, steps, n_choices) -> None:
        self._log.append(("set_domain",))

    def append(self, block) -> None:
        assert block.shape[1] == self._dims
        self._rows += len(block)
        self._log.append(("append", len(block)))

    def upload_sorted(self, cols) -> None:
        self._log.append(("upload_sorted", len(cols[0]) if cols else 0))

    def insert_sorted_by_value(self, first_row, n_new) -> None:
        self._log.append(("insert_sorted_by_value", first_row, n_new))

    def fused_prepare(self, *args) -> None:
        self._log.append(("fused_prepare", args))

    def fused_score(self, *args):
        self._log.append(("fused_score", args))
        return np.zeros(len(args[2]))

    def score(self, sorted_cols, pos, n_above, logw, alow, ahigh, steps, n_choices,
              prior_weight, x, xedges, ce, mc, **kwargs):
        self._log.append(("score",))
        return np.zeros(len(x))


class _StubCore:
    def __init__(self, log: list) -> None:
        self._log = log

    def available(self) -> bool:
        return True

    def TpeDeviceHistory(self, dims: int) -> _StubHistory:  # noqa: N802
        return _StubHistory(self._log, dims)


@pytest.fixture
def log(monkeypatch):
    """Stub core in place; the log also records the host steps of interest."""
    events: list = []
    core = _StubCore(events)
    monkeypatch.setattr(_hip, "get", lambda: core)
    monkeypatch.setattr(_hip, "is_available", lambda: True)
    monkeypatch.setattr(_device, "device_ready", lambda n_kernels: n_kernels >= 512)

    def wrap(cls, name, tag):
        orig = getattr(cls, name)

        def wrapped(self, *args, **kwargs):
            events.append((tag,))
            return orig(self, *args, **kwargs)

        monkeypatch.setattr(cls, name, wrapped)

    wrap(TPESampler, "_build_mpe", "build_mpe")
    wrap(_device._SpaceDeviceMirror, "sync", "sync")
    wrap(_SpaceCache, "excluded_rows", "excluded_rows")
    return events


def _study(seed: int, n: int = 600, **sampler_kwargs):
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    space = {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(4)}
    rng = np.random.RandomState(seed)
    study = optuna_amd.create_study(
        sampler=TPESampler(seed=seed, n_startup_trials=5, **sampler_kwargs)
    )
    trials = []
    for _ in range(n):
        params = {name: float(rng.uniform(-5.0, 5.0)) for name in space}
        value = float(sum(v**2 for v in params.values()))
        trials.append(optuna_amd.create_trial(params=params, distributions=space, value=value))
    study.add_trials(trials)
    return study, space


def _suggest(study, space):
    t = study.ask()
    for name, dist in space.items():
        t.suggest_float(name, dist.low, dist.high)
    return t


def _names(events: list) -> list[str]:
    return [e[0] for e in events]


def test_prepare_runs_before_the_below_estimator(monkeypatch, log) -> None:
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    study, space = _study(1)
    _suggest(study, space)
    names = _names(log)
    assert names.count("fused_prepare") == 1 and names.count("fused_score") == 1
    assert names.count("build_mpe") == 1  # the below estimator only
    assert names.index("fused_prepare") < names.index("build_mpe") < names.index("fused_score")
    # The mirror was brought up to date before the fit was launched.
    assert names.index("append") < names.index("upload_sorted") < names.index("fused_prepare")


def test_sync_and_exclusion_list_once_per_suggest(monkeypatch, log) -> None:
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    study, space = _study(2)
    for step in range(3):
        del log[:]
        t = _suggest(study, space)
        names = _names(log)
        assert names.count("sync") == 1, names
        assert names.count("excluded_rows") == 1, names
        assert names.count("fused_prepare") == 1 and names.count("fused_score") == 1
        study.tell(t, float(step))


def test_score_receives_the_prepared_arguments(monkeypatch, log) -> None:
    """The scoring call passes the very fit arguments of the prepare call, so
    the native side finds its prepared fit valid."""
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    study, space = _study(3, weights=lambda n: np.linspace(0.5, 1.5, n))
    _suggest(study, space)
    (prep,) = [e[1] for e in log if e[0] == "fused_prepare"]
    (score,) = [e[1] for e in log if e[0] == "fused_score"]
    # prepare: excl, n_above, logw, w_num, w_start, w_step, log_total, pw, ce, mc
    # score:   excl, n_above, x, xedges, bmu, bsig, bw, logw, w_num, ..., mc, parts
    assert score[0] is prep[0] and score[1] == prep[1] == 575
    assert score[7] is prep[2] and score[7].shape == (576,)
    assert tuple(score[8:15]) == tuple(prep[3:10])
    assert score[2].shape == (24, 4) and score[4].shape == (26, 4)


def test_no_prepare_on_the_unfused_path(monkeypatch, log) -> None:
    monkeypatch.setenv("OPTUNA_AMD_TPE_FUSED", "0")
    study, space = _study(1)
    _suggest(study, space)
    names = _names(log)
    assert "fused_prepare" not in names and "fused_score" not in names
    assert names.count("score") == 1


def test_no_prepare_below_the_device_threshold(monkeypatch, log) -> None:
    """Small histories stay on the host: no mirror, no prepare."""
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    study, space = _study(1, n=100)
    _suggest(study, space)
    assert _names(log).count("build_mpe") == 2  # below and above, on the host
    assert "fused_prepare" not in _names(log) and "new" not in _names(log)


def test_score_without_prepare_prepares_itself(monkeypatch, log) -> None:
    """Direct callers of the scoring entry get the same two native calls."""
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    study, space = _study(4)
    _suggest(study, space)  # fills the sampler's history
    history = study.sampler._histories[study._study_id]
    cache = history.space_cache(space)
    below = np.arange(25)
    req = _device.FusedRequest(
        below_rows=below, n_above=len(cache.valid) - 25,
        x_raw=np.zeros((24, 4)), below_mus=np.zeros((26, 4)),
        below_sigmas=np.ones((26, 4)), below_weights=np.full(26, 1 / 26),
    )
    del log[:]
    _device.score_above_resident(cache, None, None, None, False, True, fused=req)
    names = _names(log)
    assert names.count("fused_prepare") == 1 and names.count("fused_score") == 1
    assert names.count("sync") == 1 and names.count("excluded_rows") == 1
    # A prepare for another split is not taken over by the scoring call.
    del log[:]
    _device.prepare_fused_resident(cache, np.arange(10), len(cache.valid) - 10, None, False, True)
    _device.score_above_resident(cache, None, None, None, False, True, fused=req)
    names = _names(log)
    assert names.count("fused_prepare") == 2 and names.count("fused_score") == 1
    score_args = [e[1] for e in log if e[0] == "fused_score"][0]
    np.testing.assert_array_equal(score_args[0], np.arange(25))
