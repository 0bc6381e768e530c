"""The native step route of the fused TPE suggest (one ``fused_step`` call from
the tell to the chosen candidate, the told row and the exclusion list passed
to the kernels by value) against the two-call route it replaces
(``OPTUNA_AMD_TPE_NATIVE_STEP=0``), bit for bit: twin studies with the same
seeds, one per route, are stepped side by side, and after every step the
suggested parameters, the resident sorted index and the told row of the device
table are compared; ``fused_score(..., return_parts=True)`` on both histories
with the same inputs closes each case.

Shapes: 1, 3, 20 and 33 dims (33 is past the by-value row, so the copy takes
over); histories that cross the 256-row fit tile and one right after start-up
(with the device threshold lowered); exclusion lists of 63, 64 and 65 rows
(64 is the by-value limit); told values that are the smallest, the largest and
an exact duplicate in every dim; two rows between suggests; a maximise study.
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
from optuna_amd.trial import TrialState


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    return c


class _Counter:
    """Forwards to a ``TpeDeviceHistory`` and counts the calls by name. The
    step entry is looked up on the history's type, so it is a method here."""

    def __init__(self, hist, counts: dict) -> None:
        self._hist = hist
        self._counts = counts

    def fused_step(self, *args):
        self._counts["fused_step"] = self._counts.get("fused_step", 0) + 1
        return self._hist.fused_step(*args)

    def __getattr__(self, name):
        attr = getattr(self._hist, name)
        if not name.startswith("fused_") and name != "append":
            return attr

        def counted(*args, **kwargs):
            self._counts[name] = self._counts.get(name, 0) + 1
            return attr(*args, **kwargs)

        return counted


def _space(dims: int) -> dict:
    space = {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(dims)}
    if dims >= 3:
        space["x1"] = FloatDistribution(1e-3, 10.0, log=True)
        space["x2"] = FloatDistribution(-5.0, 5.0, step=0.5)
    return space


def _value(params: dict) -> float:
    # One decimal: tied objective values, so the ledger's tie order shows.
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


def _trial(space, params, value):
    return optuna_amd.create_trial(
        params=params, distributions={k: space[k] for k in params}, value=value
    )


def _trials(r, space, n, n_lacking=0, lacking=()):
    """``n`` trials; the first ``n_lacking`` miss the ``lacking`` parameters
    and rank last, so that no below set holds one."""
    out = []
    for row in range(n):
        params = _draw(r, space, lacking if row < n_lacking else ())
        out.append(_trial(space, params, _value(params) + (10.0 if row < n_lacking else 0.0)))
    return out


class _Twin:
    """One of the two studies: ``switch`` is its OPTUNA_AMD_TPE_NATIVE_STEP."""

    def __init__(self, monkeypatch, switch, space, initial, direction, sampler_kwargs) -> None:
        self._mp, self._switch, self.space = monkeypatch, switch, space
        self.counts: dict = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sampler = TPESampler(seed=11, n_startup_trials=10, **sampler_kwargs)
        self.study = optuna_amd.create_study(sampler=sampler, direction=direction)
        self.study.add_trials(initial)

    def suggest(self):
        self._mp.setenv("OPTUNA_AMD_TPE_NATIVE_STEP", self._switch)
        orig_init = _device._SpaceDeviceMirror.__init__
        counts = self.counts

        def init(mirror, sp):
            orig_init(mirror, sp)
            mirror._hist = _Counter(mirror._hist, counts)

        self._mp.setattr(_device._SpaceDeviceMirror, "__init__", init)
        trial = self.study.ask()
        params = {
            name: trial.suggest_float(name, d.low, d.high, log=d.log, step=d.step)
            for name, d in self.space.items()
        }
        self._mp.setattr(_device._SpaceDeviceMirror, "__init__", orig_init)
        return trial, params

    def caches(self):
        history = self.study.sampler._histories[self.study._study_id]
        return {
            tuple(c.names): c
            for c in history._spaces.values()
            if getattr(c, "_device_mirror", None) is not None
        }


def _parts(cache, seed: int):
    """``fused_score(..., return_parts=True)`` on the cache's device history
    for inputs that depend on the table's size and ``seed`` alone."""
    hist = cache._device_mirror._hist
    n, dims = hist.n_rows, len(cache.names)
    r = np.random.RandomState(seed)
    excl = cache.excluded_rows(np.arange(0, n, max(1, n // 9)))
    n_above = hist.n_sorted - int(np.count_nonzero(cache.valid[:n][excl]))
    mirror = cache._device_mirror
    x = r.uniform(mirror._alow, mirror._ahigh, size=(7, dims))
    xedges = np.concatenate([x - 0.25, x + 0.25], axis=1) if mirror._has_steps else np.empty(0)
    bmu = r.uniform(mirror._alow, mirror._ahigh, size=(3, dims))
    bsig = r.uniform(0.5, 2.0, size=(3, dims))
    bw = np.array([0.2, 0.3, 0.5])
    ramp = _device.default_weight_ramp(n_above, 1.0)
    return hist.fused_score(
        excl, n_above, x, xedges, bmu, bsig, bw, np.empty(0), *ramp, 1.0, False, True, True
    )


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run_twins(monkeypatch, space, initial, n_steps, *, direction="minimize", arrivals=None,
               crafted=None, min_kernels=None, **sampler_kwargs):
    """Steps both routes side by side and compares after every step.
    ``arrivals`` maps a step to trials added ahead of its suggest (with the
    tell before it: more than one new row); ``crafted`` maps a step to a
    function of the study giving the parameters told in place of the
    suggested ones (the suggested trial fails: exactly one new row)."""
    if min_kernels is not None:
        monkeypatch.setattr(_device, "DEVICE_MIN_KERNELS", min_kernels)
    sampler_kwargs.setdefault("multivariate", True)
    twins = [
        _Twin(monkeypatch, switch, space, initial, direction, sampler_kwargs)
        for switch in ("1", "0")
    ]
    for step in range(n_steps):
        outs = []
        for twin in twins:
            if arrivals and step in arrivals:
                twin.study.add_trials(arrivals[step])
            outs.append(twin.suggest())
        (t_on, p_on), (t_off, p_off) = outs
        assert list(p_on) == list(p_off)
        np.testing.assert_array_equal(_bits(list(p_on.values())), _bits(list(p_off.values())))
        c_on, c_off = (twin.caches() for twin in twins)
        assert c_on.keys() == c_off.keys()
        for names in c_on:
            h_on, h_off = (c[names]._device_mirror._hist for c in (c_on, c_off))
            assert h_on.n_rows == h_off.n_rows and h_on.n_sorted == h_off.n_sorted
            np.testing.assert_array_equal(h_on.sorted_index(), h_off.sorted_index())
            # The rows this step brought (the told row, the arrivals with it):
            # equal on both routes, and the host table's rows in the KDE domain.
            n_new = 1 + (len(arrivals[step]) if arrivals and step in arrivals else 0)
            first = max(0, h_on.n_rows - n_new)
            rows_on = h_on.table_rows(first, h_on.n_rows - first)
            rows_off = h_off.table_rows(first, h_off.n_rows - first)
            np.testing.assert_array_equal(_bits(rows_on), _bits(rows_off))
            host = np.array(c_on[names].params[first : h_on.n_rows], dtype=np.float64)
            is_log = c_on[names]._device_mirror._is_log
            host[:, is_log] = np.log(host[:, is_log])
            np.testing.assert_array_equal(_bits(rows_on), _bits(host))
        for twin, trial, params in zip(twins, (t_on, t_off), (p_on, p_off)):
            if crafted and step in crafted:
                twin.study.tell(trial, state=TrialState.FAIL)
                told = crafted[step](twin.study)
                twin.study.add_trial(_trial(space, told, _value(told)))
            else:
                twin.study.tell(trial, _value(params))
    c_on, c_off = (twin.caches() for twin in twins)
    assert c_on
    for names in c_on:
        (parts_on, lw_on), (parts_off, lw_off) = (_parts(c[names], 5) for c in (c_on, c_off))
        assert parts_on.shape == (3, 7)
        np.testing.assert_array_equal(_bits(parts_on), _bits(parts_off))
        np.testing.assert_array_equal(_bits(lw_on), _bits(lw_off))
    return twins


@pytest.mark.parametrize("dims", [1, 3, 20, 33])
def test_routes_agree_over_dims(monkeypatch, dims) -> None:
    space = _space(dims)
    initial = _trials(np.random.RandomState(dims), space, 600)
    on, off = _run_twins(monkeypatch, space, initial, 24)
    # The first suggest uploads the index in bulk; every later one is one call.
    assert on.counts.get("fused_step") == 23 and "fused_advance" not in on.counts
    assert "fused_step" not in off.counts and off.counts.get("fused_advance") == 23
    assert on.counts.get("append") == off.counts.get("append") == 1


def test_routes_agree_on_a_maximise_study(monkeypatch) -> None:
    space = _space(3)
    initial = _trials(np.random.RandomState(8), space, 600)
    on, _ = _run_twins(monkeypatch, space, initial, 12, direction="maximize")
    assert on.counts.get("fused_step") == 11


@pytest.mark.parametrize("n0", [11, 254], ids=["start-up", "fit-tile"])
def test_small_histories_and_the_fit_tile(monkeypatch, n0) -> None:
    """With the device threshold lowered: 11 rows right after the 10 start-up
    trials, and 254 rows growing through 255, 256 and 257, the fit's tile."""
    space = _space(3)
    initial = _trials(np.random.RandomState(n0), space, n0)
    on, _ = _run_twins(monkeypatch, space, initial, 8, min_kernels=1)
    assert on.counts.get("fused_step") == 7


def test_exclusion_lists_around_the_by_value_limit(monkeypatch) -> None:
    """Two groups, (x0, x1) and b; 37 of 600 trials lack b, so b's list holds
    25 below rows and 37 rows its space does not cover. One more such trial
    arrives ahead of steps 2, 4 and 6 (with the tell: two rows at once, the
    copy route): 63, 64 (the last by value) and 65 rows (the staged upload)."""
    space = {"x0": FloatDistribution(-5.0, 5.0), "x1": FloatDistribution(-5.0, 5.0),
             "b": FloatDistribution(0.0, 1.0)}
    r = np.random.RandomState(3)
    initial = _trials(r, space, 600, n_lacking=37, lacking=("b",))
    arrivals = {s: _trials(r, space, 1, n_lacking=1, lacking=("b",)) for s in (2, 4, 6)}
    on, off = _run_twins(monkeypatch, space, initial, 9, arrivals=arrivals, group=True)
    cache = on.caches()[("b",)]
    assert cache.n_invalid == 40 and len(cache.excluded_rows(np.arange(100, 125))) == 65
    assert on.counts.get("fused_step") == 2 * 8 and "fused_advance" not in on.counts


def test_told_values_at_the_ends_and_duplicated(monkeypatch) -> None:
    space = {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(3)}
    initial = _trials(np.random.RandomState(4), space, 600)
    crafted = {
        1: lambda study: {name: -5.0 for name in space},  # the smallest in every dim
        3: lambda study: {name: 5.0 for name in space},  # the largest
        5: lambda study: dict(study.trials[17].params),  # an exact duplicate of row 17
        6: lambda study: {name: -5.0 for name in space},  # a tie at the low end
    }
    on, _ = _run_twins(monkeypatch, space, initial, 9, crafted=crafted)
    assert on.counts.get("fused_step") == 8
    index = on.caches()[tuple(space)]._device_mirror._hist.sorted_index()
    # Ties go behind equal values: row 601 (-5) first, its later tie 606 next.
    assert index[:, 0].tolist() == [601] * 3 and index[:, 1].tolist() == [606] * 3
    assert index[:, -1].tolist() == [603] * 3
    pos17 = [int(np.nonzero(col == 17)[0][0]) for col in index]
    assert [int(col[p + 1]) for col, p in zip(index, pos17)] == [605] * 3
