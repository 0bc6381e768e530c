"""Native fit of the TPE below estimator (``_hip/csrc/tpe_below_host.h``).

The header is plain C++17, so a stand-alone program (``tests/cpp/
tpe_below_check.cpp``) is compiled against it with the host compiler and run
on the cases of ``optuna_amd.testing.tpe_below_cases``; its six outputs must
equal, bit for bit, what ``_ParzenEstimator`` and the numpy expressions of
``_sample_array`` give.

The routing tests replace the device calls by a recorder and the extension by
a stub whose ``tpe_below_kernels`` is a numpy transcription, and check when the
sampler takes the native route and that it draws, returns and leaves behind
the same as the Python estimator.
"""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from optuna_amd import _hip
from optuna_amd.distributions import CategoricalDistribution, FloatDistribution
from optuna_amd.samplers import TPESampler
from optuna_amd.samplers._tpe import _device
from optuna_amd.samplers._tpe._history import _TpeHistory
from optuna_amd.samplers._tpe.parzen import _ParzenEstimator, _ParzenEstimatorParameters
from optuna_amd.samplers._tpe.sampler import default_weights
from optuna_amd.testing import tpe_below_cases as tc


_ROOT = Path(__file__).resolve().parent.parent
_CSRC = _ROOT / "optuna_amd" / "_hip" / "csrc"
_PROGRAM = Path(__file__).resolve().parent / "cpp" / "tpe_below_check.cpp"


# ---------------------------------------------------------------------------
# The header against the Python estimator
# ---------------------------------------------------------------------------


def _write_cases(path: Path, cases) -> None:
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.int64).tobytes())
        for c in cases:
            n, D = c.obs.shape
            head = [n, D, len(c.active), int(c.consider_endpoints), int(c.consider_magic_clip)]
            f.write(np.array(head, dtype=np.int64).tobytes())
            for arr in (c.obs, c.alow, c.ahigh):
                f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(c.active, dtype=np.int64).tobytes())


def _read_results(path: Path, cases) -> list[dict[str, np.ndarray]]:
    flat = np.fromfile(path, dtype=np.float64)
    out, at = [], 0
    for c in cases:
        n, D = c.obs.shape
        S = len(c.active)
        got = {}
        for key, rows in zip(tc.OUTPUTS, (n + 1, n + 1, S, S, S, S)):
            got[key] = flat[at : at + rows * D].reshape(rows, D)
            at += rows * D
        out.append(got)
    assert at == len(flat)
    return out


def test_header_matches_parzen_estimator(tmp_path) -> None:
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "tpe_below_check"
    subprocess.run(
        [cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", f"-I{_CSRC}",
         str(_PROGRAM), "-o", str(exe)],
        check=True,
    )
    cases = tc.cases()
    assert len(cases) == len(tc.N_OBS) * len(tc.N_DIMS) * 4
    _write_cases(tmp_path / "cases.bin", cases)
    run = subprocess.run(
        [str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")],
        capture_output=True, text=True,
    )
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{len(cases)} cases written" in run.stdout
    for case, got in zip(cases, _read_results(tmp_path / "results.bin", cases)):
        tc.assert_bits_equal(got, tc.expected(case), case.name)


def test_cases_cover_the_edge_columns() -> None:
    """Ties, an all-equal column and values on both adapted bounds occur."""
    seen = {"ties": False, "equal": False, "on_low": False, "on_high": False, "log": False}
    for c in tc.cases():
        n, D = c.obs.shape
        assert c.active[0] == 0 and c.active[1] == n and c.active[2] == c.active[3]
        for d, dist in enumerate(c.space.values()):
            col = c.obs[:, d]
            if n >= 25:
                seen["ties"] |= 1 < len(np.unique(col)) < n
                seen["equal"] |= len(np.unique(col)) == 1
            seen["on_low"] |= bool((col == c.alow[d]).any())
            seen["on_high"] |= bool((col == c.ahigh[d]).any())
            seen["log"] |= bool(getattr(dist, "log", False)) and n > 0
    assert all(seen.values()), seen


# ---------------------------------------------------------------------------
# Sampler routing (device calls replaced by a recorder, the binding by a stub)
# ---------------------------------------------------------------------------

_CONT4 = {f"x{i}": FloatDistribution(-5.0, 5.0) for i in range(4)}
_MIXED4 = tc.MIXED4  # the space of the sampler-level GPU test
_study = tc.seeded_study
_suggest = tc.suggest_all


def _numpy_below_kernels(obs, alow, ahigh, consider_endpoints, consider_magic_clip, active):
    """``tpe_below_kernels`` through the estimator's per-dim numpy fit."""
    parameters = _ParzenEstimatorParameters(
        prior_weight=1.0, consider_magic_clip=consider_magic_clip,
        consider_endpoints=consider_endpoints, weights=default_weights, multivariate=True,
    )
    cols = [
        _ParzenEstimator._numerical_kernels(None, obs[:, d], alow[d], ahigh[d], parameters)
        for d in range(obs.shape[1])
    ]
    mus = np.column_stack([m for m, _ in cols])
    sigmas = np.column_stack([s for _, s in cols])
    loc, scale = mus[active, :], sigmas[active, :]
    return mus, sigmas, (alow[None, :] - loc) / scale, (ahigh[None, :] - loc) / scale, loc, scale


class _StubCore:
    def __init__(self, calls: list) -> None:
        self._calls = calls

    def available(self) -> bool:
        return False

    def tpe_below_kernels(self, obs, alow, ahigh, ce, mc, active):
        assert obs.flags.c_contiguous and obs.dtype == np.float64 and active.dtype == np.int64
        self._calls.append(dict(obs=obs.copy(), active=active.copy(), ce=ce, mc=mc))
        return _numpy_below_kernels(obs, alow, ahigh, ce, mc, active)


@pytest.fixture
def route(monkeypatch):
    """Pretend a device and an extension are there; record what the sampler
    asks of them and which host steps of the Python estimator it runs."""
    rec = {"native": [], "score": [], "build_mpe": 0, "observations": 0}

    def fake_score(cache, sel, weights, samples, ce, mc, prior_weight=1.0, extras=None,
                   per_dim=False, fused=None):
        rec["score"].append(dict(fused=fused, samples=samples, per_dim=per_dim))
        S = len(fused.x_raw) if fused is not None else len(next(iter(samples.values())))
        vals = -np.abs(np.arange(S) - 7.0)  # candidate 7 wins
        return np.repeat(vals[:, None], len(cache.names), axis=1) if per_dim else vals

    monkeypatch.setattr(_hip, "get", lambda: _StubCore(rec["native"]))
    monkeypatch.setattr(_device, "device_ready", lambda n_kernels: n_kernels >= 512)
    monkeypatch.setattr(_device, "score_above_resident", fake_score)
    monkeypatch.setattr(_device, "prepare_fused_resident", lambda *a, **k: None)
    monkeypatch.delenv("OPTUNA_AMD_TPE_FUSED", raising=False)
    monkeypatch.delenv("OPTUNA_AMD_TPE_NATIVE_BELOW", raising=False)

    def count(cls, name, key):
        orig = getattr(cls, name)

        def wrapped(self, *args, **kwargs):
            rec[key] += 1
            return orig(self, *args, **kwargs)

        monkeypatch.setattr(cls, name, wrapped)

    count(TPESampler, "_build_mpe", "build_mpe")
    count(_TpeHistory, "observations", "observations")
    return rec


def test_native_route_taken_when_eligible(route) -> None:
    study = _study(1, _CONT4)
    _suggest(study, _CONT4)
    assert len(route["native"]) == 1 and len(route["score"]) == 1
    assert route["build_mpe"] == 0 and route["observations"] == 0
    call, req = route["native"][0], route["score"][0]["fused"]
    assert call["obs"].shape == (25, 4) and call["active"].shape == (24,)
    assert call["ce"] is False and call["mc"] is True
    assert req.x_raw.shape == (24, 4)
    assert req.below_mus.shape == req.below_sigmas.shape == (26, 4)
    assert req.below_weights.shape == (26,) and req.n_above == 575


def test_env_switch_keeps_the_python_estimator(monkeypatch, route) -> None:
    monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_BELOW", "0")
    study = _study(1, _CONT4)
    _suggest(study, _CONT4)
    assert route["native"] == [] and route["build_mpe"] == 1 and route["observations"] == 1
    assert route["score"][0]["fused"] is not None  # still the fused suggest
    monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_BELOW", "1")
    _suggest(study, _CONT4)
    assert len(route["native"]) == 1 and route["build_mpe"] == 1


def test_unfused_path_keeps_the_python_estimator(monkeypatch, route) -> None:
    monkeypatch.setenv("OPTUNA_AMD_TPE_FUSED", "0")
    study = _study(1, _CONT4)
    _suggest(study, _CONT4)
    assert route["native"] == [] and route["build_mpe"] == 1
    assert route["score"][0]["fused"] is None


def test_no_binding_keeps_the_python_estimator(monkeypatch, route) -> None:
    monkeypatch.setattr(_hip, "get", lambda: None)
    study = _study(1, _CONT4)
    _suggest(study, _CONT4)
    assert route["native"] == [] and route["build_mpe"] == 1
    assert route["score"][0]["fused"] is not None


def test_custom_weights_keep_the_python_estimator(route) -> None:
    study = _study(1, _CONT4, weights=lambda n: np.linspace(0.5, 1.5, n))
    _suggest(study, _CONT4)
    assert route["native"] == [] and route["build_mpe"] == 1
    assert route["score"][0]["fused"] is not None


def test_custom_estimator_class_keeps_the_python_estimator(route) -> None:
    class Mine(_ParzenEstimator):
        pass

    study = _study(1, _CONT4)
    study.sampler._parzen_estimator_cls = Mine
    _suggest(study, _CONT4)
    assert route["native"] == [] and route["score"] == [] and route["build_mpe"] == 2


def test_per_dim_mode_keeps_the_python_estimator(route) -> None:
    # Two objectives: independent sampling, served by one per-dim batch.
    study = _study(1, _CONT4, n_objectives=2)
    _suggest(study, _CONT4)
    assert route["native"] == [] and route["build_mpe"] == 1
    assert [s["per_dim"] for s in route["score"]] == [True]


def test_categorical_space_keeps_the_python_estimator(route) -> None:
    space = {"x": FloatDistribution(-5.0, 5.0), "k": CategoricalDistribution(["a", "b", "c"])}
    study = _study(2, space)
    _suggest(study, space)
    assert route["native"] == [] and route["build_mpe"] == 1
    assert route["score"][0]["fused"] is None


@pytest.mark.parametrize(
    "space,kwargs",
    [
        (_CONT4, {}),
        (_MIXED4, {}),
        (_MIXED4, dict(consider_endpoints=True, consider_magic_clip=False, prior_weight=0.3)),
        (_CONT4, dict(n_objectives=2, multivariate=True)),
    ],
    ids=["cont4", "mixed4", "mixed4-flags", "two-objectives"],
)
def test_route_on_and_off_agree(monkeypatch, route, space, kwargs) -> None:
    """Same candidates, kernels, weights, returned parameters and RNG state,
    over three suggests (the history grows in between)."""
    runs = []
    for env in ("1", "0"):
        monkeypatch.setenv("OPTUNA_AMD_TPE_NATIVE_BELOW", env)
        del route["score"][:], route["native"][:]
        study = _study(3, space, **kwargs)
        params = []
        for step in range(3):
            t = _suggest(study, space)
            params.append(list(t.params.values()))
            study.tell(t, [float(step)] * len(study.directions))
        assert len(route["native"]) == (3 if env == "1" else 0)
        reqs = [s["fused"] for s in route["score"]]
        assert len(reqs) == 3 and all(r is not None for r in reqs)
        runs.append((params, reqs, study.sampler._rng.rng.get_state()))
    (p_on, r_on, s_on), (p_off, r_off, s_off) = runs
    assert p_on == p_off
    for a, b in zip(r_on, r_off):
        np.testing.assert_array_equal(a.below_rows, b.below_rows)
        assert a.n_above == b.n_above
        for key in ("x_raw", "below_mus", "below_sigmas", "below_weights"):
            ga = np.ascontiguousarray(getattr(a, key))
            gb = np.ascontiguousarray(getattr(b, key))
            assert ga.shape == gb.shape, key
            np.testing.assert_array_equal(ga.view(np.uint64), gb.view(np.uint64), err_msg=key)
    assert s_on[0] == s_off[0] and s_on[2:] == s_off[2:]
    np.testing.assert_array_equal(s_on[1], s_off[1])


def test_below_weights_are_memoised_and_read_only(route) -> None:
    study = _study(1, _CONT4)
    for step in range(2):
        t = _suggest(study, _CONT4)
        study.tell(t, float(step))
    w0, w1 = (s["fused"].below_weights for s in route["score"])
    assert w0 is w1 and not w0.flags.writeable
    expect = np.append(default_weights(25), [1.0])
    np.testing.assert_array_equal(w0, expect / expect.sum())


# ---------------------------------------------------------------------------
# Seed of the sampler-level GPU test
# ---------------------------------------------------------------------------


def test_gpu_mixed_space_seed_has_no_near_ties(monkeypatch) -> None:
    """tests/gpu/test_tpe_below_native_binding.py compares three routes bit for bit
    over 16 steps and allows no skipped step, so on the host path the top-two
    acquisition gap of its seed must stay clear of rounding differences."""
    seed = 0  # SAMPLER_SEED of the GPU test
    monkeypatch.setattr(_device, "device_ready", lambda n_kernels: False)  # host path
    study = _study(seed, _MIXED4)
    gaps: list[float] = []
    orig = TPESampler._compare

    def spy(samples, vals):
        top = np.sort(np.asarray(vals))[-2:]
        gaps.append(float(top[1] - top[0]))
        return orig(samples, vals)

    monkeypatch.setattr(TPESampler, "_compare", staticmethod(spy))
    for _ in range(16):
        t = _suggest(study, _MIXED4)
        study.tell(t, tc.mixed4_value(t.params))
    assert len(gaps) == 16
    print("top-two gaps:", gaps)
    assert min(gaps) >= 1e-6
