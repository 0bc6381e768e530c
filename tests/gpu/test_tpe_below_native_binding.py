"""The extension's ``tpe_below_kernels`` (the hipcc host build of
``_hip/csrc/tpe_below_host.h``) against the Python estimator, bit for bit, on
the cases of ``optuna_amd.testing.tpe_below_cases``; its argument checks; and
the sampler on a mixed space with the native below route on, off, and with the
fused suggest off altogether: all three must suggest the same parameters, bit
for bit, on every one of 16 steps (the seed's top-two acquisition gap on the
host path is checked on the CPU by tests/test_tpe_below_native.py).
"""
from __future__ import annotations

import numpy as np
import pytest

from optuna_amd import _hip
from optuna_amd.samplers._tpe import _device
from optuna_amd.testing import tpe_below_cases as tc


pytestmark = pytest.mark.gpu

SAMPLER_SEED = 0


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    if c is None or not c.available():
        pytest.fail("HIP extension must be available on a GPU box (no silent fallback)")
    return c


def test_binding_matches_parzen_estimator(core) -> None:
    for case in tc.cases():
        got = core.tpe_below_kernels(
            np.ascontiguousarray(case.obs), case.alow, case.ahigh,
            case.consider_endpoints, case.consider_magic_clip, case.active,
        )
        tc.assert_bits_equal(dict(zip(tc.OUTPUTS, got)), tc.expected(case), case.name)


def test_binding_rejects_bad_inputs(core) -> None:
    case = next(c for c in tc.cases() if c.name == "n25-D3-ce0-mc1")
    obs, active = np.ascontiguousarray(case.obs), case.active

    def call(obs=obs, alow=case.alow, ahigh=case.ahigh, active=active):
        return core.tpe_below_kernels(obs, alow, ahigh, False, True, active)

    call()
    with pytest.raises(RuntimeError):
        call(obs=np.asfortranarray(obs))  # not C-contiguous
    with pytest.raises(RuntimeError):
        call(obs=obs.astype(np.float32))
    with pytest.raises(RuntimeError):
        call(obs=obs[:, 0].copy())  # not 2-D
    with pytest.raises(RuntimeError):
        call(alow=case.alow[:2].copy())
    with pytest.raises(RuntimeError):
        call(ahigh=np.zeros((3, 1)))
    with pytest.raises(RuntimeError):
        call(active=active.astype(np.int32))
    with pytest.raises(RuntimeError):
        call(active=np.array([26], dtype=np.int64))  # n is 25: kernels 0..25
    with pytest.raises(RuntimeError):
        call(active=np.array([-1], dtype=np.int64))
    with pytest.raises(RuntimeError):  # more kernels than the fused entry scores
        core.tpe_below_kernels(
            np.zeros((_device.FUSED_MAX_BELOW, 1)), np.zeros(1), np.ones(1), False, True,
            np.zeros(1, dtype=np.int64),
        )


def _run(monkeypatch, env: dict[str, str]) -> tuple[np.ndarray, int, int]:
    """(params of 16 steps, fused scoring calls, native below calls)."""
    seen = {"fused": 0, "native": 0}
    orig_score = _device.score_above_resident
    orig_native = _device.native_below

    def score_spy(*args, **kwargs):
        if kwargs.get("fused") is not None:
            seen["fused"] += 1
        return orig_score(*args, **kwargs)

    def native_spy(cache):
        fn = orig_native(cache)
        if fn is None:
            return None

        def counted(*args):
            seen["native"] += 1
            return fn(*args)

        return counted

    with monkeypatch.context() as m:
        for key, value in env.items():
            m.setenv(key, value)
        m.setattr(_device, "score_above_resident", score_spy)
        m.setattr(_device, "native_below", native_spy)
        study = tc.seeded_study(SAMPLER_SEED, tc.MIXED4)
        out = []
        for _ in range(16):
            t = tc.suggest_all(study, tc.MIXED4)
            study.tell(t, tc.mixed4_value(t.params))
            out.append([float(t.params[name]) for name in tc.MIXED4])
    return np.array(out), seen["fused"], seen["native"]


def test_sampler_three_routes_agree(core, monkeypatch) -> None:
    on = {"OPTUNA_AMD_TPE_FUSED": "1", "OPTUNA_AMD_TPE_NATIVE_BELOW": "1"}
    p_on, fused_on, native_on = _run(monkeypatch, on)
    assert (fused_on, native_on) == (16, 16)
    p_off, fused_off, native_off = _run(monkeypatch, {**on, "OPTUNA_AMD_TPE_NATIVE_BELOW": "0"})
    assert (fused_off, native_off) == (16, 0)
    p_unfused, fused_un, native_un = _run(monkeypatch, {**on, "OPTUNA_AMD_TPE_FUSED": "0"})
    assert (fused_un, native_un) == (0, 0)
    for other in (p_off, p_unfused):
        assert other.shape == p_on.shape == (16, 4)
        np.testing.assert_array_equal(p_on.view(np.uint64), other.view(np.uint64))
