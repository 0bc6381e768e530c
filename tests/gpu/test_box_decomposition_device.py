"""The device box decomposition (``core.box_decompose``, K6e) against the host
``_get_boxes`` run per draw. Nothing is computed but one subtraction that both sides
do identically, so per draw the lex-sorted rows of (lower | intervals) must be equal
bit for bit."""
import warnings
from functools import partial

import numpy as np
import pytest
import torch

import optuna_amd
from optuna_amd import _hip
from optuna_amd._gp import acqf as acqf_mod, gp as gp_mod, prior, search_space as gp_ss
from optuna_amd._hypervolume import box_decomposition as bd
from optuna_amd.distributions import FloatDistribution
from optuna_amd.testing.hv_reference import lattice_points, sphere_front, tied_front4


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core():
    c = _hip.require()
    assert c is not None and c.available(), "the HIP extension must run here: no fallback"
    return c


def _canon(lo, iv):
    rows = np.concatenate([lo, iv], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def _host(base, extra, ref):
    out = []
    for rows in extra:
        lo, up = acqf_mod._get_boxes(torch.from_numpy(-np.concatenate([base, rows])), ref)
        out.append(_canon(lo.numpy(), (up - lo).clamp_min_(1e-12).numpy()))
    return out


def _assert_equal(got, want):
    lo, iv, offsets = got
    assert len(offsets) == len(want) + 1 and offsets[0] == 0 and offsets[-1] == len(lo)
    for q, rows in enumerate(want):
        part = slice(offsets[q], offsets[q + 1])
        assert offsets[q + 1] - offsets[q] == len(rows), q
        assert np.array_equal(_canon(lo[part], iv[part]), rows), q


def _inputs(case, M):
    rng = np.random.RandomState(11 * M + len(case))
    ref, extra = np.full(M, 1.1), np.empty((1, 0, M))
    if case == "none_below":
        base = np.full((3, M), 2.0)
    elif case == "one":
        base = np.full((1, M), 0.5)
    elif case == "n65":
        base = sphere_front(65, M, 1)
    elif case == "fantasies":  # R = 8 rows around the front for each of Q = 3 draws
        base = sphere_front({2: 300, 3: 300, 4: 100}[M], M, 2)
        extra = sphere_front(24, M, 3).reshape(3, 8, M) * rng.uniform(0.8, 1.2, (3, 8, 1))
    elif case == "lattice":
        base = tied_front4(1) if M == 4 else lattice_points(60, M, 4)
        extra = np.round(rng.uniform(0.1, 0.9, (2, 3, M)), 1)
    elif case == "special":
        # a copy of a base row, a row beyond ref, a dominated row, and in draw 1 a row
        # that dominates the whole base
        base = sphere_front(40, M, 5)
        beyond = np.where(np.arange(M) == 0, 1.5, 0.01)
        extra = np.stack([
            np.stack([base[7], beyond, base[3] * 1.05, base[9]]),
            np.stack([base[7], beyond, base[3] * 1.05, np.full(M, 1e-3)]),
        ])
    else:  # "n150": the second pass holds 931 active entries, hits span wavefronts
        base = sphere_front(150, M, 6)
    return base, extra, ref


CASES = [(case, M) for case in ("none_below", "one", "n65", "fantasies", "lattice", "special")
         for M in (2, 3, 4)] + [("n150", 4)]


@pytest.mark.parametrize("case, M", CASES)
def test_box_decompose_equals_host(core, case, M) -> None:
    base, extra, ref = _inputs(case, M)
    lo, iv, offsets, host_needed = core.box_decompose(base, extra, ref)
    assert len(host_needed) == 0
    _assert_equal((lo, iv, offsets), _host(base, extra, ref))
    again = core.box_decompose(base, extra, ref)
    assert np.array_equal(again[0], lo) and np.array_equal(again[1], iv)  # same order too


def test_small_output_capacity_relaunches(core) -> None:
    base, extra, ref = _inputs("n65", 3)
    lo, iv, offsets, host_needed = core.box_decompose(base, extra, ref, out_cap=20)
    assert len(host_needed) == 0
    _assert_equal((lo, iv, offsets), _host(base, extra, ref))


def test_small_active_capacity_goes_to_the_host(core, monkeypatch) -> None:
    base, extra, ref = _inputs("n65", 3)
    lo, _, offsets, host_needed = core.box_decompose(base, extra, ref, active_cap=4)
    assert list(host_needed) == [0] and len(lo) == 0 and list(offsets) == [0, 0]
    monkeypatch.setattr(core, "box_decompose", partial(core.box_decompose, active_cap=4))
    monkeypatch.setattr(bd, "_DEVICE_BOXES_MIN_ROWS", {3: 0})
    _assert_equal(bd.get_non_dominated_boxes_batched(base, extra, ref), _host(base, extra, ref))


def _spy(core, monkeypatch):
    calls, orig = [], core.box_decompose

    def spy(*args, **kwargs):
        calls.append(args)
        return orig(*args, **kwargs)

    monkeypatch.setattr(core, "box_decompose", spy)
    monkeypatch.setattr(bd, "_DEVICE_BOXES_MIN_ROWS", {2: 0, 3: 0, 4: 0})
    return calls


def test_qlogehvi_boxes_route_on_and_off(core, monkeypatch) -> None:
    n, d, rng = 40, 3, np.random.RandomState(3)
    X = rng.rand(n, d)
    Y = np.stack([-np.sum(np.square(X - c), axis=1) + 0.1 * rng.randn(n) for c in (0.2, 0.5, 0.8)], -1)
    Y = (Y - Y.mean(0)) / Y.std(0)
    gprs = [
        gp_mod.fit_kernel_params(X, y, np.zeros(d, bool), prior.default_log_prior, 1e-6, False)
        for y in Y.T
    ]
    space = gp_ss.SearchSpace({f"x{i}": FloatDistribution(0.0, 1.0) for i in range(d)})
    make = partial(acqf_mod.qLogEHVI, gprs, space, torch.from_numpy(Y), 0.4 + 0.2 * rng.rand(2, d),
                   n_qmc_samples=8, qmc_seed=5)
    calls = _spy(core, monkeypatch)
    on = make()
    assert len(calls) == 1
    monkeypatch.setenv("OPTUNA_AMD_GP_BOXES_DEVICE", "0")
    off = make()
    assert len(calls) == 1 and on._box_counts == off._box_counts and len(on._box_counts) == 8
    lo, iv, offsets = off._box_packed
    want = [_canon(lo[a:b], iv[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
    _assert_equal(on._box_packed, want)
    x = torch.from_numpy(rng.rand(6, d)).to(on._box_lower.device)
    np.testing.assert_allclose(
        on.eval_acqf(x).cpu().numpy(), off.eval_acqf(x).cpu().numpy(), rtol=1e-10, atol=0
    )


def test_gp_sampler_with_a_running_trial_decomposes_on_the_device(core, monkeypatch) -> None:
    calls = _spy(core, monkeypatch)
    warnings.simplefilter("ignore")
    optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
    rng = np.random.RandomState(4)
    names = [f"x{i}" for i in range(3)]
    dists = {name: FloatDistribution(0.0, 1.0) for name in names}
    study = optuna_amd.create_study(
        directions=["minimize"] * 3,
        sampler=optuna_amd.samplers.GPSampler(seed=0, n_startup_trials=5),
    )

    def values(x):
        return [float(np.sum(np.square(np.asarray(x) - c))) for c in (0.2, 0.5, 0.8)]

    study.add_trials([
        optuna_amd.create_trial(params=dict(zip(names, map(float, row))), distributions=dists,
                                values=values(row))
        for row in rng.rand(40, 3)
    ])
    peer = study.ask()  # stays RUNNING: the next suggest fantasizes over it
    for name in names:
        peer.suggest_float(name, 0.0, 1.0)
    study.optimize(lambda t: values([t.suggest_float(name, 0.0, 1.0) for name in names]), n_trials=1)
    assert len(calls) >= 1 and calls[-1][1].shape[1:] == (1, 3)  # (Q, R = 1, M = 3)
