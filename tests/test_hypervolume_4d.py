"""Four-objective hypervolume / HSSP: the host references are pinned against each
other and against the WFG, and the device dispatch is checked with a recording
fake in place of the HIP extension (no GPU needed)."""
from __future__ import annotations

import numpy as np
import pytest

from optuna_amd import _hip
from optuna_amd._hypervolume import hssp, wfg
from optuna_amd.testing.hv_reference import (
    hssp_views4,
    hv4d_nested_sweep,
    hv_grid,
    lattice_points,
    sphere_front,
    tied_front4,
)


_REF = np.array([1.2, 1.3, 1.4, 1.25])


# ---------------------------------------------------------------------------
# Reference pinning
# ---------------------------------------------------------------------------


def _pin_cases() -> dict[str, np.ndarray]:
    cases = {f"sphere-{n}": sphere_front(n, 4, 40 + n) for n in (1, 2, 17)}
    cases["lattice-30"] = lattice_points(30, 4, 7)
    for axis in range(4):
        cases[f"tied-{'wxyz'[axis]}"] = tied_front4(axis)
    return cases


_PIN = _pin_cases()


@pytest.mark.parametrize("name", list(_PIN))
def test_references_agree_with_wfg(name: str) -> None:
    pts = _PIN[name]
    grid = hv_grid(pts, _REF)
    sweep = hv4d_nested_sweep(pts, _REF)
    host = wfg.compute_hypervolume(pts, _REF)
    print(f"{name}: grid {grid!r} sweep {sweep!r} wfg {host!r}")
    np.testing.assert_allclose(sweep, grid, rtol=1e-12)
    np.testing.assert_allclose(host, grid, rtol=1e-12)


def test_pin_inputs_have_the_advertised_edges() -> None:
    lat = _PIN["lattice-30"]
    assert len(np.unique(lat, axis=0)) < len(lat)  # duplicate rows
    for d in range(4):
        assert len(np.unique(lat[:, d])) < len(lat)  # ties in every axis
    from optuna_amd.study._multi_objective import _is_pareto_front

    uniq = np.unique(lat, axis=0)
    assert not _is_pareto_front(uniq, assume_unique_lexsorted=True).all()  # dominated rows
    for axis in range(4):
        assert len(np.unique(tied_front4(axis)[:, axis])) == 2


def test_hv_grid_matches_lower_dimensions() -> None:
    r = np.random.RandomState(3)
    for m in (1, 2, 3, 5):
        pts = np.round(r.uniform(0.1, 0.9, (9, m)), 1)
        ref = np.full(m, 1.1)
        np.testing.assert_allclose(
            hv_grid(pts, ref), wfg.compute_hypervolume(pts, ref), rtol=1e-12
        )
    assert hv_grid(np.empty((0, 4)), _REF) == 0.0
    assert hv4d_nested_sweep(np.empty((0, 4)), _REF) == 0.0


def test_hssp_views4_are_sorted_and_consistent() -> None:
    sel = lattice_points(12, 4, 9)
    sw, sx, sy, syz, syrw, syrx = hssp_views4(sel)
    assert (np.diff(sw) >= 0).all() and (np.diff(sx) >= 0).all() and (np.diff(sy) >= 0).all()
    assert syrw.dtype == np.int32 and syrx.dtype == np.int32
    # every stream entry names the same point in all three views
    oy = np.argsort(sel[:, 2], kind="stable")
    np.testing.assert_array_equal(sw[syrw], sel[oy, 0])
    np.testing.assert_array_equal(sx[syrx], sel[oy, 1])
    np.testing.assert_array_equal(syz, sel[oy, 3])
    assert sorted(syrw) == list(range(12)) and sorted(syrx) == list(range(12))
    assert all(len(v) == 0 for v in hssp_views4(np.empty((0, 4))))


# ---------------------------------------------------------------------------
# Dispatch (recording fake core)
# ---------------------------------------------------------------------------


class _FakeCore:
    def __init__(self, available: bool = True) -> None:
        self.calls: list[tuple] = []
        self._available = available
        fake = self

        class _Session:
            def __init__(self, name: str, cand: np.ndarray, *ref: float) -> None:
                self.name = name
                fake.calls.append((name, np.array(cand), ref))

            def run(self, subset_size: int) -> np.ndarray:
                fake.calls.append((self.name + ".run", subset_size))
                return np.arange(subset_size, dtype=np.int64)

        self.Hssp3dSession = lambda cand, *ref: _Session("Hssp3dSession", cand, *ref)
        self.Hssp4dSession = lambda cand, *ref: _Session("Hssp4dSession", cand, *ref)

    def available(self) -> bool:
        return self._available

    def hv3d(self, pts: np.ndarray, *ref: float) -> float:
        self.calls.append(("hv3d", len(pts)))
        return wfg._compute_3d(np.asarray(pts), np.array(ref))

    def hv4d(self, pts: np.ndarray, *ref: float) -> float:
        self.calls.append(("hv4d", len(pts)))
        return hv_grid(np.asarray(pts), np.array(ref))

    def names(self) -> list[str]:
        return [c[0] for c in self.calls]


@pytest.fixture
def fake(monkeypatch) -> _FakeCore:
    core = _FakeCore()
    monkeypatch.setattr(_hip, "get", lambda: core)
    return core


def test_hv4d_dispatch_gate(fake, monkeypatch) -> None:
    monkeypatch.setattr(wfg, "_DEVICE_HV4D_MIN_ROWS", 9)
    ref = np.full(4, 1.2)
    at = sphere_front(9, 4, 1)
    got = wfg.compute_hypervolume(at, ref)
    assert fake.calls == [("hv4d", 9)]
    np.testing.assert_allclose(got, hv_grid(at, ref), rtol=1e-12)

    fake.calls.clear()
    below = sphere_front(8, 4, 2)
    got = wfg.compute_hypervolume(below, ref)
    assert fake.calls == []
    np.testing.assert_allclose(got, hv_grid(below, ref), rtol=1e-12)

    # the gate counts Pareto rows, not input rows
    padded = np.vstack([below, below[:4] + 0.01])
    wfg.compute_hypervolume(padded, ref)
    assert fake.calls == []


def test_hv_other_dimensions_keep_their_paths(fake, monkeypatch) -> None:
    monkeypatch.setattr(wfg, "_DEVICE_HV4D_MIN_ROWS", 2)
    monkeypatch.setattr(wfg, "_DEVICE_HV3D_MIN_ROWS", 2)
    wfg.compute_hypervolume(sphere_front(6, 3, 3), np.full(3, 1.2))
    assert fake.calls == [("hv3d", 6)]
    fake.calls.clear()
    for m in (2, 5):
        wfg.compute_hypervolume(sphere_front(6, m, 3), np.full(m, 1.2))
    assert fake.calls == []


def test_hv4d_without_device_keeps_host(monkeypatch) -> None:
    monkeypatch.setattr(wfg, "_DEVICE_HV4D_MIN_ROWS", 2)
    pts = sphere_front(7, 4, 4)
    ref = np.full(4, 1.2)
    want = wfg._compute_hv(pts, ref)
    off = _FakeCore(available=False)
    monkeypatch.setattr(_hip, "get", lambda: off)
    assert wfg.compute_hypervolume(pts, ref) == want
    assert off.calls == []
    monkeypatch.setattr(_hip, "get", lambda: None)
    assert wfg.compute_hypervolume(pts, ref) == want


def _host_hssp(vals: np.ndarray, k: int, ref: np.ndarray, monkeypatch) -> np.ndarray:
    with monkeypatch.context() as mp:
        mp.setattr(_hip, "get", lambda: None)
        return hssp._solve_hssp(vals, np.arange(len(vals)), k, ref)


def test_hssp4d_dispatch_gate(fake, monkeypatch) -> None:
    monkeypatch.setattr(wfg, "_DEVICE_HV4D_MIN_ROWS", 10**9)
    monkeypatch.setattr(hssp, "_DEVICE_HSSP4D_MIN_WORK", 40)
    ref = np.full(4, 1.2)
    vals = sphere_front(10, 4, 5)
    idx = np.arange(100, 110)
    got = hssp._solve_hssp(vals, idx, 4, ref)
    assert fake.names() == ["Hssp4dSession", "Hssp4dSession.run"]
    np.testing.assert_array_equal(fake.calls[0][1], vals)  # unique-lexsorted rows
    assert fake.calls[0][2] == (1.2, 1.2, 1.2, 1.2)
    assert fake.calls[1] == ("Hssp4dSession.run", 4)
    np.testing.assert_array_equal(got, idx[:4])  # the fake picks rows 0..3

    fake.calls.clear()
    below = sphere_front(9, 4, 6)  # 9 * 4 = 36 < 40
    got = hssp._solve_hssp(below, np.arange(9), 4, ref)
    assert fake.calls == []
    np.testing.assert_array_equal(got, _host_hssp(below, 4, ref, monkeypatch))


def test_hssp_other_dimensions_keep_their_paths(fake, monkeypatch) -> None:
    monkeypatch.setattr(wfg, "_DEVICE_HV4D_MIN_ROWS", 10**9)
    monkeypatch.setattr(hssp, "_DEVICE_HSSP4D_MIN_WORK", 0)
    monkeypatch.setattr(hssp, "_DEVICE_HSSP_MIN_WORK", 0)
    hssp._solve_hssp(sphere_front(8, 3, 7), np.arange(8), 3, np.full(3, 1.2))
    assert fake.names() == ["Hssp3dSession", "Hssp3dSession.run"]
    fake.calls.clear()
    for m in (2, 5):
        hssp._solve_hssp(sphere_front(8, m, 7), np.arange(8), 3, np.full(m, 1.2))
    assert fake.calls == []


def test_hssp4d_host_path_is_kept(fake, monkeypatch) -> None:
    monkeypatch.setattr(wfg, "_DEVICE_HV4D_MIN_ROWS", 10**9)
    monkeypatch.setattr(hssp, "_DEVICE_HSSP4D_MIN_WORK", 0)
    ref = np.full(4, 1.2)
    vals = sphere_front(8, 4, 8)

    # a non-finite loss value
    bad = vals.copy()
    bad[3, 1] = -np.inf
    got = hssp._solve_hssp(bad, np.arange(8), 3, ref)
    assert fake.calls == []
    assert len(np.unique(got)) == 3

    # a subset above the session bound
    monkeypatch.setattr(hssp, "_DEVICE_HSSP4D_MAX_SUBSET", 3)
    got = hssp._solve_hssp(vals, np.arange(8), 4, ref)
    assert fake.calls == []
    np.testing.assert_array_equal(got, _host_hssp(vals, 4, ref, monkeypatch))
    hssp._solve_hssp(vals, np.arange(8), 3, ref)  # at the bound: device
    assert fake.names() == ["Hssp4dSession", "Hssp4dSession.run"]

    # a core without a device
    off = _FakeCore(available=False)
    monkeypatch.setattr(_hip, "get", lambda: off)
    got = hssp._solve_hssp(vals, np.arange(8), 3, ref)
    assert off.calls == []
    np.testing.assert_array_equal(got, _host_hssp(vals, 3, ref, monkeypatch))


def test_session_bound_matches_the_kernel_constants() -> None:
    # 8 register slots x 256 lanes in k_hssp4d_insert
    assert hssp._DEVICE_HSSP4D_MAX_SUBSET == 8 * 256


def test_hssp_dedup_and_padding_with_fake(fake, monkeypatch) -> None:
    monkeypatch.setattr(wfg, "_DEVICE_HV4D_MIN_ROWS", 10**9)
    monkeypatch.setattr(hssp, "_DEVICE_HSSP4D_MIN_WORK", 0)
    ref = np.full(4, 1.2)
    base = sphere_front(6, 4, 9)
    vals = np.vstack([base, base[:4]])  # 10 rows, 6 unique
    idx = np.arange(50, 60)

    # more slots than unique rows: padded with duplicates, no device call
    got = hssp._solve_hssp(vals, idx, 8, ref)
    assert fake.calls == []
    np.testing.assert_array_equal(got, _host_hssp(vals, 8, ref, monkeypatch) + 50)
    assert len(got) == 8 and set(idx[:6]) <= set(got)

    # enough unique rows: the session sees only the unique ones
    got = hssp._solve_hssp(vals, idx, 3, ref)
    assert fake.names() == ["Hssp4dSession", "Hssp4dSession.run"]
    uniq, first = np.unique(vals, return_index=True, axis=0)
    np.testing.assert_array_equal(fake.calls[0][1], uniq)
    np.testing.assert_array_equal(got, idx[first[:3]])

    # every slot taken: returned as is
    np.testing.assert_array_equal(hssp._solve_hssp(vals, idx, 10, ref), idx)
