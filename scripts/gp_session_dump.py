"""Outputs of the three native GP sessions on fixed synthetic inputs, as one .npz.

``python scripts/gp_session_dump.py OUT.npz`` writes ``f`` and ``g`` of
``GpLogEiSession`` and ``GpLogEhviSession`` (M = 2 and 4), each with and without
``constraints=``, and of ``GpConstraintSet`` alone (C = 1 and 3), at the smallest
shapes that reach every branch: N in {1, 257}, D in {1, 64}, B in {1, 9}, Q = 5,
J in {1, GP_EHVI_BOX_TILE + 1}, with and without the gradient, and B = 13 under
a scratch budget that makes seven chunks of it.

``python scripts/gp_session_dump.py --compare A.npz B.npz`` exits 0 if both hold
the same arrays bit for bit and prints how many there are.

It imports ``optuna_amd`` from the current directory and uses the extension's
bindings only, so it also runs from an export of an older commit: dump from
both trees in one job and compare. A GPU is required for the dump.
"""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np


STAB = 1e-12


def _matern(r2: np.ndarray) -> np.ndarray:
    u = np.sqrt(5.0 * r2)
    return np.exp(-u) * ((5.0 / 3.0) * r2 + u + 1.0)


class _Gps:
    """n synthetic GPs over one X: random eta / scale / alpha and the inverse of
    the GP's own Matern covariance plus 0.1 I, on the device."""

    def __init__(self, N: int, D: int, n: int, seed: int) -> None:
        import torch

        rng = np.random.RandomState(seed)
        self.N, self.D, self.n = N, D, n
        X = rng.rand(N, D)
        self.scale = [float(0.5 + rng.rand()) for _ in range(n)]
        eta = [(0.5 + rng.rand(D)) * (2.0 / D) for _ in range(n)]
        alpha = [rng.randn(N) / np.sqrt(N) for _ in range(n)]
        cinv = []
        for i in range(n):
            r2 = (np.square(X[:, None, :] - X[None, :, :]) * eta[i]).sum(-1)
            cinv.append(np.linalg.inv(self.scale[i] * _matern(r2) + 0.1 * np.eye(N)))
        self.thresholds = [float(t) for t in 0.3 * rng.randn(n)]
        self.rng = rng

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).cuda()

        self.X = up(X)
        self.eta, self.alpha, self.cinv = ([up(a) for a in l] for l in (eta, alpha, cinv))
        torch.cuda.synchronize()

    def _ptrs(self, lo: int, hi: int):
        return (
            [self.X.data_ptr()] * (hi - lo),
            [t.data_ptr() for t in self.alpha[lo:hi]],
            [t.data_ptr() for t in self.cinv[lo:hi]],
            [t.data_ptr() for t in self.eta[lo:hi]],
            self.scale[lo:hi],
        )

    def constraint_set(self, core, lo: int, hi: int, **kw):
        return core.GpConstraintSet(
            *self._ptrs(lo, hi), self.thresholds[lo:hi], self.N, self.D, STAB, **kw
        )

    def logei(self, core):
        X, alpha, cinv, eta, scale = self._ptrs(0, 1)
        return core.GpLogEiSession(
            X[0], alpha[0], cinv[0], eta[0], self.N, self.D, scale[0], STAB, 0.1
        )

    def logehvi(self, core, M: int, Q: int, J: int, **kw):
        eps = self.rng.randn(Q, M)
        lo = 0.7 * self.rng.randn(J, M)
        iv = 0.05 + 1.95 * self.rng.rand(J, M)
        iv[J // 2, 0] = np.inf
        return core.GpLogEhviSession(*self._ptrs(0, M), self.N, self.D, STAB, eps, lo, iv, **kw)


def dump(path: str) -> None:
    sys.path.insert(0, os.getcwd())
    import torch

    from optuna_amd import _hip

    # torch opens the device before the extension does, as in the sampler.
    if not torch.cuda.is_available():
        raise SystemExit("gp_session_dump: a GPU is required")
    torch.zeros(1, device="cuda")
    core = _hip.require()
    if core is None or not core.available():
        raise SystemExit("gp_session_dump: a GPU and the built extension are required")
    out: dict[str, np.ndarray] = {}

    def record(name: str, x: np.ndarray, evaluate) -> None:
        for grad in (False, True):
            f, g = evaluate(x, grad)
            out[f"{name} grad={int(grad)} f"] = np.asarray(f)
            out[f"{name} grad={int(grad)} g"] = np.asarray(g)

    def record_all(gps: _Gps, tag: str, x: np.ndarray, budget_rows: "int | None") -> None:
        # GPs 0..3 are objectives, 4..6 constraints. budget_rows candidates of
        # one K / MP / V set per objective kept (the gradient's need) fit.
        def kw(n_sets: int) -> dict:
            if budget_rows is None:
                return {}
            return dict(scratch_budget_bytes=budget_rows * n_sets * 3 * gps.N * 8)

        three = gps.constraint_set(core, 4, 7, **kw(1))
        for C in (1, 3):
            record(f"{tag} set C={C}", x, gps.constraint_set(core, 4, 4 + C, **kw(1)).eval)
        if budget_rows is None:  # the LogEI session does not chunk
            sess = gps.logei(core)
            record(f"{tag} logei", x, sess.eval)
            record(f"{tag} logei+c", x, lambda x, grad: sess.eval(x, grad, constraints=three))
        for M, J in itertools.product((2, 4), (1, core.GP_EHVI_BOX_TILE + 1)):
            sess = gps.logehvi(core, M, 5, J, **kw(M))
            record(f"{tag} ehvi M={M} J={J}", x, sess.eval)
            record(
                f"{tag} ehvi+c M={M} J={J}", x,
                lambda x, grad: sess.eval(x, grad, constraints=three),
            )
            if budget_rows is not None:
                assert sess.n_chunks(len(x), True) == 7, sess.n_chunks(len(x), True)
        if budget_rows is not None:
            assert three.n_chunks(len(x), True) == 7

    for N, D in itertools.product((1, 257), (1, 64)):
        gps = _Gps(N, D, 7, seed=1000 * N + D)
        for B in (1, 9):
            x = np.random.RandomState(B).rand(B, D)
            record_all(gps, f"N={N} D={D} B={B}", x, None)
    gps = _Gps(257, 7, 7, seed=77)
    record_all(gps, "N=257 D=7 B=13 chunks", np.random.RandomState(13).rand(13, 7), 2)

    assert all(np.isfinite(a).all() for a in out.values())
    np.savez(path, **out)
    print(f"gp_session_dump: wrote {len(out)} arrays to {path}")


def compare(path_a: str, path_b: str) -> None:
    a, b = np.load(path_a), np.load(path_b)
    if sorted(a.files) != sorted(b.files):
        raise SystemExit("gp_session_dump: the two files hold different cases")
    differ = [k for k in a.files if not np.array_equal(a[k], b[k])]
    for k in differ:
        print(f"DIFFERS: {k}: max abs {np.max(np.abs(a[k] - b[k])):.3e}")
    nonempty = sum(a[k].size > 0 for k in a.files)
    print(f"gp_session_dump: {len(a.files)} arrays compared ({nonempty} non-empty), "
          f"{len(differ)} differ")
    raise SystemExit(1 if differ else 0)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 2:
        dump(sys.argv[1])
    else:
        raise SystemExit(__doc__)
