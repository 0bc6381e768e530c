#!/usr/bin/env python
"""Generate ``tests/golden/gp_logei_edges.json``: edge points of the GP sampler's
log-EI acquisition, evaluated with mpmath at 80 digits and rounded to float64.

The file is committed so that the tests need no mpmath. Inputs are float64
values taken exactly; every expected value is the correctly rounded result for
those exact inputs, independent of the host formula (``acqf.standard_logei``)
and of the device kernel (``k_gp_logei_final``), which mirror each other.

Usage: ``python scripts/gen_gp_logei_golden.py`` (rewrites the JSON file and
prints the two figures behind the series cut of the implementations).

Section ``standard``: for each z, with h(z) = z Phi(z) + phi(z),
``log_h`` = log h, ``r_m`` = Phi / h = d log h / dz and ``r_v`` = phi / h.

Section ``session``: complete small problems for one candidate ``x``. The rules:

* k_i = scale * m52(r2_i), m52(r2) = exp(-u) (5/3 r2 + u + 1), u = sqrt(5 r2),
  r2_i = sum_d eta_d (x_d - X_id)^2; on a column of ``cat_mask`` (bit d = column
  d) the Hamming term eta_d [x_d != X_id] replaces the squared difference;
* mean = k . alpha;  raw = scale - k . Cinv . k  (``cinv`` is any symmetric
  matrix, it need not be an inverse: that is how a case steers ``raw``);
* var = max(raw, 0) + stab;  z = (mean - threshold) / sqrt(var);
* f = 1/2 log var + log h(z);
* grad = df/dmean grad(mean) + [raw >= 0] df/dvar grad(raw), with
  df/dmean = r_m / sqrt(var), df/dvar = r_v / (2 var),
  dk_i/dx_d = scale m52'(r2_i) 2 eta_d (x_d - X_id), m52' = -5/6 (1 + u) exp(-u),
  grad(raw) = -2 sum_i (Cinv k)_i grad(k_i), and exactly 0 on a masked column.

A case whose threshold is given as a target z takes
threshold = mean - z sqrt(var) rounded to float64; everything is then evaluated
for that float64 threshold.

Admissibility (enforced, see ``_admit``): the tolerances of the tests are
value rtol 1e-8 / atol 1e-10 and gradient rtol 1e-6 / atol 1e-8. A correct
float64 evaluation gets ``mean`` within 4 * 2^-53 * sum|k_i alpha_i| and ``raw``
within 4 * 2^-53 * (scale + sum|k_i (Cinv k)_i|). The reference is re-evaluated
with ``mean`` and with ``raw`` shifted by these amounts either way; a case in
which f or grad then moves by more than a tenth of its tolerance, or in which
the shift of ``raw`` crosses 0, is refused, and other inputs have to be picked.
The deep-tail cases sit on the variance clamp for this reason: sqrt(var) is
then exactly sqrt(stab), whatever ``raw`` rounds to.
"""
from __future__ import annotations

import json
import math
from pathlib import Path

import mpmath as mp


OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "gp_logei_edges.json"

DPS = 80  # z = -1e10 cancels 20 digits in z Phi + phi; 60 are left
F_TOL = dict(rtol=1e-8, atol=1e-10)
G_TOL = dict(rtol=1e-6, atol=1e-8)
STAB = 1e-12

# Where the implementations switch from 1 + m (m = sqrt(pi/2) z erfcx(-z/sqrt 2))
# to its asymptotic series, and after how many terms they stop. Used here only
# to place points and to print the figures that justify the pair.
SERIES_Z = -256.0
SERIES_TERMS = 4


def _f(v) -> float:
    return float(v)


def _nbrs(v: float) -> list[float]:
    return [math.nextafter(v, -math.inf), v, math.nextafter(v, math.inf)]


STANDARD_Z = (
    _nbrs(-1.0)
    + [-1.5, -0.5, 0.0, 1e-300, -1e-300, 3.0, 8.0, 40.0]
    + [-5.0, -20.0, -38.0, -39.0, -100.0]
    + _nbrs(SERIES_Z)
    + [-1e3, -1e4, -1e5, -1e6, -1e7, -1e8, -1e10]
)


def standard(z):
    """(log h, Phi / h, phi / h) at the mpf z."""
    Phi = mp.erfc(-z / mp.sqrt(2)) / 2
    phi = mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi)
    h = z * Phi + phi
    return mp.log(h), Phi / h, phi / h


def series_figures(cut: float = SERIES_Z, terms: int = SERIES_TERMS) -> dict:
    """Relative truncation error of the series at the cut, with ``terms`` and
    with one term fewer, and the loss z^2 2^-53 of the direct form there."""
    z = mp.mpf(cut)
    exact = 1 + mp.sqrt(mp.pi / 2) * z * mp.erfc(-z / mp.sqrt(2)) * mp.exp(z * z / 2)

    def partial(n):
        return sum((-1) ** (j + 1) * mp.fac2(2 * j - 1) / z ** (2 * j) for j in range(1, n + 1))

    return {
        "cut": cut,
        "terms": terms,
        "truncation": _f(abs(partial(terms) / exact - 1)),
        "truncation_one_term_fewer": _f(abs(partial(terms - 1) / exact - 1)),
        "two_to_minus_53": 2.0**-53,
        "direct_form_loss": cut * cut * 2.0**-53,
        "largest_cut_for_loss_1e-8": _f(mp.sqrt(mp.mpf(1e-8) * 2**53)),
    }


# ---- the session cases ---------------------------------------------------------------

X32 = [[0.125, 0.75], [0.5, 0.25], [0.875, 0.625]]
X23 = [[0.25, 0.5, 0.75], [0.625, 0.125, 0.375]]

GPS = {
    # raw of order one
    "n3d2": dict(
        N=3, D=2, cat_mask=0, X=X32, eta=[1.5, 0.75], scale=1.25,
        alpha=[0.5, -0.25, 0.75],
        cinv=[[0.2, 0.03, -0.02], [0.03, 0.15, 0.01], [-0.02, 0.01, 0.25]],
    ),
    "n1d1": dict(N=1, D=1, cat_mask=0, X=[[0.25]], eta=[2.0], scale=0.8, alpha=[1.5],
                 cinv=[[0.9]]),
    # column 1 is categorical
    "n2d3cat": dict(
        N=2, D=3, cat_mask=0b010, X=[[0.2, 0.0, 0.7], [0.6, 1.0, 0.1]],
        eta=[1.0, 0.5, 2.0], scale=1.0, alpha=[0.4, -0.9], cinv=[[0.3, 0.05], [0.05, 0.2]],
    ),
    # every k_i underflows in float64
    "n2d2far": dict(
        N=2, D=2, cat_mask=0, X=[[0.1, 0.2], [0.8, 0.9]], eta=[1e6, 1e6], scale=1.0,
        alpha=[1.0, -2.0], cinv=[[0.5, 0.0], [0.0, 0.5]],
    ),
    # cinv = 50 I with 50 k.k > scale: raw < 0
    "n3d2clamp": dict(
        N=3, D=2, cat_mask=0, X=X32, eta=[0.3, 0.2], scale=1.0, alpha=[0.5, -0.25, 0.75],
        cinv=[[50.0, 0.0, 0.0], [0.0, 50.0, 0.0], [0.0, 0.0, 50.0]],
    ),
    "n2d3clamp": dict(
        N=2, D=3, cat_mask=0, X=X23, eta=[0.2, 0.3, 0.1], scale=1.5, alpha=[0.75, -0.5],
        cinv=[[50.0, 0.0], [0.0, 50.0]],
    ),
    "n1d1clamp": dict(N=1, D=1, cat_mask=0, X=[[0.5]], eta=[1.0], scale=1.0, alpha=[2.0],
                      cinv=[[50.0]]),
}

X_N3D2 = [0.3125, 0.4375]
X_N2D3 = [0.4375, 0.3125, 0.5625]

# (name, gp, x, target z or None, threshold or None, expected sign of raw)
CASES = [
    ("order one, z = -3", "n3d2", X_N3D2, -3.0, None, 1),
    ("order one, z just below -1", "n3d2", X_N3D2, -1.0 - 1e-6, None, 1),
    ("order one, z just above -1", "n3d2", X_N3D2, -1.0 + 1e-6, None, 1),
    ("order one, z = 0", "n3d2", X_N3D2, 0.0, None, 1),
    ("order one, z = +5", "n3d2", X_N3D2, 5.0, None, 1),
    ("order one, z above the series cut", "n3d2", X_N3D2, -250.0, None, 1),
    ("order one, z below the series cut", "n3d2", X_N3D2, -260.0, None, 1),
    ("order one, z = -2000", "n3d2", X_N3D2, -2000.0, None, 1),
    ("order one, z = -1e5", "n3d2", X_N3D2, -1e5, None, 1),
    ("candidate on a training row, N = 3", "n3d2", X32[1], -2.0, None, 1),
    ("N = 1, z = -3", "n1d1", [0.625], -3.0, None, 1),
    ("candidate on the training row, N = 1", "n1d1", [0.25], -1.25, None, 1),
    ("masked column", "n2d3cat", [0.45, 1.0, 0.3], -1.5, None, 1),
    ("masked column, code no row has", "n2d3cat", [0.45, 7.0, 0.3], 0.5, None, 1),
    ("all k underflow", "n2d2far", [0.5, 0.5], None, 0.5, 1),
    ("all k underflow, z = +2", "n2d2far", [0.4375, 0.5625], None, -2.0, 1),
    ("clamp, z = +4", "n3d2clamp", X_N3D2, 4.0, None, -1),
    ("clamp, z = -20", "n3d2clamp", X_N3D2, -20.0, None, -1),
    ("clamp, z = -1e3", "n3d2clamp", X_N3D2, -1e3, None, -1),
    ("clamp, mean = threshold", "n3d2clamp", X_N3D2, 0.0, None, -1),
    ("clamp, z above the series cut", "n3d2clamp", X_N3D2, -255.5, None, -1),
    ("clamp, z below the series cut", "n3d2clamp", X_N3D2, -256.5, None, -1),
    ("clamp, z = -1e5", "n2d3clamp", X_N2D3, -1e5, None, -1),
    ("clamp, z = -1e6", "n2d3clamp", X_N2D3, -1e6, None, -1),
    ("clamp, z = -1e7", "n2d3clamp", X_N2D3, -1e7, None, -1),
    ("clamp, z = -1e8", "n2d3clamp", X_N2D3, -1e8, None, -1),
    ("clamp, z = -1e10", "n2d3clamp", X_N2D3, -1e10, None, -1),
    ("clamp, N = 1, z = -3", "n1d1clamp", [0.75], -3.0, None, -1),
    ("clamp, N = 1, z = -1e6", "n1d1clamp", [0.75], -1e6, None, -1),
]


def posterior(gp: dict, x: list[float]) -> dict:
    """mean, raw, their input gradients and the two rounding scales, as mpf."""
    N, D, mask = gp["N"], gp["D"], gp["cat_mask"]
    X = [[mp.mpf(v) for v in row] for row in gp["X"]]
    eta = [mp.mpf(v) for v in gp["eta"]]
    alpha = [mp.mpf(v) for v in gp["alpha"]]
    cinv = [[mp.mpf(v) for v in row] for row in gp["cinv"]]
    assert all(gp["cinv"][i][j] == gp["cinv"][j][i] for i in range(N) for j in range(N))
    scale = mp.mpf(gp["scale"])
    xs = [mp.mpf(v) for v in x]
    k, dk = [], []  # dk[i][d] = dk_i / dx_d
    for i in range(N):
        r2 = mp.mpf(0)
        for d in range(D):
            if (mask >> d) & 1:
                r2 += eta[d] * (1 if xs[d] != X[i][d] else 0)
            else:
                r2 += eta[d] * (xs[d] - X[i][d]) ** 2
        u = mp.sqrt(5 * r2)
        k.append(scale * mp.exp(-u) * (mp.mpf(5) / 3 * r2 + u + 1))
        slope = scale * (-mp.mpf(5) / 6) * (1 + u) * mp.exp(-u)
        dk.append([
            mp.mpf(0) if (mask >> d) & 1 else slope * 2 * eta[d] * (xs[d] - X[i][d])
            for d in range(D)
        ])
    v = [sum(cinv[i][j] * k[j] for j in range(N)) for i in range(N)]
    return dict(
        mean=sum(k[i] * alpha[i] for i in range(N)),
        raw=scale - sum(k[i] * v[i] for i in range(N)),
        gmean=[sum(alpha[i] * dk[i][d] for i in range(N)) for d in range(D)],
        graw=[-2 * sum(v[i] * dk[i][d] for i in range(N)) for d in range(D)],
        mean_scale=sum(abs(k[i] * alpha[i]) for i in range(N)),
        raw_scale=scale + sum(abs(k[i] * v[i]) for i in range(N)),
    )


def acquisition(mean, raw, gmean, graw, threshold, stab):
    """(f, grad, z) of log-EI from the posterior quantities."""
    passes = raw >= 0
    var = (raw if passes else mp.mpf(0)) + stab
    sd = mp.sqrt(var)
    z = (mean - threshold) / sd
    log_h, r_m, r_v = standard(z)
    w_m = r_m / sd
    w_v = r_v / (2 * var) if passes else mp.mpf(0)
    grad = [w_m * gm + w_v * gr for gm, gr in zip(gmean, graw)]
    return mp.log(var) / 2 + log_h, grad, z


def _within_a_tenth(moved, base, tol) -> bool:
    return abs(moved - base) <= (tol["atol"] + tol["rtol"] * abs(base)) / 10


def _admit(name: str, post: dict, threshold, stab) -> None:
    f, grad, _ = acquisition(post["mean"], post["raw"], post["gmean"], post["graw"],
                             threshold, stab)
    ulps = 4 * mp.mpf(2) ** -53
    d_mean = ulps * post["mean_scale"]
    d_raw = ulps * post["raw_scale"]
    if post["raw"] == 0 or (post["raw"] + d_raw >= 0) != (post["raw"] - d_raw >= 0):
        raise ValueError(f"{name}: the rounding of raw crosses 0")
    for mean, raw in (
        (post["mean"] + d_mean, post["raw"]), (post["mean"] - d_mean, post["raw"]),
        (post["mean"], post["raw"] + d_raw), (post["mean"], post["raw"] - d_raw),
    ):
        f2, grad2, _ = acquisition(mean, raw, post["gmean"], post["graw"], threshold, stab)
        if not _within_a_tenth(f2, f, F_TOL):
            raise ValueError(f"{name}: f moves by {_f(f2 - f)} under rounding of its inputs")
        for g2, g in zip(grad2, grad):
            if not _within_a_tenth(g2, g, G_TOL):
                raise ValueError(f"{name}: grad moves by {_f(g2 - g)} under rounding")


def session_case(name, gp_name, x, z_target, threshold, raw_sign) -> dict:
    gp = GPS[gp_name]
    stab = mp.mpf(STAB)
    post = posterior(gp, x)
    if threshold is None:
        var = (post["raw"] if post["raw"] >= 0 else mp.mpf(0)) + stab
        threshold = _f(post["mean"] - mp.mpf(z_target) * mp.sqrt(var))
    thr = mp.mpf(threshold)
    _admit(name, post, thr, stab)
    f, grad, z = acquisition(post["mean"], post["raw"], post["gmean"], post["graw"], thr, stab)
    if (post["raw"] >= 0) != (raw_sign > 0):
        raise ValueError(f"{name}: raw = {_f(post['raw'])} is on the wrong side of 0")
    if z_target is not None and z_target != 0.0:
        # The rounding of the threshold leaves z on its side of every branch.
        if abs(z / mp.mpf(z_target) - 1) > mp.mpf(10) ** -9:
            raise ValueError(f"{name}: z = {_f(z)} missed its target {z_target}")
    return dict(
        name=name, gp=gp_name, **gp, stab=STAB, threshold=threshold, x=list(x),
        f=_f(f), grad=[_f(g) for g in grad], mean=_f(post["mean"]), raw=_f(post["raw"]),
        z=_f(z),
    )


def standard_row(z: float) -> dict:
    log_h, r_m, r_v = standard(mp.mpf(z))
    return {"z": z, "log_h": _f(log_h), "r_m": _f(r_m), "r_v": _f(r_v)}


def generate() -> dict:
    mp.mp.dps = DPS
    return {
        "standard": [standard_row(z) for z in STANDARD_Z],
        "session": [session_case(*case) for case in CASES],
    }


def main() -> None:
    OUT.parent.mkdir(parents=True, exist_ok=True)
    OUT.write_text(json.dumps(generate(), indent=1) + "\n")
    print(f"wrote {OUT}")
    for key, value in series_figures().items():
        print(f"  {key}: {value!r}")


if __name__ == "__main__":
    main()
