#!/usr/bin/env python
"""Generate ``tests/golden/truncnorm_edges.json``: truncated-normal edge points
evaluated with mpmath at 50 digits and rounded to float64.

The file is committed so that the tests need no mpmath. Inputs are float64
values taken exactly; every expected value is the correctly rounded result for
those exact inputs, independent of any of the project's (or scipy's) formulas.

Usage: ``python scripts/gen_truncnorm_golden.py`` (rewrites the JSON file).

Excluded on purpose (ppf): a < 0 with b > 6 and q > 1 - 1e-6, where the
formulation ``logaddexp(log Phi(a), log q + log mass)`` used by host, device
and scipy alike is ill-conditioned (host error 1.8e-5 at q = 1 - 1e-12 on
(-1, 40)); and a == b, where host gives NaN and device gives a.
"""
from __future__ import annotations

import json
from pathlib import Path

import mpmath as mp


OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "truncnorm_edges.json"

DEEP_LEFT = [(-40.0, -39.0), (-38.5, -38.4), (-37.3, -37.0)]
DEEP_RIGHT = [(-b, -a) for a, b in DEEP_LEFT]

MASS_INTERVALS = (
    DEEP_LEFT
    + DEEP_RIGHT
    + [(-1e10, 1e10), (-1e10, -35.0), (29.0, 1e10)]
    + [(-1e-3, 1e-3), (-5e-4, 5e-4), (0.0, 1e-3), (-1e-3, 0.0)]
    + [(-8.0, 8.0), (-8.0, 1e-3), (0.0, 40.0), (-1.0, 40.0)]
    + [(5.0, 5.0 + 1e-6), (-(5.0 + 1e-6), -5.0)]
    + [(2.0, 1.0), (0.5, 0.5), (-37.0, -37.3)]  # a >= b: empty
)

PPF_INTERVALS = DEEP_LEFT + [
    (39.0, 40.0), (-40.0, 1.0), (-8.0, 8.0), (-2.0, 2.0), (0.0, 1e-3), (-1e-3, 0.0), (0.5, 3.0),
]
PPF_Q = [
    0.0, 1e-300, 1e-12, 1e-3, 0.25, 0.5, 0.75, 1.0 - 1e-3, 1.0 - 1e-12, 1.0 - 2.0**-53, 1.0,
]


def _f(v) -> float:
    return float(v)


def _cdf(x):
    return mp.erfc(-x / mp.sqrt(2)) / 2


def _sf(x):
    return mp.erfc(x / mp.sqrt(2)) / 2


def _mass(a, b):
    """Phi(b) - Phi(a) as an mpf, from the tail that does not cancel."""
    if a > 0:
        return _sf(a) - _sf(b)
    if b <= 0:
        return _cdf(b) - _cdf(a)
    return 1 - (_cdf(a) + _sf(b))


def log_mass(a: float, b: float) -> float:
    if not a < b:
        return float("-inf")
    a_, b_ = mp.mpf(a), mp.mpf(b)
    if a_ > 0 or b_ <= 0:
        return _f(mp.log(_mass(a_, b_)))
    return _f(mp.log1p(-(_cdf(a_) + _sf(b_))))


def ppf(q: float, a: float, b: float) -> float:
    if q == 0.0:
        return a
    if q == 1.0:
        return b
    a_, b_, q_ = mp.mpf(a), mp.mpf(b), mp.mpf(q)
    mass = _mass(a_, b_)
    if a < 0:
        target = _cdf(a_) + q_ * mass
        below = lambda x: _cdf(x) < target  # noqa: E731
    else:
        target = _sf(b_) + (1 - q_) * mass
        below = lambda x: _sf(x) > target  # noqa: E731
    lo, hi = a_, b_
    for _ in range(220):
        mid = (lo + hi) / 2
        if below(mid):
            lo = mid
        else:
            hi = mid
    return _f((lo + hi) / 2)


def logpdf(x: float, a: float, b: float, loc: float, scale: float) -> float:
    z = (mp.mpf(x) - mp.mpf(loc)) / mp.mpf(scale)
    if z < a or z > b:
        return float("-inf")
    a_, b_ = mp.mpf(a), mp.mpf(b)
    if a_ > 0 or b_ <= 0:
        lm = mp.log(_mass(a_, b_))
    else:
        lm = mp.log1p(-(_cdf(a_) + _sf(b_)))
    return _f(-z * z / 2 - mp.log(2 * mp.pi) / 2 - lm - mp.log(mp.mpf(scale)))


def _ppf_excluded(q: float, a: float, b: float) -> bool:
    return a < 0 and b > 6 and q > 1 - 1e-6


def _logpdf_points() -> list[tuple[float, float, float, float, float]]:
    import math

    pts = []
    for a, b in DEEP_LEFT + DEEP_RIGHT + [(-2.0, 2.0), (0.5, 3.0)]:
        # at both bounds, inside, and one ulp outside each bound
        for x in (a, b, 0.5 * (a + b), math.nextafter(a, -math.inf), math.nextafter(b, math.inf)):
            pts.append((x, a, b, 0.0, 1.0))
    for scale in (1e-8, 1e8):
        for a, b in [(-2.0, 2.0), (-40.0, -39.0), (37.0, 37.3)]:
            for frac in (0.25, 0.5, 0.75):
                z = a + frac * (b - a)
                pts.append((3.0 + z * scale, a, b, 3.0, scale))
                pts.append((z * scale, a, b, 0.0, scale))
    return pts


def generate() -> dict:
    mp.mp.dps = 50
    return {
        "log_gauss_mass": [
            {"a": a, "b": b, "expected": log_mass(a, b)} for a, b in MASS_INTERVALS
        ],
        "ppf": [
            {"q": q, "a": a, "b": b, "expected": ppf(q, a, b)}
            for a, b in PPF_INTERVALS
            for q in PPF_Q
            if not _ppf_excluded(q, a, b)
        ],
        "logpdf": [
            {"x": x, "a": a, "b": b, "loc": loc, "scale": scale,
             "expected": logpdf(x, a, b, loc, scale)}
            for x, a, b, loc, scale in _logpdf_points()
        ],
    }


def main() -> None:
    OUT.parent.mkdir(parents=True, exist_ok=True)
    OUT.write_text(json.dumps(generate(), indent=1) + "\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
