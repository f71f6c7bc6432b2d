"""Inputs of the field-accuracy tests, shared by the GPU test (tests/test_gpu_field_ulps.py) and
the CPU test of its power (tests/test_oracle.py) so the two cannot drift apart.  Numbers only:
coordinates, kernel parameters, the bar -- no oracle and no device code.

Regimes (log-ls = log-w = 0 in the first three: a = w = 1 on any exp implementation, which keeps
the device's own exp(log-ls) out of the comparison -- one ulp of a moves e^{-r} by r ulp):
  phase    x = linspace(0, 1, n) 2 pi, freq up to 100: phases up to ~3900 rad.  Plain fp64 rounds
           the phase by ~|phase| eps: discriminating for the kinds with a cosine.
  radial   random sorted x on [0, L] (the step routes: the grid linspace(0, 1, n) L), small freq;
           L per kind so that the radial argument reaches sqrt5 L = 270 (Matern52) / L^2 = 412
           (SE), inside the normal range (<= 600: nothing is denormal), and no multiple of a
           power of two, so that a grid's a d^2 is not exact.  Discriminating for every kind.
  single   one component (Q = 1) at a high frequency.
  generic5, generic40   tests/helpers.rand_kp at fs = 50: ordinary parameters, Q = 40 puts a
           second component on each lane of the class values' 32-lane butterfly.  Not
           discriminating; it guards the formulas.
phase and radial have a freq = 0 component inside the cosine kinds; the rectangular block has one
zero distance off the diagonal and one duplicated point, the square ones the diagonal.
"""
import numpy as np

from tests.helpers import rand_kp

KINDS = ["SE_Cos_1d", "Matern52_Cos_1d", "SE_1d", "Matern52_1d"]
COS_KINDS = ("SE_Cos_1d", "Matern52_Cos_1d")

# the bar, in units of eps * B (oracle/gp_oracle.py field_scale): exp and sincos at <= 2 ulp each,
# one fma correction each, <= 3 polynomial roundings, two or four products, a three-term sum for D,
# <= 2 for accumulating Q <= 64 terms (tests/test_gpu_field_ulps.py docstring)
N_K, N_D = 8.0, 12.0
EPS = 2.0 ** -52

RADIAL_L = {"Matern52_Cos_1d": 120.7, "Matern52_1d": 120.7, "SE_Cos_1d": 20.3, "SE_1d": 20.3}
REGIMES = ("phase", "radial", "single", "generic5", "generic40")


def kernel_paras(regime):
    if regime == "phase":
        return {"freq": np.array([0.0, 33.3, 71.9, 100.0]), "log-ls": np.zeros(4), "log-w": np.zeros(4)}
    if regime == "radial":
        return {"freq": np.array([0.0, 0.4, 1.1, 2.3]), "log-ls": np.zeros(4), "log-w": np.zeros(4)}
    if regime == "single":
        return {"freq": np.array([71.9]), "log-ls": np.zeros(1), "log-w": np.zeros(1)}
    Q = {"generic5": 5, "generic40": 40}[regime]
    return rand_kp(np.random.default_rng(100 + Q), Q, 50.0)


def extent(regime, kind):
    return RADIAL_L[kind] if regime == "radial" else 2.0 * np.pi


def grid(regime, kind, n):
    """The collocation grid of the step routes: linspace(0, 1, n) * extent."""
    return np.linspace(0, 1, n) * extent(regime, kind)


def scattered(regime, kind, n, seed):
    """Random sorted points on [0, extent] (the per-pair routes; no distance classes)."""
    return np.sort(np.random.default_rng(seed).uniform(0.0, extent(regime, kind), n))


def rect_block(regime, kind):
    """(x1 [37], x2 [29]) of the rectangular block: the phase regime's grid points / random sorted
    points elsewhere, with x2[4] = x1[7] (a zero distance off the diagonal: abs'(0) = +1) and
    x1[21] = x1[20] (a duplicated point: two equal rows)."""
    if regime == "phase":
        x1, x2 = grid(regime, kind, 37), grid(regime, kind, 29)
    else:
        x1, x2 = scattered(regime, kind, 37, 11), scattered(regime, kind, 29, 12)
    x1[21] = x1[20]
    x2[4] = x1[7]
    return x1, x2


def square_block(regime, kind):
    """x [33] of the square block with jitter."""
    return grid(regime, kind, 33) if regime == "phase" else scattered(regime, kind, 33, 13)


def discriminating(regime, kind):
    """Plain fp64 must miss the bar by 2x here (checked on the CPU, tests/test_oracle.py)."""
    return regime == "radial" or (regime == "phase" and kind in COS_KINDS)


def blocks(regime, kind):
    """Every (name, x1, x2) the tests evaluate for a regime and kind: the direct routes' blocks
    and the step routes' grids (1D n = 33; 2D 33 x 40) and scattered axis."""
    x1, x2 = rect_block(regime, kind)
    xs = square_block(regime, kind)
    out = [("rect", x1, x2), ("square", xs, xs)]
    for n in (33, 40):
        g = grid(regime, kind, n)
        out.append((f"grid{n}", g, g))
    # 40 scattered points: 39 distinct distances on the first diagonal, more than the 32 a
    # distance-class table holds, so the step assembles this axis per pair (33 points would not)
    sc = scattered(regime, kind, 40, 14)
    out.append(("scattered", sc, sc))
    return out


def dd_inputs(kind):
    """(d [257], a, freq) of the double-double field tests: d = 0 and 256 random sorted distances
    over the ranges the double-double exp / sincos were validated on (radial argument <= 60,
    phase <= 1200 rad), one component with a = 3.7, freq = 23.3."""
    a, freq = 3.7, 23.3
    dmax = 60.0 / (np.sqrt(5.0) * a) if "Matern" in kind else np.sqrt(60.0 / a)
    dmax = min(dmax, 1200.0 / (2.0 * np.pi * freq))
    d = np.sort(np.random.default_rng(21).uniform(0.0, dmax, 256))
    return np.concatenate(([0.0], d)), a, freq


DD_BAR = 1e-26  # x the field's absolute-monomial scale (tests/mp_fields.py)
