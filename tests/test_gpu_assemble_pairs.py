"""The per-pair assembly kernel alone (gpk_assemble_pairs), in its three derivative modes: order 2,
order 1 and both (DERIV_BOTH, the mixed-order axes of gpk_create3_opx).

Sizes n = 1, 2 (one ragged tile), 31, 32, 33 (a second, ragged tile row: the mirror path), 65 (three
tile rows); Q = 1, 4, 64 (fewer components than the four waves that share them, one each, sixteen
each); the four kinds.  Bars, none of them measured:
  * K: the same bits in the three modes (the same expression, the same reduction order).
  * mixed D against c2 D2 + c1 D1 formed from the mode-2 and mode-1 blocks: 4 eps S elementwise,
    S = |c2| |D2| + |c1| |D1|.  The kernel rounds c1 (s dv1) and the two-term sum, <= 3 u S with
    u = eps / 2 and <= 2 u S fused; the host's c2 D2 + c1 D1 rounds three times, <= 3 u S: 3 eps S
    together, 4 with the margin of one rounding.
  * D - D^T = 2 c1 D1, the same bar: two kernel elements (<= 3 eps S) and the subtraction
    (u |D - D^T| <= eps |c1| |D1|).
  * D2 and D1 against gpk_kernel_matrices at the field tests' bar (tests/field_ulp_inputs.py N_D
    units of eps B, B = oracle field_scale): both routes evaluate the same terms and differ in the
    order they add the Q of them.
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.field_ulp_inputs import EPS, N_D, N_K
from tests.helpers import rand_kp
from tests.test_gpu_kron3 import KINDS

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 31, 32, 33, 65)
C2, C1, JITTER = -0.3, 0.8, 1e-6


def _x(n):
    return np.linspace(0, 1, n) * 2 * np.pi if n > 1 else np.array([0.3])


@pytest.mark.parametrize("Q", [1, 4, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_three_modes(kind, Q):
    from gpk._lib import assemble_pairs
    from gpk.core import kernel_matrices
    kp = rand_kp(np.random.default_rng(40 + Q), Q, 5.0)
    for n in SIZES:
        x = _x(n)
        K2, D2 = assemble_pairs(kind, x, kp, JITTER, 1.0, 0.0)
        K1, D1 = assemble_pairs(kind, x, kp, JITTER, 0.0, 1.0)
        Kb, Db = assemble_pairs(kind, x, kp, JITTER, C2, C1)
        assert K2.shape == D2.shape == Db.shape == (n, n)
        assert np.isfinite(K2).all() and np.isfinite(D2).all() and np.isfinite(D1).all() and np.isfinite(Db).all()
        # K: bitwise across the modes; symmetric; the unweighted blocks whatever the weight
        assert np.array_equal(K2, K1) and np.array_equal(K2, Kb)
        assert np.array_equal(K2, K2.T) and np.array_equal(D2, D2.T)
        assert np.array_equal(D1[~np.eye(n, dtype=bool)], -D1.T[~np.eye(n, dtype=bool)])
        assert np.array_equal(assemble_pairs(kind, x, kp, JITTER, -7.5, 0.0)[1], D2)
        assert np.array_equal(assemble_pairs(kind, x, kp, JITTER, 0.0, 3.25)[1], D1)
        # mixed D against the two fields of the same entry
        S = abs(C2) * np.abs(D2) + abs(C1) * np.abs(D1)
        e_mix = np.abs(Db - (C2 * D2 + C1 * D1))
        e_asym = np.abs((Db - Db.T) - 2.0 * C1 * D1)
        with np.errstate(invalid="ignore", divide="ignore"):
            u_mix = float(np.nanmax(np.where(S > 0, e_mix / (EPS * S), 0.0)))
            u_asym = float(np.nanmax(np.where(S > 0, e_asym / (EPS * S), 0.0)))
        # the two fields against the rectangular-block route
        Kr, Dr2 = kernel_matrices(kind, x, x, kp, JITTER, 2)
        _, Dr1 = kernel_matrices(kind, x, x, kp, JITTER, 1)
        BK, B2 = O.field_scale(kind, x, x, kp, 2)
        _, B1 = O.field_scale(kind, x, x, kp, 1)
        units = lambda a, b, B: float(np.max(np.where(B > 0, np.abs(a - b) / (EPS * np.where(B > 0, B, 1.0)), 0.0)))
        uK, u2, u1 = units(K2, Kr, BK), units(D2, Dr2, B2), units(D1, Dr1, B1)
        print(kind, "Q", Q, "n", n, "mixed %.2f asym %.2f (eps S) | K %.2f D2 %.2f D1 %.2f (eps B)"
              % (u_mix, u_asym, uK, u2, u1))
        assert np.all(e_mix <= 4.0 * EPS * S), (n, u_mix)
        assert np.all(e_asym <= 4.0 * EPS * S), (n, u_asym)
        assert uK <= N_K and u2 <= N_D and u1 <= N_D, (n, uK, u2, u1)
        assert np.all(D1[B1 == 0] == 0) and np.all(Dr1[B1 == 0] == 0)
        if n > 1:  # neither symmetric nor antisymmetric
            assert not np.array_equal(Db, Db.T) and not np.array_equal(Db, -Db.T)
        # the same bits again
        Kb2, Db2 = assemble_pairs(kind, x, kp, JITTER, C2, C1)
        assert np.array_equal(Kb, Kb2) and np.array_equal(Db, Db2)

