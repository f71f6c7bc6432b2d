"""The per-pair assembly kernel's two-block mode alone (gpk_assemble_pairs2; DERIV_SPLIT, what a
convective axis of gpk_create3_opc assembles in): K and D = c2 DD + c1 D1 as DERIV_BOTH stores
them, plus the order-1 block D1 on its own.

n = 33 (a second, ragged tile row: the mirror path) and 70 (three tile rows); Q = 1 and 30; the four
kinds.  Bars, none of them measured:
  * K and D: the bits of gpk_assemble_pairs at the same non-zero (c2, c1) -- the same expressions and
    reduction order, one more store.
  * D1: what tests/test_gpu_assemble_pairs.py::test_three_modes checks of its mode-1 block --
    off-diagonal antisymmetric to the bit, and within N_D (tests/field_ulp_inputs.py) units of
    eps B of the rectangular-block route, B = oracle field_scale.
  * zero weights: D = 0 exactly, D1 unchanged.
  * two calls: equal bits.
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.field_ulp_inputs import EPS, N_D
from tests.helpers import rand_kp
from tests.test_gpu_kron3 import KINDS

pytestmark = pytest.mark.gpu

C2, C1, JITTER = -0.3, 0.8, 1e-6


@pytest.mark.parametrize("Q", [1, 30])
@pytest.mark.parametrize("kind", KINDS)
def test_two_block_mode(kind, Q):
    from gpk._lib import assemble_pairs, assemble_pairs2
    from gpk.core import kernel_matrices
    kp = rand_kp(np.random.default_rng(70 + Q), Q, 5.0)
    for n in (33, 70):
        x = np.linspace(0, 1, n) * 2 * np.pi
        K, D, D1 = assemble_pairs2(kind, x, kp, JITTER, C2, C1)
        Kb, Db = assemble_pairs(kind, x, kp, JITTER, C2, C1)
        assert K.shape == D.shape == D1.shape == (n, n)
        assert np.isfinite(K).all() and np.isfinite(D).all() and np.isfinite(D1).all()
        assert np.array_equal(K, Kb) and np.array_equal(D, Db)
        off = ~np.eye(n, dtype=bool)
        assert np.array_equal(D1[off], -D1.T[off])
        _, Dr1 = kernel_matrices(kind, x, x, kp, JITTER, 1)
        _, B1 = O.field_scale(kind, x, x, kp, 1)
        u1 = float(np.max(np.where(B1 > 0, np.abs(D1 - Dr1) / (EPS * np.where(B1 > 0, B1, 1.0)), 0.0)))
        print(kind, "Q", Q, "n", n, "D1 %.2f (eps B)" % u1)
        assert u1 <= N_D, (n, u1)
        assert np.all(D1[B1 == 0] == 0)
        assert np.abs(D1).max() > 0.0
        # zero weights: a pure convective axis
        K0, D0, D10 = assemble_pairs2(kind, x, kp, JITTER, 0.0, 0.0)
        assert np.array_equal(K0, K) and np.all(D0 == 0.0) and np.array_equal(D10, D1)
        # the same bits again
        K2, D2, D12 = assemble_pairs2(kind, x, kp, JITTER, C2, C1)
        assert np.array_equal(K, K2) and np.array_equal(D, D2) and np.array_equal(D1, D12)
