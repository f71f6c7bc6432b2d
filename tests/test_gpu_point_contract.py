"""The scattered-point contraction kernel alone (gpk_point_contract, csrc/point_eval.hip):
out[p][c] = sum_{j < n} field(t[p], x[j]) T[p][j][c] with the field evaluated on the fly.

Reference: F @ T per point with F the block gpk_kernel_matrices(kind, deriv, t, x, ...) returns
(the kernel must evaluate those values).  Bar, element by element: the dot-product bound of the
mode-GEMM tests, |err| <= 2 n eps sum_j |F_pj| |T_pjc|.
"""
import numpy as np
import pytest

from tests.helpers import rand_kp

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
KINDS = ["SE_Cos_1d", "Matern52_Cos_1d", "SE_1d", "Matern52_1d"]
NS = [1, 31, 32, 33, 63, 64, 65, 257]   # lane and wave boundaries of the j stride
CS = [1, 2, 31, 32, 33, 257]            # both regimes, a column-block boundary, a ragged last block
MS = [1, 5, 67]                         # a partly filled points-per-workgroup group
X_MAX = 2.0


def _field(kind, t, x, kp, deriv):
    from gpk.core import kernel_matrices
    K, D = kernel_matrices(kind, t, x, kp, 0.0, deriv)
    return D if deriv else K


def _check(out, F, T3, label):
    """out (m, C) against sum_j F[p, j] T3[p, j, c] (T3 (m, n, C), or (1, n, C) broadcast)."""
    n = F.shape[1]
    ref = np.einsum("pj,pjc->pc", F, np.broadcast_to(T3, (F.shape[0],) + T3.shape[1:]))
    bound = 2 * n * EPS * np.einsum("pj,pjc->pc", np.abs(F), np.abs(np.broadcast_to(T3, (F.shape[0],) + T3.shape[1:])))
    err = np.abs(out - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
    print(label, "max err / bound", worst)
    assert out.shape == ref.shape
    assert np.all(err <= bound), label


@pytest.mark.parametrize("broadcast", [False, True])
def test_shapes(broadcast):
    """Every (n, C, m) of the lists, sp = n C and sp = 0 (one T for all points); derivative orders
    in rotation."""
    from gpk._lib import point_contract
    kind = "Matern52_Cos_1d"
    rng = np.random.default_rng(5)
    kp = rand_kp(rng, 5, 20.0)
    fields = {}
    i = 0
    for n in NS:
        x = np.linspace(0, 1, n) * X_MAX
        for m in MS:
            t = rng.uniform(-0.03, 1.02, size=m) * X_MAX
            for C in CS:
                deriv = i % 3
                i += 1
                if (n, m, deriv) not in fields:
                    fields[(n, m, deriv)] = (t, _field(kind, t, x, kp, deriv))
                tt, F = fields[(n, m, deriv)]
                T3 = rng.normal(size=(1 if broadcast else m, n, C))
                out, _ = point_contract(kind, tt, x, kp, T3, C=C, sp=0 if broadcast else None, deriv=deriv)
                _check(out, F, T3, ("shape", n, C, m, deriv, broadcast))


@pytest.mark.parametrize("Q", [1, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_fields(kind, Q):
    """Every kind and derivative order at Q = 1 and Q = 64, points inside the collocation range,
    outside it and exactly on collocation points (zero distance: the abs'(0) branch)."""
    from gpk._lib import point_contract
    rng = np.random.default_rng(9)
    kp = rand_kp(rng, Q, 20.0)
    n = 65
    x = np.linspace(0, 1, n) * X_MAX
    t = np.concatenate([rng.uniform(0, 1, size=40) * X_MAX, np.array([-0.5, -0.03, 1.02, 1.7]) * X_MAX, x[::3]])
    assert t.size == 66
    for deriv in (0, 1, 2):
        F = _field(kind, t, x, kp, deriv)
        for C in (1, 33):
            T3 = rng.normal(size=(t.size, n, C))
            out, _ = point_contract(kind, t, x, kp, T3, C=C, deriv=deriv)
            _check(out, F, T3, ("field", kind, Q, deriv, C))


@pytest.mark.parametrize("C", [1, 33])
def test_padding_is_not_read(C):
    """T in a padded [m][P][Cp] layout whose rows j >= n and columns c >= C hold NaN."""
    from gpk._lib import point_contract
    rng = np.random.default_rng(3)
    kp = rand_kp(rng, 5, 20.0)
    n, P, Cp, m = 33, 64, 64, 7
    x = np.linspace(0, 1, n) * X_MAX
    t = rng.uniform(-0.03, 1.02, size=m) * X_MAX
    T3 = rng.normal(size=(m, n, C))
    Tp = np.full((m, P, Cp), np.nan)
    Tp[:, :n, :C] = T3
    out, _ = point_contract("SE_Cos_1d", t, x, kp, Tp, C=C, sp=P * Cp, sj=Cp, deriv=2)
    assert np.all(np.isfinite(out))
    _check(out, _field("SE_Cos_1d", t, x, kp, 2), T3, ("padded", C))


def test_limits_and_determinism():
    from gpk._lib import GPKError, point_contract
    rng = np.random.default_rng(4)
    kp = rand_kp(rng, 3, 20.0)
    x = np.linspace(0, 1, 4097) * X_MAX
    t = np.array([0.3, 1.1])
    with pytest.raises(GPKError):   # C > 1 keeps the n field values in LDS: n <= 4096
        point_contract("Matern52_1d", t, x, kp, np.zeros((1, 4097, 2)), C=2, sp=0)
    T3 = rng.normal(size=(1, 4097, 1))
    out, _ = point_contract("Matern52_1d", t, x, kp, T3, C=1, sp=0)   # C = 1 has no such limit
    _check(out, _field("Matern52_1d", t, x, kp, 0), T3, "n = 4097, C = 1")
    for bad in ({"deriv": 3}, {"deriv": -1}, {"sj": 0}, {"sp": -1}):
        with pytest.raises(GPKError):
            point_contract("Matern52_1d", t, x[:8], kp, np.zeros((2, 8, 1)), **bad)
    for C in (1, 33):
        T3 = rng.normal(size=(67, 257, C))
        tt = rng.uniform(0, 1, size=67) * X_MAX
        a, _ = point_contract("Matern52_Cos_1d", tt, x[:257], kp, T3, C=C, deriv=1)
        b, us = point_contract("Matern52_Cos_1d", tt, x[:257], kp, T3, C=C, deriv=1, iters=2)
        assert np.array_equal(a, b)
        assert us is not None and us > 0
