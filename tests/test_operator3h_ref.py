"""Pins tests/operator3h_ref.py (the yardstick of the high-order handles' GPU tests) before anything
on the device relies on it: the order-3 and order-4 fields against 50-digit differentiation of kappa
(tests/mp_fields_high.py), loss_grad_3d_oph without high-order weights against loss_grad_3d_opb, and
the loss and full gradient against torch autograd of the dense-Kronecker log joint whose blocks come
from nested autograd of kappa itself."""
import mpmath as mp
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import autograd_ref as AR
from tests import mp_fields_high as MH
from tests.mp_fields import mp_of
from tests.operator3_ref import FACES
from tests.operator3b_ref import adam_replay_b, criterion_3d_opb, loss_grad_3d_opb
from tests.operator3h_ref import (adam_replay_h, criterion_3d_oph, kernel_block_n, kernel_kd_high, loss_grad_3d_oph,
                                  param_grad_contract_high)
from tests.operator3m_ref import PAIRS
from tests.operator3n_ref import face_data
from tests.test_operator3b_ref import DRIFT_CASES, NS, _setup, drift_fields_for
from tests.test_operator3c_ref import _tol
from tests.test_operator3x_ref import _blocks

KINDS = ["SE_Cos_1d", "Matern52_Cos_1d", "SE_1d", "Matern52_1d"]
EPS = 2.0 ** -52


# ---- 1. the fields against differentiation of kappa ------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [3, 4])
def test_high_fields_vs_differentiation_of_kappa(kind, n):
    """kernel_block_n at ~40 pairs (d = 0, the smallest and the largest distance among them) of a
    rectangular block, Q = 5 components with frequencies up to 5 and a in [0.3, 3]: the long-double
    evaluation within 0.1 units of eps B_n (as tests/test_oracle.py holds the order-0..2 yardstick; the
    Matern kinds within 0.1 + n / 2: the closed forms write sqrt5^2 as 5, and with the fp64 SQRT5, off
    by up to 2^-53 relative, a monomial carrying sqrt5^n differs from the derivative of the function
    written with SQRT5 throughout by up to n / 2 eps),
    the fp64 evaluation within N_n units plus the rounding of its two arguments, 2 (|om d| + r)
    relative (fp64 NumPy carries no low part of the phase or the radial argument)."""
    rng = np.random.default_rng(31 + n)
    Q = 5
    kp = {"log-w": np.log(rng.uniform(0.2, 1.0, Q)), "log-ls": np.log(rng.uniform(0.3, 3.0, Q)),
          "freq": rng.uniform(0.0, 5.0, Q)}
    x1 = np.sort(rng.uniform(0.0, 2.0, 9))
    x2 = np.sort(rng.uniform(0.0, 2.0, 7))
    x2[2] = x1[4]          # d = 0 off the block's diagonal
    x2[0], x1[8] = 0.0, 2.0  # the extent
    x2[5] = x1[1] + 1e-9   # a tiny distance, negative difference
    D64 = kernel_block_n(kind, x1, x2, kp, n)
    Dld = kernel_block_n(kind, x1, x2, kp, n, np.longdouble)
    B = MH.block_scale(kind, n, x1, x2, kp)
    bar64 = MH.N_3 if n == 3 else MH.N_4
    k = O._kind_id(kind)
    amax = float(np.exp(kp["log-ls"]).max())
    bar_ld = 0.1 + (n / 2.0 if O._is_matern(k) else 0.0)
    worst_ld = worst_64 = 0.0
    for i in range(9):
        for j in range(0, 7, 1 if i in (1, 4, 8) else 2):
            De, b = MH.block_entry(kind, n, x1[i], x2[j], kp)
            assert abs(b - B[i, j]) <= 1e-12 * b
            d = abs(x1[i] - x2[j])
            if b == 0.0:
                assert De == 0 and D64[i, j] == 0.0 and Dld[i, j] == 0.0
                continue
            e_ld = abs(float(mp_of(Dld[i, j]) - De)) / (EPS * b)
            e_64 = abs(float(mp.mpf(float(D64[i, j])) - De)) / (EPS * b)
            arg = 2.0 * ((O.TWO_PI * 5.0 * d if O._has_cos(k) else 0.0)
                         + (O.SQRT5 * amax * d if O._is_matern(k) else amax * d * d))
            worst_ld, worst_64 = max(worst_ld, e_ld), max(worst_64, e_64)
            assert e_ld <= bar_ld, (kind, n, i, j, e_ld)
            assert e_64 <= bar64 + bar_ld + arg, (kind, n, i, j, e_64, bar64 + bar_ld + arg)
    print(kind, "order", n, "worst long double %.3g, fp64 %.3g units" % (worst_ld, worst_64))
    assert worst_ld > 0.0 or not O._has_cos(k)
    # signs: order 3 carries s_ij (s = +1 at 0, where the field is exactly 0), order 4 is symmetric
    x = np.sort(rng.uniform(0.0, 2.0, 8))
    D4, D3 = kernel_kd_high(kind, x, kp)
    assert np.array_equal(D4, D4.T) and np.array_equal(D3, -D3.T) and np.all(np.diag(D3) == 0.0)
    assert np.abs(D3).max() > 0.0 and np.abs(np.diag(D4)).min() > 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_high_contraction_vs_finite_differences_of_the_blocks(kind):
    """param_grad_contract_high against central differences of sum G4 . D4 + G3 . D3 in every kernel
    parameter (long double blocks, h = 1e-6: truncation ~1e-12 relative, rounding ~1e-13)."""
    rng = np.random.default_rng(3)
    Q = 3
    kp = {"log-w": np.log(rng.uniform(0.2, 1.0, Q)), "log-ls": np.log(rng.uniform(0.5, 2.0, Q)),
          "freq": rng.uniform(0.2, 2.0, Q)}
    x = np.sort(rng.uniform(0.0, 1.5, 6))
    G4, G3 = rng.normal(size=(6, 6)), rng.normal(size=(6, 6))
    got = param_grad_contract_high(kind, x, kp, G4, G3)

    def f(p):
        D4, D3 = kernel_kd_high(kind, x, p, np.longdouble)
        return np.sum(G4 * D4) + np.sum(G3 * D3)
    h = 1e-6
    for key in ("freq", "log-ls", "log-w"):
        for c in range(Q):
            up, dn = {k: v.copy() for k, v in kp.items()}, {k: v.copy() for k, v in kp.items()}
            up[key][c] += h
            dn[key][c] -= h
            fd = float((f(up) - f(dn)) / (2 * h))
            scale = max(abs(fd), float(np.abs(got[key]).max()), 1e-300)
            assert abs(got[key][c] - fd) <= 1e-8 * scale, (kind, key, c, got[key][c], fd)
    if not O._has_cos(O._kind_id(kind)):
        assert np.all(got["freq"] == 0.0)


# ---- 2. no high-order weight: loss_grad_3d_opb itself ---------------------------------------------
@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which,dfaces,conv,cross,axes", DRIFT_CASES[:1] + DRIFT_CASES[3:])
def test_zero_high_weights_is_loss_grad_3d_opb_exactly(op, which, dfaces, conv, cross, axes, kind):
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    drift = drift_fields_for(NS, axes)
    tb, th = {}, {}
    lo, go = loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift, terms=tb)
    for high in (None, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))):
        th.clear()
        l, g = loss_grad_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, terms=th)
        assert l == lo and set(th) == set(tb)
        assert all(np.array_equal(th[k], tb[k]) for k in tb)
        for k in go:
            assert np.array_equal(O.flatten_params(g[k]), O.flatten_params(go[k])), k
    assert (criterion_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift)
            == criterion_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift))
    (la, pa), (lb, pb) = (adam_replay_h(prob, params, op, coef, dfaces, dvals, conv, cross, drift, None, 2),
                          adam_replay_b(prob, params, op, coef, dfaces, dvals, conv, cross, drift, 2))
    assert la == lb and np.array_equal(O.flatten_params(pa), O.flatten_params(pb))


# ---- 3. torch autograd of the dense-Kronecker form ------------------------------------------------
def mats4(kind, x, p, jitter):
    """(K, [D1, D2, D3, D4]) by nested autograd of kappa in its first argument (tests/autograd_ref.py
    mats, two orders further)."""
    n = x.numel()
    X1 = x.reshape(-1, 1).expand(n, n).reshape(-1).clone().requires_grad_(True)
    X2 = x.reshape(1, -1).expand(n, n).reshape(-1)
    k = AR.kappa(kind, X1, X2, p)
    K = k.reshape(n, n) + jitter * torch.eye(n)
    Ds, g = [], k
    for _ in range(4):
        g, = torch.autograd.grad(g.sum(), X1, create_graph=True)
        Ds.append(g.reshape(n, n))
    return K, Ds


def dense_loss_grad_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high):
    """tests/test_operator3b_ref.py dense_loss_grad_3d_opb with D_k = c4 D4 + c3 D3 + c2 DD + c1 D1, every
    block by nested autograd of kappa."""
    c4, c3 = high
    tp = AR._tp(params)
    kind = prob["kind"]
    xs = [torch.tensor(prob[f"x{a}"]) for a in (1, 2, 3)]
    Ks, Ds, D1s = [], [], []
    for k in range(3):
        K, (D1, D2, D3, D4) = mats4(kind, xs[k], tp[f"kernel_paras_{k + 1}"], prob["jitter"])
        Ks.append(K)
        D1s.append(D1)
        Ds.append(c4[k] * D4 + c3[k] * D3 + op["c2"][k] * D2 + op["c1"][k] * D1)
    K1, K2, K3 = Ks
    U = tp["U"]
    u = U.reshape(-1)
    fld = lambda f: torch.ones_like(u) if f is None else torch.tensor(np.asarray(f, np.float64).reshape(-1))
    a = [fld(f) for f in coef["a"]]
    K = torch.kron(K1, torch.kron(K2, K3))
    Kinv_u = torch.linalg.solve(K, u)
    on_axis = lambda k, M: torch.kron(M if k == 0 else K1, torch.kron(M if k == 1 else K2, M if k == 2 else K3))
    L = sum(a[k] * (on_axis(k, Ds[k]) @ Kinv_u) for k in range(3))
    r1, r2, r3 = op["react"]
    R = L - torch.tensor(prob["src"]).reshape(-1) + r1 * u + r2 * u ** 2 + r3 * u ** 3
    if coef["rho"] is not None:
        R = R + fld(coef["rho"]) * u
    for k in range(3):
        if conv[k] != 0.0:
            R = R + u * (conv[k] * (on_axis(k, D1s[k]) @ Kinv_u))
    for (j, k), m in zip(PAIRS, cross):
        if m != 0.0:
            f = [D1s[i] if i in (j, k) else Ks[i] for i in range(3)]
            R = R + m * (torch.kron(f[0], torch.kron(f[1], f[2])) @ Kinv_u)
    for k in range(3):
        if drift[k] is not None:
            R = R + fld(drift[k]) * (on_axis(k, D1s[k]) @ Kinv_u)
    egap = (R ** 2).sum()
    bv = torch.tensor(np.nan_to_num(np.asarray(prob["bvals"], np.float64), nan=0.0))
    bgap, Nb, o = 0.0, 0, 0
    for f, sl in enumerate(FACES):
        n = U[sl].numel()
        if (op["faces"] >> f) & 1:
            bgap = bgap + ((U[sl].reshape(-1) - bv[o:o + n]) ** 2).sum()
            Nb += n
        o += n
    ns = tuple(U.shape)
    for f, h in (face_data(dvals, ns, dfaces) if dfaces else {}).items():
        k, s = divmod(f, 2)
        Ak = torch.linalg.solve(Ks[k], torch.movedim(U, k, 0).reshape(ns[k], -1))
        g = D1s[k][ns[k] - 1 if s else 0] @ Ak
        bgap = bgap + ((g - torch.tensor(h).reshape(-1)) ** 2).sum()
        Nb += g.numel()
    log_prior = -0.5 * torch.linalg.slogdet(K)[1] * prob["logdet"] - 0.5 * (u * Kinv_u).sum()
    log_b = 0.5 * Nb * tp["log_tau"] - 0.5 * torch.exp(tp["log_tau"]) * bgap
    eq_ll = 0.5 * u.numel() * tp["log_v"] - 0.5 * torch.exp(tp["log_v"]) * egap
    loss = -(log_prior + log_b * prob["llk_weight"] + eq_ll)
    loss.backward()
    return float(loss.detach()), AR._grads(tp)


PLAIN = dict(c2=(0.0, 0.7, -0.2), c1=(0.0, 0.0, 1.0), react=(0.0, 0.0, 0.0), faces=63)
ZERO3 = (0.0, 0.0, 0.0)
NONE3 = (None, None, None)
# one case per kind: a pure high axis (c2 = c1 = 0) with both orders; both orders next to c2, c1 in
# another position; a fourth-order term alone on the last axis; a third-order term alone
KIND_CASES = [
    ("SE_Cos_1d", PLAIN, ((0.05, 0.0, 0.0), (-0.2, 0.0, 0.0))),
    ("Matern52_Cos_1d", dict(PLAIN, c2=(-0.3, 0.7, -0.2), c1=(0.8, 0.4, 1.0)), ((0.0, 0.03, 0.0), (0.0, 0.1, 0.0))),
    ("SE_1d", PLAIN, ((0.0, 0.0, -0.04), ZERO3)),
    ("Matern52_1d", PLAIN, (ZERO3, (1.5, 0.0, 0.0))),
]


@pytest.mark.parametrize("kind,op,high", KIND_CASES)
def test_high_terms_vs_dense_kronecker_autograd_every_kind(kind, op, high):
    """(5, 4, 3) grid; the blocks of the dense form come from nested autograd of kappa."""
    from tests.helpers import problem_3d
    from tests.test_operator3x_ref import _mask
    ns = (5, 4, 3)
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=ns, Q=2, seed=11)
    prob = _mask(prob, ns, op["faces"])
    coef = dict(a=NONE3, rho=None)
    l, g = loss_grad_3d_oph(prob, params, op, coef, 0, None, None, None, None, high)
    la, ga = dense_loss_grad_3d_oph(prob, params, op, coef, 0, None, ZERO3, ZERO3, NONE3, high)
    errs = _blocks(g, ga)
    print("oph vs autograd", kind, high, abs(l - la) / abs(la), errs)
    assert np.isfinite(l) and all(np.all(np.isfinite(O.flatten_params(g[k]))) for k in g)
    assert abs(loss_grad_3d_opb(prob, params, op, coef)[0] - l) > 1e-6 * abs(l)  # the terms matter
    tol = _tol(prob, params)
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_Cos_1d"])
def test_all_four_orders_convective_and_drift_on_the_same_axis(kind):
    """c4, c3, c2, c1, a convective weight and a drift field all on axis 1 (which also has the field
    a_1, a derivative face and the pairs (1,2), (1,3)): DRIFT_CASES' last case plus high-order weights
    on every axis."""
    op, which, dfaces, conv, cross, axes = DRIFT_CASES[3]
    assert op["c2"][0] != 0.0 and op["c1"][0] != 0.0 and conv[0] != 0.0 and 0 in axes
    high = ((0.04, 0.0, -0.02), (-0.15, 0.1, 0.0))
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    drift = drift_fields_for(NS, axes)
    l, g = loss_grad_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high)
    la, ga = dense_loss_grad_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high)
    errs = _blocks(g, ga)
    print("oph everything vs autograd", kind, abs(l - la) / abs(la), errs)
    assert abs(loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift)[0] - l) > 1e-6 * abs(l)
    tol = _tol(prob, params)
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)
