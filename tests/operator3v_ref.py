"""NumPy restatement of the 3-axis log joint for an operator with coefficient fields
(include/gpk.h gpk_coef3 / gpk_create3_opv; test infrastructure, no test).

tests/operator3x_ref.py loss_grad_3d_opx with a field a_k on each axis's term and a field rho on
the linear reaction term (each None: a_k = 1, rho = 0), . elementwise:
    T_k = D_k x_k A_k,   D_k = c2_k DD_k + c1_k D1_k,   A_k = K_k^{-1} x_k U,
    R   = a_1 . T_1 + a_3 . T_3 + a_2 . T_2 - F + (r1 + rho) . U + r2 U^2 + r3 U^3,
    W_k = a_k . R,   X_k = K_k^{-1} x_k (D_k^T x_k W_k),
    dL/dU = S + v sum_k X_k + v (r1 + rho + 2 r2 U + 3 r3 U^2) . R + w tau scatter_active(u_b - b),
    G_Kk = c/2 (N / N_k) K_k^{-1} - (S/2 + v X_k)_(k) A_k,(k)^T,   G_Dk = v (W_k)_(k) A_k,(k)^T,
and the kernel-parameter gradient of axis k as in loss_grad_3d_opx.  With coef all None every
expression below is loss_grad_3d_opx's own, operation for operation.  Pinned by
tests/test_operator3v_ref.py against loss_grad_3d_opx (no fields, constant fields) and against
torch autograd of the dense-Kronecker form (fields that vary).
"""
import math

import numpy as np

from oracle import gp_oracle as O
from oracle.gp_oracle import (_lu, _mode_solve, _slogdet_from_lu, _solve, _unfold, mode_product,
                              param_grad_contract)
from tests.operator3_ref import FACES
from tests.operator3x_ref import axis_blocks, opx_fields


def coef_fields(coef, Ns):
    """([a1, a2, a3], rho) as float64 arrays of shape Ns or None, from None, a dict with 'a' and
    'rho', or any object with those attributes."""
    if coef is None:
        return [None, None, None], None
    get = coef.get if isinstance(coef, dict) else lambda k, d=None: getattr(coef, k, d)
    a = get("a", None) or (None, None, None)
    arr = lambda f: None if f is None else np.asarray(f, np.float64).reshape(Ns)
    return [arr(f) for f in a], arr(get("rho", None))


def loss_grad_3d_opv(prob, params, op, coef, terms=None):
    """Negative log joint and gradient; prob, params, op and terms as loss_grad_3d_opx's."""
    c2, c1, react, faces = opx_fields(op)
    kind = prob["kind"]
    xs = [np.asarray(prob[f"x{a}"], np.float64).reshape(-1) for a in (1, 2, 3)]
    Ns = tuple(x.size for x in xs)
    Nc = Ns[0] * Ns[1] * Ns[2]
    af, rho = coef_fields(coef, Ns)
    U = np.asarray(params["U"], np.float64).reshape(Ns)
    kps = [params[f"kernel_paras_{a}"] for a in (1, 2, 3)]
    log_tau, log_v = float(params["log_tau"]), float(params["log_v"])
    tau, v = math.exp(log_tau), math.exp(log_v)
    wb, c = float(prob["llk_weight"]), float(prob["logdet"])
    F = np.asarray(prob["src"], np.float64).reshape(Ns)
    bv = np.asarray(prob["bvals"], np.float64).reshape(-1)
    KD = [axis_blocks(kind, xs[k], kps[k], prob["jitter"], c2[k], c1[k]) for k in range(3)]
    lus = [_lu(K) for K, _ in KD]
    A = [_mode_solve(lus[k], U, k) for k in range(3)]
    times = lambda k, T: T if af[k] is None else af[k] * T
    R = sum(times(k, mode_product(KD[k][1], A[k], k)) for k in range(3)) - F
    r1, r2, r3 = react
    if any(react):
        R = R + r1 * U + r2 * U * U + r3 * U * U * U
    if rho is not None:
        R = R + rho * U
    egap = float(np.sum(R * R))
    S = _mode_solve(lus[2], _mode_solve(lus[1], A[0], 1), 2)
    quad = float(np.sum(U * S))
    lds = [_slogdet_from_lu(f) for f in lus]
    bgap, Nb, o = 0.0, 0, 0
    scatter = np.zeros(Ns)
    for f, sl in enumerate(FACES):
        n = U[sl].size
        if (faces >> f) & 1:
            res = U[sl] - bv[o:o + n].reshape(U[sl].shape)
            bgap += float(np.sum(res * res))
            scatter[sl] += res
            Nb += n
        o += n
    assert o == bv.size, "bvals must have the six-face layout"
    log_prior = -0.5 * c * sum(Nc // Ns[k] * lds[k] for k in range(3)) - 0.5 * quad
    log_b = 0.5 * Nb * log_tau - 0.5 * tau * bgap
    eq_ll = 0.5 * Nc * log_v - 0.5 * v * egap
    loss = -(log_prior + log_b * wb + eq_ll)
    if terms is not None:
        terms.update(loss=loss, logdet_1=lds[0], logdet_2=lds[1], logdet_3=lds[2], quad=quad, egap=egap,
                     bgap=bgap, Nb=Nb)
    W = [times(k, R) for k in range(3)]
    X = [_mode_solve(lus[k], mode_product(KD[k][1].T, W[k], k), k) for k in range(3)]
    gU = S + v * sum(X)
    if any(react):
        gU = gU + v * (r1 + 2.0 * r2 * U + 3.0 * r3 * U * U) * R
    if rho is not None:
        gU = gU + v * rho * R
    gU = gU + wb * tau * scatter
    grad = {"U": gU, "log_tau": wb * (-0.5 * Nb + 0.5 * tau * bgap), "log_v": -0.5 * Nc + 0.5 * v * egap}
    for k in range(3):
        Kinv = _solve(lus[k], np.eye(Ns[k]))
        Ak = _unfold(A[k], k)
        GK = 0.5 * c * (Nc // Ns[k]) * Kinv - _unfold(0.5 * S + v * X[k], k) @ Ak.T
        GD = v * (_unfold(W[k], k) @ Ak.T)
        g2 = param_grad_contract(kind, xs[k], kps[k], GK, c2[k] * GD, 2)
        g1 = param_grad_contract(kind, xs[k], kps[k], np.zeros_like(GK), c1[k] * GD, 1)
        grad[f"kernel_paras_{k + 1}"] = {key: np.asarray(g2[key]) + np.asarray(g1[key]) for key in g2}
    return loss, grad


def criterion_3d_opv(prob, params, op, coef):
    """boundary_gap / Nb + eq_gap / Nc with the mask's Nb."""
    t = {}
    loss_grad_3d_opv(prob, params, op, coef, terms=t)
    return t["bgap"] / t["Nb"] + t["egap"] / np.asarray(params["U"]).size


def adam_replay_v(prob, params, op, coef, nsteps, lr=0.01, after=None):
    """tests/operator3_ref.py adam_replay on loss_grad_3d_opv."""
    opt = O.Adam(lr)
    st = opt.init(params)
    p, losses = params, []
    for i in range(nsteps):
        lo, go = loss_grad_3d_opv(prob, p, op, coef)
        losses.append(lo)
        p, st = opt.update(go, st, p)
        if after is not None:
            after(i, p)
    return losses, p
