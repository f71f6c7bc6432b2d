"""NumPy restatement of the 3-axis log joint for an operator with a second- and a first-order
term per axis (include/gpk.h gpk_operator3x; test infrastructure, no test).

tests/operator3_ref.py loss_grad_3d_op with the axis block
    D_k = c2_k DD_k + c1_k D1_k,   DD_k = kernel_kd(.., 2)[1],  D1_k = kernel_kd(.., 1)[1],
the weights inside the block and no further factor on the axis:
    R = sum_k D_k x_k A_k - F + r1 U + r2 U^2 + r3 U^3,   A_k = K_k^{-1} x_k U,
    X_k = K_k^{-1} x_k (D_k^T x_k R),
    dL/dU = S + v sum_k X_k + v (r1 + 2 r2 U + 3 r3 U^2) R + w tau scatter_active(u_b - b),
    G_Kk = c/2 (N / N_k) K_k^{-1} - (S/2 + v X_k)_(k) A_k,(k)^T,   G_Dk = v R_(k) A_k,(k)^T,
and the kernel-parameter gradient of axis k as the sum of two contractions, one per field:
    param_grad_contract(G_Kk, c2_k G_Dk, order 2) + param_grad_contract(0, c1_k G_Dk, order 1).
Pinned by tests/test_operator3x_ref.py against loss_grad_3d_op (one order per axis) and against
torch autograd of the dense-Kronecker form (mixed axes).
"""
import math

import numpy as np

from oracle import gp_oracle as O
from oracle.gp_oracle import (_lu, _mode_solve, _slogdet_from_lu, _solve, _unfold, kernel_kd, mode_product,
                              param_grad_contract)
from tests.operator3_ref import FACES


def opx_fields(op):
    """(c2, c1, react, faces) of a dict or of any object with those attributes."""
    get = op.get if isinstance(op, dict) else lambda k, d=None: getattr(op, k, d)
    react = get("react", None)
    faces = get("faces", None)
    return (tuple(float(c) for c in get("c2")), tuple(float(c) for c in get("c1")),
            (0.0, 0.0, 0.0) if react is None else tuple(float(r) for r in react), 63 if faces is None else int(faces))


def as_op(op):
    """The gpk_operator3 form (a dict) of an operator with at most one non-zero weight per axis:
    that order with that weight; both zero: order 2 with weight 0."""
    c2, c1, react, faces = opx_fields(op)
    assert not any(a != 0.0 and b != 0.0 for a, b in zip(c2, c1)), "a mixed axis has no gpk_operator3 form"
    order = tuple(1 if (b != 0.0 and a == 0.0) else 2 for a, b in zip(c2, c1))
    return dict(order=order, coef=tuple(b if o == 1 else a for o, a, b in zip(order, c2, c1)), react=react, faces=faces)


def axis_blocks(kind, x, kp, jitter, c2, c1):
    """(K, D) of one axis: D = c2 DD + c1 D1, a zero weight's field left out."""
    K, D = kernel_kd(kind, x, kp, jitter, 2)
    D = c2 * D if c2 != 0.0 else np.zeros_like(K)
    if c1 != 0.0:
        D = D + c1 * kernel_kd(kind, x, kp, jitter, 1)[1]
    return K, D


def loss_grad_3d_opx(prob, params, op, terms=None):
    """Negative log joint and gradient; prob, params and terms as loss_grad_3d_op's."""
    c2, c1, react, faces = opx_fields(op)
    kind = prob["kind"]
    xs = [np.asarray(prob[f"x{a}"], np.float64).reshape(-1) for a in (1, 2, 3)]
    Ns = tuple(x.size for x in xs)
    Nc = Ns[0] * Ns[1] * Ns[2]
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
    R = sum(mode_product(KD[k][1], A[k], k) for k in range(3)) - F
    r1, r2, r3 = react
    if any(react):
        R = R + r1 * U + r2 * U * U + r3 * U * U * U
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
    X = [_mode_solve(lus[k], mode_product(KD[k][1].T, R, k), k) for k in range(3)]
    gU = S + v * sum(X)
    if any(react):
        gU = gU + v * (r1 + 2.0 * r2 * U + 3.0 * r3 * U * U) * R
    gU = gU + wb * tau * scatter
    grad = {"U": gU, "log_tau": wb * (-0.5 * Nb + 0.5 * tau * bgap), "log_v": -0.5 * Nc + 0.5 * v * egap}
    for k in range(3):
        Kinv = _solve(lus[k], np.eye(Ns[k]))
        Ak = _unfold(A[k], k)
        GK = 0.5 * c * (Nc // Ns[k]) * Kinv - _unfold(0.5 * S + v * X[k], k) @ Ak.T
        GD = v * (_unfold(R, k) @ Ak.T)
        g2 = param_grad_contract(kind, xs[k], kps[k], GK, c2[k] * GD, 2)
        g1 = param_grad_contract(kind, xs[k], kps[k], np.zeros_like(GK), c1[k] * GD, 1)
        grad[f"kernel_paras_{k + 1}"] = {key: np.asarray(g2[key]) + np.asarray(g1[key]) for key in g2}
    return loss, grad


def criterion_3d_opx(prob, params, op):
    """boundary_gap / Nb + eq_gap / Nc with the mask's Nb."""
    t = {}
    loss_grad_3d_opx(prob, params, op, terms=t)
    return t["bgap"] / t["Nb"] + t["egap"] / np.asarray(params["U"]).size


def adam_replay_x(prob, params, op, nsteps, lr=0.01, after=None):
    """tests/operator3_ref.py adam_replay on loss_grad_3d_opx."""
    opt = O.Adam(lr)
    st = opt.init(params)
    p, losses = params, []
    for i in range(nsteps):
        lo, go = loss_grad_3d_opx(prob, p, op)
        losses.append(lo)
        p, st = opt.update(go, st, p)
        if after is not None:
            after(i, p)
    return losses, p
