"""NumPy restatement of the 3-axis log joint for a stated operator (include/gpk.h gpk_operator3;
test infrastructure, no test).

oracle/gp_oracle.py loss_grad_3d with one derivative order o_k and one weight c_k per axis, the
reaction polynomial r1 U + r2 U^2 + r3 U^3 and a face mask:
    R = sum_k c_k D_k^(o_k) x_k A_k - F + r1 U + r2 U^2 + r3 U^3,   A_k = K_k^{-1} x_k U,
    X_k = K_k^{-1} x_k (D_k^T x_k R),
    dL/dU = S + v sum_k c_k X_k + v (r1 + 2 r2 U + 3 r3 U^2) R + w tau scatter_active(u_b - b),
    G_Kk = c/2 (N / N_k) K_k^{-1} - (S/2 + v c_k X_k)_(k) A_k,(k)^T,   G_Dk = v c_k R_(k) A_k,(k)^T,
boundary_gap and Nb over the active faces only (an edge of two active faces counts twice).  Built
from the oracle's own pieces (kernel_kd, LU solves, mode products, param_grad_contract); pinned
against the oracle and against torch autograd of the dense-Kronecker form by
tests/test_operator3_ref.py.
"""
import math

import numpy as np

from oracle import gp_oracle as O
from oracle.gp_oracle import (_lu, _mode_solve, _slogdet_from_lu, _solve, _unfold, kernel_kd, mode_product,
                              param_grad_contract)

# the six faces in bvals order (bit f of the mask): index tuples into U
FACES = ((0,), (-1,), (slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0),
         (slice(None), slice(None), -1))
POISSON_OP = dict(order=(2, 2, 2), coef=(1.0, 1.0, 1.0), react=(0.0, 0.0, 0.0), faces=63)


def op_fields(op):
    """(order, coef, react, faces) of a dict or of any object with those attributes."""
    get = op.get if isinstance(op, dict) else lambda k, d=None: getattr(op, k, d)
    react = get("react", None)
    faces = get("faces", None)
    return (tuple(int(o) for o in get("order")), tuple(float(c) for c in get("coef")),
            (0.0, 0.0, 0.0) if react is None else tuple(float(r) for r in react), 63 if faces is None else int(faces))


def face_count(shape, faces):
    """Nb: the entries of the active faces."""
    return sum(int(np.zeros(shape)[sl].size) for f, sl in enumerate(FACES) if (faces >> f) & 1)


def loss_grad_3d_op(prob, params, op, terms=None):
    """Negative log joint and gradient.  prob as oracle loss_grad_3d's (its 'eq' is not read);
    prob['bvals'] has the six-face layout whatever the mask -- entries of open faces are never
    read.  terms: a dict that receives loss, logdet_1..3, quad, egap, bgap, Nb."""
    order, coef, react, faces = op_fields(op)
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
    KD = [kernel_kd(kind, xs[k], kps[k], prob["jitter"], order[k]) for k in range(3)]
    lus = [_lu(K) for K, _ in KD]
    A = [_mode_solve(lus[k], U, k) for k in range(3)]
    R = sum(coef[k] * mode_product(KD[k][1], A[k], k) for k in range(3)) - F
    r1, r2, r3 = react
    if any(react):
        R = R + r1 * U + r2 * U * U + r3 * U * U * U
    egap = float(np.sum(R * R))
    S = _mode_solve(lus[2], _mode_solve(lus[1], A[0], 1), 2)
    quad = float(np.sum(U * S))
    lds = [_slogdet_from_lu(f) for f in lus]
    # boundary: the six face slices under the mask
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
    gU = S + v * sum(coef[k] * X[k] for k in range(3))
    if any(react):
        gU = gU + v * (r1 + 2.0 * r2 * U + 3.0 * r3 * U * U) * R
    gU = gU + wb * tau * scatter
    grad = {"U": gU, "log_tau": wb * (-0.5 * Nb + 0.5 * tau * bgap), "log_v": -0.5 * Nc + 0.5 * v * egap}
    for k in range(3):
        Kinv = _solve(lus[k], np.eye(Ns[k]))
        Ak = _unfold(A[k], k)
        GK = 0.5 * c * (Nc // Ns[k]) * Kinv - _unfold(0.5 * S + v * coef[k] * X[k], k) @ Ak.T
        GD = v * coef[k] * (_unfold(R, k) @ Ak.T)
        grad[f"kernel_paras_{k + 1}"] = param_grad_contract(kind, xs[k], kps[k], GK, GD, order[k])
    return loss, grad


def criterion_3d_op(prob, params, op):
    """boundary_gap / Nb + eq_gap / Nc with the mask's Nb."""
    t = {}
    loss_grad_3d_op(prob, params, op, terms=t)
    return t["bgap"] / t["Nb"] + t["egap"] / np.asarray(params["U"]).size


def adam_replay(prob, params, op, nsteps, lr=0.01, after=None):
    """nsteps of optax.adam on the log joint: (losses before each update, final params).
    after(step, params): called with the params after each update (train-loop records)."""
    opt = O.Adam(lr)
    st = opt.init(params)
    p, losses = params, []
    for i in range(nsteps):
        lo, go = loss_grad_3d_op(prob, p, op)
        losses.append(lo)
        p, st = opt.update(go, st, p)
        if after is not None:
            after(i, p)
    return losses, p
