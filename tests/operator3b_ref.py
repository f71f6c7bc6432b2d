"""NumPy restatement of the 3-axis log joint with drift fields (include/gpk.h gpk_drift3 /
gpk_create3_opb; test infrastructure, no test).

tests/operator3m_ref.py loss_grad_3d_opm with, for each axis k whose drift field b_k is given,
    Z_k  = D1_k x_k A_k                      (D1_k the plain order-1 block, no weight)
    R    = [loss_grad_3d_opm's residual] + b_1 . Z_1 + b_3 . Z_3 + b_2 . Z_2     ( . elementwise)
and in the reverse pass
    E_k  = b_k . R,   T_k += D1_k^T x_k E_k  (before X_k = K_k^{-1} x_k T_k),
    G_D1k += v E_k,(k) A_k,(k)^T.
b_k is data: dL/dU has no direct term, and the coefficient fields a_k do not multiply it.  With no
drift field (None, or three Nones) it calls loss_grad_3d_opm itself.  Pinned by
tests/test_operator3b_ref.py against torch autograd of the dense-Kronecker form.
"""
import math

import numpy as np

from oracle import gp_oracle as O
from oracle.gp_oracle import (_lu, _mode_solve, _slogdet_from_lu, _solve, _unfold, mode_product,
                              param_grad_contract)
from tests.operator3_ref import FACES
from tests.operator3c_ref import conv_of
from tests.operator3m_ref import PAIRS, SUM_ORDER, cross_of, loss_grad_3d_opm
from tests.operator3n_ref import face_data
from tests.operator3v_ref import coef_fields
from tests.operator3x_ref import axis_blocks, opx_fields

DRIFT_ORDER = (0, 2, 1)  # R += b_1 Z_1 + b_3 Z_3 + b_2 Z_2


def drift_of(drift, Ns):
    """[b_1, b_2, b_3] as float64 arrays of the grid's shape, None where absent; None is three Nones."""
    if drift is None:
        return [None, None, None]
    assert len(drift) == 3, "drift has three entries"
    out = []
    for b in drift:
        if b is None:
            out.append(None)
            continue
        b = np.asarray(b, np.float64)
        assert b.shape == tuple(Ns), "a drift field has the grid's shape"
        out.append(b)
    return out


def loss_grad_3d_opb(prob, params, op, coef, dfaces=0, dvals=None, conv=None, cross=None, drift=None, terms=None):
    """Negative log joint and gradient; every argument but drift as loss_grad_3d_opm's; drift: three
    entries, each None or an array of the grid's shape."""
    if drift is None or all(b is None for b in drift):
        return loss_grad_3d_opm(prob, params, op, coef, dfaces, dvals, conv, cross, terms=terms)
    mx = cross_of(cross)
    g = conv_of(conv)
    c2, c1, react, faces = opx_fields(op)
    kind = prob["kind"]
    xs = [np.asarray(prob[f"x{a}"], np.float64).reshape(-1) for a in (1, 2, 3)]
    Ns = tuple(x.size for x in xs)
    Nc = Ns[0] * Ns[1] * Ns[2]
    af, rho = coef_fields(coef, Ns)
    bf = drift_of(drift, Ns)
    U = np.asarray(params["U"], np.float64).reshape(Ns)
    kps = [params[f"kernel_paras_{a}"] for a in (1, 2, 3)]
    log_tau, log_v = float(params["log_tau"]), float(params["log_v"])
    tau, v = math.exp(log_tau), math.exp(log_v)
    wb, c = float(prob["llk_weight"]), float(prob["logdet"])
    F = np.asarray(prob["src"], np.float64).reshape(Ns)
    bv = np.asarray(prob["bvals"], np.float64).reshape(-1)
    KD = [axis_blocks(kind, xs[k], kps[k], prob["jitter"], c2[k], c1[k]) for k in range(3)]
    D1 = [O.kernel_block(kind, xs[k], xs[k], kps[k], 1) for k in range(3)]
    lus = [_lu(K) for K, _ in KD]
    A = [_mode_solve(lus[k], U, k) for k in range(3)]
    times = lambda k, T: T if af[k] is None else af[k] * T
    R = sum(times(k, mode_product(KD[k][1], A[k], k)) for k in range(3)) - F
    r1, r2, r3 = react
    if any(react):
        R = R + r1 * U + r2 * U * U + r3 * U * U * U
    if rho is not None:
        R = R + rho * U
    N = np.zeros(Ns)
    for k in range(3):
        if g[k] != 0.0:
            N = N + g[k] * mode_product(D1[k], A[k], k)
    R = R + U * N
    H = [None, None, None]
    for t in SUM_ORDER:
        if mx[t] != 0.0:
            j, k = PAIRS[t]
            H[t] = _mode_solve(lus[k], mode_product(D1[j], A[j], j), k)
            R = R + mx[t] * mode_product(D1[k], H[t], k)
    for k in DRIFT_ORDER:
        if bf[k] is not None:
            R = R + bf[k] * mode_product(D1[k], A[k], k)
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
    hs = face_data(dvals, Ns, dfaces) if dfaces else {}
    dgap, Nd = 0.0, 0
    Z = [np.zeros(Ns) for _ in range(3)]
    Grow = [np.zeros((Ns[k], Ns[k])) for k in range(3)]
    wt = wb * tau
    for f, h in hs.items():
        k, s = divmod(f, 2)
        i_f = Ns[k] - 1 if s else 0
        d = D1[k][i_f]
        r = np.tensordot(d, A[k], axes=(0, k)) - h
        assert np.all(np.isfinite(h)), "dvals of a face in dfaces must be finite"
        dgap += float(np.sum(r * r))
        Nd += r.size
        shape = [1, 1, 1]
        shape[k] = Ns[k]
        Z[k] = Z[k] + d.reshape(shape) * np.expand_dims(r, k)
        other = [a for a in range(3) if a != k]
        Grow[k][i_f] += wt * np.tensordot(A[k], r, axes=(other, [0, 1]))
    log_prior = -0.5 * c * sum(Nc // Ns[k] * lds[k] for k in range(3)) - 0.5 * quad
    log_b = 0.5 * (Nb + Nd) * log_tau - 0.5 * tau * (bgap + dgap)
    eq_ll = 0.5 * Nc * log_v - 0.5 * v * egap
    loss = -(log_prior + log_b * wb + eq_ll)
    if terms is not None:
        terms.update(loss=loss, logdet_1=lds[0], logdet_2=lds[1], logdet_3=lds[2], quad=quad, egap=egap,
                     bgap=bgap, Nb=Nb, dgap=dgap, Nd=Nd, N=N, R=R)
    W = [times(k, R) for k in range(3)]
    Q = U * R
    # the cross terms' reverse pass: per-axis additions to T_j, G_D1 and G_K
    Tx = [np.zeros(Ns) for _ in range(3)]
    GD1x = [np.zeros((Ns[k], Ns[k])) for k in range(3)]
    GKx = [np.zeros((Ns[k], Ns[k])) for k in range(3)]
    for t in range(3):
        if mx[t] == 0.0:
            continue
        j, k = PAIRS[t]
        Zb = _mode_solve(lus[k], mx[t] * mode_product(D1[k].T, R, k), k)
        GD1x[k] += v * mx[t] * (_unfold(R, k) @ _unfold(H[t], k).T)
        GKx[k] += -v * (_unfold(Zb, k) @ _unfold(H[t], k).T)
        GD1x[j] += v * (_unfold(Zb, j) @ _unfold(A[j], j).T)
        Tx[j] = Tx[j] + mode_product(D1[j].T, Zb, j)
    # the drift terms' reverse pass
    for k in range(3):
        if bf[k] is not None:
            E = bf[k] * R
            Tx[k] = Tx[k] + mode_product(D1[k].T, E, k)
            GD1x[k] += v * (_unfold(E, k) @ _unfold(A[k], k).T)
    X = []
    for k in range(3):
        T = mode_product(KD[k][1].T, W[k], k) + (wt / v) * Z[k]
        if g[k] != 0.0:
            T = T + g[k] * mode_product(D1[k].T, Q, k)
        T = T + Tx[k]
        X.append(_mode_solve(lus[k], T, k))
    gU = S + v * sum(X)
    if any(react):
        gU = gU + v * (r1 + 2.0 * r2 * U + 3.0 * r3 * U * U) * R
    if rho is not None:
        gU = gU + v * rho * R
    gU = gU + v * N * R
    gU = gU + wt * scatter
    grad = {"U": gU, "log_tau": wb * (-0.5 * (Nb + Nd) + 0.5 * tau * (bgap + dgap)),
            "log_v": -0.5 * Nc + 0.5 * v * egap}
    for k in range(3):
        Kinv = _solve(lus[k], np.eye(Ns[k]))
        Ak = _unfold(A[k], k)
        GK = 0.5 * c * (Nc // Ns[k]) * Kinv - _unfold(0.5 * S + v * X[k], k) @ Ak.T + GKx[k]
        GD = v * (_unfold(W[k], k) @ Ak.T)
        GD1 = v * g[k] * (_unfold(Q, k) @ Ak.T) + GD1x[k]
        g2 = param_grad_contract(kind, xs[k], kps[k], GK, c2[k] * GD, 2)
        g1 = param_grad_contract(kind, xs[k], kps[k], np.zeros_like(GK), c1[k] * GD + GD1 + Grow[k], 1)
        grad[f"kernel_paras_{k + 1}"] = {key: np.asarray(g2[key]) + np.asarray(g1[key]) for key in g2}
    return loss, grad


def criterion_3d_opb(prob, params, op, coef, dfaces=0, dvals=None, conv=None, cross=None, drift=None):
    """(boundary_gap + dgap) / (Nb + Nd) + eq_gap / Nc."""
    t = {}
    loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift, terms=t)
    return (t["bgap"] + t.get("dgap", 0.0)) / (t["Nb"] + t.get("Nd", 0)) + t["egap"] / np.asarray(params["U"]).size


def adam_replay_b(prob, params, op, coef, dfaces, dvals, conv, cross, drift, nsteps, lr=0.01, after=None):
    """tests/operator3_ref.py adam_replay on loss_grad_3d_opb."""
    opt = O.Adam(lr)
    st = opt.init(params)
    p, losses = params, []
    for i in range(nsteps):
        lo, go = loss_grad_3d_opb(prob, p, op, coef, dfaces, dvals, conv, cross, drift)
        losses.append(lo)
        p, st = opt.update(go, st, p)
        if after is not None:
            after(i, p)
    return losses, p
