"""NumPy restatement of the 3-axis log joint with third- and fourth-order terms (include/gpk.h
gpk_high3 / gpk_create3_oph; test infrastructure, no test).

tests/operator3b_ref.py loss_grad_3d_opb with the axis block
    D_k = c4_k D4_k + c3_k D3_k + c2_k DD_k + c1_k D1_k,
Dn_k[i][j] the n-th derivative in the first argument of kappa_k at (x_i, x_j): per mixture
component w sum_m C(n, m) m_m(d) c_{n-m}(d), d = |x_i - x_j|, the odd orders times the sign s_ij of
x_i - x_j (s = +1 at 0, oracle/gp_oracle.py _pairs).  Everything else is loss_grad_3d_opb's: the
coefficient field a_k multiplies the whole block's term; convective terms, cross pairs, drift terms
and derivative faces use the plain order-1 block; the kernel-parameter gradient of axis k gains
    param_grad_contract_high(c4_k G_Dk, c3_k G_Dk).
With no high-order weight (None, or six zeros) it calls loss_grad_3d_opb itself.  Pinned by
tests/test_operator3h_ref.py against 50-digit differentiation of kappa and against torch autograd of
the dense-Kronecker form.

dtype: the field functions take np.float64 or np.longdouble (the inputs and the constants SQRT5 and
TWO_PI stay the fp64 values; everything after them in that type), which is how the GPU test module
measures the fp64 yardstick's own rounding.
"""
import math

import numpy as np

from oracle import gp_oracle as O
from oracle.gp_oracle import (_lu, _mode_solve, _slogdet_from_lu, _solve, _unfold, mode_product,
                              param_grad_contract)
from tests.operator3_ref import FACES
from tests.operator3b_ref import DRIFT_ORDER, drift_of, loss_grad_3d_opb
from tests.operator3c_ref import conv_of
from tests.operator3m_ref import PAIRS, SUM_ORDER, cross_of
from tests.operator3n_ref import face_data
from tests.operator3v_ref import coef_fields
from tests.operator3x_ref import axis_blocks, opx_fields

BINOM = {1: (1, 1), 2: (1, 2, 1), 3: (1, 3, 3, 1), 4: (1, 4, 6, 4, 1)}


def high_of(high):
    """(c4, c3), two triples of floats; None is six zeros."""
    if high is None:
        return (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    c4, c3 = high
    c4, c3 = tuple(float(c) for c in c4), tuple(float(c) for c in c3)
    assert len(c4) == 3 and len(c3) == 3, "high is (c4, c3), two triples"
    return c4, c3


def radial4(k, d, a, want_l=False):
    """[m_0 .. m_4] of the radial factor at d >= 0 (and their d/dlog-ls when want_l); m_0..m_2 are
    oracle/gp_oracle.py _radial's.  Matern52, r = sqrt5 a d: m_3 = (5 sqrt5 / 3) a^3 r (3 - r) e^-r,
    m_4 = (25 / 3) a^4 (r^2 - 5 r + 3) e^-r; SE: m_3 = -4 a^2 d (2 a d^2 - 3) g, m_4 = 4 a^2 (4 a^2 d^4 -
    12 a d^2 + 3) g.  log-ls: a d/da at fixed d; Matern52 m_n = p^n h_n(r) gives p^n (n h_n + r h_{n+1})."""
    if O._is_matern(k):
        s5 = d.dtype.type(O.SQRT5) if hasattr(d, "dtype") else O.SQRT5
        r = s5 * a * d
        E = np.exp(-r)
        ka, k2, k3, k4 = s5 * a / 3, 5 * a * a / 3, 5 * s5 * a ** 3 / 3, 25 * a ** 4 / 3
        m = [(1 + r + r * r / 3) * E, -ka * r * (1 + r) * E, k2 * (r * r - r - 1) * E, k3 * r * (3 - r) * E,
             k4 * (r * r - 5 * r + 3) * E]
        if not want_l:
            return m
        ml = [-(r * r / 3) * (1 + r) * E, -ka * r * (2 + 2 * r - r * r) * E,
              k2 * (-r ** 3 + 5 * r * r - 2 * r - 2) * E, k3 * r * (r * r - 8 * r + 12) * E,
              k4 * (-r ** 3 + 11 * r * r - 28 * r + 12) * E]
        return m, ml
    u = a * d * d
    g = np.exp(-u)
    a2 = a * a
    m = [g, -2 * a * d * g, (4 * a2 * d * d - 2 * a) * g, -4 * a2 * d * (2 * u - 3) * g,
         4 * a2 * (4 * u * u - 12 * u + 3) * g]
    if not want_l:
        return m
    ml = [-u * g, (-2 * a * d + 2 * a2 * d ** 3) * g, (10 * a2 * d * d - 2 * a - 4 * a ** 3 * d ** 4) * g,
          a2 * d * (24 - 36 * u + 8 * u * u) * g, a2 * (24 - 156 * u + 112 * u * u - 16 * u ** 3) * g]
    return m, ml


def cosine4(k, d, f, want_f=False):
    """[c_0 .. c_4] of cos(2 pi f d) = C, -w S, -w^2 C, w^3 S, w^4 C (and their d/dfreq)."""
    if not O._has_cos(k):
        one = np.ones_like(d * f)
        z = np.zeros_like(one)
        c = [one, z, z, z, z]
        return (c, [z, z, z, z, z]) if want_f else c
    tp = d.dtype.type(O.TWO_PI) if hasattr(d, "dtype") else O.TWO_PI
    w = tp * f
    C, S = np.cos(w * d), np.sin(w * d)
    c = [C, -w * S, -w * w * C, w ** 3 * S, w ** 4 * C]
    if not want_f:
        return c
    cf = [-tp * d * S, -tp * S - tp * w * d * C, -2 * tp * w * C + tp * w * w * d * S,
          tp * (3 * w * w * S + w ** 3 * d * C), tp * (4 * w ** 3 * C - w ** 4 * d * S)]
    return c, cf


def leibniz(n, m, c):
    """sum_j C(n, j) m_j c_{n-j}: the order-n field of one component (unsigned)."""
    return sum(b * m[j] * c[n - j] for j, b in enumerate(BINOM[n]))


def _paras(paras, dtype):
    # (w and a are the reference's fp64 values e^{log-w}, e^{log-ls} in every dtype)
    return (np.exp(np.asarray(paras["log-w"], np.float64)).astype(dtype),
            np.exp(np.asarray(paras["log-ls"], np.float64)).astype(dtype),
            np.asarray(paras["freq"], np.float64).astype(dtype))


def kernel_block_n(kind, x1, x2, paras, n, dtype=np.float64):
    """Row-major [n1, n2] block of the n-th derivative (1..4) in the first argument of kappa."""
    k = O._kind_id(kind)
    d, s = O._pairs(x1, x2)  # (fp64: the distances are the reference's inputs)
    w, a, f = _paras(paras, dtype)
    dd = d.astype(dtype)[:, :, None]
    v = leibniz(n, radial4(k, dd, a), cosine4(k, dd, f)) @ w
    return v * s.astype(dtype) if n % 2 else v


def kernel_kd_high(kind, x, paras, dtype=np.float64):
    """(D4, D3) over the square block of x: the order-4 block (symmetric) and the signed order-3
    block (antisymmetric up to the convention s = +1 at 0, where the field is exactly 0)."""
    return kernel_block_n(kind, x, x, paras, 4, dtype), kernel_block_n(kind, x, x, paras, 3, dtype)


def param_grad_contract_high(kind, x, paras, G4, G3, dtype=np.float64):
    """sum_ij G4[i,j] dD4_ij/dtheta_q + G3[i,j] dD3_ij/dtheta_q for theta in (freq, log-ls, log-w);
    a dict of [Q] arrays like oracle/gp_oracle.py param_grad_contract."""
    k = O._kind_id(kind)
    d, s = O._pairs(x, x)
    w, a, f = _paras(paras, dtype)
    dd = d.astype(dtype)[:, :, None]
    m, ml = radial4(k, dd, a, True)
    c, cf = cosine4(k, dd, f, True)
    g4 = np.asarray(G4).astype(dtype).reshape(-1)
    g3 = (np.asarray(G3).astype(dtype) * s.astype(dtype)).reshape(-1)
    Q = len(w)
    out = {}
    for key, mm, cc in (("log-w", m, c), ("log-ls", ml, c), ("freq", m, cf)):
        out[key] = (g4 @ leibniz(4, mm, cc).reshape(-1, Q) + g3 @ leibniz(3, mm, cc).reshape(-1, Q)) * w
    if not O._has_cos(k):
        out["freq"] = np.zeros(Q, dtype)
    return out


def axis_blocks_high(kind, x, kp, jitter, c4, c3, c2, c1):
    """(K, D) of one axis: D = c4 D4 + c3 D3 + c2 DD + c1 D1, a zero weight's field left out."""
    K, D = axis_blocks(kind, x, kp, jitter, c2, c1)
    for n, c in ((4, c4), (3, c3)):
        if c != 0.0:
            D = D + c * kernel_block_n(kind, x, x, kp, n)
    return K, D


def loss_grad_3d_oph(prob, params, op, coef, dfaces=0, dvals=None, conv=None, cross=None, drift=None, high=None,
                     terms=None):
    """Negative log joint and gradient; every argument but high as loss_grad_3d_opb's; high: (c4, c3),
    two triples, or None."""
    c4, c3 = high_of(high)
    if not any(c4) and not any(c3):
        return loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift, terms=terms)
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
    KD = [axis_blocks_high(kind, xs[k], kps[k], prob["jitter"], c4[k], c3[k], c2[k], c1[k]) for k in range(3)]
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
        gh = param_grad_contract_high(kind, xs[k], kps[k], c4[k] * GD, c3[k] * GD)
        grad[f"kernel_paras_{k + 1}"] = {key: np.asarray(g2[key]) + np.asarray(g1[key]) + np.asarray(gh[key])
                                         for key in g2}
    return loss, grad


def criterion_3d_oph(prob, params, op, coef, dfaces=0, dvals=None, conv=None, cross=None, drift=None, high=None):
    """(boundary_gap + dgap) / (Nb + Nd) + eq_gap / Nc."""
    t = {}
    loss_grad_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, terms=t)
    return (t["bgap"] + t.get("dgap", 0.0)) / (t["Nb"] + t.get("Nd", 0)) + t["egap"] / np.asarray(params["U"]).size


def adam_replay_h(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, nsteps, lr=0.01, after=None):
    """tests/operator3_ref.py adam_replay on loss_grad_3d_oph."""
    opt = O.Adam(lr)
    st = opt.init(params)
    p, losses = params, []
    for i in range(nsteps):
        lo, go = loss_grad_3d_oph(prob, p, op, coef, dfaces, dvals, conv, cross, drift, high)
        losses.append(lo)
        p, st = opt.update(go, st, p)
        if after is not None:
            after(i, p)
    return losses, p
