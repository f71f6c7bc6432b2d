"""50-digit mpmath restatement of the kernel fields (oracle/gp_oracle.py _radial / _cosine), the
reference of the field-accuracy tests.  Inputs and constants are the reference's fp64 values
(x, e^{log-ls}, e^{log-w}, freq, SQRT5, TWO_PI); everything after them is exact to 50 digits, the
phase 2 pi f d in particular (an exact product of three fp64 numbers)."""
import numpy as np

from oracle import gp_oracle as O

DPS = 50


def mp_of(x):
    """A long double (or fp64) as an mpf, exactly: its fp64 rounding plus the remainder."""
    import mpmath as mp
    mp.mp.dps = DPS
    x = np.longdouble(x)
    h = np.float64(x)
    return mp.mpf(float(h)) + mp.mpf(float(np.float64(x - np.longdouble(h))))


def component(kind, deriv, d, a, freq):
    """The six derivative fields of one mixture component at distance d >= 0, per unit weight:
    (f_w, f_l, f_f, d_w, d_l, d_f) = kappa_c / w_c, its d/dlog-ls and d/dfreq, and the same three
    of D_x1_kappa (deriv 1, unsigned) or DD_x1_kappa (deriv 2) -- param_grad_contract's Fw, Fl, Ff,
    Dw, Dl, Df.  Returns (values, scales): scales are the same expressions with every monomial
    taken in absolute value (|cos|, |sin| -> 1), exactly 0 where the field is identically 0."""
    import mpmath as mp
    mp.mp.dps = DPS
    k = O._kind_id(kind)
    d, a, f = mp.mpf(float(d)), mp.mpf(float(a)), mp.mpf(float(freq))
    s5, tp = mp.mpf(O.SQRT5), mp.mpf(O.TWO_PI)
    if O._is_matern(k):
        r = s5 * a * d
        E = mp.exp(-r)
        ka, k2 = s5 * a / 3, 5 * a * a / 3
        m = [(1 + r + r * r / 3) * E, -ka * r * (1 + r) * E, k2 * (r * r - r - 1) * E,
             -(r * r / 3) * (1 + r) * E, -ka * r * (2 + 2 * r - r * r) * E,
             k2 * (-r ** 3 + 5 * r * r - 2 * r - 2) * E]
        M = [(1 + r + r * r / 3) * E, ka * r * (1 + r) * E, k2 * (r * r + r + 1) * E,
             (r * r / 3) * (1 + r) * E, ka * r * (2 + 2 * r + r * r) * E,
             k2 * (r ** 3 + 5 * r * r + 2 * r + 2) * E]
    else:
        d2 = d * d
        g = mp.exp(-a * d2)
        m = [g, -2 * a * d * g, (4 * a * a * d2 - 2 * a) * g,
             -a * d2 * g, (-2 * a * d + 2 * a * a * d2 * d) * g,
             (10 * a * a * d2 - 2 * a - 4 * a ** 3 * d2 * d2) * g]
        M = [g, 2 * a * d * g, (4 * a * a * d2 + 2 * a) * g,
             a * d2 * g, (2 * a * d + 2 * a * a * d2 * d) * g,
             (10 * a * a * d2 + 2 * a + 4 * a ** 3 * d2 * d2) * g]
    if O._has_cos(k):
        w = tp * f
        C, S = mp.cos(w * d), mp.sin(w * d)
        c = [C, -w * S, -w * w * C, -tp * d * S, -tp * S - tp * w * d * C,
             -2 * tp * w * C + tp * w * w * d * S]
        wa = abs(w)
        Ca = [mp.mpf(1), wa, wa * wa, tp * d, tp + tp * wa * d, 2 * tp * wa + tp * wa * wa * d]
    else:
        z = mp.mpf(0)
        c = Ca = [mp.mpf(1), z, z, z, z, z]

    def fields(m, c):
        m0, m1, m2, m0l, m1l, m2l = m
        c0, c1, c2, c0f, c1f, c2f = c
        out = [m0 * c0, m0l * c0, m0 * c0f]
        if deriv == 2:
            out += [m2 * c0 + 2 * m1 * c1 + m0 * c2, m2l * c0 + 2 * m1l * c1 + m0l * c2,
                    m2 * c0f + 2 * m1 * c1f + m0 * c2f]
        else:
            out += [m1 * c0 + m0 * c1, m1l * c0 + m0l * c1, m1 * c0f + m0 * c1f]
        return out

    return fields(m, c), fields(M, Ca)


def block_entry(kind, deriv, x1, x2, paras):
    """(K, D, B_K, B_D) of kernel_block at one pair (x1, x2) as mpf: the sum over the mixture of
    w_c times the component fields, D with _pairs' sign; B: the absolute-monomial scales."""
    import mpmath as mp
    mp.mp.dps = DPS
    diff = float(x1) - float(x2)  # (exact or not, it is the reference's fp64 input)
    s = 1 if diff >= 0.0 else -1
    w = np.exp(np.asarray(paras["log-w"], np.float64))
    a = np.exp(np.asarray(paras["log-ls"], np.float64))
    f = np.asarray(paras["freq"], np.float64)
    K = D = BK = BD = mp.mpf(0)
    for c in range(len(w)):
        v, sc = component(kind, deriv if deriv else 2, abs(diff), a[c], f[c])
        wc = mp.mpf(float(w[c]))
        K, BK = K + wc * v[0], BK + wc * sc[0]
        D, BD = D + wc * v[3], BD + wc * sc[3]
    if deriv == 1:
        D = D * s
    return K, D, BK, BD
