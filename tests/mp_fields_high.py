"""The order-3 and order-4 kernel fields by 50-digit differentiation of kappa itself, and their
absolute-monomial scales (test infrastructure; the counterpart of tests/mp_fields.py for the
high-order terms of gpk_create3_oph).

exact(): kappa_c(d) / w_c = m(d) cos(2 pi f d) is written out as the reference writes it (Matern52:
(1 + sqrt5 a d + 5/3 a^2 d^2) e^{-sqrt5 a d}; SE: e^{-a d^2}), differentiated n times in d by sympy and
evaluated by mpmath at 50 digits on the fp64 inputs and constants (SQRT5, TWO_PI as oracle/gp_oracle.py
has them; Matern52's 5/3 a^2 d^2 is written r^2 / 3 with r = SQRT5 a d, the function whose derivatives the
closed forms are -- with the fp64 SQRT5 the two differ by one eps relative).  No closed form of tests/operator3h_ref.py or of the device code enters.  d = 0 is the
one-sided value (kappa is a function of d = |x_i - x_j| >= 0; odd orders carry the sign outside).

scales(): B_n = sum_j C(n, j) M_j W_{n-j}, M_j the radial derivative with every monomial of its
polynomial taken in absolute value, W_k = |om|^k (|cos|, |sin| -> 1): the quantity whose eps-multiple
bounds the rounding of any evaluation that forms the monomials to a few ulp each.

Bars in units of eps B_n, from the operation count of the device's five-output eval_kd_part per
component, extending tests/field_ulp_inputs.py N_D = 12 (exp and sincos <= 2 ulp each, one fma
correction each, <= 3 polynomial roundings, the products, a three-term sum, <= 2 for the mixture
sum): order 3 has a four-term sum, a^3 and om^3 (two more products on the longest monomial) and the
binomial factor: N_3 = 16; order 4 a five-term sum, a^4 and om^4: N_4 = 18.  The weighted block
c4 D4 + c3 D3 + c2 DD + c1 D1 adds one product and one sum rounding per field: + 2 each.
"""
import functools

import numpy as np

from oracle import gp_oracle as O

DPS = 50
N_3, N_4, N_COMBINE = 16.0, 18.0, 2.0
BINOM = {3: (1, 3, 3, 1), 4: (1, 4, 6, 4, 1)}


@functools.lru_cache(maxsize=None)
def _derivs(matern, cos):
    import sympy as sp
    d, a, w, s5 = sp.symbols("d a w s5", positive=True)
    if matern:
        r = s5 * d * a  # (5/3 a^2 d^2 as r^2 / 3: see the module docstring)
        m = (1 + r + r ** 2 / 3) * sp.exp(-r)
    else:
        m = sp.exp(-d ** 2 * a)
    k = m * sp.cos(w * d) if cos else m
    return {n: sp.lambdify((d, a, w, s5), sp.diff(k, d, n), modules="mpmath") for n in (1, 2, 3, 4)}


def exact(kind, n, d, a, freq):
    """d^n / dd^n of kappa_c / w_c at distance d >= 0, as an mpf."""
    import mpmath as mp
    mp.mp.dps = DPS
    k = O._kind_id(kind)
    w = mp.mpf(O.TWO_PI) * mp.mpf(float(freq))
    return _derivs(O._is_matern(k), O._has_cos(k))[n](mp.mpf(float(d)), mp.mpf(float(a)), w, mp.mpf(O.SQRT5))


def scales(kind, n, d, a, freq):
    """B_n of one component (float)."""
    k = O._kind_id(kind)
    d, a = float(d), float(a)
    if O._is_matern(k):
        r = O.SQRT5 * a * d
        E = np.exp(-r)
        p = O.SQRT5 * a
        M = [(1 + r + r * r / 3) * E, p / 3 * r * (1 + r) * E, p ** 2 / 3 * (r * r + r + 1) * E,
             p ** 3 / 3 * r * (3 + r) * E, p ** 4 / 3 * (r * r + 5 * r + 3) * E]
    else:
        u = a * d * d
        g = np.exp(-u)
        M = [g, 2 * a * d * g, (4 * a * u + 2 * a) * g, 4 * a * a * d * (2 * u + 3) * g,
             4 * a * a * (4 * u * u + 12 * u + 3) * g]
    wa = abs(O.TWO_PI * float(freq)) if O._has_cos(k) else 0.0
    return float(sum(b * M[j] * wa ** (n - j) for j, b in enumerate(BINOM[n])))


def block_scale(kind, n, x1, x2, paras):
    """[n1, n2] array of B_n over a block: sum over the mixture of w_c times the component scales."""
    k = O._kind_id(kind)
    d = np.abs(np.asarray(x1, np.float64).reshape(-1, 1) - np.asarray(x2, np.float64).reshape(1, -1))[:, :, None]
    w = np.exp(np.asarray(paras["log-w"], np.float64))
    a = np.exp(np.asarray(paras["log-ls"], np.float64))
    f = np.asarray(paras["freq"], np.float64)
    if O._is_matern(k):
        r = O.SQRT5 * a * d
        E = np.exp(-r)
        p = O.SQRT5 * a
        M = [(1 + r + r * r / 3) * E, p / 3 * r * (1 + r) * E, p ** 2 / 3 * (r * r + r + 1) * E,
             p ** 3 / 3 * r * (3 + r) * E, p ** 4 / 3 * (r * r + 5 * r + 3) * E]
    else:
        u = a * d * d
        g = np.exp(-u)
        M = [g, 2 * a * d * g, (4 * a * u + 2 * a) * g, 4 * a * a * d * (2 * u + 3) * g,
             4 * a * a * (4 * u * u + 12 * u + 3) * g]
    wa = np.abs(O.TWO_PI * f) if O._has_cos(k) else np.zeros_like(f)
    return sum(b * M[j] * wa ** (n - j) for j, b in enumerate(BINOM[n])) @ w


def block_entry(kind, n, x1, x2, paras):
    """(Dn, B_n) of the order-n block at one pair (x1, x2): the mixture sum as an mpf, odd orders with
    _pairs' sign, and its scale."""
    import mpmath as mp
    mp.mp.dps = DPS
    diff = float(x1) - float(x2)
    s = 1 if diff >= 0.0 or n % 2 == 0 else -1
    w = np.exp(np.asarray(paras["log-w"], np.float64))
    a = np.exp(np.asarray(paras["log-ls"], np.float64))
    f = np.asarray(paras["freq"], np.float64)
    D, B = mp.mpf(0), 0.0
    for c in range(len(w)):
        D += mp.mpf(float(w[c])) * exact(kind, n, abs(diff), a[c], f[c])
        B += float(w[c]) * scales(kind, n, abs(diff), a[c], f[c])
    return D * s, B
