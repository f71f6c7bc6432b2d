"""Plain NumPy restatements of one GEMM descriptor and one GEMV of the step, epilogues included
(csrc/gpk_internal.h GemmDesc / GemvDesc, include/gpk.h gpk_gemm_case), with no project code.

    P = alpha' op(A) op(B) + alpha2' op(A2) op(B2),   alpha' = alpha v when vscale (alpha2 likewise)
    STORE  C = P + beta C0                          Y = 0.5 Ys + v C (when asked for)
    RESID  C = P - F [+ u (u^2 - 1), u = U]         red[t] = sum_t C^2, red2[t] = sum_t Q1 Q2
    QUAD   C = P + beta C0                          red[t] = sum_t C U

t runs over the square tiles of side `tile` in row-major order; edge tiles hold only the rows < M
and columns < N.  The GEMV is the same on vectors with beta C0 applied under every epilogue,
u = U + U0, red2 formed under every epilogue, and t the blocks of 4 consecutive rows.

mode "f64": every operation in float64 (np.sum for the partials).  mode "ld": every operation in
np.longdouble and each partial the correctly rounded sum (math.fsum) of its long-double terms,
each term split exactly into two doubles.
"""
import math

import numpy as np

STORE, RESID, QUAD = 0, 1, 2


def _dtype(mode):
    return {"f64": np.float64, "ld": np.longdouble}[mode]


def _sum(terms, mode):
    terms = np.asarray(terms).reshape(-1)
    if mode == "f64":
        return float(np.sum(terms))
    hi = terms.astype(np.float64)
    lo = (terms - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(list(hi) + list(lo))


def tile_sums(X, tile, mode="f64"):
    """Sums of the 2D array X over its tiles of side `tile`, row-major tile order."""
    M, N = X.shape
    return np.array([_sum(X[i:i + tile, j:j + tile], mode)
                     for i in range(0, M, tile) for j in range(0, N, tile)], dtype=np.float64)


def gemm_ref(c, v, tile, mode="f64"):
    """One descriptor (the case dict of gpk._lib.dgemm_epi).  Returns a dict with C, Y, red, red2
    (None where the case does not ask for them); C and Y in the mode's dtype, partials float64."""
    T = _dtype(mode)

    def arr(name):
        return None if c.get(name) is None else np.asarray(c[name], dtype=T)

    def op(name, t):
        X = arr(name)
        return X.T if c.get(t) else X

    epi = c.get("epi", STORE)
    v = T(v)
    alpha = T(c.get("alpha", 1.0)) * (v if c.get("vscale") else T(1))
    C = alpha * (op("A", "ta") @ op("B", "tb"))
    if c.get("A2") is not None:
        alpha2 = T(c.get("alpha2", 1.0)) * (v if c.get("vscale2") else T(1))
        C = C + alpha2 * (op("A2", "ta2") @ op("B2", "tb2"))
    beta = T(c.get("beta", 0.0))
    out = {"Y": None, "red": None, "red2": None}
    if epi in (STORE, QUAD) and beta != 0:
        C = C + beta * arr("C0")
    if epi == RESID:
        C = C - arr("F")
        if c.get("ac"):
            u = arr("U")
            C = C + u * (u * u - T(1))
        if c.get("red"):
            out["red"] = tile_sums(C * C, tile, mode)
        if c.get("red2"):
            out["red2"] = tile_sums(arr("Q1") * arr("Q2"), tile, mode)
    if epi == QUAD and c.get("red"):
        out["red"] = tile_sums(C * arr("U"), tile, mode)
    if c.get("Ys") is not None:
        out["Y"] = T(0.5) * arr("Ys") + v * C
    out["C"] = C
    return out


def expand_classes(cid, cv, cdiag, ident):
    """The matrix a class operand stands for: cv[cid] (0 for negative pad ids); with ident, + cdiag
    on the diagonal and 1 on diagonal pads."""
    cid = np.asarray(cid)
    cv = np.asarray(cv)
    A = np.where(cid >= 0, cv[np.maximum(cid, 0)], cv.dtype.type(0))
    if ident:
        for i in range(min(cid.shape)):
            A[i, i] = A[i, i] + cv.dtype.type(cdiag) if cid[i, i] >= 0 else cv.dtype.type(1)
    return A


def gemv_ref(A, x, alpha=1.0, C0=None, beta=0.0, epi=STORE, ac=False, F=None, U=None, U0=None, Q1=None,
             Q2=None, mode="f64"):
    """One GEMV on the rows of A.  Returns (y, red, red2): y in the mode's dtype, the per-block
    partials float64 (red None under STORE, red2 None without Q1)."""
    T = _dtype(mode)

    def arr(a):
        return None if a is None else np.asarray(a, dtype=T).reshape(-1)

    A = np.asarray(A, dtype=T)
    rows = A.shape[0]
    y = T(alpha) * (A @ arr(x))
    if beta != 0:
        y = y + T(beta) * arr(C0)[:rows]
    red = red2 = None
    if epi == RESID:
        y = y - arr(F)[:rows]
        if ac:
            u = arr(U)[:rows] + (arr(U0)[:rows] if U0 is not None else T(0))
            y = y + u * (u * u - T(1))
        red = tile_sums((y * y).reshape(-1, 1), 4, mode)
    elif epi == QUAD:
        red = tile_sums((y * arr(U)[:rows]).reshape(-1, 1), 4, mode)
    if Q1 is not None:
        red2 = tile_sums((arr(Q1)[:rows] * arr(Q2)[:rows]).reshape(-1, 1), 4, mode)
    return y, red, red2
