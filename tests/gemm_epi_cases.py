"""The cases of tests/test_gpu_gemm_epilogues.py, built here so that tests/test_gemm_epi_ref.py can
prove on the CPU what the GPU test relies on: with integer operands in [-4, 4] and signed
power-of-two scalars every value a kernel can form is exactly representable, so the result does
not depend on the summation order and may be compared bit for bit.

A GEMM case is the dict gpk._lib.dgemm_epi takes (and tests/gemm_epi_ref.gemm_ref restates); a
GEMV case is the keyword dict of gpk._lib.dgemv_epi plus the class form's operands.
"""
import itertools

import numpy as np

from tests.gemm_epi_ref import tile_sums

EPS = np.finfo(np.float64).eps
STORE, RESID, QUAD = 0, 1, 2
SMALL, BIG, HUGE = 1, 2, 3  # GEMM variants: 16x16, 64x64, 128x128 tiles
TILE = {SMALL: 16, BIG: 64, HUGE: 128}
POW2 = (0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
# the epilogue configurations every kernel is run with
EPILOGUES = ("store_y", "store_beta", "resid", "resid_ac_q", "quad_beta")
SIGNATURES = list(itertools.product((0, 1), repeat=4))  # (ta, tb, ta2, tb2)


def _draw(rng, real, rows, cols):
    if real:
        return rng.uniform(-1.0, 1.0, size=(rows, cols))
    return rng.integers(-4, 5, size=(rows, cols)).astype(np.float64)


def gemm_case(seed, M, N, K, K2=0, sig=(0, 0, 0, 0), epi="store_y", real=False, **over):
    """One GEMM case.  Layer A (real = False): integer arrays, scalars drawn from POW2.  Layer B:
    uniform(-1, 1) arrays and the non-dyadic scalars alpha = 0.75, alpha2 = -0.3, beta = 0.25.
    `over` overrides or adds keys (inplace, vscale, vscale2, gate, pad, alpha, ...)."""
    rng = np.random.default_rng(seed)
    ta, tb, ta2, tb2 = sig
    c = {"A": _draw(rng, real, *((K, M) if ta else (M, K))), "B": _draw(rng, real, *((N, K) if tb else (K, N))),
         "ta": ta, "tb": tb}
    pick = (lambda: 1.0) if real else (lambda: float(rng.choice(POW2)))
    c["alpha"] = 0.75 if real else pick()
    if K2:
        c.update(A2=_draw(rng, real, *((K2, M) if ta2 else (M, K2))), B2=_draw(rng, real, *((N, K2) if tb2 else (K2, N))),
                 ta2=ta2, tb2=tb2, alpha2=-0.3 if real else pick())
    mn = lambda: _draw(rng, real, M, N)
    if epi == "store_y":
        c.update(epi=STORE, Ys=mn())
    elif epi == "store_beta":
        c.update(epi=STORE, beta=0.25 if real else pick(), C0=mn())
    elif epi == "resid":
        c.update(epi=RESID, F=mn(), red=True)
    elif epi == "resid_ac_q":
        c.update(epi=RESID, ac=1, F=mn(), U=mn(), Q1=mn(), Q2=mn(), red=True, red2=True)
    elif epi == "quad_beta":
        c.update(epi=QUAD, beta=0.25 if real else pick(), C0=mn(), U=mn(), red=True)
    else:
        raise KeyError(epi)
    c.update(over)
    return c


def sweep(variant, shapes, seed0):
    """(name, variant, v, [case]) for every shape x epilogue: one descriptor per launch, the
    transpose signature and v rotating with the case index."""
    out = []
    for si, (M, N, K, K2) in enumerate(shapes):
        for ei, epi in enumerate(EPILOGUES):
            i = si * len(EPILOGUES) + ei
            sig = SIGNATURES[(5 * i + seed0) % 16]
            c = gemm_case(seed0 + i, M, N, K, K2, sig, epi, vscale=i % 3 == 1, vscale2=bool(K2) and i % 3 == 2,
                          pad=2 * (i % 2))
            out.append((f"v{variant}-{M}x{N}x{K}+{K2}-{epi}-{''.join(map(str, sig))}", variant, POW2[i % 8], [c]))
    return out


SMALL_SHAPES = [(32, 64, 256, 0), (32, 64, 256, 256),   # the one-block path; 8 tiles (XCD-major dealing)
                (96, 32, 224, 0), (96, 32, 224, 160),   # K quarters 32 and 64 deep; 12 tiles (identity dealing)
                (32, 64, 32, 0), (32, 64, 32, 32),      # waves with an empty K range
                (32, 96, 96, 0), (32, 96, 96, 96)]
BIG_SHAPES = [(M, N, K, K2) for M in (32, 96, 160) for N in (32, 96, 160) for K in (32, 96) for K2 in (0, 64)]
HUGE_SHAPES = [(160, 96, 96, 0), (672, 160, 96, 0)]   # (tm, tn) = (2, 1) and (6, 2): across the GROUP_M swizzle


def huge_extra():
    """The 128x128 kernel beyond the sweep: every single signature, and dual products (two passes)
    in mixed signatures with each epilogue, beta placement, in-place C0 and one-sided vscale."""
    out = []
    for i, (ta, tb) in enumerate(itertools.product((0, 1), repeat=2)):
        c = gemm_case(700 + i, 160, 160, 64, 0, (ta, tb, 0, 0), "resid_ac_q")
        out.append((f"v3-single-sig{ta}{tb}", HUGE, 0.5, [c]))
    duals = [("resid", dict(beta=0.5, C0=True)),            # pass 0 must drop beta
             ("resid_ac_q", dict(vscale=1)),                 # v on the first product only
             ("quad_beta", dict(vscale2=1)),                 # v on the second product only
             ("store_beta", dict()),                         # pass 0 applies beta C0 once
             ("store_beta", dict(inplace=True)),             # C0 == C
             ("store_y", dict(vscale=1, vscale2=1))]
    mixed = [(0, 1, 1, 0), (1, 0, 0, 1), (1, 1, 0, 0), (0, 0, 1, 1), (0, 1, 0, 0), (1, 0, 1, 1)]
    for i, ((epi, over), sig) in enumerate(zip(duals, mixed)):
        for M, N in ((160, 96), (672, 160)):
            o = dict(over)
            if o.get("C0") is True:
                o["C0"] = _draw(np.random.default_rng(800 + i), False, M, N)
            c = gemm_case(810 + 2 * i + (M > 160), M, N, 96, 32, sig, epi, **o)
            out.append((f"v3-dual-{M}x{N}-{epi}-{'-'.join(k for k in o)}-{''.join(map(str, sig))}",
                        HUGE, POW2[(i + 2) % 8], [c]))
    return out


def batches():
    """Four descriptors in one launch on each variant: different M x N (different tile counts, so
    blocks of the smaller ones leave on tile >= tiles), different epilogues and signatures (on
    the 128x128 tile: two descriptors share a signature, the others do not; one dual per pass)."""
    out = []
    for variant in (SMALL, BIG, HUGE):
        s = 900 + 10 * variant
        cs = [gemm_case(s, 160, 96, 96, 64, (0, 1, 1, 0), "resid_ac_q", vscale2=1),
              gemm_case(s + 1, 32, 32, 32, 0, (1, 0, 0, 0), "store_y", pad=2),
              gemm_case(s + 2, 96, 160, 64, 0, (0, 1, 0, 0), "quad_beta", vscale=1),
              gemm_case(s + 3, 64, 32, 32, 96, (1, 0, 0, 1), "store_beta", inplace=True)]
        out.append((f"v{variant}-batch4", variant, -0.5, cs))
    return out


def layer_a():
    return (sweep(SMALL, SMALL_SHAPES, 100) + sweep(BIG, BIG_SHAPES, 300) + sweep(HUGE, HUGE_SHAPES, 600)
            + huge_extra() + batches())


def layer_b():
    """One real-valued case per kernel and epilogue (v = 0.37), duals where the kernel has them."""
    shape = {SMALL: (96, 32, 224, 160), BIG: (96, 160, 96, 64), HUGE: (160, 96, 96, 32)}
    out = []
    for variant in (SMALL, BIG, HUGE):
        for ei, epi in enumerate(EPILOGUES):
            M, N, K, K2 = shape[variant]
            sig = SIGNATURES[(3 * ei + variant) % 16]
            c = gemm_case(1000 + 10 * variant + ei, M, N, K, K2, sig, epi, real=True, vscale=ei % 2 == 1)
            out.append((f"real-v{variant}-{epi}", variant, 0.37, [c]))
    return out


def partial_bounds(c, ref, tile, dC):
    """Per-tile bounds on |red - red_ref| and |red2 - red2_ref| of a case whose C is within dC of
    ref["C"] elementwise and whose tile sums are float64 sums in some order (T = elements of the
    tile inside M x N): RESID sum(2 |c| dC + dC^2) + (T + 2) eps sum c^2; QUAD sum |u| dC +
    (T + 2) eps sum |c u|; red2 (T + 2) eps sum |q1 q2|."""
    f = lambda X: tile_sums(np.asarray(np.abs(X), dtype=np.float64), tile)
    Cr = np.asarray(np.abs(ref["C"]), dtype=np.float64)
    T = f(np.ones_like(Cr))
    out = {"red": None, "red2": None}
    if c.get("red") and c["epi"] == RESID:
        out["red"] = f(2 * Cr * dC + dC * dC) + (T + 2) * EPS * f(Cr * Cr)
    if c.get("red") and c["epi"] == QUAD:
        out["red"] = f(np.abs(c["U"]) * dC) + (T + 2) * EPS * f(Cr * c["U"])
    if c.get("red2"):
        out["red2"] = (T + 2) * EPS * f(np.asarray(c["Q1"]) * c["Q2"])
    return out


# ---- GEMV ---------------------------------------------------------------------------------

GEMV_P = (32, 96, 544, 512, 2048, 2560)   # tail only; 256-pair loop + a tail lanes < 16 run; 1, 4, 4 + 1 groups
GEMV_EPILOGUES = ("store", "store_beta_inplace", "resid", "resid_ac", "resid_ac_u0_q", "quad_beta")


def gemv_operand(seed, p, real=False):
    """The class operand of one p: ids (negative pads on and off the diagonal), values, cdiag."""
    rng = np.random.default_rng(seed)
    ncls = 37
    cid = rng.integers(0, ncls, size=(p, p)).astype(np.int32)
    cid[rng.random((p, p)) < 0.03] = -1
    for i in (1, 4, p - 2):
        cid[i, i] = -1 - (i % 3)
    cid[2, 2] = 5
    cv = rng.uniform(-1.0, 1.0, size=ncls) if real else rng.integers(-4, 5, size=ncls).astype(np.float64)
    return cid, cv, (0.001 if real else 3.0)


def gemv_case(seed, p, rows, epi, real=False, gate=0):
    """Keyword arguments of dgemv_epi / gemv_ref shared by both operand forms (x, scalars, epilogue)."""
    rng = np.random.default_rng(seed)
    vec = (lambda n: rng.uniform(-1.0, 1.0, size=n)) if real else (lambda n: rng.integers(-4, 5, size=n).astype(np.float64))
    pick = lambda: float(rng.choice(POW2))
    k = {"x": vec(p), "alpha": 0.75 if real else pick()}
    if epi == "store":
        k.update(epi=STORE, Q1=vec(rows), Q2=vec(rows))
    elif epi == "store_beta_inplace":
        k.update(epi=STORE, beta=0.25 if real else pick(), C0=vec(rows), inplace=True)
    elif epi == "resid":
        k.update(epi=RESID, F=vec(rows))
    elif epi == "resid_ac":
        k.update(epi=RESID, ac=True, F=vec(rows), U=vec(rows))
    elif epi == "resid_ac_u0_q":
        k.update(epi=RESID, ac=True, F=vec(rows), U=vec(rows), U0=vec(rows), Q1=vec(rows), Q2=vec(rows),
                 beta=0.25 if real else pick(), C0=vec(rows))
    elif epi == "quad_beta":
        k.update(epi=QUAD, U=vec(rows), beta=0.25 if real else pick(), C0=vec(rows))
    else:
        raise KeyError(epi)
    if gate:
        k["gate"] = gate
    return k


def gemv_layer_a():
    """(p, rows, ident, epilogue name, case): every (p, rows) with a rotating epilogue and ident;
    every epilogue with both ident values at p = 544 (all loop regimes but the batched one) and
    p = 512 (the batched one)."""
    out = []
    i = 0
    for p in GEMV_P:
        for rows in (p, p - 3, 5):
            epi = GEMV_EPILOGUES[i % len(GEMV_EPILOGUES)]
            out.append((p, rows, i % 2, epi, gemv_case(2000 + i, p, rows, epi)))
            i += 1
    for p in (544, 512):
        for epi in GEMV_EPILOGUES:
            for ident in (0, 1):
                out.append((p, p - 7, ident, epi, gemv_case(2100 + i, p, p - 7, epi)))
                i += 1
    return out
