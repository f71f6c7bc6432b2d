"""No GPU: the premise of tests/test_gpu_gemm_epilogues.py's bitwise layer, and the argument
checks of the two diagnostic entries it drives (gpk_dgemm_epi, gpk_dgemv_epi).

Premise: every Layer A case (integer operands in [-4, 4], signed power-of-two scalars, K + K2 <=
512) is computed once more in integers -- C scaled by 64, Y by 512 -- and the float64 reference
must equal that exactly.  The integer sums of absolute terms of every partial stay below 2^53
units of the last place, so every partial sum in any order is representable: no summation order
a kernel may choose can change a bit of C, Y, red or red2.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import gemm_epi_cases as GC
from tests import gemm_epi_ref as R
from tests.conftest import ROOT

LAYER_A = GC.layer_a()
GEMV_A = GC.gemv_layer_a()


def _scaled(x, s):
    q = int(round(float(x) * s))
    assert q / s == float(x), (x, s)
    return q


def _ints(a):
    a = np.asarray(a)
    q = a.astype(np.int64)
    assert np.array_equal(q, a) and np.abs(q).max() <= 4
    return q


def _abs_tile_max(X, tile):
    return max(int(np.abs(X[i:i + tile, j:j + tile]).sum())
               for i in range(0, X.shape[0], tile) for j in range(0, X.shape[1], tile))


def _int_gemm(c, v, tile):
    """(C * 64, Y * 512 or None, red * 4096 (RESID) / * 64 (QUAD) or None, red2 or None) in int64."""
    I = lambda k: _ints(c[k])
    op = lambda k, t: I(k).T if c.get(t) else I(k)
    assert abs(v) in (0.25, 0.5, 1.0, 2.0)
    for k in ("alpha", "alpha2", "beta"):
        assert abs(c.get(k, 1.0)) in (0.25, 0.5, 1.0, 2.0) or (k == "beta" and c.get(k, 0.0) == 0.0)
    K = op("A", "ta").shape[1] + (op("A2", "ta2").shape[1] if c.get("A2") is not None else 0)
    assert K <= 512
    C = _scaled(c["alpha"] * (v if c.get("vscale") else 1.0), 64) * (op("A", "ta") @ op("B", "tb"))
    if c.get("A2") is not None:
        C = C + _scaled(c["alpha2"] * (v if c.get("vscale2") else 1.0), 64) * (op("A2", "ta2") @ op("B2", "tb2"))
    epi = c.get("epi", R.STORE)
    red = red2 = Y = None
    if epi in (R.STORE, R.QUAD) and c.get("beta", 0.0) != 0.0:
        C = C + _scaled(c["beta"], 64) * I("C0")
    if epi == R.RESID:
        C = C - 64 * I("F")
        if c.get("ac"):
            C = C + 64 * I("U") * (I("U") ** 2 - 1)
        if c.get("red"):
            red = C * C
        if c.get("red2"):
            red2 = I("Q1") * I("Q2")
    if epi == R.QUAD and c.get("red"):
        red = C * I("U")
    if c.get("Ys") is not None:
        Y = 256 * I("Ys") + _scaled(v, 8) * C
    for X in (red, red2):
        if X is not None:
            assert _abs_tile_max(X, tile) < 2 ** 53
    sums = lambda X: None if X is None else np.array(
        [int(X[i:i + tile, j:j + tile].sum()) for i in range(0, X.shape[0], tile) for j in range(0, X.shape[1], tile)])
    return C, Y, sums(red), sums(red2)


@pytest.mark.parametrize("name,variant,v,cases", LAYER_A, ids=[t[0] for t in LAYER_A])
def test_layer_a_gemm_cases_are_exact(name, variant, v, cases):
    from gpk._lib import gemm_case_shape
    tile = GC.TILE[variant]
    for c in cases:
        M, N, _, _ = gemm_case_shape(c)
        for k in ("C0", "F", "U", "Q1", "Q2", "Ys"):
            assert c.get(k) is None or c[k].shape == (M, N), k
        ref = R.gemm_ref(c, v, tile)
        C, Y, red, red2 = _int_gemm(c, v, tile)
        assert np.array_equal(ref["C"] * 64.0, C.astype(np.float64))
        assert (Y is None) == (ref["Y"] is None)
        if Y is not None:
            assert np.array_equal(ref["Y"] * 512.0, Y.astype(np.float64))
        assert (red is None) == (ref["red"] is None) and (red2 is None) == (ref["red2"] is None)
        if red is not None:
            scale = 4096.0 if c["epi"] == R.RESID else 64.0
            assert np.array_equal(ref["red"] * scale, red.astype(np.float64))
        if red2 is not None:
            assert np.array_equal(ref["red2"], red2.astype(np.float64))


def _gemv_ref_args(k):
    return {a: b for a, b in k.items() if a not in ("inplace", "gate")}


@pytest.mark.parametrize("p,rows,ident,epi,k", GEMV_A, ids=[f"p{t[0]}-r{t[1]}-i{t[2]}-{t[3]}" for t in GEMV_A])
def test_layer_a_gemv_cases_are_exact(p, rows, ident, epi, k):
    cid, cv, cdiag = GC.gemv_operand(p, p)
    A = R.expand_classes(cid[:rows], cv, cdiag, ident)
    y, red, red2 = R.gemv_ref(A, **_gemv_ref_args(k))
    Ai, x = A.astype(np.int64), _ints(k["x"])
    assert np.array_equal(Ai, A) and np.abs(Ai).max() <= 7  # (class value + cdiag on the diagonal)
    Y = _scaled(k["alpha"], 8) * (Ai @ x)
    if k.get("beta", 0.0) != 0.0:
        Y = Y + _scaled(k["beta"], 8) * _ints(k["C0"])
    T = None
    if k["epi"] == R.RESID:
        Y = Y - 8 * _ints(k["F"])
        if k.get("ac"):
            u = _ints(k["U"]) + (_ints(k["U0"]) if k.get("U0") is not None else 0)
            Y = Y + 8 * u * (u * u - 1)
        T, scale = Y * Y, 64.0
    elif k["epi"] == R.QUAD:
        T, scale = Y * _ints(k["U"]), 8.0
    assert np.array_equal(y * 8.0, Y.astype(np.float64))
    blocks = lambda X: np.array([int(X[i:i + 4].sum()) for i in range(0, rows, 4)])
    assert (T is None) == (red is None)
    if T is not None:
        assert int(np.abs(T).sum()) < 2 ** 53
        assert np.array_equal(red * scale, blocks(T).astype(np.float64))
    assert (red2 is None) == (k.get("Q1") is None)
    if red2 is not None:
        assert np.array_equal(red2, blocks(_ints(k["Q1"]) * _ints(k["Q2"])).astype(np.float64))


def test_reference_modes_agree_on_real_inputs():
    """The float64 and long-double modes restate the same operation: on the real-valued cases
    they differ by the float64 mode's rounding only.  |dC| <= (K + 8) K eps: a float64 dot product
    of K terms bounded by 1 in any order, then the epilogue's few operations on values below K."""
    from gpk._lib import gemm_case_shape
    for name, variant, v, cases in GC.layer_b():
        c, tile = cases[0], GC.TILE[variant]
        a, b = R.gemm_ref(c, v, tile), R.gemm_ref(c, v, tile, "ld")
        K = sum(gemm_case_shape(c)[2:])
        dC = (K + 8) * K * GC.EPS
        assert np.abs(a["C"] - b["C"]).max() <= dC
        bars = GC.partial_bounds(c, b, tile, dC)
        for k in ("red", "red2"):
            assert (a[k] is None) == (b[k] is None)
            if a[k] is not None:
                assert np.all(np.abs(a[k] - b[k]) <= bars[k]), (name, k)


# ---- the ctypes mirror and the argument checks (before any device work) --------------------

def test_gemm_case_struct_layout_matches_header(tmp_path):
    from gpk._lib import gpk_gemm_case
    fields = [f for f, _ in gpk_gemm_case._fields_]
    probe = tmp_path / "probe.c"
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(gpk_gemm_case, {f}));' for f in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpk.h"\nint main(void){\n'
                     'printf("sizeof %zu\\n", sizeof(gpk_gemm_case));\n' + body + "\nreturn 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(gpk_gemm_case)
    for f in fields:
        assert int(out[f]) == getattr(gpk_gemm_case, f).offset, f


def _einval(fn, *a, **k):
    from gpk import _lib
    with pytest.raises(_lib.GPKError) as e:
        fn(*a, **k)
    assert e.value.code == _lib.GPK_EINVAL, e.value
    return str(e.value)


def test_dgemm_epi_refuses_what_the_kernels_do_not_support():
    from gpk import _lib
    ok = lambda **o: GC.gemm_case(1, 160, 96, 32, **o)
    for variant in (0, 4):
        _einval(_lib.dgemm_epi, variant, [ok()])
    _einval(_lib.dgemm_epi, 1, [])
    _einval(_lib.dgemm_epi, 1, [ok()] * 5)
    _einval(_lib.dgemm_epi, 1, [ok()], v=float("nan"))
    # sizes that are not multiples of 32 (M, N, K, K2 in turn)
    for M, N, K, K2 in ((48, 32, 32, 0), (32, 80, 32, 0), (32, 32, 16, 0), (32, 32, 32, 48)):
        assert "multiples of 32" in _einval(_lib.dgemm_epi, 2, [GC.gemm_case(1, M, N, K, K2)])
    # the side output with an epilogue other than STORE
    for epi in ("resid", "quad_beta"):
        c = ok(epi=epi)
        c["Ys"] = c["F"] if epi == "resid" else c["U"]
        assert "side output" in _einval(_lib.dgemm_epi, 2, [c])
    # partials below the tile count (160 x 96: 60 / 6 / 2 tiles)
    for variant in (1, 2, 3):
        assert "tile count" in _einval(_lib.dgemm_epi, variant, [ok(epi="resid")], spare=-1)
    # partials no epilogue forms
    _einval(_lib.dgemm_epi, 1, [ok(epi="store_beta", red=True)])
    _einval(_lib.dgemm_epi, 1, [ok(epi="quad_beta", red2=True)])
    # beta without C0, an odd leading dimension, missing epilogue operands, bad selectors
    _einval(_lib.dgemm_epi, 1, [ok(epi="store_y", beta=0.5)])
    assert "leading dimension" in _einval(_lib.dgemm_epi, 1, [ok(pad=1)])
    _einval(_lib.dgemm_epi, 1, [ok(epi="resid", F=None)])
    _einval(_lib.dgemm_epi, 1, [ok(epi="resid", ac=1)])
    _einval(_lib.dgemm_epi, 1, [ok(epi="quad_beta", U=None)])
    _einval(_lib.dgemm_epi, 1, [dict(ok(), epi=3)])
    _einval(_lib.dgemm_epi, 1, [ok(gate=3)])


def test_dgemm_epi_refuses_aliased_outputs_and_reports_tiles():
    """Raw struct: C also an operand, one C for two descriptors; `tiles` is set before the refusal."""
    from gpk import _lib
    lib = _lib.load()
    a = np.zeros((32, 32))
    g = (_lib.gpk_gemm_case * 2)()
    for x in g:
        x.M = x.N = x.K = 32
        x.A, x.B, x.C = _lib.dptr(a), _lib.dptr(a), _lib.dptr(a)
        x.lda = x.ldb = x.ldc = 32
        x.alpha = 1.0
    assert lib.gpk_dgemm_epi(3, 1, g, 1.0) == _lib.GPK_EINVAL
    assert b"output" in lib.gpk_last_error() and g[0].tiles == 1
    c = np.zeros((32, 32))
    for x in g:
        x.A, x.B, x.C = _lib.dptr(a), _lib.dptr(a), _lib.dptr(c)
    assert lib.gpk_dgemm_epi(1, 2, g, 1.0) == _lib.GPK_EINVAL
    assert g[0].tiles == 4 and g[1].tiles == 4
    assert lib.gpk_dgemm_epi(1, 1, None, 1.0) == _lib.GPK_EINVAL


def test_dgemv_epi_argument_checks():
    from gpk import _lib
    cid, cv, _ = GC.gemv_operand(3, 32)
    A = np.ones((32, 32))
    k = GC.gemv_case(4, 32, 32, "resid")
    _einval(_lib.dgemv_epi, A=np.ones((48, 48)), **dict(k, x=np.ones(48)))       # p not a multiple of 32
    _einval(_lib.dgemv_epi, A=np.ones((40, 32)), **k)                             # rows > p
    _einval(_lib.dgemv_epi, A=A, rows=0, **k)
    _einval(_lib.dgemv_epi, A=A, pad=2, **k)                                      # lda not a multiple of 32
    _einval(_lib.dgemv_epi, cid=np.where(cid == 3, len(cv), cid), cv=cv, **k)     # class id >= ncls
    _einval(_lib.dgemv_epi, A=A, **dict(k, F=None))
    _einval(_lib.dgemv_epi, A=A, **dict(k, ac=True))
    _einval(_lib.dgemv_epi, A=A, **dict(k, epi=R.QUAD))
    _einval(_lib.dgemv_epi, A=A, **dict(k, beta=0.5))
    _einval(_lib.dgemv_epi, A=A, **dict(k, red2=True))
    _einval(_lib.dgemv_epi, A=A, **dict(GC.gemv_case(4, 32, 32, "store"), red=True))
    _einval(_lib.dgemv_epi, A=A, **dict(k, epi=5))
    _einval(_lib.dgemv_epi, A=A, **dict(k, gate=-1))
    lib = _lib.load()
    x = np.ones(32)
    args = lambda A_, cid_, x_, y_: (32, 32, A_, cid_, _lib.dptr(cv), len(cv), 0.0, 0, 32, x_, 1.0, None, 0.0, 0, 0,
                                     None, None, None, None, None, None, None, 0, y_)
    pc = cid.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.gpk_dgemv_epi(*args(_lib.dptr(A), pc, _lib.dptr(x), _lib.dptr(x))) == _lib.GPK_EINVAL  # A and cid
    assert lib.gpk_dgemv_epi(*args(None, None, _lib.dptr(x), _lib.dptr(x))) == _lib.GPK_EINVAL        # neither
    assert lib.gpk_dgemv_epi(*args(_lib.dptr(A), None, _lib.dptr(x), _lib.dptr(x))) == _lib.GPK_EINVAL  # y == x
    assert lib.gpk_dgemv_epi(*args(_lib.dptr(A), None, _lib.dptr(x), None)) == _lib.GPK_EINVAL
