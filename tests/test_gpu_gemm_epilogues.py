"""The fused epilogues of the step's GEMM kernels and of its GEMV, kernel by kernel, through the
diagnostic entries gpk_dgemm_epi / gpk_dgemv_epi (one launch_gemm_auto / launch_gemv exactly as
the step issues it) against the NumPy restatement of tests/gemm_epi_ref.py.

Layer A, bit for bit.  Operands and epilogue arrays are integers in [-4, 4], alpha, alpha2, beta
and v signed powers of two, K + K2 <= 512: every product, sum, u (u^2 - 1), c^2 and tile sum is
exactly representable (tests/test_gemm_epi_ref.py proves it for every case here, in integers), so
the result does not depend on the order a kernel sums in and C, Y, every red[tile] and every
red2[tile] must EQUAL the reference.  This is what sees a partial in the wrong slot (the
128x128 kernel's GROUP_M swizzle, the XCD-major dealing), an edge tile summing elements outside
M x N, beta applied in the wrong pass of a dual product on the 128x128 tile, a batch mixing tile
counts and transpose signatures, a write past the tile count or into the padding columns, and a
closed gate that writes.

Layer B, rounding.  Integers cannot see a narrowed intermediate, so one case per kernel and
epilogue (and the GEMV at p = 544 in both forms) runs on uniform(-1, 1) operands with alpha = 0.75,
alpha2 = -0.3, beta = 0.25, v = 0.37 against the long-double reference, with derived bars:
    C     bar_C = 64 eps (K |a| max|A| max|B| + K2 |a2| max|A2| max|B2|) + 4 eps max|C_ref|
          (a, a2: the factors applied, v included where vscale says so)
    Y     |v| bar_C + 4 eps max|Y_ref|
    red   RESID: sum_tile (2 |c| bar_C + bar_C^2) + (T + 2) eps sum_tile c^2
          QUAD:  sum_tile |u| bar_C + (T + 2) eps sum_tile |c u|
    red2  (T + 2) eps sum_tile |q1 q2|          T: the tile's elements inside M x N
    GEMV  the same with K = p and T = 4.
"""
import numpy as np
import pytest

from gpk import _lib
from gpk._lib import GATE_CLOSED, GATE_OPEN, SENTINEL, dgemm_epi, dgemv_epi, gemm_case_shape
from tests import gemm_epi_cases as GC
from tests import gemm_epi_ref as R

pytestmark = pytest.mark.gpu
EPS = GC.EPS
LAYER_A = GC.layer_a()
LAYER_B = GC.layer_b()
GEMV_A = GC.gemv_layer_a()


def _tiles(c, variant):
    M, N, _, _ = gemm_case_shape(c)
    t = GC.TILE[variant]
    return -(-M // t) * -(-N // t)


def _check_untouched(out, c, variant):
    """What no launch may write: the padding columns of C and Y, partial entries past the tiles."""
    pad = c.get("pad", 0)
    if pad:
        assert np.all(out["C_buf"][:, -pad:] == SENTINEL)
        if out["Y_buf"] is not None:
            assert np.all(out["Y_buf"][:, -pad:] == SENTINEL)
    for k in ("red", "red2"):
        if out[k] is not None:
            assert np.all(out[k][out["tiles"]:] == SENTINEL), k


def _check_exact(outs, cases, variant, v):
    for i, (out, c) in enumerate(zip(outs, cases)):
        ref = R.gemm_ref(c, v, GC.TILE[variant])
        assert out["tiles"] == _tiles(c, variant)
        bad = np.argwhere(out["C"] != ref["C"])
        assert bad.size == 0, f"desc {i}: C differs at {len(bad)} elements, first {bad[0]}"
        if ref["Y"] is not None:
            assert np.array_equal(out["Y"], ref["Y"]), f"desc {i}: Y"
        for k in ("red", "red2"):
            assert (out[k] is None) == (ref[k] is None)
            if ref[k] is not None:
                got = out[k][:out["tiles"]]
                assert np.array_equal(got, ref[k]), f"desc {i}: {k} differs in tiles {np.flatnonzero(got != ref[k])}"
        _check_untouched(out, c, variant)


# ---- Layer A: GEMM ------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant,v,cases", LAYER_A, ids=[t[0] for t in LAYER_A])
def test_gemm_epilogue_bitwise(name, variant, v, cases):
    _check_exact(dgemm_epi(variant, cases, v), cases, variant, v)


def _gate_cases(variant):
    """A dual RESID with both partials, a STORE with the side output and an in-place QUAD, at an
    edge-tile shape of the variant."""
    s = 1200 + 10 * variant
    return [GC.gemm_case(s, 160, 96, 64, 32, (0, 1, 1, 0), "resid_ac_q", pad=2),
            GC.gemm_case(s + 1, 96, 160, 32, 0, (1, 0, 0, 0), "store_y", vscale=1),
            GC.gemm_case(s + 2, 32, 96, 96, 64, (0, 0, 1, 1), "quad_beta", inplace=True)]


@pytest.mark.parametrize("variant", [GC.SMALL, GC.BIG, GC.HUGE])
def test_gemm_open_gate_is_no_gate(variant):
    for batch in ([c] for c in _gate_cases(variant)):
        plain = dgemm_epi(variant, batch, 0.5)
        gated = dgemm_epi(variant, [dict(c, gate=GATE_OPEN) for c in batch], 0.5)
        _check_exact(gated, batch, variant, 0.5)
        for a, b in zip(plain, gated):
            for k in ("C_buf", "Y_buf", "red", "red2"):
                assert (a[k] is None) == (b[k] is None)
                assert a[k] is None or a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("variant", [GC.SMALL, GC.BIG, GC.HUGE])
def test_gemm_closed_gate_writes_nothing(variant):
    """C, Y, red and red2 keep the bytes they were uploaded with (single launches and one batch;
    on the 128x128 tile the dual product's first pass is gated as well)."""
    cases = [dict(c, gate=GATE_CLOSED) for c in _gate_cases(variant)]
    for batch in [[c] for c in cases] + [cases]:
        for out, c in zip(dgemm_epi(variant, batch, 0.5), batch):
            if c.get("inplace"):
                assert np.array_equal(out["C"], c["C0"])
            else:
                assert np.all(out["C_buf"] == SENTINEL)
            for k in ("Y_buf", "red", "red2"):
                assert out[k] is None or np.all(out[k] == SENTINEL), k


def test_gemm_batch_with_one_closed_gate():
    """The gate is per descriptor: a closed one among open and ungated ones stops only its own."""
    for variant in (GC.SMALL, GC.BIG, GC.HUGE):
        cases = _gate_cases(variant)
        cases[0]["gate"] = GATE_CLOSED
        cases[1]["gate"] = GATE_OPEN
        outs = dgemm_epi(variant, cases, -2.0)
        assert np.all(outs[0]["C_buf"] == SENTINEL) and np.all(outs[0]["red"] == SENTINEL)
        _check_exact(outs[1:], cases[1:], variant, -2.0)


# ---- Layer A: GEMV ------------------------------------------------------------------------

_OPERANDS = {}


def _operand(p, real=False):
    """One class operand per p (ids, values, cdiag), built once."""
    if (p, real) not in _OPERANDS:
        _OPERANDS[(p, real)] = GC.gemv_operand(p, p, real)
    return _OPERANDS[(p, real)]


def _ref_args(k):
    return {a: b for a, b in k.items() if a not in ("inplace", "gate")}


def _run_gemv_both(p, rows, ident, k):
    cid, cv, cdiag = _operand(p)
    A = R.expand_classes(cid[:rows], cv, cdiag, ident)
    want = dict(red=k["epi"] != R.STORE, red2=k.get("Q1") is not None)
    cls = dgemv_epi(cid=cid, cv=cv, cdiag=cdiag, ident=ident, rows=rows, **want, **k)
    mat = dgemv_epi(A=A, **want, **k)
    return A, cls, mat


@pytest.mark.parametrize("p,rows,ident,epi,k", GEMV_A, ids=[f"p{t[0]}-r{t[1]}-i{t[2]}-{t[3]}" for t in GEMV_A])
def test_gemv_epilogue_bitwise(p, rows, ident, epi, k):
    A, cls, mat = _run_gemv_both(p, rows, ident, k)
    ref = R.gemv_ref(A, **_ref_args(k))
    for form, got in (("class", cls), ("matrix", mat)):
        for name, g, r in zip(("y", "red", "red2"), got, ref):
            assert (g is None) == (r is None), (form, name)
            if r is not None:
                assert np.array_equal(g, r), f"{form} form: {name} differs at {np.flatnonzero(g != r)[:8]}"


@pytest.mark.parametrize("p", [96, 544, 512])
def test_gemv_closed_gate_leaves_y(p):
    """y keeps its bytes under a closed gate, in place as well (the partials are formed anyway:
    the step reads them only behind the same gate); an open gate is no gate."""
    rows = p - 3
    for epi in ("resid_ac_u0_q", "store_beta_inplace"):
        k = GC.gemv_case(2300 + p, p, rows, epi)
        A, cls, mat = _run_gemv_both(p, rows, 1, dict(k, gate=GATE_CLOSED))
        for y, _, _ in (cls, mat):
            assert np.array_equal(y, k["C0"]) if k.get("inplace") else np.all(y == SENTINEL)
        ref = R.gemv_ref(A, **_ref_args(k))
        for got in _run_gemv_both(p, rows, 1, dict(k, gate=GATE_OPEN))[1:]:
            assert np.array_equal(got[0], ref[0])
            assert ref[1] is None or np.array_equal(got[1], ref[1])


# ---- Layer B: rounding --------------------------------------------------------------------

def _amax(c, k):
    return np.abs(c[k]).max()


@pytest.mark.parametrize("name,variant,v,cases", LAYER_B, ids=[t[0] for t in LAYER_B])
def test_gemm_epilogue_rounding(name, variant, v, cases):
    c, tile = cases[0], GC.TILE[variant]
    out = dgemm_epi(variant, cases, v)[0]
    ref = R.gemm_ref(c, v, tile, "ld")
    _, _, K, K2 = gemm_case_shape(c)
    a1 = abs(c["alpha"] * (v if c.get("vscale") else 1.0))
    bar_C = 64 * EPS * K * a1 * _amax(c, "A") * _amax(c, "B")
    if K2:
        a2 = abs(c["alpha2"] * (v if c.get("vscale2") else 1.0))
        bar_C += 64 * EPS * K2 * a2 * _amax(c, "A2") * _amax(c, "B2")
    bar_C += 4 * EPS * float(np.abs(ref["C"]).max())
    err = float(np.abs(out["C"] - ref["C"]).max())
    print(f"{name}: C err {err:.3e} bar {bar_C:.3e}")
    assert err <= bar_C
    if ref["Y"] is not None:
        bar_Y = abs(v) * bar_C + 4 * EPS * float(np.abs(ref["Y"]).max())
        err = float(np.abs(out["Y"] - ref["Y"]).max())
        print(f"{name}: Y err {err:.3e} bar {bar_Y:.3e}")
        assert err <= bar_Y
    bars = GC.partial_bounds(c, ref, tile, bar_C)
    for k in ("red", "red2"):
        assert (out[k] is None) == (ref[k] is None)
        if ref[k] is not None:
            err = np.abs(out[k][:out["tiles"]] - ref[k])
            worst = int(np.argmax(err / bars[k]))
            print(f"{name}: {k} worst tile {worst}: err {err[worst]:.3e} bar {bars[k][worst]:.3e}")
            assert np.all(err <= bars[k]), k
    _check_untouched(out, c, variant)


@pytest.mark.parametrize("epi", ["resid_ac_u0_q", "quad_beta", "store_beta_inplace"])
def test_gemv_epilogue_rounding(epi):
    p, rows = 544, 541
    cid, cv, cdiag = _operand(p, real=True)
    k = GC.gemv_case(2400, p, rows, epi, real=True)
    want = dict(red=k["epi"] != R.STORE, red2=k.get("Q1") is not None)
    for ident in (0, 1):
        A = R.expand_classes(cid[:rows], cv, cdiag, ident)
        y_ref, red_ref, red2_ref = R.gemv_ref(A, mode="ld", **_ref_args(k))
        bar_y = 64 * EPS * p * abs(k["alpha"]) * np.abs(A).max() * np.abs(k["x"]).max() + 4 * EPS * float(np.abs(y_ref).max())
        # the GEMV's partials as a one-column GEMM case of 4-row tiles
        as_case = dict(epi=k["epi"], red=want["red"], red2=want["red2"], U=None, Q1=None, Q2=None)
        for name in ("U", "Q1", "Q2"):
            if k.get(name) is not None:
                as_case[name] = np.asarray(k[name]).reshape(-1, 1)
        bars = GC.partial_bounds(as_case, {"C": np.asarray(y_ref).reshape(-1, 1)}, 4, bar_y)
        cls = dgemv_epi(cid=cid, cv=cv, cdiag=cdiag, ident=ident, rows=rows, **want, **k)
        mat = dgemv_epi(A=A, **want, **k)
        for form, (y, red, red2) in (("class", cls), ("matrix", mat)):
            err = float(np.abs(y - y_ref).max())
            print(f"gemv {epi} ident {ident} {form}: y err {err:.3e} bar {bar_y:.3e}")
            assert err <= bar_y
            for nm, g, r in (("red", red, red_ref), ("red2", red2, red2_ref)):
                assert (g is None) == (r is None)
                if r is not None:
                    e = np.abs(g - r)
                    w = int(np.argmax(e / bars[nm]))
                    print(f"gemv {epi} ident {ident} {form}: {nm} worst block {w}: err {e[w]:.3e} bar {bars[nm][w]:.3e}")
                    assert np.all(e <= bars[nm]), nm
        assert all(np.array_equal(a, b) for a, b in zip(cls, mat) if a is not None)  # same pairs, same order
