"""Host-side surface of the mixed fourth-order partials (no GPU): header and ctypes entries, the struct
layout, every argument error of gpk_create3_opq and gpk_assemble_pairs5 (all returned before a device
is touched), the Python layer's own checks, the new configs, and the rounding of the NumPy yardstick's
chained u_jjkk term on the GPU tests' own problems."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import PKG_DIR, ROOT
from tests.test_abi import header_functions
from tests.test_operator3v_host import _valid_problem


def test_header_and_ctypes_entries():
    from gpk import _lib
    lib = _lib.load()
    for must in ("gpk_create3_opq", "gpk_bicross_info3", "gpk_assemble_pairs5"):
        assert must in header_functions() and must in _lib.EXPORTS and hasattr(lib, must)
    assert lib.gpk_abi_version() == 2
    with open(os.path.join(ROOT, "include", "gpk.h")) as f:
        header = " ".join(f.read().replace("*", " ").split())
    assert "q_jk d^4 u / d x_j^2 d x_k^2" in header
    for formula in ("Z2_j = DD_j x_j A_j", "H2_jk = K_k^{-1} x_k Z2_j", "B_jk = q_jk DD_k x_k H2_jk",
                    "+ B_13 + B_12 + B_23", "Hb2_jk = q_jk DD_k^T x_k R", "T_j += DD_j^T x_j Zb2_jk"):
        assert formula in header, formula
    for limit in ("fields on q", "u_xxxy or u_xyy", "boundary data on second derivatives", "the class path",
                  "1-axis and 2-axis handles"):
        assert limit in header, limit
    # the gap the high-order handles named is closed in all three places
    for path in (os.path.join(ROOT, "include", "gpk.h"), os.path.join(ROOT, "README.md"), os.path.join(ROOT, "DESIGN.md")):
        with open(path) as f:
            text = " ".join(f.read().replace("*", " ").split())
        assert "mixed high-order partials such as u_xxyy" not in text, path


def test_bicross3_struct_layout_matches_header(tmp_path):
    from gpk._lib import gpk_bicross3
    assert [f for f, _ in gpk_bicross3._fields_] == ["q"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpk.h"\nint main(void){\n'
                     'printf("sizeof %zu\\n", sizeof(gpk_bicross3));\n'
                     'printf("q %zu\\n", offsetof(gpk_bicross3, q));\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(gpk_bicross3) == 24
    assert int(out["q"]) == gpk_bicross3.q.offset == 0


def test_argument_errors_without_a_device():
    from gpk import _lib
    from gpk._lib import dptr
    lib = _lib.load()
    ns = (4, 3, 2)
    p, keep, n = _valid_problem(ns)
    c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
    c.c2[:], c.c1[:], c.react[:], c.faces = (1.0, 0.0, 1.0), (0.0, 0.0, 0.5), (2.0, 0.0, 0.0), 0b011111
    nb = 2 * (ns[1] * ns[2] + ns[0] * ns[2] + ns[0] * ns[1])
    dv = np.full(nb, np.nan)
    dv[:ns[1] * ns[2]] = 0.25  # face 0
    bd = _lib.gpk_bdata3()
    bd.dfaces, bd.dvals = 1, dptr(dv)
    cv = _lib.gpk_conv3()
    cv.g[:] = (1.0, 0.5, 0.0)
    mx = _lib.gpk_cross3()
    mx.m[:] = (0.5, 0.0, -1.0)
    field = np.linspace(-1.0, 1.0, n)
    dr = _lib.gpk_drift3()
    dr.b[1] = dptr(field)
    hi = _lib.gpk_high3()
    hi.c4[:], hi.c3[:] = (0.01, 0.0, 0.0), (0.0, -0.2, 0.0)
    bq = _lib.gpk_bicross3()
    bq.q[:] = (0.002, 0.0, -0.001)

    def call(pp=p, cc=c, ff=None, bb=None, vv=None, mm=None, dd=None, hh=None, qq=bq, out=h):
        """GPK_EINVAL from the argument checks, or 'device': the call passed them all and failed at
        the device check that follows."""
        ref = lambda x: None if x is None else ctypes.byref(x)
        rc = lib.gpk_create3_opq(ref(pp), ref(cc), ref(ff), ref(bb), ref(vv), ref(mm), ref(dd), ref(hh), ref(qq), 1.0,
                                 ref(out))
        assert rc != _lib.GPK_OK
        return "device" if b"device" in lib.gpk_last_error() else rc

    zero = _lib.gpk_bicross3()
    for qq in (bq, zero, None):  # (zeros and NULL: the gpk_create3_oph route)
        for hh in (hi, _lib.gpk_high3(), None):
            for dd in (dr, None):
                for mm in (mx, None):
                    for vv in (cv, None):
                        for kw in (dict(pp=None), dict(cc=None), dict(out=None)):
                            assert call(qq=qq, hh=hh, dd=dd, mm=mm, vv=vv, **kw) == _lib.GPK_EINVAL
                            assert call(qq=qq, hh=hh, dd=dd, mm=mm, vv=vv, bb=bd, **kw) == _lib.GPK_EINVAL
                        assert call(qq=qq, hh=hh, dd=dd, mm=mm, vv=vv) == "device"
                        assert call(qq=qq, hh=hh, dd=dd, mm=mm, vv=vv, bb=bd) == "device"
    # a non-finite q in each position, alone and next to everything else
    for t in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            q2 = _lib.gpk_bicross3()
            q2.q[:] = bq.q[:]
            q2.q[t] = bad
            for kw in (dict(), dict(vv=cv), dict(mm=mx, dd=dr), dict(vv=cv, mm=mx, bb=bd, dd=dr, hh=hi)):
                assert call(qq=q2, **kw) == _lib.GPK_EINVAL, (t, bad)
                assert b"q must be finite" in lib.gpk_last_error()
    # everything the older create calls reject, next to a bi-pair
    h2 = _lib.gpk_high3()
    h2.c4[1] = np.nan
    assert call(hh=h2) == _lib.GPK_EINVAL and b"c4 and c3 must be finite" in lib.gpk_last_error()
    m2 = _lib.gpk_cross3()
    m2.m[:] = (0.0, np.inf, 0.0)
    assert call(mm=m2) == _lib.GPK_EINVAL and b"m must be finite" in lib.gpk_last_error()
    v2 = _lib.gpk_conv3()
    v2.g[:] = (0.0, np.nan, 0.0)
    assert call(vv=v2) == _lib.GPK_EINVAL and b"g must be finite" in lib.gpk_last_error()
    f2 = field.copy()
    f2[n // 2] = np.nan
    d2 = _lib.gpk_drift3()
    d2.b[0] = dptr(f2)
    assert call(dd=d2) == _lib.GPK_EINVAL and b"drift field has a non-finite value" in lib.gpk_last_error()
    for bad in (-1, 64):
        b2 = _lib.gpk_bdata3()
        b2.dfaces, b2.dvals = bad, dptr(dv)
        assert call(bb=b2) == _lib.GPK_EINVAL, bad
    b2 = _lib.gpk_bdata3()
    b2.dfaces = 1
    assert call(bb=b2) == _lib.GPK_EINVAL  # NULL dvals
    dv2 = dv.copy()
    dv2[3] = np.inf
    b2.dvals = dptr(dv2)
    assert call(bb=b2) == _lib.GPK_EINVAL
    c.faces = 0
    assert call() == _lib.GPK_EINVAL and call(bb=bd) == "device"
    for faces in (64, -1):
        c.faces = faces
        assert call() == _lib.GPK_EINVAL, faces
    c.faces = 0b011111
    c.c2[1] = float("nan")
    assert call() == _lib.GPK_EINVAL
    c.c2[1] = 0.0
    p.eq = _lib.EQ_IDS["allencahn"]
    assert call() == _lib.GPK_EINVAL
    p.eq = _lib.EQ_IDS["poisson"]
    for name, bad in (("kind", 4), ("q", 0), ("q", 65), ("n1", 1), ("n3", 1025)):
        was = getattr(p, name)
        setattr(p, name, bad)
        assert call() == _lib.GPK_EINVAL, (name, bad)
        setattr(p, name, was)
    cf = _lib.gpk_coef3()
    cf.a[1] = dptr(f2)
    assert call(ff=cf) == _lib.GPK_EINVAL
    assert call() == "device"
    assert not h.value
    z3 = (ctypes.c_double * 3)()
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.gpk_bicross_info3(None, ctypes.cast(z3, dp)) == _lib.GPK_EINVAL
    del keep


def test_assemble_pairs5_argument_errors_without_a_device():
    from gpk import _lib
    from gpk._lib import dptr
    lib = _lib.load()
    x = np.linspace(0.0, 1.0, 5)
    kp = [np.zeros(2), np.zeros(2), np.ones(2)]
    K, D, D1, D2 = (np.empty((5, 5)) for _ in range(4))

    def call(kind=1, xx=x, n=5, q=2, jitter=1e-6, w=(0.1, 0.2, 0.3, 0.4), Ko=K, Do=D, D1o=D1, D2o=D2):
        opt = lambda a: None if a is None else dptr(a)
        rc = lib.gpk_assemble_pairs5(kind, opt(xx), n, dptr(kp[0]), dptr(kp[1]), dptr(kp[2]), q, jitter, *w,
                                     opt(Ko), opt(Do), opt(D1o), opt(D2o))
        assert rc != _lib.GPK_OK
        return "device" if b"device" in lib.gpk_last_error() else rc

    assert call() == "device" and call(D1o=None) == "device"  # (D1_out NULL: the mode without D1)
    for kw in (dict(kind=4), dict(kind=-1), dict(n=0), dict(n=1025), dict(q=0), dict(q=65), dict(xx=None),
               dict(Ko=None), dict(Do=None), dict(D2o=None), dict(D2o=None, D1o=None), dict(jitter=np.nan)):
        assert call(**kw) == _lib.GPK_EINVAL, kw
    for k in range(4):
        for bad in (np.nan, np.inf):
            w = [0.1, 0.2, 0.3, 0.4]
            w[k] = bad
            assert call(w=tuple(w)) == _lib.GPK_EINVAL, (k, bad)


def test_device_solver_checks_its_arguments_before_the_library():
    from gpk.equations import Operator3
    from gpk.model_GP_solver_3d import DeviceSolver3
    ns = (4, 3, 2)
    xs = [np.linspace(0.0, 1.0, m) for m in ns]
    nb = 2 * (ns[1] * ns[2] + ns[0] * ns[2] + ns[0] * ns[1])
    src, bv = np.zeros(ns), np.zeros(nb)
    opx = dict(c2=(1.0, 1.0, 1.0), c1=(0.0, 0.0, 0.0), react=(1.0, 0.0, 0.0), faces=63)
    ok = (0.002, 0.0, 0.0)
    for bad in ((0.002, 0.0), (0.002, 0.0, 0.0, 0.0), (0.002,)):
        with pytest.raises(ValueError, match="bicross has three entries"):
            DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=opx, bicross=bad)
    with pytest.raises(ValueError, match="a mixed fourth-order partial needs"):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, bicross=ok)                     # no operator
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=Operator3((2, 2, 2), (1.0, 1.0, 1.0)), bicross=ok)
    with pytest.raises(ValueError):
        DeviceSolver3("allencahn", "SE_1d", xs, src, bv, Q=2, bicross=ok)


def test_config_listings_and_builder():
    import yaml
    from gpk import model_GP_solver_3d as m3d
    from gpk.equations import (EQUATIONS_3D, EQUATIONS_3D_OP, EQUATIONS_3D_OPB, EQUATIONS_3D_OPC, EQUATIONS_3D_OPH,
                               EQUATIONS_3D_OPM, EQUATIONS_3D_OPN, EQUATIONS_3D_OPQ, EQUATIONS_3D_OPV, EQUATIONS_3D_OPX,
                               solution_3d_opq)
    from gpk.infras.exp_config import ExpConfig
    assert EQUATIONS_3D_OPQ == ["plate_t-sin", "biharmonic_3d-sin", "swift_hohenberg_t-sin", "mixed4_3d-sin"]
    older = (set(EQUATIONS_3D) | set(EQUATIONS_3D_OP) | set(EQUATIONS_3D_OPX) | set(EQUATIONS_3D_OPV)
             | set(EQUATIONS_3D_OPN) | set(EQUATIONS_3D_OPC) | set(EQUATIONS_3D_OPM) | set(EQUATIONS_3D_OPB)
             | set(EQUATIONS_3D_OPH))
    assert not older & set(EQUATIONS_3D_OPQ)
    cdir = os.path.join(PKG_DIR, "gpk", "config3d_opq")
    assert sorted(os.listdir(cdir)) == sorted(e + ".yaml" for e in EQUATIONS_3D_OPQ)
    # the older lists and their folders keep their entries
    assert EQUATIONS_3D_OPH == ["kdv_t-sin", "ks_t-sin", "beam_t-sin"]
    assert EQUATIONS_3D_OPB == ["darcy_3d-sin", "heat_div_t-sin", "convdiff_rot_t-sin"]
    assert EQUATIONS_3D_OPM == ["aniso_heat_t-sin", "aniso_3d-sin"]
    for name, lst in (("config3d_oph", EQUATIONS_3D_OPH), ("config3d_opb", EQUATIONS_3D_OPB), ("config3d_opm", EQUATIONS_3D_OPM),
                      ("config3d_opc", EQUATIONS_3D_OPC), ("config3d_opn", EQUATIONS_3D_OPN), ("config3d_opv", EQUATIONS_3D_OPV),
                      ("config3d_opx", EQUATIONS_3D_OPX), ("config3d_op", EQUATIONS_3D_OP), ("config3d", EQUATIONS_3D)):
        assert sorted(os.listdir(os.path.join(PKG_DIR, "gpk", name))) == sorted(e + ".yaml" for e in lst), name
    with open(os.path.join(PKG_DIR, "gpk", "config3d_op", "heat_3d-sin.yaml")) as f:
        ref = yaml.safe_load(f)
    for e in EQUATIONS_3D_OPQ:
        with open(os.path.join(cdir, e + ".yaml")) as f:
            c = yaml.safe_load(f)
        assert c["equation"] == e
        assert {k: v for k, v in c.items() if k != "equation"} == {k: v for k, v in ref.items() if k != "equation"}
        assert m3d.load_config(e) == c
    args = ExpConfig()
    args.parse({"equation": "plate_t-sin", "kernel": "Matern52_Cos_1d", "nepoch": 7})
    cfg = m3d.build_config(args)
    assert cfg["equation"] == "plate_t-sin" and cfg["nepoch"] == 7 and cfg["scale"] == 1.0
    assert set(m3d.GP_solver_3d_single.opq_eq_types) == {"plate_t", "biharmonic_3d", "swift_hohenberg_t", "mixed4_3d"}
    assert set(m3d.GP_solver_3d_single.oph_eq_types) == {"kdv_t", "ks_t", "beam_t"}
    # what each entry states
    want = {"plate_t-sin": ((0.0, 0.0, 1.0), (0.0,) * 3, ((0.01, 0.01, 0.0), (0.0,) * 3), (0.02, 0.0, 0.0), (0.0,) * 3,
                            0b011111, 0b011111),
            "biharmonic_3d-sin": ((0.0,) * 3, (0.0,) * 3, ((1.0, 1.0, 1.0), (0.0,) * 3), (2.0, 2.0, 2.0), (0.0,) * 3, 63, 63),
            "swift_hohenberg_t-sin": ((0.2, 0.2, 0.0), (0.0, 0.0, 1.0), ((0.01, 0.01, 0.0), (0.0,) * 3), (0.02, 0.0, 0.0),
                                      (0.7, 0.0, 1.0), 0b011111, 0b001111),
            "mixed4_3d-sin": ((-1.0,) * 3, (0.0,) * 3, ((0.0,) * 3, (0.0,) * 3), (0.01,) * 3, (0.0,) * 3, 63, 0)}
    for e in EQUATIONS_3D_OPQ:
        _, _, op, dfaces, _, conv, cross, drift, high, bq = solution_3d_opq(e)
        got = (op.c2, op.c1, tuple(map(tuple, high)), tuple(bq), op.react, op.faces, dfaces)
        for g, w in zip(got, want[e]):
            assert np.allclose(np.asarray(g, float), np.asarray(w, float), rtol=1e-15, atol=0), (e, g, w)


def test_model_class_refuses_eq_residual_with_high_order_terms_and_a_bi_pair():
    from gpk.model_GP_solver_3d import GP_solver_3d_single
    m = GP_solver_3d_single.__new__(GP_solver_3d_single)
    m.operator, m.high, m.bicross = object(), ((0.01, 0.01, 0.0), (0.0, 0.0, 0.0)), (0.02, 0.0, 0.0)
    with pytest.raises(ValueError, match="derivatives above 2"):
        m.eq_residual(None, None, None)


# ---- the yardstick's own rounding on the GPU tests' problems ---------------------------------------
def test_numpy_yardstick_rounding_of_the_chained_term_is_a_tenth_of_the_gpu_bar():
    """tests/test_gpu_kron3_opq.py compares the device with the fp64 NumPy yardstick under the project's bar
    max(1e-10, 50 cond eps).  The new term chains two LU solves and four products per pair, DD_k x_k
    K_k^{-1} x_k DD_j x_j K_j^{-1} x_j U, so its own fp64 rounding is measured here on those tests'
    problems ((33, 20, 9), Q = 4, seed 3, problem_3d's defaults and the unit cube, all four kinds): the
    chain from the fp64 LU solves against the same chain, from the same fp64 blocks, in 50-digit
    mpmath, relative in the max norm, must stay within a tenth of the bar.  (The term is separable:
    M_j = DD_j K_j^{-1} per axis, applied along modes j and k; the 50-digit side forms M_j with an mpmath
    inverse and the products in mpmath.)"""
    import mpmath as mp
    from oracle import gp_oracle as O
    from oracle.gp_oracle import _lu, _mode_solve, mode_product
    from tests.operator3m_ref import PAIRS
    from tests.test_gpu_kron3 import KINDS, _tol
    from tests.test_gpu_kron3_operator import _problem
    mp.mp.dps = 50
    ns = (33, 20, 9)
    worst = 0.0
    for kind in KINDS:
        for unit in (False, True):
            prob, params, _ = _problem(ns, kind, 4, 3, unit)
            tol = _tol(prob, params)
            xs = [np.asarray(prob[f"x{a}"], np.float64).reshape(-1) for a in (1, 2, 3)]
            kps = [params[f"kernel_paras_{a}"] for a in (1, 2, 3)]
            Ks = [O.kernel_matrix(kind, xs[k], kps[k], prob["jitter"]) for k in range(3)]
            DD = [O.kernel_block(kind, xs[k], xs[k], kps[k], 2) for k in range(3)]
            lus = [_lu(K) for K in Ks]
            U = np.asarray(params["U"], np.float64).reshape(ns)
            # M_k = DD_k K_k^{-1} in 50 digits (cond K_k <= 1e10 leaves some forty of them)
            Mm = [mp.matrix(DD[k].tolist()) * mp.inverse(mp.matrix(Ks[k].tolist())) for k in range(3)]
            for j, k in PAIRS:
                H = _mode_solve(lus[k], mode_product(DD[j], _mode_solve(lus[j], U, j), j), k)
                got = mode_product(DD[k], H, k)
                # the same chain in mpmath: (M_k x_k (M_j x_j U)), slab by slab over the third axis l
                l = 3 - j - k
                ref = np.zeros(ns)
                for i in range(ns[l]):
                    Ul = np.take(U, i, axis=l)          # [n_j, n_k] (j < k)
                    W = Mm[j] * mp.matrix(Ul.tolist()) * Mm[k].T
                    Wn = np.array([[float(W[a, b]) for b in range(ns[k])] for a in range(ns[j])])
                    idx = [slice(None)] * 3
                    idx[l] = i
                    ref[tuple(idx)] = Wn
                err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
                worst = max(worst, err / tol)
                print(kind, "unit" if unit else "2pi", "pair", (j + 1, k + 1), "err %.3g tol %.3g" % (err, tol))
                assert err < 0.1 * tol, (kind, unit, j, k, err, tol)
    print("worst yardstick rounding of u_jjkk / bar: %.3g" % worst)
