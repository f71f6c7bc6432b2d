"""Host-side surface of the quadratic gradient terms (no GPU): header and ctypes entries, the struct
layout, every argument error of gpk_create3_opg (all returned before a device is touched), the Python
layer's own checks, the new configs and the older lists and folders unchanged."""
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
    for must in ("gpk_create3_opg", "gpk_gradsq_info3"):
        assert must in header_functions() and must in _lib.EXPORTS and hasattr(lib, must)
    assert lib.gpk_abi_version() == 2
    with open(os.path.join(ROOT, "include", "gpk.h")) as f:
        header = " ".join(f.read().replace("*", " ").split())
    for formula in ("P_k = D1_k x_k A_k", "N = g_1 P_1 + g_3 P_3 + g_2 P_2",
                    "Gamma = s_1 P_1^2 + s_3 P_3^2 + s_2 P_2^2 + x_13 P_1 P_3 + x_12 P_1 P_2 + x_23 P_2 P_3",
                    "Q_k = (g_k U + 2 s_k P_k + sum_{j != k} x_jk P_j) . R", "T_k += D1_k^T x_k Q_k",
                    "G_D1k = v Q_k,(k) A_k,(k)^T", "dL/dU += v N . R"):
        assert formula in header, formula
    # the weights are constants, said as gpk_conv3 says it
    assert "THE WEIGHTS ARE CONSTANTS" in header and "never this term" in header
    for limit in ("fields on s and x", "terms cubic in grad u", "products with second derivatives",
                  "the conservative form", "1-axis and 2-axis handles"):
        assert limit in header, limit


def test_gradsq3_struct_layout_matches_header(tmp_path):
    from gpk._lib import gpk_gradsq3
    assert [f for f, _ in gpk_gradsq3._fields_] == ["s", "x"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpk.h"\nint main(void){\n'
                     'printf("sizeof %zu\\n", sizeof(gpk_gradsq3));\n'
                     'printf("s %zu\\n", offsetof(gpk_gradsq3, s));\n'
                     'printf("x %zu\\n", offsetof(gpk_gradsq3, x));\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(gpk_gradsq3) == 48
    assert int(out["s"]) == gpk_gradsq3.s.offset == 0
    assert int(out["x"]) == gpk_gradsq3.x.offset == 24


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
    gq = _lib.gpk_gradsq3()
    gq.s[:], gq.x[:] = (0.5, 0.0, -0.25), (0.0, 0.3, 0.0)

    def call(pp=p, cc=c, ff=None, bb=None, vv=None, mm=None, dd=None, hh=None, qq=None, gg=gq, out=h):
        """GPK_EINVAL from the argument checks, or 'device': the call passed them all and failed at
        the device check that follows."""
        ref = lambda x: None if x is None else ctypes.byref(x)
        rc = lib.gpk_create3_opg(ref(pp), ref(cc), ref(ff), ref(bb), ref(vv), ref(mm), ref(dd), ref(hh), ref(qq),
                                 ref(gg), 1.0, ref(out))
        assert rc != _lib.GPK_OK
        return "device" if b"device" in lib.gpk_last_error() else rc

    zero = _lib.gpk_gradsq3()
    for gg in (gq, zero, None):  # (zeros and NULL: the gpk_create3_opq route)
        for qq in (bq, _lib.gpk_bicross3(), None):
            for hh in (hi, None):
                for dd in (dr, None):
                    for mm, vv in ((mx, cv), (mx, None), (None, cv), (None, None)):
                        for kw in (dict(pp=None), dict(cc=None), dict(out=None)):
                            assert call(gg=gg, qq=qq, hh=hh, dd=dd, mm=mm, vv=vv, **kw) == _lib.GPK_EINVAL
                            assert call(gg=gg, qq=qq, hh=hh, dd=dd, mm=mm, vv=vv, bb=bd, **kw) == _lib.GPK_EINVAL
                        assert call(gg=gg, qq=qq, hh=hh, dd=dd, mm=mm, vv=vv) == "device"
                        assert call(gg=gg, qq=qq, hh=hh, dd=dd, mm=mm, vv=vv, bb=bd) == "device"
    # a non-finite weight in each of the six positions, alone and next to non-zero others
    others = (dict(), dict(vv=cv), dict(mm=mx, dd=dr), dict(vv=cv, mm=mx, bb=bd, dd=dr, hh=hi, qq=bq))
    for field_name in ("s", "x"):
        for t in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                for base in (gq, zero):  # next to non-zero weights of its own, and alone
                    g2 = _lib.gpk_gradsq3()
                    g2.s[:], g2.x[:] = base.s[:], base.x[:]
                    getattr(g2, field_name)[t] = bad
                    for kw in others:
                        assert call(gg=g2, **kw) == _lib.GPK_EINVAL, (field_name, t, bad)
                        assert b"s and x must be finite" in lib.gpk_last_error()
    # everything the older create calls reject, next to a quadratic gradient weight
    q2 = _lib.gpk_bicross3()
    q2.q[:] = (0.0, np.nan, 0.0)
    assert call(qq=q2) == _lib.GPK_EINVAL and b"q must be finite" in lib.gpk_last_error()
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
    assert lib.gpk_gradsq_info3(None, ctypes.cast(z3, dp), ctypes.cast(z3, dp)) == _lib.GPK_EINVAL
    del keep


def test_device_solver_checks_its_arguments_before_the_library():
    from gpk.equations import Operator3
    from gpk.model_GP_solver_3d import DeviceSolver3
    ns = (4, 3, 2)
    xs = [np.linspace(0.0, 1.0, m) for m in ns]
    nb = 2 * (ns[1] * ns[2] + ns[0] * ns[2] + ns[0] * ns[1])
    src, bv = np.zeros(ns), np.zeros(nb)
    opx = dict(c2=(1.0, 1.0, 1.0), c1=(0.0, 0.0, 0.0), react=(1.0, 0.0, 0.0), faces=63)
    ok = ((0.5, 0.0, 0.0), (0.0, 0.0, 0.0))
    for bad in ((0.5, 0.0, 0.0), ((0.5, 0.0, 0.0),), ((0.5, 0.0), (0.0, 0.0, 0.0)), ((0.5, 0.0, 0.0), (0.0,) * 4),
                (ok[0], ok[1], ok[1])):
        with pytest.raises(ValueError, match="gradsq has two entries"):
            DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=opx, gradsq=bad)
    with pytest.raises(ValueError, match="a quadratic gradient term needs"):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, gradsq=ok)                     # no operator
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=Operator3((2, 2, 2), (1.0, 1.0, 1.0)), gradsq=ok)
    with pytest.raises(ValueError):
        DeviceSolver3("allencahn", "SE_1d", xs, src, bv, Q=2, gradsq=ok)


def test_config_listings_and_builder():
    import yaml
    from gpk import model_GP_solver_3d as m3d
    from gpk.equations import (EQUATIONS_3D, EQUATIONS_3D_OP, EQUATIONS_3D_OPB, EQUATIONS_3D_OPC, EQUATIONS_3D_OPG,
                               EQUATIONS_3D_OPH, EQUATIONS_3D_OPM, EQUATIONS_3D_OPN, EQUATIONS_3D_OPQ, EQUATIONS_3D_OPV,
                               EQUATIONS_3D_OPX, solution_3d_opg)
    from gpk.infras.exp_config import ExpConfig
    assert EQUATIONS_3D_OPG == ["eikonal_3d-sin", "hj_t-sin", "kpz_t-sin", "aniso_eikonal_3d-sin", "ks_int_t-sin"]
    older = (set(EQUATIONS_3D) | set(EQUATIONS_3D_OP) | set(EQUATIONS_3D_OPX) | set(EQUATIONS_3D_OPV)
             | set(EQUATIONS_3D_OPN) | set(EQUATIONS_3D_OPC) | set(EQUATIONS_3D_OPM) | set(EQUATIONS_3D_OPB)
             | set(EQUATIONS_3D_OPH) | set(EQUATIONS_3D_OPQ))
    assert not older & set(EQUATIONS_3D_OPG)
    cdir = os.path.join(PKG_DIR, "gpk", "config3d_opg")
    assert sorted(os.listdir(cdir)) == sorted(e + ".yaml" for e in EQUATIONS_3D_OPG)
    # the older lists and their folders keep their entries
    assert EQUATIONS_3D_OPQ == ["plate_t-sin", "biharmonic_3d-sin", "swift_hohenberg_t-sin", "mixed4_3d-sin"]
    assert EQUATIONS_3D_OPH == ["kdv_t-sin", "ks_t-sin", "beam_t-sin"]
    assert EQUATIONS_3D_OPB == ["darcy_3d-sin", "heat_div_t-sin", "convdiff_rot_t-sin"]
    assert EQUATIONS_3D_OPM == ["aniso_heat_t-sin", "aniso_3d-sin"]
    assert EQUATIONS_3D_OPC == ["burgers_t-sin", "burgers_3d-sin"]
    for name, lst in (("config3d_opq", EQUATIONS_3D_OPQ), ("config3d_oph", EQUATIONS_3D_OPH), ("config3d_opb", EQUATIONS_3D_OPB),
                      ("config3d_opm", EQUATIONS_3D_OPM), ("config3d_opc", EQUATIONS_3D_OPC), ("config3d_opn", EQUATIONS_3D_OPN),
                      ("config3d_opv", EQUATIONS_3D_OPV), ("config3d_opx", EQUATIONS_3D_OPX), ("config3d_op", EQUATIONS_3D_OP),
                      ("config3d", EQUATIONS_3D)):
        assert sorted(os.listdir(os.path.join(PKG_DIR, "gpk", name))) == sorted(e + ".yaml" for e in lst), name
    with open(os.path.join(PKG_DIR, "gpk", "config3d_op", "heat_3d-sin.yaml")) as f:
        ref = yaml.safe_load(f)
    for e in EQUATIONS_3D_OPG:
        with open(os.path.join(cdir, e + ".yaml")) as f:
            c = yaml.safe_load(f)
        assert c["equation"] == e
        assert {k: v for k, v in c.items() if k != "equation"} == {k: v for k, v in ref.items() if k != "equation"}
        assert m3d.load_config(e) == c
    args = ExpConfig()
    args.parse({"equation": "hj_t-sin", "kernel": "Matern52_Cos_1d", "nepoch": 7})
    cfg = m3d.build_config(args)
    assert cfg["equation"] == "hj_t-sin" and cfg["nepoch"] == 7 and cfg["scale"] == 1.0
    assert set(m3d.GP_solver_3d_single.opg_eq_types) == {"eikonal_3d", "hj_t", "kpz_t", "aniso_eikonal_3d", "ks_int_t"}
    assert set(m3d.GP_solver_3d_single.opq_eq_types) == {"plate_t", "biharmonic_3d", "swift_hohenberg_t", "mixed4_3d"}
    # what each entry states: c2, c1, high, bicross, react, faces, dfaces, gradsq
    Z = (0.0,) * 3
    want = {"eikonal_3d-sin": ((-0.1,) * 3, Z, (Z, Z), Z, Z, 63, 0, ((1.0, 1.0, 1.0), Z)),
            "hj_t-sin": ((-0.05, -0.05, 0.0), (0.0, 0.0, 1.0), (Z, Z), Z, Z, 0b011111, 0, ((0.5, 0.5, 0.0), Z)),
            "kpz_t-sin": ((-0.05, -0.05, 0.0), (0.0, 0.0, 1.0), (Z, Z), Z, Z, 0b011111, 0, ((-0.5, -0.5, 0.0), Z)),
            "aniso_eikonal_3d-sin": ((-0.1,) * 3, Z, (Z, Z), Z, Z, 63, 0, ((1.0, 0.5, 2.0), (0.6, 0.0, -0.4))),
            "ks_int_t-sin": ((0.2, 0.2, 0.0), (0.0, 0.0, 1.0), ((0.01, 0.01, 0.0), Z), (0.02, 0.0, 0.0), Z, 0b011111,
                             0b001111, ((0.5, 0.5, 0.0), Z))}
    for e in EQUATIONS_3D_OPG:
        _, _, op, dfaces, _, conv, cross, drift, high, bq, gq = solution_3d_opg(e)
        assert not any(conv) and not any(cross) and all(b is None for b in drift)
        got = (op.c2, op.c1, tuple(map(tuple, high)), tuple(bq), op.react, op.faces, dfaces, tuple(map(tuple, gq)))
        for g, w in zip(got, want[e]):
            assert np.allclose(np.asarray(g, float), np.asarray(w, float), rtol=1e-15, atol=0), (e, g, w)


def test_model_class_reads_gradsq_from_trick_paras_or_the_name():
    """GP_solver_3d_single's bookkeeping up to the device: trick_paras['gradsq'] wins, else the equation's."""
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single

    class NoDevice(GP_solver_3d_single):
        def _make_device(self, device=0):
            pass
    xs = [np.linspace(0.0, 1.0, 4)] * 3
    tp = {"kernel": kernel_class("SE_1d"), "equation": "aniso_eikonal_3d-sin", "llk_weight": 200.0}
    nb = 6 * 16
    m = NoDevice(np.zeros(nb), xs, np.zeros((4, 4, 4)), 1e-6, tp)
    assert m.gradsq == ((1.0, 0.5, 2.0), (0.6, 0.0, -0.4)) and m.bicross == (0.0, 0.0, 0.0) and m.dfaces == 0
    m = NoDevice(np.zeros(nb), xs, np.zeros((4, 4, 4)), 1e-6, dict(tp, gradsq=((2.0, 0, 0), (0, 0, 1))))
    assert m.gradsq == ((2.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    m = NoDevice(np.zeros(nb), xs, np.zeros((4, 4, 4)), 1e-6, dict(tp, equation="ks_int_t-sin"))
    assert m.gradsq == ((0.5, 0.5, 0.0), (0.0, 0.0, 0.0)) and m.dfaces == 0b001111 and m.dvals is not None
    with pytest.raises(ValueError, match="derivatives above 2"):
        m.eq_residual(None, None, None)


def test_cli_accepts_the_new_names():
    from gpk import model_GP_solver_3d as m3d
    from gpk.cli import parse_flags
    from gpk.equations import EQUATIONS_3D_OPG
    from gpk.infras.exp_config import ExpConfig
    for e in EQUATIONS_3D_OPG:
        args = ExpConfig()
        args.parse(parse_flags(["-equation=%s" % e, "-kernel=Matern52_Cos_1d", "-nepoch=3"]))
        assert m3d.build_config(args)["equation"] == e
