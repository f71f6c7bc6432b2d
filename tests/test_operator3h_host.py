"""Host-side surface of the third- and fourth-order terms (no GPU): header and ctypes entries, the
struct layout, every argument error of gpk_create3_oph and gpk_assemble_pairs4 (all returned before a
device is touched), the Python layer's own checks, the new configs, the manufactured sources of
equations.EQUATIONS_3D_OPH, and the rounding of the NumPy yardstick on the GPU tests' own problems."""
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
    for must in ("gpk_create3_oph", "gpk_high_info3", "gpk_assemble_pairs4"):
        assert must in header_functions() and must in _lib.EXPORTS and hasattr(lib, must)
    assert lib.gpk_abi_version() == 2
    with open(os.path.join(ROOT, "include", "gpk.h")) as f:
        header = " ".join(f.read().replace("*", " ").split())
    assert "c4_k d^4 u / d x_k^4 + c3_k d^3 u / d x_k^3" in header
    assert "D_k = c4_k D4_k + c3_k D3_k + c2_k DD_k + c1_k D1_k" in header
    assert "ORDER 4 IS THE CEILING" in header and "no fifth derivative" in header
    for limit in ("orders above four", "u_xxyy", "second derivatives (simply supported ends)", "the class path",
                  "keep rejecting 3"):
        assert limit in header, limit


def test_high3_struct_layout_matches_header(tmp_path):
    from gpk._lib import gpk_high3
    assert [f for f, _ in gpk_high3._fields_] == ["c4", "c3"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpk.h"\nint main(void){\n'
                     'printf("sizeof %zu\\n", sizeof(gpk_high3));\n'
                     'printf("c4 %zu\\n", offsetof(gpk_high3, c4));\n'
                     'printf("c3 %zu\\n", offsetof(gpk_high3, c3));\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(gpk_high3) == 48
    assert int(out["c4"]) == gpk_high3.c4.offset == 0 and int(out["c3"]) == gpk_high3.c3.offset == 24


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

    def call(pp=p, cc=c, ff=None, bb=None, vv=None, mm=None, dd=None, hh=hi, out=h):
        """GPK_EINVAL from the argument checks, or 'device': the call passed them all and failed at
        the device check that follows."""
        ref = lambda x: None if x is None else ctypes.byref(x)
        rc = lib.gpk_create3_oph(ref(pp), ref(cc), ref(ff), ref(bb), ref(vv), ref(mm), ref(dd), ref(hh), 1.0, ref(out))
        assert rc != _lib.GPK_OK
        return "device" if b"device" in lib.gpk_last_error() else rc

    zero = _lib.gpk_high3()
    for hh in (hi, zero, None):  # (zeros and NULL: the gpk_create3_opb route)
        for dd in (dr, None):
            for mm in (mx, None):
                for vv in (cv, None):
                    for kw in (dict(pp=None), dict(cc=None), dict(out=None)):
                        assert call(hh=hh, dd=dd, mm=mm, vv=vv, **kw) == _lib.GPK_EINVAL
                        assert call(hh=hh, dd=dd, mm=mm, vv=vv, bb=bd, **kw) == _lib.GPK_EINVAL
                    assert call(hh=hh, dd=dd, mm=mm, vv=vv) == "device"
                    assert call(hh=hh, dd=dd, mm=mm, vv=vv, bb=bd) == "device"
    # a non-finite weight in every slot, alone and next to everything else
    for name in ("c4", "c3"):
        for k in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                h2 = _lib.gpk_high3()
                h2.c4[:], h2.c3[:] = hi.c4[:], hi.c3[:]
                getattr(h2, name)[k] = bad
                for kw in (dict(), dict(vv=cv), dict(mm=mx, dd=dr), dict(vv=cv, mm=mx, bb=bd, dd=dr)):
                    assert call(hh=h2, **kw) == _lib.GPK_EINVAL, (name, k, bad)
                    assert b"c4 and c3 must be finite" in lib.gpk_last_error()
    # everything the older create calls reject, next to a high-order weight
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
    assert lib.gpk_high_info3(None, ctypes.cast(z3, dp), ctypes.cast(z3, dp)) == _lib.GPK_EINVAL
    del keep


def test_assemble_pairs4_argument_errors_without_a_device():
    from gpk import _lib
    from gpk._lib import dptr
    lib = _lib.load()
    x = np.linspace(0.0, 1.0, 5)
    kp = [np.zeros(2), np.zeros(2), np.ones(2)]
    K, D, D1 = (np.empty((5, 5)) for _ in range(3))

    def call(kind=1, xx=x, n=5, q=2, jitter=1e-6, w=(0.1, 0.2, 0.3, 0.4), Ko=K, Do=D, D1o=D1):
        opt = lambda a: None if a is None else dptr(a)
        rc = lib.gpk_assemble_pairs4(kind, opt(xx), n, dptr(kp[0]), dptr(kp[1]), dptr(kp[2]), q, jitter, *w,
                                     opt(Ko), opt(Do), opt(D1o))
        assert rc != _lib.GPK_OK
        return "device" if b"device" in lib.gpk_last_error() else rc

    assert call() == "device" and call(D1o=None) == "device"  # (D1_out NULL: the plain mode)
    for kw in (dict(kind=4), dict(kind=-1), dict(n=0), dict(n=1025), dict(q=0), dict(q=65), dict(xx=None),
               dict(Ko=None), dict(Do=None), dict(jitter=np.nan)):
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
    ok = ((0.01, 0.0, 0.0), (0.0, 0.2, 0.0))
    for bad in (((0.01, 0.0, 0.0),), ((0.01, 0.0), (0.0, 0.2, 0.0)), ((0.01, 0.0, 0.0), (0.2,)),
                ((0.01, 0.0, 0.0), (0.0, 0.2, 0.0), (0.0, 0.0, 0.0))):
        with pytest.raises(ValueError):
            DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=opx, high=bad)
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, high=ok)                     # no operator
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=Operator3((2, 2, 2), (1.0, 1.0, 1.0)), high=ok)
    with pytest.raises(ValueError):
        DeviceSolver3("allencahn", "SE_1d", xs, src, bv, Q=2, high=ok)


def test_config_listings_and_builder():
    import yaml
    from gpk import model_GP_solver_3d as m3d
    from gpk.equations import (EQUATIONS_3D, EQUATIONS_3D_OP, EQUATIONS_3D_OPB, EQUATIONS_3D_OPC, EQUATIONS_3D_OPH,
                               EQUATIONS_3D_OPM, EQUATIONS_3D_OPN, EQUATIONS_3D_OPV, EQUATIONS_3D_OPX)
    from gpk.infras.exp_config import ExpConfig
    assert EQUATIONS_3D_OPH == ["kdv_t-sin", "ks_t-sin", "beam_t-sin"]
    older = (set(EQUATIONS_3D) | set(EQUATIONS_3D_OP) | set(EQUATIONS_3D_OPX) | set(EQUATIONS_3D_OPV)
             | set(EQUATIONS_3D_OPN) | set(EQUATIONS_3D_OPC) | set(EQUATIONS_3D_OPM) | set(EQUATIONS_3D_OPB))
    assert not older & set(EQUATIONS_3D_OPH)
    cdir = os.path.join(PKG_DIR, "gpk", "config3d_oph")
    assert sorted(os.listdir(cdir)) == sorted(e + ".yaml" for e in EQUATIONS_3D_OPH)
    assert EQUATIONS_3D_OPB == ["darcy_3d-sin", "heat_div_t-sin", "convdiff_rot_t-sin"]
    assert sorted(os.listdir(os.path.join(PKG_DIR, "gpk", "config3d_opb"))) == sorted(e + ".yaml" for e in EQUATIONS_3D_OPB)
    with open(os.path.join(PKG_DIR, "gpk", "config3d_op", "heat_3d-sin.yaml")) as f:
        ref = yaml.safe_load(f)
    for e in EQUATIONS_3D_OPH:
        with open(os.path.join(cdir, e + ".yaml")) as f:
            c = yaml.safe_load(f)
        assert c["equation"] == e
        assert {k: v for k, v in c.items() if k != "equation"} == {k: v for k, v in ref.items() if k != "equation"}
        assert m3d.load_config(e) == c
    args = ExpConfig()
    args.parse({"equation": "kdv_t-sin", "kernel": "Matern52_Cos_1d", "nepoch": 7})
    cfg = m3d.build_config(args)
    assert cfg["equation"] == "kdv_t-sin" and cfg["nepoch"] == 7 and cfg["scale"] == 1.0
    assert set(m3d.GP_solver_3d_single.oph_eq_types) == {"kdv_t", "ks_t", "beam_t"}
    assert set(m3d.GP_solver_3d_single.opb_eq_types) == {"darcy_3d", "heat_div_t", "convdiff_rot_t"}


def test_oph_equation_sources_are_the_operator_applied_to_u():
    """src = sum_k (c4_k d^4 + c3_k d^3 + c2_k d^2 + c1_k d) u / dx_k + u sum_k g_k du / dx_k and grad_u =
    grad u at random points, by torch autograd of the solution, to 1e-9 (fourth derivatives of
    sin(2x) sin(3y): magnitudes up to 16)."""
    import torch
    from gpk import equations as E
    sin, exp = torch.sin, torch.exp
    tu = {"kdv_t-sin": lambda x, y, t: exp(-t) * sin(2 * x) * sin(3 * y),
          "ks_t-sin": lambda x, y, t: exp(-t) * sin(2 * x) * sin(3 * y),
          "beam_t-sin": lambda x, y, t: sin(2 * x) * sin(3 * y) * sin(2.0 * t + 0.5)}
    want = {"kdv_t-sin": (((0.0,) * 3, (0.01, 0.0, 0.0)), (1.0, 0.0, 0.0), 0),
            "ks_t-sin": (((0.02, 0.0, 0.0), (0.0,) * 3), (1.0, 0.0, 0.0), 0),
            "beam_t-sin": (((0.01, 0.0, 0.0), (0.0,) * 3), (0.0, 0.0, 0.0), 0b010011)}
    pts = np.random.default_rng(0).uniform(0.05, 0.95, size=(40, 3))
    for e in E.EQUATIONS_3D_OPH:
        u, src, op, dfaces, grad_u, conv, cross, drift, high = E.solution_3d_oph(e)
        assert (tuple(map(tuple, high)), tuple(conv), dfaces) == want[e]
        assert not any(cross) and all(b is None for b in drift) and op.faces == 0b011111
        X = [torch.tensor(pts[:, k], requires_grad=True) for k in range(3)]
        uu = tu[e](*X)
        assert np.allclose(uu.detach().numpy(), u(*pts.T), rtol=0, atol=1e-15)
        lhs = op.react[0] * uu + op.react[1] * uu ** 2 + op.react[2] * uu ** 3
        for k in range(3):
            ds, g = [], uu
            for _ in range(4):
                g, = torch.autograd.grad(g.sum(), X[k], create_graph=True)
                ds.append(g)
            lhs = lhs + high[0][k] * ds[3] + high[1][k] * ds[2] + op.c2[k] * ds[1] + op.c1[k] * ds[0]
            lhs = lhs + conv[k] * uu * ds[0]
            gerr = float(np.max(np.abs(ds[0].detach().numpy() - grad_u[k](*pts.T))))
            assert gerr < 1e-10, (e, k, gerr)
        err = float(np.max(np.abs(lhs.detach().numpy() - src(*pts.T))))
        print(e, "source err", err)
        assert err < 1e-9


def test_model_class_refuses_eq_residual_with_high_order_terms():
    """eq_residual needs derivatives above 2 on the test mesh: ValueError before any device work (the
    check stands in front of the first device call)."""
    from gpk.model_GP_solver_3d import GP_solver_3d_single
    m = GP_solver_3d_single.__new__(GP_solver_3d_single)
    m.operator, m.high = object(), ((0.01, 0.0, 0.0), (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="derivatives above 2"):
        m.eq_residual(None, None, None)


# ---- the yardstick's own rounding on the GPU tests' problems ---------------------------------------
def test_numpy_yardstick_rounding_is_a_tenth_of_the_gpu_bar():
    """tests/test_gpu_kron3_oph.py compares the device with the fp64 NumPy yardstick under the
    project's bar max(1e-10, 50 cond eps).  Order-4 blocks scale with om^4, so the yardstick's own
    fp64 rounding is measured here on those tests' problems (problem_3d's defaults: x in [0, 2 pi],
    fs = 5, and the unit cube of the refinement test): every order-3 and order-4 block and their
    parameter-gradient contraction in fp64 against the same expressions in long double (11 more
    bits), relative in the max norm, must stay within a tenth of the bar."""
    from oracle import gp_oracle as O
    from tests.operator3h_ref import kernel_kd_high, param_grad_contract_high
    from tests.test_gpu_kron3 import KINDS, _tol
    from tests.test_gpu_kron3_operator import _problem
    worst = 0.0
    for ns, kind, Q, unit in [((33, 20, 9), "Matern52_Cos_1d", 4, False), ((9, 20, 33), "Matern52_Cos_1d", 4, False),
                              ((33, 20, 9), "Matern52_Cos_1d", 4, True), ((24, 18, 12), "Matern52_Cos_1d", 5, False)] + \
            [((20, 14, 9), k, 4, False) for k in KINDS] + [((20, 14, 9), "Matern52_Cos_1d", 64, False)]:
        prob, params, _ = _problem(ns, kind, Q, 8 if Q == 5 else 3, unit)
        tol = _tol(prob, params)
        rng = np.random.default_rng(1)
        for a in (1, 2, 3):
            x, kp = prob[f"x{a}"], params[f"kernel_paras_{a}"]
            D4, D3 = kernel_kd_high(kind, x, kp)
            L4, L3 = kernel_kd_high(kind, x, kp, np.longdouble)
            G4, G3 = rng.normal(size=D4.shape), rng.normal(size=D4.shape)
            g, gl = param_grad_contract_high(kind, x, kp, G4, G3), param_grad_contract_high(kind, x, kp, G4, G3, np.longdouble)
            errs = [float(np.max(np.abs(D4 - L4)) / np.max(np.abs(L4))), float(np.max(np.abs(D3 - L3)) / np.max(np.abs(L3)))]
            for key in g:
                if np.max(np.abs(gl[key])) > 0:
                    errs.append(float(np.max(np.abs(g[key] - gl[key])) / np.max(np.abs(gl[key]))))
            worst = max(worst, max(errs) / tol)
            assert max(errs) < 0.1 * tol, (ns, kind, Q, unit, a, errs, tol)
    print("worst yardstick rounding / bar: %.3g" % worst)
