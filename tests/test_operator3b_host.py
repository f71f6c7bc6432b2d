"""Host-side surface of the drift fields (no GPU): header and ctypes entries, the struct layout,
every argument error of gpk_create3_opb (all returned before a device is touched), the new configs,
and the Python layer's own checks; the existing 3-axis lists and folders are as they were."""
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
    for must in ("gpk_create3_opb", "gpk_drift_info3"):
        assert must in header_functions() and must in _lib.EXPORTS and hasattr(lib, must)
    assert lib.gpk_abi_version() == 2
    with open(os.path.join(ROOT, "include", "gpk.h")) as f:
        header = " ".join(f.read().replace("*", " ").split())
    # the term, the sum's order, that the coefficient fields do not multiply it, and the launch count
    assert "b_k(x) . d u / d x_k" in header and "b_1 . Z_1 + b_3 . Z_3 + b_2 . Z_2" in header
    assert "FIELDS a_k DO NOT MULTIPLY THE DRIFT TERM" in header
    assert "two or three further GEMM launches" in header


def test_drift3_struct_layout_matches_header(tmp_path):
    from gpk._lib import gpk_drift3
    assert [f for f, _ in gpk_drift3._fields_] == ["b"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpk.h"\nint main(void){\n'
                     'printf("sizeof %zu\\n", sizeof(gpk_drift3));\n'
                     'printf("b %zu\\n", offsetof(gpk_drift3, b));\n'
                     'printf("b2 %zu\\n", offsetof(gpk_drift3, b[2]));\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(gpk_drift3) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert int(out["b"]) == gpk_drift3.b.offset == 0 and int(out["b2"]) == 2 * ctypes.sizeof(ctypes.c_void_p)


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
    good = [np.linspace(-1.0, 1.0, n) + 0.1 * k for k in range(3)]

    def drift(fields):
        d = _lib.gpk_drift3()
        for k, f in enumerate(fields):
            if f is not None:
                d.b[k] = dptr(f)
        return d

    dr = drift(good)

    def call(pp=p, cc=c, ff=None, bb=None, vv=None, mm=None, dd=dr, out=h):
        """GPK_EINVAL from the argument checks, or 'device': the call passed them all and failed
        at the device check that follows."""
        ref = lambda x: None if x is None else ctypes.byref(x)
        rc = lib.gpk_create3_opb(ref(pp), ref(cc), ref(ff), ref(bb), ref(vv), ref(mm), ref(dd), 1.0, ref(out))
        assert rc != _lib.GPK_OK
        return "device" if b"device" in lib.gpk_last_error() else rc

    assert call() == "device" and call(bb=bd) == "device" and call(vv=cv) == "device" and call(mm=mx) == "device"
    empty = _lib.gpk_drift3()
    for dd in (dr, drift([None, good[1], None]), empty, None):  # (empty and NULL: the gpk_create3_opm route)
        for mm in (mx, None):
            for vv in (cv, None):
                for kw in (dict(pp=None), dict(cc=None), dict(out=None)):
                    assert call(dd=dd, mm=mm, vv=vv, **kw) == _lib.GPK_EINVAL
                    assert call(dd=dd, mm=mm, vv=vv, bb=bd, **kw) == _lib.GPK_EINVAL
                assert call(dd=dd, mm=mm, vv=vv) == "device"
    # a non-finite value in each field, alone and next to conv or cross, wherever it stands
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            for at in (0, n // 2, n - 1):
                f = good[k].copy()
                f[at] = bad
                alone = [None, None, None]
                alone[k] = f
                among = list(good)
                among[k] = f
                for fields in (alone, among):
                    for kw in (dict(), dict(vv=cv), dict(mm=mx), dict(vv=cv, mm=mx, bb=bd)):
                        assert call(dd=drift(fields), **kw) == _lib.GPK_EINVAL, (k, bad, at)
                        assert b"drift field has a non-finite value" in lib.gpk_last_error()
    # the cross and convective weights' own cases next to a drift field
    m2 = _lib.gpk_cross3()
    m2.m[:] = (0.0, np.inf, 0.0)
    assert call(mm=m2) == _lib.GPK_EINVAL and b"m must be finite" in lib.gpk_last_error()
    v2 = _lib.gpk_conv3()
    v2.g[:] = (0.0, np.nan, 0.0)
    assert call(vv=v2) == _lib.GPK_EINVAL and b"g must be finite" in lib.gpk_last_error()
    # the derivative data's own cases next to a drift field
    for bad in (-1, 64):
        b2 = _lib.gpk_bdata3()
        b2.dfaces, b2.dvals = bad, dptr(dv)
        assert call(bb=b2) == _lib.GPK_EINVAL, bad
    b2 = _lib.gpk_bdata3()
    b2.dfaces = 1
    assert call(bb=b2) == _lib.GPK_EINVAL  # NULL dvals
    d2 = dv.copy()
    d2[3] = np.inf
    b2.dvals = dptr(d2)
    assert call(bb=b2) == _lib.GPK_EINVAL
    # faces: 0 needs derivative data, with or without a drift field
    c.faces = 0
    assert call() == _lib.GPK_EINVAL and call(bb=bd) == "device"
    for faces in (64, -1):
        c.faces = faces
        assert call() == _lib.GPK_EINVAL, faces
    c.faces = 0b011111
    # the operator's and the problem's own cases (the grid's size is checked before a field is read)
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
    field = np.linspace(-1.0, 1.0, n)
    field[0] = np.nan
    cf = _lib.gpk_coef3()
    cf.a[1] = dptr(field)
    assert call(ff=cf) == _lib.GPK_EINVAL
    assert call() == "device"
    assert not h.value
    assert lib.gpk_drift_info3(None, (ctypes.c_int32 * 3)()) == _lib.GPK_EINVAL
    del keep


def test_device_solver_checks_its_arguments_before_the_library():
    from gpk.equations import Operator3
    from gpk.model_GP_solver_3d import DeviceSolver3
    ns = (4, 3, 2)
    xs = [np.linspace(0.0, 1.0, m) for m in ns]
    nb = 2 * (ns[1] * ns[2] + ns[0] * ns[2] + ns[0] * ns[1])
    src, bv = np.zeros(ns), np.zeros(nb)
    b = np.ones(ns)
    opx = dict(c2=(1.0, 1.0, 1.0), c1=(0.0, 0.0, 0.0), react=(1.0, 0.0, 0.0), faces=63)
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=opx, drift=(b, None))             # two entries
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, drift=(b, None, None))                     # no operator
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=Operator3((2, 2, 2), (1.0, 1.0, 1.0)),
                      drift=(None, None, b))
    with pytest.raises(ValueError):
        DeviceSolver3("allencahn", "SE_1d", xs, src, bv, Q=2, drift=(None, b, None))
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=opx, drift=(np.ones((4, 3)), None, None))  # shape


def test_callables_and_arrays_give_equal_fields():
    from gpk.equations import divergence_drift, drift_fields, solution_3d_opb
    axes = [np.linspace(0.0, 1.0, m) for m in (5, 4, 3)]
    mesh = np.meshgrid(*axes, indexing="ij")
    for e in ("darcy_3d-sin", "heat_div_t-sin", "convdiff_rot_t-sin"):
        drift = solution_3d_opb(e)[7]
        as_arrays = tuple(None if b is None else np.asarray(b(*mesh), np.float64) * np.ones(mesh[0].shape) for b in drift)
        fa, fb = drift_fields(drift, axes), drift_fields(as_arrays, axes)
        assert [x is None for x in fa] == [b is None for b in drift]
        for x, y in zip(fa, fb):
            assert (x is None and y is None) or (x.shape == (5, 4, 3) and x.flags.c_contiguous and np.array_equal(x, y))
    # divergence_drift of arrays and of callables
    ga = (lambda x, y, z: 2.0 * x * y, lambda x, y, z: x * x + z, None)
    c2 = (-0.5, 2.0, 1.0)
    fc = drift_fields(divergence_drift(ga, c2), axes)
    fv = drift_fields(divergence_drift(tuple(None if g is None else g(*mesh) for g in ga), c2), axes)
    assert fc[2] is None and fv[2] is None
    assert np.array_equal(fc[0], fv[0]) and np.array_equal(fc[1], fv[1])
    assert np.array_equal(fc[0], -0.5 * 2.0 * mesh[0] * mesh[1])
    with pytest.raises(ValueError):
        drift_fields((np.ones((5, 4)), None, None), axes)
    with pytest.raises(ValueError):
        drift_fields((None, None), axes)


def test_config_listings_and_builder():
    import yaml
    from gpk import model_GP_solver_3d as m3d
    from gpk.equations import (EQUATIONS_3D, EQUATIONS_3D_OP, EQUATIONS_3D_OPB, EQUATIONS_3D_OPC, EQUATIONS_3D_OPM,
                               EQUATIONS_3D_OPN, EQUATIONS_3D_OPV, EQUATIONS_3D_OPX)
    from gpk.infras.exp_config import ExpConfig
    assert EQUATIONS_3D_OPB == ["darcy_3d-sin", "heat_div_t-sin", "convdiff_rot_t-sin"]
    older = (set(EQUATIONS_3D) | set(EQUATIONS_3D_OP) | set(EQUATIONS_3D_OPX) | set(EQUATIONS_3D_OPV)
             | set(EQUATIONS_3D_OPN) | set(EQUATIONS_3D_OPC) | set(EQUATIONS_3D_OPM))
    assert not older & set(EQUATIONS_3D_OPB)
    cdir = os.path.join(PKG_DIR, "gpk", "config3d_opb")
    assert sorted(os.listdir(cdir)) == sorted(e + ".yaml" for e in EQUATIONS_3D_OPB)
    # the seven existing lists and folders hold what they held
    assert EQUATIONS_3D == ["poisson_3d-mix_sin", "allencahn_3d-sin"]
    assert EQUATIONS_3D_OP == ["heat_3d-sin", "advection_3d-sin", "helmholtz_3d-sin", "allencahn_t-sin"]
    assert EQUATIONS_3D_OPX == ["convdiff_t-sin", "convdiff_3d-sin"]
    assert EQUATIONS_3D_OPV == ["helmholtz_var-sin", "heat_var-sin", "transport_var-sin"]
    assert EQUATIONS_3D_OPN == ["wave_t-sin", "helmholtz_neumann-sin"]
    assert EQUATIONS_3D_OPC == ["burgers_t-sin", "burgers_3d-sin"]
    assert EQUATIONS_3D_OPM == ["aniso_heat_t-sin", "aniso_3d-sin"]
    for d, es in (("config3d", EQUATIONS_3D), ("config3d_op", EQUATIONS_3D_OP), ("config3d_opx", EQUATIONS_3D_OPX),
                  ("config3d_opv", EQUATIONS_3D_OPV), ("config3d_opn", EQUATIONS_3D_OPN),
                  ("config3d_opc", EQUATIONS_3D_OPC), ("config3d_opm", EQUATIONS_3D_OPM)):
        assert sorted(os.listdir(os.path.join(PKG_DIR, "gpk", d))) == sorted(e + ".yaml" for e in es)
    with open(os.path.join(PKG_DIR, "gpk", "config3d_op", "heat_3d-sin.yaml")) as f:
        ref = yaml.safe_load(f)
    for e in EQUATIONS_3D_OPB:
        with open(os.path.join(cdir, e + ".yaml")) as f:
            c = yaml.safe_load(f)
        assert c["equation"] == e
        assert {k: v for k, v in c.items() if k != "equation"} == {k: v for k, v in ref.items() if k != "equation"}
        assert m3d.load_config(e) == c
    args = ExpConfig()
    args.parse({"equation": "heat_div_t-sin", "kernel": "Matern52_Cos_1d", "nepoch": 7})
    cfg = m3d.build_config(args)
    assert cfg["equation"] == "heat_div_t-sin" and cfg["nepoch"] == 7 and cfg["scale"] == 1.0
    assert set(m3d.GP_solver_3d_single.opb_eq_types) == {"darcy_3d", "heat_div_t", "convdiff_rot_t"}
    assert set(m3d.GP_solver_3d_single.opm_eq_types) == {"aniso_heat_t", "aniso_3d"}
