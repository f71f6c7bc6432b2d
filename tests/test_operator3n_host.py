"""Host-side surface of derivative boundary data (no GPU): header and ctypes entries, the struct
layout, every argument error of gpk_create3_opn (all returned before a device is touched), the new
configs, and the Python layer's own checks; the existing 3-axis lists and folders are as they were."""
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
    for must in ("gpk_create3_opn", "gpk_bdata_info3", "gpk_boundary_terms3"):
        assert must in header_functions() and must in _lib.EXPORTS and hasattr(lib, must)
    assert lib.gpk_abi_version() == 2
    with open(os.path.join(ROOT, "include", "gpk.h")) as f:
        header = f.read()
    assert "not along the outward normal" in " ".join(header.replace("*", " ").split())
    assert "Not expressible: derivative" not in header and "derivative boundary data. */" not in header


def test_bdata3_struct_layout_matches_header(tmp_path):
    from gpk._lib import gpk_bdata3
    fields = [f for f, _ in gpk_bdata3._fields_]
    assert fields == ["dfaces", "dvals"]
    probe = tmp_path / "probe.c"
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(gpk_bdata3, {f}));' for f in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpk.h"\nint main(void){\n'
                     'printf("sizeof %zu\\n", sizeof(gpk_bdata3));\n' + body + "\nreturn 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(gpk_bdata3)
    for f in fields:
        assert int(out[f]) == getattr(gpk_bdata3, f).offset, f


def test_argument_errors_without_a_device():
    from gpk import _lib
    from gpk._lib import dptr
    lib = _lib.load()
    ns = (4, 3, 2)
    p, keep, n = _valid_problem(ns)
    c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
    c.c2[:], c.c1[:], c.react[:], c.faces = (1.0, 1.0, 1.0), (0.0, 0.5, 0.0), (2.0, 0.0, 0.0), 0b011111
    nb = 2 * (ns[1] * ns[2] + ns[0] * ns[2] + ns[0] * ns[1])
    dv = np.full(nb, np.nan)
    off = {f: sum(np.zeros(ns)[sl].size for sl in _faces()[:f]) for f in range(6)}
    size = {f: np.zeros(ns)[sl].size for f, sl in enumerate(_faces())}
    dfaces = 0b010010
    for f in (1, 4):
        dv[off[f]:off[f] + size[f]] = 0.25
    bd = _lib.gpk_bdata3()
    bd.dfaces, bd.dvals = dfaces, dptr(dv)

    def call(pp=p, cc=c, ff=None, bb=bd, out=h):
        """GPK_EINVAL from the argument checks, or 'device': the call passed them all and failed
        at the device check that follows."""
        rc = lib.gpk_create3_opn(None if pp is None else ctypes.byref(pp), None if cc is None else ctypes.byref(cc),
                                 None if ff is None else ctypes.byref(ff), None if bb is None else ctypes.byref(bb),
                                 1.0, None if out is None else ctypes.byref(out))
        assert rc != _lib.GPK_OK
        return "device" if b"device" in lib.gpk_last_error() else rc

    assert call() == "device"
    for kw in (dict(pp=None), dict(cc=None), dict(out=None)):
        assert call(**kw) == _lib.GPK_EINVAL
        assert call(bb=None, **kw) == _lib.GPK_EINVAL  # (the gpk_create3_opv route)
    # dfaces outside 0..63; NULL dvals with dfaces != 0
    for bad in (-1, 64, 1 << 20):
        b2 = _lib.gpk_bdata3()
        b2.dfaces, b2.dvals = bad, dptr(dv)
        assert call(bb=b2) == _lib.GPK_EINVAL, bad
    b2 = _lib.gpk_bdata3()
    b2.dfaces = dfaces
    assert call(bb=b2) == _lib.GPK_EINVAL
    # a non-finite value on a face of dfaces, its first and last entries included; NaN elsewhere is fine
    for f in (1, 4):
        for idx, bad in ((0, np.nan), (size[f] // 2, np.inf), (size[f] - 1, -np.inf)):
            d2 = dv.copy()
            d2[off[f] + idx] = bad
            b2 = _lib.gpk_bdata3()
            b2.dfaces, b2.dvals = dfaces, dptr(d2)
            assert call(bb=b2) == _lib.GPK_EINVAL, (f, idx)
            assert b"not finite" in lib.gpk_last_error()
    # faces: 0 is allowed next to derivative data, 64 and -1 are not; without it the opv rule holds
    c.faces = 0
    assert call() == "device"
    assert call(bb=None) == _lib.GPK_EINVAL
    b0 = _lib.gpk_bdata3()
    b0.dvals = dptr(dv)
    assert call(bb=b0) == _lib.GPK_EINVAL  # dfaces == 0: gpk_create3_opv itself, faces in 1..63
    for faces in (64, -1):
        c.faces = faces
        assert call() == _lib.GPK_EINVAL, faces
    c.faces = 0b011111
    # the operator's and the problem's own cases
    c.c1[1] = float("nan")
    assert call() == _lib.GPK_EINVAL
    c.c1[1] = 0.5
    p.eq = _lib.EQ_IDS["allencahn"]
    assert call() == _lib.GPK_EINVAL
    p.eq = _lib.EQ_IDS["poisson"]
    for name, bad in (("kind", 4), ("q", 0), ("n1", 1), ("n3", 1025)):
        good = getattr(p, name)
        setattr(p, name, bad)
        assert call() == _lib.GPK_EINVAL, (name, bad)
        setattr(p, name, good)
    # a non-finite coefficient field
    field = np.linspace(-1.0, 1.0, n)
    field[-1] = np.inf
    cf = _lib.gpk_coef3()
    cf.rho = dptr(field)
    assert call(ff=cf) == _lib.GPK_EINVAL
    assert call() == "device"
    assert not h.value
    f32, out4 = ctypes.c_int32(), (ctypes.c_double * 4)()
    assert lib.gpk_bdata_info3(None, ctypes.byref(f32), ctypes.byref(f32)) == _lib.GPK_EINVAL
    assert lib.gpk_boundary_terms3(None, out4) == _lib.GPK_EINVAL


def _faces():
    from tests.operator3_ref import FACES
    return list(FACES)


def test_device_solver_checks_its_arguments_before_the_library():
    from gpk.equations import Operator3
    from gpk.model_GP_solver_3d import DeviceSolver3
    ns = (4, 3, 2)
    xs = [np.linspace(0.0, 1.0, m) for m in ns]
    nb = 2 * (ns[1] * ns[2] + ns[0] * ns[2] + ns[0] * ns[1])
    src, bv = np.zeros(ns), np.zeros(nb)
    opx = dict(c2=(1.0, 1.0, 1.0), c1=(0.0, 0.0, 0.0), react=(1.0, 0.0, 0.0), faces=63)
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=opx, dfaces=3)            # no dvals
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=opx, dfaces=3, dvals=np.zeros(nb - 1))
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, dfaces=3, dvals=np.zeros(nb))     # no operator
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=Operator3((2, 2, 2), (1.0, 1.0, 1.0)),
                      dfaces=3, dvals=np.zeros(nb))


def test_config_listings_and_builder():
    import yaml
    from gpk import model_GP_solver_3d as m3d
    from gpk.equations import (EQUATIONS_3D, EQUATIONS_3D_OP, EQUATIONS_3D_OPN, EQUATIONS_3D_OPV, EQUATIONS_3D_OPX)
    from gpk.infras.exp_config import ExpConfig
    assert EQUATIONS_3D_OPN == ["wave_t-sin", "helmholtz_neumann-sin"]
    assert not (set(EQUATIONS_3D) | set(EQUATIONS_3D_OP) | set(EQUATIONS_3D_OPX) | set(EQUATIONS_3D_OPV)) & set(EQUATIONS_3D_OPN)
    cdir = os.path.join(PKG_DIR, "gpk", "config3d_opn")
    assert sorted(os.listdir(cdir)) == sorted(e + ".yaml" for e in EQUATIONS_3D_OPN)
    # the existing lists and folders hold what they held
    assert EQUATIONS_3D == ["poisson_3d-mix_sin", "allencahn_3d-sin"]
    assert EQUATIONS_3D_OP == ["heat_3d-sin", "advection_3d-sin", "helmholtz_3d-sin", "allencahn_t-sin"]
    assert EQUATIONS_3D_OPX == ["convdiff_t-sin", "convdiff_3d-sin"]
    assert EQUATIONS_3D_OPV == ["helmholtz_var-sin", "heat_var-sin", "transport_var-sin"]
    for d, es in (("config3d", EQUATIONS_3D), ("config3d_op", EQUATIONS_3D_OP), ("config3d_opx", EQUATIONS_3D_OPX),
                  ("config3d_opv", EQUATIONS_3D_OPV)):
        assert sorted(os.listdir(os.path.join(PKG_DIR, "gpk", d))) == sorted(e + ".yaml" for e in es)
    with open(os.path.join(PKG_DIR, "gpk", "config3d_op", "heat_3d-sin.yaml")) as f:
        ref = yaml.safe_load(f)
    for e in EQUATIONS_3D_OPN:
        with open(os.path.join(cdir, e + ".yaml")) as f:
            c = yaml.safe_load(f)
        assert c["equation"] == e
        assert {k: v for k, v in c.items() if k != "equation"} == {k: v for k, v in ref.items() if k != "equation"}
        assert m3d.load_config(e) == c
    args = ExpConfig()
    args.parse({"equation": "wave_t-sin", "kernel": "Matern52_Cos_1d", "nepoch": 7})
    cfg = m3d.build_config(args)
    assert cfg["equation"] == "wave_t-sin" and cfg["nepoch"] == 7 and cfg["scale"] == 1.0
    assert set(m3d.GP_solver_3d_single.opn_eq_types) == {"wave_t", "helmholtz_neumann"}
