"""Host-side surface of the convective terms (no GPU): header and ctypes entries, the struct layout,
every argument error of gpk_create3_opc (all returned before a device is touched), the new configs,
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
    for must in ("gpk_create3_opc", "gpk_conv_info3", "gpk_assemble_pairs2"):
        assert must in header_functions() and must in _lib.EXPORTS and hasattr(lib, must)
    assert lib.gpk_abi_version() == 2
    with open(os.path.join(ROOT, "include", "gpk.h")) as f:
        header = " ".join(f.read().replace("*", " ").split())
    # the term, that g_k is a constant, and that the fields do not multiply it
    assert "g_k . u . d u / d x_k" in header
    assert "g_k is a CONSTANT" in header and "never this one" in header


def test_conv3_struct_layout_matches_header(tmp_path):
    from gpk._lib import gpk_conv3
    assert [f for f, _ in gpk_conv3._fields_] == ["g"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpk.h"\nint main(void){\n'
                     'printf("sizeof %zu\\n", sizeof(gpk_conv3));\n'
                     'printf("g %zu\\n", offsetof(gpk_conv3, g));\n'
                     'printf("g2 %zu\\n", offsetof(gpk_conv3, g[2]));\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(gpk_conv3) == 24
    assert int(out["g"]) == gpk_conv3.g.offset == 0 and int(out["g2"]) == 16


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

    def call(pp=p, cc=c, ff=None, bb=None, vv=cv, out=h):
        """GPK_EINVAL from the argument checks, or 'device': the call passed them all and failed
        at the device check that follows."""
        ref = lambda x: None if x is None else ctypes.byref(x)
        rc = lib.gpk_create3_opc(ref(pp), ref(cc), ref(ff), ref(bb), ref(vv), 1.0, ref(out))
        assert rc != _lib.GPK_OK
        return "device" if b"device" in lib.gpk_last_error() else rc

    assert call() == "device" and call(bb=bd) == "device"
    zero = _lib.gpk_conv3()
    for vv in (cv, zero, None):  # (zero and NULL: the gpk_create3_opn route and, below it, opv's and opx's)
        for kw in (dict(pp=None), dict(cc=None), dict(out=None)):
            assert call(vv=vv, **kw) == _lib.GPK_EINVAL
            assert call(vv=vv, bb=bd, **kw) == _lib.GPK_EINVAL
        assert call(vv=vv) == "device"
    # a non-finite g_k, in every position, whatever the others are
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            for base in ((0.0, 0.0, 0.0), (1.0, 0.5, 0.25)):
                v2 = _lib.gpk_conv3()
                v2.g[:] = base
                v2.g[k] = bad
                assert call(vv=v2) == _lib.GPK_EINVAL, (k, bad)
                assert b"g must be finite" in lib.gpk_last_error()
    # the derivative data's own cases next to a convective axis
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
    # faces: 0 needs derivative data, with or without a convective axis
    c.faces = 0
    assert call() == _lib.GPK_EINVAL and call(bb=bd) == "device"
    for faces in (64, -1):
        c.faces = faces
        assert call() == _lib.GPK_EINVAL, faces
    c.faces = 0b011111
    # the operator's and the problem's own cases
    c.c2[1] = float("nan")
    assert call() == _lib.GPK_EINVAL
    c.c2[1] = 0.0
    p.eq = _lib.EQ_IDS["allencahn"]
    assert call() == _lib.GPK_EINVAL
    p.eq = _lib.EQ_IDS["poisson"]
    for name, bad in (("kind", 4), ("q", 0), ("q", 65), ("n1", 1), ("n3", 1025)):
        good = getattr(p, name)
        setattr(p, name, bad)
        assert call() == _lib.GPK_EINVAL, (name, bad)
        setattr(p, name, good)
    field = np.linspace(-1.0, 1.0, n)
    field[0] = np.nan
    cf = _lib.gpk_coef3()
    cf.a[1] = dptr(field)
    assert call(ff=cf) == _lib.GPK_EINVAL
    assert call() == "device"
    assert not h.value
    assert lib.gpk_conv_info3(None, (ctypes.c_double * 3)()) == _lib.GPK_EINVAL
    # the diag entry's own checks
    x, q1 = np.linspace(0.0, 1.0, 5), np.zeros(1)
    out = np.empty((5, 5))
    ap2 = lambda *a: lib.gpk_assemble_pairs2(*a)
    args = lambda **kw: [kw.get("kind", 0), dptr(x), kw.get("n", 5), dptr(q1), dptr(q1), dptr(q1), kw.get("q", 1),
                         kw.get("jitter", 0.0), kw.get("c2", 1.0), kw.get("c1", 0.0), dptr(out), dptr(out),
                         kw.get("D1", dptr(out))]
    for kw in (dict(kind=4), dict(n=0), dict(n=1025), dict(q=0), dict(q=65), dict(c2=np.nan), dict(c1=np.inf),
               dict(jitter=np.nan), dict(D1=None)):
        assert ap2(*args(**kw)) == _lib.GPK_EINVAL, kw


def test_device_solver_checks_its_arguments_before_the_library():
    from gpk.equations import Operator3
    from gpk.model_GP_solver_3d import DeviceSolver3
    ns = (4, 3, 2)
    xs = [np.linspace(0.0, 1.0, m) for m in ns]
    nb = 2 * (ns[1] * ns[2] + ns[0] * ns[2] + ns[0] * ns[1])
    src, bv = np.zeros(ns), np.zeros(nb)
    opx = dict(c2=(1.0, 1.0, 1.0), c1=(0.0, 0.0, 0.0), react=(1.0, 0.0, 0.0), faces=63)
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=opx, conv=(1.0, 0.0))    # two entries
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, conv=(1.0, 0.0, 0.0))             # no operator
    with pytest.raises(ValueError):
        DeviceSolver3("poisson", "SE_1d", xs, src, bv, Q=2, operator=Operator3((2, 2, 2), (1.0, 1.0, 1.0)),
                      conv=(0.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        DeviceSolver3("allencahn", "SE_1d", xs, src, bv, Q=2, conv=(0.0, 1.0, 0.0))


def test_config_listings_and_builder():
    import yaml
    from gpk import model_GP_solver_3d as m3d
    from gpk.equations import (EQUATIONS_3D, EQUATIONS_3D_OP, EQUATIONS_3D_OPC, EQUATIONS_3D_OPN, EQUATIONS_3D_OPV,
                               EQUATIONS_3D_OPX)
    from gpk.infras.exp_config import ExpConfig
    assert EQUATIONS_3D_OPC == ["burgers_t-sin", "burgers_3d-sin"]
    older = set(EQUATIONS_3D) | set(EQUATIONS_3D_OP) | set(EQUATIONS_3D_OPX) | set(EQUATIONS_3D_OPV) | set(EQUATIONS_3D_OPN)
    assert not older & set(EQUATIONS_3D_OPC)
    cdir = os.path.join(PKG_DIR, "gpk", "config3d_opc")
    assert sorted(os.listdir(cdir)) == sorted(e + ".yaml" for e in EQUATIONS_3D_OPC)
    # the existing lists and folders hold what they held
    assert EQUATIONS_3D == ["poisson_3d-mix_sin", "allencahn_3d-sin"]
    assert EQUATIONS_3D_OP == ["heat_3d-sin", "advection_3d-sin", "helmholtz_3d-sin", "allencahn_t-sin"]
    assert EQUATIONS_3D_OPX == ["convdiff_t-sin", "convdiff_3d-sin"]
    assert EQUATIONS_3D_OPV == ["helmholtz_var-sin", "heat_var-sin", "transport_var-sin"]
    assert EQUATIONS_3D_OPN == ["wave_t-sin", "helmholtz_neumann-sin"]
    for d, es in (("config3d", EQUATIONS_3D), ("config3d_op", EQUATIONS_3D_OP), ("config3d_opx", EQUATIONS_3D_OPX),
                  ("config3d_opv", EQUATIONS_3D_OPV), ("config3d_opn", EQUATIONS_3D_OPN)):
        assert sorted(os.listdir(os.path.join(PKG_DIR, "gpk", d))) == sorted(e + ".yaml" for e in es)
    with open(os.path.join(PKG_DIR, "gpk", "config3d_op", "heat_3d-sin.yaml")) as f:
        ref = yaml.safe_load(f)
    for e in EQUATIONS_3D_OPC:
        with open(os.path.join(cdir, e + ".yaml")) as f:
            c = yaml.safe_load(f)
        assert c["equation"] == e
        assert {k: v for k, v in c.items() if k != "equation"} == {k: v for k, v in ref.items() if k != "equation"}
        assert m3d.load_config(e) == c
    args = ExpConfig()
    args.parse({"equation": "burgers_t-sin", "kernel": "Matern52_Cos_1d", "nepoch": 7})
    cfg = m3d.build_config(args)
    assert cfg["equation"] == "burgers_t-sin" and cfg["nepoch"] == 7 and cfg["scale"] == 1.0
    assert set(m3d.GP_solver_3d_single.opc_eq_types) == {"burgers_t", "burgers_3d"}
    assert set(m3d.GP_solver_3d_single.opn_eq_types) == {"wave_t", "helmholtz_neumann"}
