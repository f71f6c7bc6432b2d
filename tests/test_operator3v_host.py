"""Host-side surface of the coefficient-field handles (no GPU): header and ctypes entries, the
struct layout, every argument error (all returned before a device is touched), the new configs
and the Operator3V class; the existing 3-axis config folders are as they were."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import PKG_DIR, ROOT
from tests.test_abi import header_functions


def test_header_and_ctypes_entries():
    from gpk import _lib
    lib = _lib.load()
    for must in ("gpk_create3_opv", "gpk_coef_info3"):
        assert must in header_functions() and must in _lib.EXPORTS and hasattr(lib, must)
    assert lib.gpk_abi_version() == 2


def test_coef3_struct_layout_matches_header(tmp_path):
    from gpk._lib import gpk_coef3
    fields = [f for f, _ in gpk_coef3._fields_]
    assert fields == ["a", "rho"]
    probe = tmp_path / "probe.c"
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(gpk_coef3, {f}));' for f in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpk.h"\nint main(void){\n'
                     'printf("sizeof %zu\\n", sizeof(gpk_coef3));\n'
                     'printf("a1 %zu\\n", offsetof(gpk_coef3, a[1]));\n' + body + "\nreturn 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(gpk_coef3)
    for f in fields:
        assert int(out[f]) == getattr(gpk_coef3, f).offset, f
    assert int(out["a1"]) == ctypes.sizeof(ctypes.c_void_p)


def _valid_problem(ns=(4, 3, 2)):
    """A gpk_problem3 that passes every check of the problem itself (its arrays are kept alive)."""
    from gpk import _lib
    from gpk._lib import dptr
    n = ns[0] * ns[1] * ns[2]
    keep = [np.linspace(0.0, 1.0, m) for m in ns] + [np.zeros(n), np.zeros(2 * (ns[1] * ns[2] + ns[0] * ns[2] + ns[0] * ns[1]))]
    p = _lib.gpk_problem3()
    p.eq, p.kind, p.q = _lib.EQ_IDS["poisson"], 1, 2
    p.n1, p.n2, p.n3 = ns
    p.x1, p.x2, p.x3, p.src, p.bvals = (dptr(a) for a in keep)
    p.device = 1 << 20  # no such device: a call that got past validation fails with another code
    return p, keep, n


def test_argument_errors_without_a_device():
    from gpk import _lib
    from gpk._lib import dptr
    lib = _lib.load()
    p, keep, n = _valid_problem()
    c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
    c.c2[:], c.c1[:], c.react[:], c.faces = (1.0, 1.0, 1.0), (0.0, 0.5, 0.0), (0.0, 0.0, 0.0), 63
    field = np.linspace(-1.0, 1.0, n)
    cf = _lib.gpk_coef3()
    cf.a[1] = dptr(field)

    def call(pp=p, cc=c, ff=cf, out=h):
        """GPK_EINVAL from the argument checks, or 'device': the call passed them all and failed
        at the device check that follows (no device here, or no device of that ordinal)."""
        rc = lib.gpk_create3_opv(None if pp is None else ctypes.byref(pp), None if cc is None else ctypes.byref(cc),
                                 None if ff is None else ctypes.byref(ff), 1.0, None if out is None else ctypes.byref(out))
        assert rc != _lib.GPK_OK
        return "device" if b"device" in lib.gpk_last_error() else rc

    assert call() == "device"
    # NULL arguments, with fields and (the gpk_create3_opx route) without
    for ff in (cf, None, _lib.gpk_coef3()):
        assert call(pp=None, ff=ff) == _lib.GPK_EINVAL
        assert call(cc=None, ff=ff) == _lib.GPK_EINVAL
        assert call(out=None, ff=ff) == _lib.GPK_EINVAL
    # the operator's cases, as on gpk_create3_opx
    for name, bad in (("c2", float("nan")), ("c1", float("inf")), ("react", float("-inf"))):
        good = tuple(getattr(c, name))
        getattr(c, name)[1] = bad
        assert call() == _lib.GPK_EINVAL, name
        getattr(c, name)[:] = good
    for faces in (0, 64, -1):
        c.faces = faces
        assert call() == _lib.GPK_EINVAL, faces
    c.faces = 63
    p.eq = _lib.EQ_IDS["allencahn"]  # the operator states the equation
    assert call() == _lib.GPK_EINVAL
    p.eq = _lib.EQ_IDS["poisson"]
    # the problem's own cases come before the fields are read
    for name, bad in (("kind", 4), ("q", 0), ("q", 65), ("n1", 1), ("n3", 1025)):
        good = getattr(p, name)
        setattr(p, name, bad)
        assert call() == _lib.GPK_EINVAL, (name, bad)
        setattr(p, name, good)
    p.src = None
    assert call() == _lib.GPK_EINVAL
    p.src = dptr(keep[3])
    # a non-finite value inside any given field, the last entry included
    for slot in (0, 1, 2, 3):
        for idx, bad in ((0, np.nan), (n // 2, np.inf), (n - 1, -np.inf)):
            f = field.copy()
            f[idx] = bad
            ff = _lib.gpk_coef3()
            if slot < 3:
                ff.a[slot] = dptr(f)
            else:
                ff.rho = dptr(f)
            assert call(ff=ff) == _lib.GPK_EINVAL, (slot, idx)
            assert b"non-finite" in lib.gpk_last_error()
    assert call() == "device"
    assert not h.value
    has = (ctypes.c_int32 * 4)()
    assert lib.gpk_coef_info3(None, has) == _lib.GPK_EINVAL


def test_operator3v_class_callables_and_arrays_agree():
    from gpk.equations import Operator3V, Operator3X
    axes = [np.linspace(0.0, 1.0, 5), np.linspace(0.0, 2.0, 4), np.linspace(-1.0, 1.0, 3)]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    f1, fr = (lambda x, y, z: 1.0 + x * y - z), (lambda x, y, z: np.sin(x) + 0.0 * y * z)
    a = Operator3V((-0.1, -0.1, 0.0), (0.0, 0.0, 1.0), faces=31, a=(f1, None, lambda x, y, z: 2.0), rho=fr)
    b = Operator3V((-0.1, -0.1, 0.0), (0.0, 0.0, 1.0), faces=31, a=(f1(X, Y, Z), None, np.full(X.shape, 2.0)),
                   rho=fr(X, Y, Z))
    fa, fb = a.fields(axes), b.fields(axes)
    assert a.has == b.has == (True, False, True, True)
    assert fa[1] is None and fb[1] is None
    for u, v in zip(fa, fb):
        if u is not None:  # a constant callable is broadcast to the grid
            assert u.shape == X.shape and u.dtype == np.float64 and u.flags.c_contiguous and np.array_equal(u, v)
    assert a.constant == Operator3X((-0.1, -0.1, 0.0), (0.0, 0.0, 1.0), faces=31)
    assert repr(a) == ("Operator3V(c2=(-0.1, -0.1, 0.0), c1=(0.0, 0.0, 1.0), react=(0.0, 0.0, 0.0), faces=31, "
                       "a=(<callable>, None, <callable>), rho=<callable>)")
    assert Operator3V((1.0,) * 3, (0.0,) * 3).has == (False,) * 4
    with pytest.raises(ValueError):
        Operator3V((1.0,) * 3, (0.0,) * 3, a=(np.zeros((5, 4, 2)), None, None)).fields(axes)
    with pytest.raises(ValueError):
        Operator3V((1.0,) * 3, (0.0,) * 3, a=(None, None))
    with pytest.raises(ValueError):
        Operator3V((1.0, 1.0), (0.0,) * 3)


def test_config_listings_and_builder():
    import yaml
    from gpk import model_GP_solver_3d as m3d
    from gpk.equations import EQUATIONS_3D, EQUATIONS_3D_OP, EQUATIONS_3D_OPV, EQUATIONS_3D_OPX
    from gpk.infras.exp_config import ExpConfig
    assert not (set(EQUATIONS_3D) | set(EQUATIONS_3D_OP) | set(EQUATIONS_3D_OPX)) & set(EQUATIONS_3D_OPV)
    cdir = os.path.join(PKG_DIR, "gpk", "config3d_opv")
    assert sorted(os.listdir(cdir)) == sorted(e + ".yaml" for e in EQUATIONS_3D_OPV)
    # the existing lists and folders hold what they held
    assert EQUATIONS_3D == ["poisson_3d-mix_sin", "allencahn_3d-sin"]
    assert EQUATIONS_3D_OP == ["heat_3d-sin", "advection_3d-sin", "helmholtz_3d-sin", "allencahn_t-sin"]
    assert EQUATIONS_3D_OPX == ["convdiff_t-sin", "convdiff_3d-sin"]
    for d, es in (("config3d", EQUATIONS_3D), ("config3d_op", EQUATIONS_3D_OP), ("config3d_opx", EQUATIONS_3D_OPX)):
        assert sorted(os.listdir(os.path.join(PKG_DIR, "gpk", d))) == sorted(e + ".yaml" for e in es)
    with open(os.path.join(PKG_DIR, "gpk", "config3d_op", "heat_3d-sin.yaml")) as f:
        ref = yaml.safe_load(f)
    for e in EQUATIONS_3D_OPV:
        with open(os.path.join(cdir, e + ".yaml")) as f:
            c = yaml.safe_load(f)
        assert c["equation"] == e
        assert {k: v for k, v in c.items() if k != "equation"} == {k: v for k, v in ref.items() if k != "equation"}
        assert m3d.load_config(e) == c
    args = ExpConfig()
    args.parse({"equation": "heat_var-sin", "kernel": "Matern52_Cos_1d", "nepoch": 7})
    cfg = m3d.build_config(args)
    assert cfg["equation"] == "heat_var-sin" and cfg["nepoch"] == 7 and cfg["scale"] == 1.0
    assert set(m3d.GP_solver_3d_single.opv_eq_types) == {"helmholtz_var", "heat_var", "transport_var"}
