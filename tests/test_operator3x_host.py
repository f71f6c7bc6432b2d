"""Host-side surface of the mixed-order operator handles (no GPU): header and ctypes entries, the
struct layout, the argument errors that need no device, the new configs and the config builder;
the existing 3-axis config folders are as they were."""
import ctypes
import os
import subprocess

import pytest

from tests.conftest import PKG_DIR, ROOT
from tests.test_abi import header_functions


def test_header_and_ctypes_entries():
    from gpk import _lib
    for must in ("gpk_create3_opx", "gpk_operator_info3x", "gpk_assemble_pairs"):
        assert must in header_functions() and must in _lib.EXPORTS
    lib = _lib.load()
    for must in ("gpk_create3_opx", "gpk_operator_info3x", "gpk_assemble_pairs"):
        assert hasattr(lib, must)


def test_operator3x_struct_layout_matches_header(tmp_path):
    from gpk._lib import gpk_operator3x
    fields = [f for f, _ in gpk_operator3x._fields_]
    assert fields == ["c2", "c1", "react", "faces"]
    probe = tmp_path / "probe.c"
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(gpk_operator3x, {f}));' for f in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpk.h"\nint main(void){\n'
                     'printf("sizeof %zu\\n", sizeof(gpk_operator3x));\n' + body + "\nreturn 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(gpk_operator3x)
    for f in fields:
        assert int(out[f]) == getattr(gpk_operator3x, f).offset, f


def test_null_arguments_without_a_device():
    from gpk import _lib
    lib = _lib.load()
    c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
    p = _lib.gpk_problem3()
    assert lib.gpk_operator_info3x(None, ctypes.byref(c)) == _lib.GPK_EINVAL
    assert lib.gpk_create3_opx(None, ctypes.byref(c), 1.0, ctypes.byref(h)) == _lib.GPK_EINVAL
    assert lib.gpk_create3_opx(ctypes.byref(p), None, 1.0, ctypes.byref(h)) == _lib.GPK_EINVAL
    assert lib.gpk_create3_opx(ctypes.byref(p), ctypes.byref(c), 1.0, None) == _lib.GPK_EINVAL
    # the operator is checked before any device is touched
    p.eq = _lib.EQ_IDS["poisson"]
    c.c2[:], c.c1[:], c.react[:], c.faces = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 63
    for field, bad in (("c2", float("nan")), ("c1", float("inf")), ("react", float("-inf"))):
        good = tuple(getattr(c, field))
        getattr(c, field)[1] = bad
        assert lib.gpk_create3_opx(ctypes.byref(p), ctypes.byref(c), 1.0, ctypes.byref(h)) == _lib.GPK_EINVAL, field
        getattr(c, field)[:] = good
    for faces in (0, 64, -1):
        c.faces = faces
        assert lib.gpk_create3_opx(ctypes.byref(p), ctypes.byref(c), 1.0, ctypes.byref(h)) == _lib.GPK_EINVAL, faces
    c.faces = 63
    p.eq = _lib.EQ_IDS["allencahn"]  # the operator states the equation: eq must be Poisson
    assert lib.gpk_create3_opx(ctypes.byref(p), ctypes.byref(c), 1.0, ctypes.byref(h)) == _lib.GPK_EINVAL
    assert not h.value
    # gpk_assemble_pairs: sizes, pointers and weights, all before the device
    z = (ctypes.c_double * 4)()
    ok = lambda **kw: lib.gpk_assemble_pairs(*[kw.get(k, d) for k, d in (
        ("kind", 1), ("x", z), ("n", 2), ("lw", z), ("ll", z), ("fr", z), ("q", 2), ("jitter", 0.0), ("c2", 1.0),
        ("c1", 1.0), ("K", z), ("D", z))])
    for kw in (dict(kind=4), dict(n=0), dict(n=1025), dict(q=0), dict(q=65), dict(x=None), dict(D=None),
               dict(c2=float("nan")), dict(c1=float("inf"))):
        assert ok(**kw) == _lib.GPK_EINVAL, kw


def test_operator3x_class():
    from gpk.equations import Operator3, Operator3X
    a = Operator3X((-0.1, -0.1, 0.0), (1.0, 0.5, 1.0), faces=31)
    assert Operator3X.of(a) is a and Operator3X.of(a.as_dict()) == a and a.mixed == (True, True, False)
    assert repr(a) == "Operator3X(c2=(-0.1, -0.1, 0.0), c1=(1.0, 0.5, 1.0), react=(0.0, 0.0, 0.0), faces=31)"
    assert a != Operator3X((-0.1, -0.1, 0.0), (1.0, 0.5, 1.0)) and a != Operator3((2, 2, 1), (-0.1, -0.1, 1.0), faces=31)
    with pytest.raises(ValueError):
        Operator3X((1.0, 1.0), (0.0, 0.0, 0.0))


def test_config_listings_and_builder():
    import yaml
    from gpk import model_GP_solver_3d as m3d
    from gpk.equations import EQUATIONS_3D, EQUATIONS_3D_OP, EQUATIONS_3D_OPX
    from gpk.infras.exp_config import ExpConfig
    assert not (set(EQUATIONS_3D) | set(EQUATIONS_3D_OP)) & set(EQUATIONS_3D_OPX)
    cdir = os.path.join(PKG_DIR, "gpk", "config3d_opx")
    assert sorted(os.listdir(cdir)) == sorted(e + ".yaml" for e in EQUATIONS_3D_OPX)
    # the existing folders hold what they held
    assert sorted(os.listdir(os.path.join(PKG_DIR, "gpk", "config3d_op"))) == sorted(
        e + ".yaml" for e in EQUATIONS_3D_OP) and len(EQUATIONS_3D_OP) == 4
    assert sorted(os.listdir(os.path.join(PKG_DIR, "gpk", "config3d"))) == sorted(e + ".yaml" for e in EQUATIONS_3D)
    for e in EQUATIONS_3D_OPX:
        with open(os.path.join(cdir, e + ".yaml")) as f:
            c = yaml.safe_load(f)
        assert c["equation"] == e
        with open(os.path.join(PKG_DIR, "gpk", "config3d_op", "heat_3d-sin.yaml")) as f:
            ref = yaml.safe_load(f)
        assert {k: v for k, v in c.items() if k != "equation"} == {k: v for k, v in ref.items() if k != "equation"}
        assert m3d.load_config(e) == c
    args = ExpConfig()
    args.parse({"equation": "convdiff_t-sin", "kernel": "Matern52_Cos_1d", "nepoch": 7})
    cfg = m3d.build_config(args)
    assert cfg["equation"] == "convdiff_t-sin" and cfg["nepoch"] == 7 and cfg["scale"] == 1.0
    assert set(m3d.GP_solver_3d_single.opx_eq_types) == {"convdiff_t", "convdiff_3d"}
