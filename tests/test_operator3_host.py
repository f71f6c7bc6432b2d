"""Host-side surface of the operator handles (no GPU): header and ctypes entries, the struct
layout, the operator equations' manufactured sources, their configs and the config builder."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import PKG_DIR, ROOT
from tests.test_abi import header_functions


def test_header_and_ctypes_entries():
    from gpk import _lib
    for must in ("gpk_create3_op", "gpk_operator_info3"):
        assert must in header_functions() and must in _lib.EXPORTS
    lib = _lib.load()
    c = _lib.gpk_operator3()
    assert lib.gpk_operator_info3(None, ctypes.byref(c)) == _lib.GPK_EINVAL
    assert lib.gpk_create3_op(None, ctypes.byref(c), 1.0, None) == _lib.GPK_EINVAL


def test_operator_struct_layout_matches_header(tmp_path):
    from gpk._lib import gpk_operator3
    fields = [f for f, _ in gpk_operator3._fields_]
    probe = tmp_path / "probe.c"
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(gpk_operator3, {f}));' for f in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpk.h"\nint main(void){\n'
                     'printf("sizeof %zu\\n", sizeof(gpk_operator3));\n' + body + "\nreturn 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(gpk_operator3)
    for f in fields:
        assert int(out[f]) == getattr(gpk_operator3, f).offset, f


def _deriv(u, p, k, order, h):
    e = np.zeros(3)
    e[k] = h
    if order == 1:
        return (u(*(p + e)) - u(*(p - e))) / (2 * h)
    return (u(*(p + e)) - 2 * u(*p) + u(*(p - e))) / h ** 2


def test_operator_equations_sources_and_configs():
    """Each entry's source is its operator applied to its solution (central differences, h = 1e-4:
    truncation ~ h^2 |u''''| / 12 and rounding ~ eps |u| / h^2, both below 1e-6 here)."""
    import yaml
    from gpk.equations import EQUATIONS_3D, EQUATIONS_3D_OP, Operator3, solution_3d_op
    assert not set(EQUATIONS_3D) & set(EQUATIONS_3D_OP)
    assert {e.split("-")[0] for e in EQUATIONS_3D_OP} == {"heat_3d", "advection_3d", "helmholtz_3d", "allencahn_t"}
    cdir = os.path.join(PKG_DIR, "gpk", "config3d_op")
    assert sorted(os.listdir(cdir)) == sorted(e + ".yaml" for e in EQUATIONS_3D_OP)
    rng = np.random.default_rng(0)
    for e in EQUATIONS_3D_OP:
        u, src, op = solution_3d_op(e)
        assert isinstance(op, Operator3) and Operator3.of(op.as_dict()) == op
        for p in rng.uniform(0.1, 0.9, size=(5, 3)):
            uu = u(*p)
            lhs = sum(op.coef[k] * _deriv(u, p, k, op.order[k], 1e-4) for k in range(3))
            lhs += op.react[0] * uu + op.react[1] * uu ** 2 + op.react[2] * uu ** 3
            assert abs(lhs - src(*p)) < 1e-6, (e, p)
        with open(os.path.join(cdir, e + ".yaml")) as f:
            c = yaml.safe_load(f)
        assert c["equation"] == e
        for key in ("Q", "lr", "logdet", "llk_weight", "freq_scale", "N_col", "scale", "nepoch", "num_fold",
                    "num_u_trick", "tol", "other_paras", "M_test"):
            assert key in c, (e, key)
    heat, adv = solution_3d_op("heat_3d-sin")[2], solution_3d_op("advection_3d-sin")[2]
    assert heat.order == (2, 2, 1) and heat.faces == 0b011111 and heat.coef[2] == 1.0
    assert adv.order == (1, 1, 1) and adv.faces == 63


def test_build_config_and_boundary_mask():
    from gpk import model_GP_solver_3d as m3d
    from gpk.infras.exp_config import ExpConfig
    args = ExpConfig()
    args.parse({"equation": "heat_3d-sin", "kernel": "Matern52_Cos_1d", "nepoch": 7})
    cfg = m3d.build_config(args)
    assert cfg["equation"] == "heat_3d-sin" and cfg["nepoch"] == 7 and cfg["scale"] == 1.0
    U = np.arange(4 * 3 * 2, dtype=float).reshape(4, 3, 2)
    full, part = m3d.boundary_3d(U), m3d.boundary_3d(U, 0b011111)
    assert full.size == part.size == 2 * (3 * 2 + 4 * 2 + 4 * 3) and not np.isnan(full).any()
    assert np.isnan(part).sum() == 12 and np.array_equal(part[:-12], full[:-12])
    assert m3d.boundary_count_3d((4, 3, 2), 0b011111) == full.size - 12
    assert m3d.boundary_count_3d((4, 3, 2)) == full.size
    with pytest.raises(ValueError):
        m3d.Operator3((2, 2), (1.0, 1.0, 1.0))
