"""Host-side surface of the 3-axis solver (no GPU): header entry points, configs, exact
solutions, the config builder and the solver class's reference method names."""
import os

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.conftest import PKG_DIR
from tests.test_abi import header_functions

NEW_ENTRY_POINTS = ["gpk_mode_gemm", "gpk_predict3", "gpk_criterion3", "gpk_get_opt_state3",
                    "gpk_set_opt_state3", "gpk_stage_variants3", "gpk_loss_terms3"]
EQS = ["poisson_3d-mix_sin", "allencahn_3d-sin"]


def test_header_declares_the_3d_entry_points():
    names = header_functions()
    for must in NEW_ENTRY_POINTS:
        assert must in names, must
    from gpk import _lib
    for must in NEW_ENTRY_POINTS:
        assert must in _lib.EXPORTS, must


def test_read_only_entry_points_reject_null():
    import ctypes
    from gpk import _lib
    lib = _lib.load()
    n = ctypes.c_int32()
    out = (ctypes.c_int32 * 8)()
    assert lib.gpk_stage_variants3(None, out, 8, ctypes.byref(n)) == _lib.GPK_EINVAL
    assert lib.gpk_loss_terms3(None, (ctypes.c_double * 7)()) == _lib.GPK_EINVAL


def test_config3d_files():
    import yaml
    cdir = os.path.join(PKG_DIR, "gpk", "config3d")
    assert sorted(os.listdir(cdir)) == sorted(e + ".yaml" for e in EQS)
    for e in EQS:
        with open(os.path.join(cdir, e + ".yaml")) as f:
            c = yaml.safe_load(f)
        assert c["equation"] == e
        for key in ("Q", "lr", "logdet", "llk_weight", "freq_scale", "N_col", "scale", "nepoch", "num_fold",
                    "num_u_trick", "tol", "other_paras", "M_test"):
            assert key in c, (e, key)
        assert c["N_col"] == 64 and c["M_test"] == 100
    assert len(os.listdir(os.path.join(PKG_DIR, "gpk", "config"))) == 11


@pytest.mark.parametrize("eq", EQS)
def test_solution_3d_is_the_oracles(eq):
    from gpk.equations import EQUATIONS_3D, solution_3d
    assert eq in EQUATIONS_3D
    u, src = solution_3d(eq)
    uo, so = O._u3d(eq)
    g = np.meshgrid(np.linspace(0, 2 * np.pi, 13), np.linspace(0, 1, 7), np.linspace(-1, 3, 9), indexing="ij")
    eps = np.finfo(float).eps
    # the same closed forms: a few roundings of the largest term apart at the most
    assert np.max(np.abs(u(*g) - uo(*g))) <= 8 * eps * np.max(np.abs(uo(*g)))
    assert np.max(np.abs(src(*g) - so(*g))) <= 8 * eps * np.max(np.abs(so(*g)))
    with pytest.raises(KeyError):
        solution_3d("poisson_2d-sin_sin")


def test_build_config_3d_like_2d():
    from gpk import model_GP_solver_3d as m3d
    from gpk.infras.exp_config import ExpConfig
    args = ExpConfig()
    args.parse({"equation": "poisson_3d-mix_sin", "kernel": "Matern52_Cos_1d", "nepoch": 200})
    cfg = m3d.build_config(args)
    assert cfg["scale"] == 2 * np.pi and cfg["nepoch"] == 200 and cfg["kernel"].__name__ == "Matern52_Cos_1d"
    assert cfg["other_paras"] == "-x-2pi-Ncol-64" and cfg["kernel_extra"] is None
    args.parse({"equation": "allencahn_3d-sin", "kernel": "SE_1d", "nepoch": 10})
    cfg = m3d.build_config(args)
    assert cfg["scale"] == 1.0 and cfg["kernel"].__name__ == "SE_1d" and cfg["other_paras"].endswith("-Ncol-64")
    with pytest.raises(AssertionError):
        args.equation = "poisson_2d-sin_sin"
        m3d.build_config(args)


def test_solver_class_surface():
    from gpk import model_GP_solver_3d as m3d
    from gpk.solver_common import SolverBase
    cls = m3d.GP_solver_3d_single
    assert issubclass(cls, SolverBase) and cls.early_stop_enabled
    for meth in ("loss", "value_and_grad", "step", "preds", "compute_early_stopping", "train",
                 "save_checkpoint", "load_checkpoint", "init_params", "_make_device", "_err",
                 "_kernel_lists", "_finish_log"):
        assert callable(getattr(cls, meth)), meth
    for meth in ("predict", "criterion", "get_opt_state", "set_opt_state", "sync", "stage_variants",
                 "loss_terms"):
        assert callable(getattr(m3d.DeviceSolver3, meth)), meth
    for fn in ("test", "evals", "main", "load_config", "build_config", "boundary_3d"):
        assert callable(getattr(m3d, fn)), fn
    log = cls._finish_log(None, {"loss_list": [1.0], "w_list_k3": [2.0], "other": 3})
    assert list(log)[:2] == ["loss_list", "err_list"] and "ls_list_k3" in log and "other" not in log
