"""Host side of the 3-axis step's gated refinement (runs without a device): the fp64 emulation
behind the bars of tests/test_gpu_kron3_refine.py, and DeviceSolver3(refine=True) with no device."""
import importlib.util
import os

import pytest

import tests.test_gpu_kron3_shapes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emulation():
    spec = importlib.util.spec_from_file_location(
        "kron3_sweep_emulation", os.path.join(ROOT, "tools", "kron3_sweep_emulation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# U's distance from the yardstick as a multiple of the LU oracle's: unrefined, refined
@pytest.mark.parametrize("case,unrefined,refined", [("T321", 7.03, 0.50), ("Q64-cos", 4.78, 0.98)])
def test_refine_emulation_reproduces_the_u_column(case, unrefined, refined):
    E = _emulation()
    (eq, kind, ns, Q), _, _ = T.ALL_CASES[case]
    ref = T._reference(eq, kind, ns, Q)
    for refine, want in ((False, unrefined), (True, refined)):
        d = T._distances(E.emulate(ref["prob"], ref["params"], E.sweep_inverse, refine), ref["ext"])
        ratio = d["U"] / ref["lu_err"]["U"]
        print(case, "refine" if refine else "plain", f"{ratio:.4f}", want)
        assert abs(ratio - want) < 0.005 + 1e-9, (case, refine, ratio, want)  # two digits
    # the log-dets come from the pivots: refinement does not move them
    a = E.emulate(ref["prob"], ref["params"], E.sweep_inverse, False)[2]
    b = E.emulate(ref["prob"], ref["params"], E.sweep_inverse, True)[2]
    for k in ("logdet_1", "logdet_2", "logdet_3"):
        assert a[k] == b[k]


def test_refined_solver_without_a_device_raises_gpk_error():
    import ctypes
    from gpk import _lib
    from tests.helpers import problem_3d
    from tests.test_gpu_kron3 import _solver
    n = ctypes.c_int32(0)
    if _lib.load().gpk_device_count(ctypes.byref(n)) == _lib.GPK_OK and n.value > 0:
        pytest.skip("a device is present")
    from gpk.model_GP_solver_3d import DeviceSolver3
    prob, _, fs = problem_3d(eq="poisson", kind="Matern52_1d", ns=(9, 8, 7), Q=4, seed=3)
    with pytest.raises(_lib.GPKError):
        _solver(prob, 4, fs)
    with pytest.raises(_lib.GPKError):
        DeviceSolver3(prob["eq"], prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"],
                      prob["bvals"], Q=4, freq_scale=fs, refine=True)
