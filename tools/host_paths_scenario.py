"""One fixed, seeded sequence of calls through every host path that builds refined solves or takes
per-call device scratch, for telling whether two builds of the library (GPK_LIB_PATH selects it)
compute the same thing bit for bit:

    python tools/host_paths_scenario.py

2D handle of the tests' open-gate case (refinement stages 1/2, 4/5 and 8/9 run): step(3),
loss_grad, predict on 11 x 7 test points; the same with GPK_FLAG_NO_CHAIN_AUG (stages A / D and the
non-augmented stage 8/9); a 1D handle's predict; a 3-axis handle (20, 14, 9) with the fused and
with the two-GEMM refinement route: step(2), loss_grad, criterion, loss_terms, predict on
(11, 37, 5); then the standalone entry points gpk_refine_panel, gpk_mode_gemm, gpk_dgemm,
gpk_kernel_matrices, gpk_kernel_pairs and gpk_fields_dd at the smallest shapes that take each of
their branches.  Prints the element count and crc32 of everything returned.
"""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-process-slover-for-high-freq-pde_amd")]
import numpy as np  # noqa: E402
from gpk import _lib  # noqa: E402
from gpk.core import fields_dd, kernel_matrices, kernel_pairs  # noqa: E402
from gpk.model_GP_solver_3d import DeviceSolver3  # noqa: E402
from tests.helpers import device_solver, problem_1d, problem_2d, problem_3d, rand_kp  # noqa: E402


def run_2d(flags):
    prob, params, _, fs = problem_2d(eq="allencahn", kind="Matern52_1d", n1=40, n2=36, Q=5, seed=4)
    s = device_solver(prob, 5, fs, flags=flags)
    try:
        s.set_params(params)
        loss, grad = s.loss_grad()
        out = [s.step(3), [loss], grad]
        out.append(s.predict(np.linspace(-0.03, 1.02, 11) * prob["x1"][-1],
                             np.linspace(-0.03, 1.02, 7) * prob["x2"][-1]))
        out.append(s.get_flat())
    finally:
        s.close()
    return out


def run_1d():
    prob, params, _ = problem_1d(kind="SE_1d", n=40, Q=5, seed=1)
    s = device_solver(prob, 5, 20.0)
    try:
        s.set_params(params)
        return [s.predict(np.linspace(-0.03, 1.02, 13) * prob["x"].reshape(-1)[-1])]
    finally:
        s.close()


def run_3d(refine):
    prob, params, fs = problem_3d(eq="poisson", kind="Matern52_Cos_1d", ns=(20, 14, 9), Q=4, seed=3)
    s = DeviceSolver3(prob["eq"], prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"],
                      prob["bvals"], Q=4, jitter=prob["jitter"], llk_weight=prob["llk_weight"],
                      logdet=prob["logdet"], freq_scale=fs, refine=refine)
    try:
        s.set_params(params)
        out = [s.step(2)]
        loss, grad = s.loss_grad()
        info = s.refine_info()
        out += [[loss], grad, [s.criterion()], list(s.loss_terms().values()), info["bound"],
                [info["route"]] + info["open"]]
        xte = [np.linspace(-0.03, 1.02, m) * prob[f"x{a}"][-1] for a, m in zip((1, 2, 3), (11, 37, 5))]
        out += [s.predict(*xte), s.get_flat()]
    finally:
        s.close()
    return out


def run_standalone():
    rng = np.random.default_rng(7)
    out = []
    P, M = 64, 96
    K = rng.normal(size=(P, P))
    K = K @ K.T / P + np.eye(P)
    Kinv = np.linalg.inv(K) * (1 + 1e-6 * rng.normal(size=(P, P)))  # (an inexact inverse to refine)
    for side in (0, 1):
        B = rng.normal(size=(P, M) if side == 0 else (M, P))
        X = Kinv @ B if side == 0 else B @ Kinv
        for route in (_lib.REFINE_GEMM, _lib.REFINE_FUSED):
            out.append(_lib.refine_panel(Kinv, K, B, X, side=side, route=route)[0])
    T = rng.normal(size=(32, 64, 32))
    for k, variants in ((1, [_lib.MODE_SLAB]), (2, [_lib.MODE_SLAB, _lib.MODE_PERMUTE]), (3, [_lib.MODE_SLAB])):
        Mat = rng.normal(size=(32, T.shape[k - 1]))
        shape = list(T.shape)
        shape[k - 1] = 32
        C0 = rng.normal(size=shape)
        for v in variants:
            out.append(_lib.mode_gemm(Mat, T, k, alpha=0.7, variant=v)[0])
            out.append(_lib.mode_gemm(Mat, T, k, alpha=0.7, beta=-1.3, C0=C0, variant=v)[0])
            out.append(_lib.mode_gemm(Mat, T, k, alpha=0.7, beta=-1.3, C0=C0, inplace=True, variant=v)[0])
    A, B, C0 = rng.normal(size=(64, 96)), rng.normal(size=(96, 32)), rng.normal(size=(64, 32))
    out.append(_lib.dgemm(A, B, alpha=-1.0, beta=1.0, C0=C0)[0])  # (the wrapper passes C0 as C itself)
    kp = rand_kp(rng, 5, 20.0)
    x1, x2 = np.sort(rng.uniform(size=23)), np.sort(rng.uniform(size=17))
    Kx, Dx = kernel_matrices("Matern52_Cos_1d", x1, x2, kp, jitter=1e-6, deriv=2)
    out += [Kx, Dx, kernel_pairs("SE_Cos_1d", x1[:17], x2, kp, deriv=1)]
    hi, lo = fields_dd("Matern52_Cos_1d", 2, np.linspace(0.0, 1.1, 12), 0.8, 3.7)
    out += [hi, lo]
    return out


def main():
    out = run_2d(0) + run_2d(_lib.GPK_FLAG_NO_CHAIN_AUG) + run_1d()
    out += run_3d(True) + run_3d("gemm") + run_standalone()
    flat = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in out])
    if not np.all(np.isfinite(flat)):
        raise SystemExit("host_paths_scenario: a call returned a non-finite value")
    print(f"values {flat.size} crc32 {zlib.crc32(flat.tobytes()):08x}")


if __name__ == "__main__":
    main()
