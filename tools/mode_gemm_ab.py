"""A/B of the mode-2 product routes (gpk_mode_gemm): the slab-batched kernel (variant 0; 2 / 3 its
32x32 / 64x64 tile forced) against permute -> GEMM -> permute (variant 1), interleaved, three
repetitions each in one process, HIP-event time per call over `iters` back-to-back launches
after a warm-up launch.  Shapes (d1, d2, d3, m): the driver's prediction products for N_col = 64,
M_test = 100, and one large one.  Also one end-to-end gpk_predict3 time (64^3 -> 100^3, host
clock around the synchronous call).  Writes JSON (default profiles/mode_gemm_ab.json).

Algorithmic bytes of a product: 8 (m d2 + d1 d2 d3 + d1 m d3) -- Mat, T and C once each.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-process-slover-for-high-freq-pde_amd")]
from gpk import _lib  # noqa: E402

SHAPES = [((128, 64, 64, 128), 2000), ((128, 64, 64, 64), 2000), ((320, 320, 320, 320), 30)]
NAMES = {0: "slab", 1: "permute", 2: "slab32", 3: "slab64"}


def ab(shape, iters, reps=3):
    d1, d2, d3, m = shape
    rng = np.random.default_rng(0)
    T, Mat = rng.normal(size=(d1, d2, d3)), rng.normal(size=(m, d2))
    nbytes = 8.0 * (m * d2 + d1 * d2 * d3 + d1 * m * d3)
    us = {v: [] for v in NAMES}
    out = {}
    for _ in range(reps):
        for v in NAMES:  # interleaved
            C, t = _lib.mode_gemm(Mat, T, 2, variant=v, iters=iters)
            us[v].append(t)
            out[v] = C
    rec = {"shape": list(shape), "iters": iters, "alg_bytes": nbytes, "alg_flops": 2.0 * d1 * d2 * d3 * m,
           "max_abs_diff_vs_permute": {NAMES[v]: float(np.max(np.abs(out[v] - out[1]))) for v in NAMES},
           "routes": {}}
    for v, name in NAMES.items():
        med = float(np.median(us[v]))
        rec["routes"][name] = {"us": us[v], "median_us": med, "spread_us": float(max(us[v]) - min(us[v])),
                               "alg_GBps": nbytes / med / 1e3, "TFLOPs": rec["alg_flops"] / med / 1e6}
    rec["slab_over_permute"] = rec["routes"]["slab"]["median_us"] / rec["routes"]["permute"]["median_us"]
    return rec


def predict_time(n=64, m=100, reps=5):
    from gpk.equations import solution_3d
    from gpk.model_GP_solver_3d import DeviceSolver3, boundary_3d
    u, src = solution_3d("poisson_3d-mix_sin")
    xs = [np.linspace(0, 1, n) * 2 * np.pi] * 3
    g = np.meshgrid(*xs, indexing="ij")
    s = DeviceSolver3("poisson", "Matern52_Cos_1d", xs, src(*g), boundary_3d(u(*g)), Q=30)
    try:
        flat = s.get_flat()
        flat[:n ** 3] = 0.1 * np.random.default_rng(0).normal(size=n ** 3)
        s.set_flat(flat)
        xt = [np.linspace(0, 1, m) * 2 * np.pi] * 3
        pred = s.predict(*xt)  # warm-up: code objects, first allocations
        # the timed size's result against numpy (LU solves, axis after axis)
        from oracle import gp_oracle as O
        p = s.get_params()
        ref = p["U"]
        for k in range(3):
            kp = p["kernel_paras_%d" % (k + 1)]
            A = np.linalg.solve(O.kernel_matrix("Matern52_Cos_1d", xs[k], kp, 1e-6),
                                np.moveaxis(ref, k, 0).reshape(n, -1))
            A = O.kernel_block("Matern52_Cos_1d", xt[k], xs[k], kp, 0) @ A
            ref = np.moveaxis(A.reshape([m] + [d for j, d in enumerate(ref.shape) if j != k]), 0, k)
        err = float(np.max(np.abs(pred - ref)) / np.max(np.abs(ref)))
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            s.predict(*xt)
            ts.append((time.perf_counter() - t0) * 1e3)
    finally:
        s.close()
    return {"n_col": n, "m_test": m, "ms": ts, "median_ms": float(np.median(ts)), "rel_err_vs_numpy": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mode_gemm_ab.json"))
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--shape", action="append", default=[], metavar="D1,D2,D3,M,ITERS",
                    help="time these shapes instead of the default three (repeatable)")
    a = ap.parse_args()
    res = {"mode2": []}
    shapes = [(tuple(v[:4]), v[4]) for v in ([int(x) for x in s.split(",")] for s in a.shape)] or SHAPES
    for shape, iters in shapes:
        r = ab(shape, iters)
        res["mode2"].append(r)
        print(shape, {k: round(v["median_us"], 1) for k, v in r["routes"].items()},
              "slab/permute %.3f" % r["slab_over_permute"], flush=True)
    if not a.no_predict:
        res["predict3"] = predict_time()
        print("predict3 64^3 -> 100^3: %.2f ms" % res["predict3"]["median_ms"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
