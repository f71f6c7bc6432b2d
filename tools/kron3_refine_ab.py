"""Cost of the 3-axis step's gated refinement (DeviceSolver3(refine=...), GPK_FLAG3_REFINE) and
A/B of its two routes: two gated GEMMs per solve against the fused panel kernel.

Step: the whole Adam step with the flag off, on with the two GEMMs forced and on with the handle's own
route (the fused kernel), interleaved, three repetitions each in one process, host clock around `steps` graph
launches of one synchronous gpk_step3 call after a warm-up call.  Grids: the Allen-Cahn config
(gpk/config3d/allencahn_3d-sin.yaml: 64^3 on [0, 1], Q = 30) at its initial params, and the
(97, 128, 130) grid of tests/test_gpu_kron3_shapes.py.  Records the gates as the last step left
them.
Panel: one refinement step on host operands (gpk_refine_panel), left and right form, both routes
interleaved, three repetitions, HIP-event time per call over `iters` back-to-back launches after
a warm-up launch; Kc a well-conditioned SPD matrix and Kinv its inverse, so the repeated step
stays finite.  Algorithmic bytes: 8 (3 P M + 2 P^2) -- X in and out, B, the two matrices once.
Writes JSON (default profiles/kron3_refine_ab.json).
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
from gpk.equations import solution_3d  # noqa: E402
from gpk.model_GP_solver_3d import DeviceSolver3, boundary_3d  # noqa: E402

GRIDS = [((64, 64, 64), 200), ((97, 128, 130), 50)]
PANELS = [((64, 4096), 2000), ((128, 20480), 300), ((512, 4096), 100)]  # (P, M), iters
MODES = {"unrefined": False, "gemm": "gemm", "fused": True}


def solver(ns, refine):
    u, src = solution_3d("allencahn_3d-sin")
    xs = [np.linspace(0, 1, n) for n in ns]
    g = np.meshgrid(*xs, indexing="ij")
    return DeviceSolver3("allencahn", "Matern52_Cos_1d", xs, src(*g), boundary_3d(u(*g)), Q=30,
                         refine=refine)


def ab(ns, steps, reps=3):
    s = {r: solver(ns, r) for r in MODES.values()}
    us = {r: [] for r in s}
    try:
        for r in s:
            s[r].step(5)  # capture, code objects
        for _ in range(reps):
            for r in s:  # interleaved
                t0 = time.perf_counter()
                s[r].step(steps)
                us[r].append((time.perf_counter() - t0) * 1e6 / steps)
        info = {r: s[r].refine_info() for r in ("gemm", True)}
    finally:
        for r in s:
            s[r].close()
    rec = {"ns": list(ns), "steps": steps, "gates": info["gemm"], "fused_route": info[True]["route"]}
    for name, r in MODES.items():
        rec[name] = {"us_per_step": us[r], "median_us": float(np.median(us[r])),
                     "spread_us": float(max(us[r]) - min(us[r]))}
    for name in ("gemm", "fused"):
        rec[name + "_over_unrefined"] = rec[name]["median_us"] / rec["unrefined"]["median_us"]
    return rec


def panel_ab(P, M, iters, reps=3):
    rng = np.random.default_rng(0)
    G = rng.normal(size=(P, P))
    Kc = np.eye(P) + G @ G.T / P
    Kinv = np.linalg.inv(Kc)
    rec = {"P": P, "M": M, "iters": iters, "alg_bytes": 8.0 * (3 * P * M + 2 * P * P), "sides": {}}
    for side, name in ((0, "left"), (1, "right")):
        shape = (P, M) if side == 0 else (M, P)
        B, X = rng.normal(size=shape), rng.normal(size=shape)
        us = {0: [], 1: []}
        out = {}
        for _ in range(reps):
            for route in (0, 1):  # interleaved
                out[route], t = _lib.refine_panel(Kinv, Kc, B, X, side=side, route=route, iters=iters)
                us[route].append(t)
        r = {"max_abs_diff": float(np.max(np.abs(out[0] - out[1])))}
        for route, rn in ((0, "gemm"), (1, "fused")):
            med = float(np.median(us[route]))
            r[rn] = {"us": us[route], "median_us": med, "spread_us": float(max(us[route]) - min(us[route])),
                     "alg_GBps": rec["alg_bytes"] / med / 1e3}
        r["fused_over_gemm"] = r["fused"]["median_us"] / r["gemm"]["median_us"]
        rec["sides"][name] = r
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron3_refine_ab.json"))
    a = ap.parse_args()
    res = {"panel": [], "step": []}
    for (P, M), iters in PANELS:
        r = panel_ab(P, M, iters)
        res["panel"].append(r)
        print((P, M), {k: "gemm %.1f (+-%.1f) fused %.1f (+-%.1f) us x%.3f" % (
            v["gemm"]["median_us"], v["gemm"]["spread_us"], v["fused"]["median_us"], v["fused"]["spread_us"],
            v["fused_over_gemm"]) for k, v in r["sides"].items()}, flush=True)
    for ns, steps in GRIDS:
        r = ab(ns, steps)
        res["step"].append(r)
        print(ns, "unrefined %.1f us (+-%.1f)  gemm %.1f us (+-%.1f) x%.3f  fused %.1f us (+-%.1f) x%.3f  open %s" % (
            r["unrefined"]["median_us"], r["unrefined"]["spread_us"], r["gemm"]["median_us"],
            r["gemm"]["spread_us"], r["gemm_over_unrefined"], r["fused"]["median_us"],
            r["fused"]["spread_us"], r["fused_over_unrefined"], r["gates"]["open"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
