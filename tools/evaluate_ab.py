"""Cost of the scattered-point evaluation (gpk_evaluate / gpk_evaluate3) next to the grid
prediction, and of its contraction kernel alone (gpk_point_contract).

Calls: host clock around the synchronous call (as DESIGN's gpk_predict3 figure is taken), one
warm-up call each, then five repetitions with the calls interleaved; median and spread (max - min).
  2D, the C4 grid (256^2, Q = 30, random field): evaluate() on 10^4 random points; predict() on a
      100 x 100 grid (the same number of outputs); predict() on the 10^4 x 10^4 tensor grid whose
      diagonal those points are -- the only route to scattered points before -- where the device
      has the memory for it (its outputs alone are 800 MB).
  3 axes, 64^3 (the Allen-Cahn config, Q = 30, random field): evaluate() on 4096 random points.
Kernel: HIP-event time per launch over `iters` back-to-back launches after a warm-up launch, five
repetitions interleaved, at (n, C, m) = (256, 1, 10^4) and (64, 64, 1024), Q = 30, orders 0 and 2.
Algorithmic work: m n Q field evaluations and 8 m n C bytes of T.
Writes JSON (default profiles/evaluate_ab.json).
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
from gpk.problems import make_solver  # noqa: E402

REPS = 5
KERNEL_SHAPES = [((256, 1, 10000), 200), ((64, 64, 1024), 200)]  # (n, C, m), iters


def stats(v):
    return {"us": v, "median_us": float(np.median(v)), "spread_us": float(max(v) - min(v))}


def time_calls(calls, reps=REPS):
    """calls: {name: thunk}; a warm-up each, then `reps` rounds with the calls interleaved."""
    us = {k: [] for k in calls}
    for f in calls.values():
        f()
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            us[k].append((time.perf_counter() - t0) * 1e6)
    return {k: stats(v) for k, v in us.items()}


def calls_2d(with_tensor=True):
    rng = np.random.default_rng(1)
    s = make_solver("C4")
    scale = 2 * np.pi
    pts = rng.uniform(0, 1, size=(10000, 2)) * scale
    xg = np.linspace(0, 1, 100) * scale
    px, py = np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])
    rec = {"grid": [256, 256], "Q": 30, "points": 10000}
    calls = {"evaluate_1e4_points": lambda: s.evaluate(pts),
             "predict_100x100_grid": lambda: s.predict(xg, xg)}
    try:
        if with_tensor:
            try:
                diag = np.diagonal(s.predict(px, py))
                rec["max_abs_diff_vs_tensor_diagonal"] = float(np.max(np.abs(diag - s.evaluate(pts))))
                rec["max_abs_value"] = float(np.max(np.abs(diag)))
                calls["predict_1e4x1e4_tensor"] = lambda: s.predict(px, py)
            except (_lib.GPKError, MemoryError) as e:
                rec["predict_1e4x1e4_tensor"] = "not run: %s" % e
        rec.update(time_calls(calls))
    finally:
        s.close()
    return rec


def calls_3d():
    ns = (64, 64, 64)
    u, src = solution_3d("allencahn_3d-sin")
    xs = [np.linspace(0, 1, n) for n in ns]
    g = np.meshgrid(*xs, indexing="ij")
    s = DeviceSolver3("allencahn", "Matern52_Cos_1d", xs, src(*g), boundary_3d(u(*g)), Q=30)
    rng = np.random.default_rng(2)
    try:
        flat = s.get_flat()
        flat[:np.prod(ns)] = 0.1 * rng.normal(size=int(np.prod(ns)))
        s.set_flat(flat)
        pts = rng.uniform(0, 1, size=(4096, 3))
        rec = {"grid": list(ns), "Q": 30, "points": 4096}
        rec.update(time_calls({"evaluate3_4096_points": lambda: s.evaluate(pts),
                               "evaluate3_4096_points_d200": lambda: s.evaluate(pts, deriv=(2, 0, 0))}))
    finally:
        s.close()
    return rec


def kernel_alone(reps=REPS):
    rng = np.random.default_rng(3)
    Q = 30
    kp = {"freq": np.linspace(0, 1, Q) * 20.0, "log-ls": np.zeros(Q), "log-w": np.log(1.0 / Q) * np.ones(Q)}
    cases = {}
    for (n, C, m), iters in KERNEL_SHAPES:
        x = np.linspace(0, 1, n) * 2 * np.pi
        t = rng.uniform(0, 1, size=m) * 2 * np.pi
        T = rng.normal(size=(m, n, C))
        for deriv in (0, 2):
            cases[(n, C, m, deriv)] = (x, t, T, iters)
    us = {k: [] for k in cases}
    for _ in range(reps):
        for (n, C, m, deriv), (x, t, T, iters) in cases.items():  # interleaved
            _, v = _lib.point_contract("Matern52_Cos_1d", t, x, kp, T, C=C, deriv=deriv, iters=iters)
            us[(n, C, m, deriv)].append(v)
    out = []
    for (n, C, m, deriv), v in us.items():
        r = {"n": n, "C": C, "m": m, "Q": Q, "deriv": deriv, "iters": cases[(n, C, m, deriv)][3],
             "field_evaluations": m * n * Q, "alg_bytes": 8.0 * m * n * C}
        r.update(stats(v))
        r["field_evaluations_per_us"] = r["field_evaluations"] / r["median_us"]
        r["alg_GBps"] = r["alg_bytes"] / r["median_us"] / 1e3
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_ab.json"))
    ap.add_argument("--no-tensor", action="store_true", help="skip the 10^4 x 10^4 tensor route")
    a = ap.parse_args()
    res = {"kernel": kernel_alone()}
    for r in res["kernel"]:
        print("kernel n %d C %d m %d deriv %d: %.1f us (+-%.1f)" % (r["n"], r["C"], r["m"], r["deriv"],
                                                                 r["median_us"], r["spread_us"]), flush=True)
    for name, rec in (("calls_3d", calls_3d()), ("calls_2d", calls_2d(not a.no_tensor))):
        res[name] = rec
        for k, v in rec.items():
            if isinstance(v, dict) and "median_us" in v:
                print(name, k, "%.1f us (+-%.1f)" % (v["median_us"], v["spread_us"]), flush=True)
            elif not isinstance(v, (dict, list)) or k == "grid":
                print(name, k, v, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
