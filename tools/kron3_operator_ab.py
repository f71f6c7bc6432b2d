"""Step time of operator handles of the 3-axis solver (gpk_create3_op) against the legacy handle.

Grid: the Allen-Cahn config's size (gpk/config3d/allencahn_3d-sin.yaml: 64^3 on [0, 1], Q = 30),
Matern52_Cos_1d, at the initial params with the Poisson source of that solution.  Modes:
    legacy     gpk_create3, Poisson
    operator   the same equation stated as an operator (orders 2, weights 1, faces 63): the same
               captured graph, so it must agree with `legacy` within the spread
    heat       orders (2, 2, 1), weights (-nu, -nu, 1), final-time face open: axes 1-2 differ in
               order, so their assembly and their contraction launch split (two more launches)
Five fresh handles per mode, interleaved mode by mode; each handle: a warm-up call (graph capture,
code objects), then the host clock around `steps` graph launches of one synchronous gpk_step3
call.  Median and spread (max - min) over the five handles.  Also checks on the way that `legacy`
and `operator` give bitwise-equal losses.  Writes JSON (default profiles/kron3_operator_ab.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-process-slover-for-high-freq-pde_amd")]
from gpk.equations import Operator3, solution_3d  # noqa: E402
from gpk.model_GP_solver_3d import DeviceSolver3, boundary_3d  # noqa: E402

NU = 0.1
MODES = {
    "legacy": None,
    "operator": Operator3((2, 2, 2), (1.0, 1.0, 1.0)),
    "heat": Operator3((2, 2, 1), (-NU, -NU, 1.0), faces=0b011111),
}


def solver(ns, q, op):
    u, _ = solution_3d("allencahn_3d-sin")
    xs = [np.linspace(0, 1, n) for n in ns]
    g = np.meshgrid(*xs, indexing="ij")
    src = -12.0 * u(*g)  # lap u: the data only sets the values, not the work
    return DeviceSolver3("poisson", "Matern52_Cos_1d", xs, src, boundary_3d(u(*g)), Q=q, operator=op)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--q", type=int, default=30)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--handles", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron3_operator_ab.json"))
    a = ap.parse_args()
    ns = (a.n,) * 3
    us = {m: [] for m in MODES}
    first = {}
    for _ in range(a.handles):
        for m, op in MODES.items():  # interleaved, a fresh handle each time
            s = solver(ns, a.q, op)
            try:
                first.setdefault(m, s.step(5))  # capture, code objects
                t0 = time.perf_counter()
                s.step(a.steps)
                us[m].append((time.perf_counter() - t0) * 1e6 / a.steps)
            finally:
                s.close()
    rec = {"ns": list(ns), "Q": a.q, "kind": "Matern52_Cos_1d", "steps": a.steps, "handles": a.handles,
           "legacy_equals_operator_bitwise": bool(np.array_equal(first["legacy"], first["operator"]))}
    for m in MODES:
        rec[m] = {"us_per_step": us[m], "median_us": float(np.median(us[m])),
                  "spread_us": float(max(us[m]) - min(us[m]))}
    for m in ("operator", "heat"):
        rec[m + "_over_legacy"] = rec[m]["median_us"] / rec["legacy"]["median_us"]
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
