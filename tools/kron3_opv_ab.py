"""Step time of coefficient-field handles of the 3-axis solver (gpk_create3_opv).

Grid: 64^3 on [0, 1], Q = 30, Matern52_Cos_1d, at the initial params (the data only sets the
values, not the work).  Modes:
    heat_opx        the heat form through gpk_create3_opx: c2 (-nu, -nu, 0), c1 (0, 0, 1), final-time
                    face open
    heat_opv_none   the same operator through gpk_create3_opv with no field: the same captured
                    graph, so it must agree with heat_opx within the spread (its losses are checked
                    bitwise equal)
    heat_opv_a12    nu(x, y) on axes 1-2 (heat_var-sin's field): k3_combine_v with two fields, W_1
                    and W_2 as operands of the reverse products
    heat_opv_all    fields on all three axes plus rho: k3_combine_v with every stream, k3_adam_u_v
Five fresh handles per mode, interleaved mode by mode; each handle: a warm-up call (graph capture,
code objects), then the host clock around `steps` graph launches of one synchronous gpk_step3 call.
Median and spread (max - min) over the five handles.  Writes JSON (default
profiles/kron3_opv_ab.json).

--only MODE: one handle of that mode, the warm-up and `steps` launches, nothing written: the
process to put under a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python
tools/kron3_opv_ab.py --only MODE).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-process-slover-for-high-freq-pde_amd")]
from gpk.equations import Operator3V, Operator3X, solution_3d, solution_3d_opv  # noqa: E402
from gpk.model_GP_solver_3d import DeviceSolver3, boundary_3d  # noqa: E402

NU = 0.1
C2, C1, FACES = (-NU, -NU, 0.0), (0.0, 0.0, 1.0), 0b011111
A12 = solution_3d_opv("heat_var-sin")[2].a[0]
A3 = lambda x, y, t: 1.0 + 0.25 * np.cos(2 * np.pi * t) * np.sin(2 * np.pi * x)
RHO = lambda x, y, t: 0.5 * np.sin(2 * np.pi * y) + 0.0 * x * t
MODES = {
    "heat_opx": Operator3X(C2, C1, faces=FACES),
    "heat_opv_none": Operator3V(C2, C1, faces=FACES),
    "heat_opv_a12": Operator3V(C2, C1, faces=FACES, a=(A12, A12, None)),
    "heat_opv_all": Operator3V(C2, C1, faces=FACES, a=(A12, A12, A3), rho=RHO),
}


def solver(ns, q, op):
    u, _ = solution_3d("allencahn_3d-sin")
    xs = [np.linspace(0, 1, n) for n in ns]
    g = np.meshgrid(*xs, indexing="ij")
    return DeviceSolver3("poisson", "Matern52_Cos_1d", xs, -12.0 * u(*g), boundary_3d(u(*g)), Q=q, operator=op)


def step_times(ns, q, steps, handles):
    us = {m: [] for m in MODES}
    first, has = {}, {}
    for _ in range(handles):
        for m, op in MODES.items():  # interleaved, a fresh handle each time
            s = solver(ns, q, op)
            try:
                has[m] = list(s.coef_info())
                first.setdefault(m, s.step(5))  # capture, code objects
                t0 = time.perf_counter()
                s.step(steps)
                us[m].append((time.perf_counter() - t0) * 1e6 / steps)
            finally:
                s.close()
    rec = {"heat_opx_equals_heat_opv_none_bitwise": bool(np.array_equal(first["heat_opx"], first["heat_opv_none"]))}
    for m in MODES:
        rec[m] = {"fields": has[m], "us_per_step": us[m], "median_us": float(np.median(us[m])),
                  "spread_us": float(max(us[m]) - min(us[m]))}
    for m in ("heat_opv_none", "heat_opv_a12", "heat_opv_all"):
        rec[m + "_minus_heat_opx_us"] = rec[m]["median_us"] - rec["heat_opx"]["median_us"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--q", type=int, default=30)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--handles", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron3_opv_ab.json"))
    ap.add_argument("--only", choices=list(MODES))
    a = ap.parse_args()
    ns = (a.n,) * 3
    if a.only:
        s = solver(ns, a.q, MODES[a.only])
        try:
            s.step(5)
            s.step(a.steps)
        finally:
            s.close()
        return
    rec = {"ns": list(ns), "Q": a.q, "kind": "Matern52_Cos_1d", "steps": a.steps, "handles": a.handles}
    rec.update(step_times(ns, a.q, a.steps, a.handles))
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
