"""Step time of 3-axis handles with derivative boundary data (gpk_create3_opn).

Grid: 64^3 on [0, 1], Q = 30, Matern52_Cos_1d, at the initial params (the data only sets the
values, not the work).  The heat form c2 (-nu, -nu, 0), c1 (0, 0, 1), final-time face open, with
    heat_opx    no derivative data (gpk_create3_opx; the mode that also runs on the parent commit)
    opn_none    the same through gpk_create3_opn with dfaces = 0: the same captured graph (its
                losses are checked bitwise equal to heat_opx's)
    face_1 / face_2 / face_3   one derivative face on axis 1 / 2 / 3 (faces 0, 2, 4): the leading
                form on the natural layout, on the permuted layout, and the trailing form
    six         all six faces
Five fresh handles per mode, interleaved mode by mode; each handle: a warm-up call (graph capture,
code objects), then the host clock around `steps` graph launches of one synchronous gpk_step3 call.
Median and spread (max - min) over the handles.  Writes JSON (default profiles/kron3_opn_ab.json).

--modes A,B: only those modes (heat_opx alone needs nothing of this feature, so the same file
times a checkout of the parent commit).  --only MODE: one handle, the warm-up and `steps`
launches, nothing written: the process to put under a kernel trace of its own.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-process-slover-for-high-freq-pde_amd")]
from gpk.equations import Operator3X, solution_3d  # noqa: E402
from gpk.model_GP_solver_3d import DeviceSolver3, boundary_3d  # noqa: E402

NU = 0.1
OP = Operator3X((-NU, -NU, 0.0), (0.0, 0.0, 1.0), faces=0b011111)
MODES = {"heat_opx": None, "opn_none": 0, "face_1": 0b000001, "face_2": 0b000100, "face_3": 0b010000, "six": 63}


def solver(ns, q, dfaces):
    u, _ = solution_3d("allencahn_3d-sin")
    xs = [np.linspace(0, 1, n) for n in ns]
    g = np.meshgrid(*xs, indexing="ij")
    bv = boundary_3d(u(*g))
    kw = {} if dfaces is None else dict(dfaces=dfaces, dvals=np.cos(np.arange(bv.size)))
    return DeviceSolver3("poisson", "Matern52_Cos_1d", xs, -12.0 * u(*g), bv, Q=q, operator=OP, **kw)


def step_times(ns, q, steps, handles, modes):
    us = {m: [] for m in modes}
    first = {}
    for _ in range(handles):
        for m in modes:  # interleaved, a fresh handle each time
            s = solver(ns, q, MODES[m])
            try:
                first.setdefault(m, s.step(5))  # capture, code objects
                t0 = time.perf_counter()
                s.step(steps)
                us[m].append((time.perf_counter() - t0) * 1e6 / steps)
            finally:
                s.close()
    rec = {}
    if "heat_opx" in modes and "opn_none" in modes:
        rec["heat_opx_equals_opn_none_bitwise"] = bool(np.array_equal(first["heat_opx"], first["opn_none"]))
    for m in modes:
        rec[m] = {"us_per_step": us[m], "median_us": float(np.median(us[m])),
                  "spread_us": float(max(us[m]) - min(us[m])), "first_losses": [float(x) for x in first[m]]}
    if "heat_opx" in modes:
        for m in modes:
            if m != "heat_opx":
                rec[m + "_minus_heat_opx_us"] = rec[m]["median_us"] - rec["heat_opx"]["median_us"]
    # four passes over one padded tensor (two reads of A_k, a read and a write of T_k)
    rec["four_passes_bytes"] = 4 * 8 * int(np.prod([(n + 31) // 32 * 32 for n in ns]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--q", type=int, default=30)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--handles", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron3_opn_ab.json"))
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
    modes = [m for m in a.modes.split(",") if m]
    rec = {"ns": list(ns), "Q": a.q, "kind": "Matern52_Cos_1d", "steps": a.steps, "handles": a.handles}
    rec.update(step_times(ns, a.q, a.steps, a.handles, modes))
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
