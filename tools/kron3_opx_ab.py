"""Step time of mixed-order operator handles of the 3-axis solver (gpk_create3_opx), the assembly
launch of a mixed axis alone, and what the two default configs reach.

Grid: 64^3 on [0, 1], Q = 30, Matern52_Cos_1d, at the initial params (the data only sets the
values, not the work).  Step-time modes:
    heat_op      the heat form through gpk_create3_op: orders (2, 2, 1), weights (-nu, -nu, 1),
                 final-time face open (the number of tools/kron3_operator_ab.py, measured again)
    heat_opx     the same operator through gpk_create3_opx: the same captured graph, so it must
                 agree with heat_op within the spread (its losses are checked bitwise equal)
    convdiff_t   c2 (-nu, -nu, 0), c1 (b1, b2, 1): two mixed axes in one shared assembly and one
                 shared contraction launch, axis 3 first order
    convdiff_3d  all three axes mixed
Five fresh handles per mode, interleaved mode by mode; each handle: a warm-up call (graph capture,
code objects), then the host clock around `steps` graph launches of one synchronous gpk_step3 call.
Median and spread (max - min) over the five handles.

Assembly launch alone (gpk_assemble_pairs_time: HIP events around back-to-back launches of the
per-pair kernel on one axis of n points, after a checked and a warm-up launch), five repeats each,
interleaved: mode both, mode 2, and mode 2 plus mode 1 as two launches -- what mode both replaces if
the two blocks are formed separately.

--defaults: also trains the two gpk/config3d_opx/ configs at their own nepoch and records the
relative L2 error at the last and at the best record.  Writes JSON (default
profiles/kron3_opx_ab.json).
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
from gpk.equations import EQUATIONS_3D_OPX, Operator3, Operator3X, solution_3d, solution_3d_opx  # noqa: E402
from gpk.model_GP_solver_3d import (DeviceSolver3, GP_solver_3d_single, boundary_3d, build_config,  # noqa: E402
                                    get_mesh_data)

NU, BETA = 0.05, (1.0, 0.5, 0.25)
MODES = {
    "heat_op": Operator3((2, 2, 1), (-NU, -NU, 1.0), faces=0b011111),
    "heat_opx": Operator3X((-NU, -NU, 0.0), (0.0, 0.0, 1.0), faces=0b011111),
    "convdiff_t": Operator3X((-NU, -NU, 0.0), (BETA[0], BETA[1], 1.0), faces=0b011111),
    "convdiff_3d": Operator3X((-NU,) * 3, BETA),
}


def solver(ns, q, op):
    u, _ = solution_3d("allencahn_3d-sin")
    xs = [np.linspace(0, 1, n) for n in ns]
    g = np.meshgrid(*xs, indexing="ij")
    return DeviceSolver3("poisson", "Matern52_Cos_1d", xs, -12.0 * u(*g), boundary_3d(u(*g)), Q=q, operator=op)


def step_times(ns, q, steps, handles):
    us = {m: [] for m in MODES}
    first = {}
    for _ in range(handles):
        for m, op in MODES.items():  # interleaved, a fresh handle each time
            s = solver(ns, q, op)
            try:
                first.setdefault(m, s.step(5))  # capture, code objects
                t0 = time.perf_counter()
                s.step(steps)
                us[m].append((time.perf_counter() - t0) * 1e6 / steps)
            finally:
                s.close()
    rec = {"heat_op_equals_heat_opx_bitwise": bool(np.array_equal(first["heat_op"], first["heat_opx"]))}
    for m in MODES:
        rec[m] = {"us_per_step": us[m], "median_us": float(np.median(us[m])),
                  "spread_us": float(max(us[m]) - min(us[m]))}
    for m in ("heat_opx", "convdiff_t", "convdiff_3d"):
        rec[m + "_over_heat_op"] = rec[m]["median_us"] / rec["heat_op"]["median_us"]
    return rec


def assembly_times(n, q, iters, repeats):
    """The per-pair assembly launch of one axis at the handle's initial kernel parameters."""
    kp = {"freq": np.linspace(0, 1, q) * 20.0, "log-ls": np.zeros(q), "log-w": np.log(1.0 / q) * np.ones(q)}
    x = np.linspace(0, 1, n)
    kinds = {"both": dict(c2=-NU, c1=BETA[0]), "mode2": dict(c2=1.0, c1=0.0), "mode1": dict(c2=0.0, c1=1.0),
             "mode2_plus_mode1": dict(c2=1.0, c1=1.0, split=True)}
    us = {k: [] for k in kinds}
    for _ in range(repeats):
        for k, a in kinds.items():
            us[k].append(_lib.assemble_pairs_time("Matern52_Cos_1d", x, kp, iters=iters, **a))
    return {k: {"us_per_launch": v, "median_us": float(np.median(v)), "spread_us": float(max(v) - min(v))}
            for k, v in us.items()} | {"n": n, "iters": iters}


def default_run(equation):
    """One training of the equation's default config: relative L2 at the last and the best record."""
    class Args:
        kernel, nepoch, device, refine = "Matern52_Cos_1d", None, None, None
    Args.equation = equation
    cfg = build_config(Args)
    u, src, op = solution_3d_opx(equation)
    M, N = cfg["M_test"], cfg["N_col"]
    xte, ute = get_mesh_data(u, (M,) * 3, cfg["scale"])
    xc, umh = get_mesh_data(u, (N,) * 3, cfg["scale"])
    _, srcv = get_mesh_data(src, (N,) * 3, cfg["scale"])
    m = GP_solver_3d_single(boundary_3d(umh, op.faces), xc, srcv, 1e-6, cfg, X_test=xte, u_test=ute)
    try:
        t0 = time.perf_counter()
        log, stop, min_err = m.train(cfg["nepoch"], 0, verbose=False)
        sec = time.perf_counter() - t0
    finally:
        m.dev.close()
    return {"nepoch": cfg["nepoch"], "N_col": N, "M_test": M, "records": len(log["err_list"]),
            "last_epoch": int(log["epoch_list"][-1]), "last_rel_l2": float(log["err_list"][-1]),
            "best_rel_l2": float(min_err), "best_epoch": int(log["epoch_list"][int(np.argmin(log["err_list"]))]),
            "seconds": sec}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--q", type=int, default=30)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--handles", type=int, default=5)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--defaults", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron3_opx_ab.json"))
    a = ap.parse_args()
    ns = (a.n,) * 3
    rec = {"ns": list(ns), "Q": a.q, "kind": "Matern52_Cos_1d", "steps": a.steps, "handles": a.handles}
    rec.update(step_times(ns, a.q, a.steps, a.handles))
    rec["assembly"] = assembly_times(a.n, a.q, a.iters, a.handles)
    if a.defaults:
        rec["defaults"] = {e: default_run(e) for e in EQUATIONS_3D_OPX}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
