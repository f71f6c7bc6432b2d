"""Step time of 3-axis handles with mixed partials (gpk_create3_opm).

Grid: n^3 on [0, 1] (64 and 256), Q = 30, Matern52_Cos_1d, at the initial params (the data only
sets the values, not the work).  The heat form c2 (-nu, -nu, 0), c1 (0, 0, 1), final-time face
open, with
    heat_opn    no cross term, the handle made by gpk_create3_opn itself (called with no fields and
                no derivative data; the mode that also runs on the parent commit)
    opm_zero    the same through gpk_create3_opm with m = (0, 0, 0): the same captured graph (its
                losses are checked bitwise equal to heat_opn's)
    pair_12 / pair_13 / pair_23   one pair, of each kind ((1,2): one permute each way; (1,3): natural
                throughout; (2,3): permuted throughout)
    aniso_heat  aniso_heat_t-sin's form: c2 (-0.1, -0.06, 0), m = (-0.08, 0, 0)
    all_pairs   all three pairs
Fresh handles per mode, interleaved mode by mode; each handle: a warm-up call (graph capture, code
objects), then the host clock around `steps` graph launches of one synchronous gpk_step3 call.
Median and spread (max - min) over the handles.  Writes JSON (default profiles/kron3_opm_ab.json).

--modes A,B: only those modes (heat_opn alone needs nothing of this feature, so the same file
times a checkout of the parent commit).  --only MODE: one handle, the warm-up and `steps`
launches, nothing written: the process to put under a kernel trace of its own.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-process-slover-for-high-freq-pde_amd")]
from gpk import _lib  # noqa: E402
from gpk.equations import Operator3X, solution_3d  # noqa: E402
from gpk.model_GP_solver_3d import DeviceSolver3, boundary_3d  # noqa: E402

NU = 0.1
HEAT = Operator3X((-NU, -NU, 0.0), (0.0, 0.0, 1.0), faces=0b011111)
ANISO = Operator3X((-0.1, -0.06, 0.0), (0.0, 0.0, 1.0), faces=0b011111)
# mode -> (operator, cross); cross None: the handle comes from gpk_create3_opn (solver)
MODES = {"heat_opn": (HEAT, None), "opm_zero": (HEAT, (0.0, 0.0, 0.0)), "pair_12": (HEAT, (1.0, 0.0, 0.0)),
         "pair_13": (HEAT, (0.0, 1.0, 0.0)), "pair_23": (HEAT, (0.0, 0.0, 1.0)),
         "aniso_heat": (ANISO, (-0.08, 0.0, 0.0)), "all_pairs": (HEAT, (1.0, 1.0, 1.0))}


def solver(ns, q, mode):
    op, cross = MODES[mode]
    u, _ = solution_3d("allencahn_3d-sin")
    xs = [np.linspace(0, 1, n) for n in ns]
    g = np.meshgrid(*xs, indexing="ij")
    kw = {} if cross is None else dict(cross=cross)
    s = DeviceSolver3("poisson", "Matern52_Cos_1d", xs, -12.0 * u(*g), boundary_3d(u(*g)), Q=q, operator=op, **kw)
    if cross is None:  # the same problem through gpk_create3_opn: the handle is replaced by that call's
        lib = _lib.load()
        _lib.check(lib.gpk_destroy3(s._h))
        s._h = None
        c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
        c.c2[:], c.c1[:], c.react[:], c.faces = op.c2, op.c1, op.react, op.faces
        _lib.check(lib.gpk_create3_opn(ctypes.byref(s._prob), ctypes.byref(c), None, None, 20.0, ctypes.byref(h)))
        s._h = h
    return s


def step_times(ns, q, steps, handles, modes):
    us = {m: [] for m in modes}
    first, variants = {}, {}
    for _ in range(handles):
        for m in modes:  # interleaved, a fresh handle each time
            s = solver(ns, q, m)
            try:
                first.setdefault(m, s.step(5))  # capture, code objects
                variants.setdefault(m, s.stage_variants())
                t0 = time.perf_counter()
                s.step(steps)
                us[m].append((time.perf_counter() - t0) * 1e6 / steps)
            finally:
                s.close()
    rec = {}
    if "heat_opn" in modes and "opm_zero" in modes:
        rec["heat_opn_equals_opm_zero_bitwise"] = bool(np.array_equal(first["heat_opn"], first["opm_zero"]))
        rec["same_stage_variants"] = variants["heat_opn"] == variants["opm_zero"]
    for m in modes:
        rec[m] = {"us_per_step": us[m], "median_us": float(np.median(us[m])),
                  "spread_us": float(max(us[m]) - min(us[m])), "first_losses": [float(x) for x in first[m]],
                  "stage_variants": variants[m]}
    if "heat_opn" in modes:
        for m in modes:
            if m != "heat_opn":
                rec[m + "_minus_heat_opn_us"] = rec[m]["median_us"] - rec["heat_opn"]["median_us"]
    rec["padded_tensor_bytes"] = 8 * int(np.prod([(n + 31) // 32 * 32 for n in ns]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--q", type=int, default=30)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--handles", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron3_opm_ab.json"))
    ap.add_argument("--only", choices=list(MODES))
    a = ap.parse_args()
    ns = (a.n,) * 3
    if a.only:
        s = solver(ns, a.q, a.only)
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
