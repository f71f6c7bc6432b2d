"""Step time of 3-axis handles with drift fields (gpk_create3_opb).

Grid: n^3 on [0, 1] (64 and 256), Q = 30, Matern52_Cos_1d, at the initial params (the data only
sets the values, not the work).  The heat form c2 (-nu, -nu, 0), c1 (0, 0, 1), final-time face
open, with
    heat_opm    no drift, the handle made by gpk_create3_opm itself (called with no fields, no
                derivative data, no convective axis and no pair; the mode that also runs on the
                parent commit)
    opb_none    the same through gpk_create3_opb with three NULL fields: the same captured graph (its
                losses are checked bitwise equal to heat_opm's)
    drift_1 / drift_2 / drift_3   one drift axis, of each kind (1: natural, D1 on the left; 2: the
                permuted E_2 / Z_2; 3: D1 on the right)
    heat_div    heat_div_t-sin's form: fields a on axes 1-2 and the drift -nu grad a on axes 1-2
    drift_all   drift on all three axes
Fresh handles per mode, interleaved mode by mode; each handle: a warm-up call (graph capture, code
objects), then the host clock around `steps` graph launches of one synchronous gpk_step3 call.
Median and spread (max - min) over the handles.  Writes JSON (default profiles/kron3_opb_ab.json).

--modes A,B: only those modes (heat_opm alone needs nothing of this feature, so the same file
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
ROT = (lambda x, y, t: -(y - 0.5), lambda x, y, t: x - 0.5, lambda x, y, t: 0.5 + 0.0 * t)
# mode -> the drift axes (None: the handle comes from gpk_create3_opm; "div": heat_div_t-sin's form)
MODES = {"heat_opm": None, "opb_none": (), "drift_1": (0,), "drift_2": (1,), "drift_3": (2,), "heat_div": "div",
         "drift_all": (0, 1, 2)}


def solver(ns, q, mode):
    u, _ = solution_3d("allencahn_3d-sin")
    xs = [np.linspace(0, 1, n) for n in ns]
    g = np.meshgrid(*xs, indexing="ij")
    axes, op, kw = MODES[mode], HEAT, {}
    if axes == "div":
        from gpk.equations import solution_3d_opb
        _, _, op, _, _, _, _, drift = solution_3d_opb("heat_div_t-sin")
        kw = dict(drift=drift)
    elif axes:
        kw = dict(drift=tuple(ROT[k] if k in axes else None for k in range(3)))
    s = DeviceSolver3("poisson", "Matern52_Cos_1d", xs, -12.0 * u(*g), boundary_3d(u(*g)), Q=q, operator=op, **kw)
    if not axes:  # the same problem through gpk_create3_opm, or through gpk_create3_opb with three NULL
        lib = _lib.load()  # fields: the handle is replaced by that call's
        _lib.check(lib.gpk_destroy3(s._h))
        s._h = None
        c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
        c.c2[:], c.c1[:], c.react[:], c.faces = op.c2, op.c1, op.react, op.faces
        if axes is None:
            _lib.check(lib.gpk_create3_opm(ctypes.byref(s._prob), ctypes.byref(c), None, None, None, None, 20.0,
                                           ctypes.byref(h)))
        else:
            dr = _lib.gpk_drift3()
            _lib.check(lib.gpk_create3_opb(ctypes.byref(s._prob), ctypes.byref(c), None, None, None, None,
                                           ctypes.byref(dr), 20.0, ctypes.byref(h)))
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
    if "heat_opm" in modes and "opb_none" in modes:
        rec["heat_opm_equals_opb_none_bitwise"] = bool(np.array_equal(first["heat_opm"], first["opb_none"]))
        rec["same_stage_variants"] = variants["heat_opm"] == variants["opb_none"]
    for m in modes:
        rec[m] = {"us_per_step": us[m], "median_us": float(np.median(us[m])),
                  "spread_us": float(max(us[m]) - min(us[m])), "first_losses": [float(x) for x in first[m]],
                  "stage_variants": variants[m]}
    if "heat_opm" in modes:
        for m in modes:
            if m != "heat_opm":
                rec[m + "_minus_heat_opm_us"] = rec[m]["median_us"] - rec["heat_opm"]["median_us"]
    rec["padded_tensor_bytes"] = 8 * int(np.prod([(n + 31) // 32 * 32 for n in ns]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--q", type=int, default=30)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--handles", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron3_opb_ab.json"))
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
