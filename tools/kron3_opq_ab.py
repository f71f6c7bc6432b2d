"""Step time of 3-axis handles with mixed fourth-order partials (gpk_create3_opq).

Grid: n^3 on [0, 1] (64 and 256), Q = 30, Matern52_Cos_1d, at the initial params (the data only
sets the values, not the work).  The heat form c2 (-nu, -nu, 0), c1 (0, 0, 1), final-time face
open, with
    heat_oph    no bi-pair, the handle made by gpk_create3_oph itself (called with no fields, no
                derivative data, no convective axis, no pair, no drift and no high-order weight; the
                mode that also runs on the parent commit)
    opq_none    the same through gpk_create3_opq with q = 0: the same captured graph (its losses are
                checked bitwise equal to heat_oph's)
    pair_12 / pair_13 / pair_23   one bi-pair (12: permuted with a permute each way; 13: natural; 23:
                permuted throughout)
    pair_all    all three pairs
    plate       plate_t-sin's form: c2 on t, c4 on x and y, the pair (1,2)
Fresh handles per mode, interleaved mode by mode; each handle: a warm-up call (graph capture, code
objects), then the host clock around `steps` graph launches of one synchronous gpk_step3 call.
Median and spread (max - min) over the handles.  Writes JSON (default profiles/kron3_opq_ab.json).

--modes A,B: only those modes (heat_oph alone needs nothing of this feature, so the same file
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
QW = 1e-3
# mode -> bicross (None: the handle comes from gpk_create3_oph; (): gpk_create3_opq with zeros)
MODES = {"heat_oph": None, "opq_none": (), "pair_12": (QW, 0.0, 0.0), "pair_13": (0.0, QW, 0.0),
         "pair_23": (0.0, 0.0, QW), "pair_all": (QW, QW, QW), "plate": "plate"}


def solver(ns, q, mode):
    u, _ = solution_3d("allencahn_3d-sin")
    xs = [np.linspace(0, 1, n) for n in ns]
    g = np.meshgrid(*xs, indexing="ij")
    bq, op, kw = MODES[mode], HEAT, {}
    if bq == "plate":
        op = Operator3X((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), faces=0b011111)
        kw = dict(high=((0.01, 0.01, 0.0), (0.0, 0.0, 0.0)), bicross=(0.02, 0.0, 0.0))
    elif bq:
        kw = dict(bicross=bq)
    s = DeviceSolver3("poisson", "Matern52_Cos_1d", xs, -12.0 * u(*g), boundary_3d(u(*g)), Q=q, operator=op, **kw)
    if bq is None or bq == ():  # the same problem through gpk_create3_oph, or through gpk_create3_opq with
        lib = _lib.load()       # q = 0: the handle is replaced by that call's
        _lib.check(lib.gpk_destroy3(s._h))
        s._h = None
        c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
        c.c2[:], c.c1[:], c.react[:], c.faces = op.c2, op.c1, op.react, op.faces
        if bq is None:
            _lib.check(lib.gpk_create3_oph(ctypes.byref(s._prob), ctypes.byref(c), None, None, None, None, None,
                                           None, 20.0, ctypes.byref(h)))
        else:
            zero = _lib.gpk_bicross3()
            _lib.check(lib.gpk_create3_opq(ctypes.byref(s._prob), ctypes.byref(c), None, None, None, None, None,
                                           None, ctypes.byref(zero), 20.0, ctypes.byref(h)))
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
    if "heat_oph" in modes and "opq_none" in modes:
        rec["heat_oph_equals_opq_none_bitwise"] = bool(np.array_equal(first["heat_oph"], first["opq_none"]))
        rec["same_stage_variants"] = variants["heat_oph"] == variants["opq_none"]
    for m in modes:
        rec[m] = {"us_per_step": us[m], "median_us": float(np.median(us[m])),
                  "spread_us": float(max(us[m]) - min(us[m])), "first_losses": [float(x) for x in first[m]],
                  "stage_variants": variants[m]}
    if "heat_oph" in modes:
        for m in modes:
            if m != "heat_oph":
                rec[m + "_minus_heat_oph_us"] = rec[m]["median_us"] - rec["heat_oph"]["median_us"]
    rec["padded_tensor_bytes"] = 8 * int(np.prod([(n + 31) // 32 * 32 for n in ns]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--q", type=int, default=30)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--handles", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron3_opq_ab.json"))
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
