"""Step time of 3-axis handles with quadratic gradient terms (gpk_create3_opg).

Grid: n^3 on [0, 1] (64 and 256), Q = 30, Matern52_Cos_1d, at the initial params (the data only
sets the values, not the work).  The heat form c2 (-nu, -nu, 0), c1 (0, 0, 1), final-time face
open, with
    heat_opq    no quadratic term, the handle made by gpk_create3_opq itself (called with no fields, no
                derivative data, no convective axis, no pair, no drift, no high-order weight and no
                bi-pair; the mode that also runs on the parent commit)
    opg_none    the same through gpk_create3_opg with zero weights: the same captured graph (its losses
                are checked bitwise equal to heat_opq's)
    sq_1 / sq_2 / sq_3   one s_k (axis 2: P_2 and Q_2 in the permuted layout; axis 3: D1 on the right)
    sq_12x      s_1, s_2 and x_12
    hj          hj_t-sin's form: nu = 0.05, s = (1/2, 1/2, 0)
    conv_12     the convective form g = (1, 1, 0), for comparison (gpk_create3_opc's launches)
Fresh handles per mode, interleaved mode by mode; each handle: a warm-up call (graph capture, code
objects), then the host clock around `steps` graph launches of one synchronous gpk_step3 call.
Median and spread (max - min) over the handles.  Writes JSON (default profiles/kron3_opg_ab.json).

--modes A,B: only those modes (heat_opq and conv_12 need nothing of this feature, so the same file
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
Z3 = (0.0, 0.0, 0.0)
SW = 0.5
# mode -> DeviceSolver3 keywords (None: the handle comes from gpk_create3_opq; (): gpk_create3_opg with zeros)
MODES = {"heat_opq": None, "opg_none": (), "sq_1": dict(gradsq=((SW, 0.0, 0.0), Z3)),
         "sq_2": dict(gradsq=((0.0, SW, 0.0), Z3)), "sq_3": dict(gradsq=((0.0, 0.0, SW), Z3)),
         "sq_12x": dict(gradsq=((SW, SW, 0.0), (0.3, 0.0, 0.0))), "hj": "hj", "conv_12": dict(conv=(1.0, 1.0, 0.0))}


def solver(ns, q, mode):
    u, _ = solution_3d("allencahn_3d-sin")
    xs = [np.linspace(0, 1, n) for n in ns]
    g = np.meshgrid(*xs, indexing="ij")
    kw, op = MODES[mode], HEAT
    if kw == "hj":
        op = Operator3X((-0.05, -0.05, 0.0), (0.0, 0.0, 1.0), faces=0b011111)
        kw = dict(gradsq=((0.5, 0.5, 0.0), Z3))
    s = DeviceSolver3("poisson", "Matern52_Cos_1d", xs, -12.0 * u(*g), boundary_3d(u(*g)), Q=q, operator=op,
                      **(kw or {}))
    if not kw:  # the same problem through gpk_create3_opq, or through gpk_create3_opg with zero weights: the
        lib = _lib.load()  # handle is replaced by that call's
        _lib.check(lib.gpk_destroy3(s._h))
        s._h = None
        c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
        c.c2[:], c.c1[:], c.react[:], c.faces = op.c2, op.c1, op.react, op.faces
        if kw is None:
            _lib.check(lib.gpk_create3_opq(ctypes.byref(s._prob), ctypes.byref(c), None, None, None, None, None,
                                           None, None, 20.0, ctypes.byref(h)))
        else:
            zero = _lib.gpk_gradsq3()
            _lib.check(lib.gpk_create3_opg(ctypes.byref(s._prob), ctypes.byref(c), None, None, None, None, None,
                                           None, None, ctypes.byref(zero), 20.0, ctypes.byref(h)))
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
    if "heat_opq" in modes and "opg_none" in modes:
        rec["heat_opq_equals_opg_none_bitwise"] = bool(np.array_equal(first["heat_opq"], first["opg_none"]))
        rec["same_stage_variants"] = variants["heat_opq"] == variants["opg_none"]
    for m in modes:
        rec[m] = {"us_per_step": us[m], "median_us": float(np.median(us[m])),
                  "spread_us": float(max(us[m]) - min(us[m])), "first_losses": [float(x) for x in first[m]],
                  "stage_variants": variants[m]}
    if "heat_opq" in modes:
        for m in modes:
            if m != "heat_opq":
                rec[m + "_minus_heat_opq_us"] = rec[m]["median_us"] - rec["heat_opq"]["median_us"]
    rec["padded_tensor_bytes"] = 8 * int(np.prod([(n + 31) // 32 * 32 for n in ns]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--q", type=int, default=30)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--handles", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron3_opg_ab.json"))
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
