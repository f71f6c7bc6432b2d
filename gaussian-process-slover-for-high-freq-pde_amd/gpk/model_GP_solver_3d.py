"""3-axis Kronecker GP solver: the d > 2 generalisation of code/model_GP_solver_2d.py
(the reference itself stops at two axes).

Same log joint as GP_solver_2d_single (model_GP_solver_2d.py:87-183) with K = K1 (x) K2 (x) K3 on
a tensor grid: prior -1/2 c sum_k (prod_{j != k} N_j) logdet K_k - 1/2 <U, K^{-1} U> (the 2-axis
log-det weights :157-162), residual sum_k (D_k K_k^{-1}) x_k U - F [+ U(U^2-1)], boundary on the
six faces.  The whole step (assembly, SPD inverses, mode-k products, adjoints, Adam) runs on the
MI355X through gpk_create3 / gpk_step3 (include/gpk.h); there is no CPU fallback.

Same surface as the 2-axis module: GP_solver_3d_single (train with checkpoint / resume, preds,
compute_early_stopping), test() / evals() and the CLI
(`python -m gpk.model_GP_solver_3d -equation=poisson_3d-mix_sin -kernel=Matern52_Cos_1d
-nepoch=200`; `-refine=1` turns the gated refinement of every solve on), with its configs in
gpk/config3d/.

Operator equations (equations.EQUATIONS_3D_OP: heat, transport, Helmholtz, Allen-Cahn in time, the
third axis as time where one appears) run through gpk_create3_op: DeviceSolver3(operator=...),
GP_solver_3d_single with such an equation name, and the same CLI
(`-equation=heat_3d-sin`), with their configs in gpk/config3d_op/.

Mixed-order operator equations (equations.EQUATIONS_3D_OPX: convection-diffusion, a second- and a
first-order term on the same axis) run through gpk_create3_opx the same way: an Operator3X as
`operator`, `-equation=convdiff_t-sin`, configs in gpk/config3d_opx/.

Coefficient-field equations (equations.EQUATIONS_3D_OPV: Helmholtz in a medium, heat with a
conductivity field, transport in a rotating flow) run through gpk_create3_opv: an Operator3V as
`operator` (its fields evaluated on the collocation mesh), `-equation=heat_var-sin`, configs in
gpk/config3d_opv/.

Derivative boundary data (equations.EQUATIONS_3D_OPN: the wave equation with u and u_t on the
initial face, Helmholtz between sound-hard walls) runs through gpk_create3_opn:
DeviceSolver3(..., dfaces=, dvals=), trick_paras['dfaces'] / ['dvals'] or the equation's own,
`-equation=wave_t-sin`, configs in gpk/config3d_opn/.  Convective terms g_k u du/dx_k (viscous
Burgers) run through gpk_create3_opc: `-equation=burgers_t-sin`, configs in gpk/config3d_opc/.
Mixed partials m_jk d^2u/dx_j dx_k (anisotropic diffusion with off-diagonal entries) run through
gpk_create3_opm: `-equation=aniso_heat_t-sin`, configs in gpk/config3d_opm/.  Drift fields
b_k(x) du/dx_k (divergence form -div(a grad u), a variable velocity over a constant viscosity) run
through gpk_create3_opb: DeviceSolver3(..., drift=), `-equation=heat_div_t-sin`, configs in
gpk/config3d_opb/.  Third- and fourth-order terms c4_k d^4u/dx_k^4 + c3_k d^3u/dx_k^3 (KdV,
Kuramoto-Sivashinsky, the clamped beam) run through gpk_create3_oph: DeviceSolver3(..., high=(c4, c3)),
`-equation=kdv_t-sin`, configs in gpk/config3d_oph/.  Mixed fourth-order partials q_jk
d^4u/dx_j^2 dx_k^2 (the Kirchhoff plate, the biharmonic, Swift-Hohenberg) run through gpk_create3_opq:
DeviceSolver3(..., bicross=(q12, q13, q23)), `-equation=plate_t-sin`, configs in gpk/config3d_opq/.
Quadratic gradient terms s_k (du/dx_k)^2 + x_jk du/dx_j du/dx_k (eikonal, Hamilton-Jacobi, KPZ) run
through gpk_create3_opg: DeviceSolver3(..., gradsq=(s, x)), `-equation=hj_t-sin`, configs in
gpk/config3d_opg/.
"""
import ctypes
import os
import sys
import time

import numpy as np
import yaml

from . import _lib, init_func, replicas, utils
from ._lib import check, dptr, f64
from .cli import parse_flags
from .core import tree_flatten, tree_unflatten
from .equations import (EQUATIONS_3D, EQUATIONS_3D_OP, EQUATIONS_3D_OPB, EQUATIONS_3D_OPC, EQUATIONS_3D_OPH,
                        EQUATIONS_3D_OPM, EQUATIONS_3D_OPQ, solution_3d_opq, EQUATIONS_3D_OPG, solution_3d_opg,
                        EQUATIONS_3D_OPN, EQUATIONS_3D_OPV, EQUATIONS_3D_OPX, Operator3, Operator3V, Operator3X,
                        deriv_boundary_3d, drift_fields, solution_3d, solution_3d_op, solution_3d_opb,
                        solution_3d_opc, solution_3d_oph, solution_3d_opm, solution_3d_opn, solution_3d_opv, solution_3d_opx)
from .infras.exp_config import ExpConfig
from .kernel_matrix import kernel_class
from .solver_common import SolverBase


def params_template_3d(n1, n2, n3, Q):
    kp = lambda: {"freq": np.zeros(Q), "log-ls": np.zeros(Q), "log-w": np.zeros(Q)}
    return {"U": np.zeros((n1, n2, n3)), "kernel_paras_1": kp(), "kernel_paras_2": kp(),
            "kernel_paras_3": kp(), "log_tau": 0.0, "log_v": 0.0}


def boundary_3d(U, faces=63):
    """The six faces U[0], U[-1], U[:,0], U[:,-1], U[:,:,0], U[:,:,-1] (each row-major).  The
    layout and length do not depend on `faces`; the entries of a face whose bit is clear are NaN
    (an operator handle never reads them)."""
    U = np.asarray(U, np.float64)
    fs = [U[0], U[-1], U[:, 0], U[:, -1], U[:, :, 0], U[:, :, -1]]
    return np.concatenate([f.ravel() if (faces >> k) & 1 else np.full(f.size, np.nan)
                           for k, f in enumerate(fs)])


def boundary_count_3d(ns, faces=63):
    """Nb: the entries of the active faces."""
    n1, n2, n3 = ns
    return sum(s for k, s in enumerate((n2 * n3, n2 * n3, n1 * n3, n1 * n3, n1 * n2, n1 * n2)) if (faces >> k) & 1)


class DeviceSolver3:
    """One gpk_handle3: problem, params and Adam state resident on the device."""

    def __init__(self, eq, kind, xs, src, bvals, Q=30, jitter=1e-6, llk_weight=200.0, logdet=True,
                 lr=0.01, freq_scale=20.0, device=0, b1=0.9, b2=0.999, eps=1e-8, refine=False,
                 operator=None, dfaces=0, dvals=None, conv=None, cross=None, drift=None, high=None,
                 bicross=None, gradsq=None):
        """refine: one gated refinement step after every solve of the step (GPK_FLAG3_REFINE);
        'gemm' also forces its two-GEMM route (GPK_FLAG3_REFINE_GEMM; tests, A/B).
        operator: an Operator3 (or a dict of its fields) -- the handle then solves that operator
        (gpk_create3_op; eq must be 'poisson', the operator says everything else); an Operator3X
        (or a dict with 'c2' and 'c1') goes to gpk_create3_opx, which takes mixed-order axes; an
        Operator3V goes to gpk_create3_opv with its fields evaluated on the collocation mesh.
        dfaces, dvals: derivative boundary data (gpk_create3_opn): bit f of dfaces puts d u / d x_k
        (k = f // 2, along the coordinate) on face f, dvals in bvals' six-face layout (entries of
        faces outside dfaces are never read); needs an Operator3X or Operator3V (or a dict with
        'c2' and 'c1'), whose faces may then be 0.
        conv: three floats g_k, the constants of the convective terms g_k u du / dx_k
        (gpk_create3_opc; Burgers); a non-zero one needs an Operator3X or Operator3V as dfaces
        does.  None or three zeros is the handle without them.
        cross: three floats m_12, m_13, m_23, the constants of the mixed partials m_jk d^2 u /
        dx_j dx_k (gpk_create3_opm; anisotropic diffusion with off-diagonal entries); a non-zero one
        needs an Operator3X or Operator3V as conv does.  None or three zeros is the handle without
        them.
        drift: three entries b_1, b_2, b_3, the fields of the drift terms b_k(x) du / dx_k
        (gpk_create3_opb): each None, an array of the grid's shape or a callable of the three
        coordinate meshes, as Operator3V.a; the operator's fields a_k do not multiply them.  A
        non-None entry needs an Operator3X or Operator3V as conv does.  None or three Nones is the
        handle without them.
        high: (c4, c3), two triples of floats, the constants of the terms c4_k d^4 u / dx_k^4 + c3_k
        d^3 u / dx_k^3 (gpk_create3_oph; KdV, Kuramoto-Sivashinsky, the beam); a non-zero one needs
        an Operator3X or Operator3V as conv does, and an Operator3V's field a_k multiplies all four
        orders of its axis.  None or six zeros is the handle without them.
        bicross: three floats q_12, q_13, q_23, the constants of the mixed fourth-order partials q_jk
        d^4 u / dx_j^2 dx_k^2 (gpk_create3_opq; the plate, the biharmonic); a non-zero one needs an
        Operator3X or Operator3V as cross does, whose fields a_k do not multiply it.  None or three
        zeros is the handle without them.
        gradsq: (s, x), two triples of floats, the constants of the quadratic gradient terms s_k
        (du/dx_k)^2 + x_jk du/dx_j du/dx_k, x over the pairs (1,2), (1,3), (2,3) (gpk_create3_opg;
        eikonal, Hamilton-Jacobi, KPZ); a non-zero one needs an Operator3X or Operator3V as conv does,
        whose fields do not multiply it.  None or six zeros is the handle without them."""
        lib = _lib.load()
        if len(xs) != 3:
            raise ValueError("three coordinate axes")
        self._x = [f64(x).reshape(-1) for x in xs]
        self.ns = tuple(x.size for x in self._x)
        self._src = f64(src).reshape(-1)
        self._bvals = f64(bvals).reshape(-1)
        n1, n2, n3 = self.ns
        if self._src.size != n1 * n2 * n3:
            raise ValueError("src must have n1*n2*n3 entries")
        if self._bvals.size != 2 * (n2 * n3 + n1 * n3 + n1 * n2):
            raise ValueError("bvals must be the six faces of U (boundary_3d)")
        p = _lib.gpk_problem3()
        p.eq = _lib.EQ_IDS[eq]
        p.kind = _lib.KIND_IDS[kind] if isinstance(kind, str) else int(kind)
        p.n1, p.n2, p.n3, p.q = n1, n2, n3, int(Q)
        p.x1, p.x2, p.x3 = (dptr(x) for x in self._x)
        p.src, p.bvals = dptr(self._src), dptr(self._bvals)
        p.jitter, p.llk_weight, p.logdet = jitter, llk_weight, float(logdet)
        p.lr, p.b1, p.b2, p.eps = lr, b1, b2, eps
        p.device, p.flags = device, _lib.GPK_FLAG3_REFINE if refine else 0
        if refine == "gemm":
            p.flags |= _lib.GPK_FLAG3_REFINE_GEMM
        self.refine = bool(refine)
        self._prob = p
        h = ctypes.c_void_p()
        dfaces = int(dfaces)
        if conv is not None:
            conv = tuple(float(g) for g in np.asarray(conv, np.float64).reshape(-1))
            if len(conv) != 3:
                raise ValueError("conv has three entries (g_1, g_2, g_3)")
            if not any(g != 0.0 for g in conv):
                conv = None
        if cross is not None:
            cross = tuple(float(m) for m in np.asarray(cross, np.float64).reshape(-1))
            if len(cross) != 3:
                raise ValueError("cross has three entries (m_12, m_13, m_23)")
            if not any(m != 0.0 for m in cross):
                cross = None
        if drift is not None:
            drift = tuple(drift)
            if len(drift) != 3:
                raise ValueError("drift has three entries (b_1, b_2, b_3; None for an axis without a field)")
            if all(b is None for b in drift):
                drift = None
        if high is not None:
            if len(high) != 2:
                raise ValueError("high has two entries (c4, c3), each a triple")
            high = tuple(tuple(float(c) for c in np.asarray(t, np.float64).reshape(-1)) for t in high)
            if len(high[0]) != 3 or len(high[1]) != 3:
                raise ValueError("high has two entries (c4, c3), each a triple")
            if not any(c != 0.0 for t in high for c in t):
                high = None
        if bicross is not None:
            bicross = tuple(float(q) for q in np.asarray(bicross, np.float64).reshape(-1))
            if len(bicross) != 3:
                raise ValueError("bicross has three entries (q_12, q_13, q_23)")
            if not any(q != 0.0 for q in bicross):
                bicross = None
        if gradsq is not None:
            if len(gradsq) != 2:
                raise ValueError("gradsq has two entries (s, x), each a triple")
            gradsq = tuple(tuple(float(c) for c in np.asarray(t, np.float64).reshape(-1)) for t in gradsq)
            if len(gradsq[0]) != 3 or len(gradsq[1]) != 3:
                raise ValueError("gradsq has two entries (s, x), each a triple")
            if not any(c != 0.0 for t in gradsq for c in t):
                gradsq = None
        if dfaces or conv or cross or drift or high or bicross or gradsq:
            if dfaces and dvals is None:
                raise ValueError("dfaces needs dvals (the six-face layout of bvals)")
            if dfaces:
                self._dvals = f64(dvals).reshape(-1)
                if self._dvals.size != self._bvals.size:
                    raise ValueError("dvals must have the six-face layout of bvals (deriv_boundary_3d)")
            if not (isinstance(operator, (Operator3X, Operator3V)) or (isinstance(operator, dict) and "c2" in operator)):
                raise ValueError("%s needs an Operator3X or Operator3V"
                                 % ("derivative boundary data" if dfaces else "a convective term" if conv
                                    else "a mixed partial" if cross else "a drift field" if drift
                                    else "a high-order term" if high else "a mixed fourth-order partial" if bicross
                                    else "a quadratic gradient term"))
            c = _lib.gpk_operator3x()
            cf = _lib.gpk_coef3()
            if isinstance(operator, Operator3V):
                self._coef = operator.fields(self._x)
                for k, f in enumerate(self._coef[:3]):
                    if f is not None:
                        cf.a[k] = dptr(f)
                if self._coef[3] is not None:
                    cf.rho = dptr(self._coef[3])
                op = operator
            else:
                op = Operator3X.of(operator)
            c.c2[:], c.c1[:], c.react[:], c.faces = op.c2, op.c1, op.react, op.faces
            bd = _lib.gpk_bdata3()
            if dfaces:
                bd.dfaces, bd.dvals = dfaces, dptr(self._dvals)
            if high or bicross or gradsq:
                cv, mx, dr, hi = _lib.gpk_conv3(), _lib.gpk_cross3(), _lib.gpk_drift3(), _lib.gpk_high3()
                cv.g[:] = conv or (0.0, 0.0, 0.0)
                mx.m[:] = cross or (0.0, 0.0, 0.0)
                self._drift = drift_fields(drift, self._x) if drift else (None, None, None)
                for k, b in enumerate(self._drift):
                    if b is not None:
                        dr.b[k] = dptr(b)
                hi.c4[:], hi.c3[:] = high or ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
            if gradsq:
                bq, gq = _lib.gpk_bicross3(), _lib.gpk_gradsq3()
                bq.q[:] = bicross or (0.0, 0.0, 0.0)
                gq.s[:], gq.x[:] = gradsq
                check(lib.gpk_create3_opg(ctypes.byref(p), ctypes.byref(c), ctypes.byref(cf), ctypes.byref(bd),
                                          ctypes.byref(cv), ctypes.byref(mx), ctypes.byref(dr), ctypes.byref(hi),
                                          ctypes.byref(bq), ctypes.byref(gq), float(freq_scale), ctypes.byref(h)))
            elif bicross:
                bq = _lib.gpk_bicross3()
                bq.q[:] = bicross
                check(lib.gpk_create3_opq(ctypes.byref(p), ctypes.byref(c), ctypes.byref(cf), ctypes.byref(bd),
                                          ctypes.byref(cv), ctypes.byref(mx), ctypes.byref(dr), ctypes.byref(hi),
                                          ctypes.byref(bq), float(freq_scale), ctypes.byref(h)))
            elif high:
                check(lib.gpk_create3_oph(ctypes.byref(p), ctypes.byref(c), ctypes.byref(cf), ctypes.byref(bd),
                                          ctypes.byref(cv), ctypes.byref(mx), ctypes.byref(dr), ctypes.byref(hi),
                                          float(freq_scale), ctypes.byref(h)))
            elif drift:
                cv, mx, dr = _lib.gpk_conv3(), _lib.gpk_cross3(), _lib.gpk_drift3()
                cv.g[:] = conv or (0.0, 0.0, 0.0)
                mx.m[:] = cross or (0.0, 0.0, 0.0)
                self._drift = drift_fields(drift, self._x)  # (the library copies them; kept for the call)
                for k, b in enumerate(self._drift):
                    if b is not None:
                        dr.b[k] = dptr(b)
                check(lib.gpk_create3_opb(ctypes.byref(p), ctypes.byref(c), ctypes.byref(cf), ctypes.byref(bd),
                                          ctypes.byref(cv), ctypes.byref(mx), ctypes.byref(dr), float(freq_scale),
                                          ctypes.byref(h)))
            elif cross:
                cv, mx = _lib.gpk_conv3(), _lib.gpk_cross3()
                cv.g[:] = conv or (0.0, 0.0, 0.0)
                mx.m[:] = cross
                check(lib.gpk_create3_opm(ctypes.byref(p), ctypes.byref(c), ctypes.byref(cf), ctypes.byref(bd),
                                          ctypes.byref(cv), ctypes.byref(mx), float(freq_scale), ctypes.byref(h)))
            elif conv:
                cv = _lib.gpk_conv3()
                cv.g[:] = conv
                check(lib.gpk_create3_opc(ctypes.byref(p), ctypes.byref(c), ctypes.byref(cf), ctypes.byref(bd),
                                          ctypes.byref(cv), float(freq_scale), ctypes.byref(h)))
            else:
                check(lib.gpk_create3_opn(ctypes.byref(p), ctypes.byref(c), ctypes.byref(cf), ctypes.byref(bd),
                                          float(freq_scale), ctypes.byref(h)))
        elif operator is None:
            check(lib.gpk_create3(ctypes.byref(p), float(freq_scale), ctypes.byref(h)))
        elif isinstance(operator, Operator3V):
            c = _lib.gpk_operator3x()
            c.c2[:], c.c1[:], c.react[:], c.faces = operator.c2, operator.c1, operator.react, operator.faces
            self._coef = operator.fields(self._x)  # (the library copies them; kept for the call)
            cf = _lib.gpk_coef3()
            for k, f in enumerate(self._coef[:3]):
                if f is not None:
                    cf.a[k] = dptr(f)
            if self._coef[3] is not None:
                cf.rho = dptr(self._coef[3])
            check(lib.gpk_create3_opv(ctypes.byref(p), ctypes.byref(c), ctypes.byref(cf), float(freq_scale),
                                      ctypes.byref(h)))
        elif isinstance(operator, Operator3X) or (isinstance(operator, dict) and "c2" in operator):
            op = Operator3X.of(operator)
            c = _lib.gpk_operator3x()
            c.c2[:], c.c1[:], c.react[:], c.faces = op.c2, op.c1, op.react, op.faces
            check(lib.gpk_create3_opx(ctypes.byref(p), ctypes.byref(c), float(freq_scale), ctypes.byref(h)))
        else:
            op = Operator3.of(operator)
            c = _lib.gpk_operator3()
            c.order[:], c.coef[:], c.react[:], c.faces = op.order, op.coef, op.react, op.faces
            check(lib.gpk_create3_op(ctypes.byref(p), ctypes.byref(c), float(freq_scale), ctypes.byref(h)))
        self._h = h
        n = ctypes.c_int64()
        check(lib.gpk_num_params3(h, ctypes.byref(n)))
        self.nparams = n.value
        self.Q = int(Q)
        self.template = params_template_3d(n1, n2, n3, self.Q)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().gpk_destroy3(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_flat(self):
        out = np.empty(self.nparams)
        check(_lib.load().gpk_get_params3(self._h, dptr(out), self.nparams))
        return out

    def set_flat(self, flat):
        flat = f64(flat).reshape(-1)
        check(_lib.load().gpk_set_params3(self._h, dptr(flat), flat.size))

    def get_params(self):
        return tree_unflatten(self.template, self.get_flat())

    def set_params(self, params):
        self.set_flat(tree_flatten(params))

    def loss_grad(self):
        loss = ctypes.c_double()
        g = np.empty(self.nparams)
        check(_lib.load().gpk_loss_grad3(self._h, ctypes.byref(loss), dptr(g)))
        return loss.value, g

    def step(self, n=1):
        out = np.empty(max(int(n), 1))
        check(_lib.load().gpk_step3(self._h, int(n), dptr(out)))
        return out[:n]

    def sync(self):
        """gpk_step3 returns synchronised (its losses are read back): nothing left to wait for."""

    def get_opt_state(self):
        mu = np.empty(self.nparams)
        nu = np.empty(self.nparams)
        c = ctypes.c_int64()
        check(_lib.load().gpk_get_opt_state3(self._h, ctypes.byref(c), dptr(mu), dptr(nu), self.nparams))
        return int(c.value), mu, nu

    def set_opt_state(self, count, mu, nu):
        mu, nu = f64(mu).reshape(-1), f64(nu).reshape(-1)
        if mu.size != self.nparams or nu.size != self.nparams:
            raise ValueError("mu and nu must have nparams entries")
        check(_lib.load().gpk_set_opt_state3(self._h, int(count), dptr(mu), dptr(nu), self.nparams))

    def predict(self, xte1, xte2, xte3):
        """U_pred on the test grid, (m1, m2, m3), at the current params (gpk_predict3)."""
        xs = [None if x is None else f64(x).reshape(-1) for x in (xte1, xte2, xte3)]
        ms = [0 if x is None else x.size for x in xs]
        out = np.empty(max(ms[0] * ms[1] * ms[2], 1))
        check(_lib.load().gpk_predict3(self._h, *[a for x, m in zip(xs, ms)
                                                   for a in (None if x is None else dptr(x), m)],
                                       dptr(out)))
        return out[:ms[0] * ms[1] * ms[2]].reshape(ms)

    def predict_deriv(self, xte1, xte2, xte3, deriv):
        """The deriv[k]-th derivative (0, 1 or 2) along each axis of the solution on the test grid,
        (m1, m2, m3), taken in the test point (gpk_predict_deriv3).  (0, 0, 0) is predict()."""
        d = np.asarray(_lib.deriv_orders(deriv, 3), np.int32)
        xs = [None if x is None else f64(x).reshape(-1) for x in (xte1, xte2, xte3)]
        ms = [0 if x is None else x.size for x in xs]
        out = np.empty(max(ms[0] * ms[1] * ms[2], 1))
        check(_lib.load().gpk_predict_deriv3(self._h, *[a for x, m in zip(xs, ms)
                                                         for a in (None if x is None else dptr(x), m)],
                                             d.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dptr(out)))
        return out[:ms[0] * ms[1] * ms[2]].reshape(ms)

    def evaluate(self, points, deriv=(0, 0, 0)):
        """The same quantity at scattered points (m, 3), any m >= 1 (gpk_evaluate3); returns (m,)."""
        d = np.asarray(_lib.deriv_orders(deriv, 3), np.int32)
        if points is None:
            pts, m = None, 0
        else:
            pts = f64(points).reshape(-1, 3)
            m = pts.shape[0]
        out = np.empty(max(m, 1))
        check(_lib.load().gpk_evaluate3(self._h, None if pts is None else dptr(pts), m,
                                        d.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dptr(out)))
        return out[:m]

    def criterion(self):
        c = ctypes.c_double()
        check(_lib.load().gpk_criterion3(self._h, ctypes.byref(c)))
        return c.value

    def stage_variants(self):
        """The GEMM kernel of each of the step's GEMM launches, in stream order
        (_lib.GEMM_SMALL / GEMM_BIG / GEMM_TILE128; gpk_stage_variants3)."""
        out = np.zeros(32, np.int32)
        n = ctypes.c_int32()
        check(_lib.load().gpk_stage_variants3(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                              out.size, ctypes.byref(n)))
        assert n.value <= out.size
        return [int(v) for v in out[:n.value]]

    def refine_info(self):
        """The refinement gates of a refine=True solver as the last loss_grad() / step() left
        them (gpk_refine_info3): {'bound': K_00 max diag K_k^{-1} per axis, 'open': whether that
        run refined the axis's solves, 'route': _lib.REFINE_GEMM (two gated GEMMs per solve) or _lib.REFINE_FUSED (the panel kernel)}."""
        bound = np.empty(3)
        gates = np.zeros(3, np.int32)
        route = ctypes.c_int32()
        check(_lib.load().gpk_refine_info3(self._h, dptr(bound),
                                           gates.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                           ctypes.byref(route)))
        return {"bound": bound.tolist(), "open": [bool(g) for g in gates], "route": int(route.value)}

    def operator_info(self):
        """The Operator3 the handle runs (gpk_operator_info3); a handle created without
        `operator` reports its equation's equivalent."""
        c = _lib.gpk_operator3()
        check(_lib.load().gpk_operator_info3(self._h, ctypes.byref(c)))
        return Operator3(tuple(c.order), tuple(c.coef), tuple(c.react), c.faces)

    def operator_info_x(self):
        """The Operator3X the handle runs (gpk_operator_info3x): every 3-axis handle has one; a
        handle with a mixed-order axis has only this form (operator_info() raises on it)."""
        c = _lib.gpk_operator3x()
        check(_lib.load().gpk_operator_info3x(self._h, ctypes.byref(c)))
        return Operator3X(tuple(c.c2), tuple(c.c1), tuple(c.react), c.faces)

    def coef_info(self):
        """Which coefficient fields the handle has (gpk_coef_info3): (a1, a2, a3, rho) as bools;
        all False on every handle not made from an Operator3V with a field."""
        has = np.zeros(4, np.int32)
        check(_lib.load().gpk_coef_info3(self._h, has.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return tuple(bool(v) for v in has)

    def bdata_info(self):
        """(faces, dfaces): the faces that carry values and derivatives (gpk_bdata_info3); dfaces
        is 0 on every handle made without derivative data."""
        f, d = ctypes.c_int32(), ctypes.c_int32()
        check(_lib.load().gpk_bdata_info3(self._h, ctypes.byref(f), ctypes.byref(d)))
        return f.value, d.value

    def conv_info(self):
        """(g_1, g_2, g_3): the constants of the convective terms (gpk_conv_info3); zeros on every
        handle made without them."""
        g = np.zeros(3)
        check(_lib.load().gpk_conv_info3(self._h, dptr(g)))
        return tuple(g.tolist())

    def cross_info(self):
        """(m_12, m_13, m_23): the constants of the mixed partials (gpk_cross_info3); zeros on every
        handle made without them."""
        m = np.zeros(3)
        check(_lib.load().gpk_cross_info3(self._h, dptr(m)))
        return tuple(m.tolist())

    def gradsq_info(self):
        """((s_1, s_2, s_3), (x_12, x_13, x_23)) (gpk_gradsq_info3); zeros on every handle made without
        quadratic gradient terms."""
        s, x = np.zeros(3), np.zeros(3)
        check(_lib.load().gpk_gradsq_info3(self._h, dptr(s), dptr(x)))
        return tuple(s), tuple(x)

    def bicross_info(self):
        """(q_12, q_13, q_23) (gpk_bicross_info3); zeros on every handle made without bi-pairs."""
        q = np.zeros(3)
        check(_lib.load().gpk_bicross_info3(self._h, dptr(q)))
        return tuple(q)

    def high_info(self):
        """(c4, c3), two triples (gpk_high_info3); zeros on every handle made without high-order
        terms."""
        c4, c3 = np.zeros(3), np.zeros(3)
        check(_lib.load().gpk_high_info3(self._h, dptr(c4), dptr(c3)))
        return tuple(float(c) for c in c4), tuple(float(c) for c in c3)

    def drift_info(self):
        """(b_1, b_2, b_3) present, as bools (gpk_drift_info3); all False on every handle made
        without a drift field."""
        has = np.zeros(3, np.int32)
        check(_lib.load().gpk_drift_info3(self._h, has.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return tuple(bool(v) for v in has)

    def boundary_terms(self):
        """{'bgap', 'dgap', 'Nb', 'Nd'}: the value gap, the derivative gap and their entry counts
        as the last loss_grad() / step() left them (gpk_boundary_terms3)."""
        out = np.empty(4)
        check(_lib.load().gpk_boundary_terms3(self._h, dptr(out)))
        return {"bgap": out[0], "dgap": out[1], "Nb": int(out[2]), "Nd": int(out[3])}

    LOSS_TERMS = ("loss", "logdet_1", "logdet_2", "logdet_3", "quad", "egap", "bgap")

    def loss_terms(self):
        """The terms of the last loss_grad()'s loss (gpk_loss_terms3), keyed by LOSS_TERMS."""
        out = np.empty(7)
        check(_lib.load().gpk_loss_terms3(self._h, dptr(out)))
        return dict(zip(self.LOSS_TERMS, out.tolist()))


class GP_solver_3d_single(SolverBase):
    """GP_solver_2d_single's interface (model_GP_solver_2d.py:31-352) on three axes: SolverBase's
    train (checkpoint, resume, stop_at, perf_log), step(params, opt_state), preds,
    compute_early_stopping.

    bvals: boundary_3d(U) of the solution; X_col = (x, y, z); src_vals: N1 x N2 x N3;
    trick_paras: {'kernel': class, 'equation': 'poisson_3d-...' | 'allencahn_3d-...' or an
    operator equation (equations.EQUATIONS_3D_OP / EQUATIONS_3D_OPX / EQUATIONS_3D_OPV: its
    Operator3 / Operator3X / Operator3V is looked up by name, or given as trick_paras['operator']; bvals keeps the six-face layout, Nb
    counts the active faces),
    'llk_weight', 'logdet', 'lr', 'Q', 'freq_scale', 'refine'} (+ 'nepoch', 'tol' for train);
    'refine' (default False): DeviceSolver3's gated refinement of every solve;
    X_test = (x, y, z) test axes and u_test: M1 x M2 x M3, needed by train() and preds()."""

    dim = 3
    eq_types = ("poisson_3d", "allencahn_3d")
    op_eq_types = tuple(sorted({e.split("-")[0] for e in EQUATIONS_3D_OP}))
    opx_eq_types = tuple(sorted({e.split("-")[0] for e in EQUATIONS_3D_OPX}))
    opv_eq_types = tuple(sorted({e.split("-")[0] for e in EQUATIONS_3D_OPV}))
    opn_eq_types = tuple(sorted({e.split("-")[0] for e in EQUATIONS_3D_OPN}))
    opc_eq_types = tuple(sorted({e.split("-")[0] for e in EQUATIONS_3D_OPC}))
    opm_eq_types = tuple(sorted({e.split("-")[0] for e in EQUATIONS_3D_OPM}))
    opb_eq_types = tuple(sorted({e.split("-")[0] for e in EQUATIONS_3D_OPB}))
    oph_eq_types = tuple(sorted({e.split("-")[0] for e in EQUATIONS_3D_OPH}))
    opq_eq_types = tuple(sorted({e.split("-")[0] for e in EQUATIONS_3D_OPQ}))
    opg_eq_types = tuple(sorted({e.split("-")[0] for e in EQUATIONS_3D_OPG}))
    early_stop_enabled = True

    def __init__(self, bvals, X_col, src_vals, jitter, trick_paras, device=0, X_test=None, u_test=None):
        self.eq_type = trick_paras["equation"].split("-")[0]
        assert self.eq_type in (self.eq_types + self.op_eq_types + self.opx_eq_types + self.opv_eq_types
                                + self.opn_eq_types + self.opc_eq_types + self.opm_eq_types + self.opb_eq_types
                                + self.oph_eq_types + self.opq_eq_types + self.opg_eq_types)
        self.operator = None
        given = trick_paras.get("operator")
        if isinstance(given, Operator3V):
            self.operator = given
        elif isinstance(given, Operator3X) or (isinstance(given, dict) and "c2" in given):
            self.operator = Operator3X.of(given)
        elif given is not None:
            self.operator = Operator3.of(given)
        elif self.eq_type in self.op_eq_types:
            self.operator = solution_3d_op(trick_paras["equation"])[2]
        elif self.eq_type in self.opx_eq_types:
            self.operator = solution_3d_opx(trick_paras["equation"])[2]
        elif self.eq_type in self.opv_eq_types:  # (a resumed run rebuilds the fields the same way)
            self.operator = solution_3d_opv(trick_paras["equation"])[2]
        # derivative boundary data: given, or the equation's own on the collocation mesh
        self.dfaces, self.dvals = int(trick_paras.get("dfaces", 0)), trick_paras.get("dvals")
        # convective terms: given, or the equation's own (a resumed run rebuilds them from its name)
        conv = trick_paras.get("conv")
        self.conv = None if conv is None else tuple(float(g) for g in conv)
        # mixed partials: given, or the equation's own (likewise)
        cross = trick_paras.get("cross")
        self.cross = None if cross is None else tuple(float(m) for m in cross)
        # drift fields: given, or the equation's own (likewise; callables, evaluated on each mesh)
        drift = trick_paras.get("drift")
        self.drift = None if drift is None else tuple(drift)
        # high-order terms: given as (c4, c3), or the equation's own (likewise)
        high = trick_paras.get("high")
        self.high = None if high is None else tuple(tuple(float(c) for c in t) for t in high)
        # mixed fourth-order partials: given as (q12, q13, q23), or the equation's own (likewise)
        bicross = trick_paras.get("bicross")
        self.bicross = None if bicross is None else tuple(float(q) for q in bicross)
        # quadratic gradient terms: given as (s, x), or the equation's own (likewise)
        gradsq = trick_paras.get("gradsq")
        self.gradsq = None if gradsq is None else tuple(tuple(float(c) for c in t) for t in gradsq)
        if self.eq_type in (self.opn_eq_types + self.opc_eq_types + self.opm_eq_types + self.opb_eq_types
                            + self.oph_eq_types + self.opq_eq_types + self.opg_eq_types):
            if self.eq_type in self.oph_eq_types + self.opq_eq_types + self.opg_eq_types:
                if self.eq_type in self.opg_eq_types:
                    (_, _, op, dfaces, grad_u, conv, cross, drift, high, bicross,
                     gradsq) = solution_3d_opg(trick_paras["equation"])
                    if self.bicross is None:
                        self.bicross = tuple(bicross)
                    if self.gradsq is None:
                        self.gradsq = tuple(tuple(t) for t in gradsq)
                elif self.eq_type in self.opq_eq_types:
                    _, _, op, dfaces, grad_u, conv, cross, drift, high, bicross = solution_3d_opq(trick_paras["equation"])
                    if self.bicross is None:
                        self.bicross = tuple(bicross)
                else:
                    _, _, op, dfaces, grad_u, conv, cross, drift, high = solution_3d_oph(trick_paras["equation"])
                if self.conv is None:
                    self.conv = tuple(conv)
                if self.cross is None:
                    self.cross = tuple(cross)
                if self.drift is None:
                    self.drift = tuple(drift)
                if self.high is None:
                    self.high = tuple(tuple(t) for t in high)
            elif self.eq_type in self.opb_eq_types:
                _, _, op, dfaces, grad_u, conv, cross, drift = solution_3d_opb(trick_paras["equation"])
                if self.conv is None:
                    self.conv = tuple(conv)
                if self.cross is None:
                    self.cross = tuple(cross)
                if self.drift is None:
                    self.drift = tuple(drift)
            elif self.eq_type in self.opm_eq_types:
                _, _, op, dfaces, grad_u, conv, cross = solution_3d_opm(trick_paras["equation"])
                if self.conv is None:
                    self.conv = tuple(conv)
                if self.cross is None:
                    self.cross = tuple(cross)
            elif self.eq_type in self.opc_eq_types:
                _, _, op, dfaces, grad_u, conv = solution_3d_opc(trick_paras["equation"])
                if self.conv is None:
                    self.conv = tuple(conv)
            else:
                _, _, op, dfaces, grad_u = solution_3d_opn(trick_paras["equation"])
            self.operator = self.operator or op
            if "dfaces" not in trick_paras:
                self.dfaces = dfaces
            if self.dvals is None and self.dfaces:
                self.dvals = deriv_boundary_3d(grad_u, X_col, self.dfaces)
        self.cov_func = trick_paras["kernel"]()
        self.trick_paras = trick_paras
        self.bvals = np.asarray(bvals, np.float64)
        self.X_col = X_col
        self.jitter = jitter
        self.N1, self.N2, self.N3 = (np.asarray(x).size for x in X_col)
        self.Nb = (boundary_count_3d((self.N1, self.N2, self.N3), self.operator.faces if self.operator else 63)
                   + boundary_count_3d((self.N1, self.N2, self.N3), self.dfaces))  # (Nb + Nd)
        self.Nc = self.N1 * self.N2 * self.N3
        self.src_vals = np.asarray(src_vals, np.float64)
        self.llk_weight = trick_paras["llk_weight"]
        self.Xte = X_test
        self.ute = u_test
        self._make_device(device=device)

    def _make_device(self, device=0):
        tp = self.trick_paras
        eq = "poisson" if self.operator else {"poisson_3d": "poisson", "allencahn_3d": "allencahn"}[self.eq_type]
        self.dev = DeviceSolver3(eq, self.cov_func.KIND, self.X_col, self.src_vals, self.bvals,
                                 Q=tp.get("Q", 30), jitter=self.jitter, llk_weight=tp["llk_weight"],
                                 logdet=tp.get("logdet", True), lr=tp.get("lr", 0.01),
                                 freq_scale=tp.get("freq_scale", 20.0), device=int(tp.get("device", device)),
                                 refine=bool(tp.get("refine", False)), operator=self.operator,
                                 dfaces=self.dfaces, dvals=self.dvals, conv=self.conv, cross=self.cross,
                                 drift=self.drift, high=self.high, bicross=self.bicross, gradsq=self.gradsq)
        self._version = 0

    def eq_residual(self, params, X_test, src_test):
        """SolverBase.eq_residual; on an operator equation sum_k c_k d^{o_k} u / dx_k^{o_k} +
        r1 u + r2 u^2 + r3 u^3 - f from the derivative predictions (an Operator3X: sum_k (c2_k d^2
        + c1_k d) u / dx_k, zero weights skipped; an Operator3V: each axis's terms times a_k and
        rho added to r1, the fields -- callables only -- evaluated on the test mesh)."""
        op = self.operator
        if op is None:
            return SolverBase.eq_residual(self, params, X_test, src_test)
        if self.high is not None and any(c != 0.0 for t in self.high for c in t):
            raise ValueError("eq_residual: a handle with third- or fourth-order terms needs derivatives above 2 "
                             "on the test mesh, which predict_deriv does not form")
        self._sync(params)
        axes = self._test_axes(X_test)
        r = np.zeros(tuple(a.size for a in axes))
        a = [None, None, None]
        rho = None
        if isinstance(op, Operator3V):
            if not all(f is None or callable(f) for f in op.a + (op.rho,)):
                raise ValueError("eq_residual needs the coefficient fields as callables (to evaluate them on the test mesh)")
            *a, rho = op.fields(axes)
        if isinstance(op, (Operator3X, Operator3V)):
            terms = [(k, o, w) for k in range(3) for o, w in ((2, op.c2[k]), (1, op.c1[k]))]
        else:
            terms = [(k, op.order[k], op.coef[k]) for k in range(3)]
        for k, o, w in terms:
            if w != 0.0:
                d = [0, 0, 0]
                d[k] = o
                t = w * self.dev.predict_deriv(*axes, deriv=tuple(d))
                r = r + (t if a[k] is None else a[k] * t)
        if any(op.react) or rho is not None:
            u = self.dev.predict_deriv(*axes, deriv=(0, 0, 0))
            r = r + op.react[0] * u + op.react[1] * u ** 2 + op.react[2] * u ** 3
            if rho is not None:
                r = r + rho * u
        if self.conv is not None and any(self.conv):  # + u sum_k g_k du / dx_k
            u = self.dev.predict(*axes)
            for k, gk in enumerate(self.conv):
                if gk != 0.0:
                    d = [0, 0, 0]
                    d[k] = 1
                    r = r + gk * u * self.dev.predict_deriv(*axes, deriv=tuple(d))
        if self.cross is not None and any(self.cross):  # + sum_{j<k} m_jk d^2 u / dx_j dx_k
            for (j, k), m in zip(((0, 1), (0, 2), (1, 2)), self.cross):
                if m != 0.0:
                    d = [0, 0, 0]
                    d[j] = d[k] = 1
                    r = r + m * self.dev.predict_deriv(*axes, deriv=tuple(d))
        if self.drift is not None and any(b is not None for b in self.drift):  # + sum_k b_k(x_test) du / dx_k
            if not all(b is None or callable(b) for b in self.drift):
                raise ValueError("eq_residual needs the drift fields as callables (to evaluate them on the test mesh)")
            for k, b in enumerate(drift_fields(self.drift, axes)):
                if b is not None:
                    d = [0, 0, 0]
                    d[k] = 1
                    r = r + b * self.dev.predict_deriv(*axes, deriv=tuple(d))
        if self.bicross is not None and any(self.bicross):  # + sum_{j<k} q_jk d^4 u / dx_j^2 dx_k^2
            for (j, k), q in zip(((0, 1), (0, 2), (1, 2)), self.bicross):
                if q != 0.0:
                    d = [0, 0, 0]
                    d[j] = d[k] = 2
                    r = r + q * self.dev.predict_deriv(*axes, deriv=tuple(d))
        if self.gradsq is not None and any(c != 0.0 for t in self.gradsq for c in t):
            # + sum_k s_k (du / dx_k)^2 + sum_{j<k} x_jk du / dx_j du / dx_k
            gs, gx = self.gradsq
            on = [gs[0] != 0.0 or gx[0] != 0.0 or gx[1] != 0.0, gs[1] != 0.0 or gx[0] != 0.0 or gx[2] != 0.0,
                  gs[2] != 0.0 or gx[1] != 0.0 or gx[2] != 0.0]
            du = [self.dev.predict_deriv(*axes, deriv=tuple(int(j == k) for j in range(3))) if on[k] else None
                  for k in range(3)]
            for k in range(3):
                if gs[k] != 0.0:
                    r = r + gs[k] * du[k] ** 2
            for (j, k), w in zip(((0, 1), (0, 2), (1, 2)), gx):
                if w != 0.0:
                    r = r + w * du[j] * du[k]
        return r - np.asarray(src_test, np.float64).reshape(r.shape)

    # the device holds the params: reading fetches them, train()'s final assignment is a no-op
    @property
    def params(self):
        return self.dev.get_params()

    @params.setter
    def params(self, value):
        pass

    def init_params(self):
        """The 2-axis train() init (model_GP_solver_2d.py:245-261) with a third factor."""
        Q, fs = self.dev.Q, float(self.trick_paras.get("freq_scale", 20.0))
        kp = lambda: {"log-w": np.log(1 / Q) * np.ones(Q), "log-ls": np.zeros(Q),
                      "freq": np.linspace(0, 1, Q) * fs}
        return {"log_tau": 0.0, "log_v": 0.0, "kernel_paras_1": kp(), "kernel_paras_2": kp(),
                "kernel_paras_3": kp(), "U": np.zeros((self.N1, self.N2, self.N3))}

    def loss(self, params, key=None):
        """Negative log joint at params (model_GP_solver_2d.py:145-174 on three axes)."""
        self._sync(params)
        return self.dev.loss_grad()[0]

    def value_and_grad(self, params, key=None):
        self._sync(params)
        loss, g = self.dev.loss_grad()
        return loss, tree_unflatten(self.dev.template, g)

    def step(self, params=1, opt_state=None, key=None):
        """step(n): n Adam steps, the per-step losses.  step(params, opt_state[, key]): one step
        in the reference's form (model_GP_solver_2d.py:176-183), (params, opt_state, loss)."""
        if isinstance(params, (int, np.integer)):
            losses = self.dev.step(int(params))
            self._version += 1
            return losses
        return SolverBase.step(self, params, opt_state, key)

    def steps(self, n):
        """n steps in device batches of at most 4096 (gpk_step3's loss buffer); the n losses."""
        out = [self.dev.step(min(4096, n - k)) for k in range(0, n, 4096)]
        self._version += 1
        return np.concatenate(out) if out else np.zeros(0)

    def preds(self, params):
        """U_pred on the test grid, axis after axis as 2d.py:185-220 (gpk_predict3)."""
        if self.Xte is None:
            raise ValueError("preds() needs X_test")
        self._sync(params)
        return self.dev.predict(*self.Xte), None

    def _err(self, params):
        if self.ute is None:
            raise ValueError("the relative L2 error needs u_test")
        preds, _ = self.preds(params)
        ute = np.asarray(self.ute).reshape(-1)
        return float(np.linalg.norm(preds.reshape(-1) - ute) / np.linalg.norm(ute))

    def _kernel_lists(self, params, log):
        for a in (1, 2, 3):
            kp = params["kernel_paras_%d" % a]
            log.setdefault("w_list_k%d" % a, []).append(np.exp(kp["log-w"]))
            log.setdefault("freq_list_k%d" % a, []).append(np.asarray(kp["freq"]))
            log.setdefault("ls_list_k%d" % a, []).append(np.exp(kp["log-ls"]))

    def _finish_log(self, log):
        keys = ["loss_list", "err_list"] + ["%s_list_k%d" % (w, a) for a in (1, 2, 3)
                                             for w in ("w", "freq", "ls")] + ["epoch_list"]
        return {k: log.get(k, []) for k in keys}


# ---------------------------------------------------------------------------------------
# experiment driver (the 2-axis module's test() / evals(), 2d.py:355-510, on three axes)
# ---------------------------------------------------------------------------------------
def get_mesh_data(u, Ms, scale):
    """(axes, u_mesh) on linspace(0,1,M_k)*scale per axis (2d.py:369-374)."""
    axes = [np.linspace(0, 1, num=M) * scale for M in Ms]
    mesh = np.meshgrid(*axes, indexing="ij")
    return axes, u(*mesh) * np.ones_like(mesh[0])


SOLVER = GP_solver_3d_single


def test(trick_paras, solver_cls=None):
    """Run num_fold trainings of one equation and write result_log (2d.py:382-464)."""
    solver_cls = solver_cls or SOLVER
    op = None
    if trick_paras["equation"] in EQUATIONS_3D_OP:
        u, src, op = solution_3d_op(trick_paras["equation"])
    elif trick_paras["equation"] in EQUATIONS_3D_OPX:
        u, src, op = solution_3d_opx(trick_paras["equation"])
    elif trick_paras["equation"] in EQUATIONS_3D_OPV:
        u, src, op = solution_3d_opv(trick_paras["equation"])
    elif trick_paras["equation"] in EQUATIONS_3D_OPN:  # (the solver lays its own dvals out)
        u, src, op = solution_3d_opn(trick_paras["equation"])[:3]
    elif trick_paras["equation"] in EQUATIONS_3D_OPC:  # (... and looks its conv up)
        u, src, op = solution_3d_opc(trick_paras["equation"])[:3]
    elif trick_paras["equation"] in EQUATIONS_3D_OPM:  # (... and its cross weights)
        u, src, op = solution_3d_opm(trick_paras["equation"])[:3]
    elif trick_paras["equation"] in EQUATIONS_3D_OPB:  # (... and its drift fields)
        u, src, op = solution_3d_opb(trick_paras["equation"])[:3]
    elif trick_paras["equation"] in EQUATIONS_3D_OPH:  # (... and its high-order weights)
        u, src, op = solution_3d_oph(trick_paras["equation"])[:3]
    elif trick_paras["equation"] in EQUATIONS_3D_OPQ:  # (... and its bi-pair weights)
        u, src, op = solution_3d_opq(trick_paras["equation"])[:3]
    elif trick_paras["equation"] in EQUATIONS_3D_OPG:  # (... and its quadratic gradient weights)
        u, src, op = solution_3d_opg(trick_paras["equation"])[:3]
    else:
        u, src = solution_3d(trick_paras["equation"])
    scale = trick_paras["scale"]
    M, N = trick_paras["M_test"], trick_paras["N_col"]
    X_test, u_test = get_mesh_data(u, (M, M, M), scale)
    X_col, u_mh = get_mesh_data(u, (N, N, N), scale)
    bvals = boundary_3d(u_mh, op.faces if op else 63)
    _, src_vals = get_mesh_data(src, (N, N, N), scale)
    ctx = replicas.init()
    if ctx.world > 1:
        trick_paras = dict(trick_paras, device=ctx.local)
    results = {}
    start_time = time.time()
    model = None
    for fold in replicas.owned(trick_paras["num_fold"], ctx):
        print("fold %d training" % fold)
        model = solver_cls(bvals, X_col, src_vals, 1e-6, trick_paras, X_test=X_test, u_test=u_test)
        log_dict, early_stopping, min_err = model.train(trick_paras["nepoch"], fold)
        results[fold] = (min_err, early_stopping["epoch"])
        if fold == 0:
            utils.store_model(model, log_dict, trick_paras)
    allres = replicas.gather_by_index(results, trick_paras["num_fold"], ctx)
    err_list = [r[0] for r in allres]
    early_stopping_list = [r[1] for r in allres]
    end_time = time.time()
    err_dict = {"mean": np.mean(err_list), "std": np.std(err_list), "err_list": err_list,
                "stop_epoch_mean": np.mean(early_stopping_list), "used_time": end_time - start_time,
                "avg_time": (end_time - start_time) / trick_paras["num_fold"]}
    if ctx.rank == 0:
        utils.wrirte_log(model, err_dict, trick_paras)
        print("finish writing log ...")
    return err_dict


def load_config(equation):
    """./config3d/<equation>.yaml (the operator equations: ./config3d_op/, the mixed-order ones:
    ./config3d_opx/, the coefficient-field ones: ./config3d_opv/, derivative boundary data:
    ./config3d_opn/, convective terms: ./config3d_opc/, mixed partials: ./config3d_opm/, drift fields:
    ./config3d_opb/, third- and fourth-order terms: ./config3d_oph/, mixed fourth-order partials:
    ./config3d_opq/, quadratic gradient terms: ./config3d_opg/), falling back to the package's copy."""
    cdir = ("config3d_op" if equation in EQUATIONS_3D_OP else "config3d_opx" if equation in EQUATIONS_3D_OPX
            else "config3d_opv" if equation in EQUATIONS_3D_OPV else "config3d_opn" if equation in EQUATIONS_3D_OPN
            else "config3d_opc" if equation in EQUATIONS_3D_OPC
            else "config3d_opm" if equation in EQUATIONS_3D_OPM
            else "config3d_opb" if equation in EQUATIONS_3D_OPB
            else "config3d_oph" if equation in EQUATIONS_3D_OPH
            else "config3d_opq" if equation in EQUATIONS_3D_OPQ
            else "config3d_opg" if equation in EQUATIONS_3D_OPG else "config3d")
    for base in (os.getcwd(), os.path.dirname(os.path.abspath(__file__))):
        p = os.path.join(base, cdir, equation + ".yaml")
        if os.path.exists(p):
            with open(p, "r") as f:
                return yaml.safe_load(f)
    raise FileNotFoundError(cdir + "/" + equation + ".yaml")


def build_config(args, allowed=EQUATIONS_3D + EQUATIONS_3D_OP + EQUATIONS_3D_OPX + EQUATIONS_3D_OPV
                 + EQUATIONS_3D_OPN + EQUATIONS_3D_OPC + EQUATIONS_3D_OPM + EQUATIONS_3D_OPB + EQUATIONS_3D_OPH
                 + EQUATIONS_3D_OPQ + EQUATIONS_3D_OPG):
    """The 2-axis build_config (scale, kernel class, other_paras) on the config3d files."""
    assert args.equation in allowed
    config = load_config(args.equation)
    config["equation"] = args.equation
    config["init_u_trick"] = init_func.zeros
    config["kernel_extra"] = None
    config["scale"] = 2 * np.pi if config["scale"] == "2pi" else 1.0
    if args.nepoch is not None:
        config["nepoch"] = args.nepoch
    config["kernel"] = kernel_class(args.kernel)
    if getattr(args, "device", None) is not None:
        config["device"] = int(args.device)
    if getattr(args, "refine", None) is not None:
        config["refine"] = bool(args.refine)
    print("equation: %s, kernel: %s, freq_scale: %d" % (config["equation"], config["kernel"].__name__,
                                                        config["freq_scale"]))
    config["other_paras"] = config["other_paras"] + "-Ncol-%d" % config["N_col"]
    return config


def evals(**kwargs):
    args = ExpConfig()
    args.parse(kwargs)
    return test(build_config(args))


def main(argv=None):
    return evals(**parse_flags(sys.argv[1:] if argv is None else argv))


if __name__ == "__main__":
    main()
