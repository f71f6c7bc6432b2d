"""Derivative boundary data on the 3-axis solver (gpk_create3_opn; DeviceSolver3 with dfaces /
dvals): d u / d x_k on faces of axis k, predicted as one row of the order-1 block contracted with
A_k = K_k^{-1} x_k U (k3_face_row, k3_face_gap) and fed back into T_k and the kernel-parameter
partials (k3_face_back, k3_face_tail).

Yardstick: tests/operator3n_ref.py loss_grad_3d_opn (pinned on the CPU by
tests/test_operator3n_ref.py).  Tolerance: that of tests/test_gpu_kron3.py, max(1e-10, 50 cond eps)
with the largest cond K_k, on the loss and on every gradient block.  Every bvals / dvals entry that
must not be read is NaN throughout.  Handles without derivative faces are compared with
gpk_create3_opv's bit for bit.
"""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import rel
from tests.operator3_ref import FACES
from tests.operator3n_ref import adam_replay_n, criterion_3d_opn, face_data, loss_grad_3d_opn
from tests.test_gpu_kron3 import KINDS, _tol
from tests.test_gpu_kron3_operator import _mask_bvals, _problem
from tests.test_gpu_kron3_opv import FULL, NO_COEF
from tests.test_operator3n_ref import random_dvals
from tests.test_operator3v_ref import smooth_fields

pytestmark = pytest.mark.gpu


def _make(prob, Q, fs, op, coef, dfaces, dvals, refine=False):
    from gpk.equations import Operator3V
    from gpk.model_GP_solver_3d import DeviceSolver3
    return DeviceSolver3("poisson", prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                         Q=Q, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"], lr=0.01,
                         freq_scale=fs, refine=refine,
                         operator=Operator3V(op["c2"], op["c1"], op["react"], op["faces"], a=coef["a"], rho=coef["rho"]),
                         dfaces=dfaces, dvals=dvals)


def _check(label, loss, g, prob, params, op, coef, dfaces, dvals, tol=None):
    lo, go = loss_grad_3d_opn(prob, params, op, coef, dfaces, dvals)
    tol = _tol(prob, params) if tol is None else tol
    gd = O.unflatten_params(params, g)
    errs = {k: rel(O.flatten_params(gd[k]), O.flatten_params(go[k])) for k in go}
    errs["loss"] = abs(loss - lo) / abs(lo)
    print(label, "tol %.3e" % tol, {k: "%.3e" % v for k, v in errs.items()})
    assert np.isfinite(loss) and np.all(np.isfinite(g))
    for k, v in errs.items():
        assert v < tol, (label, k, v, tol)


def _setup(ns, op, dfaces, kind="Matern52_Cos_1d", Q=4, seed=3, unit=False):
    prob, params, fs = _problem(ns, kind, Q, seed, unit)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    return prob, params, fs, random_dvals(ns, dfaces, seed=dfaces)


def _run(ns, op, coef, dfaces, kind="Matern52_Cos_1d", Q=4, label="", refine=False, unit=False):
    prob, params, fs, dvals = _setup(ns, op, dfaces, kind, Q, unit=unit)
    s = _make(prob, Q, fs, op, coef, dfaces, dvals, refine=refine)
    try:
        s.set_params(params)
        assert s.bdata_info() == (op["faces"], dfaces)
        loss, g = s.loss_grad()
        info = s.refine_info() if refine else None
    finally:
        s.close()
    _check("%s %s %s Q%d dfaces %s" % (label, ns, kind, Q, bin(dfaces)), loss, g, prob, params, op, coef, dfaces, dvals)
    return info


# ---- 1. one axis at a time, crossing a 32-tile on the face's axis --------------------------------
@pytest.mark.parametrize("ns,axis", [((33, 20, 9), 0), ((20, 33, 9), 1), ((9, 20, 33), 2)])
def test_both_faces_of_one_axis_tile_crossing_on_the_axis(ns, axis):
    _run(ns, FULL, NO_COEF, 0b11 << (2 * axis), label="axis %d" % (axis + 1))


# ---- 2. the same three axes, crossing a 32-tile inside the face plane ----------------------------
@pytest.mark.parametrize("ns,axis", [((9, 33, 20), 0), ((33, 9, 20), 1), ((20, 33, 9), 2)])
def test_both_faces_of_one_axis_tile_crossing_in_the_face_plane(ns, axis):
    assert 33 in [n for a, n in enumerate(ns) if a != axis]
    _run(ns, FULL, NO_COEF, 0b11 << (2 * axis), label="plane of axis %d" % (axis + 1))


# ---- 3. n = 2 on the axis: the rows are i_f = 0 and 1 --------------------------------------------
@pytest.mark.parametrize("ns,axis", [((2, 14, 9), 0), ((9, 2, 14), 1), ((9, 14, 2), 2)])
def test_two_points_on_the_axis(ns, axis):
    _run(ns, FULL, NO_COEF, 0b11 << (2 * axis), label="n = 2")


# ---- 4. everything at once -----------------------------------------------------------------------
ALL_OP, ALL_DFACES = dict(FULL, faces=0b011011), 0b110110  # faces 1 and 4 carry both kinds


@pytest.mark.parametrize("kind", KINDS)
def test_everything_at_once_every_kind(kind):
    ns = (33, 33, 9)
    _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=5), ALL_DFACES, kind, label="all")


def test_everything_at_once_q64():
    ns = (33, 33, 9)
    _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=5), ALL_DFACES, Q=64, label="all")


# ---- 5. derivative data alone --------------------------------------------------------------------
def test_no_value_faces_helmholtz_with_a_reaction():
    helm = dict(c2=(1.0, 1.0, 1.0), c1=(0.0, 0.0, 0.0), react=(9.0, 0.0, 0.0), faces=0)
    ns = (20, 14, 9)
    prob, _, _, _ = _setup(ns, helm, 63)
    assert np.all(np.isnan(prob["bvals"]))
    _run(ns, helm, NO_COEF, 63, label="faces = 0")


# ---- 6. refinement -------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [True, "gemm"])
def test_refined_both_routes(refine):
    """x in [0, 1] at (33, 20, 9): the gates open; T_k takes the faces' term before the refinement of
    X_k reads it as its right-hand side, on the fused route and on the two-GEMM route."""
    from gpk import _lib
    ns = (33, 20, 9)
    info = _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=7), ALL_DFACES, label="refined %r" % refine,
                refine=refine, unit=True)
    assert info["route"] == (_lib.REFINE_FUSED if refine is True else _lib.REFINE_GEMM)
    assert any(info["open"]), info


# ---- 7. boundary terms, loss terms and the criterion ---------------------------------------------
def test_boundary_terms_loss_terms_and_criterion():
    ns = (20, 14, 9)
    prob, params, fs, dvals = _setup(ns, ALL_OP, ALL_DFACES)
    coef = smooth_fields(ns, (0, 1, 2, 3), seed=6)
    s = _make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals)
    try:
        s.set_params(params)
        loss, _ = s.loss_grad()
        terms, bt, crit = s.loss_terms(), s.boundary_terms(), s.criterion()
    finally:
        s.close()
    t = {}
    loss_grad_3d_opn(prob, params, ALL_OP, coef, ALL_DFACES, dvals, terms=t)
    tol = _tol(prob, params)
    cref = criterion_3d_opn(prob, params, ALL_OP, coef, ALL_DFACES, dvals)
    print("terms", terms, "yardstick", t, "boundary", bt, "criterion", crit, cref, "tol", tol)
    assert terms["loss"] == loss
    assert bt["Nb"] == t["Nb"] and bt["Nd"] == t["Nd"] and t["Nd"] == 14 * 9 + 20 * 9 + 2 * 20 * 14
    assert abs(bt["bgap"] - t["bgap"]) < tol * t["bgap"] and abs(bt["dgap"] - t["dgap"]) < tol * t["dgap"]
    assert terms["bgap"] == bt["bgap"] + bt["dgap"]
    expect = dict(t, bgap=t["bgap"] + t["dgap"])
    for k in terms:  # (a log det is a sum of O(1) log pivots: its error is measured against at least 1)
        assert abs(terms[k] - expect[k]) < tol * max(abs(expect[k]), 1.0), k
    assert abs(crit - cref) < tol * cref


# ---- 8. the derivative gap by an independent route -----------------------------------------------
def test_derivative_gap_from_predict_deriv_at_the_collocation_axes():
    """predict_deriv at the collocation axes, restricted to the faces, is d_f ._k A_k again when
    Kmn_j K_j^{-1} is the identity on the other axes, i.e. at jitter = 0 (with a jitter the two
    differ by jitter K_j^{-1}, which is no rounding error): the problem here has none.  Each side
    is within _tol of the yardstick, so they agree within 2 _tol."""
    ns = (14, 12, 9)
    prob, params, fs, dvals = _setup(ns, ALL_OP, ALL_DFACES)
    prob = dict(prob, jitter=0.0)
    s = _make(prob, 4, fs, ALL_OP, NO_COEF, ALL_DFACES, dvals)
    try:
        s.set_params(params)
        s.loss_grad()
        dgap = s.boundary_terms()["dgap"]
        xs = (prob["x1"], prob["x2"], prob["x3"])
        pred = [s.predict_deriv(*xs, deriv=tuple(int(a == k) for a in range(3))) for k in range(3)]
    finally:
        s.close()
    again = sum(float(np.sum((pred[f // 2][FACES[f]] - h) ** 2)) for f, h in face_data(dvals, ns, ALL_DFACES).items())
    t = {}
    loss_grad_3d_opn(prob, params, ALL_OP, NO_COEF, ALL_DFACES, dvals, terms=t)
    tol = _tol(prob, params)
    print("dgap", dgap, "from predict_deriv", again, "yardstick", t["dgap"], "rel", abs(dgap - again) / again, "tol", tol)
    assert abs(dgap - again) <= 2 * tol * again


# ---- 9. bits -------------------------------------------------------------------------------------
def _raw_opn(prob, Q, fs, op, coef, bd, refine=False):
    """A DeviceSolver3 whose handle comes from gpk_create3_opn called directly with `bd` (None: a
    NULL pointer; else a _lib.gpk_bdata3)."""
    from gpk import _lib
    from gpk._lib import dptr
    s = _make(prob, Q, fs, op, coef, 0, None, refine=refine)
    lib = _lib.load()
    _lib.check(lib.gpk_destroy3(s._h))
    s._h = None
    c, h, cf = _lib.gpk_operator3x(), ctypes.c_void_p(), _lib.gpk_coef3()
    c.c2[:], c.c1[:], c.react[:], c.faces = op["c2"], op["c1"], op["react"], op["faces"]
    for k, f in enumerate(getattr(s, "_coef", [None] * 4)[:3]):
        if f is not None:
            cf.a[k] = dptr(f)
    if getattr(s, "_coef", [None] * 4)[3] is not None:
        cf.rho = dptr(s._coef[3])
    _lib.check(lib.gpk_create3_opn(ctypes.byref(s._prob), ctypes.byref(c), ctypes.byref(cf),
                                   None if bd is None else ctypes.byref(bd), float(fs), ctypes.byref(h)))
    s._h = h
    return s


@pytest.mark.parametrize("fields", [(), (0, 1, 2, 3)])
def test_no_derivative_faces_is_the_create3_opv_handle_bitwise(fields):
    from gpk import _lib
    from gpk._lib import dptr
    ns = (33, 20, 9)
    prob, params, fs, _ = _setup(ns, FULL, 0)
    coef = smooth_fields(ns, fields, seed=4)
    nan = np.full(prob["bvals"].size, np.nan)
    b0 = _lib.gpk_bdata3()
    b0.dvals = dptr(nan)
    hs = [_make(prob, 4, fs, FULL, coef, 0, None), _raw_opn(prob, 4, fs, FULL, coef, None),
          _raw_opn(prob, 4, fs, FULL, coef, b0), _make(prob, 4, fs, FULL, coef, 0, nan)]
    try:
        for s in hs:
            s.set_params(params)
            assert s.bdata_info() == (FULL["faces"], 0)
        ref = hs[0].loss_grad()
        for s in hs[1:]:
            l, g = s.loss_grad()
            assert l == ref[0] and np.array_equal(g, ref[1])
            assert s.stage_variants() == hs[0].stage_variants()
            assert s.loss_terms() == hs[0].loss_terms()
            bt = s.boundary_terms()
            assert bt["dgap"] == 0.0 and bt["Nd"] == 0 and bt["bgap"] == s.loss_terms()["bgap"]
        steps = [s.step(3) for s in hs]
        for x in steps[1:]:
            assert np.array_equal(x, steps[0])
    finally:
        for s in hs:
            s.close()


def test_repeated_calls_equal_bits_and_step_is_loss_grad_plus_apply():
    ns = (33, 20, 9)
    prob, params, fs, dvals = _setup(ns, ALL_OP, ALL_DFACES)
    coef = smooth_fields(ns, (0, 1, 2, 3), seed=4)
    a, b = (_make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals) for _ in range(2))
    try:
        for s in (a, b):
            s.set_params(params)
        (l1, g1), (l2, g2) = a.loss_grad(), a.loss_grad()
        assert l1 == l2 and np.array_equal(g1, g2)
        assert a.boundary_terms() == a.boundary_terms()
        losses = a.step(3)
        single = []
        for _ in range(3):  # loss_grad at the params the step starts from, then that step alone
            single.append(b.loss_grad()[0])
            assert b.step(1)[0] == single[-1]
        assert np.array_equal(losses, np.asarray(single))
        assert np.array_equal(a.get_flat(), b.get_flat())
    finally:
        a.close()
        b.close()


# ---- 10. Adam trajectory -------------------------------------------------------------------------
def test_adam_trajectory_vs_replay():
    """Five steps under the bars of tests/test_gpu_kron3_opv.py's trajectory."""
    ns = (20, 14, 9)
    prob, params, fs, dvals = _setup(ns, ALL_OP, ALL_DFACES, Q=5, seed=8)
    coef = smooth_fields(ns, (0, 3), seed=8)
    s = _make(prob, 5, fs, ALL_OP, coef, ALL_DFACES, dvals)
    try:
        s.set_params(params)
        losses = s.step(5)
        flat = s.get_flat()
    finally:
        s.close()
    ref, p = adam_replay_n(prob, params, ALL_OP, coef, ALL_DFACES, dvals, 5)
    tol = _tol(prob, params)
    print("adam opn", rel(losses, ref), rel(flat, O.flatten_params(p)), "tol", tol)
    assert rel(losses, ref) < max(1e-9, tol)
    assert rel(flat, O.flatten_params(p)) < max(1e-8, 10 * tol)


# ---- 11. the wave equation through the model class -----------------------------------------------
def test_wave_equation_through_the_model_class():
    from gpk.equations import solution_3d_opn
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single, boundary_3d, get_mesh_data, load_config
    cfg = load_config("wave_t-sin")
    u, src, op, dfaces, _ = solution_3d_opn("wave_t-sin")
    xc, umh = get_mesh_data(u, (12,) * 3, 1.0)
    _, srcv = get_mesh_data(src, (12,) * 3, 1.0)
    bvals = boundary_3d(umh, op.faces)
    tp = {"kernel": kernel_class("Matern52_Cos_1d"), "equation": "wave_t-sin", "llk_weight": cfg["llk_weight"],
          "logdet": cfg["logdet"], "lr": cfg["lr"], "Q": cfg["Q"], "freq_scale": cfg["freq_scale"]}
    m = GP_solver_3d_single(bvals, xc, srcv, 1e-6, tp)
    try:
        assert m.dev.bdata_info() == (0b011111, 0b010000) and m.dev.operator_info_x() == op
        assert m.Nb == 5 * 144 + 144
        assert np.isnan(m.dvals).sum() == m.dvals.size - 144
        losses = m.step(50)
        bt = m.dev.boundary_terms()
        flat = m.dev.get_flat()
    finally:
        m.dev.close()
    print("wave_t-sin losses", losses[0], losses[-1], "boundary terms", bt)
    assert losses.shape == (50,) and np.all(np.isfinite(losses)) and np.all(np.isfinite(flat))
    assert bt["Nb"] == 5 * 144 and bt["Nd"] == 144 and np.isfinite(bt["dgap"]) and bt["dgap"] >= 0.0
