"""Drift fields on the 3-axis solver (gpk_create3_opb; DeviceSolver3 with drift): b_k(x) du / dx_k
per axis, formed as b_k . (D1_k x_k A_k) from the order-1 block of the two-block assembly
(DERIV_SPLIT), added to the residual by k3_combine_b, and carried back through E_k = b_k R into T_k
and G_D1k (build_drift_stages).

Yardstick: tests/operator3b_ref.py loss_grad_3d_opb (pinned on the CPU by
tests/test_operator3b_ref.py).  Tolerance: the project's _tol, max(1e-10, 50 cond eps) with the
largest cond K_k, on the loss and on every gradient block.  Every bvals / dvals entry that must not
be read is NaN throughout.  Each case asserts that the yardstick without the drift is another loss
(and that leaving the drift out moves some checked quantity by more than 100 tolerances).
Handles without a drift field are compared with gpk_create3_opm's bit for bit.
"""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import rel
from tests.operator3b_ref import adam_replay_b, criterion_3d_opb, loss_grad_3d_opb
from tests.operator3m_ref import loss_grad_3d_opm
from tests.test_gpu_kron3 import KINDS, _tol
from tests.test_gpu_kron3_operator import _mask_bvals, _problem
from tests.test_gpu_kron3_opn import ALL_DFACES, ALL_OP
from tests.test_gpu_kron3_opv import FULL, NO_COEF
from tests.test_operator3n_ref import random_dvals
from tests.test_operator3v_ref import smooth_fields

pytestmark = pytest.mark.gpu

ZERO3 = (0.0, 0.0, 0.0)
# everything at once: ALL_OP's mixed axes 1 and 3, fields on every axis and rho, a reaction, faces
# 0b011011 / dfaces 0b110110, drift on all three axes, and axis 1 convective as well as the inner
# axis of (1,2) and (1,3): the stage-3 dual slot and both cross slots into T_1 are full, and Z_1 is
# the cross handle's own
CONV_1 = (1.0, 0.0, 0.0)
CROSS_1 = (0.8, -0.6, 0.0)


def drift_for(ns, axes, seed=9):
    """Smooth drift fields of both signs on `axes` (another seed than any a_k of the same case)."""
    f = smooth_fields(ns, tuple(axes), seed=seed)["a"]
    return tuple(f[k] if k in axes else None for k in range(3))


def _make(prob, Q, fs, op, coef, dfaces, dvals, conv, cross, drift, refine=False):
    from gpk.equations import Operator3V
    from gpk.model_GP_solver_3d import DeviceSolver3
    return DeviceSolver3("poisson", prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                         Q=Q, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"], lr=0.01,
                         freq_scale=fs, refine=refine,
                         operator=Operator3V(op["c2"], op["c1"], op["react"], op["faces"], a=coef["a"], rho=coef["rho"]),
                         dfaces=dfaces, dvals=dvals, conv=conv, cross=cross, drift=drift)


def n_launches(conv, cross, drift):
    """include/gpk.h: six stages, two with a convective axis, eight with a pair, and with a drift
    field two, plus one when a drift axis's Z_k is not a pair's own (Z_1: (1,2), (1,3); Z_2: (2,3))."""
    conv, cross = conv or ZERO3, cross or ZERO3
    shared = (cross[0] != 0.0 or cross[1] != 0.0, cross[2] != 0.0, False)
    own = any(b is not None and not sh for b, sh in zip(drift, shared))
    return 6 + (2 if any(conv) else 0) + (8 if any(cross) else 0) + 2 + (1 if own else 0)


def _check(label, loss, g, prob, params, op, coef, dfaces, dvals, conv, cross, drift):
    lo, go = loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift)
    tol = _tol(prob, params)
    gd = O.unflatten_params(params, g)
    errs = {k: rel(O.flatten_params(gd[k]), O.flatten_params(go[k])) for k in go}
    errs["loss"] = abs(loss - lo) / abs(lo)
    print(label, "tol %.3e" % tol, {k: "%.3e" % v for k, v in errs.items()})
    assert np.isfinite(loss) and np.all(np.isfinite(g))
    # the term matters: the yardstick without it gives another loss, and the case can tell the two
    # apart -- some checked quantity moves by at least 100 tol when the drift is left out (the loss
    # itself need not: under the SE kinds the prior's quadratic term is ~1e13 and hides the residual)
    lo0, go0 = loss_grad_3d_opm(prob, params, op, coef, dfaces, dvals, conv, cross)
    moved = {k: rel(O.flatten_params(go0[k]), O.flatten_params(go[k])) for k in go}
    moved["loss"] = abs(lo0 - lo) / abs(lo)
    assert lo0 != lo and max(moved.values()) > 100 * tol, (lo0, lo, moved, tol)
    for k, v in errs.items():
        assert v < tol, (label, k, v, tol)


def _setup(ns, op, dfaces, kind="Matern52_Cos_1d", Q=4, seed=3, unit=False):
    prob, params, fs = _problem(ns, kind, Q, seed, unit)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    return prob, params, fs, (random_dvals(ns, dfaces, seed=dfaces) if dfaces else None)


def _run(ns, op, coef, dfaces, conv, cross, drift, kind="Matern52_Cos_1d", Q=4, label="", refine=False, unit=False):
    prob, params, fs, dvals = _setup(ns, op, dfaces, kind, Q, unit=unit)
    s = _make(prob, Q, fs, op, coef, dfaces, dvals, conv, cross, drift, refine=refine)
    try:
        s.set_params(params)
        assert s.drift_info() == tuple(b is not None for b in drift)
        assert s.cross_info() == tuple(cross) and s.conv_info() == tuple(conv)
        assert s.bdata_info() == (op["faces"], dfaces)
        assert s.operator_info_x().as_dict() == {k: tuple(float(x) for x in v) if k != "faces" else v
                                                 for k, v in op.items()}
        assert len(s.stage_variants()) == n_launches(conv, cross, drift)
        loss, g = s.loss_grad()
        info = s.refine_info() if refine else None
    finally:
        s.close()
    axes = tuple(k + 1 for k, b in enumerate(drift) if b is not None)
    _check("%s %s %s Q%d drift %s cross %s conv %s" % (label, ns, kind, Q, axes, cross, conv), loss, g, prob, params,
           op, coef, dfaces, dvals, conv, cross, drift)
    return info


# ---- 1. one drift axis at a time, a 32-tile crossed on each axis in turn --------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("ns", [(33, 20, 9), (20, 33, 9), (9, 20, 33)])
def test_one_drift_axis_tile_crossing_on_each_axis(ns, axis):
    """Axis 2: the permuted E_2 / Z_2 path; axis 3: D1 on the right."""
    _run(ns, FULL, NO_COEF, 0, ZERO3, ZERO3, drift_for(ns, (axis,)), label="axis %d" % (axis + 1))


# ---- 2. everything at once -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_everything_at_once_every_kind(kind):
    ns = (33, 33, 9)
    _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=5), ALL_DFACES, CONV_1, CROSS_1, drift_for(ns, (0, 1, 2)),
         kind, label="all")


def test_everything_at_once_q64():
    ns = (33, 33, 9)
    _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=5), ALL_DFACES, CONV_1, CROSS_1, drift_for(ns, (0, 1, 2)),
         Q=64, label="all")


def test_all_pairs_share_both_z():
    """All three pairs: Z_1 and Z_2p are both the cross handle's, only Z_3 is formed for the drift."""
    ns = (20, 33, 9)
    _run(ns, FULL, NO_COEF, 0, ZERO3, (0.8, -0.6, 1.1), drift_for(ns, (0, 1, 2)), label="shared Z")


# ---- 3. n = 2 on a drift axis --------------------------------------------------------------------
@pytest.mark.parametrize("axis,ns", [(0, (2, 14, 9)), (1, (9, 2, 14)), (2, (9, 14, 2))])
def test_two_points_on_a_drift_axis(axis, ns):
    _run(ns, FULL, NO_COEF, 0, ZERO3, ZERO3, drift_for(ns, (axis,)), label="n = 2")


# ---- 4. a drift axis with no other term ----------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_drift_axis_without_terms_of_its_own(axis):
    """c2 = c1 = g = 0 on the drift axis (its D block is all zeros, its D1 block carries the drift
    alone); the other two axes are mixed."""
    c2, c1 = [-0.3, 0.7, -0.2], [0.8, -0.4, 1.3]
    c2[axis] = c1[axis] = 0.0
    op = dict(c2=tuple(c2), c1=tuple(c1), react=(0.4, 0.0, 0.2), faces=0b011111)
    ns = (20, 33, 9)
    _run(ns, op, NO_COEF, 0, ZERO3, ZERO3, drift_for(ns, (axis,)), label="bare axis %d" % (axis + 1))


# ---- 5. a field holding zeros and both signs -----------------------------------------------------
def test_drift_field_with_zeros_and_both_signs():
    ns = (20, 33, 9)
    drift = [b.copy() for b in drift_for(ns, (0, 1, 2))]
    for k, b in enumerate(drift):
        b[np.abs(b) < 0.3] = 0.0
        b[k::3] = 0.0
        assert (b == 0.0).sum() > b.size // 3 and b.min() < 0.0 < b.max()
    _run(ns, FULL, smooth_fields(ns, (1,), seed=2), 0, ZERO3, ZERO3, tuple(drift), label="zeros")


# ---- 6. refinement -------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [True, "gemm"])
def test_refined_both_routes(refine):
    """x in [0, 1] at (33, 20, 9): the gates open; Z_k reads the refined A_k and T_k carries the drift
    term before the refinement of X_k reads it."""
    from gpk import _lib
    ns = (33, 20, 9)
    info = _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=7), ALL_DFACES, CONV_1, CROSS_1,
                drift_for(ns, (0, 1, 2)), label="refined %r" % refine, refine=refine, unit=True)
    assert info["route"] == (_lib.REFINE_FUSED if refine is True else _lib.REFINE_GEMM)
    assert any(info["open"]), info


# ---- 7. loss terms, boundary terms, the criterion and the launch count ---------------------------
def test_loss_terms_boundary_terms_criterion_and_stage_variants():
    ns = (20, 14, 9)
    prob, params, fs, dvals = _setup(ns, ALL_OP, ALL_DFACES)
    coef = smooth_fields(ns, (0, 1, 2, 3), seed=6)
    drift = drift_for(ns, (0, 1, 2))
    one = (drift[0], None, None)
    s = _make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, CROSS_1, drift)
    shared = _make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, None, CROSS_1, one)
    plain = _make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, None, None, one)
    try:
        s.set_params(params)
        loss, _ = s.loss_grad()
        terms, bt, crit = s.loss_terms(), s.boundary_terms(), s.criterion()
        sv, svs, svp = s.stage_variants(), shared.stage_variants(), plain.stage_variants()
        assert s.drift_info() == (True, True, True) and shared.drift_info() == plain.drift_info() == (True, False, False)
    finally:
        s.close()
        shared.close()
        plain.close()
    # six stages, the convective handle's two, the cross handle's eight; the drift handle's two, and
    # its Z launch unless every drift axis's Z_k is a pair's own
    assert len(sv) == 6 + 2 + 8 + 3 and len(svs) == 6 + 8 + 2 and len(svp) == 6 + 3
    assert all(v in (1, 2, 3) for v in sv + svs + svp)
    t = {}
    loss_grad_3d_opb(prob, params, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, CROSS_1, drift, terms=t)
    tol = _tol(prob, params)
    cref = criterion_3d_opb(prob, params, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, CROSS_1, drift)
    print("terms", terms, "boundary", bt, "criterion", crit, cref, "tol", tol)
    assert terms["loss"] == loss
    assert bt["Nb"] == t["Nb"] and bt["Nd"] == t["Nd"]
    assert abs(bt["bgap"] - t["bgap"]) < tol * t["bgap"] and abs(bt["dgap"] - t["dgap"]) < tol * t["dgap"]
    assert terms["bgap"] == bt["bgap"] + bt["dgap"]
    expect = dict(t, bgap=t["bgap"] + t["dgap"])
    for k in terms:  # (a log det is a sum of O(1) log pivots: its error is measured against at least 1)
        assert abs(terms[k] - expect[k]) < tol * max(abs(expect[k]), 1.0), k
    assert abs(crit - cref) < tol * cref
    # the term is in egap: the handle without it has another one
    t0 = {}
    loss_grad_3d_opm(prob, params, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, CROSS_1, terms=t0)
    assert abs(t0["egap"] - terms["egap"]) > 1e-6 * terms["egap"]


# ---- 8. bits -------------------------------------------------------------------------------------
def _raw_opb(prob, Q, fs, op, coef, dfaces, dvals, conv, cross, dr):
    """A DeviceSolver3 whose handle comes from gpk_create3_opb called directly with `dr` (None: a
    NULL pointer; else a _lib.gpk_drift3)."""
    from gpk import _lib
    from gpk._lib import dptr
    s = _make(prob, Q, fs, op, coef, dfaces, dvals, conv, cross, None)
    lib = _lib.load()
    _lib.check(lib.gpk_destroy3(s._h))
    s._h = None
    c, h, cf, bd = _lib.gpk_operator3x(), ctypes.c_void_p(), _lib.gpk_coef3(), _lib.gpk_bdata3()
    cv, mx = _lib.gpk_conv3(), _lib.gpk_cross3()
    c.c2[:], c.c1[:], c.react[:], c.faces = op["c2"], op["c1"], op["react"], op["faces"]
    for k, f in enumerate(getattr(s, "_coef", [None] * 4)[:3]):
        if f is not None:
            cf.a[k] = dptr(f)
    if getattr(s, "_coef", [None] * 4)[3] is not None:
        cf.rho = dptr(s._coef[3])
    if dfaces:
        bd.dfaces, bd.dvals = dfaces, dptr(s._dvals)
    cv.g[:] = conv
    mx.m[:] = cross
    _lib.check(lib.gpk_create3_opb(ctypes.byref(s._prob), ctypes.byref(c), ctypes.byref(cf), ctypes.byref(bd),
                                   ctypes.byref(cv), ctypes.byref(mx), None if dr is None else ctypes.byref(dr),
                                   float(fs), ctypes.byref(h)))
    s._h = h
    return s


@pytest.mark.parametrize("dfaces,fields,conv,cross", [(0, (), ZERO3, ZERO3),
                                                      (ALL_DFACES, (0, 1, 2, 3), (1.0, -0.7, 0.5), (0.8, -0.6, 1.1))])
def test_no_drift_field_is_the_create3_opm_handle_bitwise(dfaces, fields, conv, cross):
    from gpk import _lib
    ns = (33, 20, 9)
    op = ALL_OP if dfaces else FULL
    prob, params, fs, dvals = _setup(ns, op, dfaces)
    coef = smooth_fields(ns, fields, seed=4)
    hs = [_make(prob, 4, fs, op, coef, dfaces, dvals, conv, cross, None),
          _raw_opb(prob, 4, fs, op, coef, dfaces, dvals, conv, cross, None),
          _raw_opb(prob, 4, fs, op, coef, dfaces, dvals, conv, cross, _lib.gpk_drift3()),
          _make(prob, 4, fs, op, coef, dfaces, dvals, conv, cross, (None, None, None))]
    try:
        for s in hs:
            s.set_params(params)
            assert s.drift_info() == (False, False, False)
            assert s.cross_info() == cross and s.conv_info() == conv
            assert s.bdata_info() == (op["faces"], dfaces)
        ref = hs[0].loss_grad()
        assert len(hs[0].stage_variants()) == 6 + (2 if any(conv) else 0) + (8 if any(cross) else 0)
        for s in hs[1:]:
            l, g = s.loss_grad()
            assert l == ref[0] and np.array_equal(g, ref[1])
            assert s.stage_variants() == hs[0].stage_variants()
            assert s.loss_terms() == hs[0].loss_terms()
            assert s.boundary_terms() == hs[0].boundary_terms()
        steps = [s.step(3) for s in hs]
        for x in steps[1:]:
            assert np.array_equal(x, steps[0])
        flats = [s.get_flat() for s in hs]
        for x in flats[1:]:
            assert np.array_equal(x, flats[0])
    finally:
        for s in hs:
            s.close()


def test_repeated_calls_equal_bits_and_step_is_loss_grad_plus_apply():
    ns = (33, 20, 9)
    prob, params, fs, dvals = _setup(ns, ALL_OP, ALL_DFACES)
    coef = smooth_fields(ns, (0, 1, 2, 3), seed=4)
    drift = drift_for(ns, (0, 1, 2))
    a, b = (_make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, CROSS_1, drift) for _ in range(2))
    try:
        for s in (a, b):
            s.set_params(params)
        (l1, g1), (l2, g2) = a.loss_grad(), a.loss_grad()
        assert l1 == l2 and np.array_equal(g1, g2)
        assert a.loss_terms() == a.loss_terms()
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


def test_predictions_are_a_legacy_handles_bitwise():
    """Predictions, predict_deriv and evaluate depend on K_k and U only."""
    from gpk.model_GP_solver_3d import DeviceSolver3
    ns = (20, 14, 9)
    prob, params, fs, _ = _setup(ns, dict(FULL, faces=63), 0)
    s = _make(prob, 4, fs, dict(FULL, faces=63), NO_COEF, 0, None, ZERO3, ZERO3, drift_for(ns, (0, 1, 2)))
    legacy = DeviceSolver3("poisson", prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                           Q=4, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"], lr=0.01,
                           freq_scale=fs)
    xte = [np.linspace(x[0], x[-1], m) for x, m in zip((prob["x1"], prob["x2"], prob["x3"]), (7, 6, 5))]
    pts = np.random.default_rng(1).uniform(0.0, 1.0, size=(11, 3)) * [x[-1] for x in xte]
    try:
        for h in (s, legacy):
            h.set_params(params)
        assert np.array_equal(s.predict(*xte), legacy.predict(*xte))
        assert np.array_equal(s.predict_deriv(*xte, deriv=(1, 0, 2)), legacy.predict_deriv(*xte, deriv=(1, 0, 2)))
        assert np.array_equal(s.evaluate(pts, (0, 1, 0)), legacy.evaluate(pts, (0, 1, 0)))
    finally:
        s.close()
        legacy.close()


# ---- 9. Adam trajectory --------------------------------------------------------------------------
def test_adam_trajectory_vs_replay():
    """Five steps under the bars of tests/test_gpu_kron3_opn.py's trajectory."""
    ns = (20, 14, 9)
    prob, params, fs, dvals = _setup(ns, ALL_OP, ALL_DFACES, Q=5, seed=8)
    coef = smooth_fields(ns, (0, 3), seed=8)
    drift = drift_for(ns, (0, 1, 2))
    s = _make(prob, 5, fs, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, CROSS_1, drift)
    try:
        s.set_params(params)
        losses = s.step(5)
        flat = s.get_flat()
    finally:
        s.close()
    ref, p = adam_replay_b(prob, params, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, CROSS_1, drift, 5)
    tol = _tol(prob, params)
    print("adam opb", rel(losses, ref), rel(flat, O.flatten_params(p)), "tol", tol)
    assert rel(losses, ref) < max(1e-9, tol)
    assert rel(flat, O.flatten_params(p)) < max(1e-8, 10 * tol)


# ---- 10. heat in divergence form through the model class -----------------------------------------
def _heat_div_model(ncol=8, mtest=9):
    from gpk.equations import drift_fields, solution_3d_opb
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single, boundary_3d, get_mesh_data, load_config
    cfg = load_config("heat_div_t-sin")
    u, src, op, dfaces, _, conv, cross, drift = solution_3d_opb("heat_div_t-sin")
    xte, ute = get_mesh_data(u, (mtest,) * 3, 1.0)
    xc, umh = get_mesh_data(u, (ncol,) * 3, 1.0)
    _, srcv = get_mesh_data(src, (ncol,) * 3, 1.0)
    bvals = boundary_3d(umh, op.faces)
    tp = {"kernel": kernel_class("Matern52_Cos_1d"), "equation": "heat_div_t-sin", "llk_weight": cfg["llk_weight"],
          "logdet": cfg["logdet"], "lr": cfg["lr"], "Q": cfg["Q"], "freq_scale": cfg["freq_scale"], "nepoch": 20,
          "tol": -1}
    prob = dict(kind="Matern52_Cos_1d", x1=xc[0], x2=xc[1], x3=xc[2], src=srcv, bvals=bvals, jitter=1e-6,
                llk_weight=float(cfg["llk_weight"]), logdet=float(cfg["logdet"]))
    a = op.fields(xc)
    coef = dict(a=tuple(a[:3]), rho=a[3])

    def make():
        return GP_solver_3d_single(bvals, xc, srcv, 1e-6, tp, X_test=xte, u_test=ute)
    return prob, op, coef, tuple(drift_fields(drift, xc)), tp, xte, ute, make


def test_train_heat_div_vs_replay_and_resume(tmp_path):
    from tests.test_gpu_kron3_predict import ref_predict
    prob, op, coef, drift, tp, xte, ute, make = _heat_div_model()
    assert np.isnan(prob["bvals"]).sum() == 64  # the final-time face is open
    assert drift[2] is None and drift[0].shape == drift[1].shape == (8, 8, 8)
    m = make()
    try:
        assert m.Nb == 5 * 64 and m.dev.operator_info_x() == op.constant
        assert m.dev.drift_info() == (True, True, False) and m.dev.coef_info() == (True, True, False, False)
        assert m.dev.cross_info() == ZERO3 and m.dev.conv_info() == ZERO3
        assert m.dev.bdata_info() == (0b011111, 0)
        log, stop, min_err = m.train(20, verbose=False)
        flat = m.dev.get_flat()
    finally:
        m.dev.close()
    p0 = O.init_params_3d(8, 8, 8, tp["Q"], tp["freq_scale"])
    errs = []

    def after(i, p):
        pr = ref_predict(prob, p, xte)
        errs.append(np.linalg.norm(pr.ravel() - ute.ravel()) / np.linalg.norm(ute.ravel()))
    losses, _ = adam_replay_b(prob, p0, op.constant.as_dict(), coef, 0, None, None, None, drift, 20, lr=tp["lr"],
                              after=after)
    losses = [np.log(lo) if lo > 1 else lo for lo in losses]
    tol = max(1e-8, 10 * _tol(prob, p0))
    print("train heat_div_t loss rel", rel(log["loss_list"], losses), "err rel", rel(log["err_list"], errs), "tol", tol)
    assert log["epoch_list"] == list(range(20))
    assert rel(log["loss_list"], losses) < tol
    assert rel(log["err_list"], errs) < tol
    assert min_err == min(log["err_list"]) and not stop["flag"]
    ck = str(tmp_path / "ck.npz")
    m1 = make()
    try:
        log1, _, _ = m1.train(20, verbose=False, checkpoint=ck, stop_at=10)
        assert log1["epoch_list"] == list(range(10))
    finally:
        m1.dev.close()
    m2 = make()
    try:
        log2, _, min2 = m2.train(20, verbose=False, resume=ck)
        assert m2.dev.drift_info() == (True, True, False)  # the drift comes back from the equation's name
        assert np.array_equal(m2.dev.get_flat(), flat)
    finally:
        m2.dev.close()
    assert min2 == min_err and sorted(log2) == sorted(log)
    for k in log:
        assert np.array_equal(np.asarray(log2[k]), np.asarray(log[k])), k


@pytest.mark.parametrize("equation", ["darcy_3d-sin", "heat_div_t-sin", "convdiff_rot_t-sin"])
def test_eq_residual_opb(equation):
    """eq_residual on a 7 x 6 x 5 test grid against NumPy on the reference predictions, at the bar
    of tests/test_gpu_eq_residual.py (the project's bar scaled by the largest term; a drift term is
    one first-derivative prediction times its field on the test mesh)."""
    from gpk.equations import Operator3V, drift_fields, solution_3d_opb
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single
    from tests import predict_deriv_ref as R
    _, _, op, _, _, conv, cross, drift = solution_3d_opb(equation)
    ns, ms = (20, 14, 9), (7, 6, 5)
    prob, params, fs = _problem(ns)
    tp = {"kernel": kernel_class(prob["kind"]), "llk_weight": prob["llk_weight"], "Q": 4, "lr": 0.01,
          "freq_scale": fs, "logdet": True, "equation": equation}
    m = GP_solver_3d_single(_mask_bvals(prob["bvals"], ns, op.faces), (prob["x1"], prob["x2"], prob["x3"]),
                            prob["src"], prob["jitter"], tp)
    xte = R.grid_axes(prob, params, ms)
    src = np.random.default_rng(2).normal(size=ms)
    try:
        assert m.dev.drift_info() == tuple(b is not None for b in drift)
        assert m.dev.cross_info() == cross == ZERO3 and m.dev.conv_info() == conv == ZERO3
        res = m.eq_residual(params, tuple(xte), src)
    finally:
        m.dev.close()
    a = op.fields(xte)[:3] if isinstance(op, Operator3V) else [None] * 3
    terms = []
    for k in range(3):
        for o, w in ((2, op.c2[k]), (1, op.c1[k])):
            if w != 0.0:
                d = [0, 0, 0]
                d[k] = o
                t = w * R.ref_grid(prob, params, xte, d)
                terms.append(t if a[k] is None else a[k] * t)
    nlin = len(terms)
    for k, b in enumerate(drift_fields(drift, xte)):
        if b is not None:
            d = [0, 0, 0]
            d[k] = 1
            terms.append(b * R.ref_grid(prob, params, xte, d))
    assert len(terms) - nlin == {"darcy_3d-sin": 3, "heat_div_t-sin": 2, "convdiff_rot_t-sin": 2}[equation]
    expect = sum(terms) - src
    tol = R.bar(prob, params)
    scale = max([float(np.max(np.abs(t))) for t in terms] + [float(np.max(np.abs(src)))])
    err = float(np.max(np.abs(res - expect)))
    print("eq_residual", equation, "err / scale", err / scale, "tol", tol)
    assert res.shape == ms
    assert err < tol * scale
