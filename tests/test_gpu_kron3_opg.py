"""Quadratic gradient terms on the 3-axis solver (gpk_create3_opg; DeviceSolver3 with gradsq=): the handle
adds sum_k s_k (du/dx_k)^2 + sum_{j<k} x_jk du/dx_j du/dx_k.  P_k = D1_k x_k A_k per gradient-active axis
stands in the convective V_k launch's place, k3_combine_g forms N, Gamma, R and the reverse operands
Q_k, the stage-3 dual slot adds D1_k^T x_k Q_k to T_k and G_D1k = v Q_k A_k^T stands in the convective
G_D1k launch's place.

Yardstick: tests/operator3g_ref.py loss_grad_3d_opg (pinned on the CPU by tests/test_operator3g_ref.py
against torch autograd of the dense-Kronecker form).  Tolerance: the project's _tol of
tests/test_gpu_kron3.py, max(1e-10, 50 cond eps) with the largest cond K_k, on the loss and on every
gradient block.  Every bvals / dvals entry that must not be read is NaN.  Each case asserts that the
yardstick without gradsq moves some checked quantity by over 100 tolerances; the weights are of order
0.1 to 1.  Handles without a weight are compared with gpk_create3_opq's bit for bit, predictions with a
legacy handle's.
"""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import rel
from tests.operator3g_ref import adam_replay_g, criterion_3d_opg, loss_grad_3d_opg
from tests.operator3m_ref import PAIRS
from tests.operator3q_ref import loss_grad_3d_opq
from tests.test_gpu_kron3 import KINDS, _tol
from tests.test_gpu_kron3_operator import _mask_bvals, _problem
from tests.test_gpu_kron3_opb import drift_for
from tests.test_gpu_kron3_opv import NO_COEF
from tests.test_operator3n_ref import random_dvals
from tests.test_operator3v_ref import smooth_fields

pytestmark = pytest.mark.gpu

ZERO3 = (0.0, 0.0, 0.0)
NONE3 = (None, None, None)
NO_HIGH = (ZERO3, ZERO3)
PLAIN = dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, 0.0, 1.0), react=ZERO3, faces=63)
S1, X1 = 0.6, -0.7
# everything at once on (33, 33, 9): axes 1-2 share their launch
ALL_OP = dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, -0.6, 1.3), react=(0.4, -0.5, 0.2), faces=0b011011)
ALL_HIGH = ((2e-3, -1e-3, 1.5e-3), (-3e-2, 2e-2, 4e-2))
ALL_BQ = (1.5e-3, 0.0, 0.0)
ALL_GQ = ((0.5, -0.3, 0.4), (0.25, -0.35, 0.3))
ALL_DFACES = 0b110110
ALL_KW = dict(conv=(1.0, 0.0, -0.5), cross=(0.8, 0.0, 0.0))
# the Hamilton-Jacobi form: u_t + (u_x^2 + u_y^2) / 2 - nu (u_xx + u_yy)
HJ = (dict(c2=(-0.05, -0.05, 0.0), c1=(0.0, 0.0, 1.0), react=ZERO3, faces=0b011111), ((0.5, 0.5, 0.0), ZERO3))


def _make(prob, Q, fs, op, coef=NO_COEF, dfaces=0, dvals=None, conv=None, cross=None, drift=None, high=None,
          bicross=None, gradsq=None, refine=False):
    from gpk.equations import Operator3V
    from gpk.model_GP_solver_3d import DeviceSolver3
    return DeviceSolver3("poisson", prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                         Q=Q, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"], lr=0.01,
                         freq_scale=fs, refine=refine,
                         operator=Operator3V(op["c2"], op["c1"], op["react"], op["faces"], a=coef["a"], rho=coef["rho"]),
                         dfaces=dfaces, dvals=dvals, conv=conv, cross=cross, drift=drift, high=high, bicross=bicross,
                         gradsq=gradsq)


def _check(label, loss, g, prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, bq, gq):
    lo, go = loss_grad_3d_opg(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, bq, gq)
    tol = _tol(prob, params)
    gd = O.unflatten_params(params, g)
    errs = {k: rel(O.flatten_params(gd[k]), O.flatten_params(go[k])) for k in go}
    errs["loss"] = abs(loss - lo) / abs(lo)
    print(label, "tol %.3e" % tol, {k: "%.3e" % v for k, v in errs.items()})
    assert np.isfinite(loss) and np.all(np.isfinite(g))
    # the term matters: the yardstick without it moves some checked quantity by over 100 tol
    lo0, go0 = loss_grad_3d_opq(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, bq)
    moved = {k: rel(O.flatten_params(go0[k]), O.flatten_params(go[k])) for k in go}
    moved["loss"] = abs(lo0 - lo) / abs(lo)
    assert lo0 != lo and max(moved.values()) > 100 * tol, (lo0, lo, moved, tol)
    for k, v in errs.items():
        assert v < tol, (label, k, v, tol)


def _setup(ns, op, dfaces=0, kind="Matern52_Cos_1d", Q=4, seed=3, unit=False):
    prob, params, fs = _problem(ns, kind, Q, seed, unit)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    return prob, params, fs, (random_dvals(ns, dfaces, seed=dfaces) if dfaces else None)


def _run(ns, op, gq, high=None, bq=None, coef=NO_COEF, dfaces=0, conv=None, cross=None, drift=None,
         kind="Matern52_Cos_1d", Q=4, label="", refine=False, unit=False):
    prob, params, fs, dvals = _setup(ns, op, dfaces, kind, Q, unit=unit)
    s = _make(prob, Q, fs, op, coef, dfaces, dvals, conv, cross, drift, high, bq, gq, refine)
    try:
        s.set_params(params)
        assert np.array_equal(s.get_flat(), O.flatten_params(params))
        assert s.gradsq_info() == (tuple(gq[0]), tuple(gq[1]))
        assert s.conv_info() == tuple(conv or ZERO3) and s.bicross_info() == tuple(bq or ZERO3)
        loss, g = s.loss_grad()
        info = s.refine_info() if refine else None
    finally:
        s.close()
    _check("%s %s %s Q%d gq %s" % (label, ns, kind, Q, gq), loss, g, prob, params, op, coef, dfaces, dvals,
           conv, cross, drift or NONE3, high, bq, gq)
    return info


def _s(k, w=S1):
    return tuple(w if a == k else 0.0 for a in range(3)), ZERO3


def _x(t, w=X1):
    return ZERO3, tuple(w if a == t else 0.0 for a in range(3))


# ---- 1. each weight alone, the 32-tile crossed on each axis ---------------------------------------
@pytest.mark.parametrize("ns", [(33, 20, 9), (20, 33, 9), (9, 20, 33)])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_one_square_tile_crossing_on_each_axis(ns, k):
    """s_k alone: P_k and Q_k natural on axes 1 and 3, permuted on axis 2."""
    _run(ns, PLAIN, _s(k), label="s_%d" % (k + 1))


@pytest.mark.parametrize("t", [0, 1, 2])
def test_one_product_alone(t):
    _run((33, 20, 9), PLAIN, _x(t), label="x_%d%d" % (PAIRS[t][0] + 1, PAIRS[t][1] + 1))


# ---- 2. everything at once ------------------------------------------------------------------------
def _everything(kind, Q):
    ns = (33, 33, 9)
    _run(ns, ALL_OP, ALL_GQ, ALL_HIGH, ALL_BQ, coef=smooth_fields(ns, (0, 1, 3), seed=5), dfaces=ALL_DFACES,
         drift=drift_for(ns, (0, 2)), kind=kind, Q=Q, label="everything", **ALL_KW)


@pytest.mark.parametrize("kind", KINDS)
def test_everything_at_once_every_kind(kind):
    """All six weights over all four orders on every axis, fields a_1, a_2 and rho, a reaction, two
    convective axes, a cross pair and a bi-pair on axes 1-2, drift fields, faces 0b011011 and derivative
    faces 0b110110."""
    _everything(kind, 4)


def test_everything_at_once_q64():
    _everything("Matern52_Cos_1d", 64)


# ---- 3. n = 2 on a gradient-active axis, and axes with nothing else -------------------------------
@pytest.mark.parametrize("ns", [(2, 14, 9), (9, 2, 14), (9, 14, 2)])
def test_two_points_on_a_gradient_active_axis(ns):
    _run(ns, PLAIN, ((0.6, -0.5, 0.4), (0.3, -0.4, 0.5)), label="n = 2")


@pytest.mark.parametrize("k", [0, 1, 2])
def test_pure_gradient_axis_next_to_a_mixed_one(k):
    """Axis k has c4 = c3 = c2 = c1 = g = 0 and s_k != 0 (the inviscid eikonal's axis: D_k all zeros, GEMM
    weight 1.0, the split mode); the next axis is mixed (c2 and c1) and gradient-active through x."""
    n = (k + 1) % 3
    c2 = tuple(0.0 if a == k else -0.4 for a in range(3))
    c1 = tuple(0.7 if a == n else 0.0 for a in range(3))
    t = [i for i, p in enumerate(PAIRS) if set(p) == {k, n}][0]
    gq = (_s(k)[0], _x(t, 0.5)[1])
    _run((20, 14, 9), dict(c2=c2, c1=c1, react=ZERO3, faces=63), gq, label="pure axis %d" % (k + 1))


# ---- 4. sharing with the older terms --------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_square_and_convective_weight_on_the_same_axis(k):
    """s_k with g_k: one P_k serves N and Gamma, and Q_k = (g_k U + 2 s_k P_k) R."""
    conv = tuple(0.9 if a == k else 0.0 for a in range(3))
    _run((33, 20, 9), PLAIN, _s(k), conv=conv, label="s and g on axis %d" % (k + 1))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_gradient_active_drift_and_cross_axis(k):
    """Axis k is gradient-active, a drift axis and an axis of a cross pair: G_D1k is written by the
    gradient launch, added to by the cross launch and by the drift launch, in that order."""
    ns = (33, 20, 9)
    t = 0 if k < 2 else 1
    cross = tuple(0.8 if a == t else 0.0 for a in range(3))
    _run(ns, PLAIN, (_s(k)[0], _x(2 - t, 0.5)[1]), cross=cross, drift=drift_for(ns, (k,)),
         label="active + drift + cross on axis %d" % (k + 1))


def test_modes_in_separate_launches_with_high_and_bicross():
    """Axis 1 gradient-active over c4 (D + D1), axis 2 in a bi-pair without D1, axis 3 gradient-active in a
    bi-pair (D + D1 + DD)."""
    _run((33, 20, 9), PLAIN, ((0.6, 0.0, -0.5), (0.0, 0.4, 0.0)), high=((2e-3, 0.0, 0.0), ZERO3),
         bq=(0.0, 0.0, 1.5e-3), label="modes apart")


# ---- 5. refinement --------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [True, "gemm"])
def test_refined_both_routes(refine):
    """x in [0, 1] at (33, 20, 9): the gates open; the fused route and the two-GEMM route.  No solve is
    added: both routes see a T_k that already carries D1_k^T x_k Q_k."""
    from gpk import _lib
    info = _run((33, 20, 9), dict(PLAIN, c2=(-0.05, 0.05, -0.02)), ((0.5, -0.3, 0.4), (0.25, -0.35, 0.3)),
                conv=(1.0, 0.0, 0.0), label="refined %r" % refine, refine=refine, unit=True)
    assert info["route"] == (_lib.REFINE_FUSED if refine is True else _lib.REFINE_GEMM)
    assert any(info["open"]), info


# ---- 6. loss terms, boundary terms, criterion, stage variants -------------------------------------
def test_loss_terms_boundary_terms_criterion_and_stage_variants():
    ns = (20, 14, 9)
    dfaces = 0b000011
    op = dict(ALL_OP, faces=0b011100)
    conv = (1.0, 0.0, 0.0)
    prob, params, fs, dvals = _setup(ns, op, dfaces)
    args = (op, NO_COEF, dfaces, dvals, conv, None, NONE3, ALL_HIGH, ALL_BQ)
    s = _make(prob, 4, fs, op, NO_COEF, dfaces, dvals, conv, high=ALL_HIGH, bicross=ALL_BQ, gradsq=ALL_GQ)
    base = _make(prob, 4, fs, op, NO_COEF, dfaces, dvals, conv, high=ALL_HIGH, bicross=ALL_BQ)
    # (no convective weight: the handle still reports the convective handle's entries)
    bare = _make(prob, 4, fs, op, NO_COEF, dfaces, dvals, None, high=ALL_HIGH, bicross=ALL_BQ, gradsq=_s(1))
    try:
        s.set_params(params)
        loss, _ = s.loss_grad()
        terms, bt, crit = s.loss_terms(), s.boundary_terms(), s.criterion()
        nb, ng, n0 = len(base.stage_variants()), len(s.stage_variants()), len(bare.stage_variants())
        assert base.gradsq_info() == NO_HIGH and bare.gradsq_info() == _s(1)
    finally:
        for h in (s, base, bare):
            h.close()
    assert ng == nb and n0 == nb, (nb, ng, n0)
    t = {}
    loss_grad_3d_opg(prob, params, *args, ALL_GQ, terms=t)
    tol = _tol(prob, params)
    cref = criterion_3d_opg(prob, params, *args, ALL_GQ)
    print("terms", terms, "boundary", bt, "criterion", crit, cref, "tol", tol)
    assert terms["loss"] == loss
    assert bt["Nb"] == t["Nb"] and bt["Nd"] == t["Nd"]
    assert abs(bt["bgap"] - t["bgap"]) < tol * t["bgap"] and abs(bt["dgap"] - t["dgap"]) < tol * t["dgap"]
    assert terms["bgap"] == bt["bgap"] + bt["dgap"]
    expect = dict(t, bgap=t["bgap"] + t["dgap"])
    for k in terms:  # (a log det is a sum of O(1) log pivots: its error is measured against at least 1)
        assert abs(terms[k] - expect[k]) < tol * max(abs(expect[k]), 1.0), k
    assert abs(crit - cref) < tol * cref
    t0 = {}
    loss_grad_3d_opq(prob, params, *args, terms=t0)
    assert abs(t0["egap"] - terms["egap"]) > 1e-6 * terms["egap"]  # Gamma is in egap


# ---- 7. bits --------------------------------------------------------------------------------------
def _raw(prob, Q, fs, op, conv, cross, high, bq, gq, opg=True):
    """A DeviceSolver3 whose handle comes from gpk_create3_opg called directly with `gq` (None: a NULL
    pointer; else a _lib.gpk_gradsq3), or from gpk_create3_opq (opg = False)."""
    from gpk import _lib
    s = _make(prob, Q, fs, op, conv=conv, cross=cross)
    lib = _lib.load()
    _lib.check(lib.gpk_destroy3(s._h))
    s._h = None
    c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
    cv, mx, hi, bi = _lib.gpk_conv3(), _lib.gpk_cross3(), _lib.gpk_high3(), _lib.gpk_bicross3()
    c.c2[:], c.c1[:], c.react[:], c.faces = op["c2"], op["c1"], op["react"], op["faces"]
    cv.g[:] = conv
    mx.m[:] = cross
    hi.c4[:], hi.c3[:] = high
    bi.q[:] = bq
    head = (ctypes.byref(s._prob), ctypes.byref(c), None, None, ctypes.byref(cv), ctypes.byref(mx), None,
            ctypes.byref(hi), ctypes.byref(bi))
    if opg:
        _lib.check(lib.gpk_create3_opg(*head, None if gq is None else ctypes.byref(gq), float(fs), ctypes.byref(h)))
    else:
        _lib.check(lib.gpk_create3_opq(*head, float(fs), ctypes.byref(h)))
    s._h = h
    return s


@pytest.mark.parametrize("conv,cross,high,bq", [(ZERO3, ZERO3, NO_HIGH, ZERO3),
                                                ((1.0, -0.7, 0.5), (0.8, -0.6, 1.1), ALL_HIGH, (1.5e-3, -1e-3, 2e-3))])
def test_no_gradsq_weight_is_the_create3_opq_handle_bitwise(conv, cross, high, bq):
    from gpk import _lib
    ns = (33, 20, 9)
    op = dict(ALL_OP, faces=0b011111)
    prob, params, fs, _ = _setup(ns, op)
    hs = [_raw(prob, 4, fs, op, conv, cross, high, bq, None, opg=False),
          _raw(prob, 4, fs, op, conv, cross, high, bq, None),
          _raw(prob, 4, fs, op, conv, cross, high, bq, _lib.gpk_gradsq3()),
          _make(prob, 4, fs, op, conv=conv, cross=cross, high=high, bicross=bq, gradsq=NO_HIGH),
          _make(prob, 4, fs, op, conv=conv, cross=cross, high=high, bicross=bq)]
    try:
        for s in hs:
            s.set_params(params)
            assert s.gradsq_info() == NO_HIGH
            assert s.cross_info() == cross and s.conv_info() == conv and s.high_info() == high
            assert s.bicross_info() == bq
        ref = hs[0].loss_grad()
        for s in hs[1:]:
            l, g = s.loss_grad()
            assert l == ref[0] and np.array_equal(g, ref[1])
            assert s.stage_variants() == hs[0].stage_variants()
            assert s.loss_terms() == hs[0].loss_terms()
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
    a, b = (_make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, high=ALL_HIGH, bicross=ALL_BQ, gradsq=ALL_GQ, **ALL_KW)
            for _ in range(2))
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
    from gpk.model_GP_solver_3d import DeviceSolver3
    ns = (20, 14, 9)
    op = dict(ALL_OP, faces=63)
    prob, params, fs, _ = _setup(ns, op)
    s = _make(prob, 4, fs, op, gradsq=ALL_GQ)
    legacy = DeviceSolver3("poisson", prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                           Q=4, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"], lr=0.01,
                           freq_scale=fs)
    xte = [np.linspace(x[0], x[-1], m) for x, m in zip((prob["x1"], prob["x2"], prob["x3"]), (7, 6, 5))]
    pts = np.random.default_rng(1).uniform(0.0, 1.0, size=(11, 3)) * [x[-1] for x in xte]
    try:
        for h in (s, legacy):
            h.set_params(params)
        assert np.array_equal(s.predict(*xte), legacy.predict(*xte))
        assert np.array_equal(s.predict_deriv(*xte, deriv=(1, 0, 1)), legacy.predict_deriv(*xte, deriv=(1, 0, 1)))
        assert np.array_equal(s.evaluate(pts, (0, 1, 0)), legacy.evaluate(pts, (0, 1, 0)))
    finally:
        s.close()
        legacy.close()


# ---- 8. Adam trajectory ---------------------------------------------------------------------------
def test_adam_trajectory_hamilton_jacobi_vs_replay():
    """Ten steps of the Hamilton-Jacobi form, under tests/test_gpu_kron3_opx.py's trajectory bars."""
    ns = (24, 18, 12)
    op, gq = HJ
    prob, params, fs, _ = _setup(ns, op, Q=5, seed=8)
    s = _make(prob, 5, fs, op, gradsq=gq)
    try:
        s.set_params(params)
        losses = s.step(10)
        flat = s.get_flat()
    finally:
        s.close()
    ref, p = adam_replay_g(prob, params, op, NO_COEF, 0, None, None, None, None, None, None, gq, 10)
    tol = _tol(prob, params)
    print("adam hj", rel(losses, ref), rel(flat, O.flatten_params(p)), "tol", tol)
    assert rel(losses, ref) < max(1e-9, tol)
    assert rel(flat, O.flatten_params(p)) < max(1e-8, 10 * tol)


# ---- 9. the five configs through the model class --------------------------------------------------
def _model(equation):
    from gpk.equations import solution_3d_opg
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single, boundary_3d, get_mesh_data, load_config
    cfg = load_config(equation)
    sol = solution_3d_opg(equation)
    u, src, op = sol[:3]
    xte, ute = get_mesh_data(u, (9,) * 3, 1.0)
    xc, umh = get_mesh_data(u, (8,) * 3, 1.0)
    _, srcv = get_mesh_data(src, (8,) * 3, 1.0)
    bvals = boundary_3d(umh, op.faces)
    tp = {"kernel": kernel_class("Matern52_Cos_1d"), "equation": equation, "llk_weight": cfg["llk_weight"],
          "logdet": cfg["logdet"], "lr": cfg["lr"], "Q": cfg["Q"], "freq_scale": cfg["freq_scale"], "nepoch": 20,
          "tol": -1}
    prob = dict(kind="Matern52_Cos_1d", x1=xc[0], x2=xc[1], x3=xc[2], src=srcv, bvals=bvals, jitter=1e-6,
                llk_weight=float(cfg["llk_weight"]), logdet=float(cfg["logdet"]))

    def make():
        return GP_solver_3d_single(bvals, xc, srcv, 1e-6, tp, X_test=xte, u_test=ute)
    return prob, sol, tp, xte, ute, make


EXPECT = {"eikonal_3d-sin": (63, 0), "hj_t-sin": (0b011111, 0), "kpz_t-sin": (0b011111, 0),
          "aniso_eikonal_3d-sin": (63, 0), "ks_int_t-sin": (0b011111, 0b001111)}


@pytest.mark.parametrize("equation", list(EXPECT))
def test_train_config_vs_replay(equation, tmp_path):
    """20 epochs at 8^3 with the config's own settings against the replay; hj_t-sin also through
    checkpoint / resume; eq_residual refuses ks_int_t-sin (its fourth-order terms)."""
    from tests.test_gpu_kron3_predict import ref_predict
    prob, sol, tp, xte, ute, make = _model(equation)
    _, _, op, dfaces, _, conv, cross, drift, high, bq, gq = sol
    faces, dexp = EXPECT[equation]
    assert op.faces == faces and dfaces == dexp
    assert np.isnan(prob["bvals"]).sum() == (64 if faces != 63 else 0)
    m = make()
    try:
        assert m.dev.gradsq_info() == (tuple(gq[0]), tuple(gq[1]))
        assert m.dev.bicross_info() == tuple(bq) and m.dev.high_info() == (tuple(high[0]), tuple(high[1]))
        assert m.dev.bdata_info() == (faces, dfaces)
        assert m.Nb == (bin(faces).count("1") + bin(dfaces).count("1")) * 64
        dvals = m.dvals
        log, stop, min_err = m.train(20, verbose=False)
        flat = m.dev.get_flat()
        if equation == "ks_int_t-sin":
            with pytest.raises(ValueError):
                m.eq_residual(m.params, tuple(xte), np.zeros((9, 9, 9)))
    finally:
        m.dev.close()
    p0 = O.init_params_3d(8, 8, 8, tp["Q"], tp["freq_scale"])
    errs = []

    def after(i, p):
        pr = ref_predict(prob, p, xte)
        errs.append(np.linalg.norm(pr.ravel() - ute.ravel()) / np.linalg.norm(ute.ravel()))
    losses, _ = adam_replay_g(prob, p0, op.as_dict(), NO_COEF, dfaces, dvals, conv, cross, drift, high, bq, gq, 20,
                              lr=tp["lr"], after=after)
    losses = [np.log(lo) if lo > 1 else lo for lo in losses]
    tol = max(1e-8, 10 * _tol(prob, p0))
    print("train", equation, "loss rel", rel(log["loss_list"], losses), "err rel", rel(log["err_list"], errs), "tol", tol)
    assert log["epoch_list"] == list(range(20))
    assert rel(log["loss_list"], losses) < tol
    assert rel(log["err_list"], errs) < tol
    assert min_err == min(log["err_list"]) and not stop["flag"]
    if equation != "hj_t-sin":
        return
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
        assert m2.dev.gradsq_info() == (tuple(gq[0]), tuple(gq[1]))  # gradsq comes back from the equation's name
        assert np.array_equal(m2.dev.get_flat(), flat)
    finally:
        m2.dev.close()
    assert min2 == min_err and sorted(log2) == sorted(log)
    for k in log:
        assert np.array_equal(np.asarray(log2[k]), np.asarray(log[k])), k


@pytest.mark.parametrize("equation", ["aniso_eikonal_3d-sin", "hj_t-sin"])
def test_eq_residual(equation):
    """eq_residual on a 7 x 6 x 5 test grid against NumPy on the reference predictions, at the bar of
    tests/test_gpu_kron3_opm.py's eq_residual test (the project's bar scaled by the largest term; a
    quadratic term is the product of two first-derivative predictions, each within the bar)."""
    from gpk.equations import solution_3d_opg
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single
    from tests import predict_deriv_ref as R
    sol = solution_3d_opg(equation)
    op, gq = sol[2], sol[10]
    ns, ms = (20, 14, 9), (7, 6, 5)
    prob, params, fs = _problem(ns)
    tp = {"kernel": kernel_class(prob["kind"]), "llk_weight": prob["llk_weight"], "Q": 4, "lr": 0.01,
          "freq_scale": fs, "logdet": True, "equation": equation}
    m = GP_solver_3d_single(_mask_bvals(prob["bvals"], ns, op.faces), (prob["x1"], prob["x2"], prob["x3"]),
                            prob["src"], prob["jitter"], tp)
    xte = R.grid_axes(prob, params, ms)
    src = np.random.default_rng(2).normal(size=ms)
    try:
        assert m.dev.operator_info_x() == op and m.dev.gradsq_info() == (tuple(gq[0]), tuple(gq[1]))
        res = m.eq_residual(params, tuple(xte), src)
    finally:
        m.dev.close()
    terms = []
    for k in range(3):
        for o, w in ((2, op.c2[k]), (1, op.c1[k])):
            if w != 0.0:
                d = [0, 0, 0]
                d[k] = o
                terms.append(w * R.ref_grid(prob, params, xte, d))
    du = [R.ref_grid(prob, params, xte, [int(a == k) for a in range(3)]) for k in range(3)]
    terms += [w * du[k] ** 2 for k, w in enumerate(gq[0]) if w != 0.0]
    terms += [w * du[j] * du[k] for (j, k), w in zip(PAIRS, gq[1]) if w != 0.0]
    assert len(terms) == (8 if equation == "aniso_eikonal_3d-sin" else 5)
    expect = sum(terms) - src
    tol = R.bar(prob, params)
    # (a product's error is each factor's error times the other factor's size: its scale is |w| max|du_j| max|du_k|)
    mx = [float(np.max(np.abs(d))) for d in du]
    scale = max([float(np.max(np.abs(t))) for t in terms] + [float(np.max(np.abs(src)))]
                + [abs(w) * mx[k] ** 2 for k, w in enumerate(gq[0])]
                + [abs(w) * mx[j] * mx[k] for (j, k), w in zip(PAIRS, gq[1])])
    err = float(np.max(np.abs(res - expect)))
    print("eq_residual", equation, "err / scale", err / scale, "tol", tol)
    assert res.shape == ms
    assert err < tol * scale
