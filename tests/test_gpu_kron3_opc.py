"""Convective terms on the 3-axis solver (gpk_create3_opc; DeviceSolver3 with conv): g_k u du/dx_k
per axis, formed from the order-1 block of the two-block assembly (DERIV_SPLIT), added to the
residual by k3_combine_c, and carried back through the dual-product T_k, the G_D1k products, the
DERIV_SPLIT contraction and k3_adam_u_c.

Yardstick: tests/operator3c_ref.py loss_grad_3d_opc (pinned on the CPU by
tests/test_operator3c_ref.py).  Tolerance: that of tests/test_gpu_kron3_opn.py, max(1e-10, 50 cond
eps) with the largest cond K_k, on the loss and on every gradient block.  Every bvals / dvals entry
that must not be read is NaN throughout.  Handles without a convective axis are compared with
gpk_create3_opn's bit for bit.
"""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import rel
from tests.operator3c_ref import adam_replay_c, criterion_3d_opc, loss_grad_3d_opc
from tests.test_gpu_kron3 import KINDS, _tol
from tests.test_gpu_kron3_operator import _mask_bvals, _problem
from tests.test_gpu_kron3_opn import ALL_DFACES, ALL_OP
from tests.test_gpu_kron3_opv import FULL, NO_COEF
from tests.test_operator3n_ref import random_dvals
from tests.test_operator3v_ref import smooth_fields

pytestmark = pytest.mark.gpu

ALL_CONV = (1.0, -0.7, 0.5)


def _make(prob, Q, fs, op, coef, dfaces, dvals, conv, refine=False):
    from gpk.equations import Operator3V
    from gpk.model_GP_solver_3d import DeviceSolver3
    return DeviceSolver3("poisson", prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                         Q=Q, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"], lr=0.01,
                         freq_scale=fs, refine=refine,
                         operator=Operator3V(op["c2"], op["c1"], op["react"], op["faces"], a=coef["a"], rho=coef["rho"]),
                         dfaces=dfaces, dvals=dvals, conv=conv)


def _check(label, loss, g, prob, params, op, coef, dfaces, dvals, conv):
    lo, go = loss_grad_3d_opc(prob, params, op, coef, dfaces, dvals, conv)
    tol = _tol(prob, params)
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
    return prob, params, fs, (random_dvals(ns, dfaces, seed=dfaces) if dfaces else None)


def _run(ns, op, coef, dfaces, conv, kind="Matern52_Cos_1d", Q=4, label="", refine=False, unit=False):
    prob, params, fs, dvals = _setup(ns, op, dfaces, kind, Q, unit=unit)
    s = _make(prob, Q, fs, op, coef, dfaces, dvals, conv, refine=refine)
    try:
        s.set_params(params)
        assert s.conv_info() == tuple(conv) and s.bdata_info() == (op["faces"], dfaces)
        assert s.operator_info_x().as_dict() == {k: tuple(float(x) for x in v) if k != "faces" else v
                                                 for k, v in op.items()}
        assert len(s.stage_variants()) == 8  # the six stages and the two launches of V_k and G_D1k
        loss, g = s.loss_grad()
        info = s.refine_info() if refine else None
    finally:
        s.close()
    _check("%s %s %s Q%d conv %s" % (label, ns, kind, Q, conv), loss, g, prob, params, op, coef, dfaces, dvals, conv)
    return info


def _one(axis, g=1.25):
    return tuple(g if a == axis else 0.0 for a in range(3))


# ---- 1. one convective axis in each position, crossing a 32-tile on that axis --------------------
@pytest.mark.parametrize("ns,axis", [((33, 20, 9), 0), ((20, 33, 9), 1), ((9, 20, 33), 2)])
def test_one_convective_axis_tile_crossing_on_the_axis(ns, axis):
    _run(ns, FULL, NO_COEF, 0, _one(axis), label="axis %d" % (axis + 1))


# ---- 2. everything at once -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_everything_at_once_every_kind(kind):
    ns = (33, 33, 9)
    _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=5), ALL_DFACES, ALL_CONV, kind, label="all")


def test_everything_at_once_q64():
    ns = (33, 33, 9)
    _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=5), ALL_DFACES, ALL_CONV, Q=64, label="all")


# ---- 3. n = 2 on the convective axis -------------------------------------------------------------
@pytest.mark.parametrize("ns,axis", [((2, 14, 9), 0), ((9, 2, 14), 1), ((9, 14, 2), 2)])
def test_two_points_on_the_convective_axis(ns, axis):
    _run(ns, FULL, NO_COEF, 0, _one(axis), label="n = 2")


# ---- 4. a pure convective axis next to a mixed one -----------------------------------------------
@pytest.mark.parametrize("pure", [0, 1, 2])
def test_pure_convective_axis_next_to_a_mixed_convective_axis(pure):
    """Axis `pure` has c2 = c1 = 0 (inviscid: its D block is all zeros, its D1 block carries the
    term); the next axis is mixed and convective (the two blocks coexist); the third is plain."""
    mixed, plain = (pure + 1) % 3, (pure + 2) % 3
    c2, c1, conv = [0.0] * 3, [0.0] * 3, [0.0] * 3
    c2[mixed], c1[mixed], conv[mixed] = -0.3, 0.8, -0.6
    c2[plain] = 0.7
    conv[pure] = 1.5
    op = dict(c2=tuple(c2), c1=tuple(c1), react=(0.4, 0.0, 0.2), faces=0b011111)
    _run((20, 33, 9), op, NO_COEF, 0, tuple(conv), label="pure axis %d" % (pure + 1))


# ---- 5. refinement -------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [True, "gemm"])
def test_refined_both_routes(refine):
    """x in [0, 1] at (33, 20, 9): the gates open; V_k reads the refined A_k, and T_k carries the
    convective term before the refinement of X_k reads it as its right-hand side."""
    from gpk import _lib
    ns = (33, 20, 9)
    info = _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=7), ALL_DFACES, ALL_CONV,
                label="refined %r" % refine, refine=refine, unit=True)
    assert info["route"] == (_lib.REFINE_FUSED if refine is True else _lib.REFINE_GEMM)
    assert any(info["open"]), info


# ---- 6. loss terms, boundary terms and the criterion ---------------------------------------------
def test_loss_terms_boundary_terms_and_criterion():
    ns = (20, 14, 9)
    prob, params, fs, dvals = _setup(ns, ALL_OP, ALL_DFACES)
    coef = smooth_fields(ns, (0, 1, 2, 3), seed=6)
    s = _make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, ALL_CONV)
    try:
        s.set_params(params)
        loss, _ = s.loss_grad()
        terms, bt, crit = s.loss_terms(), s.boundary_terms(), s.criterion()
    finally:
        s.close()
    t = {}
    loss_grad_3d_opc(prob, params, ALL_OP, coef, ALL_DFACES, dvals, ALL_CONV, terms=t)
    tol = _tol(prob, params)
    cref = criterion_3d_opc(prob, params, ALL_OP, coef, ALL_DFACES, dvals, ALL_CONV)
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
    loss_grad_3d_opc(prob, params, ALL_OP, coef, ALL_DFACES, dvals, None, terms=t0)
    assert abs(t0["egap"] - terms["egap"]) > 1e-6 * terms["egap"]


# ---- 7. bits -------------------------------------------------------------------------------------
def _raw_opc(prob, Q, fs, op, coef, dfaces, dvals, cv, refine=False):
    """A DeviceSolver3 whose handle comes from gpk_create3_opc called directly with `cv` (None: a
    NULL pointer; else a _lib.gpk_conv3)."""
    from gpk import _lib
    from gpk._lib import dptr
    s = _make(prob, Q, fs, op, coef, dfaces, dvals, None, refine=refine)
    lib = _lib.load()
    _lib.check(lib.gpk_destroy3(s._h))
    s._h = None
    c, h, cf, bd = _lib.gpk_operator3x(), ctypes.c_void_p(), _lib.gpk_coef3(), _lib.gpk_bdata3()
    c.c2[:], c.c1[:], c.react[:], c.faces = op["c2"], op["c1"], op["react"], op["faces"]
    for k, f in enumerate(getattr(s, "_coef", [None] * 4)[:3]):
        if f is not None:
            cf.a[k] = dptr(f)
    if getattr(s, "_coef", [None] * 4)[3] is not None:
        cf.rho = dptr(s._coef[3])
    if dfaces:
        bd.dfaces, bd.dvals = dfaces, dptr(s._dvals)
    _lib.check(lib.gpk_create3_opc(ctypes.byref(s._prob), ctypes.byref(c), ctypes.byref(cf), ctypes.byref(bd),
                                   None if cv is None else ctypes.byref(cv), float(fs), ctypes.byref(h)))
    s._h = h
    return s


@pytest.mark.parametrize("dfaces,fields", [(0, ()), (ALL_DFACES, (0, 1, 2, 3))])
def test_no_convective_axis_is_the_create3_opn_handle_bitwise(dfaces, fields):
    from gpk import _lib
    ns = (33, 20, 9)
    op = ALL_OP if dfaces else FULL
    prob, params, fs, dvals = _setup(ns, op, dfaces)
    coef = smooth_fields(ns, fields, seed=4)
    hs = [_make(prob, 4, fs, op, coef, dfaces, dvals, None), _raw_opc(prob, 4, fs, op, coef, dfaces, dvals, None),
          _raw_opc(prob, 4, fs, op, coef, dfaces, dvals, _lib.gpk_conv3()),
          _make(prob, 4, fs, op, coef, dfaces, dvals, (0.0, 0.0, 0.0))]
    try:
        for s in hs:
            s.set_params(params)
            assert s.conv_info() == (0.0, 0.0, 0.0) and s.bdata_info() == (op["faces"], dfaces)
        ref = hs[0].loss_grad()
        assert len(hs[0].stage_variants()) == 6
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
    a, b = (_make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, ALL_CONV) for _ in range(2))
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


# ---- 8. Adam trajectory --------------------------------------------------------------------------
def test_adam_trajectory_vs_replay():
    """Five steps under the bars of tests/test_gpu_kron3_opn.py's trajectory."""
    ns = (20, 14, 9)
    prob, params, fs, dvals = _setup(ns, ALL_OP, ALL_DFACES, Q=5, seed=8)
    coef = smooth_fields(ns, (0, 3), seed=8)
    s = _make(prob, 5, fs, ALL_OP, coef, ALL_DFACES, dvals, ALL_CONV)
    try:
        s.set_params(params)
        losses = s.step(5)
        flat = s.get_flat()
    finally:
        s.close()
    ref, p = adam_replay_c(prob, params, ALL_OP, coef, ALL_DFACES, dvals, ALL_CONV, 5)
    tol = _tol(prob, params)
    print("adam opc", rel(losses, ref), rel(flat, O.flatten_params(p)), "tol", tol)
    assert rel(losses, ref) < max(1e-9, tol)
    assert rel(flat, O.flatten_params(p)) < max(1e-8, 10 * tol)


# ---- 9. Burgers through the model class ----------------------------------------------------------
def _burgers_model(ncol=8, mtest=9):
    from gpk.equations import solution_3d_opc
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single, boundary_3d, get_mesh_data, load_config
    cfg = load_config("burgers_t-sin")
    u, src, op, dfaces, _, conv = solution_3d_opc("burgers_t-sin")
    xte, ute = get_mesh_data(u, (mtest,) * 3, 1.0)
    xc, umh = get_mesh_data(u, (ncol,) * 3, 1.0)
    _, srcv = get_mesh_data(src, (ncol,) * 3, 1.0)
    bvals = boundary_3d(umh, op.faces)
    tp = {"kernel": kernel_class("Matern52_Cos_1d"), "equation": "burgers_t-sin", "llk_weight": cfg["llk_weight"],
          "logdet": cfg["logdet"], "lr": cfg["lr"], "Q": cfg["Q"], "freq_scale": cfg["freq_scale"], "nepoch": 20,
          "tol": -1}
    prob = dict(kind="Matern52_Cos_1d", x1=xc[0], x2=xc[1], x3=xc[2], src=srcv, bvals=bvals, jitter=1e-6,
                llk_weight=float(cfg["llk_weight"]), logdet=float(cfg["logdet"]))

    def make():
        return GP_solver_3d_single(bvals, xc, srcv, 1e-6, tp, X_test=xte, u_test=ute)
    return prob, op, conv, tp, xte, ute, make


def test_train_burgers_vs_replay_and_resume(tmp_path):
    from tests.test_gpu_kron3_predict import ref_predict
    prob, op, conv, tp, xte, ute, make = _burgers_model()
    assert np.isnan(prob["bvals"]).sum() == 64  # the final-time face is open
    m = make()
    try:
        assert m.Nb == 5 * 64 and m.dev.operator_info_x() == op
        assert m.dev.conv_info() == conv == (1.0, 1.0, 0.0) and m.dev.bdata_info() == (0b011111, 0)
        log, stop, min_err = m.train(20, verbose=False)
        flat = m.dev.get_flat()
    finally:
        m.dev.close()
    p0 = O.init_params_3d(8, 8, 8, tp["Q"], tp["freq_scale"])
    errs = []

    def after(i, p):
        pr = ref_predict(prob, p, xte)
        errs.append(np.linalg.norm(pr.ravel() - ute.ravel()) / np.linalg.norm(ute.ravel()))
    losses, _ = adam_replay_c(prob, p0, op.as_dict(), NO_COEF, 0, None, conv, 20, lr=tp["lr"], after=after)
    losses = [np.log(lo) if lo > 1 else lo for lo in losses]
    tol = max(1e-8, 10 * _tol(prob, p0))
    print("train burgers_t loss rel", rel(log["loss_list"], losses), "err rel", rel(log["err_list"], errs), "tol", tol)
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
        assert m2.dev.conv_info() == (1.0, 1.0, 0.0)  # conv comes back from the equation's name
        assert np.array_equal(m2.dev.get_flat(), flat)
    finally:
        m2.dev.close()
    assert min2 == min_err and sorted(log2) == sorted(log)
    for k in log:
        assert np.array_equal(np.asarray(log2[k]), np.asarray(log[k])), k


@pytest.mark.parametrize("equation", ["burgers_t-sin", "burgers_3d-sin"])
def test_eq_residual_opc(equation):
    """eq_residual on a 7 x 6 x 5 test grid against NumPy on the reference predictions, at the bar
    of tests/test_gpu_eq_residual.py (the project's bar scaled by the largest term; the convective
    terms are products of two predictions, each within that bar of its reference, so their scale is
    the product of the factors' largest values)."""
    from gpk.equations import solution_3d_opc
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single
    from tests import predict_deriv_ref as R
    op, conv = solution_3d_opc(equation)[2], solution_3d_opc(equation)[5]
    ns, ms = (20, 14, 9), (7, 6, 5)
    prob, params, fs = _problem(ns)
    tp = {"kernel": kernel_class(prob["kind"]), "llk_weight": prob["llk_weight"], "Q": 4, "lr": 0.01,
          "freq_scale": fs, "logdet": True, "equation": equation}
    m = GP_solver_3d_single(_mask_bvals(prob["bvals"], ns, op.faces), (prob["x1"], prob["x2"], prob["x3"]),
                            prob["src"], prob["jitter"], tp)
    xte = R.grid_axes(prob, params, ms)
    src = np.random.default_rng(2).normal(size=ms)
    try:
        assert m.dev.operator_info_x() == op and m.dev.conv_info() == conv
        res = m.eq_residual(params, tuple(xte), src)
    finally:
        m.dev.close()
    terms, scales = [], []
    for k in range(3):
        for o, w in ((2, op.c2[k]), (1, op.c1[k])):
            if w != 0.0:
                d = [0, 0, 0]
                d[k] = o
                terms.append(w * R.ref_grid(prob, params, xte, d))
                scales.append(float(np.max(np.abs(terms[-1]))))
    u = R.ref_grid(prob, params, xte, [0, 0, 0])
    nconv = 0
    for k in range(3):
        if conv[k] != 0.0:
            d = [0, 0, 0]
            d[k] = 1
            du = R.ref_grid(prob, params, xte, d)
            terms.append(conv[k] * u * du)
            scales.append(2.0 * abs(conv[k]) * float(np.max(np.abs(u))) * float(np.max(np.abs(du))))
            nconv += 1
    assert nconv == {"burgers_t-sin": 2, "burgers_3d-sin": 3}[equation] and len(terms) == nconv + 3
    expect = sum(terms) - src
    tol = R.bar(prob, params)
    scale = max(scales + [float(np.max(np.abs(src)))])
    err = float(np.max(np.abs(res - expect)))
    print("eq_residual", equation, "err / scale", err / scale, "tol", tol)
    assert res.shape == ms
    assert err < tol * scale
