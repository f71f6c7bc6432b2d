"""Mixed-order operator handles of the 3-axis solver (gpk_create3_opx; DeviceSolver3 with an
Operator3X): a second- and a first-order term on the same axis, D_k = c2_k DD_k + c1_k D1_k
assembled by one kernel (DERIV_BOTH) and contracted by one.

Yardstick: tests/operator3x_ref.py loss_grad_3d_opx (pinned on the CPU by
tests/test_operator3x_ref.py).  Tolerance: that of tests/test_gpu_kron3.py, max(1e-10, 50 cond eps)
with the largest cond K_k, on the loss and on every gradient block.  Open faces' bvals are NaN
throughout: they are never read.  Handles without a mixed axis are compared with gpk_create3_op's,
and predictions with a legacy handle's, bit for bit.
"""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import rel
from tests.operator3x_ref import adam_replay_x, as_op, criterion_3d_opx, loss_grad_3d_opx
from tests.test_gpu_kron3 import KINDS, _tol
from tests.test_gpu_kron3_operator import _mask_bvals, _problem, _solver

pytestmark = pytest.mark.gpu

NU, B1, B2 = 0.05, 1.0, 0.5
CONVDIFF_T = dict(c2=(-NU, -NU, 0.0), c1=(B1, B2, 1.0), react=(0.0, 0.0, 0.0), faces=0b011111)
ALL_MIXED = dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, -0.6, 1.3), react=(0.4, -0.5, 0.2), faces=0b011111)
# the mixed axis in each position at n = 33 (two 32-tiles; position 1 is the permuted mode-2 path):
# (both, 1, 2) and (2, both, 1) launch every axis alone, (2, 2, both) shares the launch of axes 1-2
POSITION_CASES = [
    ((33, 20, 9), dict(c2=(-0.3, 0.0, 1.0), c1=(0.8, -0.7, 0.0), react=(0.0, 0.0, 0.0), faces=63)),
    ((20, 33, 9), dict(c2=(1.0, 0.6, 0.0), c1=(0.0, -1.1, 1.0), react=(0.0, 0.0, 0.0), faces=63)),
    ((9, 20, 33), dict(c2=(-0.2, -0.2, 0.9), c1=(0.0, 0.0, -0.4), react=(0.0, 0.0, 0.0), faces=63)),
]
# two mixed axes with different weights in one shared launch
SHARED = ((33, 33, 9), dict(c2=(-0.3, 0.7, 0.0), c1=(0.8, -0.6, 1.0), react=(0.0, 0.0, 0.0), faces=63))


def _make(prob, Q, fs, op, refine=False):
    from gpk.equations import Operator3X
    return _solver(prob, Q, fs, op=Operator3X.of(op), refine=refine)


def _check(label, loss, g, prob, params, op, tol=None):
    lo, go = loss_grad_3d_opx(prob, params, op)
    tol = _tol(prob, params) if tol is None else tol
    gd = O.unflatten_params(params, g)
    errs = {k: rel(O.flatten_params(gd[k]), O.flatten_params(go[k])) for k in go}
    errs["loss"] = abs(loss - lo) / abs(lo)
    print(label, "tol %.3e" % tol, {k: "%.3e" % v for k, v in errs.items()})
    assert np.isfinite(loss) and np.all(np.isfinite(g))
    for k, v in errs.items():
        assert v < tol, (label, k, v, tol)


def _run(ns, op, kind="Matern52_Cos_1d", Q=4, label="", seed=3):
    prob, params, fs = _problem(ns, kind, Q, seed)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    s = _make(prob, Q, fs, op)
    try:
        s.set_params(params)
        assert np.array_equal(s.get_flat(), O.flatten_params(params))
        loss, g = s.loss_grad()
    finally:
        s.close()
    _check("%s %s %s Q%d" % (label, ns, kind, Q), loss, g, prob, params, op)


# ---- 1. the mixed axis in every position, shared and separate launches ---------------------------
@pytest.mark.parametrize("ns,op", POSITION_CASES + [SHARED])
def test_mixed_axis_positions_and_shared_launch(ns, op):
    from gpk.equations import Operator3X
    assert sum(Operator3X.of(op).mixed) == (2 if ns == SHARED[0] else 1)
    _run(ns, op, label="position")


@pytest.mark.parametrize("kind", KINDS)
def test_all_axes_mixed_reaction_open_face_every_kind(kind):
    _run((20, 14, 9), ALL_MIXED, kind, label="all mixed")


def test_all_axes_mixed_q64():
    _run((20, 14, 9), ALL_MIXED, Q=64, label="all mixed")


@pytest.mark.parametrize("ns,axis", [((2, 14, 9), 0), ((9, 14, 2), 2)])
def test_two_points_on_a_mixed_axis(ns, axis):
    c2, c1 = [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]
    c2[axis], c1[axis] = -0.3, 0.8
    _run(ns, dict(c2=tuple(c2), c1=tuple(c1), react=(0.0, 0.0, 0.0), faces=63), label="n = 2")


# ---- 2. loss terms and the criterion -------------------------------------------------------------
def test_loss_terms_and_criterion():
    ns = (20, 14, 9)
    prob, params, fs = _problem(ns)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, ALL_MIXED["faces"]))
    s = _make(prob, 4, fs, ALL_MIXED)
    try:
        s.set_params(params)
        loss, _ = s.loss_grad()
        terms = s.loss_terms()
        crit = s.criterion()
    finally:
        s.close()
    t = {}
    loss_grad_3d_opx(prob, params, ALL_MIXED, terms=t)
    tol = _tol(prob, params)
    cref = criterion_3d_opx(prob, params, ALL_MIXED)
    print("terms", {k: (terms[k], t[k]) for k in terms}, "criterion", crit, cref, "tol", tol)
    assert terms["loss"] == loss
    for k in terms:  # (a log det is a sum of O(1) log pivots: its error is measured against at least 1)
        assert abs(terms[k] - t[k]) < tol * max(abs(t[k]), 1.0), k
    assert abs(crit - cref) < tol * cref


# ---- 3. Adam trajectory --------------------------------------------------------------------------
def test_adam_trajectory_convdiff_t_vs_replay():
    """Ten steps of the convection-diffusion form, under test_adam_trajectory_3d_vs_oracle's bars."""
    ns = (24, 18, 12)
    prob, params, fs = _problem(ns, Q=5, seed=8)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, CONVDIFF_T["faces"]))
    s = _make(prob, 5, fs, CONVDIFF_T)
    try:
        s.set_params(params)
        losses = s.step(10)
        flat = s.get_flat()
    finally:
        s.close()
    ref, p = adam_replay_x(prob, params, CONVDIFF_T, 10)
    tol = _tol(prob, params)
    print("adam convdiff_t", rel(losses, ref), rel(flat, O.flatten_params(p)), "tol", tol)
    assert rel(losses, ref) < max(1e-9, tol)
    assert rel(flat, O.flatten_params(p)) < max(1e-8, 10 * tol)


# ---- 4. refinement -------------------------------------------------------------------------------
def test_mixed_refined_both_routes():
    """x in [0, 1] at (33, 20, 9): the gates open; the fused route and the two-GEMM route."""
    from gpk import _lib
    ns = (33, 20, 9)
    prob, params, fs = _problem(ns, unit=True)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, CONVDIFF_T["faces"]))
    bounds = []
    for a in (1, 2, 3):
        K = O.kernel_matrix(prob["kind"], prob[f"x{a}"], params[f"kernel_paras_{a}"], prob["jitter"])
        bounds.append(K[0, 0] * np.max(np.diag(np.linalg.inv(K))))
    print("gate bounds", bounds)
    assert any(b > 100.0 for b in bounds)
    for refine, route in ((True, _lib.REFINE_FUSED), ("gemm", _lib.REFINE_GEMM)):
        s = _make(prob, 4, fs, CONVDIFF_T, refine=refine)
        try:
            s.set_params(params)
            loss, g = s.loss_grad()
            info = s.refine_info()
        finally:
            s.close()
        assert info["route"] == route
        assert info["open"] == [b > 100.0 for b in bounds], (info, bounds)
        _check("convdiff_t refined route %d" % route, loss, g, prob, params, CONVDIFF_T)


# ---- 5. no mixed axis: gpk_create3_op's handle, bit for bit --------------------------------------
ONE_ORDER = [((20, 14, 9), dict(c2=(-0.1, -0.1, 0.0), c1=(0.0, 0.0, 1.0), react=(0.0, 0.0, 0.0), faces=0b011111)),
             ((33, 20, 9), dict(c2=(0.0, 0.7, 1.0), c1=(-0.3, 0.0, 0.0), react=(0.4, -0.5, 0.2), faces=0b011111)),
             ((20, 14, 9), dict(c2=(1.0, 0.0, 1.0), c1=(0.0, 0.0, 0.0), react=(0.0, 0.0, 0.0), faces=63))]


@pytest.mark.parametrize("ns,op", ONE_ORDER)
def test_no_mixed_axis_equals_create3_op_bitwise(ns, op):
    from gpk.equations import Operator3, Operator3X
    prob, params, fs = _problem(ns)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    a, b = _solver(prob, 4, fs, op=as_op(op)), _make(prob, 4, fs, op)
    try:
        for s in (a, b):
            s.set_params(params)
        (la, ga), (lb, gb) = a.loss_grad(), b.loss_grad()
        assert la == lb and np.array_equal(ga, gb)
        assert a.loss_terms() == b.loss_terms()
        assert np.array_equal(a.step(5), b.step(5))
        assert np.array_equal(a.get_flat(), b.get_flat())
        assert a.stage_variants() == b.stage_variants()
        assert b.operator_info() == Operator3.of(as_op(op)) == a.operator_info()
        assert a.operator_info_x() == b.operator_info_x() == Operator3X.of(op)
    finally:
        a.close()
        b.close()


# ---- 6. predictions and the info calls -----------------------------------------------------------
def test_predictions_equal_legacy_and_operator_info_x():
    from gpk import _lib
    from gpk._lib import GPKError
    from gpk.equations import Operator3X
    ns = (20, 14, 9)
    prob, params, fs = _problem(ns)
    a = _solver(prob, 4, fs)
    b = _make(dict(prob, bvals=_mask_bvals(prob["bvals"], ns, ALL_MIXED["faces"])), 4, fs, ALL_MIXED)
    c = _solver(_problem(ns, unit=True)[0], 4, fs, eq="allencahn")
    try:
        for s in (a, b):
            s.set_params(params)
        xte = [np.linspace(-0.03, 1.02, m) * prob[f"x{k}"][-1] for k, m in zip((1, 2, 3), (11, 37, 5))]
        pts = np.random.default_rng(7).uniform(-0.03, 1.02, size=(50, 3)) * 2 * np.pi
        assert np.array_equal(a.predict(*xte), b.predict(*xte))
        assert np.array_equal(a.predict_deriv(*xte, deriv=(1, 0, 2)), b.predict_deriv(*xte, deriv=(1, 0, 2)))
        assert np.array_equal(a.evaluate(pts), b.evaluate(pts))
        assert np.array_equal(a.evaluate(pts, deriv=(1, 0, 2)), b.evaluate(pts, deriv=(1, 0, 2)))
        assert b.operator_info_x() == Operator3X.of(ALL_MIXED)
        assert a.operator_info_x() == Operator3X((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
        assert c.operator_info_x() == Operator3X((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (-1.0, 0.0, 1.0), 63)
        with pytest.raises(GPKError) as e:  # gpk_operator3 cannot state a mixed axis
            b.operator_info()
        assert e.value.code == _lib.GPK_EINVAL
        lib, x = _lib.load(), _lib.gpk_operator3x()
        assert lib.gpk_operator_info3x(b._h, None) == _lib.GPK_EINVAL
        assert lib.gpk_operator_info3x(None, ctypes.byref(x)) == _lib.GPK_EINVAL
    finally:
        for s in (a, b, c):
            s.close()


# ---- 7. argument errors --------------------------------------------------------------------------
def test_create3_opx_argument_errors():
    from gpk import _lib
    from gpk._lib import GPKError
    prob, params, fs = _problem((8, 7, 6), Q=3, seed=1)
    ok = dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, -0.6, 1.3), react=(0.0, 0.0, 0.0), faces=63)
    bad = [dict(ok, c2=(1.0, np.nan, 1.0)), dict(ok, c2=(np.inf, 1.0, 1.0)), dict(ok, c1=(0.0, 0.0, np.nan)),
           dict(ok, c1=(-np.inf, 0.0, 0.0)), dict(ok, react=(0.0, 0.0, np.inf)), dict(ok, react=(np.nan, 0.0, 0.0)),
           dict(ok, faces=0), dict(ok, faces=64), dict(ok, faces=-1)]
    for op in bad:
        with pytest.raises(GPKError) as e:
            _make(prob, 3, fs, op)
        assert e.value.code == _lib.GPK_EINVAL, op
    with pytest.raises(GPKError) as e:  # the operator says everything: eq must be Poisson
        from gpk.equations import Operator3X
        _solver(prob, 3, fs, op=Operator3X.of(ok), eq="allencahn")
    assert e.value.code == _lib.GPK_EINVAL
    good = _make(prob, 3, fs, ok)
    try:
        lib, h = _lib.load(), ctypes.c_void_p()
        c = _lib.gpk_operator3x()
        assert lib.gpk_create3_opx(ctypes.byref(good._prob), None, fs, ctypes.byref(h)) == _lib.GPK_EINVAL
        assert lib.gpk_create3_opx(ctypes.byref(good._prob), ctypes.byref(c), fs, None) == _lib.GPK_EINVAL
        assert lib.gpk_create3_opx(None, ctypes.byref(c), fs, ctypes.byref(h)) == _lib.GPK_EINVAL
        good.set_params(params)
        loss, g = good.loss_grad()
    finally:
        good.close()
    _check("all mixed (8, 7, 6)", loss, g, prob, params, ok)


# ---- 8. model class ------------------------------------------------------------------------------
def _convdiff_model(ncol=8, mtest=9):
    from gpk.equations import solution_3d_opx
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single, boundary_3d, get_mesh_data, load_config
    cfg = load_config("convdiff_t-sin")
    u, src, op = solution_3d_opx("convdiff_t-sin")
    scale = 2 * np.pi if cfg["scale"] == "2pi" else 1.0
    xte, ute = get_mesh_data(u, (mtest,) * 3, scale)
    xc, umh = get_mesh_data(u, (ncol,) * 3, scale)
    _, srcv = get_mesh_data(src, (ncol,) * 3, scale)
    bvals = boundary_3d(umh, op.faces)
    tp = {"kernel": kernel_class("Matern52_Cos_1d"), "equation": "convdiff_t-sin", "llk_weight": cfg["llk_weight"],
          "logdet": cfg["logdet"], "lr": cfg["lr"], "Q": cfg["Q"], "freq_scale": cfg["freq_scale"], "nepoch": 20,
          "tol": -1}
    prob = dict(kind="Matern52_Cos_1d", x1=xc[0], x2=xc[1], x3=xc[2], src=srcv, bvals=bvals, jitter=1e-6,
                llk_weight=float(cfg["llk_weight"]), logdet=float(cfg["logdet"]))

    def make():
        return GP_solver_3d_single(bvals, xc, srcv, 1e-6, tp, X_test=xte, u_test=ute)
    return prob, op, tp, xte, ute, make


def test_train_convdiff_t_vs_replay_and_resume(tmp_path):
    from tests.test_gpu_kron3_predict import ref_predict
    prob, op, tp, xte, ute, make = _convdiff_model()
    assert np.isnan(prob["bvals"]).sum() == 64  # the final-time face is open
    m = make()
    try:
        assert m.Nb == 5 * 64 and m.dev.operator_info_x() == op and op.mixed == (True, True, False)
        log, stop, min_err = m.train(20, verbose=False)
        flat = m.dev.get_flat()
    finally:
        m.dev.close()
    p0 = O.init_params_3d(8, 8, 8, tp["Q"], tp["freq_scale"])
    errs = []

    def after(i, p):
        pr = ref_predict(prob, p, xte)
        errs.append(np.linalg.norm(pr.ravel() - ute.ravel()) / np.linalg.norm(ute.ravel()))
    losses, _ = adam_replay_x(prob, p0, op, 20, lr=tp["lr"], after=after)
    losses = [np.log(lo) if lo > 1 else lo for lo in losses]
    tol = max(1e-8, 10 * _tol(prob, p0))
    print("train convdiff_t loss rel", rel(log["loss_list"], losses), "err rel", rel(log["err_list"], errs), "tol", tol)
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
        assert np.array_equal(m2.dev.get_flat(), flat)
    finally:
        m2.dev.close()
    assert min2 == min_err and sorted(log2) == sorted(log)
    for k in log:
        assert np.array_equal(np.asarray(log2[k]), np.asarray(log[k])), k


@pytest.mark.parametrize("equation", ["convdiff_t-sin", "convdiff_3d-sin"])
def test_eq_residual_opx(equation):
    """eq_residual on a 7 x 6 x 5 test grid against NumPy on the reference predictions, at the bar
    of tests/test_gpu_eq_residual.py (the project's bar scaled by the largest term)."""
    from gpk.equations import solution_3d_opx
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single
    from tests import predict_deriv_ref as R
    op = solution_3d_opx(equation)[2]
    ns, ms = (20, 14, 9), (7, 6, 5)
    prob, params, fs = _problem(ns)
    tp = {"kernel": kernel_class(prob["kind"]), "llk_weight": prob["llk_weight"], "Q": 4, "lr": 0.01,
          "freq_scale": fs, "logdet": True, "equation": equation}
    m = GP_solver_3d_single(_mask_bvals(prob["bvals"], ns, op.faces), (prob["x1"], prob["x2"], prob["x3"]),
                            prob["src"], prob["jitter"], tp)
    xte = R.grid_axes(prob, params, ms)
    src = np.random.default_rng(2).normal(size=ms)
    try:
        assert m.dev.operator_info_x() == op
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
    assert len(terms) == (5 if equation == "convdiff_t-sin" else 6)
    expect = sum(terms) - src
    tol = R.bar(prob, params)
    scale = max(float(np.max(np.abs(t))) for t in terms + [src])
    err = float(np.max(np.abs(res - expect)))
    print("eq_residual", equation, "err / scale", err / scale, "tol", tol)
    assert res.shape == ms
    assert err < tol * scale
