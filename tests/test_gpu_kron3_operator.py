"""Operator handles of the 3-axis solver (gpk_create3_op; DeviceSolver3(operator=...)): one
derivative order and weight per axis, a reaction polynomial, a face mask.

Yardstick: tests/operator3_ref.py loss_grad_3d_op (pinned on the CPU by tests/test_operator3_ref.py).
Tolerance: that of tests/test_gpu_kron3.py, max(1e-10, 50 cond eps) with the largest cond K_k, on
the loss and on every gradient block.  Open faces' bvals are NaN throughout: they are never read.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import problem_3d, rel
from tests.operator3_ref import FACES, POISSON_OP, adam_replay, criterion_3d_op, loss_grad_3d_op
from tests.test_gpu_kron3 import KINDS, _tol

pytestmark = pytest.mark.gpu

NU = 0.1
HEAT = dict(order=(2, 2, 1), coef=(-NU, -NU, 1.0), react=(0.0, 0.0, 0.0), faces=0b011111)
MIXED = dict(coef=(-0.3, -0.7, 1.0), react=(0.4, -0.5, 0.2), faces=0b011111)


def _mask_bvals(bvals, ns, faces):
    """bvals in the six-face layout with the open faces' entries NaN."""
    bv, o = np.array(bvals, np.float64), 0
    for f, sl in enumerate(FACES):
        n = np.zeros(ns)[sl].size
        if not (faces >> f) & 1:
            bv[o:o + n] = np.nan
        o += n
    return bv


@functools.lru_cache(maxsize=None)
def _problem(ns, kind="Matern52_Cos_1d", Q=4, seed=3, unit=False):
    """problem_3d's seeded data and params (unit: x in [0, 1], else [0, 2 pi]); read-only."""
    return problem_3d(eq="allencahn" if unit else "poisson", kind=kind, ns=ns, Q=Q, seed=seed)


def _solver(prob, Q, fs, op=None, refine=False, eq="poisson"):
    from gpk.model_GP_solver_3d import DeviceSolver3
    return DeviceSolver3(eq, prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                         Q=Q, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"],
                         lr=0.01, freq_scale=fs, refine=refine, operator=op)


def _check(label, loss, g, prob, params, op, tol=None):
    lo, go = loss_grad_3d_op(prob, params, op)
    tol = _tol(prob, params) if tol is None else tol
    gd = O.unflatten_params(params, g)
    errs = {k: rel(O.flatten_params(gd[k]), O.flatten_params(go[k])) for k in go}
    errs["loss"] = abs(loss - lo) / abs(lo)
    print(label, "tol %.3e" % tol, {k: "%.3e" % v for k, v in errs.items()})
    assert np.isfinite(loss) and np.all(np.isfinite(g))
    for k, v in errs.items():
        assert v < tol, (label, k, v, tol)


# ---- 1. Poisson stated as an operator equals gpk_create3 ---------------------------------------
@pytest.mark.parametrize("ns", [(20, 14, 9), (33, 20, 9)])
def test_poisson_operator_equals_legacy_bitwise(ns):
    prob, params, fs = _problem(ns)
    a, b = _solver(prob, 4, fs), _solver(prob, 4, fs, op=POISSON_OP)
    try:
        for s in (a, b):
            s.set_params(params)
        (la, ga), (lb, gb) = a.loss_grad(), b.loss_grad()
        assert la == lb and np.array_equal(ga, gb)
        assert a.loss_terms() == b.loss_terms()
        assert np.array_equal(a.step(5), b.step(5))
        assert np.array_equal(a.get_flat(), b.get_flat())
        assert a.stage_variants() == b.stage_variants()
    finally:
        a.close()
        b.close()


# ---- 2. orders and weights ---------------------------------------------------------------------
# n = 33 (two 32-tiles) on the first-order axis in each position; axes 0 and 1 with different
# orders (two assembly / contraction launches each) and with equal orders (one shared launch)
ORDER_CASES = [((33, 20, 9), (1, 2, 2)), ((20, 33, 9), (2, 1, 2)), ((9, 20, 33), (2, 2, 1)), ((33, 20, 9), (1, 1, 1))]
assert {o[0] == o[1] for _, o in ORDER_CASES} == {True, False}


def _run_orders(ns, order, kind):
    prob, params, fs = _problem(ns, kind)
    op = dict(MIXED, order=order)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    s = _solver(prob, 4, fs, op=op)
    try:
        s.set_params(params)
        loss, g = s.loss_grad()
    finally:
        s.close()
    _check("orders %s %s %s" % (ns, order, kind), loss, g, prob, params, op)


@pytest.mark.parametrize("ns,order", ORDER_CASES)
def test_orders_and_weights(ns, order):
    _run_orders(ns, order, "Matern52_Cos_1d")


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "Matern52_Cos_1d"])
def test_first_order_last_axis_every_kind(kind):
    _run_orders((9, 20, 33), (2, 2, 1), kind)


# ---- 3. faces ----------------------------------------------------------------------------------
@pytest.mark.parametrize("faces", [63 ^ (1 << f) for f in range(6)] + [0b010000])
def test_face_masks(faces):
    ns = (6, 5, 4)
    prob, params, fs = _problem(ns, seed=5)
    op = dict(order=(2, 1, 2), coef=(-0.3, -0.7, 1.0), react=(0.4, -0.5, 0.2), faces=faces)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, faces))
    s = _solver(prob, 4, fs, op=op)
    try:
        s.set_params(params)
        loss, g = s.loss_grad()
        terms = s.loss_terms()
        crit = s.criterion()
        assert np.array_equal(s.get_flat(), O.flatten_params(params))
    finally:
        s.close()
    _check("faces %s" % bin(faces), loss, g, prob, params, op)
    t = {}
    loss_grad_3d_op(prob, params, op, terms=t)
    tol = _tol(prob, params)
    cref = criterion_3d_op(prob, params, op)
    print("faces", bin(faces), "bgap", terms["bgap"], t["bgap"], "Nb", t["Nb"], "criterion", crit, cref)
    assert np.isfinite(terms["bgap"]) and abs(terms["bgap"] - t["bgap"]) < tol * t["bgap"]
    assert abs(terms["egap"] - t["egap"]) < tol * t["egap"]
    assert abs(crit - cref) < tol * cref


# ---- 4. Adam trajectory ------------------------------------------------------------------------
def test_adam_trajectory_heat_vs_replay():
    """Ten steps of the heat form from seeded params, under test_adam_trajectory_3d_vs_oracle's bars."""
    ns = (24, 18, 12)
    prob, params, fs = _problem(ns, Q=5, seed=8)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, HEAT["faces"]))
    s = _solver(prob, 5, fs, op=HEAT)
    try:
        s.set_params(params)
        losses = s.step(10)
        flat = s.get_flat()
    finally:
        s.close()
    ref, p = adam_replay(prob, params, HEAT, 10)
    tol = _tol(prob, params)
    print("adam heat", rel(losses, ref), rel(flat, O.flatten_params(p)), "tol", tol)
    assert rel(losses, ref) < max(1e-9, tol)
    assert rel(flat, O.flatten_params(p)) < max(1e-8, 10 * tol)


# ---- 5. refinement -----------------------------------------------------------------------------
def test_heat_refined_both_routes():
    """x in [0, 1] at (33, 20, 9): the gates open; the fused route and the two-GEMM route."""
    from gpk import _lib
    ns = (33, 20, 9)
    prob, params, fs = _problem(ns, unit=True)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, HEAT["faces"]))
    bounds = []
    for a in (1, 2, 3):
        K = O.kernel_matrix(prob["kind"], prob[f"x{a}"], params[f"kernel_paras_{a}"], prob["jitter"])
        bounds.append(K[0, 0] * np.max(np.diag(np.linalg.inv(K))))
    print("gate bounds", bounds)
    assert any(b > 100.0 for b in bounds)
    for refine, route in ((True, _lib.REFINE_FUSED), ("gemm", _lib.REFINE_GEMM)):
        s = _solver(prob, 4, fs, op=HEAT, refine=refine)
        try:
            s.set_params(params)
            loss, g = s.loss_grad()
            info = s.refine_info()
        finally:
            s.close()
        assert info["route"] == route
        assert info["open"] == [b > 100.0 for b in bounds], (info, bounds)
        _check("heat refined route %d" % route, loss, g, prob, params, HEAT)


# ---- 6. predictions and operator_info ----------------------------------------------------------
def test_predictions_equal_legacy_and_operator_info():
    from gpk.equations import Operator3
    ns = (20, 14, 9)
    prob, params, fs = _problem(ns)
    op = dict(MIXED, order=(2, 1, 2))
    a = _solver(prob, 4, fs)
    b = _solver(dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"])), 4, fs, op=op)
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
        assert b.operator_info() == Operator3.of(op)
        assert a.operator_info() == Operator3.of(POISSON_OP)
        assert c.operator_info() == Operator3((2, 2, 2), (1.0, 1.0, 1.0), (-1.0, 0.0, 1.0), 63)
    finally:
        for s in (a, b, c):
            s.close()


# ---- 7. argument errors ------------------------------------------------------------------------
def test_create3_op_argument_errors():
    from gpk import _lib
    from gpk._lib import GPKError
    prob, params, fs = _problem((8, 7, 6), Q=3, seed=1)
    bad = [dict(POISSON_OP, order=(2, 0, 2)), dict(POISSON_OP, order=(3, 2, 2)),
           dict(POISSON_OP, coef=(1.0, np.nan, 1.0)), dict(POISSON_OP, coef=(np.inf, 1.0, 1.0)),
           dict(POISSON_OP, react=(0.0, 0.0, np.inf)), dict(POISSON_OP, react=(np.nan, 0.0, 0.0)),
           dict(POISSON_OP, faces=0), dict(POISSON_OP, faces=64), dict(POISSON_OP, faces=-1)]
    for op in bad:
        with pytest.raises(GPKError) as e:
            _solver(prob, 3, fs, op=op)
        assert e.value.code == _lib.GPK_EINVAL, op
    with pytest.raises(GPKError) as e:  # the operator says everything: eq must be Poisson
        _solver(prob, 3, fs, op=POISSON_OP, eq="allencahn")
    assert e.value.code == _lib.GPK_EINVAL
    # NULL op / NULL out, straight on the ABI
    good = _solver(prob, 3, fs, op=POISSON_OP)
    try:
        lib, h = _lib.load(), ctypes.c_void_p()
        assert lib.gpk_create3_op(ctypes.byref(good._prob), None, fs, ctypes.byref(h)) == _lib.GPK_EINVAL
        c = _lib.gpk_operator3()
        assert lib.gpk_create3_op(ctypes.byref(good._prob), ctypes.byref(c), fs, None) == _lib.GPK_EINVAL
        assert lib.gpk_operator_info3(good._h, None) == _lib.GPK_EINVAL
        assert lib.gpk_operator_info3(None, ctypes.byref(c)) == _lib.GPK_EINVAL
        # a weight of zero is allowed: it drops that axis's term
        z = _solver(prob, 3, fs, op=dict(POISSON_OP, coef=(1.0, 0.0, 1.0)))
        try:
            z.set_params(params)
            loss, g = z.loss_grad()
        finally:
            z.close()
        _check("zero weight", loss, g, prob, params, dict(POISSON_OP, coef=(1.0, 0.0, 1.0)))
    finally:
        good.close()


# ---- 8. model class ----------------------------------------------------------------------------
def _heat_model(ncol=8, mtest=9):
    from gpk.equations import solution_3d_op
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single, boundary_3d, get_mesh_data, load_config
    cfg = load_config("heat_3d-sin")
    u, src, op = solution_3d_op("heat_3d-sin")
    scale = 2 * np.pi if cfg["scale"] == "2pi" else 1.0
    xte, ute = get_mesh_data(u, (mtest,) * 3, scale)
    xc, umh = get_mesh_data(u, (ncol,) * 3, scale)
    _, srcv = get_mesh_data(src, (ncol,) * 3, scale)
    bvals = boundary_3d(umh, op.faces)
    tp = {"kernel": kernel_class("Matern52_Cos_1d"), "equation": "heat_3d-sin", "llk_weight": cfg["llk_weight"],
          "logdet": cfg["logdet"], "lr": cfg["lr"], "Q": cfg["Q"], "freq_scale": cfg["freq_scale"], "nepoch": 20,
          "tol": -1}
    prob = dict(kind="Matern52_Cos_1d", x1=xc[0], x2=xc[1], x3=xc[2], src=srcv, bvals=bvals, jitter=1e-6,
                llk_weight=float(cfg["llk_weight"]), logdet=float(cfg["logdet"]))

    def make():
        return GP_solver_3d_single(bvals, xc, srcv, 1e-6, tp, X_test=xte, u_test=ute)
    return prob, op.as_dict(), tp, xte, ute, make


def test_train_heat_vs_replay_and_resume(tmp_path):
    from tests.test_gpu_kron3_predict import ref_predict
    prob, op, tp, xte, ute, make = _heat_model()
    assert np.isnan(prob["bvals"]).sum() == 64  # the final-time face is open
    m = make()
    try:
        assert m.Nb == 5 * 64 and m.dev.operator_info().as_dict() == op
        log, stop, min_err = m.train(20, verbose=False)
        flat = m.dev.get_flat()
    finally:
        m.dev.close()
    p0 = O.init_params_3d(8, 8, 8, tp["Q"], tp["freq_scale"])
    errs = []

    def after(i, p):
        pr = ref_predict(prob, p, xte)
        errs.append(np.linalg.norm(pr.ravel() - ute.ravel()) / np.linalg.norm(ute.ravel()))
    losses, _ = adam_replay(prob, p0, op, 20, lr=tp["lr"], after=after)
    losses = [np.log(lo) if lo > 1 else lo for lo in losses]
    tol = max(1e-8, 10 * _tol(prob, p0))
    print("train heat loss rel", rel(log["loss_list"], losses), "err rel", rel(log["err_list"], errs), "tol", tol)
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


@pytest.mark.parametrize("equation", ["heat_3d-sin", "allencahn_t-sin"])
def test_eq_residual_operator(equation):
    """eq_residual on a 7 x 6 x 5 test grid against NumPy on the reference predictions, at the bar
    of tests/test_gpu_eq_residual.py (the project's bar scaled by the largest term)."""
    from gpk.equations import solution_3d_op
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single
    from tests import predict_deriv_ref as R
    op = solution_3d_op(equation)[2]
    ns, ms = (20, 14, 9), (7, 6, 5)
    prob, params, fs = _problem(ns)
    tp = {"kernel": kernel_class(prob["kind"]), "llk_weight": prob["llk_weight"], "Q": 4, "lr": 0.01,
          "freq_scale": fs, "logdet": True, "equation": equation}
    m = GP_solver_3d_single(_mask_bvals(prob["bvals"], ns, op.faces), (prob["x1"], prob["x2"], prob["x3"]),
                            prob["src"], prob["jitter"], tp)
    xte = R.grid_axes(prob, params, ms)
    src = np.random.default_rng(2).normal(size=ms)
    try:
        assert m.dev.operator_info() == op
        res = m.eq_residual(params, tuple(xte), src)
    finally:
        m.dev.close()
    terms = []
    for k in range(3):
        d = [0, 0, 0]
        d[k] = op.order[k]
        terms.append(op.coef[k] * R.ref_grid(prob, params, xte, d))
    if any(op.react):
        u = R.ref_grid(prob, params, xte, (0, 0, 0))
        terms.append(op.react[0] * u + op.react[1] * u ** 2 + op.react[2] * u ** 3)
    expect = sum(terms) - src
    tol = R.bar(prob, params)
    scale = max(float(np.max(np.abs(t))) for t in terms + [src])
    err = float(np.max(np.abs(res - expect)))
    print("eq_residual", equation, "err / scale", err / scale, "tol", tol)
    assert res.shape == ms
    assert err < tol * scale
