"""Coefficient-field handles of the 3-axis solver (gpk_create3_opv; DeviceSolver3 with an
Operator3V): a field a_k on each axis's term and a field rho on the linear reaction term, entering
where the residual is formed (k3_combine_v) and where it is fed back (W_k = a_k R as the operand of
the reverse products; rho in k3_adam_u_v).

Yardstick: tests/operator3v_ref.py loss_grad_3d_opv (pinned on the CPU by
tests/test_operator3v_ref.py).  Tolerance: that of tests/test_gpu_kron3.py, max(1e-10, 50 cond eps)
with the largest cond K_k, on the loss and on every gradient block.  Open faces' bvals are NaN
throughout: they are never read.  Handles without a field, and handles whose fields are exactly 1.0
(rho exactly 0.0), are compared with gpk_create3_opx's bit for bit; predictions with a legacy
handle's.
"""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import rel
from tests.operator3v_ref import adam_replay_v, criterion_3d_opv, loss_grad_3d_opv
from tests.test_gpu_kron3 import KINDS, _tol
from tests.test_gpu_kron3_operator import _mask_bvals, _problem, _solver
from tests.test_operator3v_ref import smooth_fields

pytestmark = pytest.mark.gpu

NU = 0.1
HEAT = dict(c2=(-NU, -NU, 0.0), c1=(0.0, 0.0, 1.0), react=(0.0, 0.0, 0.0), faces=0b011111)
# a mixed-order axis (axis 1), a reaction, the final face open
FULL = dict(c2=(-0.3, 0.7, 0.0), c1=(0.8, 0.0, 1.3), react=(0.4, -0.5, 0.2), faces=0b011111)
NO_COEF = dict(a=(None, None, None), rho=None)
# the smallest sizes that cross a 32-tile boundary on the axis that has the field (axis 2: the
# permuted W_2 path); the operator's mixed axis is the field's axis
POSITION_CASES = [
    ((33, 20, 9), 0, dict(c2=(-0.3, 0.0, 1.0), c1=(0.8, -0.7, 0.0), react=(0.0, 0.0, 0.0), faces=63)),
    ((20, 33, 9), 1, dict(c2=(1.0, 0.6, 0.0), c1=(0.0, -1.1, 1.0), react=(0.0, 0.0, 0.0), faces=63)),
    ((9, 20, 33), 2, dict(c2=(-0.2, -0.2, 0.9), c1=(0.0, 0.0, -0.4), react=(0.0, 0.0, 0.0), faces=63)),
]


def _make(prob, Q, fs, op, coef, refine=False):
    from gpk.equations import Operator3V
    return _solver(prob, Q, fs, op=Operator3V(op["c2"], op["c1"], op["react"], op["faces"], a=coef["a"], rho=coef["rho"]),
                   refine=refine)


def _check(label, loss, g, prob, params, op, coef, tol=None):
    lo, go = loss_grad_3d_opv(prob, params, op, coef)
    tol = _tol(prob, params) if tol is None else tol
    gd = O.unflatten_params(params, g)
    errs = {k: rel(O.flatten_params(gd[k]), O.flatten_params(go[k])) for k in go}
    errs["loss"] = abs(loss - lo) / abs(lo)
    print(label, "tol %.3e" % tol, {k: "%.3e" % v for k, v in errs.items()})
    assert np.isfinite(loss) and np.all(np.isfinite(g))
    for k, v in errs.items():
        assert v < tol, (label, k, v, tol)


def _run(ns, op, coef, kind="Matern52_Cos_1d", Q=4, label="", seed=3):
    prob, params, fs = _problem(ns, kind, Q, seed)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    s = _make(prob, Q, fs, op, coef)
    try:
        s.set_params(params)
        assert np.array_equal(s.get_flat(), O.flatten_params(params))
        assert s.coef_info() == tuple(f is not None for f in tuple(coef["a"]) + (coef["rho"],))
        loss, g = s.loss_grad()
    finally:
        s.close()
    _check("%s %s %s Q%d" % (label, ns, kind, Q), loss, g, prob, params, op, coef)


# ---- 1. one field, on each axis in turn ----------------------------------------------------------
@pytest.mark.parametrize("ns,axis,op", POSITION_CASES)
def test_field_on_one_axis(ns, axis, op):
    _run(ns, op, smooth_fields(ns, (axis,), seed=axis), label="field on axis %d" % (axis + 1))


# ---- 2. every field at once ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_all_fields_mixed_axis_reaction_open_face_every_kind(kind):
    ns = (33, 33, 9)
    _run(ns, FULL, smooth_fields(ns, (0, 1, 2, 3), seed=5), kind, label="all fields")


def test_all_fields_q64():
    ns = (33, 33, 9)
    _run(ns, FULL, smooth_fields(ns, (0, 1, 2, 3), seed=5), Q=64, label="all fields")


@pytest.mark.parametrize("ns,axis", [((2, 14, 9), 0), ((9, 2, 14), 1), ((9, 14, 2), 2)])
def test_two_points_on_an_axis_with_a_field(ns, axis):
    _run(ns, FULL, smooth_fields(ns, (axis, 3), seed=axis), label="n = 2")


def test_rho_alone_and_fields_with_zeros_and_negative_values():
    ns = (6, 5, 4)
    helm = dict(c2=(1.0, 1.0, 1.0), c1=(0.0, 0.0, 0.0), react=(0.0, 0.0, 0.0), faces=63)
    _run(ns, helm, smooth_fields(ns, (3,), seed=1), label="rho alone")
    coef = smooth_fields(ns, (0, 1, 2, 3), seed=2)
    a = [f.copy() for f in coef["a"]]
    a[0][1:3] = 0.0          # a slab where axis 1's term vanishes
    a[1][:, :, 0] = 0.0
    a[2][a[2] > 0.0] = 0.0   # non-positive everywhere
    rho = -np.abs(coef["rho"])
    rho[0] = 0.0
    assert all((f == 0.0).any() and (f < 0.0).any() for f in a + [rho])
    _run(ns, FULL, dict(a=tuple(a), rho=rho), label="zeros and negative values")


# ---- 3. loss terms and the criterion -------------------------------------------------------------
def test_loss_terms_and_criterion():
    ns = (20, 14, 9)
    prob, params, fs = _problem(ns)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, FULL["faces"]))
    coef = smooth_fields(ns, (0, 1, 2, 3), seed=6)
    s = _make(prob, 4, fs, FULL, coef)
    try:
        s.set_params(params)
        loss, _ = s.loss_grad()
        terms = s.loss_terms()
        crit = s.criterion()
    finally:
        s.close()
    t = {}
    loss_grad_3d_opv(prob, params, FULL, coef, terms=t)
    tol = _tol(prob, params)
    cref = criterion_3d_opv(prob, params, FULL, coef)
    print("terms", {k: (terms[k], t[k]) for k in terms}, "criterion", crit, cref, "tol", tol)
    assert terms["loss"] == loss
    for k in terms:  # (a log det is a sum of O(1) log pivots: its error is measured against at least 1)
        assert abs(terms[k] - t[k]) < tol * max(abs(t[k]), 1.0), k
    assert abs(crit - cref) < tol * cref


# ---- 4. Adam trajectory --------------------------------------------------------------------------
def _heat_coef(prob):
    """heat_var-sin's conductivity ratio on the problem's own axes, rescaled to [0, 1]."""
    from gpk.equations import solution_3d_opv
    f = solution_3d_opv("heat_var-sin")[2].a[0]
    g = np.meshgrid(*[np.asarray(prob[f"x{k}"]) / np.asarray(prob[f"x{k}"])[-1] for k in (1, 2, 3)], indexing="ij")
    a = f(*g)
    assert a.min() >= 0.5 and a.max() <= 1.5 and a.std() > 0.1
    return dict(a=(a, a, None), rho=None)


def test_adam_trajectory_heat_form_vs_replay():
    """Ten steps of u_t - nu(x,y) (u_xx + u_yy), under test_adam_trajectory_3d_vs_oracle's bars."""
    ns = (24, 18, 12)
    prob, params, fs = _problem(ns, Q=5, seed=8)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, HEAT["faces"]))
    coef = _heat_coef(prob)
    s = _make(prob, 5, fs, HEAT, coef)
    try:
        s.set_params(params)
        losses = s.step(10)
        flat = s.get_flat()
    finally:
        s.close()
    ref, p = adam_replay_v(prob, params, HEAT, coef, 10)
    tol = _tol(prob, params)
    print("adam heat form", rel(losses, ref), rel(flat, O.flatten_params(p)), "tol", tol)
    assert rel(losses, ref) < max(1e-9, tol)
    assert rel(flat, O.flatten_params(p)) < max(1e-8, 10 * tol)


# ---- 5. refinement -------------------------------------------------------------------------------
def test_fields_refined_both_routes():
    """x in [0, 1] at (33, 20, 9), fields on all axes and rho: the gates open; the fused route and
    the two-GEMM route, whose residual scratch is Rx / Ryp / Rz (the W_k are tensors of their own)."""
    from gpk import _lib
    ns = (33, 20, 9)
    prob, params, fs = _problem(ns, unit=True)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, FULL["faces"]))
    coef = smooth_fields(ns, (0, 1, 2, 3), seed=7)
    bounds = []
    for a in (1, 2, 3):
        K = O.kernel_matrix(prob["kind"], prob[f"x{a}"], params[f"kernel_paras_{a}"], prob["jitter"])
        bounds.append(K[0, 0] * np.max(np.diag(np.linalg.inv(K))))
    print("gate bounds", bounds)
    assert any(b > 100.0 for b in bounds)
    for refine, route in ((True, _lib.REFINE_FUSED), ("gemm", _lib.REFINE_GEMM)):
        s = _make(prob, 4, fs, FULL, coef, refine=refine)
        try:
            s.set_params(params)
            loss, g = s.loss_grad()
            info = s.refine_info()
        finally:
            s.close()
        assert info["route"] == route
        assert info["open"] == [b > 100.0 for b in bounds] and any(info["open"]), (info, bounds)
        _check("fields refined route %d" % route, loss, g, prob, params, FULL, coef)


# ---- 6. no field, or fields of ones: gpk_create3_opx's handle, bit for bit -----------------------
def _raw_opv(prob, Q, fs, op, cf, refine=False):
    """A DeviceSolver3 whose handle comes from gpk_create3_opv called directly with `cf` (None: a
    NULL pointer; else a _lib.gpk_coef3)."""
    from gpk import _lib
    from gpk.equations import Operator3X
    s = _solver(prob, Q, fs, op=Operator3X.of(op), refine=refine)
    lib = _lib.load()
    _lib.check(lib.gpk_destroy3(s._h))
    s._h = None
    c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
    c.c2[:], c.c1[:], c.react[:], c.faces = op["c2"], op["c1"], op["react"], op["faces"]
    _lib.check(lib.gpk_create3_opv(ctypes.byref(s._prob), ctypes.byref(c), None if cf is None else ctypes.byref(cf),
                                   float(fs), ctypes.byref(h)))
    s._h = h
    return s


def _assert_same_bits(a, b, params):
    for s in (a, b):  # (a handle compared a second time starts from the same params and Adam state)
        s.set_params(params)
        s.set_opt_state(0, np.zeros(s.nparams), np.zeros(s.nparams))
    (la, ga), (lb, gb) = a.loss_grad(), b.loss_grad()
    assert la == lb and np.array_equal(ga, gb)
    assert a.loss_terms() == b.loss_terms()
    assert np.array_equal(a.step(5), b.step(5))
    assert np.array_equal(a.get_flat(), b.get_flat())
    assert a.stage_variants() == b.stage_variants()
    assert a.operator_info_x() == b.operator_info_x()


@pytest.mark.parametrize("ns,op,refine", [((33, 20, 9), FULL, False), ((20, 14, 9), HEAT, False), ((20, 14, 9), FULL, "gemm")])
def test_no_field_is_the_create3_opx_handle_bitwise(ns, op, refine):
    from gpk import _lib
    from gpk.equations import Operator3X
    prob, params, fs = _problem(ns, unit=bool(refine))
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    hs = [_solver(prob, 4, fs, op=Operator3X.of(op), refine=refine), _raw_opv(prob, 4, fs, op, None, refine),
          _raw_opv(prob, 4, fs, op, _lib.gpk_coef3(), refine), _make(prob, 4, fs, op, NO_COEF, refine)]
    try:
        for b in hs[1:]:
            assert b.coef_info() == (False,) * 4
            _assert_same_bits(hs[0], b, params)
    finally:
        for s in hs:
            s.close()


@pytest.mark.parametrize("ns,op,refine", [((33, 33, 9), FULL, False), ((20, 33, 9), HEAT, False), ((20, 14, 9), FULL, "gemm")])
def test_fields_of_ones_equal_the_create3_opx_handle_bitwise(ns, op, refine):
    """Every field exactly 1.0 and rho exactly 0.0: other kernels and operands (k3_combine_v,
    W_k, k3_adam_u_v), the same bits."""
    from gpk.equations import Operator3X
    prob, params, fs = _problem(ns, unit=bool(refine))
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    ones = dict(a=(np.ones(ns),) * 3, rho=np.zeros(ns))
    a, b = _solver(prob, 4, fs, op=Operator3X.of(op), refine=refine), _make(prob, 4, fs, op, ones, refine)
    try:
        assert b.coef_info() == (True,) * 4 and a.coef_info() == (False,) * 4
        _assert_same_bits(a, b, params)
    finally:
        a.close()
        b.close()


# ---- 7. predictions, repeated calls, the info calls ----------------------------------------------
def test_predictions_equal_legacy_repeated_calls_and_info():
    from gpk import _lib
    from gpk.equations import Operator3, Operator3X
    ns = (20, 14, 9)
    prob, params, fs = _problem(ns)
    coef = smooth_fields(ns, (0, 1, 2, 3), seed=9)
    a = _solver(prob, 4, fs)
    b = _make(dict(prob, bvals=_mask_bvals(prob["bvals"], ns, FULL["faces"])), 4, fs, FULL, coef)
    c = _solver(prob, 4, fs, op=Operator3X.of(FULL))
    d = _make(prob, 4, fs, dict(HEAT, faces=63), dict(a=(coef["a"][0], None, None), rho=None))
    e = _solver(prob, 4, fs, op=dict(order=(2, 2, 1), coef=(-NU, -NU, 1.0), react=(0.0, 0.0, 0.0), faces=63))
    try:
        for s in (a, b):
            s.set_params(params)
        xte = [np.linspace(-0.03, 1.02, m) * prob[f"x{k}"][-1] for k, m in zip((1, 2, 3), (11, 37, 5))]
        pts = np.random.default_rng(7).uniform(-0.03, 1.02, size=(50, 3)) * 2 * np.pi
        assert np.array_equal(a.predict(*xte), b.predict(*xte))
        assert np.array_equal(a.predict_deriv(*xte, deriv=(1, 0, 2)), b.predict_deriv(*xte, deriv=(1, 0, 2)))
        assert np.array_equal(a.evaluate(pts), b.evaluate(pts))
        assert np.array_equal(a.evaluate(pts, deriv=(1, 0, 2)), b.evaluate(pts, deriv=(1, 0, 2)))
        # repeated calls: equal bits (nothing the step leaves behind feeds the next one)
        (l1, g1), (l2, g2) = b.loss_grad(), b.loss_grad()
        assert l1 == l2 and np.array_equal(g1, g2)
        # the info calls report the constant part, as for the opx handle of the same operator
        assert b.operator_info_x() == Operator3X.of(FULL) == c.operator_info_x()
        with pytest.raises(_lib.GPKError) as err:  # FULL has a mixed axis
            b.operator_info()
        assert err.value.code == _lib.GPK_EINVAL
        assert d.operator_info() == Operator3((2, 2, 1), (-NU, -NU, 1.0)) == e.operator_info()
        assert b.coef_info() == (True, True, True, True) and d.coef_info() == (True, False, False, False)
        for s in (a, c, e):
            assert s.coef_info() == (False, False, False, False)
        lib, has = _lib.load(), (ctypes.c_int32 * 4)()
        assert lib.gpk_coef_info3(b._h, None) == _lib.GPK_EINVAL
        assert lib.gpk_coef_info3(None, has) == _lib.GPK_EINVAL
    finally:
        for s in (a, b, c, d, e):
            s.close()


def test_create3_opv_argument_errors_on_the_device():
    from gpk._lib import GPK_EINVAL, GPKError
    ns = (8, 7, 6)
    prob, params, fs = _problem(ns, Q=3, seed=1)
    coef = smooth_fields(ns, (1, 3), seed=1)
    for slot, bad in ((1, np.nan), (3, np.inf)):
        f = [None, coef["a"][1].copy(), None, coef["rho"].copy()]
        f[slot][-1, -1, -1] = bad
        with pytest.raises(GPKError) as e:
            _make(prob, 3, fs, dict(FULL, faces=63), dict(a=tuple(f[:3]), rho=f[3]))
        assert e.value.code == GPK_EINVAL
    for op in (dict(FULL, faces=0), dict(FULL, c1=(0.0, np.nan, 0.0))):
        with pytest.raises(GPKError) as e:
            _make(prob, 3, fs, op, coef)
        assert e.value.code == GPK_EINVAL
    with pytest.raises(ValueError):  # an array of another shape never reaches the library
        _make(prob, 3, fs, dict(FULL, faces=63), dict(a=(np.ones((8, 7, 5)), None, None), rho=None))


# ---- 8. model class ------------------------------------------------------------------------------
def _heat_var_model(ncol=8, mtest=9):
    from gpk.equations import solution_3d_opv
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single, boundary_3d, get_mesh_data, load_config
    cfg = load_config("heat_var-sin")
    u, src, op = solution_3d_opv("heat_var-sin")
    scale = 2 * np.pi if cfg["scale"] == "2pi" else 1.0
    xte, ute = get_mesh_data(u, (mtest,) * 3, scale)
    xc, umh = get_mesh_data(u, (ncol,) * 3, scale)
    _, srcv = get_mesh_data(src, (ncol,) * 3, scale)
    bvals = boundary_3d(umh, op.faces)
    tp = {"kernel": kernel_class("Matern52_Cos_1d"), "equation": "heat_var-sin", "llk_weight": cfg["llk_weight"],
          "logdet": cfg["logdet"], "lr": cfg["lr"], "Q": cfg["Q"], "freq_scale": cfg["freq_scale"], "nepoch": 20,
          "tol": -1}
    prob = dict(kind="Matern52_Cos_1d", x1=xc[0], x2=xc[1], x3=xc[2], src=srcv, bvals=bvals, jitter=1e-6,
                llk_weight=float(cfg["llk_weight"]), logdet=float(cfg["logdet"]))
    fields = op.fields(xc)
    coef = dict(a=tuple(fields[:3]), rho=fields[3])

    def make():
        return GP_solver_3d_single(bvals, xc, srcv, 1e-6, tp, X_test=xte, u_test=ute)
    return prob, op, coef, tp, xte, ute, make


def test_train_heat_var_vs_replay_resume_and_eq_residual(tmp_path):
    from gpk.equations import solution_3d_opv
    from gpk.model_GP_solver_3d import get_mesh_data
    from tests.test_gpu_kron3_predict import ref_predict
    prob, op, coef, tp, xte, ute, make = _heat_var_model()
    assert np.isnan(prob["bvals"]).sum() == 64  # the final-time face is open
    m = make()
    try:
        assert m.Nb == 5 * 64 and m.dev.operator_info_x() == op.constant
        assert m.dev.coef_info() == op.has == (True, True, False, False)
        log, stop, min_err = m.train(20, verbose=False)
        flat = m.dev.get_flat()
        axes, src_te = get_mesh_data(solution_3d_opv("heat_var-sin")[1], (9, 7, 5), 1.0)
        res = m.eq_residual(m.params, tuple(axes), src_te)
    finally:
        m.dev.close()
    assert res.shape == (9, 7, 5) and np.all(np.isfinite(res))
    p0 = O.init_params_3d(8, 8, 8, tp["Q"], tp["freq_scale"])
    errs = []

    def after(i, p):
        pr = ref_predict(prob, p, xte)
        errs.append(np.linalg.norm(pr.ravel() - ute.ravel()) / np.linalg.norm(ute.ravel()))
    losses, _ = adam_replay_v(prob, p0, op.constant.as_dict(), coef, 20, lr=tp["lr"], after=after)
    losses = [np.log(lo) if lo > 1 else lo for lo in losses]
    tol = max(1e-8, 10 * _tol(prob, p0))
    print("train heat_var loss rel", rel(log["loss_list"], losses), "err rel", rel(log["err_list"], errs), "tol", tol)
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
        assert m2.dev.coef_info() == (True, True, False, False)  # the fields come back from the equation's name
        assert np.array_equal(m2.dev.get_flat(), flat)
    finally:
        m2.dev.close()
    assert min2 == min_err and sorted(log2) == sorted(log)
    for k in log:
        assert np.array_equal(np.asarray(log2[k]), np.asarray(log[k])), k


@pytest.mark.parametrize("equation", ["helmholtz_var-sin", "heat_var-sin", "transport_var-sin"])
def test_eq_residual_opv(equation):
    """eq_residual on a 7 x 6 x 5 test grid against NumPy on the reference predictions with the
    fields evaluated on that grid, at the bar of tests/test_gpu_eq_residual.py (the project's bar
    scaled by the largest term)."""
    from gpk.equations import solution_3d_opv
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single
    from tests import predict_deriv_ref as R
    op = solution_3d_opv(equation)[2]
    ns, ms = (20, 14, 9), (7, 6, 5)
    prob, params, fs = _problem(ns)
    tp = {"kernel": kernel_class(prob["kind"]), "llk_weight": prob["llk_weight"], "Q": 4, "lr": 0.01,
          "freq_scale": fs, "logdet": True, "equation": equation}
    m = GP_solver_3d_single(_mask_bvals(prob["bvals"], ns, op.faces), (prob["x1"], prob["x2"], prob["x3"]),
                            prob["src"], prob["jitter"], tp)
    xte = R.grid_axes(prob, params, ms)
    src = np.random.default_rng(2).normal(size=ms)
    try:
        assert m.dev.operator_info_x() == op.constant and m.dev.coef_info() == op.has
        res = m.eq_residual(params, tuple(xte), src)
    finally:
        m.dev.close()
    *a, rho = op.fields(xte)
    terms = []
    for k in range(3):
        for o, w in ((2, op.c2[k]), (1, op.c1[k])):
            if w != 0.0:
                d = [0, 0, 0]
                d[k] = o
                t = w * R.ref_grid(prob, params, xte, d)
                terms.append(t if a[k] is None else a[k] * t)
    if rho is not None:
        terms.append(rho * R.ref_grid(prob, params, xte, [0, 0, 0]))
    assert len(terms) == {"helmholtz_var-sin": 4, "heat_var-sin": 3, "transport_var-sin": 3}[equation]
    expect = sum(terms) - src
    tol = R.bar(prob, params)
    scale = max(float(np.max(np.abs(t))) for t in terms + [src])
    err = float(np.max(np.abs(res - expect)))
    print("eq_residual", equation, "err / scale", err / scale, "tol", tol)
    assert res.shape == ms
    assert err < tol * scale
