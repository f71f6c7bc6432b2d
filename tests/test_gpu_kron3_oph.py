"""Third- and fourth-order terms on the 3-axis solver (gpk_create3_oph; DeviceSolver3 with high=):
axis k's block is D_k = c4_k D4_k + c3_k D3_k + c2_k DD_k + c1_k D1_k, assembled by one kernel
(DERIV_HIGH; DERIV_HIGH_SPLIT where the axis also owns the plain order-1 block: convective, cross
and drift axes) and contracted by one.

Yardstick: tests/operator3h_ref.py loss_grad_3d_oph (pinned on the CPU by
tests/test_operator3h_ref.py against 50-digit differentiation of kappa and torch autograd).
Tolerance: the project's _tol of tests/test_gpu_kron3.py, max(1e-10, 50 cond eps) with the largest
cond K_k, on the loss and on every gradient block.  Order-4 blocks scale with om^4, so the
yardstick's own fp64 rounding was measured on these problems (problem_3d's defaults, x in [0, 2 pi]
and fs = 5, and the unit cube): against its long-double evaluation every order-3 / order-4 block and
their parameter-gradient contraction is within 2.3e-4 of the bar (tests/test_operator3h_host.py
asserts a tenth), so the defaults stand.  Every bvals / dvals entry that must not be read is NaN.
Each case asserts that the yardstick without the high-order weights gives another answer by more
than 100 tolerances.  Handles without a high-order weight are compared with gpk_create3_opb's bit for
bit, predictions with a legacy handle's.
"""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import mp_fields_high as MH
from tests.field_ulp_inputs import EPS, N_D
from tests.helpers import rand_kp, rel
from tests.operator3b_ref import loss_grad_3d_opb
from tests.operator3h_ref import adam_replay_h, criterion_3d_oph, kernel_block_n, loss_grad_3d_oph
from tests.test_gpu_kron3 import KINDS, _tol
from tests.test_gpu_kron3_operator import _mask_bvals, _problem
from tests.test_gpu_kron3_opb import drift_for
from tests.test_gpu_kron3_opv import NO_COEF
from tests.test_operator3n_ref import random_dvals
from tests.test_operator3v_ref import smooth_fields

pytestmark = pytest.mark.gpu

ZERO3 = (0.0, 0.0, 0.0)
NONE3 = (None, None, None)
# the weights: om reaches 2 pi 5 ~ 31, so c4 om^4 ~ c3 om^3 ~ c2 om^2 at c4 ~ 1e-3, c3 ~ 3e-2, c2 ~ 1
# the high axis in each position at n = 33 (two 32-tiles; position 2 is the permuted mode-2 path):
# (high, 1, 2) and (2, high, 1) launch every axis alone, (2, 2, high) shares the launch of axes 1-2
POSITION_CASES = [
    ((33, 20, 9), dict(c2=(-0.3, 0.0, 1.0), c1=(0.8, -0.7, 0.0), react=ZERO3, faces=63), ((2e-3, 0.0, 0.0), (-3e-2, 0.0, 0.0))),
    ((20, 33, 9), dict(c2=(1.0, 0.6, 0.0), c1=(0.0, -1.1, 1.0), react=ZERO3, faces=63), ((0.0, -1.5e-3, 0.0), (0.0, 4e-2, 0.0))),
    ((9, 20, 33), dict(c2=(-0.2, -0.2, 0.9), c1=(0.0, 0.0, -0.4), react=ZERO3, faces=63), ((0.0, 0.0, 1e-3), (0.0, 0.0, 2e-2))),
]
# two high axes with different weights in one shared launch (axis 2 without c2 and c1)
SHARED = ((33, 33, 9), dict(c2=(-0.3, 0.0, 0.0), c1=(0.8, 0.0, 1.0), react=ZERO3, faces=63),
          ((2e-3, -1e-3, 0.0), (0.0, 3e-2, 0.0)))
ALL_OP = dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, -0.6, 1.3), react=(0.4, -0.5, 0.2), faces=0b011111)
ALL_HIGH = ((2e-3, -1e-3, 1.5e-3), (-3e-2, 2e-2, 4e-2))
KDV = (dict(c2=ZERO3, c1=(0.0, 0.0, 1.0), react=ZERO3, faces=0b011111), (1.0, 0.0, 0.0), (ZERO3, (0.01, 0.0, 0.0)))


def _make(prob, Q, fs, op, coef=NO_COEF, dfaces=0, dvals=None, conv=None, cross=None, drift=None, high=None,
          refine=False):
    from gpk.equations import Operator3V
    from gpk.model_GP_solver_3d import DeviceSolver3
    return DeviceSolver3("poisson", prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                         Q=Q, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"], lr=0.01,
                         freq_scale=fs, refine=refine,
                         operator=Operator3V(op["c2"], op["c1"], op["react"], op["faces"], a=coef["a"], rho=coef["rho"]),
                         dfaces=dfaces, dvals=dvals, conv=conv, cross=cross, drift=drift, high=high)


def _check(label, loss, g, prob, params, op, coef, dfaces, dvals, conv, cross, drift, high):
    lo, go = loss_grad_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high)
    tol = _tol(prob, params)
    gd = O.unflatten_params(params, g)
    errs = {k: rel(O.flatten_params(gd[k]), O.flatten_params(go[k])) for k in go}
    errs["loss"] = abs(loss - lo) / abs(lo)
    print(label, "tol %.3e" % tol, {k: "%.3e" % v for k, v in errs.items()})
    assert np.isfinite(loss) and np.all(np.isfinite(g))
    # the terms matter: the yardstick without them moves some checked quantity by over 100 tol
    lo0, go0 = loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift)
    moved = {k: rel(O.flatten_params(go0[k]), O.flatten_params(go[k])) for k in go}
    moved["loss"] = abs(lo0 - lo) / abs(lo)
    assert lo0 != lo and max(moved.values()) > 100 * tol, (lo0, lo, moved, tol)
    for k, v in errs.items():
        assert v < tol, (label, k, v, tol)


def _setup(ns, op, dfaces=0, kind="Matern52_Cos_1d", Q=4, seed=3, unit=False):
    prob, params, fs = _problem(ns, kind, Q, seed, unit)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    return prob, params, fs, (random_dvals(ns, dfaces, seed=dfaces) if dfaces else None)


def _run(ns, op, high, coef=NO_COEF, dfaces=0, conv=None, cross=None, drift=None, kind="Matern52_Cos_1d", Q=4,
         label="", refine=False, unit=False):
    prob, params, fs, dvals = _setup(ns, op, dfaces, kind, Q, unit=unit)
    s = _make(prob, Q, fs, op, coef, dfaces, dvals, conv, cross, drift, high, refine)
    try:
        s.set_params(params)
        assert np.array_equal(s.get_flat(), O.flatten_params(params))
        assert s.high_info() == (tuple(high[0]), tuple(high[1]))
        assert s.operator_info_x().as_dict() == {k: tuple(float(x) for x in v) if k != "faces" else v
                                                 for k, v in op.items()}
        loss, g = s.loss_grad()
        info = s.refine_info() if refine else None
    finally:
        s.close()
    _check("%s %s %s Q%d high %s" % (label, ns, kind, Q, high), loss, g, prob, params, op, coef, dfaces, dvals,
           conv, cross, drift or NONE3, high)
    return info


# ---- 1. the high axis in every position, shared and separate launches -----------------------------
@pytest.mark.parametrize("ns,op,high", POSITION_CASES + [SHARED])
def test_high_axis_positions_and_shared_launch(ns, op, high):
    _run(ns, op, high, label="position")


@pytest.mark.parametrize("kind", KINDS)
def test_all_four_orders_on_all_axes_every_kind(kind):
    _run((20, 14, 9), ALL_OP, ALL_HIGH, kind=kind, label="all four")


def test_all_four_orders_on_all_axes_q64():
    _run((20, 14, 9), ALL_OP, ALL_HIGH, Q=64, label="all four")


@pytest.mark.parametrize("ns,axis", [((2, 14, 9), 0), ((9, 14, 2), 2)])
def test_two_points_on_a_high_axis(ns, axis):
    c2, c1, c4, c3 = [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    c2[axis], c1[axis], c4[axis], c3[axis] = -0.3, 0.8, 2e-3, -3e-2
    _run(ns, dict(c2=tuple(c2), c1=tuple(c1), react=ZERO3, faces=63), (tuple(c4), tuple(c3)), label="n = 2")


# ---- 2. the two-block mode: the axis also owns the plain order-1 block ----------------------------
@pytest.mark.parametrize("what", ["conv", "cross", "drift", "dfaces"])
def test_high_axis_with_the_order_1_block_alongside(what):
    """Axis 1 of (33, 20, 9) carries all four orders and, in turn, a convective weight, a cross pair,
    a drift field (each needs D1_1 and G_D1_1: DERIV_HIGH_SPLIT) and derivative data on its faces (the
    face rows are formed on their own: DERIV_HIGH)."""
    ns = (33, 20, 9)
    op, high = POSITION_CASES[0][1], ((2e-3, 0.0, 0.0), (-3e-2, 0.0, 0.0))
    kw = dict(conv=dict(conv=(1.0, 0.0, 0.0)), cross=dict(cross=(0.8, 0.0, 0.0)),
              drift=dict(drift=drift_for(ns, (0,))), dfaces=dict(dfaces=0b000011))[what]
    _run(ns, dict(op, faces=0b111100) if what == "dfaces" else op, high, label=what, **kw)


def test_everything_on_the_same_axis():
    """c4, c3, c2, c1, a field a_1, a convective weight, both pairs, a drift field and derivative data,
    all on axis 1; the other axes high as well."""
    ns = (33, 20, 9)
    _run(ns, dict(ALL_OP, faces=0b011110), ALL_HIGH, coef=smooth_fields(ns, (0, 3), seed=5), dfaces=0b000001,
         conv=(1.0, 0.0, 0.5), cross=(0.8, -0.6, 0.0), drift=drift_for(ns, (0, 2)), label="everything")


# ---- 3. a coefficient field on a high axis --------------------------------------------------------
@pytest.mark.parametrize("ns,op,high", POSITION_CASES)
def test_coefficient_field_multiplies_all_four_orders(ns, op, high):
    axis = [k for k in range(3) if high[0][k] != 0.0][0]
    _run(ns, op, high, coef=smooth_fields(ns, (axis,), seed=2), label="a_%d" % (axis + 1))


# ---- 4. bits --------------------------------------------------------------------------------------
def _raw_oph(prob, Q, fs, op, conv, cross, hi):
    """A DeviceSolver3 whose handle comes from gpk_create3_oph called directly with `hi` (None: a NULL
    pointer; else a _lib.gpk_high3)."""
    from gpk import _lib
    s = _make(prob, Q, fs, op, conv=conv, cross=cross)
    lib = _lib.load()
    _lib.check(lib.gpk_destroy3(s._h))
    s._h = None
    c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
    cv, mx = _lib.gpk_conv3(), _lib.gpk_cross3()
    c.c2[:], c.c1[:], c.react[:], c.faces = op["c2"], op["c1"], op["react"], op["faces"]
    cv.g[:] = conv
    mx.m[:] = cross
    _lib.check(lib.gpk_create3_oph(ctypes.byref(s._prob), ctypes.byref(c), None, None, ctypes.byref(cv),
                                   ctypes.byref(mx), None, None if hi is None else ctypes.byref(hi), float(fs),
                                   ctypes.byref(h)))
    s._h = h
    return s


@pytest.mark.parametrize("conv,cross", [(ZERO3, ZERO3), ((1.0, -0.7, 0.5), (0.8, -0.6, 1.1))])
def test_no_high_weight_is_the_create3_opb_handle_bitwise(conv, cross):
    from gpk import _lib
    ns = (33, 20, 9)
    prob, params, fs, _ = _setup(ns, ALL_OP)
    hs = [_make(prob, 4, fs, ALL_OP, conv=conv, cross=cross),
          _raw_oph(prob, 4, fs, ALL_OP, conv, cross, None),
          _raw_oph(prob, 4, fs, ALL_OP, conv, cross, _lib.gpk_high3()),
          _make(prob, 4, fs, ALL_OP, conv=conv, cross=cross, high=(ZERO3, ZERO3))]
    try:
        for s in hs:
            s.set_params(params)
            assert s.high_info() == (ZERO3, ZERO3)
            assert s.cross_info() == cross and s.conv_info() == conv
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


def test_stage_list_is_the_opb_handles_and_info_calls():
    """The host treats D_k as opaque: a high handle launches the GEMM stages of the same handle with
    the axis entered as a mixed one; gpk_operator_info3 refuses it as it refuses a mixed axis."""
    from gpk import _lib
    from gpk._lib import GPKError
    ns = (20, 14, 9)
    prob, params, fs, _ = _setup(ns, ALL_OP)
    a = _make(prob, 4, fs, ALL_OP, conv=(1.0, 0.0, 0.0))
    b = _make(prob, 4, fs, ALL_OP, conv=(1.0, 0.0, 0.0), high=ALL_HIGH)
    try:
        assert a.stage_variants() == b.stage_variants()
        assert a.high_info() == (ZERO3, ZERO3) and b.high_info() == ALL_HIGH
        assert a.operator_info_x() == b.operator_info_x()
        with pytest.raises(GPKError) as e:
            b.operator_info()
        assert e.value.code == _lib.GPK_EINVAL
        with pytest.raises(GPKError) as e:  # the 0..2 range of the derivative predictions stands
            b.predict_deriv(prob["x1"][:3], prob["x2"][:3], prob["x3"][:3], deriv=(3, 0, 0))
        assert e.value.code == _lib.GPK_EINVAL
    finally:
        a.close()
        b.close()


def test_predictions_are_a_legacy_handles_bitwise():
    from gpk.model_GP_solver_3d import DeviceSolver3
    ns = (20, 14, 9)
    op = dict(ALL_OP, faces=63)
    prob, params, fs, _ = _setup(ns, op)
    s = _make(prob, 4, fs, op, high=ALL_HIGH)
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


# ---- 5. the assembly kernel's two new modes alone -------------------------------------------------
W4 = dict(c4=1.5e-3, c3=-2e-2, c2=-0.3, c1=0.8)
JITTER = 1e-6


@pytest.mark.parametrize("Q", [1, 4, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_assemble_pairs4_both_modes(kind, Q):
    """n = 33 (a second, ragged tile row: the mirror path) and 70 (three tile rows).  At c4 = c3 = 0 the
    blocks are gpk_assemble_pairs2's bits.  With all four weights every element of D is within
    sum_n |c_n| (N_n + 2) eps B_n of sum_n c_n Dn, Dn the long-double fields (held to 0.1 units of the
    differentiated kappa by tests/test_operator3h_ref.py) and B_n the absolute-monomial scales
    (tests/mp_fields_high.py; N_2 = N_1 = N_D of tests/field_ulp_inputs.py); pure order-4 and order-3
    blocks within N_4 / N_3; the order-3 block off-diagonal antisymmetric to the bit with an exactly
    zero diagonal, the order-4 block symmetric to the bit."""
    from gpk._lib import assemble_pairs2, assemble_pairs4
    kp = rand_kp(np.random.default_rng(70 + Q), Q, 5.0)
    for n in (33, 70):
        x = np.linspace(0, 1, n) * 2 * np.pi
        K2, D2, D12 = assemble_pairs2(kind, x, kp, JITTER, W4["c2"], W4["c1"])
        for split in (False, True):
            out = assemble_pairs4(kind, x, kp, JITTER, 0.0, 0.0, W4["c2"], W4["c1"], split=split)
            assert np.array_equal(out[0], K2) and np.array_equal(out[1], D2)
            assert not split or np.array_equal(out[2], D12)
        Ld = {o: kernel_block_n(kind, x, x, kp, o, np.longdouble) for o in (1, 2, 3, 4)}
        B = {o: MH.block_scale(kind, o, x, x, kp) for o in (3, 4)}
        B[1], B[2] = (O.field_scale(kind, x, x, kp, o)[1] for o in (1, 2))
        N = {1: N_D, 2: N_D, 3: MH.N_3, 4: MH.N_4}
        K, D, D1 = assemble_pairs4(kind, x, kp, JITTER, split=True, **W4)
        Kp, Dp = assemble_pairs4(kind, x, kp, JITTER, **W4)
        assert np.array_equal(K, K2) and np.array_equal(Kp, K2) and np.array_equal(D1, D12) and np.array_equal(Dp, D)
        assert np.isfinite(D).all()
        want = sum(W4["c%d" % o] * Ld[o] for o in (1, 2, 3, 4))
        bar = sum(abs(W4["c%d" % o]) * (N[o] + MH.N_COMBINE) * B[o] for o in (1, 2, 3, 4))
        u = float(np.max(np.abs(D - want) / (EPS * bar)))
        _, D4 = assemble_pairs4(kind, x, kp, JITTER, 1.0, 0.0, 0.0, 0.0)
        _, D3 = assemble_pairs4(kind, x, kp, JITTER, 0.0, 1.0, 0.0, 0.0)
        u4 = float(np.max(np.abs(D4 - Ld[4]) / (EPS * B[4])))
        u3 = float(np.max(np.where(B[3] > 0, np.abs(D3 - Ld[3]) / (EPS * np.where(B[3] > 0, B[3], 1.0)), 0.0)))
        print(kind, "Q", Q, "n", n, "D %.2f of its bar; D4 %.2f, D3 %.2f (eps B)" % (u, u4, u3))
        assert u <= 1.0 and u4 <= MH.N_4 and u3 <= MH.N_3, (n, u, u4, u3)
        off = ~np.eye(n, dtype=bool)
        assert np.array_equal(D4, D4.T) and np.array_equal(D3[off], -D3.T[off]) and np.all(np.diag(D3) == 0.0)
        assert np.abs(D3).max() > 0.0 and np.abs(D4).max() > 0.0


# ---- 6. loss terms, boundary terms, the criterion -------------------------------------------------
def test_loss_terms_boundary_terms_and_criterion():
    ns = (20, 14, 9)
    dfaces = 0b000011
    op = dict(ALL_OP, faces=0b011100)
    prob, params, fs, dvals = _setup(ns, op, dfaces)
    args = (op, NO_COEF, dfaces, dvals, (1.0, 0.0, 0.0), None, NONE3)
    s = _make(prob, 4, fs, op, NO_COEF, dfaces, dvals, (1.0, 0.0, 0.0), high=ALL_HIGH)
    try:
        s.set_params(params)
        loss, _ = s.loss_grad()
        terms, bt, crit = s.loss_terms(), s.boundary_terms(), s.criterion()
    finally:
        s.close()
    t = {}
    loss_grad_3d_oph(prob, params, *args, ALL_HIGH, terms=t)
    tol = _tol(prob, params)
    cref = criterion_3d_oph(prob, params, *args, ALL_HIGH)
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
    loss_grad_3d_opb(prob, params, *args, terms=t0)
    assert abs(t0["egap"] - terms["egap"]) > 1e-6 * terms["egap"]  # the terms are in egap


# ---- 7. Adam trajectory ---------------------------------------------------------------------------
def test_adam_trajectory_kdv_vs_replay():
    """Ten steps of the KdV form u_t + u u_x + delta u_xxx, under tests/test_gpu_kron3_opx.py's
    trajectory bars."""
    ns = (24, 18, 12)
    op, conv, high = KDV
    prob, params, fs, _ = _setup(ns, op, Q=5, seed=8)
    s = _make(prob, 5, fs, op, conv=conv, high=high)
    try:
        s.set_params(params)
        losses = s.step(10)
        flat = s.get_flat()
    finally:
        s.close()
    ref, p = adam_replay_h(prob, params, op, NO_COEF, 0, None, conv, None, None, high, 10)
    tol = _tol(prob, params)
    print("adam kdv", rel(losses, ref), rel(flat, O.flatten_params(p)), "tol", tol)
    assert rel(losses, ref) < max(1e-9, tol)
    assert rel(flat, O.flatten_params(p)) < max(1e-8, 10 * tol)


# ---- 8. refinement --------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [True, "gemm"])
def test_refined_both_routes(refine):
    """x in [0, 1] at (33, 20, 9): the gates open; the fused route and the two-GEMM route."""
    from gpk import _lib
    ns = (33, 20, 9)
    op, conv, _ = KDV
    info = _run(ns, dict(op, c2=(0.0, -0.05, 0.0)), ((1e-3, 0.0, 0.0), (0.01, 0.0, 0.0)), conv=conv,
                label="refined %r" % refine, refine=refine, unit=True)
    assert info["route"] == (_lib.REFINE_FUSED if refine is True else _lib.REFINE_GEMM)
    assert any(info["open"]), info


# ---- 9. the three configs through the model class -------------------------------------------------
@pytest.mark.parametrize("equation", ["kdv_t-sin", "ks_t-sin", "beam_t-sin"])
def test_train_config_vs_replay(equation):
    """20 epochs at 8^3 with the config's own settings against the replay, as the other operator tests
    run their configs; eq_residual refuses the handle."""
    from gpk.equations import solution_3d_oph
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single, boundary_3d, get_mesh_data, load_config
    from tests.test_gpu_kron3_predict import ref_predict
    cfg = load_config(equation)
    u, src, op, dfaces, _, conv, cross, drift, high = solution_3d_oph(equation)
    xte, ute = get_mesh_data(u, (9,) * 3, 1.0)
    xc, umh = get_mesh_data(u, (8,) * 3, 1.0)
    _, srcv = get_mesh_data(src, (8,) * 3, 1.0)
    bvals = boundary_3d(umh, op.faces)
    tp = {"kernel": kernel_class("Matern52_Cos_1d"), "equation": equation, "llk_weight": cfg["llk_weight"],
          "logdet": cfg["logdet"], "lr": cfg["lr"], "Q": cfg["Q"], "freq_scale": cfg["freq_scale"], "nepoch": 20,
          "tol": -1}
    prob = dict(kind="Matern52_Cos_1d", x1=xc[0], x2=xc[1], x3=xc[2], src=srcv, bvals=bvals, jitter=1e-6,
                llk_weight=float(cfg["llk_weight"]), logdet=float(cfg["logdet"]))
    assert np.isnan(bvals).sum() == 64  # the final-time face is open
    m = GP_solver_3d_single(bvals, xc, srcv, 1e-6, tp, X_test=xte, u_test=ute)
    try:
        assert m.dev.high_info() == (tuple(high[0]), tuple(high[1])) and m.dev.conv_info() == tuple(conv)
        assert m.dev.bdata_info() == (0b011111, dfaces) and m.Nb == (5 + bin(dfaces).count("1")) * 64
        dvals = m.dvals
        log, stop, min_err = m.train(20, verbose=False)
        with pytest.raises(ValueError):
            m.eq_residual(m.params, tuple(xte), np.zeros((9, 9, 9)))
    finally:
        m.dev.close()
    p0 = O.init_params_3d(8, 8, 8, tp["Q"], tp["freq_scale"])
    errs = []

    def after(i, p):
        pr = ref_predict(prob, p, xte)
        errs.append(np.linalg.norm(pr.ravel() - ute.ravel()) / np.linalg.norm(ute.ravel()))
    losses, _ = adam_replay_h(prob, p0, op.as_dict(), NO_COEF, dfaces, dvals, conv, cross, drift, high, 20,
                              lr=tp["lr"], after=after)
    losses = [np.log(lo) if lo > 1 else lo for lo in losses]
    tol = max(1e-8, 10 * _tol(prob, p0))
    print("train", equation, "loss rel", rel(log["loss_list"], losses), "err rel", rel(log["err_list"], errs), "tol", tol)
    assert log["epoch_list"] == list(range(20))
    assert rel(log["loss_list"], losses) < tol
    assert rel(log["err_list"], errs) < tol
    assert min_err == min(log["err_list"]) and not stop["flag"]
