"""Mixed fourth-order partials on the 3-axis solver (gpk_create3_opq; DeviceSolver3 with bicross=): a
pair (j, k) of weight q adds q d^4u/dx_j^2 dx_k^2 through the cross pairs' stages with the plain order-2
block DD for D1; both axes assemble and contract in DERIV_HIGH_D2 (DERIV_HIGH_SPLIT_D2 where the axis
also owns D1_k), and k3_combine_q sums R.

Yardstick: tests/operator3q_ref.py loss_grad_3d_opq (pinned on the CPU by tests/test_operator3q_ref.py
against torch autograd of the dense-Kronecker form).  Tolerance: the project's _tol of
tests/test_gpu_kron3.py, max(1e-10, 50 cond eps) with the largest cond K_k, on the loss and on every
gradient block; tests/test_operator3q_host.py holds the yardstick's own fp64 rounding of the chained
u_jjkk term on these problems to a tenth of that bar.  The weights are sized so that q om^4 ~ c2 om^2
at problem_3d's defaults (om up to 2 pi 5): |q| ~ 1e-3.  Every bvals / dvals entry that must not be
read is NaN.  Each case asserts that the yardstick without bicross moves some checked quantity by
over 100 tolerances.  Handles without a bi-pair are compared with gpk_create3_oph's bit for bit,
predictions with a legacy handle's.
"""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import rand_kp, rel
from tests.operator3h_ref import loss_grad_3d_oph
from tests.operator3m_ref import PAIRS
from tests.operator3q_ref import adam_replay_q, criterion_3d_opq, loss_grad_3d_opq
from tests.test_gpu_kron3 import KINDS, _tol
from tests.test_gpu_kron3_operator import _mask_bvals, _problem
from tests.test_gpu_kron3_opb import drift_for
from tests.test_gpu_kron3_opv import NO_COEF
from tests.test_operator3n_ref import random_dvals
from tests.test_operator3v_ref import smooth_fields

pytestmark = pytest.mark.gpu

ZERO3 = (0.0, 0.0, 0.0)
NONE3 = (None, None, None)
PLAIN = dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, 0.0, 1.0), react=ZERO3, faces=63)
Q1 = 1.5e-3
# everything at once on (33, 33, 9): axes 1-2 share their launch
ALL_OP = dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, -0.6, 1.3), react=(0.4, -0.5, 0.2), faces=0b011011)
ALL_HIGH = ((2e-3, -1e-3, 1.5e-3), (-3e-2, 2e-2, 4e-2))
ALL_BQ = (1.5e-3, -1e-3, 2e-3)
ALL_DFACES = 0b110110
ALL_KW = dict(conv=(1.0, 0.0, 0.0), cross=(0.8, 0.0, 0.0))
# the plate form: u_tt + kappa (u_xxxx + 2 u_xxyy + u_yyyy)
PLATE = (dict(c2=(0.0, 0.0, 1.0), c1=ZERO3, react=ZERO3, faces=0b011111), ((1e-3, 1e-3, 0.0), ZERO3), (2e-3, 0.0, 0.0))


def _make(prob, Q, fs, op, coef=NO_COEF, dfaces=0, dvals=None, conv=None, cross=None, drift=None, high=None,
          bicross=None, refine=False):
    from gpk.equations import Operator3V
    from gpk.model_GP_solver_3d import DeviceSolver3
    return DeviceSolver3("poisson", prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                         Q=Q, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"], lr=0.01,
                         freq_scale=fs, refine=refine,
                         operator=Operator3V(op["c2"], op["c1"], op["react"], op["faces"], a=coef["a"], rho=coef["rho"]),
                         dfaces=dfaces, dvals=dvals, conv=conv, cross=cross, drift=drift, high=high, bicross=bicross)


def _check(label, loss, g, prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, bq):
    lo, go = loss_grad_3d_opq(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, bq)
    tol = _tol(prob, params)
    gd = O.unflatten_params(params, g)
    errs = {k: rel(O.flatten_params(gd[k]), O.flatten_params(go[k])) for k in go}
    errs["loss"] = abs(loss - lo) / abs(lo)
    print(label, "tol %.3e" % tol, {k: "%.3e" % v for k, v in errs.items()})
    assert np.isfinite(loss) and np.all(np.isfinite(g))
    # the pairs matter: the yardstick without them moves some checked quantity by over 100 tol
    lo0, go0 = loss_grad_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high)
    moved = {k: rel(O.flatten_params(go0[k]), O.flatten_params(go[k])) for k in go}
    moved["loss"] = abs(lo0 - lo) / abs(lo)
    assert lo0 != lo and max(moved.values()) > 100 * tol, (lo0, lo, moved, tol)
    for k, v in errs.items():
        assert v < tol, (label, k, v, tol)


def _setup(ns, op, dfaces=0, kind="Matern52_Cos_1d", Q=4, seed=3, unit=False):
    prob, params, fs = _problem(ns, kind, Q, seed, unit)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    return prob, params, fs, (random_dvals(ns, dfaces, seed=dfaces) if dfaces else None)


def _run(ns, op, bq, high=None, coef=NO_COEF, dfaces=0, conv=None, cross=None, drift=None, kind="Matern52_Cos_1d",
         Q=4, label="", refine=False, unit=False):
    prob, params, fs, dvals = _setup(ns, op, dfaces, kind, Q, unit=unit)
    s = _make(prob, Q, fs, op, coef, dfaces, dvals, conv, cross, drift, high, bq, refine)
    try:
        s.set_params(params)
        assert np.array_equal(s.get_flat(), O.flatten_params(params))
        assert s.bicross_info() == tuple(bq)
        loss, g = s.loss_grad()
        info = s.refine_info() if refine else None
    finally:
        s.close()
    _check("%s %s %s Q%d bq %s" % (label, ns, kind, Q, bq), loss, g, prob, params, op, coef, dfaces, dvals,
           conv, cross, drift or NONE3, high, bq)
    return info


def _one(pair, q=Q1):
    return tuple(q if t == pair else 0.0 for t in range(3))


# ---- 1. each pair alone, the 32-tile crossed on each axis -----------------------------------------
@pytest.mark.parametrize("ns", [(33, 20, 9), (20, 33, 9), (9, 20, 33)])
@pytest.mark.parametrize("pair", [0, 1, 2])
def test_one_pair_tile_crossing_on_each_axis(ns, pair):
    _run(ns, PLAIN, _one(pair), label="pair %d" % pair)


# ---- 2. everything at once ------------------------------------------------------------------------
def _everything(kind, Q):
    ns = (33, 33, 9)
    _run(ns, ALL_OP, ALL_BQ, ALL_HIGH, coef=smooth_fields(ns, (0, 1, 3), seed=5), dfaces=ALL_DFACES,
         drift=drift_for(ns, (0, 2)), kind=kind, Q=Q, label="everything", **ALL_KW)


@pytest.mark.parametrize("kind", KINDS)
def test_everything_at_once_every_kind(kind):
    """All three bi-pairs over all four orders on every axis, fields a_1, a_2 and rho, a reaction, a
    convective axis, a cross pair on the same axes, drift fields, faces 0b011011 and derivative faces
    0b110110: the D + D1 + DD mode on axes 1-2 (one shared launch) and on axis 3."""
    _everything(kind, 4)


def test_everything_at_once_q64():
    _everything("Matern52_Cos_1d", 64)


def test_both_modes_in_separate_launches():
    """Axis 1 convective (D + D1 + DD), axis 2 without D1 (D + DD): axes 1-2 launch apart."""
    _run((33, 20, 9), PLAIN, (Q1, 0.0, -1e-3), conv=(1.0, 0.0, 0.0), label="modes apart")


# ---- 3. n = 2 on an axis of a pair, and pairs whose axes have nothing else ------------------------
@pytest.mark.parametrize("ns", [(2, 14, 9), (9, 2, 14), (9, 14, 2)])
def test_two_points_on_an_axis_of_a_pair(ns):
    _run(ns, PLAIN, (Q1, -1e-3, 2e-3), label="n = 2")


@pytest.mark.parametrize("pair", [0, 1, 2])
def test_pair_on_axes_without_terms_of_their_own(pair):
    j, k = PAIRS[pair]
    other = 3 - j - k
    c2 = tuple(1.0 if a == other else 0.0 for a in range(3))
    _run((20, 14, 9), dict(c2=c2, c1=ZERO3, react=ZERO3, faces=63), _one(pair), label="bare pair %d" % pair)


# ---- 4. refinement --------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [True, "gemm"])
def test_refined_both_routes(refine):
    """x in [0, 1] at (33, 20, 9): the gates open; the fused route and the two-GEMM route, all three
    pairs (both solves of each refined)."""
    from gpk import _lib
    info = _run((33, 20, 9), dict(PLAIN, c2=(-0.05, 0.05, -0.02)), (1e-3, -1e-3, 2e-3), label="refined %r" % refine,
                refine=refine, unit=True)
    assert info["route"] == (_lib.REFINE_FUSED if refine is True else _lib.REFINE_GEMM)
    assert any(info["open"]), info


# ---- 5. loss terms, boundary terms, criterion, stage variants -------------------------------------
def test_loss_terms_boundary_terms_criterion_and_stage_variants():
    ns = (20, 14, 9)
    dfaces = 0b000011
    op = dict(ALL_OP, faces=0b011100)
    prob, params, fs, dvals = _setup(ns, op, dfaces)
    args = (op, NO_COEF, dfaces, dvals, (1.0, 0.0, 0.0), None, NONE3, ALL_HIGH)
    s = _make(prob, 4, fs, op, NO_COEF, dfaces, dvals, (1.0, 0.0, 0.0), high=ALL_HIGH, bicross=ALL_BQ)
    base = _make(prob, 4, fs, op, NO_COEF, dfaces, dvals, (1.0, 0.0, 0.0), high=ALL_HIGH)
    both = _make(prob, 4, fs, op, NO_COEF, dfaces, dvals, (1.0, 0.0, 0.0), cross=(0.8, 0.0, 0.0), high=ALL_HIGH,
                 bicross=_one(2))
    try:
        s.set_params(params)
        loss, _ = s.loss_grad()
        terms, bt, crit = s.loss_terms(), s.boundary_terms(), s.criterion()
        nb, nq, nx = len(base.stage_variants()), len(s.stage_variants()), len(both.stage_variants())
        assert base.bicross_info() == ZERO3 and both.bicross_info() == _one(2)
    finally:
        for h in (s, base, both):
            h.close()
    assert nq == nb + 8 and nx == nb + 16, (nb, nq, nx)
    t = {}
    loss_grad_3d_opq(prob, params, *args, ALL_BQ, terms=t)
    tol = _tol(prob, params)
    cref = criterion_3d_opq(prob, params, *args, ALL_BQ)
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
    loss_grad_3d_oph(prob, params, *args, terms=t0)
    assert abs(t0["egap"] - terms["egap"]) > 1e-6 * terms["egap"]  # the pairs are in egap


# ---- 6. bits --------------------------------------------------------------------------------------
def _raw_opq(prob, Q, fs, op, conv, cross, high, bq):
    """A DeviceSolver3 whose handle comes from gpk_create3_opq called directly with `bq` (None: a NULL
    pointer; else a _lib.gpk_bicross3)."""
    from gpk import _lib
    s = _make(prob, Q, fs, op, conv=conv, cross=cross)
    lib = _lib.load()
    _lib.check(lib.gpk_destroy3(s._h))
    s._h = None
    c, h = _lib.gpk_operator3x(), ctypes.c_void_p()
    cv, mx, hi = _lib.gpk_conv3(), _lib.gpk_cross3(), _lib.gpk_high3()
    c.c2[:], c.c1[:], c.react[:], c.faces = op["c2"], op["c1"], op["react"], op["faces"]
    cv.g[:] = conv
    mx.m[:] = cross
    hi.c4[:], hi.c3[:] = high
    _lib.check(lib.gpk_create3_opq(ctypes.byref(s._prob), ctypes.byref(c), None, None, ctypes.byref(cv),
                                   ctypes.byref(mx), None, ctypes.byref(hi), None if bq is None else ctypes.byref(bq),
                                   float(fs), ctypes.byref(h)))
    s._h = h
    return s


@pytest.mark.parametrize("conv,cross,high", [(ZERO3, ZERO3, (ZERO3, ZERO3)),
                                             ((1.0, -0.7, 0.5), (0.8, -0.6, 1.1), ALL_HIGH)])
def test_no_bicross_weight_is_the_create3_oph_handle_bitwise(conv, cross, high):
    from gpk import _lib
    ns = (33, 20, 9)
    op = dict(ALL_OP, faces=0b011111)
    prob, params, fs, _ = _setup(ns, op)
    hs = [_make(prob, 4, fs, op, conv=conv, cross=cross, high=high),
          _raw_opq(prob, 4, fs, op, conv, cross, high, None),
          _raw_opq(prob, 4, fs, op, conv, cross, high, _lib.gpk_bicross3()),
          _make(prob, 4, fs, op, conv=conv, cross=cross, high=high, bicross=ZERO3)]
    try:
        for s in hs:
            s.set_params(params)
            assert s.bicross_info() == ZERO3
            assert s.cross_info() == cross and s.conv_info() == conv and s.high_info() == high
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
    a, b = (_make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, high=ALL_HIGH, bicross=ALL_BQ, **ALL_KW)
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
    s = _make(prob, 4, fs, op, high=ALL_HIGH, bicross=ALL_BQ)
    legacy = DeviceSolver3("poisson", prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                           Q=4, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"], lr=0.01,
                           freq_scale=fs)
    xte = [np.linspace(x[0], x[-1], m) for x, m in zip((prob["x1"], prob["x2"], prob["x3"]), (7, 6, 5))]
    pts = np.random.default_rng(1).uniform(0.0, 1.0, size=(11, 3)) * [x[-1] for x in xte]
    try:
        for h in (s, legacy):
            h.set_params(params)
        assert np.array_equal(s.predict(*xte), legacy.predict(*xte))
        assert np.array_equal(s.predict_deriv(*xte, deriv=(2, 0, 2)), legacy.predict_deriv(*xte, deriv=(2, 0, 2)))
        assert np.array_equal(s.evaluate(pts, (0, 1, 0)), legacy.evaluate(pts, (0, 1, 0)))
    finally:
        s.close()
        legacy.close()


# ---- 7. the assembly kernel's two new modes alone -------------------------------------------------
W4 = dict(c4=1.5e-3, c3=-2e-2, c2=-0.3, c1=0.8)
JITTER = 1e-6


@pytest.mark.parametrize("Q", [1, 4, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_assemble_pairs5_both_modes(kind, Q):
    """n = 33 (a second, ragged tile row: the mirror path) and 70 (three tile rows): K, D and D1 are
    gpk_assemble_pairs4's bits at the same weights (c4 = c3 = 0 included); D2 is the bits of its D at
    (c4, c3, c2, c1) = (0, 0, 1, 0), symmetric to the bit."""
    from gpk._lib import assemble_pairs4, assemble_pairs5
    kp = rand_kp(np.random.default_rng(70 + Q), Q, 5.0)
    for n in (33, 70):
        x = np.linspace(0, 1, n) * 2 * np.pi
        _, DD = assemble_pairs4(kind, x, kp, JITTER, 0.0, 0.0, 1.0, 0.0)
        for w in (W4, dict(W4, c4=0.0, c3=0.0)):
            K4, D4, D14 = assemble_pairs4(kind, x, kp, JITTER, split=True, **w)
            K, D, D1, D2 = assemble_pairs5(kind, x, kp, JITTER, split=True, **w)
            Kp, Dp, D2p = assemble_pairs5(kind, x, kp, JITTER, **w)
            assert np.array_equal(K, K4) and np.array_equal(D, D4) and np.array_equal(D1, D14)
            assert np.array_equal(Kp, K4) and np.array_equal(Dp, D4)
            for d2 in (D2, D2p):
                assert np.array_equal(d2, DD) and np.array_equal(d2, d2.T) and np.abs(d2).max() > 0.0


def test_order_2_block_has_zero_pads_through_the_step():
    """The pads of DD are zero: a handle at n = 33 (31 pad rows and columns per axis of a pair) gives the
    yardstick's loss, which a non-zero pad would enter through Z2_j (covered by every n = 33 case above);
    here the same at n = 2, where 30 of 32 rows are pads."""
    _run((2, 2, 9), PLAIN, _one(0), label="pads")


# ---- 8. Adam trajectory ---------------------------------------------------------------------------
def test_adam_trajectory_plate_vs_replay():
    """Ten steps of the plate form, under tests/test_gpu_kron3_opx.py's trajectory bars."""
    ns = (24, 18, 12)
    op, high, bq = PLATE
    prob, params, fs, _ = _setup(ns, op, Q=5, seed=8)
    s = _make(prob, 5, fs, op, high=high, bicross=bq)
    try:
        s.set_params(params)
        losses = s.step(10)
        flat = s.get_flat()
    finally:
        s.close()
    ref, p = adam_replay_q(prob, params, op, NO_COEF, 0, None, None, None, None, high, bq, 10)
    tol = _tol(prob, params)
    print("adam plate", rel(losses, ref), rel(flat, O.flatten_params(p)), "tol", tol)
    assert rel(losses, ref) < max(1e-9, tol)
    assert rel(flat, O.flatten_params(p)) < max(1e-8, 10 * tol)


# ---- 9. the four configs through the model class --------------------------------------------------
def _model(equation):
    from gpk.equations import solution_3d_opq
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single, boundary_3d, get_mesh_data, load_config
    cfg = load_config(equation)
    sol = solution_3d_opq(equation)
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


EXPECT = {"plate_t-sin": (0b011111, 0b011111), "biharmonic_3d-sin": (63, 63),
          "swift_hohenberg_t-sin": (0b011111, 0b001111), "mixed4_3d-sin": (63, 0)}


@pytest.mark.parametrize("equation", list(EXPECT))
def test_train_config_vs_replay(equation, tmp_path):
    """20 epochs at 8^3 with the config's own settings against the replay; the plate also through
    checkpoint / resume; eq_residual refuses a handle with high-order terms."""
    from tests.test_gpu_kron3_predict import ref_predict
    prob, sol, tp, xte, ute, make = _model(equation)
    _, _, op, dfaces, _, conv, cross, drift, high, bq = sol
    faces, dexp = EXPECT[equation]
    assert op.faces == faces and dfaces == dexp
    assert np.isnan(prob["bvals"]).sum() == (64 if faces != 63 else 0)
    m = make()
    try:
        assert m.dev.bicross_info() == tuple(bq) and m.dev.high_info() == (tuple(high[0]), tuple(high[1]))
        assert m.dev.bdata_info() == (faces, dfaces)
        assert m.Nb == (bin(faces).count("1") + bin(dfaces).count("1")) * 64
        dvals = m.dvals
        log, stop, min_err = m.train(20, verbose=False)
        flat = m.dev.get_flat()
        if any(c != 0.0 for t in high for c in t):
            with pytest.raises(ValueError):
                m.eq_residual(m.params, tuple(xte), np.zeros((9, 9, 9)))
    finally:
        m.dev.close()
    p0 = O.init_params_3d(8, 8, 8, tp["Q"], tp["freq_scale"])
    errs = []

    def after(i, p):
        pr = ref_predict(prob, p, xte)
        errs.append(np.linalg.norm(pr.ravel() - ute.ravel()) / np.linalg.norm(ute.ravel()))
    losses, _ = adam_replay_q(prob, p0, op.as_dict(), NO_COEF, dfaces, dvals, conv, cross, drift, high, bq, 20,
                              lr=tp["lr"], after=after)
    losses = [np.log(lo) if lo > 1 else lo for lo in losses]
    tol = max(1e-8, 10 * _tol(prob, p0))
    print("train", equation, "loss rel", rel(log["loss_list"], losses), "err rel", rel(log["err_list"], errs), "tol", tol)
    assert log["epoch_list"] == list(range(20))
    assert rel(log["loss_list"], losses) < tol
    assert rel(log["err_list"], errs) < tol
    assert min_err == min(log["err_list"]) and not stop["flag"]
    if equation != "plate_t-sin":
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
        assert m2.dev.bicross_info() == tuple(bq)  # bicross comes back from the equation's name
        assert np.array_equal(m2.dev.get_flat(), flat)
    finally:
        m2.dev.close()
    assert min2 == min_err and sorted(log2) == sorted(log)
    for k in log:
        assert np.array_equal(np.asarray(log2[k]), np.asarray(log[k])), k


def test_eq_residual_mixed4():
    """eq_residual of mixed4_3d-sin on a 7 x 6 x 5 test grid against NumPy on the reference predictions,
    at the bar of tests/test_gpu_kron3_opm.py's eq_residual test (the project's bar scaled by the
    largest term; a bi-pair term is one prediction with two derivatives on each of two axes)."""
    from gpk.equations import solution_3d_opq
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single
    from tests import predict_deriv_ref as R
    equation = "mixed4_3d-sin"
    op, bq = solution_3d_opq(equation)[2], solution_3d_opq(equation)[9]
    ns, ms = (20, 14, 9), (7, 6, 5)
    prob, params, fs = _problem(ns)
    tp = {"kernel": kernel_class(prob["kind"]), "llk_weight": prob["llk_weight"], "Q": 4, "lr": 0.01,
          "freq_scale": fs, "logdet": True, "equation": equation}
    m = GP_solver_3d_single(_mask_bvals(prob["bvals"], ns, op.faces), (prob["x1"], prob["x2"], prob["x3"]),
                            prob["src"], prob["jitter"], tp)
    xte = R.grid_axes(prob, params, ms)
    src = np.random.default_rng(2).normal(size=ms)
    try:
        assert m.dev.operator_info_x() == op and m.dev.bicross_info() == tuple(bq) == (0.01, 0.01, 0.01)
        res = m.eq_residual(params, tuple(xte), src)
    finally:
        m.dev.close()
    terms = []
    for k in range(3):
        d = [0, 0, 0]
        d[k] = 2
        terms.append(op.c2[k] * R.ref_grid(prob, params, xte, d))
    for (j, k), q in zip(PAIRS, bq):
        d = [0, 0, 0]
        d[j] = d[k] = 2
        terms.append(q * R.ref_grid(prob, params, xte, d))
    assert len(terms) == 6
    expect = sum(terms) - src
    tol = R.bar(prob, params)
    scale = max([float(np.max(np.abs(t))) for t in terms] + [float(np.max(np.abs(src)))])
    err = float(np.max(np.abs(res - expect)))
    print("eq_residual", equation, "err / scale", err / scale, "tol", tol)
    assert res.shape == ms
    assert err < tol * scale
