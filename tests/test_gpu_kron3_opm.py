"""Mixed partials on the 3-axis solver (gpk_create3_opm; DeviceSolver3 with cross): m_jk d^2 u /
dx_j dx_k per pair, formed as m D1_k x_k K_k^{-1} x_k D1_j x_j A_j from the order-1 blocks of the
two-block assembly (DERIV_SPLIT), added to the residual by k3_combine_m, and carried back through
the chained adjoints into T_j, G_D1j, G_D1k and G_Kk (build_cross_stages).

Yardstick: tests/operator3m_ref.py loss_grad_3d_opm (pinned on the CPU by
tests/test_operator3m_ref.py).  Tolerance: that of tests/test_gpu_kron3_opn.py, max(1e-10, 50 cond
eps) with the largest cond K_k, on the loss and on every gradient block.  Every bvals / dvals entry
that must not be read is NaN throughout.  Handles without a cross weight are compared with
gpk_create3_opc's bit for bit.
"""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import rel
from tests.operator3c_ref import loss_grad_3d_opc
from tests.operator3m_ref import PAIRS, adam_replay_m, criterion_3d_opm, loss_grad_3d_opm
from tests.test_gpu_kron3 import KINDS, _tol
from tests.test_gpu_kron3_operator import _mask_bvals, _problem
from tests.test_gpu_kron3_opn import ALL_DFACES, ALL_OP
from tests.test_gpu_kron3_opv import FULL, NO_COEF
from tests.test_operator3n_ref import random_dvals
from tests.test_operator3v_ref import smooth_fields

pytestmark = pytest.mark.gpu

NO_CONV = (0.0, 0.0, 0.0)
ALL_CROSS = (0.8, -0.6, 1.1)
# everything at once: ALL_OP's mixed axes 1 and 3, fields on every axis and rho, a reaction, faces
# 0b011011 / dfaces 0b110110, and axis 1 convective as well as the inner axis of (1,2) and (1,3)
# (its T_1 descriptor's dual slot is taken by the convective term)
CONV_1 = (1.0, 0.0, 0.0)
N_CROSS_LAUNCHES = 8  # include/gpk.h: whichever pairs are set


def _make(prob, Q, fs, op, coef, dfaces, dvals, conv, cross, refine=False):
    from gpk.equations import Operator3V
    from gpk.model_GP_solver_3d import DeviceSolver3
    return DeviceSolver3("poisson", prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["bvals"],
                         Q=Q, jitter=prob["jitter"], llk_weight=prob["llk_weight"], logdet=prob["logdet"], lr=0.01,
                         freq_scale=fs, refine=refine,
                         operator=Operator3V(op["c2"], op["c1"], op["react"], op["faces"], a=coef["a"], rho=coef["rho"]),
                         dfaces=dfaces, dvals=dvals, conv=conv, cross=cross)


def _check(label, loss, g, prob, params, op, coef, dfaces, dvals, conv, cross):
    lo, go = loss_grad_3d_opm(prob, params, op, coef, dfaces, dvals, conv, cross)
    tol = _tol(prob, params)
    gd = O.unflatten_params(params, g)
    errs = {k: rel(O.flatten_params(gd[k]), O.flatten_params(go[k])) for k in go}
    errs["loss"] = abs(loss - lo) / abs(lo)
    print(label, "tol %.3e" % tol, {k: "%.3e" % v for k, v in errs.items()})
    assert np.isfinite(loss) and np.all(np.isfinite(g))
    # the term matters: the yardstick without it is another loss
    assert abs(loss_grad_3d_opc(prob, params, op, coef, dfaces, dvals, conv)[0] - lo) > 1e-9 * abs(lo)
    for k, v in errs.items():
        assert v < tol, (label, k, v, tol)


def _setup(ns, op, dfaces, kind="Matern52_Cos_1d", Q=4, seed=3, unit=False):
    prob, params, fs = _problem(ns, kind, Q, seed, unit)
    prob = dict(prob, bvals=_mask_bvals(prob["bvals"], ns, op["faces"]))
    return prob, params, fs, (random_dvals(ns, dfaces, seed=dfaces) if dfaces else None)


def _n_launches(conv):
    return 6 + (2 if any(conv) else 0) + N_CROSS_LAUNCHES


def _run(ns, op, coef, dfaces, conv, cross, kind="Matern52_Cos_1d", Q=4, label="", refine=False, unit=False):
    prob, params, fs, dvals = _setup(ns, op, dfaces, kind, Q, unit=unit)
    s = _make(prob, Q, fs, op, coef, dfaces, dvals, conv, cross, refine=refine)
    try:
        s.set_params(params)
        assert s.cross_info() == tuple(cross) and s.conv_info() == tuple(conv)
        assert s.bdata_info() == (op["faces"], dfaces)
        assert s.operator_info_x().as_dict() == {k: tuple(float(x) for x in v) if k != "faces" else v
                                                 for k, v in op.items()}
        assert len(s.stage_variants()) == _n_launches(conv)
        loss, g = s.loss_grad()
        info = s.refine_info() if refine else None
    finally:
        s.close()
    _check("%s %s %s Q%d cross %s conv %s" % (label, ns, kind, Q, cross, conv), loss, g, prob, params, op, coef,
           dfaces, dvals, conv, cross)
    return info


def _one(pair, m=1.25):
    return tuple(m if t == pair else 0.0 for t in range(3))


# ---- 1. one pair at a time, a 32-tile crossed on its inner axis, then on its outer axis -----------
@pytest.mark.parametrize("pair", [0, 1, 2])
@pytest.mark.parametrize("ns", [(33, 20, 9), (20, 33, 9), (9, 20, 33)])
def test_one_pair_tile_crossing_on_each_axis(ns, pair):
    _run(ns, FULL, NO_COEF, 0, NO_CONV, _one(pair), label="pair %s" % (PAIRS[pair],))


# ---- 2. everything at once -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_everything_at_once_every_kind(kind):
    ns = (33, 33, 9)
    _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=5), ALL_DFACES, CONV_1, ALL_CROSS, kind, label="all")


def test_everything_at_once_q64():
    ns = (33, 33, 9)
    _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=5), ALL_DFACES, CONV_1, ALL_CROSS, Q=64, label="all")


# ---- 3. n = 2 on an axis of a pair ---------------------------------------------------------------
@pytest.mark.parametrize("ns", [(2, 14, 9), (9, 2, 14), (9, 14, 2)])
def test_two_points_on_an_axis_of_a_pair(ns):
    _run(ns, FULL, NO_COEF, 0, NO_CONV, ALL_CROSS, label="n = 2")


# ---- 4. a pair whose axes carry no term of their own ---------------------------------------------
@pytest.mark.parametrize("pair", [0, 1, 2])
def test_pair_on_axes_without_terms_of_their_own(pair):
    """Both axes of the pair have c2 = c1 = 0 (their D blocks are all zeros, their D1 blocks carry
    the cross term alone); the third axis is mixed."""
    j, k = PAIRS[pair]
    third = 3 - j - k
    c2, c1 = [0.0] * 3, [0.0] * 3
    c2[third], c1[third] = -0.3, 0.8
    op = dict(c2=tuple(c2), c1=tuple(c1), react=(0.4, 0.0, 0.2), faces=0b011111)
    _run((20, 33, 9), op, NO_COEF, 0, NO_CONV, _one(pair, -0.9), label="bare pair %s" % (PAIRS[pair],))


# ---- 5. refinement -------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [True, "gemm"])
def test_refined_both_routes(refine):
    """x in [0, 1] at (33, 20, 9): the gates open; H_jk and Zb_jk are refined against their outer
    axis, C_jk reads the refined H_jk and T_j carries Zb_jk before the refinement of X_j reads it."""
    from gpk import _lib
    ns = (33, 20, 9)
    info = _run(ns, ALL_OP, smooth_fields(ns, (0, 1, 2, 3), seed=7), ALL_DFACES, CONV_1, ALL_CROSS,
                label="refined %r" % refine, refine=refine, unit=True)
    assert info["route"] == (_lib.REFINE_FUSED if refine is True else _lib.REFINE_GEMM)
    assert any(info["open"]), info


# ---- 6. loss terms, boundary terms, the criterion and the launch count ---------------------------
def test_loss_terms_boundary_terms_criterion_and_stage_variants():
    ns = (20, 14, 9)
    prob, params, fs, dvals = _setup(ns, ALL_OP, ALL_DFACES)
    coef = smooth_fields(ns, (0, 1, 2, 3), seed=6)
    s = _make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, ALL_CROSS)
    one = _make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, None, _one(2))
    try:
        s.set_params(params)
        loss, _ = s.loss_grad()
        terms, bt, crit = s.loss_terms(), s.boundary_terms(), s.criterion()
        sv, sv1 = s.stage_variants(), one.stage_variants()
    finally:
        s.close()
        one.close()
    # six stages, the convective handle's two, the cross handle's eight whatever the pair set
    assert len(sv) == 6 + 2 + N_CROSS_LAUNCHES and len(sv1) == 6 + N_CROSS_LAUNCHES
    assert all(v in (1, 2, 3) for v in sv + sv1)
    t = {}
    loss_grad_3d_opm(prob, params, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, ALL_CROSS, terms=t)
    tol = _tol(prob, params)
    cref = criterion_3d_opm(prob, params, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, ALL_CROSS)
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
    loss_grad_3d_opm(prob, params, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, None, terms=t0)
    assert abs(t0["egap"] - terms["egap"]) > 1e-6 * terms["egap"]


# ---- 7. bits -------------------------------------------------------------------------------------
def _raw_opm(prob, Q, fs, op, coef, dfaces, dvals, conv, mx):
    """A DeviceSolver3 whose handle comes from gpk_create3_opm called directly with `mx` (None: a
    NULL pointer; else a _lib.gpk_cross3)."""
    from gpk import _lib
    from gpk._lib import dptr
    s = _make(prob, Q, fs, op, coef, dfaces, dvals, conv, None)
    lib = _lib.load()
    _lib.check(lib.gpk_destroy3(s._h))
    s._h = None
    c, h, cf, bd, cv = _lib.gpk_operator3x(), ctypes.c_void_p(), _lib.gpk_coef3(), _lib.gpk_bdata3(), _lib.gpk_conv3()
    c.c2[:], c.c1[:], c.react[:], c.faces = op["c2"], op["c1"], op["react"], op["faces"]
    for k, f in enumerate(getattr(s, "_coef", [None] * 4)[:3]):
        if f is not None:
            cf.a[k] = dptr(f)
    if getattr(s, "_coef", [None] * 4)[3] is not None:
        cf.rho = dptr(s._coef[3])
    if dfaces:
        bd.dfaces, bd.dvals = dfaces, dptr(s._dvals)
    cv.g[:] = conv
    _lib.check(lib.gpk_create3_opm(ctypes.byref(s._prob), ctypes.byref(c), ctypes.byref(cf), ctypes.byref(bd),
                                   ctypes.byref(cv), None if mx is None else ctypes.byref(mx), float(fs),
                                   ctypes.byref(h)))
    s._h = h
    return s


@pytest.mark.parametrize("dfaces,fields,conv", [(0, (), NO_CONV), (ALL_DFACES, (0, 1, 2, 3), (1.0, -0.7, 0.5))])
def test_no_cross_weight_is_the_create3_opc_handle_bitwise(dfaces, fields, conv):
    from gpk import _lib
    ns = (33, 20, 9)
    op = ALL_OP if dfaces else FULL
    prob, params, fs, dvals = _setup(ns, op, dfaces)
    coef = smooth_fields(ns, fields, seed=4)
    hs = [_make(prob, 4, fs, op, coef, dfaces, dvals, conv, None),
          _raw_opm(prob, 4, fs, op, coef, dfaces, dvals, conv, None),
          _raw_opm(prob, 4, fs, op, coef, dfaces, dvals, conv, _lib.gpk_cross3()),
          _make(prob, 4, fs, op, coef, dfaces, dvals, conv, (0.0, 0.0, 0.0))]
    try:
        for s in hs:
            s.set_params(params)
            assert s.cross_info() == (0.0, 0.0, 0.0) and s.conv_info() == conv
            assert s.bdata_info() == (op["faces"], dfaces)
        ref = hs[0].loss_grad()
        assert len(hs[0].stage_variants()) == (8 if any(conv) else 6)
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
    a, b = (_make(prob, 4, fs, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, ALL_CROSS) for _ in range(2))
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
    s = _make(prob, 5, fs, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, ALL_CROSS)
    try:
        s.set_params(params)
        losses = s.step(5)
        flat = s.get_flat()
    finally:
        s.close()
    ref, p = adam_replay_m(prob, params, ALL_OP, coef, ALL_DFACES, dvals, CONV_1, ALL_CROSS, 5)
    tol = _tol(prob, params)
    print("adam opm", rel(losses, ref), rel(flat, O.flatten_params(p)), "tol", tol)
    assert rel(losses, ref) < max(1e-9, tol)
    assert rel(flat, O.flatten_params(p)) < max(1e-8, 10 * tol)


# ---- 9. anisotropic heat through the model class -------------------------------------------------
def _aniso_model(ncol=8, mtest=9):
    from gpk.equations import solution_3d_opm
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single, boundary_3d, get_mesh_data, load_config
    cfg = load_config("aniso_heat_t-sin")
    u, src, op, dfaces, _, conv, cross = solution_3d_opm("aniso_heat_t-sin")
    xte, ute = get_mesh_data(u, (mtest,) * 3, 1.0)
    xc, umh = get_mesh_data(u, (ncol,) * 3, 1.0)
    _, srcv = get_mesh_data(src, (ncol,) * 3, 1.0)
    bvals = boundary_3d(umh, op.faces)
    tp = {"kernel": kernel_class("Matern52_Cos_1d"), "equation": "aniso_heat_t-sin", "llk_weight": cfg["llk_weight"],
          "logdet": cfg["logdet"], "lr": cfg["lr"], "Q": cfg["Q"], "freq_scale": cfg["freq_scale"], "nepoch": 20,
          "tol": -1}
    prob = dict(kind="Matern52_Cos_1d", x1=xc[0], x2=xc[1], x3=xc[2], src=srcv, bvals=bvals, jitter=1e-6,
                llk_weight=float(cfg["llk_weight"]), logdet=float(cfg["logdet"]))

    def make():
        return GP_solver_3d_single(bvals, xc, srcv, 1e-6, tp, X_test=xte, u_test=ute)
    return prob, op, conv, cross, tp, xte, ute, make


def test_train_aniso_heat_vs_replay_and_resume(tmp_path):
    from tests.test_gpu_kron3_predict import ref_predict
    prob, op, conv, cross, tp, xte, ute, make = _aniso_model()
    assert np.isnan(prob["bvals"]).sum() == 64  # the final-time face is open
    m = make()
    try:
        assert m.Nb == 5 * 64 and m.dev.operator_info_x() == op
        assert m.dev.cross_info() == cross == (-0.08, 0.0, 0.0) and m.dev.conv_info() == conv == NO_CONV
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
    losses, _ = adam_replay_m(prob, p0, op.as_dict(), NO_COEF, 0, None, conv, cross, 20, lr=tp["lr"], after=after)
    losses = [np.log(lo) if lo > 1 else lo for lo in losses]
    tol = max(1e-8, 10 * _tol(prob, p0))
    print("train aniso_heat_t loss rel", rel(log["loss_list"], losses), "err rel", rel(log["err_list"], errs), "tol", tol)
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
        assert m2.dev.cross_info() == (-0.08, 0.0, 0.0)  # cross comes back from the equation's name
        assert np.array_equal(m2.dev.get_flat(), flat)
    finally:
        m2.dev.close()
    assert min2 == min_err and sorted(log2) == sorted(log)
    for k in log:
        assert np.array_equal(np.asarray(log2[k]), np.asarray(log[k])), k


@pytest.mark.parametrize("equation", ["aniso_heat_t-sin", "aniso_3d-sin"])
def test_eq_residual_opm(equation):
    """eq_residual on a 7 x 6 x 5 test grid against NumPy on the reference predictions, at the bar
    of tests/test_gpu_eq_residual.py (the project's bar scaled by the largest term; a cross term is
    one prediction with a derivative on each of two axes)."""
    from gpk.equations import solution_3d_opm
    from gpk.kernel_matrix import kernel_class
    from gpk.model_GP_solver_3d import GP_solver_3d_single
    from tests import predict_deriv_ref as R
    _, _, op, _, _, conv, cross = solution_3d_opm(equation)
    ns, ms = (20, 14, 9), (7, 6, 5)
    prob, params, fs = _problem(ns)
    tp = {"kernel": kernel_class(prob["kind"]), "llk_weight": prob["llk_weight"], "Q": 4, "lr": 0.01,
          "freq_scale": fs, "logdet": True, "equation": equation}
    m = GP_solver_3d_single(_mask_bvals(prob["bvals"], ns, op.faces), (prob["x1"], prob["x2"], prob["x3"]),
                            prob["src"], prob["jitter"], tp)
    xte = R.grid_axes(prob, params, ms)
    src = np.random.default_rng(2).normal(size=ms)
    try:
        assert m.dev.operator_info_x() == op and m.dev.cross_info() == cross and m.dev.conv_info() == conv
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
    ncross = 0
    for (j, k), mjk in zip(PAIRS, cross):
        if mjk != 0.0:
            d = [0, 0, 0]
            d[j] = d[k] = 1
            terms.append(mjk * R.ref_grid(prob, params, xte, d))
            ncross += 1
    assert not any(conv) and ncross == {"aniso_heat_t-sin": 1, "aniso_3d-sin": 3}[equation] and len(terms) == ncross + 3
    expect = sum(terms) - src
    tol = R.bar(prob, params)
    scale = max([float(np.max(np.abs(t))) for t in terms] + [float(np.max(np.abs(src)))])
    err = float(np.max(np.abs(res - expect)))
    print("eq_residual", equation, "err / scale", err / scale, "tol", tol)
    assert res.shape == ms
    assert err < tol * scale
