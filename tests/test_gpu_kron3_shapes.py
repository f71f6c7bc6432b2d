"""3-axis step (gpk_create3 / gpk_loss_grad3 / gpk_step3) where the three padded sizes differ,
against the long-double yardstick.

Every other 3-axis test steps a grid whose padded sizes are all 32: there a swap of two axes'
strides (K3Geom::at / atp, the GEMM leading dimensions, k3_permute, k3_combine, k3_adam_u), the
inverse's output-buffer parity (T = P / 32 sweeps, T even), the log-det accumulation over T > 1
sweeps and every GEMM kernel but the 16x16 one go unseen.  Here: three distinct P in all three
rotations, n = 2 / n = P / n = P + 1 on every axis, two grids whose stages leave the 16x16
kernel (asserted through DeviceSolver3.stage_variants), Q = 1 and Q = 64, n = 1024.

Yardstick: oracle.gp_oracle.loss_grad_3d under set_extended(True) (80-bit LU solves and
log-dets, exact K and D fields, exact parameter contraction).  Bar, per key (loss, U,
kernel_paras_1..3, log_tau, log_v and the seven loss terms; tests.helpers.rel, max-abs error
over max-abs value):
    min(_tol, max(FLOOR, MULT x |fp64 LU oracle - yardstick|))
with FLOOR 1e-12 and MULT 2 as tests/test_gpu_accuracy.py, _tol the fp64 bar of
tests/test_gpu_kron3.py.  test_lu_oracle_distance_from_yardstick (CPU) keeps the LU oracle's
distance below 1e-8 on every case, so the bar is never vacuous.  Every measured device error,
LU distance and bar goes to the parity log (tests.helpers.record_parity).

MULT above 2 (MI355X; the largest measured device / LU ratio of the key beside it, MULT = 1.5 x
that ratio rounded up to one digit):
    log_v, term_egap       268.7   ("huge-stages0-4")          -> 500
    U                       11.53  ("huge-stages0-4")          -> 20
    kernel_paras_1           6.75  ("Q64-cos")                 -> 20
    kernel_paras_3           6.51  ("Q64-cos")                 -> 10
    term_logdet_1            6.25  ("T321")                    -> 10
    loss, term_loss          4.75  ("Q64-cos")                 -> 8
    term_quad                3.52  ("huge-stages0-4")          -> 6
    term_logdet_2            2.97  ("edge-2-P-P1")             -> 5
Why these are the algorithm's and no layout's.  Every excess is on the four Allen-Cahn cases
(x in [0, 1]: cond(K) 5e6 - 1e8, with a factor of more than one 32-block) and stays below
0.2 cond eps; every Poisson case (cond(K) <= 2e7), at the same padded sizes, rotations and GEMM
kernels -- "huge-stages0-4-wellcond" was added for the 128x128 kernel's stages -- is within 1.3 x
LU above the floor.  The 3-axis step applies K_k^{-1} as an explicit inverse from 32-wide
Cholesky-Gauss-Jordan sweeps with no refinement step (Refinement: such a
product's error is unstructured, the residual's D_k amplifies it, and log_v's
-N/2 + v ||R||^2 / 2 shows it first: 28.8 x LU in the unrefined 2-axis C5).  An fp64 NumPy
emulation of exactly that (tools/kron3_sweep_emulation.py: no layout in it) is off the yardstick
by the same factors: U 7.0 / 7.9 / 10.1 / 4.8 x LU at T321 / edge-2-P-P1 / huge-stages0-4 /
Q64-cos against the device's 7.5 / 5.7 / 11.5 / 7.5, log_v 83.9 x at huge-stages0-4 (device
268.7; 0.05 and 0.16 cond eps, the LU oracle's 2.8e-12 there is 6e-4 cond eps), kernel_paras_3
6.5 x at Q64-cos (6.5); with one Cholesky of the whole factor instead (--inverse potri) U is
within 2 x LU at all four and log_v 10 x at huge-stages0-4.  On the device, Allen-Cahn at
all-32 padded sizes (one pivot block, no sweep; (20,14,9) and (30,31,32), all four kernels) is
within 2 x LU on U and 4.2 x on log_v.
The bar is never looser than _tol.
"""
import functools

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import problem_3d, record_parity, rel
from tests.test_gpu_kron3 import _solver, _tol

gpu = pytest.mark.gpu

FLOOR = 1e-12
MULT = {"log_v": 500.0, "term_egap": 500.0, "U": 20.0, "kernel_paras_1": 20.0, "kernel_paras_3": 10.0,
        "term_logdet_1": 10.0, "loss": 8.0, "term_loss": 8.0, "term_quad": 6.0,
        "term_logdet_2": 5.0}  # per key; 2 unless named here (module docstring)
TERMS = ("loss", "logdet_1", "logdet_2", "logdet_3", "quad", "egap", "bgap")
S, H = 1, 3  # gpk._lib.GEMM_SMALL, GEMM_TILE128 (the 16x16 and the 128x128 kernel)

# (eq, kind, ns, Q) -> padded sizes, the GEMM kernel of each of the six stages
CASES = {
    "T213": (("poisson", "Matern52_Cos_1d", (33, 9, 70), 4), (64, 32, 96), [S] * 6),
    "T321": (("allencahn", "Matern52_1d", (70, 33, 9), 4), (96, 64, 32), [S] * 6),
    "T132": (("poisson", "SE_Cos_1d", (9, 70, 33), 4), (32, 96, 64), [S] * 6),
    "edge-2-P-P1": (("allencahn", "SE_1d", (2, 64, 33), 4), (32, 64, 64), [S] * 6),
    "edge-P-2-P1": (("poisson", "Matern52_Cos_1d", (32, 2, 65), 4), (32, 32, 96), [S] * 6),
    "edge-P1-P-2": (("poisson", "SE_Cos_1d", (65, 32, 2), 4), (96, 32, 32), [S] * 6),
    # stage 2: 4 x 4608 = 18432 16x16 tiles (> 16384), 360 128x128 tiles; stage 3: 13888
    "huge-stage2": (("poisson", "Matern52_Cos_1d", (100, 70, 90), 4), (128, 96, 96), [S, S, H, S, S, S]),
    "huge-stages0-4": (("allencahn", "Matern52_Cos_1d", (97, 128, 130), 4), (128, 128, 160), [H] * 5 + [S]),
    # the same grid on x in [0, 2 pi]: cond(K) ~ 1e5, so the 128x128 kernel's stages are held to ~1e-11
    "huge-stages0-4-wellcond": (("poisson", "Matern52_Cos_1d", (97, 128, 130), 4), (128, 128, 160), [H] * 5 + [S]),
}
# Q = 1 and Q = 64 (k3_prep / k3_finalize loops, the pg[a*3*QMAX + ty*QMAX + cq] index); SE_1d
# has no cosine factor: its frequency gradient is zeroed (has_cos)
Q_CASES = {
    "Q1": (("poisson", "Matern52_Cos_1d", (9, 33, 5), 1), (32, 64, 32), [S] * 6),
    "Q64-cos": (("allencahn", "SE_Cos_1d", (9, 33, 5), 64), (32, 64, 32), [S] * 6),
    "Q64-nocos": (("poisson", "SE_1d", (9, 33, 5), 64), (32, 64, 32), [S] * 6),
}
ALL_CASES = {**CASES, **Q_CASES}
STATE = CASES["T213"][0]


def _distances(got, ref):
    """Per-key distance of (loss, gradient tree, terms) from ref's."""
    out = {"loss": abs(got[0] - ref[0]) / abs(ref[0])}
    for k in ref[1]:
        out[k] = rel(O.flatten_params(got[1][k]), O.flatten_params(ref[1][k]))
    for t in TERMS:
        out["term_" + t] = rel(got[2][t], ref[2][t])
    return out


@functools.lru_cache(maxsize=None)
def _reference(eq, kind, ns, Q):
    """The case's problem and seeded params, the yardstick, the fp64 LU oracle's distance from
    it per key, and the fp64 bar _tol.  Computed once per session; read-only."""
    prob, params, fs = problem_3d(eq=eq, kind=kind, ns=ns, Q=Q, seed=3)
    res = {}
    for mode in (True, False):
        O.set_extended(mode)
        try:
            terms = {}
            loss, grad = O.loss_grad_3d(prob, params, terms=terms)
        finally:
            O.set_extended(False)
        res[mode] = (loss, grad, terms)
    return {"prob": prob, "params": params, "fs": fs, "ext": res[True],
            "lu_err": _distances(res[False], res[True]), "tol": _tol(prob, params)}


def _bars(ref):
    return {k: min(ref["tol"], max(FLOOR, MULT.get(k, 2.0) * d)) for k, d in ref["lu_err"].items()}


@pytest.mark.parametrize("case", list(ALL_CASES))
def test_lu_oracle_distance_from_yardstick(case):
    """The bar's reference term is meaningful: on every case the fp64 LU oracle is within 1e-8
    of the yardstick on every key, and the table's padded sizes are the cases' own."""
    (eq, kind, ns, Q), P, _ = ALL_CASES[case]
    assert tuple(-(-n // 32) * 32 for n in ns) == P
    ref = _reference(eq, kind, ns, Q)
    print(case, {k: f"{v:.2e}" for k, v in ref["lu_err"].items()})
    assert set(ref["lu_err"]) == {"loss", "U", "kernel_paras_1", "kernel_paras_2", "kernel_paras_3",
                                  "log_tau", "log_v"} | {"term_" + t for t in TERMS}
    for k, d in ref["lu_err"].items():
        assert d <= 1e-8, (case, k, d)


@gpu
@pytest.mark.parametrize("case", list(ALL_CASES))
def test_loss_grad_3d_shapes_vs_yardstick(case):
    """Loss, every gradient block and the seven loss terms within the bar of the yardstick, on
    the GEMM kernels the table names."""
    (eq, kind, ns, Q), P, variants = ALL_CASES[case]
    ref = _reference(eq, kind, ns, Q)
    params = ref["params"]
    s = _solver(ref["prob"], Q, ref["fs"])
    try:
        assert s.stage_variants() == variants
        s.set_params(params)
        assert np.array_equal(s.get_flat(), O.flatten_params(params))
        loss, g = s.loss_grad()
        terms = s.loss_terms()
    finally:
        s.close()
    assert terms["loss"] == loss
    gd = O.unflatten_params(params, g)
    errs = _distances((loss, gd, terms), ref["ext"])
    bars = _bars(ref)
    record_parity("test_loss_grad_3d_shapes_vs_yardstick", case, errs, bars,
                  {"lu_oracle_err": ref["lu_err"], "fp64_tol": ref["tol"], "ns": list(ns), "padded": list(P),
                   "stage_variants": variants})
    for k in errs:
        print(case, k, f"device {errs[k]:.3e} lu {ref['lu_err'][k]:.3e} bar {bars[k]:.3e}")
    if "Cos" not in kind:
        for a in (1, 2, 3):
            assert np.all(gd[f"kernel_paras_{a}"]["freq"] == 0.0)
    for k in errs:
        assert errs[k] < bars[k], (case, k, errs[k], ref["lu_err"][k], bars[k])


# ---- state and sequencing at P = (64, 32, 96) ---------------------------------------------
def _state_solver():
    eq, kind, ns, Q = STATE
    ref = _reference(eq, kind, ns, Q)
    s = _solver(ref["prob"], Q, ref["fs"])
    s.set_params(ref["params"])
    return s, ref


@gpu
def test_loss_grad_after_steps_vs_oracle():
    """After 5 steps the handle's own state (pads, permuted copies, Adam writes) still gives
    the oracle's loss and gradient at the handle's params."""
    s, ref = _state_solver()
    try:
        s.step(5)
        flat = s.get_flat()
        loss, g = s.loss_grad()
        assert np.array_equal(s.get_flat(), flat)
    finally:
        s.close()
    params = O.unflatten_params(ref["params"], flat)
    lo, go = O.loss_grad_3d(ref["prob"], params)
    tol = _tol(ref["prob"], params)
    gd = O.unflatten_params(params, g)
    errs = {k: rel(O.flatten_params(gd[k]), O.flatten_params(go[k])) for k in go}
    errs["loss"] = abs(loss - lo) / abs(lo)
    record_parity("test_loss_grad_after_steps_vs_oracle", "T213@5", errs, tol)
    for k, e in errs.items():
        assert e < tol, (k, e, tol)


@gpu
def test_adam_trajectory_unequal_padding_vs_oracle():
    """test_adam_trajectory_3d_vs_oracle (10 steps, its bars) at P = (64, 32, 96)."""
    s, ref = _state_solver()
    try:
        losses = s.step(10)
        flat = s.get_flat()
    finally:
        s.close()
    prob, p = ref["prob"], ref["params"]
    opt = O.Adam(0.01)
    st = opt.init(p)
    want = []
    for _ in range(10):
        lo, go = O.loss_grad_3d(prob, p)
        want.append(lo)
        p, st = opt.update(go, st, p)
    tol = ref["tol"]
    errs = {"losses": rel(losses, want), "params": rel(flat, O.flatten_params(p))}
    record_parity("test_adam_trajectory_unequal_padding_vs_oracle", "T213x10", errs,
                  {"losses": max(1e-9, tol), "params": max(1e-8, 10 * tol)})
    assert errs["losses"] < max(1e-9, tol)
    assert errs["params"] < max(1e-8, 10 * tol)


@gpu
def test_loss_grad_between_steps_leaves_adam_state():
    s, _ = _state_solver()
    try:
        s.step(2)
        flat, (count, mu, nu) = s.get_flat(), s.get_opt_state()
        assert count == 2
        s.loss_grad()
        c2, m2, n2 = s.get_opt_state()
        assert c2 == count and np.array_equal(m2, mu) and np.array_equal(n2, nu)
        assert np.array_equal(s.get_flat(), flat)
    finally:
        s.close()


@gpu
def test_two_solvers_step_bitwise_and_step0():
    """Two handles give bitwise-equal losses and params over 3 steps (one of them with a
    loss_grad() in between); step(0) changes nothing."""
    a, _ = _state_solver()
    b, _ = _state_solver()
    try:
        la = a.step(3)
        lb = np.concatenate([b.step(1), b.step(0), b.step(1)])
        b.loss_grad()
        lb = np.concatenate([lb, b.step(1)])
        assert np.array_equal(la, lb)
        assert np.array_equal(a.get_flat(), b.get_flat())
        flat, (count, mu, nu) = a.get_flat(), a.get_opt_state()
        assert a.step(0).size == 0
        c2, m2, n2 = a.get_opt_state()
        assert np.array_equal(a.get_flat(), flat)
        assert c2 == count == 3 and np.array_equal(m2, mu) and np.array_equal(n2, nu)
        cb, mb, nb = b.get_opt_state()
        assert cb == 3 and np.array_equal(mb, mu) and np.array_equal(nb, nu)
    finally:
        a.close()
        b.close()


# ---- the per-axis limit -------------------------------------------------------------------
@gpu
def test_n1024_axis_vs_oracle():
    """n = 1024 (K3_MAX_N): T = 32 sweeps, the even-T output buffer, 32 log-det partials;
    cond(K1) ~ 4e8.  Against the fp64 oracle under _tol.  Every stage has exactly 16384 16x16
    tiles or fewer: the last size on the 16x16 kernel."""
    prob, params, fs = problem_3d(eq="poisson", kind="Matern52_1d", ns=(1024, 2, 3), Q=4, seed=3)
    s = _solver(prob, 4, fs)
    try:
        assert s.stage_variants() == [S] * 6
        s.set_params(params)
        loss, g = s.loss_grad()
        terms = s.loss_terms()
    finally:
        s.close()
    want = {}
    lo, go = O.loss_grad_3d(prob, params, terms=want)
    tol = _tol(prob, params)
    gd = O.unflatten_params(params, g)
    errs = _distances((loss, gd, terms), (lo, go, want))
    record_parity("test_n1024_axis_vs_oracle", "1024x2x3", errs, tol)
    for k, e in errs.items():
        assert e < tol, (k, e, tol)


@pytest.mark.parametrize("ns", [(1025, 2, 3), (2, 1025, 3), (2, 3, 1025), (1, 2, 3), (2, 1, 3), (2, 3, 1)])
def test_create3_rejects_axis_sizes_outside_2_to_1024(ns):
    """Refused on the arguments alone, before any device work (runs without a device)."""
    from gpk._lib import GPK_EINVAL, GPKError
    prob, _, fs = problem_3d(eq="poisson", kind="Matern52_1d", ns=ns, Q=4, seed=3)
    with pytest.raises(GPKError) as e:
        _solver(prob, 4, fs)
    assert e.value.code == GPK_EINVAL
