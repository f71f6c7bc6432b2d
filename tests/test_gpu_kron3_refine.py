"""3-axis step with the gated refinement of every solve (GPK_FLAG3_REFINE, DeviceSolver3(refine=
True)): X += K_k^{-1} (B - K_k X) after each of A1, A2, A3, T, S, X1, X2, X3, gated per axis on
K_00 max diag K_k^{-1} > 100.

Cases, yardstick (80-bit LU oracle), LU distance, FLOOR and the bar
    min(_tol, max(FLOOR, MULT x |fp64 LU oracle - yardstick|))
are those of tests/test_gpu_kron3_shapes.py (imported; its yardstick is computed once per session).
MULT is that file's table, never looser on any key, with two overrides:
    U                 4   (the per-size multiplier of tests/test_gpu_accuracy.py; the refined fp64
                           emulation, tools/kron3_sweep_emulation.py --refine, is <= 0.98 x LU on
                           all four Allen-Cahn cases; the unrefined device measures 7.5 / 5.7 /
                           11.5 / 7.5 x there, so the unrefined step fails this bar)
    log_v, term_egap  7   (1.5 x the refined device's measured ratio at "huge-stages0-4", 4.05
                           on the two-GEMM route and 3.88 on the fused one, rounded up to one
                           digit; the emulation there: 4.89; the rule's cap is 30; the unrefined
                           step: 268.7 x, so it fails this bar too)
Measured on the MI355X with refine=True (two-GEMM route; the fused route within 0.11 of each),
device / LU: U 0.44 / 0.54 / 0.40 / 0.41 at T321 / edge-2-P-P1 / huge-stages0-4 / Q64-cos (at most
1.18 over all twelve cases), log_v 1.32 / 0.89 / 4.05 / 0.12.  Every measured error, LU distance and bar goes to the parity log.

Gate bounds of the cases (NumPy, K_00 max diag K^{-1} per axis; threshold 100; no case within 4 x
of it): T213 6.9 / 1.0 / 8.5, edge-P-2-P1 13.7 / 1.0 / 20.4 (none open); T132 1.07 / 3.96e3 / 20.3
and Q64-cos 1.1 / 5.6e5 / 1.1 (axis 2); edge-P1-P-2 415 / 1.5 / 1.0 (axis 1); T321 and
huge-stages0-4 (all three).
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import record_parity, rel
from tests.test_gpu_kron3_shapes import ALL_CASES, FLOOR, MULT, S, _distances, _reference

gpu = pytest.mark.gpu

LOGV_MULT = 7.0
REFINE_MULT = dict(MULT, U=4.0, log_v=LOGV_MULT, term_egap=LOGV_MULT)
assert all(REFINE_MULT[k] <= MULT[k] for k in MULT)

# which axes' gates are open (module docstring)
GATES = {
    "T213": (False, False, False),
    "edge-P-2-P1": (False, False, False),
    "T132": (False, True, False),
    "edge-P1-P-2": (True, False, False),
    "Q64-cos": (False, True, False),
    "T321": (True, True, True),
    "huge-stages0-4": (True, True, True),
}


def _ref(case):
    (eq, kind, ns, Q), _, _ = ALL_CASES[case]
    return _reference(eq, kind, ns, Q), Q


def _refined(prob, Q, fs, refine=True):
    from gpk.model_GP_solver_3d import DeviceSolver3
    return DeviceSolver3(prob["eq"], prob["kind"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"],
                         prob["bvals"], Q=Q, jitter=prob["jitter"], llk_weight=prob["llk_weight"],
                         logdet=prob["logdet"], lr=0.01, freq_scale=fs, refine=refine)


def _solver_at(case, refine=True):
    ref, Q = _ref(case)
    s = _refined(ref["prob"], Q, ref["fs"], refine)
    s.set_params(ref["params"])
    return s, ref


def _loss_grad(case, refine=True):
    """(loss, flat gradient, terms, refine_info or None) of the case at its seeded params."""
    s, ref = _solver_at(case, refine)
    try:
        loss, g = s.loss_grad()
        return loss, g, s.loss_terms(), (s.refine_info() if refine else None)
    finally:
        s.close()


def _bars(ref):
    return {k: min(ref["tol"], max(FLOOR, REFINE_MULT.get(k, 2.0) * d)) for k, d in ref["lu_err"].items()}


def _check_bars(test, case, loss, g, terms, extra=None, label=None):
    ref, _ = _ref(case)
    gd = O.unflatten_params(ref["params"], g)
    errs = _distances((loss, gd, terms), ref["ext"])
    bars = _bars(ref)
    record_parity(test, label or case, errs, bars, dict({"lu_oracle_err": ref["lu_err"], "fp64_tol": ref["tol"]},
                                               **(extra or {})))
    for k in errs:
        lu = ref["lu_err"][k]
        print(case, k, f"device {errs[k]:.3e} lu {lu:.3e} ratio {errs[k] / lu if lu else float('inf'):.2f} "
              f"bar {bars[k]:.3e}")
    for k in errs:
        assert errs[k] < bars[k], (case, k, errs[k], ref["lu_err"][k], bars[k])


def _numpy_bounds(ref):
    prob, params = ref["prob"], ref["params"]
    out = []
    for a in (1, 2, 3):
        K = O.kernel_matrix(prob["kind"], prob[f"x{a}"], params[f"kernel_paras_{a}"], prob["jitter"])
        out.append(K[0, 0] * np.max(np.diag(np.linalg.inv(K))))
    return out


@gpu
@pytest.mark.parametrize("case", list(GATES))
def test_gate_table(case):
    """refine_info() after one loss_grad(): the open pattern of the table, each bound within 1e-6
    (relative) of NumPy's K_00 max diag K^{-1} -- the device's own K^{-1}."""
    _, _, _, info = _loss_grad(case)
    ref, _ = _ref(case)
    want = _numpy_bounds(ref)
    print(case, "device", info["bound"], "numpy", want)
    assert info["route"] == 1  # the fused panel kernel: every padded size here is <= 512
    assert tuple(info["open"]) == GATES[case]
    assert tuple(b > 100.0 for b in want) == GATES[case]
    for a in range(3):
        assert abs(info["bound"][a] - want[a]) <= 1e-6 * want[a], (case, a, info["bound"][a], want[a])


@gpu
@pytest.mark.parametrize("case", ["T213", "edge-P-2-P1"])
def test_closed_gates_change_nothing(case):
    """Every gate closed: a refine=True handle and a flags = 0 handle give bitwise-equal loss,
    gradient and loss terms, and bitwise-equal losses and params over 3 steps."""
    la, ga, ta, info = _loss_grad(case)
    lb, gb, tb, _ = _loss_grad(case, refine=False)
    assert info["open"] == [False] * 3
    assert la == lb and np.array_equal(ga, gb) and ta == tb
    a, _ = _solver_at(case)
    b, _ = _solver_at(case, refine=False)
    try:
        assert np.array_equal(a.step(3), b.step(3))
        assert np.array_equal(a.get_flat(), b.get_flat())
        assert a.refine_info()["open"] == [False] * 3
    finally:
        a.close()
        b.close()


@gpu
@pytest.mark.parametrize("case", ["T132", "edge-P1-P-2"])
def test_per_axis_gating(case):
    """One gate open: the results differ from the flags = 0 handle's and stay within the bars."""
    la, ga, ta, info = _loss_grad(case)
    lb, gb, _, _ = _loss_grad(case, refine=False)
    assert tuple(info["open"]) == GATES[case]
    assert not np.array_equal(ga, gb)
    assert la != lb
    _check_bars("test_per_axis_gating", case, la, ga, ta, {"open": info["open"]})


@gpu
@pytest.mark.parametrize("case", list(ALL_CASES))
def test_refined_loss_grad_vs_yardstick(case):
    """All twelve cases with refine=True within the bar of the yardstick (U: 4 x LU; log_v and
    term_egap: LOGV_MULT x LU; the unrefined step is at 11.5 x and 268.7 x at "huge-stages0-4")."""
    la, ga, ta, info = _loss_grad(case)
    assert ta["loss"] == la
    _check_bars("test_refined_loss_grad_vs_yardstick", case, la, ga, ta,
                {"open": info["open"], "bound": info["bound"]})


# ---- trajectory and state at T321 (every gate open, P = (96, 64, 32)) ----------------------
@gpu
def test_refined_adam_trajectory_vs_oracle():
    """10 Adam steps against the oracle replay under the bars of
    test_adam_trajectory_unequal_padding_vs_oracle."""
    s, ref = _solver_at("T321")
    try:
        losses = s.step(10)
        flat = s.get_flat()
        assert s.refine_info()["open"] == [True] * 3
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
    bars = {"losses": max(1e-9, tol), "params": max(1e-8, 10 * tol)}
    record_parity("test_refined_adam_trajectory_vs_oracle", "T321x10", errs, bars)
    print("T321x10", errs, bars)
    assert errs["losses"] < bars["losses"]
    assert errs["params"] < bars["params"]


@gpu
def test_refined_state_bitwise_and_opt_state_round_trip():
    """Two refine=True handles stay bitwise equal over 3 steps with a loss_grad() interleaved in
    one of them; get / set_opt_state round-trips into a third, which then steps as they do."""
    a, _ = _solver_at("T321")
    b, _ = _solver_at("T321")
    c, _ = _solver_at("T321")
    try:
        la = a.step(3)
        lb = np.concatenate([b.step(2), b.step(0)])
        flat, (count, mu, nu) = b.get_flat(), b.get_opt_state()
        b.loss_grad()
        c2, m2, n2 = b.get_opt_state()
        assert c2 == count == 2 and np.array_equal(m2, mu) and np.array_equal(n2, nu)
        assert np.array_equal(b.get_flat(), flat)
        lb = np.concatenate([lb, b.step(1)])
        assert np.array_equal(la, lb)
        assert np.array_equal(a.get_flat(), b.get_flat())
        c.set_flat(flat)
        c.set_opt_state(count, mu, nu)
        c3, m3, n3 = c.get_opt_state()
        assert c3 == count and np.array_equal(m3, mu) and np.array_equal(n3, nu)
        assert c.step(1)[0] == la[2]
        assert np.array_equal(c.get_flat(), a.get_flat())
    finally:
        a.close()
        b.close()
        c.close()


# ---- ABI -------------------------------------------------------------------------------
@gpu
def test_refine_info_needs_the_flag_and_stage_variants_stay_six():
    from gpk._lib import GPK_EINVAL, GPKError
    plain, _ = _solver_at("T213", refine=False)
    refined, _ = _solver_at("T213")
    try:
        with pytest.raises(GPKError) as e:
            plain.refine_info()
        assert e.value.code == GPK_EINVAL
        assert "GPK_FLAG3_REFINE" in str(e.value)
        assert refined.stage_variants() == plain.stage_variants() == [S] * 6
        assert refined.refine and not plain.refine
    finally:
        plain.close()
        refined.close()
