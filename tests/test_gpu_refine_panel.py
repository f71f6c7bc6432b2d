"""The refinement step X + Kinv (B - Kc X) of one mode solve on both routes (gpk_refine_panel:
the step's two GEMMs, and the fused panel kernel of refine_panel.hip) and both forms (left: the
matrices act on rows of a P x M operand; right: X + (B - X Kc) Kinv on M x P), against NumPy.

Operands N(0, 1); Kinv and Kc are unrelated (and unsymmetric) matrices, so a swapped or
transposed operand shows.  P in {32, 96, 512}, M in {32, 160}: one 16-row tile per wave slot, an
odd tile count, the LDS limit; two and ten panels.  Bar (the dot-product bound of
tests/test_gpu_kron3_predict.py): a length-P dot product in fp64 with any summation order is
within P eps sum|a_i b_i| of exact; here two nested ones, so per element
    |err| <= 4 P eps (|X| + |Kinv| (|B| + |Kc| |X|))
with eps = 2^-53 (the factor 4: both products, the subtraction and the addition, first order).
"""
import numpy as np
import pytest

from tests.test_gpu_kron3_refine import _check_bars, _ref, _refined

gpu = pytest.mark.gpu
EPS = 2.0 ** -53


def _operands(P, M, side, seed=0):
    rng = np.random.default_rng(seed)
    Kinv, Kc = rng.normal(size=(P, P)), rng.normal(size=(P, P))
    shape = (P, M) if side == 0 else (M, P)
    return Kinv, Kc, rng.normal(size=shape), rng.normal(size=shape)


@gpu
@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("P,M", [(32, 32), (32, 160), (96, 32), (96, 160), (512, 32), (512, 160)])
def test_refine_panel_vs_numpy(route, side, P, M):
    from gpk import _lib
    Kinv, Kc, B, X = _operands(P, M, side)
    got, us = _lib.refine_panel(Kinv, Kc, B, X, side=side, route=route)
    assert us is None
    if side == 0:
        want = X + Kinv @ (B - Kc @ X)
        bound = np.abs(X) + np.abs(Kinv) @ (np.abs(B) + np.abs(Kc) @ np.abs(X))
    else:
        want = X + (B - X @ Kc) @ Kinv
        bound = np.abs(X) + (np.abs(B) + np.abs(X) @ np.abs(Kc)) @ np.abs(Kinv)
    err = np.max(np.abs(got - want) / bound)
    print(route, side, P, M, f"max err / bound unit {err / (4 * P * EPS):.3e}")
    assert err <= 4 * P * EPS


@gpu
def test_fused_route_refuses_p544_and_the_handle_falls_back():
    """Two 544 x 16 panels do not fit LDS: gpk_refine_panel refuses the fused route there, and a
    handle with a 544-point axis reports the two-GEMM route."""
    from gpk import _lib
    from tests.helpers import problem_3d
    Kinv, Kc, B, X = _operands(544, 32, 0)
    with pytest.raises(_lib.GPKError) as e:
        _lib.refine_panel(Kinv, Kc, B, X, side=0, route=_lib.REFINE_FUSED)
    assert e.value.code == _lib.GPK_EINVAL
    got, _ = _lib.refine_panel(Kinv, Kc, B, X, side=0, route=_lib.REFINE_GEMM)
    assert np.all(np.isfinite(got))
    prob, params, fs = problem_3d(eq="poisson", kind="Matern52_1d", ns=(544, 2, 3), Q=4, seed=3)
    s = _refined(prob, 4, fs)
    try:
        s.set_params(params)
        s.loss_grad()
        assert s.refine_info()["route"] == _lib.REFINE_GEMM
    finally:
        s.close()


@gpu
@pytest.mark.parametrize("route", ["gemm", "fused"])  # "fused": the handle's own choice at these sizes
@pytest.mark.parametrize("case", ["huge-stages0-4", "Q64-cos"])
def test_refined_step_on_each_route_vs_yardstick(case, route):
    """The accuracy test of tests/test_gpu_kron3_refine.py, same bars, with the route forced."""
    from gpk import _lib
    ref, Q = _ref(case)
    s = _refined(ref["prob"], Q, ref["fs"], refine="gemm" if route == "gemm" else True)
    try:
        s.set_params(ref["params"])
        loss, g = s.loss_grad()
        terms, info = s.loss_terms(), s.refine_info()
    finally:
        s.close()
    assert info["route"] == (_lib.REFINE_FUSED if route == "fused" else _lib.REFINE_GEMM)
    _check_bars("test_refined_step_on_each_route_vs_yardstick", case, loss, g, terms,
                {"route": info["route"]}, label=f"{case}/{route}")
