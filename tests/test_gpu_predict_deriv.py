"""Derivative predictions and scattered-point evaluation (gpk_predict_deriv[3], gpk_evaluate[3])
against NumPy: the reference's association with LU solves and kernel_block(deriv = d_k) as the
cross block (tests/predict_deriv_ref.py), at the project's per-size bar max(1e-10, 50 cond eps).
tests/test_evaluate_host.py checks on the CPU that the reference agrees with a Cholesky
restatement of itself within a quarter of that bar for every case used here.
"""
import numpy as np
import pytest

from tests import predict_deriv_ref as R
from tests.helpers import device_solver, rel
from tests.test_gpu_kron3 import _solver

pytestmark = pytest.mark.gpu


def _state(s):
    return s.get_flat(), s.get_opt_state()[0]


def _same_state(s, st):
    return np.array_equal(s.get_flat(), st[0]) and s.get_opt_state()[0] == st[1]


def _check(figs, tol):
    """figs: [(label, rel err)]; print every figure, then assert them all."""
    for label, e in figs:
        print(label, "rel err", e, "tol", tol)
    bad = [(label, e) for label, e in figs if not e < tol]
    assert not bad, (bad, tol)


def _grid_points(xte):
    return np.stack(np.meshgrid(*xte, indexing="ij"), -1).reshape(-1, len(xte))


# ---- 2D ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("eq,ns", R.CASES_2D)
def test_predict_deriv_2d_vs_numpy(eq, ns, kind):
    prob, params, fs = R.case_2d(eq, ns, kind)
    tol = R.bar(prob, params)
    s = device_solver(prob, 5, fs)
    figs = []
    try:
        s.set_params(params)
        st = _state(s)
        for ms in R.MS_2D:
            xte = R.grid_axes(prob, params, ms)
            for d in R.DERIVS_2D:
                out = s.predict_deriv(xte[0], xte[1], deriv=d)
                assert out.shape == ms
                figs.append(((eq, ns, kind, ms, d), rel(out, R.ref_grid(prob, params, xte, d))))
        assert _same_state(s, st)
    finally:
        s.close()
    _check(figs, tol)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("eq,ns", R.CASES_2D)
def test_evaluate_2d_vs_numpy(eq, ns, kind):
    """37 random points against the reference at the points; an 11 x 7 grid passed as a list of
    points against predict_deriv on that grid (the last contraction sums in another order)."""
    prob, params, fs = R.case_2d(eq, ns, kind)
    tol = R.bar(prob, params)
    pts = R.random_points(prob, params, R.N_RANDOM)
    xte = R.grid_axes(prob, params, (11, 7))
    s = device_solver(prob, 5, fs)
    figs = []
    try:
        s.set_params(params)
        st = _state(s)
        for d in R.DERIVS_2D:
            out = s.evaluate(pts, deriv=d)
            assert out.shape == (R.N_RANDOM,)
            figs.append((("points", eq, ns, kind, d), rel(out, R.ref_points(prob, params, pts, d))))
            g = s.evaluate(_grid_points(xte), deriv=d)
            figs.append((("grid list", eq, ns, kind, d), rel(g, s.predict_deriv(xte[0], xte[1], deriv=d).ravel())))
        assert _same_state(s, st)
    finally:
        s.close()
    _check(figs, tol)


# ---- 1D ---------------------------------------------------------------------------------
@pytest.mark.parametrize("eq,n", R.CASES_1D)
def test_predict_deriv_and_evaluate_1d_vs_numpy(eq, n):
    prob, params, fs = R.case_1d(eq, n)
    tol = R.bar(prob, params)
    xte = R.grid_axes(prob, params, (R.M_1D,))
    pts = R.random_points(prob, params, R.N_RANDOM)
    s = device_solver(prob, 5, fs)
    figs = []
    try:
        s.set_params(params)
        st = _state(s)
        for d in (0, 1, 2):
            out = s.predict_deriv(xte[0], deriv=d)
            assert out.shape == (R.M_1D,)
            figs.append((("grid", eq, n, d), rel(out, R.ref_grid(prob, params, xte, (d,)))))
            e = s.evaluate(pts, deriv=d)
            assert e.shape == (R.N_RANDOM,)
            figs.append((("points", eq, n, d), rel(e, R.ref_points(prob, params, pts, (d,)))))
            figs.append((("grid list", eq, n, d), rel(s.evaluate(xte[0], deriv=(d,)), out)))
        assert _same_state(s, st)
    finally:
        s.close()
    _check(figs, tol)


# ---- 3 axes -----------------------------------------------------------------------------
@pytest.mark.parametrize("ns,ms", R.CASES_3D)
def test_predict_deriv_3d_vs_numpy(ns, ms):
    prob, params, fs = R.case_3d(ns)
    tol = R.bar(prob, params)
    xte = R.grid_axes(prob, params, ms)
    pts = R.random_points(prob, params, R.N_RANDOM)
    s = _solver(prob, 4, fs)
    figs = []
    try:
        s.set_params(params)
        st = _state(s)
        for d in R.DERIVS_3D:
            out = s.predict_deriv(*xte, deriv=d)
            assert out.shape == tuple(ms)
            figs.append((("grid", ns, ms, d), rel(out, R.ref_grid(prob, params, xte, d))))
            e = s.evaluate(pts, deriv=d)
            assert e.shape == (R.N_RANDOM,)
            figs.append((("points", ns, d), rel(e, R.ref_points(prob, params, pts, d))))
        assert _same_state(s, st)
    finally:
        s.close()
    _check(figs, tol)


def test_evaluate3_chunks():
    """1500 points: more than one chunk of 1024, the last one ragged.  All 1500 against NumPy; the
    first 1024 bitwise equal to a call with only those (chunking changes no result)."""
    ns = (20, 14, 9)
    prob, params, fs = R.case_3d(ns)
    pts = R.random_points(prob, params, 1500, seed=11)
    d = (1, 0, 2)
    s = _solver(prob, 4, fs)
    try:
        s.set_params(params)
        out = s.evaluate(pts, deriv=d)
        head = s.evaluate(pts[:1024], deriv=d)
        again = s.evaluate(pts, deriv=d)
    finally:
        s.close()
    assert out.shape == (1500,)
    _check([(("1500 points", d), rel(out, R.ref_points(prob, params, pts, d)))], R.bar(prob, params))
    assert np.array_equal(out[:1024], head)
    assert np.array_equal(out, again)  # deterministic


# ---- order 0 is the old call ------------------------------------------------------------
def test_order_zero_is_predict_bitwise():
    prob, params, fs = R.case_2d("allencahn", (33, 70), "Matern52_Cos_1d")
    xte = R.grid_axes(prob, params, (35, 7))
    s = device_solver(prob, 5, fs)
    try:
        s.set_params(params)
        assert np.array_equal(s.predict_deriv(xte[0], xte[1], deriv=(0, 0)), s.predict(xte[0], xte[1]))
    finally:
        s.close()
    prob, params, fs = R.case_1d("allencahn", 70)
    xte = R.grid_axes(prob, params, (R.M_1D,))
    s = device_solver(prob, 5, fs)
    try:
        s.set_params(params)
        assert np.array_equal(s.predict_deriv(xte[0], deriv=0), s.predict(xte[0]))
    finally:
        s.close()
    ns, ms = R.CASES_3D[1]
    prob, params, fs = R.case_3d(ns)
    xte = R.grid_axes(prob, params, ms)
    s = _solver(prob, 4, fs)
    try:
        s.set_params(params)
        assert np.array_equal(s.predict_deriv(*xte, deriv=(0, 0, 0)), s.predict(*xte))
    finally:
        s.close()


# ---- argument errors --------------------------------------------------------------------
def test_argument_errors_2d_and_1d():
    from gpk._lib import GPKError
    x = np.linspace(0, 1, 5)
    for prob, params, fs in (R.case_2d("poisson", (24, 20), "SE_Cos_1d"), R.case_1d("poisson", 40)):
        dim = 1 if "x" in prob else 2
        s = device_solver(prob, 5, fs)
        try:
            s.set_params(params)
            before = s.loss_grad()[0]
            grid = (x,) * dim
            for bad in (3, -1):
                with pytest.raises(GPKError):
                    s.predict_deriv(*grid, deriv=(bad,) * dim)
                with pytest.raises(GPKError):
                    s.evaluate(np.zeros((4, dim)), deriv=(0,) * (dim - 1) + (bad,))
            with pytest.raises(GPKError):
                s.predict_deriv(np.zeros(0), *grid[1:], deriv=(1,) * dim)  # m = 0
            with pytest.raises(GPKError):
                s.evaluate(np.zeros((0, dim)), deriv=(1,) * dim)          # m = 0
            with pytest.raises(GPKError):
                s.evaluate(None, deriv=(1,) * dim)                        # NULL points
            if dim == 2:
                with pytest.raises(GPKError):
                    s.predict_deriv(x, None, deriv=(1, 1))                # NULL axis
            with pytest.raises(ValueError):
                s.predict_deriv(*grid, deriv=(0,) * (dim + 1))
            assert s.loss_grad()[0] == before
            assert np.all(np.isfinite(s.step(1)))
            assert s.predict_deriv(*grid, deriv=(2,) * dim).shape == (5,) * dim
        finally:
            s.close()


def test_argument_errors_3d():
    from gpk._lib import GPKError
    from tests.helpers import problem_3d
    prob, params, fs = problem_3d(eq="poisson", kind="SE_Cos_1d", ns=(8, 7, 6), Q=3, seed=1)
    s = _solver(prob, 3, fs)
    try:
        s.set_params(params)
        before = s.loss_grad()[0]
        x = np.linspace(0, 1, 5)
        for bad in (3, -1):
            with pytest.raises(GPKError):
                s.predict_deriv(x, x, x, deriv=(0, bad, 0))
            with pytest.raises(GPKError):
                s.evaluate(np.zeros((4, 3)), deriv=(bad, 0, 0))
        with pytest.raises(GPKError):
            s.predict_deriv(x, np.zeros(0), x, deriv=(1, 0, 0))       # m = 0
        with pytest.raises(GPKError):
            s.predict_deriv(x, None, x, deriv=(1, 0, 0))              # NULL axis
        with pytest.raises(GPKError):
            s.predict_deriv(x, x, np.linspace(0, 1, 1025), deriv=(1, 0, 0))  # a grid axis is capped
        with pytest.raises(GPKError):
            s.evaluate(np.zeros((0, 3)), deriv=(1, 0, 0))             # m = 0
        with pytest.raises(GPKError):
            s.evaluate(None, deriv=(1, 0, 0))                         # NULL points
        assert s.loss_grad()[0] == before
        big = s.evaluate(np.random.default_rng(0).uniform(0, 1, size=(5000, 3)), deriv=(0, 1, 0))
        assert big.shape == (5000,) and np.all(np.isfinite(big))      # scattered points are not capped
        assert s.loss_grad()[0] == before
        assert np.all(np.isfinite(s.step(1)))
    finally:
        s.close()
