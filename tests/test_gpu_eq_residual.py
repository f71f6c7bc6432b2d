"""The model classes' derivative surface: preds_deriv, preds_at and eq_residual of
GP_solver_1d_single, GP_solver_2d_single (Poisson, Allen-Cahn), its advection subclass and
GP_solver_3d_single.  eq_residual on a test grid equals the class's own equation expression
assembled in NumPy from the reference predictions (tests/predict_deriv_ref.py), within the
project's bar scaled by the largest term."""
import numpy as np
import pytest

from tests import predict_deriv_ref as R

pytestmark = pytest.mark.gpu

KIND = "Matern52_Cos_1d"
EQ_NAMES = {"poisson": "poisson_2d-sin_sin", "allencahn": "allencahn_2d-mix-sincos",
            "advection": "advection-multiscale"}


def _tp(prob, Q, fs, equation, **extra):
    from gpk.kernel_matrix import kernel_class
    tp = {"kernel": kernel_class(prob["kind"]), "llk_weight": prob["llk_weight"], "Q": Q, "lr": 0.01,
          "freq_scale": fs, "logdet": True, "equation": equation}
    tp.update(extra)
    return tp


def _make(case):
    """(solver object, prob, params, test-grid sizes) of one class."""
    if case == "1d":
        from gpk.model_GP_solver_1d import GP_solver_1d_single
        prob, params, fs = R.case_1d("poisson", 40)
        m = GP_solver_1d_single(prob["xind"], prob["y"], prob["x"].reshape(-1, 1), prob["src"], prob["jitter"],
                                None, None, _tp(prob, 5, fs, "poisson_1d-single_sin"))
        return m, prob, params, (R.M_1D,)
    if case == "3d":
        from gpk.model_GP_solver_3d import GP_solver_3d_single
        prob, params, fs = R.case_3d((20, 14, 9))
        m = GP_solver_3d_single(prob["bvals"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"], prob["jitter"],
                                _tp(prob, 4, fs, "poisson_3d-mix_sin"))
        return m, prob, params, (11, 37, 5)
    from gpk import model_GP_solver_2d as m2d
    from gpk import model_GP_solver_advection as madv
    prob, params, fs = R.case_2d(case, (24, 20), KIND)
    cls, extra = m2d.GP_solver_2d_single, {}
    if case == "advection":
        cls, extra = madv.GP_solver_2d_single_advection, {"beta": prob["beta"]}
    m = cls(prob["bvals"], (prob["x1"], prob["x2"]), prob["src"], prob["jitter"], None, None,
            _tp(prob, 5, fs, EQ_NAMES[case], **extra))
    return m, prob, params, (11, 37)


@pytest.mark.parametrize("case", ["1d", "poisson", "allencahn", "advection", "3d"])
def test_eq_residual_and_shapes(case):
    m, prob, params, ms = _make(case)
    dim = len(ms)
    xte = R.grid_axes(prob, params, ms)
    X_test = xte[0] if dim == 1 else tuple(xte)
    src = np.random.default_rng(2).normal(size=ms)
    pts = R.random_points(prob, params, 9)
    try:
        res = m.eq_residual(params, X_test, src)
        one = tuple(1 if k == 0 else 0 for k in range(dim))
        pd = m.preds_deriv(params, one, X_test)
        at = m.preds_at(params, pts, deriv=one)
        at0 = m.preds_at(params, pts)
        with pytest.raises(ValueError):
            m.preds_deriv(params, one)  # no X_test and the solver has no grid of its own
    finally:
        m.dev.close()

    def ref(k, order):
        d = [0] * dim
        d[k] = order
        return R.ref_grid(prob, params, xte, d)

    if case == "advection":
        terms = [prob["beta"] * ref(0, 1), ref(1, 1)]
    else:
        terms = [ref(k, 2) for k in range(dim)]
        if case == "allencahn":
            u = ref(0, 0)
            terms.append(u * (u ** 2 - 1))
    expect = sum(terms) - src
    tol = R.bar(prob, params)
    scale = max(float(np.max(np.abs(t))) for t in terms + [src])
    err = float(np.max(np.abs(res - expect)))
    print("eq_residual", case, "err / scale", err / scale, "tol", tol)
    assert res.shape == tuple(ms) and pd.shape == tuple(ms)
    assert at.shape == (9,) and at0.shape == (9,)
    assert err < tol * scale
    assert float(np.max(np.abs(pd - ref(0, 1)))) < tol * float(np.max(np.abs(ref(0, 1))))
    r1 = R.ref_points(prob, params, pts, one)
    assert float(np.max(np.abs(at - r1))) < tol * float(np.max(np.abs(r1)))
    r0 = R.ref_points(prob, params, pts, (0,) * dim)
    assert float(np.max(np.abs(at0 - r0))) < tol * float(np.max(np.abs(r0)))
