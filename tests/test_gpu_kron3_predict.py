"""3-axis solver beyond the step: the slab-batched mode-2 GEMM (gpk_mode_gemm), test-grid
predictions (gpk_predict3), the stop criterion (gpk_criterion3), the Adam state round trip
(gpk_get/set_opt_state3) and GP_solver_3d_single.train with checkpoint / resume.

References are numpy on the oracle's pieces (kernel_matrix, kernel_block, kernel_kd, mode_product,
loss_grad_3d, Adam); the solves are LU (numpy.linalg.solve), axis after axis.
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.helpers import problem_3d, rel
from tests.test_gpu_kron3 import KINDS, _solver, _tol

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps


# ---- gpk_mode_gemm ----------------------------------------------------------------------
def _apply(M, T, k):
    """M x_k T for any M (m, T.shape[k - 1]), k in 1..3."""
    return np.einsum(("mi,ijk->mjk", "mj,ijk->imk", "mk,ijk->ijm")[k - 1], M, T)


def _mode_case(shape, k, seed):
    d1, d2, d3, m = shape
    rng = np.random.default_rng(seed)
    T = rng.normal(size=(d1, d2, d3))
    Mat = rng.normal(size=(m, (d1, d2, d3)[k - 1]))
    out = [d1, d2, d3]
    out[k - 1] = m
    return Mat, T, rng.normal(size=out)


def _check_mode(C, Mat, T, k, alpha=1.0, beta=0.0, C0=None):
    ref = alpha * _apply(Mat, T, k)
    bound = abs(alpha) * _apply(np.abs(Mat), np.abs(T), k)
    if C0 is not None:
        ref = ref + beta * C0
        bound = bound + abs(beta) * np.abs(C0)
    bound = 2 * Mat.shape[1] * EPS * bound  # the dot-product bound, K = d_k terms
    err = np.abs(C - ref)
    print("mode", k, "max err / bound", float(np.max(err / bound)))
    assert C.shape == ref.shape
    assert np.all(err <= bound)


# (d1, d2, d3, m): one slab row against several; m <, =, > K (slab strides of B and C differ);
# N at one and at an odd number of 32- and 64-wide tiles.  Variants 2 / 3 force the slab
# kernel's 32x32 / 64x64 tile at each of them (at 32-wide M and 160-wide N the 64x64 tiles are
# half empty); AUTO64_SHAPE has 512 x 512 slab outputs, where the launch takes the 64x64 tile on
# its own (SLAB_TILE64_MIN)
MODE_SHAPES = [(32, 32, 32, 32), (96, 64, 32, 128), (32, 96, 160, 32)]
AUTO64_SHAPE = (32, 32, 512, 512)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])  # slab, permute route, slab 32 / 64 tile forced
@pytest.mark.parametrize("shape", MODE_SHAPES)
def test_mode2_gemm_vs_einsum(shape, variant):
    from gpk._lib import mode_gemm
    Mat, T, _ = _mode_case(shape, 2, 11)
    C, _ = mode_gemm(Mat, T, 2, variant=variant)
    _check_mode(C, Mat, T, 2)


def test_mode2_gemm_auto_tile64():
    from gpk._lib import mode_gemm
    Mat, T, _ = _mode_case(AUTO64_SHAPE, 2, 14)
    C, _ = mode_gemm(Mat, T, 2)
    _check_mode(C, Mat, T, 2)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("shape", MODE_SHAPES[:2])
def test_mode13_gemm_vs_einsum(shape, k):
    from gpk._lib import mode_gemm
    Mat, T, _ = _mode_case(shape, k, 12)
    C, _ = mode_gemm(Mat, T, k)
    _check_mode(C, Mat, T, k)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_mode2_gemm_epilogue(variant):
    """beta = 1 with C0 = C (in place), and alpha = -1, beta = 1 with a separate C0."""
    from gpk._lib import mode_gemm
    Mat, T, C0 = _mode_case(MODE_SHAPES[1], 2, 13)
    C, _ = mode_gemm(Mat, T, 2, beta=1.0, C0=C0, inplace=True, variant=variant)
    _check_mode(C, Mat, T, 2, 1.0, 1.0, C0)
    C, _ = mode_gemm(Mat, T, 2, alpha=-1.0, beta=1.0, C0=C0, variant=variant)
    _check_mode(C, Mat, T, 2, -1.0, 1.0, C0)


def test_mode_gemm_rejects_bad_sizes():
    from gpk._lib import GPKError, mode_gemm
    with pytest.raises(GPKError):
        mode_gemm(np.zeros((32, 40)), np.zeros((32, 40, 32)), 2)
    with pytest.raises(GPKError):
        mode_gemm(np.zeros((32, 32)), np.zeros((32, 32, 32)), 4)


# ---- predictions ------------------------------------------------------------------------
def ref_predict(prob, params, xte):
    """T <- Kmn_k x_k solve(K_k, T) for k = 1, 2, 3 from T = U, LU solves."""
    T = np.asarray(params["U"], np.float64)
    for k in (1, 2, 3):
        x, kp = prob[f"x{k}"], params[f"kernel_paras_{k}"]
        K = O.kernel_matrix(prob["kind"], x, kp, prob["jitter"])
        Tk = np.moveaxis(T, k - 1, 0)
        A = np.moveaxis(np.linalg.solve(K, Tk.reshape(Tk.shape[0], -1)).reshape(Tk.shape), 0, k - 1)
        T = _apply(O.kernel_block(prob["kind"], np.asarray(xte[k - 1]), x, kp, 0), A, k)
    return T


def _test_axes(prob, ms):
    # inside and a little outside the collocation range, not on its points
    return [np.linspace(-0.03, 1.02, m) * prob[f"x{a}"][-1] for a, m in zip((1, 2, 3), ms)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("eq", ["poisson", "allencahn"])
@pytest.mark.parametrize("ns,ms", [((20, 14, 9), (11, 37, 5)), ((33, 40, 9), (35, 7, 33))])
def test_predict3_vs_numpy(ns, ms, eq, kind):
    prob, params, fs = problem_3d(eq=eq, kind=kind, ns=ns, Q=4, seed=3)
    xte = _test_axes(prob, ms)
    s = _solver(prob, 4, fs)
    try:
        s.set_params(params)
        flat = s.get_flat()
        cnt0 = s.get_opt_state()[0]
        pred = s.predict(*xte)
        assert np.array_equal(s.get_flat(), flat)  # params untouched
        assert np.array_equal(flat, O.flatten_params(params))
        assert s.get_opt_state()[0] == cnt0
    finally:
        s.close()
    ref = ref_predict(prob, params, xte)
    tol = _tol(prob, params)
    print("predict3", ns, ms, eq, kind, "rel err", rel(pred, ref), "tol", tol)
    assert pred.shape == tuple(ms)
    assert rel(pred, ref) < tol


# ---- criterion --------------------------------------------------------------------------
@pytest.mark.parametrize("eq", ["poisson", "allencahn"])
def test_criterion3_vs_numpy(eq):
    prob, params, fs = problem_3d(eq=eq, kind="Matern52_Cos_1d", ns=(20, 14, 9), Q=4, seed=5)
    s = _solver(prob, 4, fs)
    try:
        s.set_params(params)
        c = s.criterion()
        assert np.array_equal(s.get_flat(), O.flatten_params(params))
    finally:
        s.close()
    U = params["U"]
    R = -np.asarray(prob["src"], np.float64).reshape(U.shape)
    for k in range(3):
        K, D = O.kernel_kd(prob["kind"], prob[f"x{k + 1}"], params[f"kernel_paras_{k + 1}"], prob["jitter"], 2)
        Uk = np.moveaxis(U, k, 0)
        A = np.moveaxis(np.linalg.solve(K, Uk.reshape(Uk.shape[0], -1)).reshape(Uk.shape), 0, k)
        R = R + O.mode_product(D, A, k)
    if eq == "allencahn":
        R = R + U * (U * U - 1.0)
    bres = O.boundary_3d(U) - prob["bvals"]
    n1, n2, n3 = U.shape
    assert bres.size == 2 * (n2 * n3 + n1 * n3 + n1 * n2)
    ref = float(bres @ bres) / bres.size + float(np.sum(R * R)) / U.size
    print("criterion3", eq, c, ref)
    assert abs(c - ref) / abs(ref) < _tol(prob, params)


# ---- Adam state -------------------------------------------------------------------------
def test_opt_state3_round_trip():
    prob, params, fs = problem_3d(eq="poisson", kind="Matern52_Cos_1d", ns=(12, 10, 8), Q=4, seed=2)
    a, b, c = (_solver(prob, 4, fs) for _ in range(3))
    try:
        a.set_params(params)
        la = a.step(6)
        b.set_params(params)
        lb = b.step(3)
        flat, (count, mu, nu) = b.get_flat(), b.get_opt_state()
        assert count == 3 and mu.shape == nu.shape == flat.shape
        c.set_flat(flat)
        c.set_opt_state(count, mu, nu)
        lc = c.step(3)
        assert np.array_equal(np.concatenate([lb, lc]), la)
        assert np.array_equal(c.get_flat(), a.get_flat())
        ca, ma, na = a.get_opt_state()
        cc, mc, nc = c.get_opt_state()
        assert ca == cc == 6 and np.array_equal(ma, mc) and np.array_equal(na, nc)
        with pytest.raises(ValueError):
            c.set_opt_state(0, mu[:-1], nu[:-1])
        with pytest.raises(ValueError):
            c.set_opt_state(0, mu, np.concatenate([nu, nu]))
    finally:
        for s in (a, b, c):
            s.close()


# ---- train ------------------------------------------------------------------------------
def _train_problem():
    from gpk.kernel_matrix import kernel_class
    prob, _, fs = problem_3d(eq="poisson", kind="Matern52_Cos_1d", ns=(12, 10, 8), Q=4, seed=0)
    xte = [np.linspace(0, 1, 9) * 2 * np.pi for _ in range(3)]
    ute = O._u3d("poisson_3d-mix_sin")[0](*np.meshgrid(*xte, indexing="ij"))
    tp = {"kernel": kernel_class("Matern52_Cos_1d"), "equation": "poisson_3d-mix_sin", "llk_weight": 200.0,
          "logdet": True, "lr": 0.01, "Q": 4, "freq_scale": fs, "nepoch": 20, "tol": -1}

    def make():
        from gpk.model_GP_solver_3d import GP_solver_3d_single
        return GP_solver_3d_single(prob["bvals"], (prob["x1"], prob["x2"], prob["x3"]), prob["src"],
                                   prob["jitter"], tp, X_test=xte, u_test=ute)
    return prob, fs, xte, ute, make


def test_train_3d_vs_oracle_replay_and_resume(tmp_path):
    prob, fs, xte, ute, make = _train_problem()
    m = make()
    try:
        log, stop, min_err = m.train(20, verbose=False)
        flat = m.dev.get_flat()
        assert isinstance(m.params["U"], np.ndarray) and m.params["U"].shape == (12, 10, 8)
    finally:
        m.dev.close()
    # oracle replay: loss before each update, error after it
    p = O.init_params_3d(12, 10, 8, 4, fs)
    tol = max(1e-8, 10 * _tol(prob, p))
    opt = O.Adam(0.01)
    st = opt.init(p)
    losses, errs = [], []
    for _ in range(20):
        lo, go = O.loss_grad_3d(prob, p)
        p, st = opt.update(go, st, p)
        losses.append(np.log(lo) if lo > 1 else lo)
        pr = ref_predict(prob, p, xte)
        errs.append(np.linalg.norm(pr.ravel() - ute.ravel()) / np.linalg.norm(ute.ravel()))
    print("train3d loss rel", rel(log["loss_list"], losses), "err rel", rel(log["err_list"], errs), "tol", tol)
    assert log["epoch_list"] == list(range(20))
    assert rel(log["loss_list"], losses) < tol
    assert rel(log["err_list"], errs) < tol
    assert min_err == min(log["err_list"]) and not stop["flag"]
    assert len(log["w_list_k3"]) == 20 and log["freq_list_k1"][0].shape == (4,)
    # checkpoint at 10 epochs, resume on a fresh handle: bitwise the uninterrupted run
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
    assert min2 == min_err
    assert sorted(log2) == sorted(log)
    for k in log:
        assert np.array_equal(np.asarray(log2[k]), np.asarray(log[k])), k


def test_solver3d_reference_call_forms():
    """step(params, opt_state) / compute_early_stopping next to the step(n) / loss forms."""
    prob, fs, xte, ute, make = _train_problem()
    m = make()
    try:
        p0 = m.init_params()
        l0 = m.loss(p0)
        lv, g = m.value_and_grad(p0)
        assert l0 == lv and g["U"].shape == (12, 10, 8)
        params, opt, loss = m.step(p0, m.reset_optimizer())
        assert loss == l0
        params, opt, loss2 = m.step(params, opt)
        assert opt.fetch()["count"] == 2
        crit = m.compute_early_stopping(params)
        assert np.isfinite(crit) and crit > 0
        l3 = m.step(2)
        assert l3.shape == (2,) and m.dev.get_opt_state()[0] == 4
        pred, _ = m.preds(m.current())
        assert pred.shape == (9, 9, 9)
    finally:
        m.dev.close()


# ---- argument errors --------------------------------------------------------------------
def test_predict3_argument_errors():
    from gpk._lib import GPKError
    prob, params, fs = problem_3d(eq="poisson", kind="SE_Cos_1d", ns=(8, 7, 6), Q=3, seed=1)
    s = _solver(prob, 3, fs)
    try:
        s.set_params(params)
        before = s.loss_grad()[0]
        x = np.linspace(0, 1, 5)
        with pytest.raises(GPKError):
            s.predict(x, np.zeros(0), x)       # m = 0
        with pytest.raises(GPKError):
            s.predict(x, None, x)              # NULL axis
        with pytest.raises(GPKError):
            s.predict(x, x, np.linspace(0, 1, 1025))
        assert s.loss_grad()[0] == before
        assert s.predict(x, x, x).shape == (5, 5, 5)
    finally:
        s.close()
