"""NumPy references and the case lists of the derivative / scattered-point prediction tests
(tests/test_gpu_predict_deriv.py, tests/test_gpu_eq_residual.py, tests/test_evaluate_host.py).

The reference is the reference's own association (code/model_GP_solver_2d.py:185-220), axis after
axis: T <- kappa_k^(d_k)(x*_k, x_k) x_k solve(K_k, T) from T = U, with kernel_block(deriv = d_k)
as the cross block -- on a grid, or per point.  `solve` is LU (numpy.linalg.solve) unless a test
passes another (Cholesky: the CPU test that checks the reference against itself).
"""
import functools

import numpy as np

from oracle import gp_oracle as O
from tests.helpers import problem_1d, problem_2d, problem_3d

EPS = np.finfo(float).eps
KINDS = ["SE_Cos_1d", "Matern52_Cos_1d", "SE_1d", "Matern52_1d"]
DERIVS_2D = [(a, b) for a in range(3) for b in range(3)]
DERIVS_3D = [(0, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 2)]
# (eq, (n1, n2)): the issue's two sizes for Poisson and Allen-Cahn, advection at the small one
CASES_2D = [(eq, ns) for ns in ((24, 20), (33, 70)) for eq in ("poisson", "allencahn")] + [("advection", (24, 20))]
MS_2D = [(11, 37), (35, 7)]
CASES_1D = [(eq, n) for n in (40, 70) for eq in ("poisson", "allencahn")]
M_1D = 37
CASES_3D = [((20, 14, 9), (11, 37, 5)), ((33, 40, 9), (35, 7, 33))]
N_RANDOM = 37


@functools.lru_cache(maxsize=None)
def case_2d(eq, ns, kind):
    prob, params, _, fs = problem_2d(eq=eq, kind=kind, n1=ns[0], n2=ns[1], Q=5, seed=3)
    return prob, params, fs


@functools.lru_cache(maxsize=None)
def case_1d(eq, n):
    prob, params, _ = problem_1d(eq=eq, n=n, Q=5, seed=3)
    return prob, params, 20.0


@functools.lru_cache(maxsize=None)
def case_3d(ns):
    return problem_3d(ns=ns, seed=3)  # (prob, params, fs), Q = 4


def axes_of(prob, params):
    """[(x_k, kernel params of axis k)] and the field U with one array axis per grid axis."""
    if "x" in prob:
        return [(prob["x"], params["kernel_paras"])], np.asarray(params["u"], np.float64).reshape(-1)
    dim = 3 if "x3" in prob else 2
    return ([(prob[f"x{k}"], params[f"kernel_paras_{k}"]) for k in range(1, dim + 1)],
            np.asarray(params["U"], np.float64))


def bar(prob, params):
    """The project's per-size bar (tests/test_gpu_kron3.py _tol): max(1e-10, 50 cond eps) with cond
    the largest cond_2(K_k) of the handle's factors."""
    ax, _ = axes_of(prob, params)
    c = max(np.linalg.cond(O.kernel_matrix(prob["kind"], x, kp, prob["jitter"])) for x, kp in ax)
    return max(1e-10, 50 * c * EPS)


def grid_axes(prob, params, ms):
    """linspace(-0.03, 1.02, m) x_max per axis: inside and a little outside the collocation range."""
    ax, _ = axes_of(prob, params)
    return [np.linspace(-0.03, 1.02, m) * x[-1] for (x, _), m in zip(ax, ms)]


def random_points(prob, params, m, seed=7):
    ax, _ = axes_of(prob, params)
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.03, 1.02, size=(m, len(ax))) * np.array([x[-1] for x, _ in ax])


def chol_solve(K, B):
    L = np.linalg.cholesky(K)
    return np.linalg.solve(L.T, np.linalg.solve(L, B))


def _solve_axis(solve, K, T, k):
    """solve(K, .) along array axis k of T."""
    Tk = np.moveaxis(T, k, 0)
    return np.moveaxis(solve(K, Tk.reshape(Tk.shape[0], -1)).reshape(Tk.shape), 0, k)


def ref_grid(prob, params, xte, d, solve=np.linalg.solve):
    """The d-th derivatives of the interpolant on the grid xte[0] x xte[1] x ..."""
    ax, T = axes_of(prob, params)
    for k, (x, kp) in enumerate(ax):
        A = _solve_axis(solve, O.kernel_matrix(prob["kind"], x, kp, prob["jitter"]), T, k)
        F = O.kernel_block(prob["kind"], np.asarray(xte[k], np.float64), x, kp, int(d[k]))
        T = np.moveaxis(np.tensordot(F, A, axes=(1, k)), 0, k)
    return T


def ref_points(prob, params, pts, d, solve=np.linalg.solve):
    """The same at scattered points pts (m, dim): the association per point."""
    ax, T = axes_of(prob, params)
    pts = np.asarray(pts, np.float64).reshape(-1, len(ax))
    for k, (x, kp) in enumerate(ax):
        K = O.kernel_matrix(prob["kind"], x, kp, prob["jitter"])
        F = O.kernel_block(prob["kind"], np.ascontiguousarray(pts[:, k]), x, kp, int(d[k]))
        if k == 0:  # [n1, ...] -> [m, ...]
            T = np.tensordot(F, _solve_axis(solve, K, T, 0), axes=(1, 0))
        else:       # [m, n_k, ...] -> [m, ...], each point against its own slice
            A = _solve_axis(solve, K, T, 1)
            T = np.einsum("pj,pj...->p...", F, A)
    return T
