"""Pins tests/operator3_ref.py loss_grad_3d_op (the yardstick of the operator handles' GPU tests)
before anything on the device relies on it: against the 3-axis oracle where the operator states
one of its two equations, and against torch autograd of the dense-Kronecker log joint for mixed
orders, weights, a reaction polynomial and face masks."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import autograd_ref as AR
from tests.helpers import problem_3d, rel
from tests.operator3_ref import FACES, POISSON_OP, loss_grad_3d_op


def _blocks(ga, gb):
    return {k: rel(O.flatten_params(ga[k]), O.flatten_params(gb[k])) for k in gb}


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
def test_poisson_operator_is_the_oracle(kind):
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=(9, 7, 6), Q=3, seed=4)
    lo, go = O.loss_grad_3d(prob, params)
    l, g = loss_grad_3d_op(prob, params, POISSON_OP)
    errs = _blocks(g, go)
    print("poisson op vs oracle", abs(l - lo) / abs(lo), errs)
    assert abs(l - lo) / abs(lo) <= 1e-14
    assert max(errs.values()) <= 1e-14


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
def test_allencahn_reaction_is_the_oracle(kind):
    prob, params, _ = problem_3d(eq="allencahn", kind=kind, ns=(9, 7, 6), Q=3, seed=4)
    lo, go = O.loss_grad_3d(prob, params)
    l, g = loss_grad_3d_op(prob, params, dict(POISSON_OP, react=(-1.0, 0.0, 1.0)))
    errs = _blocks(g, go)
    print("allencahn op vs oracle", abs(l - lo) / abs(lo), errs)
    assert abs(l - lo) / abs(lo) <= 1e-13
    assert max(errs.values()) <= 1e-13


def dense_loss_grad_3d_op(prob, params, op):
    """The operator log joint with DENSE Kronecker products and torch autograd, in the manner of
    tests/autograd_ref.py loss_grad_3d: K = K1 (x) K2 (x) K3, the axis-k term (.. D_k ..) K^{-1} vec U,
    the log-det of K itself, the boundary as the six face slices under the mask."""
    tp = AR._tp(params)
    kind = prob["kind"]
    xs = [torch.tensor(prob[f"x{a}"]) for a in (1, 2, 3)]
    KD = [AR.mats(kind, xs[k], tp[f"kernel_paras_{k + 1}"], prob["jitter"], op["order"][k]) for k in range(3)]
    (K1, D1), (K2, D2), (K3, D3) = KD
    U = tp["U"]
    u = U.reshape(-1)
    K = torch.kron(K1, torch.kron(K2, K3))
    Kinv_u = torch.linalg.solve(K, u)
    c1, c2, c3 = op["coef"]
    L = (c1 * torch.kron(D1, torch.kron(K2, K3)) + c2 * torch.kron(K1, torch.kron(D2, K3))
         + c3 * torch.kron(K1, torch.kron(K2, D3))) @ Kinv_u
    r1, r2, r3 = op["react"]
    R = L - torch.tensor(prob["src"]).reshape(-1) + r1 * u + r2 * u ** 2 + r3 * u ** 3
    egap = (R ** 2).sum()
    bv = torch.tensor(np.nan_to_num(np.asarray(prob["bvals"], np.float64), nan=0.0))
    bgap, Nb, o = 0.0, 0, 0
    for f, sl in enumerate(FACES):
        n = U[sl].numel()
        if (op["faces"] >> f) & 1:
            bgap = bgap + ((U[sl].reshape(-1) - bv[o:o + n]) ** 2).sum()
            Nb += n
        o += n
    log_prior = -0.5 * torch.linalg.slogdet(K)[1] * prob["logdet"] - 0.5 * (u * Kinv_u).sum()
    log_b = 0.5 * Nb * tp["log_tau"] - 0.5 * torch.exp(tp["log_tau"]) * bgap
    eq_ll = 0.5 * u.numel() * tp["log_v"] - 0.5 * torch.exp(tp["log_v"]) * egap
    loss = -(log_prior + log_b * prob["llk_weight"] + eq_ll)
    loss.backward()
    return float(loss.detach()), AR._grads(tp)


# (orders, faces): one face open; one face active.  Open faces' bvals are NaN.
AUTOGRAD_CASES = [((2, 1, 2), 0b011111), ((1, 2, 1), 0b010000), ((2, 1, 2), 0b010000), ((1, 2, 1), 0b111011)]


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("order,faces", AUTOGRAD_CASES)
def test_operator_vs_dense_kronecker_autograd(order, faces, kind):
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=(5, 4, 3), Q=2, seed=11)
    op = dict(order=order, coef=(-0.3, -0.7, 1.0), react=(0.4, -0.5, 0.2), faces=faces)
    bv, o = np.array(prob["bvals"], np.float64), 0
    for f, sl in enumerate(FACES):
        n = np.zeros((5, 4, 3))[sl].size
        if not (faces >> f) & 1:
            bv[o:o + n] = np.nan
        o += n
    prob = dict(prob, bvals=bv)
    l, g = loss_grad_3d_op(prob, params, op)
    la, ga = dense_loss_grad_3d_op(prob, params, op)
    errs = _blocks(g, ga)
    print("op vs autograd", order, bin(faces), kind, abs(l - la) / abs(la), errs)
    assert np.isfinite(l) and all(np.all(np.isfinite(O.flatten_params(g[k]))) for k in g)
    # the bar of tests/test_oracle.py's 3-axis comparison, and never looser than 1e-9
    conds = [np.linalg.cond(O.kernel_matrix(kind, prob[f"x{a}"], params[f"kernel_paras_{a}"], prob["jitter"]))
             for a in (1, 2, 3)]
    tol = min(1e-9, max(1e-11, 100 * float(np.prod(conds)) * np.finfo(float).eps))
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)
