"""Pins tests/operator3x_ref.py loss_grad_3d_opx (the yardstick of the mixed-order handles' GPU
tests) before anything on the device relies on it: against loss_grad_3d_op where every axis has
one order, against torch autograd of the dense-Kronecker log joint on mixed axes, and the
manufactured sources of equations.EQUATIONS_3D_OPX against autograd of their solutions."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import autograd_ref as AR
from tests.helpers import problem_3d, rel
from tests.operator3_ref import FACES, loss_grad_3d_op
from tests.operator3x_ref import as_op, loss_grad_3d_opx


def _blocks(ga, gb):
    return {k: rel(O.flatten_params(ga[k]), O.flatten_params(gb[k])) for k in gb}


def _mask(prob, ns, faces):
    bv, o = np.array(prob["bvals"], np.float64), 0
    for f, sl in enumerate(FACES):
        n = np.zeros(ns)[sl].size
        if not (faces >> f) & 1:
            bv[o:o + n] = np.nan
        o += n
    return dict(prob, bvals=bv)


# one order per axis, stated with two weight vectors: orders (2,2,1), (1,1,1), (2,1,2), a zero axis
ONE_ORDER = [dict(c2=(-0.1, -0.1, 0.0), c1=(0.0, 0.0, 1.0), react=(0.0, 0.0, 0.0), faces=0b011111),
             dict(c2=(0.0, 0.0, 0.0), c1=(1.0, 0.5, 1.0), react=(0.0, 0.0, 0.0), faces=63),
             dict(c2=(-0.3, 0.0, 1.0), c1=(0.0, -0.7, 0.0), react=(0.4, -0.5, 0.2), faces=0b111011),
             dict(c2=(1.0, 0.0, 1.0), c1=(0.0, 0.0, 0.0), react=(-1.0, 0.0, 1.0), faces=63)]


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op", ONE_ORDER)
def test_one_order_per_axis_is_loss_grad_3d_op(op, kind):
    ns = (9, 7, 6)
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=ns, Q=3, seed=4)
    prob = _mask(prob, ns, op["faces"])
    lo, go = loss_grad_3d_op(prob, params, as_op(op))
    l, g = loss_grad_3d_opx(prob, params, op)
    errs = _blocks(g, go)
    print("opx vs op", as_op(op)["order"], kind, abs(l - lo) / abs(lo), errs)
    assert abs(l - lo) / abs(lo) <= 1e-13
    assert max(errs.values()) <= 1e-13


def dense_loss_grad_3d_opx(prob, params, op):
    """tests/test_operator3_ref.py dense_loss_grad_3d_op with D_k = c2_k DD_k + c1_k D1_k: DENSE
    Kronecker products, the log-det of K itself, torch autograd."""
    tp = AR._tp(params)
    kind = prob["kind"]
    xs = [torch.tensor(prob[f"x{a}"]) for a in (1, 2, 3)]
    Ks, Ds = [], []
    for k in range(3):
        kp = tp[f"kernel_paras_{k + 1}"]
        K, DD = AR.mats(kind, xs[k], kp, prob["jitter"], 2)
        _, D1 = AR.mats(kind, xs[k], kp, prob["jitter"], 1)
        Ks.append(K)
        Ds.append(op["c2"][k] * DD + op["c1"][k] * D1)
    K1, K2, K3 = Ks
    D1, D2, D3 = Ds
    U = tp["U"]
    u = U.reshape(-1)
    K = torch.kron(K1, torch.kron(K2, K3))
    Kinv_u = torch.linalg.solve(K, u)
    L = (torch.kron(D1, torch.kron(K2, K3)) + torch.kron(K1, torch.kron(D2, K3))
         + torch.kron(K1, torch.kron(K2, D3))) @ Kinv_u
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


# mixed on one, two and three axes; weights of both signs; a reaction; one face open
MIXED_CASES = [
    dict(c2=(-0.3, 0.0, 1.0), c1=(0.8, -0.7, 0.0), react=(0.0, 0.0, 0.0), faces=63),            # axis 1
    dict(c2=(1.0, 0.6, 0.0), c1=(0.0, -1.1, 1.0), react=(0.4, -0.5, 0.2), faces=0b011111),       # axis 2
    dict(c2=(0.0, -0.2, 0.9), c1=(1.0, 0.0, -0.4), react=(0.0, 0.0, 0.0), faces=0b111011),       # axis 3
    dict(c2=(-0.05, -0.05, 0.0), c1=(1.0, 0.5, 1.0), react=(0.0, 0.0, 0.0), faces=0b011111),     # two (convdiff_t)
    dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, -0.6, 1.3), react=(0.4, -0.5, 0.2), faces=0b011111),     # three
]


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op", MIXED_CASES)
def test_mixed_axes_vs_dense_kronecker_autograd(op, kind):
    ns = (6, 5, 4)
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=ns, Q=2, seed=11)
    prob = _mask(prob, ns, op["faces"])
    l, g = loss_grad_3d_opx(prob, params, op)
    la, ga = dense_loss_grad_3d_opx(prob, params, op)
    errs = _blocks(g, ga)
    print("opx vs autograd", op["c2"], op["c1"], bin(op["faces"]), kind, abs(l - la) / abs(la), errs)
    assert np.isfinite(l) and all(np.all(np.isfinite(O.flatten_params(g[k]))) for k in g)
    # the three-axis bar of tests/test_operator3_ref.py
    conds = [np.linalg.cond(O.kernel_matrix(kind, prob[f"x{a}"], params[f"kernel_paras_{a}"], prob["jitter"]))
             for a in (1, 2, 3)]
    tol = min(1e-9, max(1e-11, 100 * float(np.prod(conds)) * np.finfo(float).eps))
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


def test_opx_equation_sources_are_the_operator_applied_to_u():
    """src = sum_k (c2_k d^2 + c1_k d) u / dx_k + reaction at random points, by torch autograd of
    the solution, to 1e-10."""
    from gpk import equations as E
    assert E.EQUATIONS_3D_OPX == ["convdiff_t-sin", "convdiff_3d-sin"]
    tu = {"convdiff_t-sin": lambda x, y, t: torch.exp(-t) * torch.sin(2 * x) * torch.sin(3 * y),
          "convdiff_3d-sin": lambda x, y, z: torch.sin(2 * x) * torch.sin(3 * y) * torch.sin(z)}
    pts = np.random.default_rng(0).uniform(0.05, 0.95, size=(40, 3))
    for e in E.EQUATIONS_3D_OPX:
        u, src, op = E.solution_3d_opx(e)
        assert isinstance(op, E.Operator3X) and E.Operator3X.of(op.as_dict()) == op
        X = [torch.tensor(pts[:, k], requires_grad=True) for k in range(3)]
        uu = tu[e](*X)
        assert np.allclose(uu.detach().numpy(), u(*pts.T), rtol=0, atol=1e-15)
        lhs = op.react[0] * uu + op.react[1] * uu ** 2 + op.react[2] * uu ** 3
        for k in range(3):
            g, = torch.autograd.grad(uu.sum(), X[k], create_graph=True)
            gg, = torch.autograd.grad(g.sum(), X[k], create_graph=True)
            lhs = lhs + op.c2[k] * gg + op.c1[k] * g
        err = float(np.max(np.abs(lhs.detach().numpy() - src(*pts.T))))
        print(e, "source err", err)
        assert err < 1e-10
    t, s3 = E.solution_3d_opx("convdiff_t-sin")[2], E.solution_3d_opx("convdiff_3d-sin")[2]
    assert t.mixed == (True, True, False) and t.faces == 0b011111 and t.c2[2] == 0.0 and t.c1[2] == 1.0
    assert s3.mixed == (True, True, True) and s3.faces == 63
