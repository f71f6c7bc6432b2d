"""Pins tests/operator3m_ref.py loss_grad_3d_opm (the yardstick of the cross handles' GPU tests)
before anything on the device relies on it: with cross of zeros it is loss_grad_3d_opc, with mixed
partials it matches torch autograd of the dense-Kronecker log joint, and the sources of
equations.EQUATIONS_3D_OPM are their operators applied to their solutions."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import autograd_ref as AR
from tests.helpers import problem_3d
from tests.operator3_ref import FACES
from tests.operator3c_ref import adam_replay_c, criterion_3d_opc, loss_grad_3d_opc
from tests.operator3m_ref import PAIRS, adam_replay_m, criterion_3d_opm, loss_grad_3d_opm
from tests.operator3n_ref import face_data
from tests.test_operator3c_ref import CONV_CASES, _tol
from tests.test_operator3n_ref import random_dvals
from tests.test_operator3v_ref import smooth_fields
from tests.test_operator3x_ref import _blocks, _mask

NS = (6, 5, 4)


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which,dfaces,conv", CONV_CASES)
def test_zero_cross_is_loss_grad_3d_opc_exactly(op, which, dfaces, conv, kind):
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=NS, Q=2, seed=11)
    prob = _mask(prob, NS, op["faces"])
    coef = smooth_fields(NS, which, seed=len(which))
    dvals = random_dvals(NS, dfaces, seed=dfaces) if dfaces else None
    tc, tm = {}, {}
    lo, go = loss_grad_3d_opc(prob, params, op, coef, dfaces, dvals, conv, terms=tc)
    for cross in (None, (0.0, 0.0, 0.0)):
        tm.clear()
        l, g = loss_grad_3d_opm(prob, params, op, coef, dfaces, dvals, conv, cross, terms=tm)
        assert l == lo and set(tm) == set(tc)
        assert all(np.array_equal(tm[k], tc[k]) for k in tc)
        for k in go:
            assert np.array_equal(O.flatten_params(g[k]), O.flatten_params(go[k])), k
    assert (criterion_3d_opm(prob, params, op, coef, dfaces, dvals, conv)
            == criterion_3d_opc(prob, params, op, coef, dfaces, dvals, conv))
    (la, pa), (lb, pb) = (adam_replay_m(prob, params, op, coef, dfaces, dvals, conv, None, 2),
                          adam_replay_c(prob, params, op, coef, dfaces, dvals, conv, 2))
    assert la == lb and np.array_equal(O.flatten_params(pa), O.flatten_params(pb))


def dense_loss_grad_3d_opm(prob, params, op, coef, dfaces, dvals, conv, cross):
    """tests/test_operator3c_ref.py dense_loss_grad_3d_opc with the cross terms: m_jk times (D1_j and
    D1_k in the Kronecker product's places j and k, K in the third) K^{-1} u."""
    tp = AR._tp(params)
    kind = prob["kind"]
    xs = [torch.tensor(prob[f"x{a}"]) for a in (1, 2, 3)]
    Ks, Ds, D1s = [], [], []
    for k in range(3):
        kp = tp[f"kernel_paras_{k + 1}"]
        K, DD = AR.mats(kind, xs[k], kp, prob["jitter"], 2)
        _, D1 = AR.mats(kind, xs[k], kp, prob["jitter"], 1)
        Ks.append(K)
        D1s.append(D1)
        Ds.append(op["c2"][k] * DD + op["c1"][k] * D1)
    K1, K2, K3 = Ks
    U = tp["U"]
    u = U.reshape(-1)
    fld = lambda f: torch.ones_like(u) if f is None else torch.tensor(np.asarray(f, np.float64).reshape(-1))
    a = [fld(f) for f in coef["a"]]
    K = torch.kron(K1, torch.kron(K2, K3))
    Kinv_u = torch.linalg.solve(K, u)
    on_axis = lambda k, M: torch.kron(M if k == 0 else K1, torch.kron(M if k == 1 else K2, M if k == 2 else K3))
    L = sum(a[k] * (on_axis(k, Ds[k]) @ Kinv_u) for k in range(3))
    r1, r2, r3 = op["react"]
    R = L - torch.tensor(prob["src"]).reshape(-1) + r1 * u + r2 * u ** 2 + r3 * u ** 3
    if coef["rho"] is not None:
        R = R + fld(coef["rho"]) * u
    for k in range(3):
        if conv[k] != 0.0:
            R = R + u * (conv[k] * (on_axis(k, D1s[k]) @ Kinv_u))
    for (j, k), m in zip(PAIRS, cross):
        if m != 0.0:
            f = [D1s[i] if i in (j, k) else Ks[i] for i in range(3)]
            R = R + m * (torch.kron(f[0], torch.kron(f[1], f[2])) @ Kinv_u)
    egap = (R ** 2).sum()
    bv = torch.tensor(np.nan_to_num(np.asarray(prob["bvals"], np.float64), nan=0.0))
    bgap, Nb, o = 0.0, 0, 0
    for f, sl in enumerate(FACES):
        n = U[sl].numel()
        if (op["faces"] >> f) & 1:
            bgap = bgap + ((U[sl].reshape(-1) - bv[o:o + n]) ** 2).sum()
            Nb += n
        o += n
    ns = tuple(U.shape)
    for f, h in (face_data(dvals, ns, dfaces) if dfaces else {}).items():
        k, s = divmod(f, 2)
        Ak = torch.linalg.solve(Ks[k], torch.movedim(U, k, 0).reshape(ns[k], -1))
        g = D1s[k][ns[k] - 1 if s else 0] @ Ak
        bgap = bgap + ((g - torch.tensor(h).reshape(-1)) ** 2).sum()
        Nb += g.numel()
    log_prior = -0.5 * torch.linalg.slogdet(K)[1] * prob["logdet"] - 0.5 * (u * Kinv_u).sum()
    log_b = 0.5 * Nb * tp["log_tau"] - 0.5 * torch.exp(tp["log_tau"]) * bgap
    eq_ll = 0.5 * u.numel() * tp["log_v"] - 0.5 * torch.exp(tp["log_v"]) * egap
    loss = -(log_prior + log_b * prob["llk_weight"] + eq_ll)
    loss.backward()
    return float(loss.detach()), AR._grads(tp)


# (operator, fields on, dfaces, conv, cross): each pair alone on a plain operator (the third one on
# axes with c2 = c1 = 0); all three pairs over CONV_CASES[0]'s mixed axis, field, reaction, open
# face, derivative face and convective axes
PLAIN = dict(c2=(-0.3, 0.7, -0.2), c1=(0.0, 0.0, 0.0), react=(0.0, 0.0, 0.0), faces=63)
CROSS_CASES = [
    (PLAIN, (), 0, (0.0, 0.0, 0.0), (0.8, 0.0, 0.0)),
    (PLAIN, (), 0, (0.0, 0.0, 0.0), (0.0, -0.6, 0.0)),
    (dict(PLAIN, c2=(-0.3, 0.0, 0.0)), (), 0, (0.0, 0.0, 0.0), (0.0, 0.0, 1.1)),
    CONV_CASES[0] + ((0.8, -0.6, 1.1),),
]


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which,dfaces,conv,cross", CROSS_CASES)
def test_cross_terms_vs_dense_kronecker_autograd(op, which, dfaces, conv, cross, kind):
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=NS, Q=2, seed=11)
    prob = _mask(prob, NS, op["faces"])
    coef = smooth_fields(NS, which, seed=len(which))
    dvals = random_dvals(NS, dfaces, seed=dfaces) if dfaces else None
    l, g = loss_grad_3d_opm(prob, params, op, coef, dfaces, dvals, conv, cross)
    la, ga = dense_loss_grad_3d_opm(prob, params, op, coef, dfaces, dvals, conv, cross)
    errs = _blocks(g, ga)
    print("opm vs autograd", cross, conv, bin(dfaces), which, kind, abs(l - la) / abs(la), errs)
    assert np.isfinite(l) and all(np.all(np.isfinite(O.flatten_params(g[k]))) for k in g)
    # the term matters: without it the loss is another one
    assert abs(loss_grad_3d_opc(prob, params, op, coef, dfaces, dvals, conv)[0] - l) > 1e-6 * abs(l)
    tol = _tol(prob, params)
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


def test_opm_equation_sources_are_the_operator_applied_to_u():
    """src = sum_k (c2_k d^2 + c1_k d) u / dx_k + sum_{j<k} m_jk d^2 u / dx_j dx_k (+ convective and
    reaction terms) and grad_u = grad u at random points, by torch autograd of the solution, to 1e-10."""
    from gpk import equations as E
    assert E.EQUATIONS_3D_OPM == ["aniso_heat_t-sin", "aniso_3d-sin"]
    tu = {"aniso_heat_t-sin": lambda x, y, t: torch.exp(-t) * torch.sin(2 * x) * torch.sin(3 * y),
          "aniso_3d-sin": lambda x, y, z: torch.sin(2 * x) * torch.sin(3 * y) * torch.sin(z)}
    pts = np.random.default_rng(0).uniform(0.05, 0.95, size=(40, 3))
    for e in E.EQUATIONS_3D_OPM:
        u, src, op, dfaces, grad_u, conv, cross = E.solution_3d_opm(e)
        assert isinstance(op, E.Operator3X) and len(grad_u) == 3 and len(conv) == 3 and len(cross) == 3 and dfaces == 0
        X = [torch.tensor(pts[:, k], requires_grad=True) for k in range(3)]
        uu = tu[e](*X)
        assert np.allclose(uu.detach().numpy(), u(*pts.T), rtol=0, atol=1e-15)
        lhs = op.react[0] * uu + op.react[1] * uu ** 2 + op.react[2] * uu ** 3
        gs = []
        for k in range(3):
            g, = torch.autograd.grad(uu.sum(), X[k], create_graph=True)
            gg, = torch.autograd.grad(g.sum(), X[k], create_graph=True)
            gs.append(g)
            lhs = lhs + op.c2[k] * gg + op.c1[k] * g + conv[k] * uu * g
            gerr = float(np.max(np.abs(g.detach().numpy() - grad_u[k](*pts.T))))
            assert gerr < 1e-10, (e, k, gerr)
        for (j, k), m in zip(PAIRS, cross):
            gjk, = torch.autograd.grad(gs[j].sum(), X[k], create_graph=True)
            lhs = lhs + m * gjk
        err = float(np.max(np.abs(lhs.detach().numpy() - src(*pts.T))))
        print(e, "source err", err)
        assert err < 1e-10
    ht, a3 = (E.solution_3d_opm(e) for e in E.EQUATIONS_3D_OPM)
    assert ht[2] == E.Operator3X((-0.1, -0.06, 0.0), (0.0, 0.0, 1.0), faces=0b011111)
    assert ht[5] == (0.0, 0.0, 0.0) and ht[6] == (-0.08, 0.0, 0.0)
    assert a3[2] == E.Operator3X((-1.0, -1.0, -1.0), (0.0, 0.0, 0.0), faces=63)
    assert a3[5] == (0.0, 0.0, 0.0) and a3[6] == (-0.6, -0.4, -0.2)
