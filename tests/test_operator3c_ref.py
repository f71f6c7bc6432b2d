"""Pins tests/operator3c_ref.py loss_grad_3d_opc (the yardstick of the convective handles' GPU
tests) before anything on the device relies on it: with conv of zeros it is loss_grad_3d_opn, with
convective axes it matches torch autograd of the dense-Kronecker log joint, a frozen-field identity
ties it to the pinned loss_grad_3d_opv, and the sources of equations.EQUATIONS_3D_OPC are their
operators applied to their solutions."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import autograd_ref as AR
from tests.helpers import problem_3d, rel
from tests.operator3_ref import FACES
from tests.operator3c_ref import adam_replay_c, criterion_3d_opc, loss_grad_3d_opc
from tests.operator3n_ref import adam_replay_n, criterion_3d_opn, face_data, loss_grad_3d_opn
from tests.operator3v_ref import loss_grad_3d_opv
from tests.test_operator3n_ref import DERIV_CASES, random_dvals
from tests.test_operator3v_ref import smooth_fields
from tests.test_operator3x_ref import _blocks, _mask

NS = (6, 5, 4)


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which,dfaces", DERIV_CASES[:2])
def test_zero_conv_is_loss_grad_3d_opn_exactly(op, which, dfaces, kind):
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=NS, Q=2, seed=11)
    prob = _mask(prob, NS, op["faces"])
    coef = smooth_fields(NS, which, seed=len(which))
    dvals = random_dvals(NS, dfaces, seed=dfaces)
    tn, tc = {}, {}
    lo, go = loss_grad_3d_opn(prob, params, op, coef, dfaces, dvals, terms=tn)
    for conv in (None, (0.0, 0.0, 0.0)):
        tc.clear()
        l, g = loss_grad_3d_opc(prob, params, op, coef, dfaces, dvals, conv, terms=tc)
        assert l == lo and tc == tn
        for k in go:
            assert np.array_equal(O.flatten_params(g[k]), O.flatten_params(go[k])), k
    assert criterion_3d_opc(prob, params, op, coef, dfaces, dvals) == criterion_3d_opn(prob, params, op, coef, dfaces, dvals)
    (la, pa), (lb, pb) = (adam_replay_c(prob, params, op, coef, dfaces, dvals, None, 2),
                          adam_replay_n(prob, params, op, coef, dfaces, dvals, 2))
    assert la == lb and np.array_equal(O.flatten_params(pa), O.flatten_params(pb))


def dense_loss_grad_3d_opc(prob, params, op, coef, dfaces, dvals, conv):
    """tests/test_operator3n_ref.py dense_loss_grad_3d_opn with the convective term: u times
    sum_k g_k (autograd's D1_k in the Kronecker product) K^{-1} u."""
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


# (operator, fields on, dfaces, conv): all three axes convective over a mixed axis, a coefficient
# field, a reaction, one open face and one derivative face; a pure convective axis (c2 = c1 = 0)
CONV_CASES = [
    (dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, 0.0, 1.3), react=(0.4, -0.5, 0.2), faces=0b011111), (0, 3), 0b000100,
     (1.0, -0.7, 0.5)),
    (dict(c2=(0.0, -0.1, 0.0), c1=(0.0, 0.0, 1.0), react=(0.0, 0.0, 0.0), faces=0b011111), (), 0, (1.5, 0.0, 0.0)),
]


def _tol(prob, params):
    """the three-axis bar of tests/test_operator3_ref.py"""
    conds = [np.linalg.cond(O.kernel_matrix(prob["kind"], prob[f"x{a}"], params[f"kernel_paras_{a}"], prob["jitter"]))
             for a in (1, 2, 3)]
    return min(1e-9, max(1e-11, 100 * float(np.prod(conds)) * np.finfo(float).eps))


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which,dfaces,conv", CONV_CASES)
def test_convective_axes_vs_dense_kronecker_autograd(op, which, dfaces, conv, kind):
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=NS, Q=2, seed=11)
    prob = _mask(prob, NS, op["faces"])
    coef = smooth_fields(NS, which, seed=len(which))
    dvals = random_dvals(NS, dfaces, seed=dfaces) if dfaces else None
    t = {}
    l, g = loss_grad_3d_opc(prob, params, op, coef, dfaces, dvals, conv, terms=t)
    la, ga = dense_loss_grad_3d_opc(prob, params, op, coef, dfaces, dvals, conv)
    errs = _blocks(g, ga)
    print("opc vs autograd", conv, bin(dfaces), which, kind, abs(l - la) / abs(la), errs)
    assert np.isfinite(l) and all(np.all(np.isfinite(O.flatten_params(g[k]))) for k in g)
    # the term matters: without it the loss is another one
    assert abs(loss_grad_3d_opn(prob, params, op, coef, dfaces, dvals)[0] - l) > 1e-6 * abs(l)
    assert np.abs(t["N"]).max() > 0.0
    tol = _tol(prob, params)
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_frozen_field_identity_with_loss_grad_3d_opv(k, kind):
    """One convective axis k with c2_k = c1_k = 0 against loss_grad_3d_opv with c1_k = g_k and the
    field a_k frozen at the current U: the same loss and kernel-parameter, tau and v gradients;
    dL/dU differs by exactly v V_k . R (the field's own dependence on U)."""
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=NS, Q=2, seed=5)
    gk = 0.8
    c2, c1 = [-0.2, 0.3, -0.1], [0.5, 0.0, 1.0]
    c2[k] = c1[k] = 0.0
    op = dict(c2=tuple(c2), c1=tuple(c1), react=(0.3, 0.0, -0.2), faces=0b110111)
    prob = _mask(prob, NS, op["faces"])
    conv = tuple(gk if a == k else 0.0 for a in range(3))
    none = dict(a=(None, None, None), rho=None)
    t = {}
    l, g = loss_grad_3d_opc(prob, params, op, none, 0, None, conv, terms=t)
    c1v = list(c1)
    c1v[k] = gk
    U = np.asarray(params["U"], np.float64).reshape(NS)
    frozen = dict(a=tuple(U.copy() if a == k else None for a in range(3)), rho=None)
    lv, gv = loss_grad_3d_opv(prob, params, dict(op, c1=tuple(c1v)), frozen)
    bar = 1e-13
    assert abs(l - lv) / abs(lv) < bar, (l, lv)
    for key in g:
        if key == "U":
            continue
        e = rel(O.flatten_params(g[key]), O.flatten_params(gv[key]))
        print("frozen field", k, kind, key, e)
        assert e < bar, (key, e)
    v = np.exp(float(params["log_v"]))
    assert abs(float(np.sum(t["R"] ** 2)) - t["egap"]) <= 1e-15 * t["egap"] and np.abs(t["N"]).max() > 0.0
    want = np.asarray(gv["U"]).reshape(NS) + v * t["N"] * t["R"]
    e = rel(np.asarray(g["U"]).reshape(NS), want)
    print("frozen field", k, kind, "dL/dU against opv's + v V_k . R", e)
    assert e < bar, e
    assert rel(np.asarray(g["U"]).reshape(NS), np.asarray(gv["U"]).reshape(NS)) > 1e3 * bar  # (the difference is there)


def test_opc_equation_sources_are_the_operator_applied_to_u():
    """src = sum_k (c2_k d^2 + c1_k d) u / dx_k + u sum_k g_k du / dx_k (+ the reaction terms) and
    grad_u = grad u at random points, by torch autograd of the solution, to 1e-10."""
    from gpk import equations as E
    assert E.EQUATIONS_3D_OPC == ["burgers_t-sin", "burgers_3d-sin"]
    tu = {"burgers_t-sin": lambda x, y, t: torch.exp(-t) * torch.sin(2 * x) * torch.sin(3 * y),
          "burgers_3d-sin": lambda x, y, z: torch.sin(2 * x) * torch.sin(3 * y) * torch.sin(z)}
    pts = np.random.default_rng(0).uniform(0.05, 0.95, size=(40, 3))
    for e in E.EQUATIONS_3D_OPC:
        u, src, op, dfaces, grad_u, conv = E.solution_3d_opc(e)
        assert isinstance(op, E.Operator3X) and len(grad_u) == 3 and len(conv) == 3 and dfaces == 0
        X = [torch.tensor(pts[:, k], requires_grad=True) for k in range(3)]
        uu = tu[e](*X)
        assert np.allclose(uu.detach().numpy(), u(*pts.T), rtol=0, atol=1e-15)
        lhs = op.react[0] * uu + op.react[1] * uu ** 2 + op.react[2] * uu ** 3
        for k in range(3):
            g, = torch.autograd.grad(uu.sum(), X[k], create_graph=True)
            gg, = torch.autograd.grad(g.sum(), X[k], create_graph=True)
            lhs = lhs + op.c2[k] * gg + op.c1[k] * g + conv[k] * uu * g
            gerr = float(np.max(np.abs(g.detach().numpy() - grad_u[k](*pts.T))))
            assert gerr < 1e-10, (e, k, gerr)
        err = float(np.max(np.abs(lhs.detach().numpy() - src(*pts.T))))
        print(e, "source err", err)
        assert err < 1e-10
    bt, b3 = (E.solution_3d_opc(e) for e in E.EQUATIONS_3D_OPC)
    nu = E._BURGERS_NU
    assert nu == 0.05
    assert bt[2] == E.Operator3X((-nu, -nu, 0.0), (0.0, 0.0, 1.0), faces=0b011111) and bt[5] == (1.0, 1.0, 0.0)
    assert b3[2] == E.Operator3X((-nu, -nu, -nu), (0.0, 0.0, 0.0), faces=63) and b3[5] == (1.0, 1.0, 1.0)
