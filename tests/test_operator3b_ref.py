"""Pins tests/operator3b_ref.py loss_grad_3d_opb (the yardstick of the drift handles' GPU tests)
before anything on the device relies on it: with no drift it is loss_grad_3d_opm, a constant drift
is a constant c1, a drift of the frozen solution is the convective term with U held fixed, with
drift fields it matches torch autograd of the dense-Kronecker log joint, and the sources of
equations.EQUATIONS_3D_OPB are their operators applied to their solutions."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import autograd_ref as AR
from tests.helpers import problem_3d
from tests.operator3_ref import FACES
from tests.operator3b_ref import adam_replay_b, criterion_3d_opb, loss_grad_3d_opb
from tests.operator3c_ref import loss_grad_3d_opc
from tests.operator3m_ref import PAIRS, adam_replay_m, criterion_3d_opm, loss_grad_3d_opm
from tests.operator3n_ref import face_data
from tests.test_operator3c_ref import CONV_CASES, _tol
from tests.test_operator3m_ref import CROSS_CASES
from tests.test_operator3n_ref import random_dvals
from tests.test_operator3v_ref import smooth_fields
from tests.test_operator3x_ref import _blocks, _mask

NS = (6, 5, 4)


def drift_fields_for(ns, axes, seed=5):
    """Smooth non-constant drift fields of both signs on the given axes (smooth_fields' kind, another
    seed: different from any a_k of the same case)."""
    f = smooth_fields(ns, tuple(axes), seed=seed)["a"]
    return tuple(f[k] if k in axes else None for k in range(3))


def _setup(op, which, dfaces, kind):
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=NS, Q=2, seed=11)
    prob = _mask(prob, NS, op["faces"])
    coef = smooth_fields(NS, which, seed=len(which))
    dvals = random_dvals(NS, dfaces, seed=dfaces) if dfaces else None
    return prob, params, coef, dvals


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which,dfaces,conv,cross", CROSS_CASES[:1] + CROSS_CASES[3:])
def test_no_drift_is_loss_grad_3d_opm_exactly(op, which, dfaces, conv, cross, kind):
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    tm, tb = {}, {}
    lo, go = loss_grad_3d_opm(prob, params, op, coef, dfaces, dvals, conv, cross, terms=tm)
    for drift in (None, (None, None, None)):
        tb.clear()
        l, g = loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift, terms=tb)
        assert l == lo and set(tb) == set(tm)
        assert all(np.array_equal(tb[k], tm[k]) for k in tm)
        for k in go:
            assert np.array_equal(O.flatten_params(g[k]), O.flatten_params(go[k])), k
    assert (criterion_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross)
            == criterion_3d_opm(prob, params, op, coef, dfaces, dvals, conv, cross))
    (la, pa), (lb, pb) = (adam_replay_b(prob, params, op, coef, dfaces, dvals, conv, cross, None, 2),
                          adam_replay_m(prob, params, op, coef, dfaces, dvals, conv, cross, 2))
    assert la == lb and np.array_equal(O.flatten_params(pa), O.flatten_params(pb))


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which,dfaces,conv,cross", CROSS_CASES[:1] + CROSS_CASES[3:])
def test_constant_drift_is_a_constant_c1(op, which, dfaces, conv, cross, kind):
    """b_k = beta_k everywhere is loss_grad_3d_opm with c1_k + beta_k, on the axes without a field a_k
    (a field multiplies c1_k but not the drift), at the bar of the constant-field identity of
    tests/test_operator3v_ref.py."""
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    beta = [0.7, -1.3, 0.45]
    for k in range(3):
        if coef["a"][k] is not None:
            beta[k] = None
    drift = tuple(None if b is None else np.full(NS, b) for b in beta)
    op2 = dict(op, c1=tuple(c + (b or 0.0) for c, b in zip(op["c1"], beta)))
    l, g = loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift)
    lo, go = loss_grad_3d_opm(prob, params, op2, coef, dfaces, dvals, conv, cross)
    errs = _blocks(g, go)
    print("constant drift", kind, abs(l - lo) / abs(lo), errs)
    assert abs(l - lo) / abs(lo) < 1e-13
    assert max(errs.values()) < 1e-13


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_frozen_field_identity_with_the_convective_term(k, kind):
    """b_k = g_k U (held fixed) against loss_grad_3d_opc with a convective axis of weight g_k: the same
    loss and kernel-parameter, tau and v blocks; dL/dU is opc's minus the direct term v V_k . R."""
    op, which, dfaces, _ = CONV_CASES[0]
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    gk = (1.0, -0.7, 0.5)[k]
    conv = tuple(gk if a == k else 0.0 for a in range(3))
    U = np.asarray(params["U"], np.float64).reshape(NS)
    drift = tuple(gk * U if a == k else None for a in range(3))
    t = {}
    lc, gc = loss_grad_3d_opc(prob, params, op, coef, dfaces, dvals, conv, terms=t)
    l, g = loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, None, None, drift)
    v = np.exp(float(params["log_v"]))
    want = dict(gc, U=np.asarray(gc["U"]).reshape(NS) - v * t["N"] * t["R"])
    errs = _blocks(g, want)
    print("frozen field", k, kind, abs(l - lc) / abs(lc), errs)
    assert np.abs(t["N"]).max() > 0.0
    assert abs(l - lc) / abs(lc) < 1e-13
    assert max(errs.values()) < 1e-13


def dense_loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift):
    """tests/test_operator3m_ref.py dense_loss_grad_3d_opm with the drift terms: diag(b_k) times (D1_k in
    the Kronecker product's place k, K in the others) K^{-1} u."""
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
    for k in range(3):
        if drift[k] is not None:
            R = R + fld(drift[k]) * (on_axis(k, D1s[k]) @ Kinv_u)
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


# (operator, fields on, dfaces, conv, cross, drift axes): each axis alone on a plain operator (axis 2
# with c2 = c1 = 0); all three over CONV_CASES[0]'s mixed axis, field a_1 (different from b_1), rho,
# reaction, open face, derivative face and convective axes, with the pairs (1,2) and (1,3) sharing Z_1
PLAIN = dict(c2=(-0.3, 0.7, -0.2), c1=(0.0, 0.0, 0.0), react=(0.0, 0.0, 0.0), faces=63)
ZERO3 = (0.0, 0.0, 0.0)
DRIFT_CASES = [
    (PLAIN, (), 0, ZERO3, ZERO3, (0,)),
    (dict(PLAIN, c2=(-0.3, 0.0, -0.2)), (), 0, ZERO3, ZERO3, (1,)),
    (PLAIN, (), 0, ZERO3, ZERO3, (2,)),
    CONV_CASES[0] + ((0.8, -0.6, 0.0), (0, 1, 2)),
]


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which,dfaces,conv,cross,axes", DRIFT_CASES)
def test_drift_terms_vs_dense_kronecker_autograd(op, which, dfaces, conv, cross, axes, kind):
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    drift = drift_fields_for(NS, axes)
    for k in axes:
        assert coef["a"][k] is None or not np.array_equal(coef["a"][k], drift[k])
    l, g = loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift)
    la, ga = dense_loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, conv, cross, drift)
    errs = _blocks(g, ga)
    print("opb vs autograd", axes, cross, conv, bin(dfaces), which, kind, abs(l - la) / abs(la), errs)
    assert np.isfinite(l) and all(np.all(np.isfinite(O.flatten_params(g[k]))) for k in g)
    # the term matters: without it the loss is another one
    assert abs(loss_grad_3d_opm(prob, params, op, coef, dfaces, dvals, conv, cross)[0] - l) > 1e-6 * abs(l)
    tol = _tol(prob, params)
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


def test_opb_equation_sources_are_the_operator_applied_to_u():
    """src = sum_k a_k (c2_k d^2 + c1_k d) u / dx_k + sum_k b_k du / dx_k and grad_u = grad u at random
    points, by torch autograd of the solution, to 1e-10; the divergence-form sources are also
    -+div(a grad u) formed directly (which checks divergence_drift)."""
    from gpk import equations as E
    assert E.EQUATIONS_3D_OPB == ["darcy_3d-sin", "heat_div_t-sin", "convdiff_rot_t-sin"]
    sin, cos, exp, pi = torch.sin, torch.cos, torch.exp, np.pi
    u_t = lambda x, y, t: exp(-t) * sin(2 * x) * sin(3 * y)
    tu = {"darcy_3d-sin": lambda x, y, z: sin(2 * x) * sin(3 * y) * sin(z), "heat_div_t-sin": u_t,
          "convdiff_rot_t-sin": u_t}
    # the diffusivity of the divergence-form entries, in torch, and the axes it acts on
    ta = {"darcy_3d-sin": (lambda x, y, z: 1.0 + 0.5 * sin(2 * pi * x) * cos(2 * pi * y) + 0.25 * z, (0, 1, 2), 1.0),
          "heat_div_t-sin": (lambda x, y, t: 0.1 * (1.0 + 0.5 * sin(2 * pi * x) * cos(2 * pi * y)), (0, 1), 1.0)}
    pts = np.random.default_rng(0).uniform(0.05, 0.95, size=(40, 3))
    for e in E.EQUATIONS_3D_OPB:
        u, src, op, dfaces, grad_u, conv, cross, drift = E.solution_3d_opb(e)
        assert len(grad_u) == 3 and len(drift) == 3 and dfaces == 0 and not any(conv) and not any(cross)
        assert all(b is None or callable(b) for b in drift) and any(b is not None for b in drift)
        X = [torch.tensor(pts[:, k], requires_grad=True) for k in range(3)]
        uu = tu[e](*X)
        assert np.allclose(uu.detach().numpy(), u(*pts.T), rtol=0, atol=1e-15)
        a = op.a if isinstance(op, E.Operator3V) else (None, None, None)
        lhs = op.react[0] * uu + op.react[1] * uu ** 2 + op.react[2] * uu ** 3
        gs = []
        for k in range(3):
            g, = torch.autograd.grad(uu.sum(), X[k], create_graph=True)
            gg, = torch.autograd.grad(g.sum(), X[k], create_graph=True)
            gs.append(g)
            ak = 1.0 if a[k] is None else torch.tensor(a[k](*pts.T))
            lhs = lhs + ak * (op.c2[k] * gg + op.c1[k] * g)
            if drift[k] is not None:
                lhs = lhs + torch.tensor(drift[k](*pts.T) * np.ones(len(pts))) * g
            gerr = float(np.max(np.abs(g.detach().numpy() - grad_u[k](*pts.T))))
            assert gerr < 1e-10, (e, k, gerr)
        err = float(np.max(np.abs(lhs.detach().numpy() - src(*pts.T))))
        print(e, "source err", err)
        assert err < 1e-10
        if e in ta:  # u_t - div(a grad u), the flux differentiated by autograd
            fa, axes, _ = ta[e]
            div = 0.0
            for k in axes:
                d, = torch.autograd.grad((fa(*X) * gs[k]).sum(), X[k], create_graph=True)
                div = div + d
            direct = -div + (gs[2] if e == "heat_div_t-sin" else 0.0)
            derr = float(np.max(np.abs(direct.detach().numpy() - src(*pts.T))))
            print(e, "divergence-form err", derr)
            assert derr < 1e-10
    # divergence_drift itself: b_k = c2_k da/dx_k, None where a does not vary or c2_k = 0
    g = (lambda x, y, z: 2.0 * x, None, lambda x, y, z: y + z)
    b = E.divergence_drift(g, (-0.5, 3.0, 0.0))
    assert b[1] is None and b[2] is None and np.array_equal(b[0](*pts.T), -0.5 * 2.0 * pts[:, 0])
    arr = np.arange(24.0).reshape(2, 3, 4)
    assert np.array_equal(E.divergence_drift((arr, arr, None), (2.0, -1.0, 1.0))[1], -arr)
    with pytest.raises(ValueError):
        E.divergence_drift((None, None), (1.0, 1.0, 1.0))
