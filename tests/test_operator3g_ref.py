"""Pins tests/operator3g_ref.py loss_grad_3d_opg (the yardstick of the quadratic-gradient handles' GPU
tests) before anything on the device relies on it: with zero weights it is loss_grad_3d_opq, with weights
it matches torch autograd of the dense-Kronecker log joint whose blocks come from nested autograd of
kappa, a single s_k is a drift term with the field frozen at the current U, and the sources of
equations.EQUATIONS_3D_OPG are their operators applied to their solutions."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import autograd_ref as AR
from tests.helpers import problem_3d
from tests.operator3_ref import FACES
from tests.operator3b_ref import loss_grad_3d_opb
from tests.operator3g_ref import adam_replay_g, criterion_3d_opg, gradient_active, loss_grad_3d_opg
from tests.operator3m_ref import PAIRS
from tests.operator3n_ref import face_data
from tests.operator3q_ref import adam_replay_q, criterion_3d_opq, loss_grad_3d_opq
from tests.test_operator3b_ref import DRIFT_CASES, NS, _setup, drift_fields_for
from tests.test_operator3c_ref import _tol
from tests.test_operator3h_ref import mats4
from tests.test_operator3x_ref import _blocks, _mask

ZERO3 = (0.0, 0.0, 0.0)
NONE3 = (None, None, None)
HIGH = ((0.04, 0.0, -0.02), (-0.15, 0.1, 0.0))
BQ = (2e-3, -1.5e-3, 0.0)


# ---- 1. zero weights: loss_grad_3d_opq itself -------------------------------------------------------
@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("bq", [None, BQ])
def test_zero_gradsq_is_loss_grad_3d_opq_exactly(kind, bq):
    op, which, dfaces, conv, cross, axes = DRIFT_CASES[3]
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    drift = drift_fields_for(NS, axes)
    tq, tg = {}, {}
    lo, go = loss_grad_3d_opq(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, bq, terms=tq)
    for gq in (None, (ZERO3, ZERO3)):
        tg.clear()
        l, g = loss_grad_3d_opg(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, bq, gq, terms=tg)
        assert l == lo and set(tg) == set(tq)
        for k in tq:
            a, b = tg[k], tq[k]
            if isinstance(b, list):
                assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b)), k
            else:
                assert np.array_equal(a, b), k
        for k in go:
            assert np.array_equal(O.flatten_params(g[k]), O.flatten_params(go[k])), k
    assert (criterion_3d_opg(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, bq)
            == criterion_3d_opq(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, bq))
    (la, pa), (lb, pb) = (adam_replay_g(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, bq, None, 2),
                          adam_replay_q(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, bq, 2))
    assert la == lb and np.array_equal(O.flatten_params(pa), O.flatten_params(pb))


# ---- 2. torch autograd of the dense-Kronecker form ------------------------------------------------
def dense_loss_grad_3d_opg(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, bicross, gradsq):
    """tests/test_operator3q_ref.py dense_loss_grad_3d_opq plus s_k ((D1_k in its place) K^{-1} u)^2 and
    x_jk (.)(.), every block by nested autograd of kappa."""
    c4, c3 = high
    gs, gx = gradsq
    tp = AR._tp(params)
    kind = prob["kind"]
    xs = [torch.tensor(prob[f"x{a}"]) for a in (1, 2, 3)]
    Ks, Ds, D1s, D2s = [], [], [], []
    for k in range(3):
        K, (D1, D2, D3, D4) = mats4(kind, xs[k], tp[f"kernel_paras_{k + 1}"], prob["jitter"])
        Ks.append(K)
        D1s.append(D1)
        D2s.append(D2)
        Ds.append(c4[k] * D4 + c3[k] * D3 + op["c2"][k] * D2 + op["c1"][k] * D1)
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
    du = [on_axis(k, D1s[k]) @ Kinv_u for k in range(3)]
    for k in range(3):
        if conv[k] != 0.0:
            R = R + u * (conv[k] * du[k])
    for (j, k), m in zip(PAIRS, cross):
        if m != 0.0:
            f = [D1s[i] if i in (j, k) else Ks[i] for i in range(3)]
            R = R + m * (torch.kron(f[0], torch.kron(f[1], f[2])) @ Kinv_u)
    for k in range(3):
        if drift[k] is not None:
            R = R + fld(drift[k]) * du[k]
    for (j, k), q in zip(PAIRS, bicross):
        if q != 0.0:
            f = [D2s[i] if i in (j, k) else Ks[i] for i in range(3)]
            R = R + q * (torch.kron(f[0], torch.kron(f[1], f[2])) @ Kinv_u)
    for k in range(3):
        if gs[k] != 0.0:
            R = R + gs[k] * du[k] ** 2
    for (j, k), w in zip(PAIRS, gx):
        if w != 0.0:
            R = R + w * du[j] * du[k]
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


PLAIN = dict(c2=(-0.4, 0.7, -0.2), c1=(0.0, 0.0, 1.0), react=(0.0, 0.0, 0.0), faces=63)
ALONE = ([(tuple(0.6 if t == i else 0.0 for t in range(3)), ZERO3) for i in range(3)]
         + [(ZERO3, tuple(-0.7 if t == i else 0.0 for t in range(3))) for i in range(3)])


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_Cos_1d"])
@pytest.mark.parametrize("gq", ALONE, ids=["s1", "s2", "s3", "x12", "x13", "x23"])
def test_each_weight_alone_vs_dense_kronecker_autograd(kind, gq):
    """(5, 4, 3) grid, one s_k or one x_jk; D1 in the dense form from nested autograd of kappa."""
    ns = (5, 4, 3)
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=ns, Q=2, seed=11)
    prob = _mask(prob, ns, PLAIN["faces"])
    # (the seeded U is small and the term quadratic in it; three points across [0, 2 pi] leave D1_3 near zero under
    # an SE factor, so axis 3 is drawn in)
    params = dict(params, U=10.0 * np.asarray(params["U"]))
    prob = dict(prob, x3=np.asarray(prob["x3"], np.float64) / 4.0)
    coef = dict(a=NONE3, rho=None)
    l, g = loss_grad_3d_opg(prob, params, PLAIN, coef, 0, None, None, None, None, None, None, gq)
    la, ga = dense_loss_grad_3d_opg(prob, params, PLAIN, coef, 0, None, ZERO3, ZERO3, NONE3, (ZERO3, ZERO3), ZERO3, gq)
    errs = _blocks(g, ga)
    print("opg", gq, "vs autograd", kind, abs(l - la) / abs(la), errs)
    assert np.isfinite(l) and all(np.all(np.isfinite(O.flatten_params(g[k]))) for k in g)
    tol = _tol(prob, params)
    # the term matters: without it some gradient block moves by over 100 tolerances
    assert max(_blocks(g, loss_grad_3d_opq(prob, params, PLAIN, coef)[1]).values()) > 100 * tol
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_Cos_1d"])
def test_all_six_weights_over_everything_vs_autograd(kind):
    """(6, 5, 4): all six weights over c4, c3, c2, c1, a field, a reaction, convective weights, a cross
    pair, a bi-pair, drift fields, one open face and one derivative face (DRIFT_CASES' last case)."""
    op, which, dfaces, conv, cross, axes = DRIFT_CASES[3]
    assert op["faces"] != 63 and dfaces and any(conv) and any(cross) and any(op["react"]) and which
    gq = ((0.5, -0.3, 0.4), (0.25, -0.35, 0.3))
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    drift = drift_fields_for(NS, axes)
    l, g = loss_grad_3d_opg(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, BQ, gq)
    la, ga = dense_loss_grad_3d_opg(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, BQ, gq)
    errs = _blocks(g, ga)
    print("opg everything vs autograd", kind, abs(l - la) / abs(la), errs)
    without = loss_grad_3d_opq(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, BQ)[1]
    tol = _tol(prob, params)
    assert max(_blocks(g, without).values()) > 100 * tol  # the term matters
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


# ---- 3. the frozen-field identity --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_frozen_field_identity_with_a_drift_term(k, kind):
    """One axis with only s_k != 0 against loss_grad_3d_opb with the drift field frozen at the current U.
    b_k = s_k P_k gives the same residual, so the loss and the tau and v blocks agree to 1e-13.  The
    kernel-parameter blocks of that handle carry dR = s_k P_k dP_k where the quadratic term has 2 s_k P_k
    dP_k, so they are compared on the handle that has both the residual and its derivative right: b_k =
    2 s_k P_k with the source raised by s_k P_k^2 (R = R_0 + 2 s_k P_k^2 - s_k P_k^2).  There the loss and
    every block -- kernel parameters, tau, v and U, Gamma having no direct U term -- agree to 1e-13."""
    op, which, dfaces, conv, cross, axes = DRIFT_CASES[3]
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    sk = (0.6, -0.8, 0.5)[k]
    gq = (tuple(sk if a == k else 0.0 for a in range(3)), ZERO3)
    assert gradient_active(None, gq) == tuple(a == k for a in range(3))
    t = {}
    l, g = loss_grad_3d_opg(prob, params, op, coef, dfaces, dvals, None, cross, None, None, None, gq, terms=t)
    P = t["P"][k]
    without = loss_grad_3d_opq(prob, params, op, coef, dfaces, dvals, None, cross)[1]
    assert max(_blocks(g, without).values()) > 100 * 1e-13  # the term matters at this bar
    # the identity as stated: b_k = s_k P_k
    l1, g1 = loss_grad_3d_opb(prob, params, op, coef, dfaces, dvals, None, cross,
                              tuple(sk * P if a == k else None for a in range(3)))
    assert abs(l - l1) / abs(l1) < 1e-13
    for key in ("log_tau", "log_v"):
        assert abs(g[key] - g1[key]) <= 1e-13 * abs(g1[key]), key
    # and with the derivative right as well
    prob2 = dict(prob, src=np.asarray(prob["src"], np.float64).reshape(NS) + sk * P * P)
    l2, g2 = loss_grad_3d_opb(prob2, params, op, coef, dfaces, dvals, None, cross,
                              tuple(2.0 * sk * P if a == k else None for a in range(3)))
    errs = _blocks(g, g2)
    print("frozen field", k, kind, abs(l - l2) / abs(l2), errs)
    assert abs(l - l2) / abs(l2) < 1e-13
    assert max(errs.values()) < 1e-13, errs


# ---- 4. the equations' sources ----------------------------------------------------------------------
def _torch_u(name):
    """The solutions of EQUATIONS_3D_OPG in torch (equations.py states them in NumPy)."""
    s, e = torch.sin, torch.exp
    steady = lambda x, y, z: s(2 * x) * s(3 * y) * s(z)
    decay = lambda x, y, t: e(-t) * s(2 * x) * s(3 * y)
    return {"eikonal_3d-sin": steady, "aniso_eikonal_3d-sin": steady, "hj_t-sin": decay, "kpz_t-sin": decay,
            "ks_int_t-sin": decay}[name]


def test_equations_3d_opg_sources_are_the_operator_applied_to_u():
    from gpk import equations as E
    assert E.EQUATIONS_3D_OPG == ["eikonal_3d-sin", "hj_t-sin", "kpz_t-sin", "aniso_eikonal_3d-sin", "ks_int_t-sin"]
    older = (E.EQUATIONS_3D + E.EQUATIONS_3D_OP + E.EQUATIONS_3D_OPX + E.EQUATIONS_3D_OPV + E.EQUATIONS_3D_OPN
             + E.EQUATIONS_3D_OPC + E.EQUATIONS_3D_OPM + E.EQUATIONS_3D_OPB + E.EQUATIONS_3D_OPH + E.EQUATIONS_3D_OPQ)
    assert not set(E.EQUATIONS_3D_OPG) & set(older)
    assert not {e.split("-")[0] for e in E.EQUATIONS_3D_OPG} & {e.split("-")[0] for e in older}
    rng = np.random.default_rng(7)
    want = {"eikonal_3d-sin": ((1.0, 1.0, 1.0), ZERO3), "hj_t-sin": ((0.5, 0.5, 0.0), ZERO3),
            "kpz_t-sin": ((-0.5, -0.5, 0.0), ZERO3), "aniso_eikonal_3d-sin": ((1.0, 0.5, 2.0), (0.6, 0.0, -0.4)),
            "ks_int_t-sin": ((0.5, 0.5, 0.0), ZERO3)}
    for name in E.EQUATIONS_3D_OPG:
        u, src, op, dfaces, grad_u, conv, cross, drift, high, bq, gq = E.solution_3d_opg(name)
        assert not any(conv) and not any(cross) and all(b is None for b in drift)
        assert (tuple(gq[0]), tuple(gq[1])) == want[name]
        assert op.faces == (63 if "3d" in name else 0b011111)
        P = rng.uniform(0.0, 1.0, (3, 40))
        X = [torch.tensor(P[k], requires_grad=True) for k in range(3)]
        ut = _torch_u(name)(*X)
        assert np.allclose(ut.detach().numpy(), u(*P), rtol=0, atol=1e-14)

        def d(f, k, n):
            for _ in range(n):
                f, = torch.autograd.grad(f.sum(), X[k], create_graph=True)
            return f
        L = sum(w * d(ut, k, n) for n, ws in ((4, high[0]), (3, high[1]), (2, op.c2), (1, op.c1))
                for k, w in enumerate(ws) if w != 0.0)
        L = L + sum(q * d(d(ut, j, 2), k, 2) for (j, k), q in zip(PAIRS, bq) if q != 0.0)
        L = L + op.react[0] * ut + op.react[1] * ut ** 2 + op.react[2] * ut ** 3
        L = L + sum(w * d(ut, k, 1) ** 2 for k, w in enumerate(gq[0]) if w != 0.0)
        L = L + sum(w * d(ut, j, 1) * d(ut, k, 1) for (j, k), w in zip(PAIRS, gq[1]) if w != 0.0)
        err = np.abs(L.detach().numpy() - src(*P)).max()
        print(name, "source vs autograd", err)
        assert err < 1e-10, (name, err)
        for k in range(3):
            assert np.allclose(d(ut, k, 1).detach().numpy(), grad_u[k](*P), rtol=0, atol=1e-13)
    # the equations as the issue states them: eps = 0.1, nu = 0.05, lambda = 1; ks_int in swift_hohenberg's layout
    assert E.solution_3d_opg("eikonal_3d-sin")[2].c2 == (-0.1, -0.1, -0.1)
    assert E.solution_3d_opg("hj_t-sin")[2].c2 == (-0.05, -0.05, 0.0) and E.solution_3d_opg("hj_t-sin")[2].c1 == (0.0, 0.0, 1.0)
    ks, sh = E.solution_3d_opg("ks_int_t-sin"), E.solution_3d_opq("swift_hohenberg_t-sin")
    assert ks[2].c2 == sh[2].c2 and ks[2].c1 == sh[2].c1 and ks[3] == sh[3] == 0b001111 and ks[8] == sh[8] and ks[9] == sh[9]
    assert ks[2].faces == sh[2].faces and not any(ks[2].react)
