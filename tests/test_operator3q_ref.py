"""Pins tests/operator3q_ref.py loss_grad_3d_opq (the yardstick of the bi-pair handles' GPU tests) before
anything on the device relies on it: with zero weights it is loss_grad_3d_oph, with weights it matches
torch autograd of the dense-Kronecker log joint whose blocks come from nested autograd of kappa, and
the sources of equations.EQUATIONS_3D_OPQ are their operators applied to their solutions."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import autograd_ref as AR
from tests.helpers import problem_3d
from tests.operator3_ref import FACES
from tests.operator3h_ref import adam_replay_h, criterion_3d_oph, loss_grad_3d_oph
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


# ---- 1. zero weights: loss_grad_3d_oph itself -------------------------------------------------------
@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("high", [None, HIGH])
def test_zero_bicross_is_loss_grad_3d_oph_exactly(kind, high):
    op, which, dfaces, conv, cross, axes = DRIFT_CASES[3]
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    drift = drift_fields_for(NS, axes)
    th, tq = {}, {}
    lo, go = loss_grad_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, terms=th)
    for bq in (None, ZERO3):
        tq.clear()
        l, g = loss_grad_3d_opq(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, bq, terms=tq)
        assert l == lo and set(tq) == set(th)
        assert all(np.array_equal(tq[k], th[k]) for k in th)
        for k in go:
            assert np.array_equal(O.flatten_params(g[k]), O.flatten_params(go[k])), k
    assert (criterion_3d_opq(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high)
            == criterion_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high))
    (la, pa), (lb, pb) = (adam_replay_q(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, None, 2),
                          adam_replay_h(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, 2))
    assert la == lb and np.array_equal(O.flatten_params(pa), O.flatten_params(pb))


# ---- 2. torch autograd of the dense-Kronecker form ------------------------------------------------
def dense_loss_grad_3d_opq(prob, params, op, coef, dfaces, dvals, conv, cross, drift, high, bicross):
    """tests/test_operator3h_ref.py dense_loss_grad_3d_oph plus q (DD_j (x) DD_k (x) K_l in their places)
    K^{-1} u per pair, every block by nested autograd of kappa."""
    c4, c3 = high
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
    for (j, k), q in zip(PAIRS, bicross):
        if q != 0.0:
            f = [D2s[i] if i in (j, k) else Ks[i] for i in range(3)]
            R = R + q * (torch.kron(f[0], torch.kron(f[1], f[2])) @ Kinv_u)
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


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_Cos_1d"])
@pytest.mark.parametrize("pair", [0, 1, 2])
def test_each_pair_alone_vs_dense_kronecker_autograd(kind, pair):
    """(5, 4, 3) grid, one bi-pair; DD in the dense form from nested autograd of kappa."""
    ns = (5, 4, 3)
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=ns, Q=2, seed=11)
    prob = _mask(prob, ns, PLAIN["faces"])
    coef = dict(a=NONE3, rho=None)
    bq = tuple(3e-3 if t == pair else 0.0 for t in range(3))
    l, g = loss_grad_3d_opq(prob, params, PLAIN, coef, 0, None, None, None, None, None, bq)
    la, ga = dense_loss_grad_3d_opq(prob, params, PLAIN, coef, 0, None, ZERO3, ZERO3, NONE3, (ZERO3, ZERO3), bq)
    errs = _blocks(g, ga)
    print("opq pair", pair, "vs autograd", kind, abs(l - la) / abs(la), errs)
    assert np.isfinite(l) and all(np.all(np.isfinite(O.flatten_params(g[k]))) for k in g)
    assert abs(loss_grad_3d_oph(prob, params, PLAIN, coef)[0] - l) > 1e-6 * abs(l)  # the term matters
    tol = _tol(prob, params)
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_Cos_1d"])
def test_all_three_pairs_over_everything_vs_autograd(kind):
    """(6, 5, 4): all three bi-pairs over c4, c3, c2, c1, a field, a reaction, convective weights, a
    cross pair, drift fields, one open face and one derivative face (DRIFT_CASES' last case)."""
    op, which, dfaces, conv, cross, axes = DRIFT_CASES[3]
    assert op["faces"] != 63 and dfaces and any(conv) and any(cross) and any(op["react"]) and which
    bq = (2e-3, -1.5e-3, 1e-3)
    prob, params, coef, dvals = _setup(op, which, dfaces, kind)
    drift = drift_fields_for(NS, axes)
    l, g = loss_grad_3d_opq(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, bq)
    la, ga = dense_loss_grad_3d_opq(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH, bq)
    errs = _blocks(g, ga)
    print("opq everything vs autograd", kind, abs(l - la) / abs(la), errs)
    assert abs(loss_grad_3d_oph(prob, params, op, coef, dfaces, dvals, conv, cross, drift, HIGH)[0] - l) > 1e-6 * abs(l)
    tol = _tol(prob, params)
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


# ---- 3. the equations' sources ----------------------------------------------------------------------
def _torch_u(name):
    """The solutions of EQUATIONS_3D_OPQ in torch (equations.py states them in NumPy)."""
    s, e = torch.sin, torch.exp
    return {"plate_t-sin": lambda x, y, t: s(2 * x) * s(3 * y) * s(2.0 * t + 0.5),
            "biharmonic_3d-sin": lambda x, y, z: s(2 * x) * s(3 * y) * s(z),
            "swift_hohenberg_t-sin": lambda x, y, t: e(-t) * s(2 * x) * s(3 * y),
            "mixed4_3d-sin": lambda x, y, z: s(2 * x) * s(3 * y) * s(z)}[name]


def test_equations_3d_opq_sources_are_the_operator_applied_to_u():
    from gpk.equations import EQUATIONS_3D_OPQ, solution_3d_opq
    assert EQUATIONS_3D_OPQ == ["plate_t-sin", "biharmonic_3d-sin", "swift_hohenberg_t-sin", "mixed4_3d-sin"]
    rng = np.random.default_rng(7)
    for name in EQUATIONS_3D_OPQ:
        u, src, op, dfaces, grad_u, conv, cross, drift, high, bq = solution_3d_opq(name)
        assert not any(conv) and not any(cross) and all(b is None for b in drift)
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
        err = np.abs(L.detach().numpy() - src(*P)).max()
        print(name, "source vs autograd", err)
        assert err < 1e-10, (name, err)
        for k in range(3):
            assert np.allclose(d(ut, k, 1).detach().numpy(), grad_u[k](*P), rtol=0, atol=1e-13)
