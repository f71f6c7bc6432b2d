"""Pins tests/operator3n_ref.py loss_grad_3d_opn (the yardstick of the derivative-boundary-data
handles' GPU tests) before anything on the device relies on it: without derivative faces it is
loss_grad_3d_opv, with them it matches torch autograd of the dense-Kronecker log joint, and the
sources and gradients of equations.EQUATIONS_3D_OPN are those of their solutions."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import autograd_ref as AR
from tests.helpers import problem_3d
from tests.operator3_ref import FACES
from tests.operator3n_ref import adam_replay_n, criterion_3d_opn, face_data, loss_grad_3d_opn
from tests.operator3v_ref import adam_replay_v, criterion_3d_opv, loss_grad_3d_opv
from tests.test_operator3v_ref import FIELD_CASES, smooth_fields
from tests.test_operator3x_ref import _blocks, _mask


def random_dvals(ns, dfaces, seed=0):
    """Seeded data on the faces of dfaces, NaN everywhere else (never read)."""
    rng = np.random.default_rng(seed)
    out = []
    for f, sl in enumerate(FACES):
        n = np.zeros(ns)[sl].size
        out.append(rng.normal(size=n) if (dfaces >> f) & 1 else np.full(n, np.nan))
    return np.concatenate(out)


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which", FIELD_CASES[1:2] + FIELD_CASES[4:])
def test_no_derivative_faces_is_loss_grad_3d_opv_exactly(op, which, kind):
    ns = (6, 5, 4)
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=ns, Q=2, seed=11)
    prob = _mask(prob, ns, op["faces"])
    coef = smooth_fields(ns, which, seed=len(which))
    tv, tn = {}, {}
    lo, go = loss_grad_3d_opv(prob, params, op, coef, terms=tv)
    for dvals in (None, np.full(np.asarray(prob["bvals"]).size, np.nan)):
        l, g = loss_grad_3d_opn(prob, params, op, coef, 0, dvals, terms=tn)
        assert l == lo and tn == tv
        for k in go:
            assert np.array_equal(O.flatten_params(g[k]), O.flatten_params(go[k])), k
    assert criterion_3d_opn(prob, params, op, coef) == criterion_3d_opv(prob, params, op, coef)
    (la, pa), (lb, pb) = adam_replay_n(prob, params, op, coef, 0, None, 2), adam_replay_v(prob, params, op, coef, 2)
    assert la == lb and np.array_equal(O.flatten_params(pa), O.flatten_params(pb))


def dense_loss_grad_3d_opn(prob, params, op, coef, dfaces, dvals):
    """tests/test_operator3v_ref.py dense_loss_grad_3d_opv with the derivative faces' term: the
    prediction g_f is row i_f of autograd's D1_k contracted with K_k^{-1} x_k U along axis k."""
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
    D1, D2, D3 = Ds
    U = tp["U"]
    u = U.reshape(-1)
    fld = lambda f: torch.ones_like(u) if f is None else torch.tensor(np.asarray(f, np.float64).reshape(-1))
    a1, a2, a3 = (fld(f) for f in coef["a"])
    K = torch.kron(K1, torch.kron(K2, K3))
    Kinv_u = torch.linalg.solve(K, u)
    L = (a1 * (torch.kron(D1, torch.kron(K2, K3)) @ Kinv_u) + a2 * (torch.kron(K1, torch.kron(D2, K3)) @ Kinv_u)
         + a3 * (torch.kron(K1, torch.kron(K2, D3)) @ Kinv_u))
    r1, r2, r3 = op["react"]
    R = L - torch.tensor(prob["src"]).reshape(-1) + r1 * u + r2 * u ** 2 + r3 * u ** 3
    if coef["rho"] is not None:
        R = R + fld(coef["rho"]) * u
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
    for f, h in face_data(dvals, ns, dfaces).items():
        k, s = divmod(f, 2)
        Ak = torch.linalg.solve(Ks[k], torch.movedim(U, k, 0).reshape(ns[k], -1))  # K_k^{-1} x_k U, unfolded
        g = D1s[k][ns[k] - 1 if s else 0] @ Ak
        bgap = bgap + ((g - torch.tensor(h).reshape(-1)) ** 2).sum()
        Nb += g.numel()
    log_prior = -0.5 * torch.linalg.slogdet(K)[1] * prob["logdet"] - 0.5 * (u * Kinv_u).sum()
    log_b = 0.5 * Nb * tp["log_tau"] - 0.5 * torch.exp(tp["log_tau"]) * bgap
    eq_ll = 0.5 * u.numel() * tp["log_v"] - 0.5 * torch.exp(tp["log_v"]) * egap
    loss = -(log_prior + log_b * prob["llk_weight"] + eq_ll)
    loss.backward()
    return float(loss.detach()), AR._grads(tp)


_MIXED_FIELDS = dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, -0.6, 1.3), react=(0.4, -0.5, 0.2))
# (operator, fields on, dfaces): derivative faces on all three axes with a mixed-order axis under
# a field and a reaction (faces 1 and 4 carry both kinds); both faces of one axis; one face with
# both kinds of data on a one-order operator; no value data at all (Helmholtz with a reaction)
DERIV_CASES = [
    (dict(_MIXED_FIELDS, faces=0b011011), (0, 1, 2, 3), 0b110110),
    (dict(c2=(-0.1, -0.1, 0.0), c1=(0.0, 0.0, 1.0), react=(0.0, 0.0, 0.0), faces=0b011111), (0, 1), 0b001100),
    (dict(c2=(-0.25, -0.25, 1.0), c1=(0.0, 0.0, 0.0), react=(0.0, 0.0, 0.0), faces=0b011111), (), 0b010000),
    (dict(c2=(1.0, 1.0, 1.0), c1=(0.0, 0.0, 0.0), react=(9.0, 0.0, 0.0), faces=0), (3,), 63),
]


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which,dfaces", DERIV_CASES)
def test_derivative_faces_vs_dense_kronecker_autograd(op, which, dfaces, kind):
    ns = (6, 5, 4)
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=ns, Q=2, seed=11)
    prob = _mask(prob, ns, op["faces"])
    coef = smooth_fields(ns, which, seed=len(which))
    dvals = random_dvals(ns, dfaces, seed=dfaces)
    t = {}
    l, g = loss_grad_3d_opn(prob, params, op, coef, dfaces, dvals, terms=t)
    la, ga = dense_loss_grad_3d_opn(prob, params, op, coef, dfaces, dvals)
    errs = _blocks(g, ga)
    print("opn vs autograd", bin(op["faces"]), bin(dfaces), which, kind, abs(l - la) / abs(la), errs)
    assert np.isfinite(l) and all(np.all(np.isfinite(O.flatten_params(g[k]))) for k in g)
    assert t["Nd"] == sum(np.zeros(ns)[sl].size for f, sl in enumerate(FACES) if (dfaces >> f) & 1)
    assert t["dgap"] > 0.0
    # the data matters: with other derivative values the loss is another one
    assert abs(loss_grad_3d_opn(prob, params, op, coef, dfaces, 0.5 * np.nan_to_num(dvals))[0] - l) > 1e-6 * abs(l)
    # the three-axis bar of tests/test_operator3_ref.py
    conds = [np.linalg.cond(O.kernel_matrix(kind, prob[f"x{a}"], params[f"kernel_paras_{a}"], prob["jitter"]))
             for a in (1, 2, 3)]
    tol = min(1e-9, max(1e-11, 100 * float(np.prod(conds)) * np.finfo(float).eps))
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


def test_opn_equation_sources_and_gradients_are_those_of_u():
    """src = sum_k (c2_k d^2 + c1_k d) u / dx_k + r1 u + r2 u^2 + r3 u^3 and grad_u = grad u at
    random points, by torch autograd of the solution, to 1e-10."""
    from gpk import equations as E
    assert E.EQUATIONS_3D_OPN == ["wave_t-sin", "helmholtz_neumann-sin"]
    tu = {"wave_t-sin": lambda x, y, t: torch.sin(2 * x) * torch.sin(3 * y) * torch.sin(E._WAVE_OM * t + 0.5),
          "helmholtz_neumann-sin": lambda x, y, z: torch.sin(2 * x) * torch.sin(3 * y) * torch.sin(z)}
    pts = np.random.default_rng(0).uniform(0.05, 0.95, size=(40, 3))
    for e in E.EQUATIONS_3D_OPN:
        u, src, op, dfaces, grad_u = E.solution_3d_opn(e)
        assert isinstance(op, E.Operator3X) and len(grad_u) == 3
        X = [torch.tensor(pts[:, k], requires_grad=True) for k in range(3)]
        uu = tu[e](*X)
        assert np.allclose(uu.detach().numpy(), u(*pts.T), rtol=0, atol=1e-15)
        lhs = op.react[0] * uu + op.react[1] * uu ** 2 + op.react[2] * uu ** 3
        for k in range(3):
            g, = torch.autograd.grad(uu.sum(), X[k], create_graph=True)
            gg, = torch.autograd.grad(g.sum(), X[k], create_graph=True)
            lhs = lhs + op.c2[k] * gg + op.c1[k] * g
            gerr = float(np.max(np.abs(g.detach().numpy() - grad_u[k](*pts.T))))
            print(e, "grad err axis", k, gerr)
            assert gerr < 1e-10
        err = float(np.max(np.abs(lhs.detach().numpy() - src(*pts.T))))
        print(e, "source err", err)
        assert err < 1e-10
    wave, helm = (E.solution_3d_opn(e) for e in E.EQUATIONS_3D_OPN)
    c2 = E._WAVE_C ** 2
    assert wave[2] == E.Operator3X((-c2, -c2, 1.0), (0.0, 0.0, 0.0), faces=0b011111) and wave[3] == 0b010000
    assert helm[2].faces == 0b111100 and helm[3] == 0b000011 and helm[2].c2 == (1.0, 1.0, 1.0)
    # the helper lays grad_u out face by face, NaN on the faces outside dfaces
    axes = [np.linspace(0.0, 1.0, n) for n in (4, 3, 5)]
    d = E.deriv_boundary_3d(wave[4], axes, wave[3])
    hs = face_data(d, (4, 3, 5), wave[3])
    X, Y = np.meshgrid(axes[0], axes[1], indexing="ij")
    assert list(hs) == [4] and np.array_equal(hs[4], wave[4][2](X, Y, 0.0 * X))
    assert np.isnan(d).sum() == d.size - 12
    d = E.deriv_boundary_3d(helm[4], axes, helm[3])
    hs = face_data(d, (4, 3, 5), helm[3])
    Y, Z = np.meshgrid(axes[1], axes[2], indexing="ij")
    assert np.array_equal(hs[0], helm[4][0](0.0 * Y, Y, Z)) and np.array_equal(hs[1], helm[4][0](0.0 * Y + 1.0, Y, Z))
