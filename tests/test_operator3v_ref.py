"""Pins tests/operator3v_ref.py loss_grad_3d_opv (the yardstick of the coefficient-field handles'
GPU tests) before anything on the device relies on it: it is loss_grad_3d_opx without fields and
with constant ones, it matches torch autograd of the dense-Kronecker log joint with fields that
vary, and the manufactured sources of equations.EQUATIONS_3D_OPV are their operators applied to
their solutions."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from tests import autograd_ref as AR
from tests.helpers import problem_3d, rel
from tests.operator3_ref import FACES
from tests.operator3v_ref import adam_replay_v, criterion_3d_opv, loss_grad_3d_opv
from tests.operator3x_ref import adam_replay_x, criterion_3d_opx, loss_grad_3d_opx
from tests.test_operator3x_ref import MIXED_CASES, ONE_ORDER, _blocks, _mask


def smooth_fields(ns, which, seed=0):
    """Smooth non-constant fields of both signs on the axes in `which` (3: rho) over [0, 1]^3
    index coordinates: low-order trigonometric products with seeded amplitudes and an offset small
    enough that each field changes sign."""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in ns], indexing="ij")
    out = []
    for k in range(4):
        if k not in which:
            out.append(None)
            continue
        am, ph = rng.uniform(0.5, 1.5, 3), rng.uniform(0.0, 2 * np.pi, 3)
        f = 0.3 + am[0] * np.sin(2 * g[0] + ph[0]) * np.cos(3 * g[1] + ph[1]) + 0.4 * am[2] * np.sin(4 * g[2] + ph[2])
        assert f.min() < 0.0 < f.max()
        out.append(f)
    return dict(a=tuple(out[:3]), rho=out[3])


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op", ONE_ORDER[2:3] + MIXED_CASES[3:])
def test_no_fields_is_loss_grad_3d_opx_exactly(op, kind):
    ns = (9, 7, 6)
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=ns, Q=3, seed=4)
    prob = _mask(prob, ns, op["faces"])
    tx, tv = {}, {}
    lo, go = loss_grad_3d_opx(prob, params, op, terms=tx)
    for coef in (None, dict(a=(None, None, None), rho=None)):
        l, g = loss_grad_3d_opv(prob, params, op, coef, terms=tv)
        assert l == lo and tv == tx
        for k in go:
            assert np.array_equal(O.flatten_params(g[k]), O.flatten_params(go[k])), k
    assert criterion_3d_opv(prob, params, op, None) == criterion_3d_opx(prob, params, op)
    (la, pa), (lb, pb) = adam_replay_v(prob, params, op, None, 2), adam_replay_x(prob, params, op, 2)
    assert la == lb and np.array_equal(O.flatten_params(pa), O.flatten_params(pb))


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op", ONE_ORDER[:3] + MIXED_CASES[1:2] + MIXED_CASES[4:])
def test_constant_fields_are_weights(op, kind):
    """a_k = alpha_k and rho = rho_0 everywhere: loss_grad_3d_opx with weights alpha_k c2_k,
    alpha_k c1_k and react[0] + rho_0, at that file's 1e-13 bar."""
    ns = (9, 7, 6)
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=ns, Q=3, seed=4)
    prob = _mask(prob, ns, op["faces"])
    al, rho0 = (0.7, -1.3, 2.1), -0.45
    coef = dict(a=tuple(np.full(ns, a) for a in al), rho=np.full(ns, rho0))
    opc = dict(op, c2=tuple(a * c for a, c in zip(al, op["c2"])), c1=tuple(a * c for a, c in zip(al, op["c1"])),
               react=(op["react"][0] + rho0,) + tuple(op["react"][1:]))
    lo, go = loss_grad_3d_opx(prob, params, opc)
    l, g = loss_grad_3d_opv(prob, params, op, coef)
    errs = _blocks(g, go)
    print("opv constant fields vs opx", op["c2"], op["c1"], kind, abs(l - lo) / abs(lo), errs)
    assert abs(l - lo) / abs(lo) <= 1e-13
    assert max(errs.values()) <= 1e-13


def dense_loss_grad_3d_opv(prob, params, op, coef):
    """tests/test_operator3x_ref.py dense_loss_grad_3d_opx with diag(a_k) on each axis's DENSE
    Kronecker term and rho on u; the log-det of K itself, torch autograd."""
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
    log_prior = -0.5 * torch.linalg.slogdet(K)[1] * prob["logdet"] - 0.5 * (u * Kinv_u).sum()
    log_b = 0.5 * Nb * tp["log_tau"] - 0.5 * torch.exp(tp["log_tau"]) * bgap
    eq_ll = 0.5 * u.numel() * tp["log_v"] - 0.5 * torch.exp(tp["log_v"]) * egap
    loss = -(log_prior + log_b * prob["llk_weight"] + eq_ll)
    loss.backward()
    return float(loss.detach()), AR._grads(tp)


# fields on one, two and three axes (+ rho), on a one-order operator, a mixed axis under a field,
# a reaction, one face open; rho alone
FIELD_CASES = [
    (dict(c2=(1.0, 1.0, 1.0), c1=(0.0, 0.0, 0.0), react=(0.0, 0.0, 0.0), faces=63), (3,)),          # rho alone
    (dict(c2=(-0.3, 0.0, 1.0), c1=(0.8, -0.7, 0.0), react=(0.0, 0.0, 0.0), faces=63), (0,)),         # one axis (mixed)
    (dict(c2=(-0.1, -0.1, 0.0), c1=(0.0, 0.0, 1.0), react=(0.0, 0.0, 0.0), faces=0b011111), (0, 1)),  # two (heat form)
    (dict(c2=(0.0, -0.2, 0.9), c1=(1.0, 0.0, -0.4), react=(0.4, -0.5, 0.2), faces=0b111011), (1, 2, 3)),
    (dict(c2=(-0.3, 0.7, -0.2), c1=(0.8, -0.6, 1.3), react=(0.4, -0.5, 0.2), faces=0b011111), (0, 1, 2, 3)),
]


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("op,which", FIELD_CASES)
def test_fields_vs_dense_kronecker_autograd(op, which, kind):
    ns = (6, 5, 4)
    prob, params, _ = problem_3d(eq="poisson", kind=kind, ns=ns, Q=2, seed=11)
    prob = _mask(prob, ns, op["faces"])
    coef = smooth_fields(ns, which, seed=len(which))
    l, g = loss_grad_3d_opv(prob, params, op, coef)
    la, ga = dense_loss_grad_3d_opv(prob, params, op, coef)
    errs = _blocks(g, ga)
    print("opv vs autograd", op["c2"], op["c1"], which, bin(op["faces"]), kind, abs(l - la) / abs(la), errs)
    assert np.isfinite(l) and all(np.all(np.isfinite(O.flatten_params(g[k]))) for k in g)
    # the fields matter: without them the loss is another one
    assert abs(loss_grad_3d_opx(prob, params, op)[0] - l) > 1e-6 * abs(l)
    # the three-axis bar of tests/test_operator3_ref.py
    conds = [np.linalg.cond(O.kernel_matrix(kind, prob[f"x{a}"], params[f"kernel_paras_{a}"], prob["jitter"]))
             for a in (1, 2, 3)]
    tol = min(1e-9, max(1e-11, 100 * float(np.prod(conds)) * np.finfo(float).eps))
    assert abs(l - la) / abs(la) < tol, (l, la, tol)
    assert max(errs.values()) < tol, (errs, tol)


def test_opv_equation_sources_are_the_operator_applied_to_u():
    """src = sum_k a_k (c2_k d^2 + c1_k d) u / dx_k + (r1 + rho) u + r2 u^2 + r3 u^3 at random
    points, by torch autograd of the solution, to 1e-10."""
    from gpk import equations as E
    assert E.EQUATIONS_3D_OPV == ["helmholtz_var-sin", "heat_var-sin", "transport_var-sin"]
    heat = lambda x, y, t: torch.exp(-t) * torch.sin(2 * x) * torch.sin(3 * y)
    tu = {"helmholtz_var-sin": lambda x, y, z: torch.sin(2 * x) * torch.sin(3 * y) * torch.sin(z),
          "heat_var-sin": heat, "transport_var-sin": heat}
    pts = np.random.default_rng(0).uniform(0.05, 0.95, size=(40, 3))
    for e in E.EQUATIONS_3D_OPV:
        u, src, op = E.solution_3d_opv(e)
        assert isinstance(op, E.Operator3V)
        a = [None if f is None else f(*pts.T) for f in op.a]
        rho = 0.0 if op.rho is None else op.rho(*pts.T)
        X = [torch.tensor(pts[:, k], requires_grad=True) for k in range(3)]
        uu = tu[e](*X)
        assert np.allclose(uu.detach().numpy(), u(*pts.T), rtol=0, atol=1e-15)
        lhs = (op.react[0] + torch.tensor(rho)) * uu + op.react[1] * uu ** 2 + op.react[2] * uu ** 3
        for k in range(3):
            g, = torch.autograd.grad(uu.sum(), X[k], create_graph=True)
            gg, = torch.autograd.grad(g.sum(), X[k], create_graph=True)
            t = op.c2[k] * gg + op.c1[k] * g
            lhs = lhs + (t if a[k] is None else torch.tensor(a[k]) * t)
        err = float(np.max(np.abs(lhs.detach().numpy() - src(*pts.T))))
        print(e, "source err", err)
        assert err < 1e-10
    hv, ht, tr = (E.solution_3d_opv(e)[2] for e in E.EQUATIONS_3D_OPV)
    assert hv.has == (False, False, False, True) and hv.faces == 63 and hv.c2 == (1.0, 1.0, 1.0)
    assert ht.has == (True, True, False, False) and ht.faces == 0b011111 and ht.c1 == (0.0, 0.0, 1.0)
    assert tr.has == (True, True, False, False) and tr.faces == 0b011111 and tr.c2 == (0.0, 0.0, 0.0)
    # k^2 = 16 (1 + x / 2) <= 24 < 3 pi^2 on [0, 1]: lap + k^2 stays definite on the unit cube
    x = np.linspace(0.0, 1.0, 101)
    assert hv.rho(x, x, x).max() == 24.0 < 3 * np.pi ** 2
    # nu(x, y) > 0 and the flow rotates about the centre
    assert ht.a[0](x[:, None], x[None, :], 0.0).min() >= 0.5
    assert tr.a[0](0.5, 0.75, 0.0) == -0.25 and tr.a[1](0.75, 0.5, 0.0) == 0.25
