"""The reference's equation_dict entries with their PDE source terms.

The reference builds sources by differentiating the exact solution with jax.grad
(code/model_GP_solver_1d.py:299-307, code/model_GP_solver_2d.py:355-366,
code/model_GP_solver_advection.py:354-362).  Here each exact solution carries its analytic
derivatives (host-side setup, not the hot path); `autodiff_source_*` offers the same
autodiff construction for user-supplied torch-expressible solutions.
"""
import numpy as np

s_, c_ = np.sin, np.cos

# name -> (u, u_x, u_xx) for 1D solutions  (code/model_GP_solver_1d.py:313-332)
_U1D = {
    "mix_sin": (lambda x: s_(x) + 0.1 * s_(20 * x) + 0.05 * s_(100 * x),
                lambda x: c_(x) + 2.0 * c_(20 * x) + 5.0 * c_(100 * x),
                lambda x: -s_(x) - 40.0 * s_(20 * x) - 500.0 * s_(100 * x)),
    "single_sin": (lambda x: s_(100 * x), lambda x: 100.0 * c_(100 * x),
                   lambda x: -1e4 * s_(100 * x)),
    "sin_cos": (lambda x: s_(6 * x) * c_(100 * x),
                lambda x: 6.0 * c_(6 * x) * c_(100 * x) - 100.0 * s_(6 * x) * s_(100 * x),
                lambda x: -10036.0 * s_(6 * x) * c_(100 * x) - 1200.0 * c_(6 * x) * s_(100 * x)),
    "x_time_sinx": (lambda x: x * s_(200 * x), lambda x: s_(200 * x) + 200.0 * x * c_(200 * x),
                    lambda x: 400.0 * c_(200 * x) - 40000.0 * x * s_(200 * x)),
    "x2_add_sinx": (lambda x: s_(500 * x) - 2 * (x - 0.5) ** 2,
                    lambda x: 500.0 * c_(500 * x) - 4.0 * (x - 0.5),
                    lambda x: -250000.0 * s_(500 * x) - 4.0),
    "x_time_sinx_scale": (lambda x: x * s_(200 * x * np.pi),
                          lambda x: s_(200 * np.pi * x) + 200 * np.pi * x * c_(200 * np.pi * x),
                          lambda x: 400 * np.pi * c_(200 * np.pi * x)
                          - (200 * np.pi) ** 2 * x * s_(200 * np.pi * x)),
}

EQUATIONS_1D = [
    "poisson_1d-mix_sin", "poisson_1d-single_sin", "poisson_1d-sin_cos", "poisson_1d-x_time_sinx",
    "poisson_1d-x2_add_sinx", "allencahn_1d-sin_cos", "allencahn_1d-single_sin",
]
EQUATIONS_2D = ["poisson_2d-sin_cos", "poisson_2d-sin_sin", "poisson_2d-sin_add_cos",
                "allencahn_2d-mix-sincos"]
EQUATIONS_ADV = ["advection-sin"]


def solution_1d(equation):
    """(u, src) with src = u'' (Poisson) or u'' + u(u^2-1) (Allen-Cahn)."""
    kind, name = equation.split("-", 1)
    u, _, uxx = _U1D[name]
    if kind == "allencahn_1d":
        return u, (lambda x: uxx(x) + u(x) * (u(x) ** 2 - 1.0))
    if kind == "poisson_1d":
        return u, uxx
    raise KeyError(equation)


def solution_2d(equation, beta=None):
    """(u, src) for the 2D Poisson / Allen-Cahn / advection equations."""
    if equation == "poisson_2d-sin_sin":
        return (lambda x, y: s_(100 * x) * s_(100 * y)), (lambda x, y: -2e4 * s_(100 * x) * s_(100 * y))
    if equation == "poisson_2d-sin_cos":
        return (lambda x, y: s_(100 * x) * c_(100 * y)), (lambda x, y: -2e4 * s_(100 * x) * c_(100 * y))
    if equation == "poisson_2d-sin_add_cos":
        g = lambda t: s_(6 * t) * c_(20 * t)
        g2 = lambda t: -436.0 * s_(6 * t) * c_(20 * t) - 240.0 * c_(6 * t) * s_(20 * t)
        return (lambda x, y: g(x) + g(y)), (lambda x, y: g2(x) + g2(y))
    if equation == "allencahn_2d-mix-sincos":
        g = lambda t: s_(t) + 0.1 * s_(20 * t) + c_(100 * t)
        g2 = lambda t: -s_(t) - 40.0 * s_(20 * t) - 1e4 * c_(100 * t)
        u = lambda x, y: g(x) * g(y)
        return u, (lambda x, y: g2(x) * g(y) + g(x) * g2(y) + u(x, y) * (u(x, y) ** 2 - 1.0))
    if equation == "advection-sin":
        # beta*u_x + u_y of sin(x - beta*y) vanishes identically (advection.py:386-388)
        return (lambda x, y: s_(x - beta * y)), (lambda x, y: 0.0 * x * y)
    if equation == "advection-multiscale":
        # synthetic multi-scale source for config C5
        u = lambda x, y: s_(x - beta * y) + 0.1 * s_(20 * np.pi * x) * s_(2 * np.pi * y)
        f = lambda x, y: (beta * 0.1 * 20 * np.pi * c_(20 * np.pi * x) * s_(2 * np.pi * y)
                          + 0.1 * s_(20 * np.pi * x) * 2 * np.pi * c_(2 * np.pi * y))
        return u, f
    raise KeyError(equation)


EQUATIONS_3D = ["poisson_3d-mix_sin", "allencahn_3d-sin"]


def solution_3d(equation):
    """(u, src) of the 3-axis equations: src = lap u (Poisson) or lap u + u(u^2-1) (Allen-Cahn).
    poisson_3d-mix_sin is a smooth mode plus a 10x finer one per axis; the reference stops at two
    axes, so these are the project's own cases (the oracle's setup_3d uses the same closed forms)."""
    if equation == "poisson_3d-mix_sin":
        return (lambda x, y, z: s_(x) * s_(y) * s_(z) + 0.05 * s_(10 * x) * s_(10 * y) * s_(10 * z)), \
               (lambda x, y, z: -3.0 * s_(x) * s_(y) * s_(z) - 15.0 * s_(10 * x) * s_(10 * y) * s_(10 * z))
    if equation == "allencahn_3d-sin":
        u = lambda x, y, z: s_(2 * x) * s_(2 * y) * s_(2 * z)
        return u, (lambda x, y, z: -12.0 * s_(2 * x) * s_(2 * y) * s_(2 * z)
                   + u(x, y, z) * (u(x, y, z) ** 2 - 1.0))
    raise KeyError(equation)


class Operator3:
    """What an operator handle solves on a 3-axis grid (include/gpk.h gpk_operator3):
    sum_k coef[k] d^order[k] u / dx_k^order[k] + react[0] u + react[1] u^2 + react[2] u^3 = f, with
    boundary data on the faces whose bit is set in `faces` (bit order of boundary_3d: i1 = 0,
    i1 = n1 - 1, i2 = 0, i2 = n2 - 1, i3 = 0, i3 = n3 - 1)."""

    __slots__ = ("order", "coef", "react", "faces")

    def __init__(self, order, coef, react=(0.0, 0.0, 0.0), faces=63):
        self.order = tuple(int(o) for o in order)
        self.coef = tuple(float(c) for c in coef)
        self.react = tuple(float(r) for r in react)
        self.faces = int(faces)
        if len(self.order) != 3 or len(self.coef) != 3 or len(self.react) != 3:
            raise ValueError("order, coef and react have three entries each")

    @classmethod
    def of(cls, value):
        """An Operator3 from an Operator3 or a dict of its fields."""
        if isinstance(value, cls):
            return value
        return cls(value["order"], value["coef"], value.get("react", (0.0, 0.0, 0.0)), value.get("faces", 63))

    def as_dict(self):
        return {"order": self.order, "coef": self.coef, "react": self.react, "faces": self.faces}

    def __eq__(self, other):
        return isinstance(other, Operator3) and self.as_dict() == other.as_dict()

    def __repr__(self):
        return "Operator3(order=%r, coef=%r, react=%r, faces=%d)" % (self.order, self.coef, self.react, self.faces)


ALL_FACES, NO_FINAL_FACE = 0b111111, 0b011111  # every face; the final-time face i3 = n3 - 1 open

# The operator equations: third axis = time where one appears.  Each entry builds (u, src,
# operator) from a manufactured solution with closed-form derivatives.
_HEAT_NU, _ADV_BETA, _HELM_K, _ACT_EPS = 0.1, (1.0, 0.5), 4.0, 0.05


def _heat_sin():
    # u = e^{-t} sin(2x) sin(3y):  u_t - nu (u_xx + u_yy) = (13 nu - 1) u
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    return u, (lambda x, y, t: (13.0 * _HEAT_NU - 1.0) * u(x, y, t)), \
        Operator3((2, 2, 1), (-_HEAT_NU, -_HEAT_NU, 1.0), faces=NO_FINAL_FACE)


def _advection_sin():
    b1, b2 = _ADV_BETA
    return (lambda x, y, t: s_(x - b1 * t + y - b2 * t)), (lambda x, y, t: 0.0 * x * y * t), \
        Operator3((1, 1, 1), (b1, b2, 1.0))


def _helmholtz_sin():
    # u = sin(2x) sin(3y) sin(z):  lap u + k^2 u = (k^2 - 14) u
    u = lambda x, y, z: s_(2 * x) * s_(3 * y) * s_(z)
    return u, (lambda x, y, z: (_HELM_K ** 2 - 14.0) * u(x, y, z)), \
        Operator3((2, 2, 2), (1.0, 1.0, 1.0), react=(_HELM_K ** 2, 0.0, 0.0))


def _allencahn_t_sin():
    # u = e^{-t} sin(2x) sin(2y):  u_t - eps (u_xx + u_yy) + u^3 - u = (8 eps - 2) u + u^3
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(2 * y)
    return u, (lambda x, y, t: (8.0 * _ACT_EPS - 2.0) * u(x, y, t) + u(x, y, t) ** 3), \
        Operator3((2, 2, 1), (-_ACT_EPS, -_ACT_EPS, 1.0), react=(-1.0, 0.0, 1.0), faces=NO_FINAL_FACE)


_OP3D = {"heat_3d-sin": _heat_sin, "advection_3d-sin": _advection_sin,
         "helmholtz_3d-sin": _helmholtz_sin, "allencahn_t-sin": _allencahn_t_sin}
EQUATIONS_3D_OP = list(_OP3D)


def solution_3d_op(equation):
    """(u, src, operator) of an EQUATIONS_3D_OP entry."""
    return _OP3D[equation]()


class Operator3X:
    """What a gpk_create3_opx handle solves (include/gpk.h gpk_operator3x): sum_k (c2[k] d^2 u /
    dx_k^2 + c1[k] du / dx_k) + react[0] u + react[1] u^2 + react[2] u^3 = f, faces as Operator3.
    An axis with both weights non-zero is a mixed axis; with one, Operator3's order 2 or 1."""

    __slots__ = ("c2", "c1", "react", "faces")

    def __init__(self, c2, c1, react=(0.0, 0.0, 0.0), faces=63):
        self.c2 = tuple(float(c) for c in c2)
        self.c1 = tuple(float(c) for c in c1)
        self.react = tuple(float(r) for r in react)
        self.faces = int(faces)
        if len(self.c2) != 3 or len(self.c1) != 3 or len(self.react) != 3:
            raise ValueError("c2, c1 and react have three entries each")

    @classmethod
    def of(cls, value):
        """An Operator3X from an Operator3X or a dict of its fields."""
        if isinstance(value, cls):
            return value
        return cls(value["c2"], value["c1"], value.get("react", (0.0, 0.0, 0.0)), value.get("faces", 63))

    @property
    def mixed(self):
        """Per axis: both weights non-zero."""
        return tuple(a != 0.0 and b != 0.0 for a, b in zip(self.c2, self.c1))

    def as_dict(self):
        return {"c2": self.c2, "c1": self.c1, "react": self.react, "faces": self.faces}

    def __eq__(self, other):
        return isinstance(other, Operator3X) and self.as_dict() == other.as_dict()

    def __repr__(self):
        return "Operator3X(c2=%r, c1=%r, react=%r, faces=%d)" % (self.c2, self.c1, self.react, self.faces)


# Convection-diffusion, u_t + beta . grad u - nu lap u = f: second- and first-order terms on the
# same axis (gpk_create3_opx).  nu and beta are fixed here, once, for both entries.
_CD_NU, _CD_BETA = 0.05, (1.0, 0.5, 0.25)


def _convdiff_t_sin():
    # u = e^{-t} sin(2x) sin(3y):  u_t + b1 u_x + b2 u_y - nu (u_xx + u_yy)
    #   = (13 nu - 1) u + e^{-t} (2 b1 cos(2x) sin(3y) + 3 b2 sin(2x) cos(3y))
    b1, b2 = _CD_BETA[:2]
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    f = lambda x, y, t: ((13.0 * _CD_NU - 1.0) * u(x, y, t)
                         + np.exp(-t) * (2.0 * b1 * c_(2 * x) * s_(3 * y) + 3.0 * b2 * s_(2 * x) * c_(3 * y)))
    return u, f, Operator3X((-_CD_NU, -_CD_NU, 0.0), (b1, b2, 1.0), faces=NO_FINAL_FACE)


def _convdiff_3d_sin():
    # steady, u = sin(2x) sin(3y) sin(z):  beta . grad u - nu lap u = beta . grad u + 14 nu u
    b1, b2, b3 = _CD_BETA
    u = lambda x, y, z: s_(2 * x) * s_(3 * y) * s_(z)
    f = lambda x, y, z: (2.0 * b1 * c_(2 * x) * s_(3 * y) * s_(z) + 3.0 * b2 * s_(2 * x) * c_(3 * y) * s_(z)
                         + b3 * s_(2 * x) * s_(3 * y) * c_(z) + 14.0 * _CD_NU * u(x, y, z))
    return u, f, Operator3X((-_CD_NU,) * 3, (b1, b2, b3))


_OPX3D = {"convdiff_t-sin": _convdiff_t_sin, "convdiff_3d-sin": _convdiff_3d_sin}
EQUATIONS_3D_OPX = list(_OPX3D)


def solution_3d_opx(equation):
    """(u, src, operator) of an EQUATIONS_3D_OPX entry (operator: an Operator3X)."""
    return _OPX3D[equation]()


class Operator3V:
    """What a gpk_create3_opv handle solves (include/gpk.h gpk_coef3): Operator3X with a
    coefficient field per axis and one on the linear reaction term,
    sum_k a[k](x) (c2[k] d^2 u / dx_k^2 + c1[k] du / dx_k) + (react[0] + rho(x)) u + react[1] u^2
    + react[2] u^3 = f.  Each of a[0..2] and rho is None (a = 1, rho = 0), an array of the grid's
    shape, or a callable of the three coordinate meshes (x, y, z); fields(axes) evaluates them."""

    __slots__ = ("c2", "c1", "react", "faces", "a", "rho")

    def __init__(self, c2, c1, react=(0.0, 0.0, 0.0), faces=63, a=(None, None, None), rho=None):
        x = Operator3X(c2, c1, react, faces)
        self.c2, self.c1, self.react, self.faces = x.c2, x.c1, x.react, x.faces
        self.a = tuple(a)
        self.rho = rho
        if len(self.a) != 3:
            raise ValueError("a has three entries (None for an axis without a field)")

    @property
    def constant(self):
        """The Operator3X of the constant part (what gpk_operator_info3x reports)."""
        return Operator3X(self.c2, self.c1, self.react, self.faces)

    @property
    def has(self):
        """(a1, a2, a3, rho) present, as DeviceSolver3.coef_info() reports."""
        return tuple(f is not None for f in self.a + (self.rho,))

    def fields(self, axes):
        """[a1, a2, a3, rho] on the tensor grid of the three coordinate axes: float64 arrays of
        shape (n1, n2, n3), None where absent.  Callables get the 'ij' meshes."""
        axes = [np.asarray(x, np.float64).reshape(-1) for x in axes]
        shape = tuple(x.size for x in axes)
        mesh = None
        out = []
        for f in self.a + (self.rho,):
            if f is None:
                out.append(None)
                continue
            if callable(f):
                mesh = np.meshgrid(*axes, indexing="ij") if mesh is None else mesh
                v = np.asarray(f(*mesh), np.float64) * np.ones(shape)
            else:
                v = np.asarray(f, np.float64)
                if v.shape != shape:
                    raise ValueError("a coefficient field given as an array must have the grid's shape %r" % (shape,))
            out.append(np.ascontiguousarray(v))
        return out

    def __repr__(self):
        kind = lambda f: "None" if f is None else "<callable>" if callable(f) else "<array>"
        return "Operator3V(c2=%r, c1=%r, react=%r, faces=%d, a=(%s), rho=%s)" % (
            self.c2, self.c1, self.react, self.faces, ", ".join(kind(f) for f in self.a), kind(self.rho))


# Coefficient-field equations on [0, 1]^3 (gpk_create3_opv); third axis = time where one appears.
_HV_K2 = lambda x, y, z: 16.0 * (1.0 + 0.5 * x)                                # k(x)^2, max 24 < 3 pi^2
_HEATV_A = lambda x, y, t: 1.0 + 0.5 * s_(2 * np.pi * x) * c_(2 * np.pi * y)    # nu(x, y) / _HEAT_NU
_ROT_B1, _ROT_B2 = (lambda x, y, t: -(y - 0.5)), (lambda x, y, t: x - 0.5)      # the rotating flow


def _helmholtz_var_sin():
    # u = sin(2x) sin(3y) sin(z):  lap u + k(x)^2 u = (k(x)^2 - 14) u
    u = lambda x, y, z: s_(2 * x) * s_(3 * y) * s_(z)
    return u, (lambda x, y, z: (_HV_K2(x, y, z) - 14.0) * u(x, y, z)), \
        Operator3V((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), rho=_HV_K2)


def _heat_var_sin():
    # u = e^{-t} sin(2x) sin(3y):  u_t - nu(x,y) (u_xx + u_yy) = (13 nu(x,y) - 1) u, nu = _HEAT_NU a
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    return u, (lambda x, y, t: (13.0 * _HEAT_NU * _HEATV_A(x, y, t) - 1.0) * u(x, y, t)), \
        Operator3V((-_HEAT_NU, -_HEAT_NU, 0.0), (0.0, 0.0, 1.0), faces=NO_FINAL_FACE, a=(_HEATV_A, _HEATV_A, None))


def _transport_var_sin():
    # the same u:  u_t + b1 u_x + b2 u_y = -u + e^{-t} (2 b1 cos(2x) sin(3y) + 3 b2 sin(2x) cos(3y))
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    f = lambda x, y, t: (-u(x, y, t) + np.exp(-t) * (2.0 * _ROT_B1(x, y, t) * c_(2 * x) * s_(3 * y)
                                                     + 3.0 * _ROT_B2(x, y, t) * s_(2 * x) * c_(3 * y)))
    return u, f, Operator3V((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), faces=NO_FINAL_FACE, a=(_ROT_B1, _ROT_B2, None))


_OPV3D = {"helmholtz_var-sin": _helmholtz_var_sin, "heat_var-sin": _heat_var_sin,
          "transport_var-sin": _transport_var_sin}
EQUATIONS_3D_OPV = list(_OPV3D)


def solution_3d_opv(equation):
    """(u, src, operator) of an EQUATIONS_3D_OPV entry (operator: an Operator3V of callables)."""
    return _OPV3D[equation]()


# Equations with derivative boundary data on [0, 1]^3 (gpk_create3_opn): the operator, the faces that
# carry d u / d x_k (along the coordinate, not the outward normal) and the closed-form gradient of u.
_WAVE_C, _WAVE_OM = 0.5, 2.0


def _wave_t_sin():
    # u = sin(2x) sin(3y) sin(om t + 1/2):  u_tt - c^2 (u_xx + u_yy) = (13 c^2 - om^2) u;
    # u(., 0) and u_t(., 0) both on face 4, the final-time face open
    c2, om = _WAVE_C ** 2, _WAVE_OM
    u = lambda x, y, t: s_(2 * x) * s_(3 * y) * s_(om * t + 0.5)
    grad = (lambda x, y, t: 2.0 * c_(2 * x) * s_(3 * y) * s_(om * t + 0.5),
            lambda x, y, t: 3.0 * s_(2 * x) * c_(3 * y) * s_(om * t + 0.5),
            lambda x, y, t: om * s_(2 * x) * s_(3 * y) * c_(om * t + 0.5))
    return u, (lambda x, y, t: (13.0 * c2 - om * om) * u(x, y, t)), \
        Operator3X((-c2, -c2, 1.0), (0.0, 0.0, 0.0), faces=NO_FINAL_FACE), 0b010000, grad


def _helmholtz_neumann_sin():
    # helmholtz_3d-sin with u_x given on the two x walls instead of u
    u = lambda x, y, z: s_(2 * x) * s_(3 * y) * s_(z)
    grad = (lambda x, y, z: 2.0 * c_(2 * x) * s_(3 * y) * s_(z),
            lambda x, y, z: 3.0 * s_(2 * x) * c_(3 * y) * s_(z),
            lambda x, y, z: s_(2 * x) * s_(3 * y) * c_(z))
    return u, (lambda x, y, z: (_HELM_K ** 2 - 14.0) * u(x, y, z)), \
        Operator3X((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), react=(_HELM_K ** 2, 0.0, 0.0), faces=0b111100), 0b000011, grad


_OPN3D = {"wave_t-sin": _wave_t_sin, "helmholtz_neumann-sin": _helmholtz_neumann_sin}
EQUATIONS_3D_OPN = list(_OPN3D)


def solution_3d_opn(equation):
    """(u, src, operator, dfaces, grad_u) of an EQUATIONS_3D_OPN entry: operator an Operator3X,
    dfaces the faces that carry d u / d x_k, grad_u = (u_x1, u_x2, u_x3) as callables."""
    return _OPN3D[equation]()


def deriv_boundary_3d(grad_u, axes, dfaces):
    """grad_u on a mesh as gpk_bdata3.dvals: the six-face layout of boundary_3d, face f = 2k + s
    holding d u / d x_k at index 0 (s = 0) or n_k - 1 (s = 1) of axis k; NaN on the faces outside
    dfaces (never read)."""
    axes = [np.asarray(x, np.float64).reshape(-1) for x in axes]
    mesh = np.meshgrid(*axes, indexing="ij")
    shape = mesh[0].shape
    out = []
    for f in range(6):
        k, s = divmod(f, 2)
        sl = [slice(None)] * 3
        sl[k] = -1 if s else 0
        sl = tuple(sl)
        if (dfaces >> f) & 1:
            g = np.asarray(grad_u[k](*[m[sl] for m in mesh]), np.float64) * np.ones(mesh[0][sl].shape)
            out.append(g.ravel())
        else:
            out.append(np.full(mesh[0][sl].size, np.nan))
    return np.concatenate(out)


# Equations with convective terms on [0, 1]^3 (gpk_create3_opc): the operator's linear part, the
# constants g_k of the terms g_k u du / dx_k, and (as for EQUATIONS_3D_OPN) the derivative faces and
# the closed-form gradient of u.  Viscous Burgers, nu fixed here for both entries.
_BURGERS_NU = 0.05


def _burgers_t_sin():
    # u = e^{-t} sin(2x) sin(3y):  u_t + u (u_x + u_y) - nu (u_xx + u_yy) = (13 nu - 1) u + u (u_x + u_y)
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    grad = (lambda x, y, t: 2.0 * np.exp(-t) * c_(2 * x) * s_(3 * y),
            lambda x, y, t: 3.0 * np.exp(-t) * s_(2 * x) * c_(3 * y),
            lambda x, y, t: -u(x, y, t))
    f = lambda x, y, t: (13.0 * _BURGERS_NU - 1.0) * u(x, y, t) + u(x, y, t) * (grad[0](x, y, t) + grad[1](x, y, t))
    return u, f, Operator3X((-_BURGERS_NU, -_BURGERS_NU, 0.0), (0.0, 0.0, 1.0), faces=NO_FINAL_FACE), 0, grad, \
        (1.0, 1.0, 0.0)


def _burgers_3d_sin():
    # steady, u = sin(2x) sin(3y) sin(z):  u (u_x + u_y + u_z) - nu lap u = u (u_x + u_y + u_z) + 14 nu u
    u = lambda x, y, z: s_(2 * x) * s_(3 * y) * s_(z)
    grad = (lambda x, y, z: 2.0 * c_(2 * x) * s_(3 * y) * s_(z),
            lambda x, y, z: 3.0 * s_(2 * x) * c_(3 * y) * s_(z),
            lambda x, y, z: s_(2 * x) * s_(3 * y) * c_(z))
    f = lambda x, y, z: (u(x, y, z) * (grad[0](x, y, z) + grad[1](x, y, z) + grad[2](x, y, z))
                         + 14.0 * _BURGERS_NU * u(x, y, z))
    return u, f, Operator3X((-_BURGERS_NU,) * 3, (0.0, 0.0, 0.0)), 0, grad, (1.0, 1.0, 1.0)


_OPC3D = {"burgers_t-sin": _burgers_t_sin, "burgers_3d-sin": _burgers_3d_sin}
EQUATIONS_3D_OPC = list(_OPC3D)


def solution_3d_opc(equation):
    """(u, src, operator, dfaces, grad_u, conv) of an EQUATIONS_3D_OPC entry: the first five as
    solution_3d_opn's, conv = (g_1, g_2, g_3), the constants of the terms g_k u du / dx_k."""
    return _OPC3D[equation]()


# Equations with mixed partials on [0, 1]^3 (gpk_create3_opm): as EQUATIONS_3D_OPC's entries, plus the
# constants m_12, m_13, m_23 of the terms m_jk d^2 u / dx_j dx_k.  Anisotropic diffusion whose tensor
# has off-diagonal entries: -div(A grad u) = -sum_k A_kk u_kk - 2 sum_{j<k} A_jk u_jk.
_ANISO_HEAT = (0.1, 0.04, 0.06)  # (a, b, c) of [[a, b], [b, c]]
_ANISO_A = ((1.0, 0.3, 0.2), (0.3, 1.0, 0.1), (0.2, 0.1, 1.0))


def _aniso_heat_t_sin():
    # u = e^{-t} sin(2x) sin(3y):  u_t - (a u_xx + 2 b u_xy + c u_yy) = (4a + 9c - 1) u - 12 b e^{-t} cos(2x) cos(3y)
    a, b, c = _ANISO_HEAT
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    grad = (lambda x, y, t: 2.0 * np.exp(-t) * c_(2 * x) * s_(3 * y),
            lambda x, y, t: 3.0 * np.exp(-t) * s_(2 * x) * c_(3 * y),
            lambda x, y, t: -u(x, y, t))
    f = lambda x, y, t: (4.0 * a + 9.0 * c - 1.0) * u(x, y, t) - 12.0 * b * np.exp(-t) * c_(2 * x) * c_(3 * y)
    return u, f, Operator3X((-a, -c, 0.0), (0.0, 0.0, 1.0), faces=NO_FINAL_FACE), 0, grad, (0.0, 0.0, 0.0), \
        (-2.0 * b, 0.0, 0.0)


def _aniso_3d_sin():
    # steady, u = sin(2x) sin(3y) sin(z):  -div(A grad u) = 14 u - 2 (A_12 u_xy + A_13 u_xz + A_23 u_yz)
    A = _ANISO_A
    u = lambda x, y, z: s_(2 * x) * s_(3 * y) * s_(z)
    grad = (lambda x, y, z: 2.0 * c_(2 * x) * s_(3 * y) * s_(z),
            lambda x, y, z: 3.0 * s_(2 * x) * c_(3 * y) * s_(z),
            lambda x, y, z: s_(2 * x) * s_(3 * y) * c_(z))
    f = lambda x, y, z: (14.0 * u(x, y, z) - 2.0 * (A[0][1] * 6.0 * c_(2 * x) * c_(3 * y) * s_(z)
                                                     + A[0][2] * 2.0 * c_(2 * x) * s_(3 * y) * c_(z)
                                                     + A[1][2] * 3.0 * s_(2 * x) * c_(3 * y) * c_(z)))
    return u, f, Operator3X((-A[0][0], -A[1][1], -A[2][2]), (0.0, 0.0, 0.0)), 0, grad, (0.0, 0.0, 0.0), \
        (-2.0 * A[0][1], -2.0 * A[0][2], -2.0 * A[1][2])


_OPM3D = {"aniso_heat_t-sin": _aniso_heat_t_sin, "aniso_3d-sin": _aniso_3d_sin}
EQUATIONS_3D_OPM = list(_OPM3D)


def solution_3d_opm(equation):
    """(u, src, operator, dfaces, grad_u, conv, cross) of an EQUATIONS_3D_OPM entry: the first six as
    solution_3d_opc's, cross = (m_12, m_13, m_23), the constants of the terms m_jk d^2 u / dx_j dx_k."""
    return _OPM3D[equation]()


# Equations with drift fields on [0, 1]^3 (gpk_create3_opb): as EQUATIONS_3D_OPM's entries, plus the
# fields b_k(x) of the terms b_k du / dx_k, each None or a callable of the three meshes.  Divergence
# form c2_k d/dx_k (a du/dx_k) is an Operator3V with a on axis k plus the drift c2_k da/dx_k.
def divergence_drift(grad_a, c2):
    """The drift (b_1, b_2, b_3) with b_k = c2[k] * grad_a[k], so that Operator3V(c2, ..., a=(a, a, a))
    plus this drift states sum_k c2[k] d/dx_k (a du/dx_k).  grad_a: three entries, each None (a does
    not vary along x_k), an array of the grid's shape or a callable of the meshes; b_k is None where
    grad_a[k] is None or c2[k] == 0."""
    if len(grad_a) != 3 or len(c2) != 3:
        raise ValueError("grad_a and c2 have three entries")
    out = []
    for g, w in zip(grad_a, c2):
        w = float(w)
        if g is None or w == 0.0:
            out.append(None)
        elif callable(g):
            out.append(lambda x, y, z, g=g, w=w: w * np.asarray(g(x, y, z), np.float64))
        else:
            out.append(w * np.asarray(g, np.float64))
    return tuple(out)


def drift_fields(drift, axes):
    """[b_1, b_2, b_3] on the tensor grid of the three coordinate axes, as Operator3V.fields lays its
    fields out: float64 arrays of shape (n1, n2, n3), None where absent.  Callables get the 'ij' meshes."""
    if len(drift) != 3:
        raise ValueError("drift has three entries (None for an axis without a field)")
    axes = [np.asarray(x, np.float64).reshape(-1) for x in axes]
    shape = tuple(x.size for x in axes)
    mesh = None
    out = []
    for f in drift:
        if f is None:
            out.append(None)
            continue
        if callable(f):
            mesh = np.meshgrid(*axes, indexing="ij") if mesh is None else mesh
            v = np.asarray(f(*mesh), np.float64) * np.ones(shape)
        else:
            v = np.asarray(f, np.float64)
            if v.shape != shape:
                raise ValueError("a drift field given as an array must have the grid's shape %r" % (shape,))
        out.append(np.ascontiguousarray(v))
    return out


_DARCY_A = lambda x, y, z: 1.0 + 0.5 * s_(2 * np.pi * x) * c_(2 * np.pi * y) + 0.25 * z
_DARCY_GRAD_A = (lambda x, y, z: np.pi * c_(2 * np.pi * x) * c_(2 * np.pi * y),
                 lambda x, y, z: -np.pi * s_(2 * np.pi * x) * s_(2 * np.pi * y),
                 lambda x, y, z: 0.25 + 0.0 * z)
_HEATV_GRAD_A = (lambda x, y, t: np.pi * c_(2 * np.pi * x) * c_(2 * np.pi * y),
                 lambda x, y, t: -np.pi * s_(2 * np.pi * x) * s_(2 * np.pi * y), None)
_ROT_NU = 0.05


def _darcy_3d_sin():
    # steady, u = sin(2x) sin(3y) sin(z):  -div(a grad u) = 14 a u - grad a . grad u
    u = lambda x, y, z: s_(2 * x) * s_(3 * y) * s_(z)
    grad = (lambda x, y, z: 2.0 * c_(2 * x) * s_(3 * y) * s_(z),
            lambda x, y, z: 3.0 * s_(2 * x) * c_(3 * y) * s_(z),
            lambda x, y, z: s_(2 * x) * s_(3 * y) * c_(z))
    f = lambda x, y, z: (14.0 * _DARCY_A(x, y, z) * u(x, y, z)
                         - sum(_DARCY_GRAD_A[k](x, y, z) * grad[k](x, y, z) for k in range(3)))
    c2 = (-1.0, -1.0, -1.0)
    return u, f, Operator3V(c2, (0.0, 0.0, 0.0), a=(_DARCY_A,) * 3), 0, grad, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), \
        divergence_drift(_DARCY_GRAD_A, c2)


def _heat_div_t_sin():
    # u = e^{-t} sin(2x) sin(3y):  u_t - div(nu grad u) = (13 nu - 1) u - grad nu . grad u, nu = _HEAT_NU a(x, y)
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    grad = (lambda x, y, t: 2.0 * np.exp(-t) * c_(2 * x) * s_(3 * y),
            lambda x, y, t: 3.0 * np.exp(-t) * s_(2 * x) * c_(3 * y),
            lambda x, y, t: -u(x, y, t))
    f = lambda x, y, t: ((13.0 * _HEAT_NU * _HEATV_A(x, y, t) - 1.0) * u(x, y, t)
                         - _HEAT_NU * sum(_HEATV_GRAD_A[k](x, y, t) * grad[k](x, y, t) for k in range(2)))
    c2 = (-_HEAT_NU, -_HEAT_NU, 0.0)
    return u, f, Operator3V(c2, (0.0, 0.0, 1.0), faces=NO_FINAL_FACE, a=(_HEATV_A, _HEATV_A, None)), 0, grad, \
        (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), divergence_drift(_HEATV_GRAD_A, c2)


def _convdiff_rot_t_sin():
    # the same u:  u_t + b . grad u - nu lap u = (13 nu - 1) u + b1 u_x + b2 u_y, b the rotating flow
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    grad = (lambda x, y, t: 2.0 * np.exp(-t) * c_(2 * x) * s_(3 * y),
            lambda x, y, t: 3.0 * np.exp(-t) * s_(2 * x) * c_(3 * y),
            lambda x, y, t: -u(x, y, t))
    f = lambda x, y, t: ((13.0 * _ROT_NU - 1.0) * u(x, y, t) + _ROT_B1(x, y, t) * grad[0](x, y, t)
                         + _ROT_B2(x, y, t) * grad[1](x, y, t))
    return u, f, Operator3X((-_ROT_NU, -_ROT_NU, 0.0), (0.0, 0.0, 1.0), faces=NO_FINAL_FACE), 0, grad, \
        (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (_ROT_B1, _ROT_B2, None)


_OPB3D = {"darcy_3d-sin": _darcy_3d_sin, "heat_div_t-sin": _heat_div_t_sin,
          "convdiff_rot_t-sin": _convdiff_rot_t_sin}
EQUATIONS_3D_OPB = list(_OPB3D)


def solution_3d_opb(equation):
    """(u, src, operator, dfaces, grad_u, conv, cross, drift) of an EQUATIONS_3D_OPB entry: the first
    seven as solution_3d_opm's (operator an Operator3X or an Operator3V of callables), drift =
    (b_1, b_2, b_3), the fields of the terms b_k du / dx_k as callables (None: no such term)."""
    return _OPB3D[equation]()


# Equations with third- and fourth-order terms on [0, 1]^3 (gpk_create3_oph): as EQUATIONS_3D_OPB's
# entries, plus high = (c4, c3), the constants of c4_k d^4 u / dx_k^4 + c3_k d^3 u / dx_k^3.  The third
# axis is time and the final-time face is open.
_KDV_DELTA, _KS_NU, _BEAM_KAPPA, _BEAM_OM = 0.01, 0.02, 0.01, 2.0


def _kdv_t_sin():
    # u = e^{-t} sin(2x) sin(3y):  u_t + u u_x + delta u_xxx = -u + u u_x - 8 delta e^{-t} cos(2x) sin(3y)
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    grad = (lambda x, y, t: 2.0 * np.exp(-t) * c_(2 * x) * s_(3 * y),
            lambda x, y, t: 3.0 * np.exp(-t) * s_(2 * x) * c_(3 * y),
            lambda x, y, t: -u(x, y, t))
    f = lambda x, y, t: (-u(x, y, t) + u(x, y, t) * grad[0](x, y, t)
                         - 8.0 * _KDV_DELTA * np.exp(-t) * c_(2 * x) * s_(3 * y))
    return u, f, Operator3X((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), faces=NO_FINAL_FACE), 0, grad, (1.0, 0.0, 0.0), \
        (0.0, 0.0, 0.0), (None, None, None), ((0.0, 0.0, 0.0), (_KDV_DELTA, 0.0, 0.0))


def _ks_t_sin():
    # the same u, Kuramoto-Sivashinsky axis-wise in x:  u_t + u u_x + u_xx + nu u_xxxx = (16 nu - 5) u + u u_x
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    grad = (lambda x, y, t: 2.0 * np.exp(-t) * c_(2 * x) * s_(3 * y),
            lambda x, y, t: 3.0 * np.exp(-t) * s_(2 * x) * c_(3 * y),
            lambda x, y, t: -u(x, y, t))
    f = lambda x, y, t: (16.0 * _KS_NU - 5.0) * u(x, y, t) + u(x, y, t) * grad[0](x, y, t)
    return u, f, Operator3X((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), faces=NO_FINAL_FACE), 0, grad, (1.0, 0.0, 0.0), \
        (0.0, 0.0, 0.0), (None, None, None), ((_KS_NU, 0.0, 0.0), (0.0, 0.0, 0.0))


def _beam_t_sin():
    # u = sin(2x) sin(3y) sin(om t + 1/2), the Euler-Bernoulli beam in x:  u_tt + kappa u_xxxx = (16 kappa - om^2) u;
    # clamped ends: u and u_x on both x walls (faces 0, 1); u and u_t on the initial face (4)
    om = _BEAM_OM
    u = lambda x, y, t: s_(2 * x) * s_(3 * y) * s_(om * t + 0.5)
    grad = (lambda x, y, t: 2.0 * c_(2 * x) * s_(3 * y) * s_(om * t + 0.5),
            lambda x, y, t: 3.0 * s_(2 * x) * c_(3 * y) * s_(om * t + 0.5),
            lambda x, y, t: om * s_(2 * x) * s_(3 * y) * c_(om * t + 0.5))
    f = lambda x, y, t: (16.0 * _BEAM_KAPPA - om * om) * u(x, y, t)
    return u, f, Operator3X((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), faces=NO_FINAL_FACE), 0b010011, grad, \
        (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (None, None, None), ((_BEAM_KAPPA, 0.0, 0.0), (0.0, 0.0, 0.0))


_OPH3D = {"kdv_t-sin": _kdv_t_sin, "ks_t-sin": _ks_t_sin, "beam_t-sin": _beam_t_sin}
EQUATIONS_3D_OPH = list(_OPH3D)


def solution_3d_oph(equation):
    """(u, src, operator, dfaces, grad_u, conv, cross, drift, high) of an EQUATIONS_3D_OPH entry: the
    first eight as solution_3d_opb's, high = (c4, c3), two triples: the constants of the terms c4_k
    d^4 u / dx_k^4 + c3_k d^3 u / dx_k^3."""
    return _OPH3D[equation]()


# Equations with mixed fourth-order partials on [0, 1]^3 (gpk_create3_opq): as EQUATIONS_3D_OPH's entries,
# plus bicross = (q_12, q_13, q_23), the constants of q_jk d^4 u / dx_j^2 dx_k^2.
_PLATE_KAPPA, _PLATE_OM, _SH_EPS, _SH_R, _MIXED4_Q = 0.01, 2.0, 0.1, 0.3, 0.01
_NO_DRIFT, _ZERO3 = (None, None, None), (0.0, 0.0, 0.0)


def _plate_t_sin():
    # u = sin(2x) sin(3y) sin(om t + 1/2), the Kirchhoff plate in (x, y):  u_tt + kappa (u_xxxx + 2 u_xxyy + u_yyyy)
    # = (169 kappa - om^2) u; clamped edges: u and u_x on the x walls, u and u_y on the y walls (faces 0-3); u and u_t
    # on the initial face (4)
    om, ka = _PLATE_OM, _PLATE_KAPPA
    u = lambda x, y, t: s_(2 * x) * s_(3 * y) * s_(om * t + 0.5)
    grad = (lambda x, y, t: 2.0 * c_(2 * x) * s_(3 * y) * s_(om * t + 0.5),
            lambda x, y, t: 3.0 * s_(2 * x) * c_(3 * y) * s_(om * t + 0.5),
            lambda x, y, t: om * s_(2 * x) * s_(3 * y) * c_(om * t + 0.5))
    f = lambda x, y, t: (169.0 * ka - om * om) * u(x, y, t)
    return u, f, Operator3X((0.0, 0.0, 1.0), _ZERO3, faces=NO_FINAL_FACE), 0b011111, grad, \
        _ZERO3, _ZERO3, _NO_DRIFT, ((ka, ka, 0.0), _ZERO3), (2.0 * ka, 0.0, 0.0)


def _biharmonic_3d_sin():
    # steady, u = sin(2x) sin(3y) sin(z):  lap^2 u = 196 u; u and du/dn on all six faces
    u = lambda x, y, z: s_(2 * x) * s_(3 * y) * s_(z)
    grad = (lambda x, y, z: 2.0 * c_(2 * x) * s_(3 * y) * s_(z),
            lambda x, y, z: 3.0 * s_(2 * x) * c_(3 * y) * s_(z),
            lambda x, y, z: s_(2 * x) * s_(3 * y) * c_(z))
    f = lambda x, y, z: 196.0 * u(x, y, z)
    return u, f, Operator3X(_ZERO3, _ZERO3), ALL_FACES, grad, _ZERO3, _ZERO3, _NO_DRIFT, \
        ((1.0, 1.0, 1.0), _ZERO3), (2.0, 2.0, 2.0)


def _swift_hohenberg_t_sin():
    # u = e^{-t} sin(2x) sin(3y):  u_t + (1 - r) u + 2 eps lap u + eps^2 lap^2 u + u^3
    # = (-r - 26 eps + 169 eps^2) u + u^3; u and du/dn on the four space walls, u on the initial face
    e, r = _SH_EPS, _SH_R
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    grad = (lambda x, y, t: 2.0 * np.exp(-t) * c_(2 * x) * s_(3 * y),
            lambda x, y, t: 3.0 * np.exp(-t) * s_(2 * x) * c_(3 * y),
            lambda x, y, t: -u(x, y, t))
    f = lambda x, y, t: (-r - 26.0 * e + 169.0 * e * e) * u(x, y, t) + u(x, y, t) ** 3
    return u, f, Operator3X((2.0 * e, 2.0 * e, 0.0), (0.0, 0.0, 1.0), react=(1.0 - r, 0.0, 1.0), faces=NO_FINAL_FACE), \
        0b001111, grad, _ZERO3, _ZERO3, _NO_DRIFT, ((e * e, e * e, 0.0), _ZERO3), (2.0 * e * e, 0.0, 0.0)


def _mixed4_3d_sin():
    # steady, u = sin(2x) sin(3y) sin(z), no order above two on one axis (so eq_residual can run):
    # -lap u + q (u_xxyy + u_xxzz + u_yyzz) = (14 + 49 q) u
    q = _MIXED4_Q
    u = lambda x, y, z: s_(2 * x) * s_(3 * y) * s_(z)
    grad = (lambda x, y, z: 2.0 * c_(2 * x) * s_(3 * y) * s_(z),
            lambda x, y, z: 3.0 * s_(2 * x) * c_(3 * y) * s_(z),
            lambda x, y, z: s_(2 * x) * s_(3 * y) * c_(z))
    f = lambda x, y, z: (14.0 + 49.0 * q) * u(x, y, z)
    return u, f, Operator3X((-1.0, -1.0, -1.0), _ZERO3), 0, grad, _ZERO3, _ZERO3, _NO_DRIFT, \
        (_ZERO3, _ZERO3), (q, q, q)


_OPQ3D = {"plate_t-sin": _plate_t_sin, "biharmonic_3d-sin": _biharmonic_3d_sin,
          "swift_hohenberg_t-sin": _swift_hohenberg_t_sin, "mixed4_3d-sin": _mixed4_3d_sin}
EQUATIONS_3D_OPQ = list(_OPQ3D)


def solution_3d_opq(equation):
    """(u, src, operator, dfaces, grad_u, conv, cross, drift, high, bicross) of an EQUATIONS_3D_OPQ entry:
    the first nine as solution_3d_oph's, bicross = (q_12, q_13, q_23), the constants of the terms q_jk
    d^4 u / dx_j^2 dx_k^2."""
    return _OPQ3D[equation]()


# Equations with quadratic gradient terms on [0, 1]^3 (gpk_create3_opg): as EQUATIONS_3D_OPQ's entries,
# plus gradsq = (s, x): the constants of s_k (du/dx_k)^2 and, over the pairs (1,2), (1,3), (2,3), of
# x_jk du/dx_j du/dx_k.
_EIK_EPS, _HJ_NU, _KPZ_NU, _KPZ_LAMBDA, _KSI_EPS = 0.1, 0.05, 0.05, 1.0, 0.1
_ANISO_S, _ANISO_X = (1.0, 0.5, 2.0), (0.6, 0.0, -0.4)


def _steady_sin():
    u = lambda x, y, z: s_(2 * x) * s_(3 * y) * s_(z)
    grad = (lambda x, y, z: 2.0 * c_(2 * x) * s_(3 * y) * s_(z),
            lambda x, y, z: 3.0 * s_(2 * x) * c_(3 * y) * s_(z),
            lambda x, y, z: s_(2 * x) * s_(3 * y) * c_(z))
    return u, grad


def _decay_sin():
    u = lambda x, y, t: np.exp(-t) * s_(2 * x) * s_(3 * y)
    grad = (lambda x, y, t: 2.0 * np.exp(-t) * c_(2 * x) * s_(3 * y),
            lambda x, y, t: 3.0 * np.exp(-t) * s_(2 * x) * c_(3 * y),
            lambda x, y, t: -u(x, y, t))
    return u, grad


def _eikonal_3d_sin():
    # steady, u = sin(2x) sin(3y) sin(z), the viscous eikonal:  |grad u|^2 - eps lap u = |grad u|^2 + 14 eps u
    e = _EIK_EPS
    u, grad = _steady_sin()
    f = lambda x, y, z: sum(g(x, y, z) ** 2 for g in grad) + 14.0 * e * u(x, y, z)
    return u, f, Operator3X((-e, -e, -e), _ZERO3), 0, grad, _ZERO3, _ZERO3, _NO_DRIFT, (_ZERO3, _ZERO3), _ZERO3, \
        ((1.0, 1.0, 1.0), _ZERO3)


def _hj_t_sin():
    # u = e^{-t} sin(2x) sin(3y), Hamilton-Jacobi:  u_t + (u_x^2 + u_y^2) / 2 - nu (u_xx + u_yy)
    # = (13 nu - 1) u + (u_x^2 + u_y^2) / 2
    nu = _HJ_NU
    u, grad = _decay_sin()
    f = lambda x, y, t: (13.0 * nu - 1.0) * u(x, y, t) + 0.5 * (grad[0](x, y, t) ** 2 + grad[1](x, y, t) ** 2)
    return u, f, Operator3X((-nu, -nu, 0.0), (0.0, 0.0, 1.0), faces=NO_FINAL_FACE), 0, grad, _ZERO3, _ZERO3, \
        _NO_DRIFT, (_ZERO3, _ZERO3), _ZERO3, ((0.5, 0.5, 0.0), _ZERO3)


def _kpz_t_sin():
    # the same u, KPZ:  u_t - nu (u_xx + u_yy) - (lambda / 2) (u_x^2 + u_y^2) = (13 nu - 1) u - (lambda / 2) (u_x^2 + u_y^2)
    nu, la = _KPZ_NU, _KPZ_LAMBDA
    u, grad = _decay_sin()
    f = lambda x, y, t: ((13.0 * nu - 1.0) * u(x, y, t)
                         - 0.5 * la * (grad[0](x, y, t) ** 2 + grad[1](x, y, t) ** 2))
    return u, f, Operator3X((-nu, -nu, 0.0), (0.0, 0.0, 1.0), faces=NO_FINAL_FACE), 0, grad, _ZERO3, _ZERO3, \
        _NO_DRIFT, (_ZERO3, _ZERO3), _ZERO3, ((-0.5 * la, -0.5 * la, 0.0), _ZERO3)


def _aniso_eikonal_3d_sin():
    # steady, u = sin(2x) sin(3y) sin(z):  grad u^T S grad u - eps lap u, S = [[1, .3, 0], [.3, .5, -.2], [0, -.2, 2]]
    # (positive definite): s = diag S, x_jk = 2 S_jk
    e, s, xw = _EIK_EPS, _ANISO_S, _ANISO_X
    u, grad = _steady_sin()

    def f(x, y, z):
        g = [gk(x, y, z) for gk in grad]
        return (s[0] * g[0] ** 2 + s[1] * g[1] ** 2 + s[2] * g[2] ** 2 + xw[0] * g[0] * g[1] + xw[1] * g[0] * g[2]
                + xw[2] * g[1] * g[2] + 14.0 * e * u(x, y, z))
    return u, f, Operator3X((-e, -e, -e), _ZERO3), 0, grad, _ZERO3, _ZERO3, _NO_DRIFT, (_ZERO3, _ZERO3), _ZERO3, \
        (s, xw)


def _ks_int_t_sin():
    # u = e^{-t} sin(2x) sin(3y), Kuramoto-Sivashinsky in its integral form in (x, y), the weights of lap and lap^2
    # scaled as Swift-Hohenberg's:  u_t + 2 eps lap u + eps^2 lap^2 u + |grad u|^2 / 2
    # = (-1 - 26 eps + 169 eps^2) u + (u_x^2 + u_y^2) / 2; u and du/dn on the four space walls, u on the initial face
    e = _KSI_EPS
    u, grad = _decay_sin()
    f = lambda x, y, t: ((-1.0 - 26.0 * e + 169.0 * e * e) * u(x, y, t)
                         + 0.5 * (grad[0](x, y, t) ** 2 + grad[1](x, y, t) ** 2))
    return u, f, Operator3X((2.0 * e, 2.0 * e, 0.0), (0.0, 0.0, 1.0), faces=NO_FINAL_FACE), 0b001111, grad, \
        _ZERO3, _ZERO3, _NO_DRIFT, ((e * e, e * e, 0.0), _ZERO3), (2.0 * e * e, 0.0, 0.0), ((0.5, 0.5, 0.0), _ZERO3)


_OPG3D = {"eikonal_3d-sin": _eikonal_3d_sin, "hj_t-sin": _hj_t_sin, "kpz_t-sin": _kpz_t_sin,
          "aniso_eikonal_3d-sin": _aniso_eikonal_3d_sin, "ks_int_t-sin": _ks_int_t_sin}
EQUATIONS_3D_OPG = list(_OPG3D)


def solution_3d_opg(equation):
    """(u, src, operator, dfaces, grad_u, conv, cross, drift, high, bicross, gradsq) of an EQUATIONS_3D_OPG
    entry: the first ten as solution_3d_opq's, gradsq = (s, x), two triples: the constants of the terms
    s_k (du/dx_k)^2 and x_jk du/dx_j du/dx_k over the pairs (1,2), (1,3), (2,3)."""
    return _OPG3D[equation]()


def boundary_2d(u_mesh):
    """get_boundary_vals: hstack(U[0,:], U[-1,:], U[:,0], U[:,-1]) (model_GP_solver_2d.py:377-379)."""
    return np.hstack((u_mesh[0, :], u_mesh[-1, :], u_mesh[:, 0], u_mesh[:, -1]))


def autodiff_source_1d(u_torch, x, allen_cahn=False):
    """src = u'' (+u(u^2-1)) by torch autograd, for a torch-expressible u (the reference's
    vmap(grad(grad(u))) construction, model_GP_solver_1d.py:299-307)."""
    import torch
    xt = torch.tensor(np.asarray(x, np.float64).reshape(-1), requires_grad=True)
    u = u_torch(xt)
    g, = torch.autograd.grad(u.sum(), xt, create_graph=True)
    gg, = torch.autograd.grad(g.sum(), xt)
    out = gg.detach().numpy()
    if allen_cahn:
        uv = u.detach().numpy()
        out = out + uv * (uv ** 2 - 1.0)
    return out
