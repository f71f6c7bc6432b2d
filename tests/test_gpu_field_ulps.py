"""GPU: the device's K and D, element by element, against the exact fields
(oracle/gp_oracle.py kernel_block_exact: long double, the phase as an exact fp64 pair) in the
regime the project is named for -- high frequency, large arguments -- on every route by which the
device evaluates fields:

  per-pair block            gpk.core.kernel_matrices (rectangular 37 x 29 with a zero distance off
                            the diagonal and a duplicated point; square 33 with jitter)
  pairs                     gpk.core.kernel_pairs on the same pairs, flattened
  step, class values        DeviceSolver.forward_field (1D Kc, D; 2D Kc1, Kc2, D1, D2), default
                            flags, the class path asserted (class_counts)
  step, per-pair assembly   the same fields with GPK_FLAG_NO_DCLASS, and a scattered x, which falls
                            back to the per-pair kernels by itself

four kinds, deriv 0 / 1 / 2 (the step: Poisson = 2, advection = 1).  Inputs:
tests/field_ulp_inputs.py, shared with the CPU test of this test's power
(tests/test_oracle.py test_field_test_power: the plain fp64 evaluation -- the low-part corrections
of csrc/gpk_internal.h om_low / phase_sincos / radial_exp deleted -- misses the bar by 2x or more on
every discriminating case).

Error unit: |device - exact| / (eps B), eps = 2^-52, B the field with every monomial taken in
absolute value (O.field_scale), so zeros of the polynomial and cancellation between components do
not make the unit meaningless; where B = 0 (D_x1 at d = 0 without a cosine) the device must return
exactly 0.  Bar: N_K = 8, N_D = 12 units, from the operation count of eval_kd_part per component
-- exp and sincos at <= 2 ulp each, one fma correction each, <= 3 polynomial roundings, two or four
products, a three-term sum for D, <= 2 for accumulating Q <= 64 terms by butterfly or serially --
derived, not measured.  The generic regimes (random log-ls, log-w) add the fields' sensitivity to a
2-ulp difference in the device's own a = exp(log-ls), w = exp(log-w) (tests/helpers.py
field_bars).  On the step routes K carries the jitter: the same fp64 jitter is added to the rounded
exact diagonal, as kernel_kd_exact does.  D_x1 carries the sign s_ij: every block is compared in
full, both triangles.

Out of scope: the pipelined class values and the wide gather (tested bitwise against the routes
here: tests/test_gpu_cls_pipe.py, tests/test_gpu_dclass.py) and the 3-axis solver (no field
readback).

Observed maxima (MI355X, units; recorded per route, kind and regime in the parity log,
tests/helpers.record_parity): block K 2.7, D 2.8; pairs K 2.6, D 2.8; step class values K 2.0,
D 2.2; step per-pair assembly K 2.0, D 2.2; scattered axis K 2.3, D 2.2.  A library built with the
low-part corrections disabled fails every discriminating case on every route."""
import functools

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import field_ulp_inputs as FI
from tests.helpers import device_solver, field_bars, field_units as _units, problem_1d, problem_2d, record_parity

pytestmark = pytest.mark.gpu

JITTER = 1e-6


@functools.lru_cache(maxsize=None)
def _reference(regime, kind, block, deriv):
    """(exact long-double block, B, bar) of a named block of tests/field_ulp_inputs.py -- computed
    once, shared by every route that evaluates the block, never modified."""
    name, x1, x2 = next(b for b in FI.blocks(regime, kind) if b[0] == block)
    kp = FI.kernel_paras(regime)
    ex = O.kernel_block_exact(kind, x1, x2, kp, deriv)
    BK, BD, barK, barD = field_bars(regime, kind, x1, x2, kp, deriv if deriv else 2)
    out = (ex, BK, barK) if deriv == 0 else (ex, BD, barD)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _check(dev, regime, kind, block, deriv, jitter=0.0):
    """max error of a device block in bar units and in plain units (asserted by the caller)."""
    ex, B, bar = _reference(regime, kind, block, deriv)
    if jitter:  # K of a step: the jitter added in fp64 to the rounded exact diagonal
        ex = ex.astype(np.float64)
        ex[np.diag_indices_from(ex)] += jitter
    assert dev.shape == ex.shape and np.isfinite(dev).all()
    return _units(dev, ex, B, bar), _units(dev, ex, B)


def _finish(route, kind, regime, res):
    errs = {k: v[1] for k, v in res.items()}
    record_parity("test_gpu_field_ulps", f"{route}/{kind}/{regime}", errs,
                  {"K": FI.N_K, "D": FI.N_D}, {"of_bar": {k: v[0] for k, v in res.items()}})
    print(route, kind, regime, {k: round(v, 3) for k, v in errs.items()})
    bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
    assert not bad, (route, kind, regime, bad)


@pytest.mark.parametrize("regime", FI.REGIMES)
@pytest.mark.parametrize("kind", FI.KINDS)
def test_block_and_pairs_routes(kind, regime):
    from gpk.core import kernel_matrices, kernel_pairs
    kp = FI.kernel_paras(regime)
    x1, x2 = FI.rect_block(regime, kind)
    xs = FI.square_block(regime, kind)
    a, b = np.repeat(x1, x2.size), np.tile(x2, x1.size)
    blk, prs = {}, {}
    for deriv in (0, 1, 2):
        K, D = kernel_matrices(kind, x1, x2, kp, 0.0, deriv)
        blk[f"rect/K@{deriv}"] = _check(K, regime, kind, "rect", 0)
        Ks, Ds = kernel_matrices(kind, xs, xs, kp, JITTER, deriv)
        blk[f"square/K@{deriv}"] = _check(Ks, regime, kind, "square", 0, JITTER)
        if deriv:
            blk[f"rect/D{deriv}"] = _check(D, regime, kind, "rect", deriv)
            blk[f"square/D{deriv}"] = _check(Ds, regime, kind, "square", deriv)
        v = kernel_pairs(kind, a, b, kp, deriv).reshape(x1.size, x2.size)
        prs["K" if deriv == 0 else f"D{deriv}"] = _check(v, regime, kind, "rect", deriv)
    _finish("block", kind, regime, blk)
    _finish("pairs", kind, regime, prs)


def _step_solver(dim, eq, kind, regime, xs, flags):
    """A solver on the axes xs with the regime's kernel parameters on every axis."""
    kp = FI.kernel_paras(regime)
    Q = len(kp["freq"])
    if dim == 1:
        prob, params, _ = problem_1d(eq=eq, kind=kind, n=len(xs[0]), Q=Q, seed=1)
        prob = dict(prob, x=xs[0], jitter=JITTER)
        params = dict(params, kernel_paras=kp)
        fs = 20.0
    else:
        prob, params, _, fs = problem_2d(eq=eq, kind=kind, n1=len(xs[0]), n2=len(xs[1]), Q=Q, seed=1)
        prob = dict(prob, x1=xs[0], x2=xs[1], jitter=JITTER)
        params = dict(params, kernel_paras_1=kp, kernel_paras_2=kp)
    s = device_solver(prob, Q, fs, flags=flags)
    s.set_params(params)
    return s


def _step_fields(s, dim, kind, regime, blocks, deriv):
    res = {}
    names = [("Kc", "D")] if dim == 1 else [("Kc1", "D1"), ("Kc2", "D2")]
    for (kn, dn), block in zip(names, blocks):
        res[f"{kn}[{block}]"] = _check(s.forward_field(kn), regime, kind, block, 0, JITTER)
        res[f"{dn}[{block}]@{deriv}"] = _check(s.forward_field(dn), regime, kind, block, deriv)
    return res


STEPS = [(1, "poisson", 2), (2, "poisson", 2), (2, "advection", 1)]


@pytest.mark.parametrize("regime", FI.REGIMES)
@pytest.mark.parametrize("dim,eq,deriv", STEPS)
@pytest.mark.parametrize("kind", FI.KINDS)
def test_step_routes(kind, dim, eq, deriv, regime):
    from gpk._lib import GPK_FLAG_NO_DCLASS
    blocks = ["grid33", "grid40"][:dim]
    xs = [FI.grid(regime, kind, n) for n in (33, 40)][:dim]
    for route, flags in (("step_class", 0), ("step_pairs", GPK_FLAG_NO_DCLASS)):
        s = _step_solver(dim, eq, kind, regime, xs, flags)
        try:
            counts = s.class_counts()
            assert all(c > 0 for c in counts) if flags == 0 else all(c == 0 for c in counts), counts
            res = _step_fields(s, dim, kind, regime, blocks, deriv)
        finally:
            s.close()
        _finish(f"{route}/{dim}d_{eq}", kind, regime, res)


@pytest.mark.parametrize("dim,eq,deriv", STEPS)
@pytest.mark.parametrize("kind", FI.KINDS)
def test_step_scattered_axis_falls_back_to_pairs(kind, dim, eq, deriv):
    """Default flags, a scattered first axis: more than 32 distances per diagonal, so the step
    assembles per pair by itself (every axis: class_counts all 0)."""
    regime = "radial"
    xs = [FI.scattered(regime, kind, 40, 14), FI.grid(regime, kind, 40)][:dim]
    s = _step_solver(dim, eq, kind, regime, xs, 0)
    try:
        assert all(c == 0 for c in s.class_counts())
        res = _step_fields(s, dim, kind, regime, ["scattered", "grid40"][:dim], deriv)
    finally:
        s.close()
    _finish(f"step_scattered/{dim}d_{eq}", kind, regime, res)
