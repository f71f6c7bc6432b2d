"""GPU: the one-wave pivot factorisation's block steps (spd_pivot.h pivot_chol_inv_1w).  A block
step issues only the rank-4 updates whose operands are not structurally zero; chain_master /
chain_master_la (spdinv.hip) reach the factorisation from one call site, pivot 0 included.  Every
accumulator still receives the same non-zero updates in the same order, so every result equals
(np.array_equal) that of the four-wave form pivot_chol_inv_block, which chain_multi_kernel keeps.

Shapes: the smallest at which a step can go wrong.  With n real rows the last 32-row pivot block
holds n - 32 (T - 1) of them and identity padding below:
    n     33  40  48  50  52  64  65  97
    rows   1   8  16  18  20  32   1   1      T = 2 2 2 2 2 2 3 4
i.e. the padding starts in the first tile row (33, 40), exactly at the tile-row boundary (48),
inside a 4-column block (50), on a 4-boundary of the second tile row (52), nowhere (64).
"""
import numpy as np
import pytest

from tests.helpers import device_solver, problem_1d, problem_2d

pytestmark = pytest.mark.gpu


def _same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("kind", ["Matern52_Cos_1d", "SE_1d"])
@pytest.mark.parametrize("n", [33, 40, 48, 50, 52, 64, 65, 97])
def test_one_wave_pivot_equals_four_wave_form(n, kind):
    """chain (one-wave pivot) against the forced macro-tile chain (four-wave pivot): loss, full
    gradient, a 3-step trajectory, the parameters after it and the predictions."""
    from gpk._lib import GPK_FLAG_FORCE_CHAIN_MULTI
    prob, params, (Xte, _) = problem_1d(eq="poisson", kind=kind, n=n, Q=6, seed=5)
    out = []
    for flags, path in ((0, "chain"), (GPK_FLAG_FORCE_CHAIN_MULTI, "chain_multi")):
        s = device_solver(prob, 6, 20.0, flags=flags)
        try:
            assert s.inverse_path() == path
            s.set_params(params)
            loss, g = s.loss_grad()
            losses = s.step(3)
            out.append((loss, g, losses, s.get_flat(), s.predict(Xte)))
        finally:
            s.close()
    _same(out[0], out[1])


@pytest.mark.parametrize("n1,n2", [(40, 72), (100, 100)])
def test_both_masters_agree_and_batches_equal_single_steps(n1, n2):
    """2D: both factors' chains in one launch, look-ahead and augmented columns on.  The
    look-ahead master against the plain one (GPK_FLAG_NO_CHAIN_LOOKAHEAD), both through the single
    call site; and forty steps in one call against forty step(1) calls."""
    from gpk._lib import GPK_FLAG_NO_CHAIN_LOOKAHEAD
    prob, params, _, fs = problem_2d(n1=n1, n2=n2, Q=5, seed=1)
    a = device_solver(prob, 5, fs)
    b = device_solver(prob, 5, fs)
    c = device_solver(prob, 5, fs, flags=GPK_FLAG_NO_CHAIN_LOOKAHEAD)
    try:
        res = []
        for s in (a, b, c):
            s.set_params(params)
            res.append(s.loss_grad())
        _same(res[0], res[2])
        la = a.step(40)
        lb = np.concatenate([b.step(1) for _ in range(40)])
        lc = c.step(40)
        assert np.array_equal(la, lb)
        assert np.array_equal(la, lc)
        assert np.array_equal(a.get_flat(), b.get_flat())
        assert np.array_equal(a.get_flat(), c.get_flat())
    finally:
        for s in (a, b, c):
            s.close()


@pytest.mark.parametrize("axis", [1, 2])
def test_not_positive_definite_still_reported(axis):
    """log-w[0] = NaN on one axis: that factor is all NaN, no pivot is positive, and the step must
    end in GPK_ENOTPD (status bit 1 from pv[], which every block step still writes).  The handle
    then takes good parameters and returns what a fresh handle returns."""
    from gpk._lib import GPKError, GPK_ENOTPD
    prob, params, _, fs = problem_2d(eq="poisson", kind="Matern52_Cos_1d", n1=72, n2=64, Q=4, seed=8)
    bad = {k: (dict(v) if isinstance(v, dict) else v) for k, v in params.items()}
    kp = dict(bad[f"kernel_paras_{axis}"])
    kp["log-w"] = np.array(kp["log-w"], dtype=float)
    kp["log-w"][0] = np.nan
    bad[f"kernel_paras_{axis}"] = kp
    s = device_solver(prob, 4, fs)
    f = device_solver(prob, 4, fs)
    try:
        assert s.inverse_path() == "chain_aug"  # (the default 2D path: chain_kernel)
        s.set_params(bad)
        with pytest.raises(GPKError) as ei:
            s.loss_grad()
        assert ei.value.code == GPK_ENOTPD, str(ei.value)
        s.set_params(params)
        f.set_params(params)
        _same(s.loss_grad(), f.loss_grad())
    finally:
        s.close()
        f.close()
