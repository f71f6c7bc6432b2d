"""GPU: the chain inverse's launch protocol (spdinv.hip chain_kernel / chain_multi_kernel).  A panel
flag carries its launch's tag (the factor's epoch + 1) and is never cleared; every workgroup of a
chain_kernel factor arrives once on a `started` word after its last use of the epoch, and the
pivot workgroup advances the epoch (whose parity selects the half of the L^{-1} / panel slots a
launch uses); chain_multi_kernel advances it from its last workgroup to exit.

What can go wrong: a word left by an earlier launch -- possibly one with another flag layout, the
step's augmented launch (TC = T + tu + td) and the K^{-1}-only launch (TC = T) share one buffer --
accepted as this launch's flag; an epoch advance that is missed or doubled (the launch then reads
the half its tiles are resetting).  Either changes bits of K^{-1}, so every check is bitwise, against
a handle whose launches differ (no K^{-1}-only launch in between, single-step calls, a fresh
handle) or that does not use the chain's flags at all (GPK_FLAG_NO_CHAIN: one launch per sweep).
That reference is bitwise for the inverse without augmented columns only (GPK_FLAG_NO_CHAIN_AUG;
tests/test_gpu_chain_lookahead.py's docstring).

These are race tests: they show a fault's presence, not its absence.  Shapes are the smallest with
T = 1 (no hand-off), 2, unequal factors (3 and 2: the two factors' active counts differ) and 4
with 3."""
import numpy as np
import pytest

from tests.helpers import device_solver, problem_1d, problem_2d

pytestmark = pytest.mark.gpu


def _state(s):
    c, mu, nu = s.get_opt_state()
    return np.array(s.get_flat()), c, np.array(mu), np.array(nu)


def _same_state(a, b):
    assert a[1] == b[1]
    for i in (0, 2, 3):
        assert np.array_equal(a[i], b[i])


def _same_lg(a, b):
    assert a[0] == b[0]
    assert np.array_equal(np.asarray(a[1]), np.asarray(b[1]))


def _mixed(prob, params, fs, flags, inverse_only, path=("chain", "chain_aug")):
    """loss_grad, step(3), [the K^{-1}-only launch], step(3), loss_grad on one handle."""
    s = device_solver(prob, 5, fs, flags=flags)
    try:
        assert s.inverse_path() in path, s.inverse_path()
        s.set_params(params)
        first = s.loss_grad()
        if inverse_only:
            losses = s.step(3)
            s.time_spd_inverse(1)
            losses = np.concatenate([losses, s.step(3)])
        else:
            losses = s.step(6)
        last = s.loss_grad()
        s.sync()
        return first, np.array(losses), last, _state(s)
    finally:
        s.close()


@pytest.mark.parametrize("aug", [True, False])
@pytest.mark.parametrize("n1,n2", [(24, 24), (40, 40), (72, 40), (100, 72)])
def test_launches_of_two_layouts_share_the_flags(n1, n2, aug):
    """The step's launches with a K^{-1}-only launch between them leave the state of step(6).  With
    augmented columns the two layouts differ; without them, both handles' losses and gradients
    are also those of the launch-per-sweep inverse."""
    from gpk import _lib as L
    flags = 0 if aug else L.GPK_FLAG_NO_CHAIN_AUG
    prob, params, _, fs = problem_2d(n1=n1, n2=n2, Q=5, seed=3)
    a = _mixed(prob, params, fs, flags, True)
    b = _mixed(prob, params, fs, flags, False)
    _same_lg(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    _same_lg(a[2], b[2])
    _same_state(a[3], b[3])
    if not aug:
        c = _mixed(prob, params, fs, flags | L.GPK_FLAG_NO_CHAIN, False, path=("sweep",))
        _same_lg(b[0], c[0])
        assert np.array_equal(b[1], c[1])
        _same_lg(b[2], c[2])
        _same_state(b[3], c[3])


@pytest.mark.parametrize("lookahead", [True, False])
@pytest.mark.parametrize("n1,n2", [(72, 40), (100, 72)])
def test_many_launches_back_to_back(n1, n2, lookahead):
    """step(40) in one call equals 40 x step(1); the plain protocol (no look-ahead) waits on more
    hand-offs per launch."""
    from gpk import _lib as L
    flags = 0 if lookahead else L.GPK_FLAG_NO_CHAIN_LOOKAHEAD
    prob, params, _, fs = problem_2d(n1=n1, n2=n2, Q=5, seed=1)
    a = device_solver(prob, 5, fs, flags=flags)
    b = device_solver(prob, 5, fs, flags=flags)
    try:
        for s in (a, b):
            s.set_params(params)
        la = a.step(40)
        lb = np.concatenate([b.step(1) for _ in range(40)])
        assert np.array_equal(la, lb)
        a.sync()
        b.sync()
        _same_state(_state(a), _state(b))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("n,multi", [(24, False), (72, False), (72, True), (100, True)])
def test_trajectory_1d_and_macro_tile_chain(n, multi):
    """1D, and chain_multi_kernel forced at small sizes: loss, gradient and a 6-step trajectory are
    bitwise those of the launch-per-sweep inverse."""
    from gpk import _lib as L
    flags = L.GPK_FLAG_FORCE_CHAIN_MULTI if multi else 0
    prob, params, _ = problem_1d(n=n, Q=5, seed=2)
    out = []
    for fl, path in ((flags, "chain_multi" if multi else "chain"), (L.GPK_FLAG_NO_CHAIN, None)):
        s = device_solver(prob, 5, 20.0, flags=fl)
        try:
            assert path is None or s.inverse_path() == path, s.inverse_path()
            s.set_params(params)
            lg = s.loss_grad()
            losses = np.array(s.step(6))
            s.sync()
            out.append((lg, losses, s.loss_grad(), _state(s)))
        finally:
            s.close()
    a, b = out
    _same_lg(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    _same_lg(a[2], b[2])
    _same_state(a[3], b[3])


@pytest.mark.parametrize("launches", [1, 2])
def test_epoch_parity(launches):
    """After an odd and after an even number of chain launches the next launch is a fresh
    handle's first."""
    prob, params, _, fs = problem_2d(n1=40, n2=72, Q=5, seed=3)
    s = device_solver(prob, 5, fs)
    f = device_solver(prob, 5, fs)
    try:
        s.set_params(params)
        f.set_params(params)
        for _ in range(launches):
            s.loss_grad()
        _same_lg(s.loss_grad(), f.loss_grad())
    finally:
        s.close()
        f.close()
