"""GPU: the pivot chain's two-block look-ahead (spdinv.hip chain_master_la; include/gpk.h
GPK_FLAG_NO_CHAIN_LOOKAHEAD restores the plain hand-off protocol).  The pivot workgroup forms each
pivot's input tiles itself, with the tile owners' own operation sequence, so every result is
bitwise that of the plain protocol and of the one-launch-per-sweep inverse (GPK_FLAG_NO_CHAIN).

Shapes: the smallest at which the window can go wrong -- T = 1 (no hop), 2 (a hop, no
look-ahead), 3 (the first full window; its last hop has none), 4, and 2D factors of unequal size
(the two chains of one launch run different hop counts).  The T cases run as 2D squares, so that
all four ways exist (augmented columns are a 2D feature, advection a 2D equation), and in 1D.

Reference: the handle with GPK_FLAG_NO_CHAIN_LOOKAHEAD at the same flags, always; and the
GPK_FLAG_NO_CHAIN handle for the inverse without augmented columns -- with them the chain solves
A, Bt and K^{-1} D^T by the sweep operator, which GPK_FLAG_NO_CHAIN (explicit-inverse GEMMs)
matches to rounding only (tests/test_gpu_chain.py), with or without the look-ahead."""
import numpy as np
import pytest

from tests.helpers import device_solver, problem_1d, problem_2d

pytestmark = pytest.mark.gpu

SHAPES_2D = [(24, 24), (40, 40), (72, 72), (100, 100), (24, 100), (40, 72)]
WAYS = ["aug", "noaug", "nodclass", "adv"]


def _flags():
    from gpk import _lib
    return _lib


def _trajectory(prob, params, Q, fs, flags):
    s = device_solver(prob, Q, fs, flags=flags)
    try:
        s.set_params(params)
        loss, grad = s.loss_grad()
        losses = s.step(6)
        return loss, np.array(grad), np.array(losses), np.array(s.get_flat())
    finally:
        s.close()


def _same(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("n1,n2", SHAPES_2D)
def test_lookahead_bitwise_2d(n1, n2, way):
    L = _flags()
    eq = "advection" if way == "adv" else "poisson"
    flags = {"aug": 0, "noaug": L.GPK_FLAG_NO_CHAIN_AUG, "nodclass": L.GPK_FLAG_NO_DCLASS, "adv": 0}[way]
    prob, params, _, fs = problem_2d(eq=eq, n1=n1, n2=n2, Q=5, seed=3)
    a = _trajectory(prob, params, 5, fs, flags)
    _same(a, _trajectory(prob, params, 5, fs, flags | L.GPK_FLAG_NO_CHAIN_LOOKAHEAD))
    # against the per-sweep launches: the inverse alone (module docstring)
    noaug = flags | L.GPK_FLAG_NO_CHAIN_AUG
    d = a if noaug == flags else _trajectory(prob, params, 5, fs, noaug)
    _same(d, _trajectory(prob, params, 5, fs, noaug | L.GPK_FLAG_NO_CHAIN))


@pytest.mark.parametrize("dclass", [True, False])
@pytest.mark.parametrize("n", [24, 40, 72, 100])
def test_lookahead_bitwise_1d(n, dclass):
    L = _flags()
    flags = 0 if dclass else L.GPK_FLAG_NO_DCLASS
    prob, params, _ = problem_1d(n=n, Q=5, seed=2)
    a = _trajectory(prob, params, 5, 20.0, flags)
    _same(a, _trajectory(prob, params, 5, 20.0, flags | L.GPK_FLAG_NO_CHAIN_LOOKAHEAD))
    _same(a, _trajectory(prob, params, 5, 20.0, flags | L.GPK_FLAG_NO_CHAIN))


@pytest.mark.parametrize("n1,n2", [(72, 40), (100, 72)])
def test_lookahead_slots_rearm(n1, n2):
    """72x40 (T = 3 and 2: slot 0 only) and 100x72 (T = 4: slots 0 and 1): 40 steps in one call
    equal 40 single-step calls -- every look-ahead slot is back at the sentinel after every
    launch, captured batch or not."""
    prob, params, _, fs = problem_2d(n1=n1, n2=n2, Q=5, seed=1)
    a = device_solver(prob, 5, fs)
    b = device_solver(prob, 5, fs)
    try:
        for s in (a, b):
            s.set_params(params)
        la = a.step(40)
        lb = np.concatenate([b.step(1) for _ in range(40)])
        assert np.array_equal(la, lb)
        assert np.array_equal(a.get_flat(), b.get_flat())
    finally:
        a.close()
        b.close()
