"""GPU: the measurement entry points (gpk_bench_kernel, gpk_time_spd_inverse, gpk_profile_stages)
on the name / inverse-path combinations bench.py runs at full size, at the smallest shapes that
select each path: the times are finite, the reported algorithmic flops and bytes are the closed
forms stated beside each case in the library source (written out again here), the profiled stage
names are the stages the path launches, and the calls leave nothing behind -- parameters and Adam
state bit for bit, and the steps that follow equal to those of a solver that ran no diagnostics
(the step is deterministic: fixed-order reductions, no floating-point atomics)."""
import math

import numpy as np
import pytest

from tests.helpers import device_solver, problem_1d, problem_2d

pytestmark = pytest.mark.gpu

ITERS = 2

# kStageNames2D, the names gpk_stage_name hands out for a 2D handle
STAGES_2D = ["prep", "assemble", "spd_inverse", "gemm_A", "gemm_A_res", "gemm_A_fix", "gemm_B",
             "gemm_B_res", "gemm_B_fix", "gemm_C", "gemm_D", "gemm_D_res", "gemm_D_fix", "gemm_E",
             "pgrad_tail"]


def _pad(n):
    return (n + 31) // 32 * 32


def _gemm_b(n1, n2):
    # S = A K2^{-1} (2 n1 n2^2); R = D1 A + Bt D2^T (2 n1^2 n2 + 2 n1 n2^2)
    flops = 4.0 * n1 * n2 * n2 + 2.0 * n1 * n1 * n2
    # reads A, K2^{-1}, D1, Bt, D2, F, U; writes S, R
    nbytes = 8.0 * (n1 * n2 + n2 * n2 + n1 * n1 + n1 * n2 + n2 * n2 + 2 * n1 * n2 + 2 * n1 * n2)
    return flops, nbytes


def _spd_chain(ns, aug):
    # potrf + potri = n^3 per factor, each augmented column a triangular solve pair (2 n^2);
    # K^{-1}, Kc, D written (24 n^2), augmented outputs written (8 n m), U read
    m = float(sum(ns)) if aug else 0.0
    nu = float(ns[0] * ns[1]) if aug else 0.0
    flops = sum(float(n) ** 3 + 2.0 * n * n * m for n in ns)
    nbytes = sum(24.0 * n * n + 8.0 * n * m + 8.0 * nu for n in ns)
    return flops, nbytes


def _timed(s, name, flops=None, nbytes=None):
    us, fl, by = s.bench_kernel(name, ITERS)
    print(name, "avg_us", us, "alg_flops", fl, "alg_bytes", by)
    assert math.isfinite(us) and us > 0.0, name
    if flops is not None:
        assert fl == flops, (name, fl, flops)
    if nbytes is not None:
        assert by == nbytes, (name, by, nbytes)
    return us, fl, by


def _inverse_time(s):
    us = s.time_spd_inverse(2)
    print("time_spd_inverse", us)
    assert math.isfinite(us) and us > 0.0


def _stages(s, expect):
    st = s.profile_stages(2)
    names = list(st)
    print("profile_stages", st)
    it = iter(STAGES_2D)
    assert all(n in it for n in names), names  # a subsequence of the name table, in its order
    assert names[:3] == ["prep", "assemble", "spd_inverse"] and names[-1] == "pgrad_tail"
    assert names == expect
    assert all(math.isfinite(v) and v >= 0.0 for v in st.values())
    assert sum(st.values()) > 0.0


def _no_residue(make, diagnostics):
    """Run `diagnostics` on one solver; its state is untouched and its next three steps are those
    of a second solver of the same problem that ran none."""
    s, ref = make(), make()
    try:
        flat0 = s.get_flat()
        count0, mu0, nu0 = s.get_opt_state()
        diagnostics(s)
        count1, mu1, nu1 = s.get_opt_state()
        assert np.array_equal(s.get_flat(), flat0)
        assert count1 == count0 and np.array_equal(mu1, mu0) and np.array_equal(nu1, nu0)
        losses, want = s.step(3), ref.step(3)
        assert np.all(np.isfinite(want))
        assert np.array_equal(losses, want)
        assert np.array_equal(s.get_flat(), ref.get_flat())
    finally:
        s.close()
        ref.close()


def test_diag_chain_aug_2d():
    n1, n2, Q = 40, 36, 8
    prob, params, _, fs = problem_2d(n1=n1, n2=n2, Q=Q)

    def make():
        s = device_solver(prob, Q, fs)
        s.set_params(params)
        return s

    def diagnostics(s):
        assert s.inverse_path() == "chain_aug"
        ncls = s.class_counts()
        assert min(ncls) > 0
        _timed(s, "spd_chain", *_spd_chain((n1, n2), True))
        _timed(s, "gemm_B", *_gemm_b(n1, n2))
        _timed(s, "pgrad", 0.0, 16.0 * (n1 * n1 + n2 * n2))  # G_K, G_D read
        # chain + classes: the class values only (distance read, K and D value written per class)
        _timed(s, "assemble", 0.0, 24.0 * sum(ncls))
        _inverse_time(s)
        _stages(s, ["prep", "assemble", "spd_inverse", "gemm_A_res", "gemm_A_fix", "gemm_B",
                    "gemm_B_res", "gemm_B_fix", "gemm_C", "gemm_D_res", "gemm_D_fix", "gemm_E",
                    "pgrad_tail"])

    _no_residue(make, diagnostics)


def test_diag_chain_1d():
    n, Q = 40, 5
    prob, params, _ = problem_1d(n=n, Q=Q)

    def make():
        s = device_solver(prob, Q, 20.0)
        s.set_params(params)
        return s

    def diagnostics(s):
        assert s.inverse_path() == "chain"
        ncls = s.class_counts()
        assert ncls[0] > 0
        _timed(s, "spd_chain", *_spd_chain((n,), False))
        _timed(s, "assemble", 0.0, 24.0 * ncls[0])

    _no_residue(make, diagnostics)


def test_diag_big_wide_2d():
    from gpk._lib import GPK_FLAG_FORCE_BIG_SPD, GPK_FLAG_FORCE_WIDE_SPD
    n1, n2, Q = 200, 150, 5
    prob, params, _, fs = problem_2d(eq="advection", n1=n1, n2=n2, Q=Q)

    def make():
        s = device_solver(prob, Q, fs, flags=GPK_FLAG_FORCE_BIG_SPD | GPK_FLAG_FORCE_WIDE_SPD)
        s.set_params(params)
        return s

    def diagnostics(s):
        assert s.inverse_path() == "big_wide"
        assert min(s.class_counts()) > 0
        _timed(s, "gemm_B", *_gemm_b(n1, n2))
        # per update launch, by the work the tile schedule lists: positive and finite
        _, fl, by = _timed(s, "spd_updates")
        assert math.isfinite(fl) and fl > 0.0 and math.isfinite(by) and by > 0.0
        # per padded element: the int32 class id read (P < 1024: no variant bytes), K, its kept
        # copy Kc and D (advection: D_x1) written
        _timed(s, "gather", 0.0, sum(float(_pad(n)) ** 2 * (4.0 + 8.0 + 8.0 + 8.0) for n in (n1, n2)))
        _inverse_time(s)
        # large factors at beta = 200: the forward solve A alone is refined, no reverse refinement
        _stages(s, ["prep", "assemble", "spd_inverse", "gemm_A", "gemm_A_res", "gemm_A_fix", "gemm_B",
                    "gemm_C", "gemm_D", "gemm_E", "pgrad_tail"])

    _no_residue(make, diagnostics)
