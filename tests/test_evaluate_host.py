"""CPU side of the derivative / scattered-point predictions.

* The NumPy reference of tests/test_gpu_predict_deriv.py is checked against itself: for every case
  those tests use, the LU form and a Cholesky restatement agree within a quarter of the bar, so the
  bar measures the device and not the reference.
* The new Python calls raise GPKError when they cannot reach the library's device path.
* The host-side index helpers of the scattered-point calls (csrc/eval_chunk.h: chunk walk,
  chunk size per grid, the extent of a strided operand) in a stand-alone program built with the
  address and undefined-behaviour sanitizers.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import predict_deriv_ref as R
from tests.conftest import ROOT
from tests.helpers import rel

CSRC = os.path.join(ROOT, "gaussian-process-slover-for-high-freq-pde_amd", "csrc")


def _stable(prob, params, ms, derivs, label):
    tol = R.bar(prob, params)
    xte = R.grid_axes(prob, params, ms)
    pts = R.random_points(prob, params, R.N_RANDOM)
    worst = 0.0
    for d in derivs:
        g = rel(R.ref_grid(prob, params, xte, d, R.chol_solve), R.ref_grid(prob, params, xte, d))
        p = rel(R.ref_points(prob, params, pts, d, R.chol_solve), R.ref_points(prob, params, pts, d))
        worst = max(worst, g, p)
    print(label, ms, "LU - Cholesky distance / bar", worst / tol)
    assert worst < 0.25 * tol, (label, ms, worst, tol)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("eq,ns", R.CASES_2D)
def test_reference_is_stable_2d(eq, ns, kind):
    prob, params, _ = R.case_2d(eq, ns, kind)
    for ms in R.MS_2D + [(11, 7)]:
        _stable(prob, params, ms, R.DERIVS_2D, (eq, ns, kind))


@pytest.mark.parametrize("eq,n", R.CASES_1D)
def test_reference_is_stable_1d(eq, n):
    prob, params, _ = R.case_1d(eq, n)
    _stable(prob, params, (R.M_1D,), [(0,), (1,), (2,)], (eq, n))


@pytest.mark.parametrize("ns,ms", R.CASES_3D)
def test_reference_is_stable_3d(ns, ms):
    prob, params, _ = R.case_3d(ns)
    _stable(prob, params, ms, R.DERIVS_3D, ns)


def test_reference_is_stable_3d_many_points():
    prob, params, _ = R.case_3d((20, 14, 9))
    pts = R.random_points(prob, params, 1500, seed=11)
    d = (1, 0, 2)
    dist = rel(R.ref_points(prob, params, pts, d, R.chol_solve), R.ref_points(prob, params, pts, d))
    assert dist < 0.25 * R.bar(prob, params)


def test_points_reference_is_the_grid_reference_on_a_grid():
    prob, params, _ = R.case_3d((20, 14, 9))
    xte = R.grid_axes(prob, params, (3, 4, 5))
    pts = np.stack(np.meshgrid(*xte, indexing="ij"), -1).reshape(-1, 3)
    for d in R.DERIVS_3D:
        assert rel(R.ref_points(prob, params, pts, d), R.ref_grid(prob, params, xte, d).ravel()) < 1e-13


def test_new_calls_raise_without_a_handle_or_device():
    from gpk import _lib
    from gpk.core import DeviceSolver
    from gpk.model_GP_solver_3d import DeviceSolver3
    x = np.linspace(0, 1, 5)
    s = DeviceSolver.__new__(DeviceSolver)  # no handle: the library refuses, nothing is computed
    s._h, s.dim = None, 2
    with pytest.raises(_lib.GPKError):
        s.predict_deriv(x, x, deriv=(1, 0))
    with pytest.raises(_lib.GPKError):
        s.evaluate(np.zeros((3, 2)), deriv=(0, 2))
    s3 = DeviceSolver3.__new__(DeviceSolver3)
    s3._h = None
    with pytest.raises(_lib.GPKError):
        s3.predict_deriv(x, x, x, deriv=(1, 0, 0))
    with pytest.raises(_lib.GPKError):
        s3.evaluate(np.zeros((3, 3)), deriv=(0, 0, 2))
    with pytest.raises(ValueError):
        s.predict_deriv(x, x, deriv=(1, 0, 0))
    kp = {"log-w": np.zeros(3), "log-ls": np.zeros(3), "freq": np.ones(3)}
    with pytest.raises(_lib.GPKError):  # argument validation comes before any device work
        _lib.point_contract("Matern52_1d", x, x, kp, np.zeros((5, 5, 1)), deriv=3)
    with pytest.raises(ValueError):     # T shorter than the strides address
        _lib.point_contract("Matern52_1d", x, x, kp, np.zeros((5, 4, 1)))
    n = ctypes.c_int32(-1)
    assert _lib.load().gpk_device_count(ctypes.byref(n)) == _lib.GPK_OK
    if n.value == 0:  # no device: the diagnostic raises instead of computing on the host
        with pytest.raises(_lib.GPKError):
            _lib.point_contract("Matern52_1d", x, x, kp, np.zeros((5, 5, 1)))


MAIN = r"""
#include <cstdio>
#include <vector>
#include "eval_chunk.h"

int main() {
  int bad = 0;
  // the chunk walk covers every point exactly once, in order, each chunk within its buffer
  const int chunks[] = {1, 32, 1000, EVAL_CHUNK3, EVAL_CHUNK};
  const long long ms[] = {1, 31, 1023, 1024, 1025, 1500, 4096, 5000, 8193};
  for (int chunk : chunks)
    for (long long m : ms) {
      std::vector<char> seen((size_t)m, 0);
      std::vector<double> buf((size_t)chunk);
      long long next = 0;
      for (int64_t k = 0; k < chunk_count(m, chunk); ++k) {
        const int64_t p0 = chunk_begin(k, chunk);
        const int mc = chunk_size(m, k, chunk);
        if (p0 != next || mc < 1 || mc > chunk) ++bad;
        for (int i = 0; i < mc; ++i) { buf[(size_t)i] = (double)(p0 + i); ++seen[(size_t)(p0 + i)]; }
        next = p0 + mc;
      }
      if (next != m || chunk_size(m, chunk_count(m, chunk), chunk) != 0) ++bad;
      for (char c : seen) bad += c != 1;
    }
  // the 3-axis chunk: a multiple of 32 in [32, 1024] whose tensor stays under the cap when it can
  const size_t slabs[] = {1, 32 * 32, 64 * 64, 512 * 512, 1024 * 1024, (size_t)1 << 40};
  for (size_t s : slabs) {
    const int c = eval3_chunk(s);
    if (c < 32 || c > EVAL_CHUNK3 || c % 32) ++bad;
    if (c > 32 && (size_t)c * s > EVAL_TENSOR_CAP) ++bad;
  }
  if (eval3_chunk(32 * 32) != 1024 || eval3_chunk(64 * 64) != 1024 || eval3_chunk(1024 * 1024) != 256) ++bad;
  // the operand extent: every index the kernel forms lies below it, and the last one reaches it
  struct { long long m, n, C, sp, sj, sc; } cs[] = {
      {5, 7, 1, 0, 1, 1}, {5, 7, 3, 21, 3, 1}, {4, 33, 33, 64 * 64, 64, 1}, {3, 9, 32, 14 * 32, 32, 1}, {2, 4, 2, 1, 3, 50}};
  for (auto& c : cs) {
    const size_t ext = point_contract_extent(c.m, c.n, c.C, c.sp, c.sj, c.sc);
    std::vector<double> T(ext, 1.0);
    double sum = 0.0;
    size_t top = 0;
    for (long long p = 0; p < c.m; ++p)
      for (long long j = 0; j < c.n; ++j)
        for (long long k = 0; k < c.C; ++k) {
          const size_t i = (size_t)(p * c.sp + j * c.sj + k * c.sc);
          sum += T[i];
          top = i > top ? i : top;
        }
    if (top + 1 != ext || sum != (double)(c.m * c.n * c.C)) ++bad;
  }
  if (point_contract_extent(0, 1, 1, 0, 1, 1) || point_contract_extent(1, 1, 1, -1, 1, 1) ||
      point_contract_extent(1, 1, 1, 0, 0, 1) || point_contract_extent(1, 1, 1, 0, 1, 0) ||
      point_contract_extent(2, 2, 2, INT64_MAX, INT64_MAX, INT64_MAX))
    ++bad;
  std::printf("%d\n", bad);
  return bad != 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_chunk_helpers_under_sanitizers(tmp_path):
    cpp = tmp_path / "chunks.cpp"
    cpp.write_text(MAIN)
    exe = tmp_path / "chunks"
    # (the sanitizer runtimes linked into the program itself: it depends on no library load order)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", CSRC, str(cpp), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.strip() == "0", (r.stdout, r.stderr)
