// point_eval.hip — contraction of a tensor with a kernel field evaluated on the fly at scattered
// points (gpk_internal.h PointContract; gpk_evaluate / gpk_evaluate3, gpk_point_contract):
//   out[p][c] = sum_{j < n} field(t[p] - x[j]) * T[p * sp + j * sj + c * sc],   c < C,
// field = kappa / D_x1_kappa / DD_x1_kappa (deriv 0 / 1 / 2; the point is the first argument).
// The field is eval_kd on t[p] - x[j] with the axis constants staged in LDS exactly as
// cross_kernel stages them: the values of gpk_kernel_matrices, no Kmn matrix in memory.  Only the
// n real collocation points are visited; T's padding is never read.
//
// Two regimes, no atomics, a summation order fixed by (n, C):
//   C = 1  (point_dot_kernel): one wave per point, four points per workgroup.  Lane l adds the
//          terms j = l, l + 64, ... in ascending order, then the 64 lane sums go through a fixed
//          xor butterfly.
//   C > 1  (point_cols_kernel): one workgroup per point.  Its threads write the point's n field
//          values to LDS (n <= POINT_MAX_N = 4096: 32 KiB), and after one barrier thread c owns
//          column c, reads T coalesced along c and adds over j in ascending order.  With C wider
//          than the workgroup the workgroup loops over its column blocks: the field row costs q
//          exp / sincos pairs per j against one load and one FMA per (j, c), so it is evaluated
//          once per point, not once per column block.
#include <algorithm>

#include "gpk_internal.h"
#include "prep_dev.h"

namespace gpk {

namespace {

__device__ __forceinline__ void stage_axis(const AxisConst* kc, int q, double* sw, double* sa,
                                           double* so, double* sol) {
  const int t = threadIdx.x;
  if (t < q) {
    sw[t] = kc->w[t];
    sa[t] = kc->a[t];
    so[t] = kc->om[t];
    sol[t] = kc->oml[t];
  }
  __syncthreads();
}

template <bool MATERN, bool COS, int DERIV>
__global__ __launch_bounds__(256) void point_dot_kernel(PointContract a) {
  __shared__ double sw[QMAX], sa[QMAX], so[QMAX], sol[QMAX];
  stage_axis(a.kc, a.q, sw, sa, so, sol);
  const int lane = threadIdx.x & 63;
  const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= a.m) return;  // (whole waves: no barrier follows)
  const double tp = a.t[p];
  const double* __restrict__ T = a.T + (size_t)p * a.sp;
  double acc = 0.0;
  for (int j = lane; j < a.n; j += 64) {
    double kv, dv;
    eval_kd<MATERN, COS, DERIV>(tp - a.x[j], sw, sa, so, sol, a.q, kv, dv);
    acc += (DERIV ? dv : kv) * T[(size_t)j * a.sj];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) a.out[p] = acc;
}

template <bool MATERN, bool COS, int DERIV>
__global__ __launch_bounds__(256) void point_cols_kernel(PointContract a) {
  __shared__ double sw[QMAX], sa[QMAX], so[QMAX], sol[QMAX];
  __shared__ double F[POINT_MAX_N];
  stage_axis(a.kc, a.q, sw, sa, so, sol);
  const int t = threadIdx.x, nt = blockDim.x;
  const long p = blockIdx.x;
  const double tp = a.t[p];
  for (int j = t; j < a.n; j += nt) {
    double kv, dv;
    eval_kd<MATERN, COS, DERIV>(tp - a.x[j], sw, sa, so, sol, a.q, kv, dv);
    F[j] = DERIV ? dv : kv;
  }
  __syncthreads();
  const double* __restrict__ T = a.T + (size_t)p * a.sp;
  for (int c = t; c < a.C; c += nt) {
    const double* __restrict__ Tc = T + (size_t)c * a.sc;
    double acc = 0.0;
    for (int j = 0; j < a.n; ++j) acc += F[j] * Tc[(size_t)j * a.sj];
    a.out[(size_t)p * a.C + c] = acc;
  }
}

template <bool MATERN, bool COS, int DERIV>
void launch_t(const PointContract& a, hipStream_t s) {
  if (a.C == 1) {
    hipLaunchKernelGGL((point_dot_kernel<MATERN, COS, DERIV>), dim3((unsigned)((a.m + 3) / 4)), dim3(256), 0, s, a);
  } else {
    // (a workgroup of whole waves just wide enough for the columns, at most 256 threads)
    const int nt = std::min(256, (a.C + 63) / 64 * 64);
    hipLaunchKernelGGL((point_cols_kernel<MATERN, COS, DERIV>), dim3((unsigned)a.m), dim3(nt), 0, s, a);
  }
}

template <bool MATERN, bool COS>
void launch_d(const PointContract& a, int deriv, hipStream_t s) {
  if (deriv == 2) launch_t<MATERN, COS, 2>(a, s);
  else if (deriv == 1) launch_t<MATERN, COS, 1>(a, s);
  else launch_t<MATERN, COS, 0>(a, s);
}

}  // namespace

hipError_t launch_point_contract(int kind, int deriv, const PointContract& a, hipStream_t s) {
  if (a.m < 1 || a.n < 1 || a.C < 1 || a.q < 1 || a.q > QMAX || deriv < 0 || deriv > 2 ||
      (a.C > 1 && a.n > POINT_MAX_N) || (a.C == 1 ? (a.m + 3) / 4 : a.m) > 0x7fffffffL)
    return hipErrorInvalidValue;
  switch (kind) {
    case SE_COS: launch_d<false, true>(a, deriv, s); break;
    case MATERN52_COS: launch_d<true, true>(a, deriv, s); break;
    case SE: launch_d<false, false>(a, deriv, s); break;
    default: launch_d<true, false>(a, deriv, s); break;
  }
  return hipGetLastError();
}

}  // namespace gpk
