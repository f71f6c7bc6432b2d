// kron3_face.hip — derivative boundary data of the 3-axis Kronecker step (gpk_create3_opn, gfx950).
//
// Face f = 2k + s of axis k (index i_f = 0 or n_k - 1) may carry data h_f on du/dx_k.  With
// d_f[j] = d_1 kappa_k(x_{i_f}, x_j) (row i_f of the order-1 block D1_k, whatever orders the
// operator puts on the axis) and A_k = K_k^{-1} x_k U, which the step already has,
//     g_f = d_f ._k A_k,   r_f = g_f - h_f,   dgap = sum_f ||r_f||^2
// joins the boundary gap, and the reverse pass adds, with wt = llk_weight tau,
//     T_k[j, .] += (wt / v) d_f[j] r_f          (T_k = c_k D_k^T x_k W_k, before X_k = K_k^{-1} x_k T_k)
//     dL/d d_f[j] = wt sum_face r_f A_k[j, .]   -> one more block of axis k's parameter partials.
// Kernels:
//   k3_face_row    d_f for the faces that carry data, zero-padded to P_k, in the assembly's own
//                  arithmetic (four component groups, summed (0 + 1) + (2 + 3), signed by x_{i_f} - x_j)
//   k3_face_gap    g_f, r_f (planes of the handle, zero pads) and per-block partials of ||r_f||^2
//   k3_face_back   the update of T_k and per-block partials of sum_face r_f A_k[j, .]
//   k3_face_colsum the reverse pass's partials summed over its workgroups (more than one of them)
//   k3_face_tail   dgap (added to *bgap) and the contraction of dL/d d_f with d d_f / d(freq, log-ls,
//                  log-w), written as blocks bpa .. bpa + K3_FACE_TAIL_BLOCKS - 1 of the axis's
//                  parameter partials (pgrad.hip's layout)
// Two layouts: the leading form (axis 1 natural, axis 2 in the mode-2 permuted layout: A is
// [P_k][M], the face the contiguous plane of M entries) and the trailing form (axis 3: A is [M][P_3],
// g a row dot product, the row gradient a column sum).  Both faces of an axis ride the same passes.
// Every sum runs in a fixed order (no atomics): repeated calls give equal bits.
#include "gpk_internal.h"
#include "gpk_kron3.h"
#include "prep_dev.h"

namespace gpk {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double face_block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int t = threadIdx.x;
  __syncthreads();
  if ((t & 63) == 0) sh[t >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// the residual of plane entry m: g - h at a real entry of a face that carries data, else zero
__device__ __forceinline__ double face_resid(const K3FaceAxis& F, int s, int m, double g) {
  const int ia = m / F.pb, ib = m % F.pb;
  if (!F.on[s] || ia >= F.na || ib >= F.nb) return 0.0;
  return g - F.h[s][(size_t)ia * F.nb + ib];
}

}  // namespace

template <bool MATERN, bool COS>
__global__ __launch_bounds__(256) void k3_face_row_kernel(K3FaceRows R) {
  const int f = blockIdx.y, a = f >> 1, s = f & 1;
  const int n = R.n[a], p = R.p[a];
  // (uniform: the grid is sized by the longest axis; an axis without data has no rows)
  if ((int)blockIdx.x * 64 >= p || !R.row[a]) return;
  const int t = threadIdx.x, e = t & 63, g = t >> 6;
  __shared__ double sw[QMAX], sa[QMAX], so[QMAX], sol[QMAX], pd[4][64];
  if (t < R.q) {
    sw[t] = R.kc[a].w[t];
    sa[t] = R.kc[a].a[t];
    so[t] = R.kc[a].om[t];
    sol[t] = R.kc[a].oml[t];
  }
  __syncthreads();
  const int j = blockIdx.x * 64 + e;
  const bool real = j < n && ((R.dfaces >> f) & 1);
  double diff = 0.0, kv = 0.0, dv = 0.0;
  if (real) {
    diff = R.x[a][s ? n - 1 : 0] - R.x[a][j];
    eval_kd_part<MATERN, COS, 1>(diff, sw, sa, so, sol, g, 4, R.q, kv, dv);
  }
  pd[g][e] = dv;
  __syncthreads();
  if (g != 0 || j >= p) return;
  dv = (pd[0][e] + pd[1][e]) + (pd[2][e] + pd[3][e]);
  const double sgn = diff >= 0.0 ? 1.0 : -1.0;  // JAX abs'(0) = +1, as the assembly
  R.row[a][(size_t)s * p + j] = real ? sgn * dv : 0.0;
}

// leading form: two adjacent plane entries per thread (16-byte loads), j in order
__global__ __launch_bounds__(256) void k3_face_gap_lead_kernel(K3FaceAxis F) {
  const size_t M = (size_t)F.pa * F.pb;
  const int m = (blockIdx.x * 256 + threadIdx.x) * 2;  // (M is a multiple of 1024: no tail)
  const double* r0 = F.row;
  const double* r1 = F.row + F.pk;
  d2 g0 = {0.0, 0.0}, g1 = {0.0, 0.0};
  const double* ap = F.A + m;
#pragma unroll 4
  for (int j = 0; j < F.nk; ++j) {
    const d2 a = *reinterpret_cast<const d2*>(ap + (size_t)j * M);
    g0 += r0[j] * a;
    g1 += r1[j] * a;
  }
  const d2 q0 = {face_resid(F, 0, m, g0.x), face_resid(F, 0, m + 1, g0.y)};
  const d2 q1 = {face_resid(F, 1, m, g1.x), face_resid(F, 1, m + 1, g1.y)};
  *reinterpret_cast<d2*>(F.r + m) = q0;
  *reinterpret_cast<d2*>(F.r + M + m) = q1;
  __shared__ double sh[4];
  const double acc = face_block_sum((q0.x * q0.x + q0.y * q0.y) + (q1.x * q1.x + q1.y * q1.y), sh);
  if (threadIdx.x == 0) F.part[blockIdx.x] = acc;
}

// trailing form: one plane entry (a row of A) per 32-lane half-wave
__global__ __launch_bounds__(256) void k3_face_gap_trail_kernel(K3FaceAxis F) {
  const size_t M = (size_t)F.pa * F.pb;
  const int t = threadIdx.x, l = t & 31;
  const int m = blockIdx.x * 8 + (t >> 5);  // (M is a multiple of 8)
  const double* ap = F.A + (size_t)m * F.pk;
  double g0 = 0.0, g1 = 0.0;
  for (int j = l; j < F.pk; j += 32) {  // (pads of the rows and of A are zero)
    const double a = ap[j];
    g0 += F.row[j] * a;
    g1 += F.row[F.pk + j] * a;
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    g0 += __shfl_xor(g0, o, 64);
    g1 += __shfl_xor(g1, o, 64);
  }
  double acc = 0.0;
  if (l == 0) {
    const double q0 = face_resid(F, 0, m, g0), q1 = face_resid(F, 1, m, g1);
    F.r[m] = q0;
    F.r[M + m] = q1;
    acc = q0 * q0 + q1 * q1;
  }
  __shared__ double sh[4];
  acc = face_block_sum(acc, sh);
  if (t == 0) F.part[blockIdx.x] = acc;
}

// leading form: workgroup (j, chunk) covers K3_FACE_CHUNK plane entries of row j of A_k and T_k
__global__ __launch_bounds__(256) void k3_face_back_lead_kernel(K3FaceAxis F, const StepScalars* sc,
                                                                double llk_weight) {
  const size_t M = (size_t)F.pa * F.pb;
  const int j = blockIdx.x, chunk = blockIdx.y;
  const double cf = llk_weight * sc->tau / sc->v;
  const double d0 = cf * F.row[j], d1 = cf * F.row[F.pk + j];
  const size_t m0 = (size_t)chunk * K3_FACE_CHUNK, m1 = m0 + K3_FACE_CHUNK < M ? m0 + K3_FACE_CHUNK : M;
  const double* ap = F.A + (size_t)j * M;
  double* tp = F.T + (size_t)j * M;
  double a0 = 0.0, a1 = 0.0;
  for (size_t m = m0 + 2 * threadIdx.x; m < m1; m += 512) {
    const d2 a = *reinterpret_cast<const d2*>(ap + m);
    const d2 q0 = *reinterpret_cast<const d2*>(F.r + m);
    const d2 q1 = *reinterpret_cast<const d2*>(F.r + M + m);
    a0 += q0.x * a.x + q0.y * a.y;
    a1 += q1.x * a.x + q1.y * a.y;
    d2 tv = *reinterpret_cast<d2*>(tp + m);
    tv += d0 * q0 + d1 * q1;
    *reinterpret_cast<d2*>(tp + m) = tv;
  }
  __shared__ double sh[4];
  a0 = face_block_sum(a0, sh);
  a1 = face_block_sum(a1, sh);
  if (threadIdx.x == 0) {
    F.gv[((size_t)chunk * 2 + 0) * F.pk + j] = a0;
    F.gv[((size_t)chunk * 2 + 1) * F.pk + j] = a1;
  }
}

// trailing form: a workgroup covers K3_FACE_ROWS rows of A_3 and T_3, 32 columns at a time (lanes
// along j, eight row groups), and writes its column sums as one block of partials
__global__ __launch_bounds__(256) void k3_face_back_trail_kernel(K3FaceAxis F, const StepScalars* sc,
                                                                 double llk_weight) {
  const size_t M = (size_t)F.pa * F.pb;
  const int t = threadIdx.x, jl = t & 31, rg = t >> 5;
  const size_t m0 = (size_t)blockIdx.x * K3_FACE_ROWS;  // (M is a multiple of K3_FACE_ROWS)
  const double cf = llk_weight * sc->tau / sc->v;
  __shared__ double sh[8][2][32];
  for (int j0 = 0; j0 < F.pk; j0 += 32) {
    const int j = j0 + jl;
    const double d0 = cf * F.row[j], d1 = cf * F.row[F.pk + j];
    double a0 = 0.0, a1 = 0.0;
#pragma unroll 4
    for (int rr = rg; rr < K3_FACE_ROWS; rr += 8) {
      const size_t m = m0 + rr;
      const double a = F.A[m * F.pk + j], q0 = F.r[m], q1 = F.r[M + m];
      a0 += q0 * a;
      a1 += q1 * a;
      F.T[m * F.pk + j] += d0 * q0 + d1 * q1;
    }
    sh[rg][0][jl] = a0;
    sh[rg][1][jl] = a1;
    __syncthreads();
    if (t < 64) {
      const int s = t >> 5;
      double x = 0.0;
#pragma unroll
      for (int g = 0; g < 8; ++g) x += sh[g][s][jl];
      F.gv[((size_t)blockIdx.x * 2 + s) * F.pk + j] = x;
    }
    __syncthreads();
  }
}

// gs[s][j] = sum over the nblk workgroups of k3_face_back of gv[b][s][j]: 32 columns of one face per
// workgroup, eight groups of b, the groups added in order
__global__ __launch_bounds__(256) void k3_face_colsum_kernel(const double* __restrict__ gv, int nblk, int pk,
                                                             double* __restrict__ gs) {
  const int t = threadIdx.x, jl = t & 31, bg = t >> 5, s = blockIdx.y;
  const int j = blockIdx.x * 32 + jl;
  double x = 0.0;
#pragma unroll 8
  for (int b = bg; b < nblk; b += 8) x += gv[((size_t)b * 2 + s) * pk + j];
  __shared__ double sh[8][32];
  sh[bg][jl] = x;
  __syncthreads();
  if (t < 32) {
    x = 0.0;
#pragma unroll
    for (int g = 0; g < 8; ++g) x += sh[g][jl];
    gs[(size_t)s * pk + j] = x;
  }
}

// Workgroup (k, y): block bpa + y of axis k's parameter partials (zeros on an axis without data),
// from the (face, j) pairs e = y, y + K3_FACE_TAIL_BLOCKS, ...; workgroup (0, 0) also sums the gap
// partials of the three axes, publishes the two gaps and adds dgap to *bgap.
template <bool MATERN, bool COS>
__global__ __launch_bounds__(256) void k3_face_tail_kernel(K3FaceTail T) {
  const int t = threadIdx.x, k = blockIdx.x, y = blockIdx.y;
  __shared__ double sh[4];
  if (k == 0 && y == 0) {
    double acc = 0.0;
    for (int a = 0; a < 3; ++a)
      for (int i = t; i < T.npart[a]; i += 256) acc += T.ax[a].part[i];
    acc = face_block_sum(acc, sh);
    if (t == 0) {
      const double vg = *T.bgap;
      T.bt[0] = vg;
      T.bt[1] = acc;
      *T.bgap = vg + acc;
    }
  }
  const K3FaceAxis& F = T.ax[k];
  double* out = T.out[k] + (size_t)y * 3 * QMAX;
  if (!F.on[0] && !F.on[1]) {
    for (int i = t; i < 3 * QMAX; i += 256) out[i] = 0.0;
    return;
  }
  // per (face, j): the weight wt s_fj sum_face r_f A_k[j, .] of d d_f[j] / d theta, and |x_if - x_j|
  __shared__ double wv[2][K3_FACE_MAX_N], dist[2][K3_FACE_MAX_N];
  __shared__ double sacc[256][3];
  const double wt = T.llk_weight * T.sc->tau;
  const int n = F.nk;
  for (int e = t; e < 2 * n; e += 256) {
    const int s = e / n, j = e % n;
    const double x = F.gs[(size_t)s * F.pk + j];
    const double diff = T.x[k][s ? n - 1 : 0] - T.x[k][j];
    dist[s][j] = fabs(diff);
    wv[s][j] = F.on[s] ? (diff >= 0.0 ? wt : -wt) * x : 0.0;
  }
  __syncthreads();
  int qp = 1;
  while (qp < T.q) qp <<= 1;
  const int c = t % qp, g = t / qp, G = 256 / qp;
  double accf = 0.0, accl = 0.0, accw = 0.0;
  if (c < T.q) {
    const double a = T.kc[k].a[c], om = T.kc[k].om[c], oml = T.kc[k].oml[c];
    for (int e = y + K3_FACE_TAIL_BLOCKS * g; e < 2 * n; e += K3_FACE_TAIL_BLOCKS * G) {
      const int s = e / n, j = e % n;
      const double wd = wv[s][j];
      if (wd == 0.0) continue;
      const double d = dist[s][j];
      double m0, m1, m2, m0l, m1l, m2l;
      radial_l<MATERN>(d, a, m0, m1, m2, m0l, m1l, m2l);
      if (COS) {  // the order-1 field's partials, as pgrad.hip forms them
        double S, C;
        phase_sincos(om, oml, d, S, C);
        const double c0 = C, c1 = -om * S;
        const double c0f = -TWO_PI * d * S;
        const double c1f = -TWO_PI * S - TWO_PI * om * d * C;
        accw += wd * (m1 * c0 + m0 * c1);
        accl += wd * (m1l * c0 + m0l * c1);
        accf += wd * (m1 * c0f + m0 * c1f);
      } else {
        accw += wd * m1;
        accl += wd * m1l;
      }
    }
  }
  sacc[t][0] = accf;
  sacc[t][1] = accl;
  sacc[t][2] = accw;
  __syncthreads();
  for (int i = t; i < 3 * QMAX; i += 256) {
    const int which = i / QMAX, cc = i % QMAX;
    double x = 0.0;
    if (cc < T.q)
      for (int gg = 0; gg < G; ++gg) x += sacc[gg * qp + cc][which];
    out[i] = x;
  }
}

hipError_t k3_launch_face_row(int kind, const K3FaceRows& R, hipStream_t s) {
  const int pmax = R.p[0] > R.p[1] ? (R.p[0] > R.p[2] ? R.p[0] : R.p[2]) : (R.p[1] > R.p[2] ? R.p[1] : R.p[2]);
  const dim3 grid((pmax + 63) / 64, 6);
  switch (kind) {
    case SE_COS: hipLaunchKernelGGL((k3_face_row_kernel<false, true>), grid, dim3(256), 0, s, R); break;
    case MATERN52_COS: hipLaunchKernelGGL((k3_face_row_kernel<true, true>), grid, dim3(256), 0, s, R); break;
    case SE: hipLaunchKernelGGL((k3_face_row_kernel<false, false>), grid, dim3(256), 0, s, R); break;
    default: hipLaunchKernelGGL((k3_face_row_kernel<true, false>), grid, dim3(256), 0, s, R); break;
  }
  return hipGetLastError();
}

int k3_face_gap_blocks(const K3FaceAxis& F, bool trailing) {
  const long M = (long)F.pa * F.pb;
  return (int)(trailing ? M / 8 : M / 512);
}

int k3_face_back_blocks(const K3FaceAxis& F, bool trailing) {
  const long M = (long)F.pa * F.pb;
  return (int)(trailing ? M / K3_FACE_ROWS : (M + K3_FACE_CHUNK - 1) / K3_FACE_CHUNK);
}

hipError_t k3_launch_face_gap(const K3FaceAxis& F, bool trailing, hipStream_t s) {
  const dim3 grid(k3_face_gap_blocks(F, trailing));
  if (trailing) hipLaunchKernelGGL(k3_face_gap_trail_kernel, grid, dim3(256), 0, s, F);
  else hipLaunchKernelGGL(k3_face_gap_lead_kernel, grid, dim3(256), 0, s, F);
  return hipGetLastError();
}

hipError_t k3_launch_face_back(const K3FaceAxis& F, bool trailing, const StepScalars* sc, double llk_weight,
                               hipStream_t s) {
  if (trailing)
    hipLaunchKernelGGL(k3_face_back_trail_kernel, dim3(k3_face_back_blocks(F, true)), dim3(256), 0, s, F, sc,
                       llk_weight);
  else
    hipLaunchKernelGGL(k3_face_back_lead_kernel, dim3(F.nk, k3_face_back_blocks(F, false)), dim3(256), 0, s, F,
                       sc, llk_weight);
  return hipGetLastError();
}

hipError_t k3_launch_face_colsum(const K3FaceAxis& F, int nblk, hipStream_t s) {
  hipLaunchKernelGGL(k3_face_colsum_kernel, dim3(F.pk / 32, 2), dim3(256), 0, s, F.gv, nblk, F.pk, F.gs);
  return hipGetLastError();
}

hipError_t k3_launch_face_tail(int kind, const K3FaceTail& T, hipStream_t s) {
  const dim3 grid(3, K3_FACE_TAIL_BLOCKS);
  switch (kind) {
    case SE_COS: hipLaunchKernelGGL((k3_face_tail_kernel<false, true>), grid, dim3(256), 0, s, T); break;
    case MATERN52_COS: hipLaunchKernelGGL((k3_face_tail_kernel<true, true>), grid, dim3(256), 0, s, T); break;
    case SE: hipLaunchKernelGGL((k3_face_tail_kernel<false, false>), grid, dim3(256), 0, s, T); break;
    default: hipLaunchKernelGGL((k3_face_tail_kernel<true, false>), grid, dim3(256), 0, s, T); break;
  }
  return hipGetLastError();
}

}  // namespace gpk
