// kron3.hip — elementwise / reduction / tail kernels of the 3-axis Kronecker step (gfx950).
//
// the d > 2 generalisation of GP_solver_2d_single's log joint
// (code/model_GP_solver_2d.py:87-183; the 2-axis special case of the log-det weights :157-162)
// for K = K1 (x) K2 (x) K3 on a tensor grid.  The dense work (assembly, SPD inverses, the
// mode-k products as GEMMs over unfoldings) reuses the 2-axis kernels (gpk_kron3.cpp); this file
// holds what is 3-axis specific:
//   k3_prep      step constants: exp of the three axes' kernel params, tau, v, Adam count and
//                bias corrections, ||u_b - b||^2 over the six faces of U
//   k3_permute   mode-2 unfolding: T[i1][i2][i3] <-> Tp[i2][i1][i3] (padded grids)
//   k3_combine   R = U_xx + U_zz + permute(U_yy) - F [+ U(U^2-1)], S = permute(Sp), the permuted
//                copy Rp of R, and per-block partials of ||R||^2 and <U, S>
//   k3_finalize  loss, small-parameter gradients and Adam (one workgroup)
//   k3_adam_u    dL/dU = S + v (X1 + X2 + X3) [+ v(3U^2-1)R] + w tau scatter(u_b - b), Adam on U
// Operator handles (gpk_create3_op, K3Eq): the mode products arrive weighted (c_k folded into the
// GEMM descriptors), so R is still Rx + Rz + Ryp - F; the reaction term is r1 U + r2 U^2 + r3 U^3
// with the factor r1 + 2 r2 U + 3 r3 U^2 in dL/dU, and the boundary sums, the scatter and Nb run
// over the faces whose mask bit is set.  Legacy handles (ac, six faces) keep their expressions on
// uniform branches, bit for bit.
// Coefficient fields (gpk_create3_opv): k3_combine_v multiplies each axis's term by its field,
// adds rho to r1 and writes the reverse pass's operands W_k = a_k R; k3_adam_u_v carries rho in the
// reaction factor.  They are kernels of their own: the two above run unchanged on every other handle.
// Convective terms (gpk_create3_opc): k3_combine_c is k3_combine_v plus u N, N = sum_k g_k D1_k x_k
// A_k, and writes N and Q = u R for the reverse pass; k3_adam_u_c carries N in the reaction factor.
// Kernels of their own again.
// Mixed partials (gpk_create3_opm): k3_combine_m is k3_combine_c plus the cross terms C_13 + C_12 +
// C_23 (formed by GEMMs, gpk_kron3.cpp build_cross_stages); the back-permute of Zb_12 is k3_permute
// on the grid with axes 1 and 2 swapped.  A kernel of its own once more.
// Drift fields (gpk_create3_opb): k3_combine_b is k3_combine_m plus b_1 Z_1 + b_3 Z_3 + b_2 Z_2, Z_k =
// D1_k x_k A_k, and writes the reverse pass's operands E_k = b_k R.  A kernel of its own as well.
// Mixed fourth-order partials (gpk_create3_opq): k3_combine_q is k3_combine_b plus B_13 + B_12 + B_23
// (formed by GEMMs, the bi-pair run of build_pair_stages).  A kernel of its own, launched only on a
// handle with a bi-pair.
// Quadratic gradient terms (gpk_create3_opg): k3_combine_g is k3_combine_q plus Gamma = sum_k s_k P_k^2 +
// sum_{j<k} x_jk P_j P_k, P_k = D1_k x_k A_k; it forms N from the P_k itself and writes the reverse
// pass's operands Q_k per axis.  A kernel of its own, launched only on a handle with such a weight.
// Grids are padded per axis to P_k (multiple of 32); pads of every tensor are zero.
#include "gpk_internal.h"
#include "gpk_kron3.h"
#include "prep_dev.h"
#include "stepk_dev.h"

namespace gpk {

__device__ __forceinline__ double k3_block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int t = threadIdx.x;
  __syncthreads();
  if ((t & 63) == 0) sh[t >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// the six faces' entry index of boundary value k (oracle boundary_3d order); returns its face
__device__ __forceinline__ int k3_face(const K3Geom& g, int k, int& i1, int& i2, int& i3) {
  const int n1 = g.n[0], n2 = g.n[1], n3 = g.n[2];
  const int f0 = n2 * n3, f2 = n1 * n3, f4 = n1 * n2;
  if (k < 2 * f0) {
    i1 = k < f0 ? 0 : n1 - 1;
    const int r = k % f0;
    i2 = r / n3; i3 = r % n3;
    return k < f0 ? 0 : 1;
  } else if (k < 2 * f0 + 2 * f2) {
    const int kk = k - 2 * f0;
    i2 = kk < f2 ? 0 : n2 - 1;
    const int r = kk % f2;
    i1 = r / n3; i3 = r % n3;
    return kk < f2 ? 2 : 3;
  } else {
    const int kk = k - 2 * f0 - 2 * f2;
    i3 = kk < f4 ? 0 : n3 - 1;
    const int r = kk % f4;
    i1 = r / n2; i2 = r % n2;
    return kk < f4 ? 4 : 5;
  }
}

__global__ __launch_bounds__(256) void k3_prep_kernel(K3Prep P) {
  const int t = threadIdx.x;
  for (int ax = 0; ax < 3; ++ax)
    for (int c = t; c < P.q; c += 256) {
      const int off = P.off_kp[ax];
      P.kc[ax].om[c] = TWO_PI * P.params[off + c];
      P.kc[ax].oml[c] = om_low(P.params[off + c], P.kc[ax].om[c]);
      P.kc[ax].a[c] = exp(P.params[off + P.q + c]);
      P.kc[ax].w[c] = exp(P.params[off + 2 * P.q + c]);
    }
  if (t == 0) {
    P.sc->tau = exp(P.params[P.off_tau]);
    P.sc->v = exp(P.params[P.off_v]);
    const int n = *P.count + 1;
    if (P.apply) *P.count = n;
    P.sc->bc1 = 1.0 - pow(P.b1, (double)n);
    P.sc->bc2 = 1.0 - pow(P.b2, (double)n);
  }
  double acc = 0.0;
  for (int k = t; k < P.nb; k += 256) {
    int i1, i2, i3;
    const int f = k3_face(P.g, k, i1, i2, i3);
    if (!((P.faces >> f) & 1)) continue;  // an open face: its bvals entries are never read
    const double d = P.Up[P.g.at(i1, i2, i3)] - P.bvals[k];
    acc += d * d;
  }
  __shared__ double sh[4];
  acc = k3_block_sum(acc, sh);
  if (t == 0) *P.bgap = acc;
}

// dst[i2][i1][i3] = src[i1][i2][i3] over the padded grid (rows of P3 stay contiguous)
__global__ __launch_bounds__(256) void k3_permute_kernel(const double* __restrict__ src,
                                                         double* __restrict__ dst, K3Geom g) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long tot = (long)g.p[0] * g.p[1] * g.p[2];
  if (e >= tot) return;
  const int i3 = (int)(e % g.p[2]);
  const long r = e / g.p[2];
  const int i2 = (int)(r % g.p[1]), i1 = (int)(r / g.p[1]);
  dst[g.atp(i1, i2, i3)] = src[e];
}

__global__ __launch_bounds__(256) void k3_combine_kernel(K3Combine C) {
  const K3Geom& g = C.g;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long tot = (long)g.p[0] * g.p[1] * g.p[2];
  double r2 = 0.0, us = 0.0;
  if (e < tot) {
    const int i3 = (int)(e % g.p[2]);
    const long rr = e / g.p[2];
    const int i2 = (int)(rr % g.p[1]), i1 = (int)(rr / g.p[1]);
    const size_t ep = g.atp(i1, i2, i3);
    const bool real = i1 < g.n[0] && i2 < g.n[1] && i3 < g.n[2];
    double R = 0.0, S = 0.0;
    if (real) {
      R = C.Rx[e] + C.Rz[e] + C.Ryp[ep] - C.F[e];
      const double u = C.Up[e];
      if (C.eq.ac) R += u * (u * u - 1.0);
      else if (C.eq.on) R += u * (C.eq.r1 + u * (C.eq.r2 + u * C.eq.r3));
      S = C.Sp[ep];
      r2 = R * R;
      us = u * S;
    }
    C.R[e] = R;
    C.Rp[ep] = R;
    C.S[e] = S;
  }
  __shared__ double sh[4];
  r2 = k3_block_sum(r2, sh);
  us = k3_block_sum(us, sh);
  if (threadIdx.x == 0) {
    C.red_egap[blockIdx.x] = r2;
    C.red_quad[blockIdx.x] = us;
  }
}

// k3_combine with coefficient fields (gpk_create3_opv): R = a1 Rx + a3 Rz + a2 Ryp - F +
// u ((r1 + rho) + u (r2 + u r3)), summed in k3_combine's order with each term multiplied by its
// field where one is present, so that fields of exact ones (and rho of exact zeros) reproduce
// k3_combine's bits: 1.0 x and r1 + 0.0 are exact, fused or not.  Keep it so.  W_k = a_k R goes to
// the reverse pass; an axis without a field has no W_k, and Rp is written only when axis 2 has
// none.  A field is read at real entries only; the pads of every output are zero.
__global__ __launch_bounds__(256) void k3_combine_v_kernel(K3CombineV V) {
  const K3Combine& C = V.c;
  const K3Geom& g = C.g;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long tot = (long)g.p[0] * g.p[1] * g.p[2];
  double r2 = 0.0, us = 0.0;
  if (e < tot) {
    const int i3 = (int)(e % g.p[2]);
    const long rr = e / g.p[2];
    const int i2 = (int)(rr % g.p[1]), i1 = (int)(rr / g.p[1]);
    const size_t ep = g.atp(i1, i2, i3);
    const bool real = i1 < g.n[0] && i2 < g.n[1] && i3 < g.n[2];
    double R = 0.0, S = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (real) {
      double tx = C.Rx[e], tz = C.Rz[e], ty = C.Ryp[ep];
      if (V.a[0]) { a1 = V.a[0][e]; tx *= a1; }
      if (V.a[2]) { a3 = V.a[2][e]; tz *= a3; }
      if (V.a[1]) { a2 = V.a[1][e]; ty *= a2; }
      R = tx + tz + ty - C.F[e];
      const double u = C.Up[e];
      if (V.rho) R += u * ((C.eq.r1 + V.rho[e]) + u * (C.eq.r2 + u * C.eq.r3));
      else if (C.eq.on) R += u * (C.eq.r1 + u * (C.eq.r2 + u * C.eq.r3));
      S = C.Sp[ep];
      r2 = R * R;
      us = u * S;
    }
    C.R[e] = R;
    C.S[e] = S;
    if (V.W[0]) V.W[0][e] = a1 * R;
    if (V.W[1]) V.W[1][ep] = a2 * R;
    else C.Rp[ep] = R;
    if (V.W[2]) V.W[2][e] = a3 * R;
  }
  __shared__ double sh[4];
  r2 = k3_block_sum(r2, sh);
  us = k3_block_sum(us, sh);
  if (threadIdx.x == 0) {
    C.red_egap[blockIdx.x] = r2;
    C.red_quad[blockIdx.x] = us;
  }
}

// k3_combine_v with convective terms (gpk_create3_opc): R is summed in k3_combine_v's order, then
// u N is added, N = V_1 + V_3 + V_2p in that fixed order, each term only where its axis is
// convective (V_2p read at the permuted index).  Besides k3_combine_v's outputs it writes N (natural
// layout, for the U update) and Q = u R, the reverse pass's operand of the convective axes: natural
// (Q) and / or permuted (Qp), whichever is asked for.  Fields and V_k are read at real entries only;
// the pads of every output are zero.
__global__ __launch_bounds__(256) void k3_combine_c_kernel(K3CombineC X) {
  const K3CombineV& V = X.v;
  const K3Combine& C = V.c;
  const K3Geom& g = C.g;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long tot = (long)g.p[0] * g.p[1] * g.p[2];
  double r2 = 0.0, us = 0.0;
  if (e < tot) {
    const int i3 = (int)(e % g.p[2]);
    const long rr = e / g.p[2];
    const int i2 = (int)(rr % g.p[1]), i1 = (int)(rr / g.p[1]);
    const size_t ep = g.atp(i1, i2, i3);
    const bool real = i1 < g.n[0] && i2 < g.n[1] && i3 < g.n[2];
    double R = 0.0, S = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, N = 0.0, u = 0.0;
    if (real) {
      double tx = C.Rx[e], tz = C.Rz[e], ty = C.Ryp[ep];
      if (V.a[0]) { a1 = V.a[0][e]; tx *= a1; }
      if (V.a[2]) { a3 = V.a[2][e]; tz *= a3; }
      if (V.a[1]) { a2 = V.a[1][e]; ty *= a2; }
      R = tx + tz + ty - C.F[e];
      u = C.Up[e];
      if (V.rho) R += u * ((C.eq.r1 + V.rho[e]) + u * (C.eq.r2 + u * C.eq.r3));
      else if (C.eq.on) R += u * (C.eq.r1 + u * (C.eq.r2 + u * C.eq.r3));
      if (X.V[0]) N += X.V[0][e];
      if (X.V[2]) N += X.V[2][e];
      if (X.V[1]) N += X.V[1][ep];
      R += u * N;
      S = C.Sp[ep];
      r2 = R * R;
      us = u * S;
    }
    C.R[e] = R;
    C.S[e] = S;
    if (V.W[0]) V.W[0][e] = a1 * R;
    if (V.W[1]) V.W[1][ep] = a2 * R;
    else C.Rp[ep] = R;
    if (V.W[2]) V.W[2][e] = a3 * R;
    X.N[e] = N;
    if (X.Q) X.Q[e] = u * R;
    if (X.Qp) X.Qp[ep] = u * R;
  }
  __shared__ double sh[4];
  r2 = k3_block_sum(r2, sh);
  us = k3_block_sum(us, sh);
  if (threadIdx.x == 0) {
    C.red_egap[blockIdx.x] = r2;
    C.red_quad[blockIdx.x] = us;
  }
}

// k3_combine_c with mixed partials (gpk_create3_opm): R is summed in k3_combine_c's order, then
// + C_13 + C_12 + C_23 in that fixed order, each only where its pair is present (C_12 and C_23 read
// at the permuted index).  N, Q and Qp are written where asked for (a handle without a convective
// axis asks for none); Rp is written when axis 2 has no field or a permuted pair reads it (rp).
// Fields, V_k and C_jk are read at real entries only; the pads of every output are zero.
__global__ __launch_bounds__(256) void k3_combine_m_kernel(K3CombineM Mx) {
  const K3CombineC& X = Mx.c;
  const K3CombineV& V = X.v;
  const K3Combine& C = V.c;
  const K3Geom& g = C.g;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long tot = (long)g.p[0] * g.p[1] * g.p[2];
  double r2 = 0.0, us = 0.0;
  if (e < tot) {
    const int i3 = (int)(e % g.p[2]);
    const long rr = e / g.p[2];
    const int i2 = (int)(rr % g.p[1]), i1 = (int)(rr / g.p[1]);
    const size_t ep = g.atp(i1, i2, i3);
    const bool real = i1 < g.n[0] && i2 < g.n[1] && i3 < g.n[2];
    double R = 0.0, S = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, N = 0.0, u = 0.0;
    if (real) {
      double tx = C.Rx[e], tz = C.Rz[e], ty = C.Ryp[ep];
      if (V.a[0]) { a1 = V.a[0][e]; tx *= a1; }
      if (V.a[2]) { a3 = V.a[2][e]; tz *= a3; }
      if (V.a[1]) { a2 = V.a[1][e]; ty *= a2; }
      R = tx + tz + ty - C.F[e];
      u = C.Up[e];
      if (V.rho) R += u * ((C.eq.r1 + V.rho[e]) + u * (C.eq.r2 + u * C.eq.r3));
      else if (C.eq.on) R += u * (C.eq.r1 + u * (C.eq.r2 + u * C.eq.r3));
      if (X.V[0]) N += X.V[0][e];
      if (X.V[2]) N += X.V[2][e];
      if (X.V[1]) N += X.V[1][ep];
      R += u * N;
      if (Mx.C[1]) R += Mx.C[1][e];
      if (Mx.C[0]) R += Mx.C[0][ep];
      if (Mx.C[2]) R += Mx.C[2][ep];
      S = C.Sp[ep];
      r2 = R * R;
      us = u * S;
    }
    C.R[e] = R;
    C.S[e] = S;
    if (V.W[0]) V.W[0][e] = a1 * R;
    if (V.W[1]) V.W[1][ep] = a2 * R;
    if (!V.W[1] || Mx.rp) C.Rp[ep] = R;
    if (V.W[2]) V.W[2][e] = a3 * R;
    if (X.N) X.N[e] = N;
    if (X.Q) X.Q[e] = u * R;
    if (X.Qp) X.Qp[ep] = u * R;
  }
  __shared__ double sh[4];
  r2 = k3_block_sum(r2, sh);
  us = k3_block_sum(us, sh);
  if (threadIdx.x == 0) {
    C.red_egap[blockIdx.x] = r2;
    C.red_quad[blockIdx.x] = us;
  }
}

// k3_combine_m with drift fields (gpk_create3_opb): R is summed in k3_combine_m's order, then
// + b_1 Z_1 + b_3 Z_3 + b_2 Z_2 in that fixed order, each only where its axis has a field (b_k read at
// the natural index, Z_2 at the permuted one).  Besides k3_combine_m's outputs, on the final R, it
// writes E_k = b_k R (E_2 permuted).  Fields, V_k, C_jk and Z_k are read at real entries only; the
// pads of every output are zero.
__global__ __launch_bounds__(256) void k3_combine_b_kernel(K3CombineB B) {
  const K3CombineM& Mx = B.m;
  const K3CombineC& X = Mx.c;
  const K3CombineV& V = X.v;
  const K3Combine& C = V.c;
  const K3Geom& g = C.g;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long tot = (long)g.p[0] * g.p[1] * g.p[2];
  double r2 = 0.0, us = 0.0;
  if (e < tot) {
    const int i3 = (int)(e % g.p[2]);
    const long rr = e / g.p[2];
    const int i2 = (int)(rr % g.p[1]), i1 = (int)(rr / g.p[1]);
    const size_t ep = g.atp(i1, i2, i3);
    const bool real = i1 < g.n[0] && i2 < g.n[1] && i3 < g.n[2];
    double R = 0.0, S = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, N = 0.0, u = 0.0;
    double b1 = 0.0, b2 = 0.0, b3 = 0.0;
    if (real) {
      double tx = C.Rx[e], tz = C.Rz[e], ty = C.Ryp[ep];
      if (V.a[0]) { a1 = V.a[0][e]; tx *= a1; }
      if (V.a[2]) { a3 = V.a[2][e]; tz *= a3; }
      if (V.a[1]) { a2 = V.a[1][e]; ty *= a2; }
      R = tx + tz + ty - C.F[e];
      u = C.Up[e];
      if (V.rho) R += u * ((C.eq.r1 + V.rho[e]) + u * (C.eq.r2 + u * C.eq.r3));
      else if (C.eq.on) R += u * (C.eq.r1 + u * (C.eq.r2 + u * C.eq.r3));
      if (X.V[0]) N += X.V[0][e];
      if (X.V[2]) N += X.V[2][e];
      if (X.V[1]) N += X.V[1][ep];
      R += u * N;
      if (Mx.C[1]) R += Mx.C[1][e];
      if (Mx.C[0]) R += Mx.C[0][ep];
      if (Mx.C[2]) R += Mx.C[2][ep];
      if (B.b[0]) { b1 = B.b[0][e]; R += b1 * B.Z[0][e]; }
      if (B.b[2]) { b3 = B.b[2][e]; R += b3 * B.Z[2][e]; }
      if (B.b[1]) { b2 = B.b[1][e]; R += b2 * B.Z[1][ep]; }
      S = C.Sp[ep];
      r2 = R * R;
      us = u * S;
    }
    C.R[e] = R;
    C.S[e] = S;
    if (V.W[0]) V.W[0][e] = a1 * R;
    if (V.W[1]) V.W[1][ep] = a2 * R;
    if (!V.W[1] || Mx.rp) C.Rp[ep] = R;
    if (V.W[2]) V.W[2][e] = a3 * R;
    if (X.N) X.N[e] = N;
    if (X.Q) X.Q[e] = u * R;
    if (X.Qp) X.Qp[ep] = u * R;
    if (B.E[0]) B.E[0][e] = b1 * R;
    if (B.E[1]) B.E[1][ep] = b2 * R;
    if (B.E[2]) B.E[2][e] = b3 * R;
  }
  __shared__ double sh[4];
  r2 = k3_block_sum(r2, sh);
  us = k3_block_sum(us, sh);
  if (threadIdx.x == 0) {
    C.red_egap[blockIdx.x] = r2;
    C.red_quad[blockIdx.x] = us;
  }
}

// k3_combine_b with mixed fourth-order partials (gpk_create3_opq): R is summed in k3_combine_b's
// order, then + B_13 + B_12 + B_23 in that fixed order, each only where its pair is present (B_12 and
// B_23 read at the permuted index).  Every output of k3_combine_b is written from the final R; Rp is
// written when axis 2 has no field or a permuted pair, cross or bi, reads it (m.rp).  Every pointer
// of b may be null (a handle without drift fields).  Inputs are read at real entries only; the pads
// of every output are zero.
__global__ __launch_bounds__(256) void k3_combine_q_kernel(K3CombineQ Qx) {
  const K3CombineB& B = Qx.b;
  const K3CombineM& Mx = B.m;
  const K3CombineC& X = Mx.c;
  const K3CombineV& V = X.v;
  const K3Combine& C = V.c;
  const K3Geom& g = C.g;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long tot = (long)g.p[0] * g.p[1] * g.p[2];
  double r2 = 0.0, us = 0.0;
  if (e < tot) {
    const int i3 = (int)(e % g.p[2]);
    const long rr = e / g.p[2];
    const int i2 = (int)(rr % g.p[1]), i1 = (int)(rr / g.p[1]);
    const size_t ep = g.atp(i1, i2, i3);
    const bool real = i1 < g.n[0] && i2 < g.n[1] && i3 < g.n[2];
    double R = 0.0, S = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, N = 0.0, u = 0.0;
    double b1 = 0.0, b2 = 0.0, b3 = 0.0;
    if (real) {
      double tx = C.Rx[e], tz = C.Rz[e], ty = C.Ryp[ep];
      if (V.a[0]) { a1 = V.a[0][e]; tx *= a1; }
      if (V.a[2]) { a3 = V.a[2][e]; tz *= a3; }
      if (V.a[1]) { a2 = V.a[1][e]; ty *= a2; }
      R = tx + tz + ty - C.F[e];
      u = C.Up[e];
      if (V.rho) R += u * ((C.eq.r1 + V.rho[e]) + u * (C.eq.r2 + u * C.eq.r3));
      else if (C.eq.on) R += u * (C.eq.r1 + u * (C.eq.r2 + u * C.eq.r3));
      if (X.V[0]) N += X.V[0][e];
      if (X.V[2]) N += X.V[2][e];
      if (X.V[1]) N += X.V[1][ep];
      R += u * N;
      if (Mx.C[1]) R += Mx.C[1][e];
      if (Mx.C[0]) R += Mx.C[0][ep];
      if (Mx.C[2]) R += Mx.C[2][ep];
      if (B.b[0]) { b1 = B.b[0][e]; R += b1 * B.Z[0][e]; }
      if (B.b[2]) { b3 = B.b[2][e]; R += b3 * B.Z[2][e]; }
      if (B.b[1]) { b2 = B.b[1][e]; R += b2 * B.Z[1][ep]; }
      if (Qx.B[1]) R += Qx.B[1][e];
      if (Qx.B[0]) R += Qx.B[0][ep];
      if (Qx.B[2]) R += Qx.B[2][ep];
      S = C.Sp[ep];
      r2 = R * R;
      us = u * S;
    }
    C.R[e] = R;
    C.S[e] = S;
    if (V.W[0]) V.W[0][e] = a1 * R;
    if (V.W[1]) V.W[1][ep] = a2 * R;
    if (!V.W[1] || Mx.rp) C.Rp[ep] = R;
    if (V.W[2]) V.W[2][e] = a3 * R;
    if (X.N) X.N[e] = N;
    if (X.Q) X.Q[e] = u * R;
    if (X.Qp) X.Qp[ep] = u * R;
    if (B.E[0]) B.E[0][e] = b1 * R;
    if (B.E[1]) B.E[1][ep] = b2 * R;
    if (B.E[2]) B.E[2][e] = b3 * R;
  }
  __shared__ double sh[4];
  r2 = k3_block_sum(r2, sh);
  us = k3_block_sum(us, sh);
  if (threadIdx.x == 0) {
    C.red_egap[blockIdx.x] = r2;
    C.red_quad[blockIdx.x] = us;
  }
}

// k3_combine_q with quadratic gradient terms (gpk_create3_opg): R is summed in k3_combine_q's order,
// with N = g_1 P_1 + g_3 P_3 + g_2 P_2 computed here from P_k = D1_k x_k A_k (P_2 read at the permuted
// index; the V pointers are null on this handle), then + Gamma = s_1 P_1^2 + s_3 P_3^2 + s_2 P_2^2 +
// x_13 P_1 P_3 + x_12 P_1 P_2 + x_23 P_2 P_3 in that fixed order, each term only where its weight is
// non-zero.  Every output of k3_combine_q is written from the final R, N in the natural layout, and per
// gradient-active axis Q_k = (g_k u + 2 s_k P_k + sum_j x_jk P_j) R (Q_2 permuted).  Inputs are read
// at real entries only; the pads of every output are zero.
__global__ __launch_bounds__(256) void k3_combine_g_kernel(K3CombineG Gx) {
  const K3CombineQ& Qx = Gx.q;
  const K3CombineB& B = Qx.b;
  const K3CombineM& Mx = B.m;
  const K3CombineC& X = Mx.c;
  const K3CombineV& V = X.v;
  const K3Combine& C = V.c;
  const K3Geom& g = C.g;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long tot = (long)g.p[0] * g.p[1] * g.p[2];
  double r2 = 0.0, us = 0.0;
  if (e < tot) {
    const int i3 = (int)(e % g.p[2]);
    const long rr = e / g.p[2];
    const int i2 = (int)(rr % g.p[1]), i1 = (int)(rr / g.p[1]);
    const size_t ep = g.atp(i1, i2, i3);
    const bool real = i1 < g.n[0] && i2 < g.n[1] && i3 < g.n[2];
    double R = 0.0, S = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, N = 0.0, u = 0.0;
    double b1 = 0.0, b2 = 0.0, b3 = 0.0;
    double q1 = 0.0, q2 = 0.0, q3 = 0.0;  // dR/dP_k
    if (real) {
      double tx = C.Rx[e], tz = C.Rz[e], ty = C.Ryp[ep];
      if (V.a[0]) { a1 = V.a[0][e]; tx *= a1; }
      if (V.a[2]) { a3 = V.a[2][e]; tz *= a3; }
      if (V.a[1]) { a2 = V.a[1][e]; ty *= a2; }
      R = tx + tz + ty - C.F[e];
      u = C.Up[e];
      if (V.rho) R += u * ((C.eq.r1 + V.rho[e]) + u * (C.eq.r2 + u * C.eq.r3));
      else if (C.eq.on) R += u * (C.eq.r1 + u * (C.eq.r2 + u * C.eq.r3));
      const double p1 = Gx.P[0] ? Gx.P[0][e] : 0.0;
      const double p3 = Gx.P[2] ? Gx.P[2][e] : 0.0;
      const double p2 = Gx.P[1] ? Gx.P[1][ep] : 0.0;
      if (Gx.g[0] != 0.0) N += Gx.g[0] * p1;
      if (Gx.g[2] != 0.0) N += Gx.g[2] * p3;
      if (Gx.g[1] != 0.0) N += Gx.g[1] * p2;
      R += u * N;
      if (Mx.C[1]) R += Mx.C[1][e];
      if (Mx.C[0]) R += Mx.C[0][ep];
      if (Mx.C[2]) R += Mx.C[2][ep];
      if (B.b[0]) { b1 = B.b[0][e]; R += b1 * B.Z[0][e]; }
      if (B.b[2]) { b3 = B.b[2][e]; R += b3 * B.Z[2][e]; }
      if (B.b[1]) { b2 = B.b[1][e]; R += b2 * B.Z[1][ep]; }
      if (Qx.B[1]) R += Qx.B[1][e];
      if (Qx.B[0]) R += Qx.B[0][ep];
      if (Qx.B[2]) R += Qx.B[2][ep];
      double G = 0.0;
      if (Gx.s[0] != 0.0) G += Gx.s[0] * (p1 * p1);
      if (Gx.s[2] != 0.0) G += Gx.s[2] * (p3 * p3);
      if (Gx.s[1] != 0.0) G += Gx.s[1] * (p2 * p2);
      if (Gx.x[1] != 0.0) G += Gx.x[1] * (p1 * p3);
      if (Gx.x[0] != 0.0) G += Gx.x[0] * (p1 * p2);
      if (Gx.x[2] != 0.0) G += Gx.x[2] * (p2 * p3);
      R += G;
      q1 = Gx.g[0] * u + 2.0 * Gx.s[0] * p1 + (Gx.x[0] * p2 + Gx.x[1] * p3);
      q2 = Gx.g[1] * u + 2.0 * Gx.s[1] * p2 + (Gx.x[0] * p1 + Gx.x[2] * p3);
      q3 = Gx.g[2] * u + 2.0 * Gx.s[2] * p3 + (Gx.x[1] * p1 + Gx.x[2] * p2);
      S = C.Sp[ep];
      r2 = R * R;
      us = u * S;
    }
    C.R[e] = R;
    C.S[e] = S;
    if (V.W[0]) V.W[0][e] = a1 * R;
    if (V.W[1]) V.W[1][ep] = a2 * R;
    if (!V.W[1] || Mx.rp) C.Rp[ep] = R;
    if (V.W[2]) V.W[2][e] = a3 * R;
    X.N[e] = N;
    if (B.E[0]) B.E[0][e] = b1 * R;
    if (B.E[1]) B.E[1][ep] = b2 * R;
    if (B.E[2]) B.E[2][e] = b3 * R;
    if (Gx.Qk[0]) Gx.Qk[0][e] = q1 * R;
    if (Gx.Qk[1]) Gx.Qk[1][ep] = q2 * R;
    if (Gx.Qk[2]) Gx.Qk[2][e] = q3 * R;
  }
  __shared__ double sh[4];
  r2 = k3_block_sum(r2, sh);
  us = k3_block_sum(us, sh);
  if (threadIdx.x == 0) {
    C.red_egap[blockIdx.x] = r2;
    C.red_quad[blockIdx.x] = us;
  }
}

// one workgroup: loss (model_GP_solver_2d.py:145-174 with three log-det weights), the small
// parameters' gradients and their Adam update (optax.adam, :179-182)
__global__ __launch_bounds__(256) void k3_finalize_kernel(K3Final F) {
  const int t = threadIdx.x;
  __shared__ double sh[4], sg[2];
  double quad = 0.0, egap = 0.0;
  for (int i = t; i < F.nred; i += 256) {
    quad += F.red_quad[i];
    egap += F.red_egap[i];
  }
  quad = k3_block_sum(quad, sh);
  egap = k3_block_sum(egap, sh);
  double ld[3];
  for (int a = 0; a < 3; ++a) {
    double x = 0.0;
    for (int k = t; k < F.nldet[a]; k += 256) x += F.ldet[a][k];
    ld[a] = k3_block_sum(x, sh);
  }
  const double tau = F.sc->tau, v = F.sc->v, bc1 = F.sc->bc1, bc2 = F.sc->bc2;
  const double wb = F.llk_weight, c = F.logdet;
  const double n1 = F.g.n[0], n2 = F.g.n[1], n3 = F.g.n[2];
  const double Nc = n1 * n2 * n3;
  double Nb = 2.0 * (n2 * n3 + n1 * n3 + n1 * n2);
  if (F.faces != K3_ALL_FACES) {  // the active faces' entries
    const int fm = F.faces;
    Nb = ((fm & 1) + ((fm >> 1) & 1)) * (n2 * n3) + (((fm >> 2) & 1) + ((fm >> 3) & 1)) * (n1 * n3) +
         (((fm >> 4) & 1) + ((fm >> 5) & 1)) * (n1 * n2);
  }
  Nb += F.nb_extra;  // the derivative faces' entries (gpk_create3_opn; + 0.0 elsewhere: exact)
  const double log_tau = F.params[F.off_tau], log_v = F.params[F.off_v];
  if (t == 0) {
    const double bgap = *F.bgap;
    const double log_prior = -0.5 * c * (n2 * n3 * ld[0] + n1 * n3 * ld[1] + n1 * n2 * ld[2]) - 0.5 * quad;
    const double log_b = 0.5 * Nb * log_tau - 0.5 * tau * bgap;
    const double eq_ll = 0.5 * Nc * log_v - 0.5 * v * egap;
    const double loss = -(log_prior + log_b * wb + eq_ll);
    sg[0] = wb * (-0.5 * Nb + 0.5 * tau * bgap);
    sg[1] = -0.5 * Nc + 0.5 * v * egap;
    const int slot = *F.loss_slot;
    F.losses[slot] = loss;
    *F.loss_slot = slot + 1;
    F.diag[0] = loss; F.diag[1] = ld[0]; F.diag[2] = ld[1]; F.diag[3] = ld[2];
    F.diag[4] = quad; F.diag[5] = egap; F.diag[6] = bgap;
  }
  __syncthreads();
  for (int k = t; k < F.nsmall; k += 256) {
    const int idx = F.off_small + k;
    double g;
    if (idx == F.off_tau) {
      g = sg[0];
    } else if (idx == F.off_v) {
      g = sg[1];
    } else {
      const int a = idx >= F.off_kp[2] ? 2 : idx >= F.off_kp[1] ? 1 : 0;
      const int rr = idx - F.off_kp[a], ty = rr / F.q, cq = rr % F.q;  // freq, log-ls, log-w
      g = (ty == 0 && !F.has_cos) ? 0.0 : F.pg[a * 3 * QMAX + ty * QMAX + cq] * F.kc[a].w[cq];
    }
    F.grad[idx] = g;
    if (F.apply) {
      double p = F.params[idx], m = F.m[idx], vv = F.v[idx];
      adam1(g, p, m, vv, F.hyper, bc1, bc2);
      F.params[idx] = p; F.m[idx] = m; F.v[idx] = vv;
    }
  }
}

__global__ __launch_bounds__(256) void k3_adam_u_kernel(K3AdamU A) {
  const K3Geom& g = A.g;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long nu = (long)g.n[0] * g.n[1] * g.n[2];
  if (e >= nu) return;
  const int i3 = (int)(e % g.n[2]);
  const long rr = e / g.n[2];
  const int i2 = (int)(rr % g.n[1]), i1 = (int)(rr / g.n[1]);
  const size_t pi = g.at(i1, i2, i3), pp = g.atp(i1, i2, i3);
  const double tau = A.sc->tau, v = A.sc->v, wt = A.llk_weight * tau;
  const double u = A.Up[pi];
  double gr = A.S[pi] + v * (A.X1[pi] + A.X2p[pp] + A.X3[pi]);
  if (A.eq.ac) gr += v * (3.0 * u * u - 1.0) * A.R[pi];
  else if (A.eq.on) gr += v * (A.eq.r1 + u * (2.0 * A.eq.r2 + 3.0 * A.eq.r3 * u)) * A.R[pi];
  const int n1 = g.n[0], n2 = g.n[1], n3 = g.n[2];
  const int f0 = n2 * n3, f2 = n1 * n3, f4 = n1 * n2;
  const int b2 = 2 * f0, b4 = 2 * f0 + 2 * f2;
  if (A.eq.faces == K3_ALL_FACES) {
    if (i1 == 0) gr += wt * (u - A.bvals[i2 * n3 + i3]);
    if (i1 == n1 - 1) gr += wt * (u - A.bvals[f0 + i2 * n3 + i3]);
    if (i2 == 0) gr += wt * (u - A.bvals[b2 + i1 * n3 + i3]);
    if (i2 == n2 - 1) gr += wt * (u - A.bvals[b2 + f2 + i1 * n3 + i3]);
    if (i3 == 0) gr += wt * (u - A.bvals[b4 + i1 * n2 + i2]);
    if (i3 == n3 - 1) gr += wt * (u - A.bvals[b4 + f4 + i1 * n2 + i2]);
  } else {  // each face under its bit (an edge of two active faces counts twice, as above)
    const int fm = A.eq.faces;
    if ((fm & 1) && i1 == 0) gr += wt * (u - A.bvals[i2 * n3 + i3]);
    if ((fm & 2) && i1 == n1 - 1) gr += wt * (u - A.bvals[f0 + i2 * n3 + i3]);
    if ((fm & 4) && i2 == 0) gr += wt * (u - A.bvals[b2 + i1 * n3 + i3]);
    if ((fm & 8) && i2 == n2 - 1) gr += wt * (u - A.bvals[b2 + f2 + i1 * n3 + i3]);
    if ((fm & 16) && i3 == 0) gr += wt * (u - A.bvals[b4 + i1 * n2 + i2]);
    if ((fm & 32) && i3 == n3 - 1) gr += wt * (u - A.bvals[b4 + f4 + i1 * n2 + i2]);
  }
  const long idx = A.off_u + e;
  A.grad[idx] = gr;
  if (A.apply) {
    double p = A.params[idx], m = A.m[idx], vv = A.v[idx];
    adam1(gr, p, m, vv, A.hyper, A.sc->bc1, A.sc->bc2);
    A.params[idx] = p; A.m[idx] = m; A.v[idx] = vv;
    A.Up[pi] = p;
  }
}

// k3_adam_u of an operator handle whose linear reaction coefficient is r1 + rho(x): the factor on
// R is (r1 + rho) + u (2 r2 + 3 r3 u) (at rho = 0.0 the bits of k3_adam_u's), rho read at the
// padded natural index.  The faces go under their bits; at faces = 63 these are k3_adam_u's adds.
__global__ __launch_bounds__(256) void k3_adam_u_v_kernel(K3AdamUV V) {
  const K3AdamU& A = V.a;
  const K3Geom& g = A.g;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long nu = (long)g.n[0] * g.n[1] * g.n[2];
  if (e >= nu) return;
  const int i3 = (int)(e % g.n[2]);
  const long rr = e / g.n[2];
  const int i2 = (int)(rr % g.n[1]), i1 = (int)(rr / g.n[1]);
  const size_t pi = g.at(i1, i2, i3), pp = g.atp(i1, i2, i3);
  const double tau = A.sc->tau, v = A.sc->v, wt = A.llk_weight * tau;
  const double u = A.Up[pi];
  double gr = A.S[pi] + v * (A.X1[pi] + A.X2p[pp] + A.X3[pi]);
  gr += v * ((A.eq.r1 + V.rho[pi]) + u * (2.0 * A.eq.r2 + 3.0 * A.eq.r3 * u)) * A.R[pi];
  const int n1 = g.n[0], n2 = g.n[1], n3 = g.n[2];
  const int f0 = n2 * n3, f2 = n1 * n3, f4 = n1 * n2;
  const int b2 = 2 * f0, b4 = 2 * f0 + 2 * f2;
  const int fm = A.eq.faces;
  if ((fm & 1) && i1 == 0) gr += wt * (u - A.bvals[i2 * n3 + i3]);
  if ((fm & 2) && i1 == n1 - 1) gr += wt * (u - A.bvals[f0 + i2 * n3 + i3]);
  if ((fm & 4) && i2 == 0) gr += wt * (u - A.bvals[b2 + i1 * n3 + i3]);
  if ((fm & 8) && i2 == n2 - 1) gr += wt * (u - A.bvals[b2 + f2 + i1 * n3 + i3]);
  if ((fm & 16) && i3 == 0) gr += wt * (u - A.bvals[b4 + i1 * n2 + i2]);
  if ((fm & 32) && i3 == n3 - 1) gr += wt * (u - A.bvals[b4 + f4 + i1 * n2 + i2]);
  const long idx = A.off_u + e;
  A.grad[idx] = gr;
  if (A.apply) {
    double p = A.params[idx], m = A.m[idx], vv = A.v[idx];
    adam1(gr, p, m, vv, A.hyper, A.sc->bc1, A.sc->bc2);
    A.params[idx] = p; A.m[idx] = m; A.v[idx] = vv;
    A.Up[pi] = p;
  }
}

// k3_adam_u_v of a convective handle (gpk_create3_opc): d(u N)/du at fixed N joins the factor on R,
// (r1 + rho + N) + u (2 r2 + 3 r3 u); rho may be absent.  (The other half of the product rule, the
// dependence of N on U, arrives through X_k: T_k carries g_k D1_k^T x_k (u R).)
__global__ __launch_bounds__(256) void k3_adam_u_c_kernel(K3AdamUC V) {
  const K3AdamU& A = V.a;
  const K3Geom& g = A.g;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long nu = (long)g.n[0] * g.n[1] * g.n[2];
  if (e >= nu) return;
  const int i3 = (int)(e % g.n[2]);
  const long rr = e / g.n[2];
  const int i2 = (int)(rr % g.n[1]), i1 = (int)(rr / g.n[1]);
  const size_t pi = g.at(i1, i2, i3), pp = g.atp(i1, i2, i3);
  const double tau = A.sc->tau, v = A.sc->v, wt = A.llk_weight * tau;
  const double u = A.Up[pi];
  double gr = A.S[pi] + v * (A.X1[pi] + A.X2p[pp] + A.X3[pi]);
  const double lin = (V.rho ? A.eq.r1 + V.rho[pi] : A.eq.r1) + V.N[pi];
  gr += v * (lin + u * (2.0 * A.eq.r2 + 3.0 * A.eq.r3 * u)) * A.R[pi];
  const int n1 = g.n[0], n2 = g.n[1], n3 = g.n[2];
  const int f0 = n2 * n3, f2 = n1 * n3, f4 = n1 * n2;
  const int b2 = 2 * f0, b4 = 2 * f0 + 2 * f2;
  const int fm = A.eq.faces;
  if ((fm & 1) && i1 == 0) gr += wt * (u - A.bvals[i2 * n3 + i3]);
  if ((fm & 2) && i1 == n1 - 1) gr += wt * (u - A.bvals[f0 + i2 * n3 + i3]);
  if ((fm & 4) && i2 == 0) gr += wt * (u - A.bvals[b2 + i1 * n3 + i3]);
  if ((fm & 8) && i2 == n2 - 1) gr += wt * (u - A.bvals[b2 + f2 + i1 * n3 + i3]);
  if ((fm & 16) && i3 == 0) gr += wt * (u - A.bvals[b4 + i1 * n2 + i2]);
  if ((fm & 32) && i3 == n3 - 1) gr += wt * (u - A.bvals[b4 + f4 + i1 * n2 + i2]);
  const long idx = A.off_u + e;
  A.grad[idx] = gr;
  if (A.apply) {
    double p = A.params[idx], m = A.m[idx], vv = A.v[idx];
    adam1(gr, p, m, vv, A.hyper, A.sc->bc1, A.sc->bc2);
    A.params[idx] = p; A.m[idx] = m; A.v[idx] = vv;
    A.Up[pi] = p;
  }
}

// flat params (U unpadded) -> padded working copy
__global__ __launch_bounds__(256) void k3_sync_u_kernel(const double* __restrict__ params, long off_u,
                                                        K3Geom g, double* __restrict__ Up) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long nu = (long)g.n[0] * g.n[1] * g.n[2];
  if (e >= nu) return;
  const int i3 = (int)(e % g.n[2]);
  const long rr = e / g.n[2];
  const int i2 = (int)(rr % g.n[1]), i1 = (int)(rr / g.n[1]);
  Up[g.at(i1, i2, i3)] = params[off_u + e];
}

static unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

hipError_t k3_launch_prep(const K3Prep& P, hipStream_t s) {
  hipLaunchKernelGGL(k3_prep_kernel, dim3(1), dim3(256), 0, s, P);
  return hipGetLastError();
}
hipError_t k3_launch_permute(const double* src, double* dst, const K3Geom& g, hipStream_t s) {
  hipLaunchKernelGGL(k3_permute_kernel, dim3(blocks_of(g.padded())), dim3(256), 0, s, src, dst, g);
  return hipGetLastError();
}
int k3_combine_blocks(const K3Geom& g) { return (int)blocks_of(g.padded()); }
hipError_t k3_launch_combine(const K3Combine& C, hipStream_t s) {
  hipLaunchKernelGGL(k3_combine_kernel, dim3(blocks_of(C.g.padded())), dim3(256), 0, s, C);
  return hipGetLastError();
}
hipError_t k3_launch_combine_v(const K3CombineV& V, hipStream_t s) {
  hipLaunchKernelGGL(k3_combine_v_kernel, dim3(blocks_of(V.c.g.padded())), dim3(256), 0, s, V);
  return hipGetLastError();
}
hipError_t k3_launch_finalize(const K3Final& F, hipStream_t s) {
  hipLaunchKernelGGL(k3_finalize_kernel, dim3(1), dim3(256), 0, s, F);
  return hipGetLastError();
}
hipError_t k3_launch_adam_u(const K3AdamU& A, hipStream_t s) {
  hipLaunchKernelGGL(k3_adam_u_kernel, dim3(blocks_of(A.g.real())), dim3(256), 0, s, A);
  return hipGetLastError();
}
hipError_t k3_launch_adam_u_v(const K3AdamUV& V, hipStream_t s) {
  hipLaunchKernelGGL(k3_adam_u_v_kernel, dim3(blocks_of(V.a.g.real())), dim3(256), 0, s, V);
  return hipGetLastError();
}
hipError_t k3_launch_combine_c(const K3CombineC& C, hipStream_t s) {
  hipLaunchKernelGGL(k3_combine_c_kernel, dim3(blocks_of(C.v.c.g.padded())), dim3(256), 0, s, C);
  return hipGetLastError();
}
hipError_t k3_launch_adam_u_c(const K3AdamUC& C, hipStream_t s) {
  hipLaunchKernelGGL(k3_adam_u_c_kernel, dim3(blocks_of(C.a.g.real())), dim3(256), 0, s, C);
  return hipGetLastError();
}
hipError_t k3_launch_combine_m(const K3CombineM& M, hipStream_t s) {
  hipLaunchKernelGGL(k3_combine_m_kernel, dim3(blocks_of(M.c.v.c.g.padded())), dim3(256), 0, s, M);
  return hipGetLastError();
}
hipError_t k3_launch_combine_b(const K3CombineB& B, hipStream_t s) {
  hipLaunchKernelGGL(k3_combine_b_kernel, dim3(blocks_of(B.m.c.v.c.g.padded())), dim3(256), 0, s, B);
  return hipGetLastError();
}
hipError_t k3_launch_combine_q(const K3CombineQ& Q, hipStream_t s) {
  hipLaunchKernelGGL(k3_combine_q_kernel, dim3(blocks_of(Q.b.m.c.v.c.g.padded())), dim3(256), 0, s, Q);
  return hipGetLastError();
}
hipError_t k3_launch_combine_g(const K3CombineG& G, hipStream_t s) {
  hipLaunchKernelGGL(k3_combine_g_kernel, dim3(blocks_of(G.q.b.m.c.v.c.g.padded())), dim3(256), 0, s, G);
  return hipGetLastError();
}
hipError_t k3_launch_unpermute(const double* src, double* dst, const K3Geom& g, hipStream_t s) {
  K3Geom w = g;  // axes 1 and 2 swapped: src is [w.p0][w.p1][p3] and w.atp the natural index of g
  w.n[0] = g.n[1]; w.n[1] = g.n[0]; w.p[0] = g.p[1]; w.p[1] = g.p[0];
  return k3_launch_permute(src, dst, w, s);
}
hipError_t k3_launch_sync_u(const double* params, long off_u, const K3Geom& g, double* Up, hipStream_t s) {
  hipLaunchKernelGGL(k3_sync_u_kernel, dim3(blocks_of(g.real())), dim3(256), 0, s, params, off_u, g, Up);
  return hipGetLastError();
}

}  // namespace gpk
