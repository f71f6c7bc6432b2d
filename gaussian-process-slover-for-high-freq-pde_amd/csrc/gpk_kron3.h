// gpk_kron3.h — argument blocks of the 3-axis Kronecker step's own kernels (kron3.hip).
#pragma once
#include "gpk_internal.h"
#include "stepk.h"

namespace gpk {

// Tensor grid: true sizes n[k], padded sizes p[k] (multiples of 32).  A grid tensor is stored
// row-major [p1][p2][p3]; its mode-2 permutation (the mode-2 unfolding, contiguous) [p2][p1][p3].
struct K3Geom {
  int n[3], p[3];
  __host__ __device__ size_t at(int i1, int i2, int i3) const {
    return ((size_t)i1 * p[1] + i2) * p[2] + i3;
  }
  __host__ __device__ size_t atp(int i1, int i2, int i3) const {
    return ((size_t)i2 * p[0] + i1) * p[2] + i3;
  }
  __host__ __device__ long padded() const { return (long)p[0] * p[1] * p[2]; }
  __host__ __device__ long real() const { return (long)n[0] * n[1] * n[2]; }
};

// Boundary faces in gpk_problem3.bvals order (bit f of a face mask): 0: i1 = 0, 1: i1 = n1 - 1,
// 2: i2 = 0, 3: i2 = n2 - 1, 4: i3 = 0, 5: i3 = n3 - 1.  K3_ALL_FACES is the legacy six-face set.
constexpr int K3_ALL_FACES = 63;

// The equation layer of an operator handle (gpk_operator3; the per-axis orders and weights live
// in the assembly launches and the GEMM descriptors): the reaction polynomial r1 u + r2 u^2 +
// r3 u^3 (on = 0 skips it) and the active faces.  ac = 1 is the legacy Allen-Cahn term u(u^2 - 1)
// in its own expression (legacy handles stay bit-identical); it excludes on.
struct K3Eq {
  int ac, on, faces;
  double r1, r2, r3;
};

struct K3Prep {
  K3Geom g;
  const double* params;
  int off_kp[3], off_tau, off_v, q;
  AxisConst* kc;        // out [3]
  StepScalars* sc;      // out
  int* count;
  int apply;
  double b1, b2;
  const double* Up; const double* bvals; int nb;  // nb: all six faces (the bvals layout)
  int faces;            // entries of a face whose bit is clear are never read
  double* bgap;         // out [1]
};

struct K3Combine {
  K3Geom g;
  const double *Rx, *Rz, *Ryp, *F, *Up, *Sp;  // U_xx, U_zz (natural), U_yy, S (permuted)
  K3Eq eq;
  double *R, *Rp, *S;                         // out: R (natural and permuted), S (natural)
  double *red_egap, *red_quad;                // out: per-block partials
};

// k3_combine_v (gpk_create3_opv): k3_combine with a coefficient field per axis and on the linear
// reaction term.  Fields are natural-layout padded tensors; a null one is absent (a_k = 1, rho = 0).
// W[k] = a_k R is the reverse pass's operand of axis k (W[1] in the mode-2 permuted layout); an
// absent field has no W[k] (null): its operand is R itself, or c.Rp, which is written only then.
struct K3CombineV {
  K3Combine c;
  const double* a[3];
  const double* rho;
  double* W[3];
};

struct K3Final {
  K3Geom g;
  AdamHyper hyper;
  double llk_weight, logdet;
  int apply, has_cos, q;
  int faces;                 // Nb = the entries of the active faces
  const double* red_quad; const double* red_egap; int nred;
  const double* ldet[3]; int nldet[3];
  const double* pg;          // [3][3*QMAX]
  const AxisConst* kc;
  const StepScalars* sc;
  const double* bgap;
  int off_kp[3], off_tau, off_v, off_small, nsmall;
  double *params, *grad, *m, *v;
  double* losses; int* loss_slot;
  double* diag;              // [8]: loss, logdet1..3, quad, egap, bgap
  double nb_extra;           // added to Nb: the entries of the derivative faces (0.0: no such data)
};

struct K3AdamU {
  K3Geom g;
  AdamHyper hyper;
  double llk_weight;
  int apply;
  K3Eq eq;
  const StepScalars* sc;
  const double *S, *X1, *X2p, *X3, *R;  // X2 in the permuted layout
  double* Up;
  const double* bvals;
  long off_u;
  double *params, *grad, *m, *v;
};

// k3_adam_u_v: k3_adam_u of an operator handle with rho (natural padded layout) added to r1
struct K3AdamUV {
  K3AdamU a;
  const double* rho;
};

// k3_combine_c (gpk_create3_opc): k3_combine_v plus the convective term u N, N = V_1 + V_3 + V_2p
// with V_k = g_k D1_k x_k A_k (null: axis k is not convective; V[1] in the mode-2 permuted layout).
// Every pointer of v may be null here (a handle without fields).  N goes to the U update in the
// natural layout; Q = u R is the reverse pass's operand of the convective axes, natural (Q: axis 1
// or 3 convective) and / or permuted (Qp: axis 2), each null when no axis reads it.
struct K3CombineC {
  K3CombineV v;
  const double* V[3];
  double *N, *Q, *Qp;
};

// k3_combine_m (gpk_create3_opm): k3_combine_c plus the mixed partials C_13 + C_12 + C_23, C_jk =
// m_jk D1_k x_k K_k^{-1} x_k D1_j x_j A_j (null: the pair is absent; C[0] = C_12 and C[2] = C_23 in
// the mode-2 permuted layout, C[1] = C_13 natural).  Every pointer of c.v and c.V, and c.N, c.Q and
// c.Qp, may be null here (a handle without fields or convective axes).  rp = 1 writes v.c.Rp even
// when axis 2 has a field: the pairs (1,2) and (2,3) read R itself in the permuted layout.
struct K3CombineM {
  K3CombineC c;
  const double* C[3];
  int rp;
};

// k3_combine_b (gpk_create3_opb): k3_combine_m plus the drift terms b_1 Z_1 + b_3 Z_3 + b_2 Z_2, Z_k =
// D1_k x_k A_k (b[k] null: axis k has no drift field, and Z[k], E[k] are then null as well).  b[k] is a
// natural-layout padded tensor; Z[1] and E[1] are in the mode-2 permuted layout.  E[k] = b_k R is
// the reverse pass's operand of the drift term.  Every pointer of m may be null as on k3_combine_m.
struct K3CombineB {
  K3CombineM m;
  const double* b[3];
  const double* Z[3];
  double* E[3];
};

// k3_combine_q (gpk_create3_opq): k3_combine_b plus the mixed fourth-order partials B_13 + B_12 + B_23,
// B_jk = q_jk DD_k x_k K_k^{-1} x_k DD_j x_j A_j (null: the pair is absent; B[0] = B_12 and B[2] = B_23
// in the mode-2 permuted layout, B[1] = B_13 natural).  Every pointer of b may be null (a handle
// without drift fields); b.m.rp also covers a permuted bi-pair, which reads R itself from Rp.
struct K3CombineQ {
  K3CombineB b;
  const double* B[3];
};

// k3_combine_g (gpk_create3_opg): k3_combine_q plus the quadratic gradient terms Gamma = s_1 P_1^2 +
// s_3 P_3^2 + s_2 P_2^2 + x_13 P_1 P_3 + x_12 P_1 P_2 + x_23 P_2 P_3, P_k = D1_k x_k A_k (null: axis k is
// not gradient-active; P[1] and Qk[1] in the mode-2 permuted layout).  x = the pairs (1,2), (1,3),
// (2,3).  N = g_1 P_1 + g_3 P_3 + g_2 P_2 is computed here (q.b.m.c.V is null on this handle; N, Q and
// Qp of q.b.m.c: N is written, Q and Qp are null).  Qk[k] = (g_k U + 2 s_k P_k + sum_j x_jk P_j) R is
// the reverse pass's operand of axis k's order-1 block.  Every pointer of q may be null as there.
struct K3CombineG {
  K3CombineQ q;
  const double* P[3];
  double g[3], s[3], x[3];
  double* Qk[3];
};

// k3_adam_u_c: k3_adam_u_v with N (natural padded layout) added to the factor on R; rho nullable
struct K3AdamUC {
  K3AdamU a;
  const double* rho;
  const double* N;
};

// Derivative boundary data (gpk_create3_opn, kron3_face.hip).  One axis's two faces 2k and 2k + 1:
// A and T are A_k and T_k in the leading form ([pk][pa pb]: axis 1, and axis 2 in the permuted
// layout) or the trailing form ([pa pb][pk]: axis 3); the face is the plane [pa][pb], real na x nb.
constexpr int K3_FACE_MAX_N = 1024;   // = K3_MAX_N (the tail kernel's LDS rows)
constexpr int K3_FACE_CHUNK = 4096;   // plane entries per workgroup of the leading-form reverse pass
constexpr int K3_FACE_ROWS = 64;      // rows of A_3 per workgroup of the trailing-form reverse pass
constexpr int K3_FACE_TAIL_BLOCKS = 8;  // workgroups (= blocks of parameter partials) per axis of k3_face_tail
struct K3FaceAxis {
  int on[2];            // face 2k + s carries data
  int nk, pk, na, nb, pa, pb;
  const double* A;
  double* T;
  const double* row;    // [2][pk]: d_f, zero-padded (zeros for a face without data)
  double* r;            // [2][pa pb]: r_f, zero pads (zeros for a face without data)
  const double* h[2];   // face s's data, [na][nb] (read only where on[s])
  double* part;         // per-block partials of ||r_f||^2 (k3_face_gap_blocks)
  double* gv;           // [k3_face_back_blocks][2][pk]: partials of sum_face r_f A_k[j, .]
  double* gs;           // [2][pk]: their sum (k3_face_colsum; gv itself where there is one block)
};

struct K3FaceRows {
  const double* x[3];
  int n[3], p[3];
  const AxisConst* kc;  // [3], as k3_prep published them
  int q, dfaces;
  double* row[3];       // out: K3FaceAxis::row per axis
};

struct K3FaceTail {
  K3FaceAxis ax[3];
  const double* x[3];
  const AxisConst* kc;
  const StepScalars* sc;
  double llk_weight;
  int q;
  int npart[3];             // gap partials per axis (0 on an axis without data)
  double* out[3];           // blocks bpa .. of each axis's parameter partials, [K3_FACE_TAIL_BLOCKS][3][QMAX]
  double* bgap;             // in: the value gap (k3_prep); out: value gap + derivative gap
  double* bt;               // out [2]: value gap, derivative gap
};

hipError_t k3_launch_face_row(int kind, const K3FaceRows& R, hipStream_t s);
int k3_face_gap_blocks(const K3FaceAxis& F, bool trailing);
int k3_face_back_blocks(const K3FaceAxis& F, bool trailing);
hipError_t k3_launch_face_gap(const K3FaceAxis& F, bool trailing, hipStream_t s);
hipError_t k3_launch_face_back(const K3FaceAxis& F, bool trailing, const StepScalars* sc, double llk_weight,
                               hipStream_t s);
hipError_t k3_launch_face_colsum(const K3FaceAxis& F, int nblk, hipStream_t s);
hipError_t k3_launch_face_tail(int kind, const K3FaceTail& T, hipStream_t s);

hipError_t k3_launch_prep(const K3Prep& P, hipStream_t s);
hipError_t k3_launch_permute(const double* src, double* dst, const K3Geom& g, hipStream_t s);
int k3_combine_blocks(const K3Geom& g);
hipError_t k3_launch_combine(const K3Combine& C, hipStream_t s);
hipError_t k3_launch_combine_v(const K3CombineV& V, hipStream_t s);
hipError_t k3_launch_finalize(const K3Final& F, hipStream_t s);
hipError_t k3_launch_adam_u(const K3AdamU& A, hipStream_t s);
hipError_t k3_launch_adam_u_v(const K3AdamUV& V, hipStream_t s);
hipError_t k3_launch_combine_c(const K3CombineC& C, hipStream_t s);
hipError_t k3_launch_adam_u_c(const K3AdamUC& C, hipStream_t s);
hipError_t k3_launch_combine_m(const K3CombineM& M, hipStream_t s);
hipError_t k3_launch_combine_b(const K3CombineB& B, hipStream_t s);
hipError_t k3_launch_combine_q(const K3CombineQ& Q, hipStream_t s);
hipError_t k3_launch_combine_g(const K3CombineG& G, hipStream_t s);
// dst[i1][i2][i3] = src[i2][i1][i3]: k3_permute's inverse (k3_permute itself on the grid with axes
// 1 and 2 swapped, where its source index is this one's and its target index the natural one)
hipError_t k3_launch_unpermute(const double* src, double* dst, const K3Geom& g, hipStream_t s);
hipError_t k3_launch_sync_u(const double* params, long off_u, const K3Geom& g, double* Up, hipStream_t s);

}  // namespace gpk
