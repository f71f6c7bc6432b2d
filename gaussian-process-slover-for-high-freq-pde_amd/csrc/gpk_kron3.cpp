// gpk_kron3.cpp — C ABI of the 3-axis Kronecker solver (include/gpk.h gpk_*3; SURVEY.md §8(f)
// row 4, the d > 2 generalisation of GP_solver_2d_single, code/model_GP_solver_2d.py:87-183).
//
// One step (one captured hipGraph) on a tensor grid U[i1][i2][i3], K = K1 (x) K2 (x) K3:
//   prep -> K_k, D_k (the 2-axis assembly kernel, per axis) -> K_k^{-1} + log det (the per-sweep
//   SPD inverse) -> mode-k products as fp64 MFMA GEMMs over unfoldings -> R, S, partials ->
//   reverse-mode products -> G_K, G_D per axis -> the 2-axis parameter contraction -> loss +
//   Adam.  Unfoldings: mode 1 is U as P1 x (P2 P3), mode 3 is U as (P1 P2) x P3 -- both plain
//   row-major views -- and mode 2 goes through the permuted copy [i2][i1][i3] (k3_permute),
//   whose rows are the mode-2 unfolding.  With A_k = K_k^{-1} x_k U, X_k = (K_k^{-1} D_k^T) x_k R:
//     S = K^{-1} U,  R = sum_k D_k x_k A_k - F,  dL/dU = S + v sum_k X_k  (+ AC, boundary)
//     G_Kk = c/2 (N / N_k) K_k^{-1} - (S/2 + v X_k)_(k) A_k,(k)^T,   G_Dk = v R_(k) A_k,(k)^T
// (the 2-axis adjoints of SURVEY.md Appendix A, one per axis).
// Operator handles (gpk_create3_op): D_k is the order-o_k derivative block (o_k = 1 or 2, the
// assembly's and the contraction's `deriv`, one order per launch, so axes 1-2 share a launch only
// at equal orders) and its weight c_k is the alpha of every product with D_k -- D_k x_k A_k,
// D_k^T x_k R and G_Dk -- so that X_k, Y_k, G_Kk and dL/dU carry it with no further change:
//     R = sum_k c_k D_k x_k A_k - F + r1 U + r2 U^2 + r3 U^3,
//     dL/dU = S + v sum_k c_k X_k + v (r1 + 2 r2 U + 3 r3 U^2) R + w tau scatter over the active faces.
// gpk_create3 fills in the legacy equivalent (orders 2, weights 1.0, six faces), which multiplies
// by alpha = 1.0 exactly and runs the launches it always ran.
// Mixed-order axes (gpk_create3_opx, both c2_k and c1_k non-zero): the assembled block is
// D_k = c2_k DD_k + c1_k D1_k (assembly and contraction in DERIV_BOTH, the weights in their
// arguments) and the three GEMM weights of that axis are exactly 1.0, so every formula above holds
// with c_k = 1 and this D_k.  Axes 1-2 share a launch when their modes are equal; two mixed axes
// with different weights still do.  An axis with one non-zero weight is the path above, unchanged.
// Coefficient fields (gpk_create3_opv): R = sum_k a_k . (D_k x_k A_k) - F + (r1 + rho) . U + ...
// (k3_combine_v), and the reverse pass reads W_k = a_k . R where it reads R above -- X_k, G_Dk --
// so dL/dU and the G's hold with no further change; rho joins r1 in dL/dU's reaction factor
// (k3_adam_u_v).  An axis without a field has no W_k: its operand stays R (Rp on axis 2).
// Convective terms (gpk_create3_opc, g_k u du/dx_k): a convective axis assembles in DERIV_SPLIT, which
// stores the plain order-1 block D1_k next to D_k; V_k = g_k D1_k x_k A_k, N = sum_k V_k and
// R += U . N (k3_combine_c); the reverse pass reads Q = U . R: T_k += g_k D1_k^T x_k Q (the second
// product of T_k's descriptor), G_D1k = v g_k Q_(k) A_k,(k)^T joins the order-1 weights of the
// contraction, and dL/dU += v N . R (k3_adam_u_c) (build_conv_stages).
// Mixed partials (gpk_create3_opm, m_jk d^2u/dx_j dx_k, j < k): both axes of a pair assemble in
// DERIV_SPLIT; Z_j = D1_j x_j A_j, H_jk = K_k^{-1} x_k Z_j (a solve, refined like every other),
// C_jk = m_jk D1_k x_k H_jk and R += C_13 + C_12 + C_23 (k3_combine_m).  The reverse pass forms
// Hb_jk = m_jk D1_k^T x_k R, Zb_jk = K_k^{-1} x_k Hb_jk (a solve), T_j += D1_j^T x_j Zb_jk before
// X_j, G_D1j += v Zb_jk,(j) A_j,(j)^T, G_D1k += v m_jk R_(k) H_jk,(k)^T and G_Kk -= v Zb_jk,(k)
// H_jk,(k)^T: eight further launches (build_pair_stages).
// High-order terms (gpk_create3_oph, c4_k d^4u/dx_k^4 + c3_k d^3u/dx_k^3): the axis's block is D_k =
// c4_k D4_k + c3_k D3_k + c2_k DD_k + c1_k D1_k, assembled and contracted in DERIV_HIGH (DERIV_HIGH_SPLIT
// where the axis also owns D1_k: convective, cross, drift).  The host treats D_k as opaque: the stage
// list, the refinement and the face kernels are untouched.
// Mixed fourth-order partials (gpk_create3_opq, q_jk d^4u/dx_j^2 dx_k^2, j < k): both axes of a pair
// assemble in DERIV_HIGH_D2 (DERIV_HIGH_SPLIT_D2 where the axis owns D1_k), which stores the plain
// order-2 block DD_k next to D_k.  The pair is the cross pair with DD for D1: Z2_j = DD_j x_j A_j, H2_jk =
// K_k^{-1} x_k Z2_j, B_jk = q_jk DD_k x_k H2_jk, R += B_13 + B_12 + B_23 after every older term
// (k3_combine_q); Hb2_jk = q_jk DD_k^T x_k R, Zb2_jk = K_k^{-1} x_k Hb2_jk, T_j += DD_j^T x_j Zb2_jk,
// G_DDj += v Zb2_jk,(j) A_j,(j)^T, G_DDk += v q_jk R_(k) H2_jk,(k)^T, G_Kk -= v Zb2_jk,(k) H2_jk,(k)^T:
// eight further launches from the same builder (build_pair_stages), each after the cross pairs' own.
// Drift fields (gpk_create3_opb, b_k(x) du/dx_k): a drift axis assembles in DERIV_SPLIT; Z_k = D1_k
// x_k A_k (a cross pair's own Z_1 / Z_2p where it forms them), R += b_1 Z_1 + b_3 Z_3 + b_2 Z_2
// (k3_combine_b), and the reverse pass reads E_k = b_k R: T_k += D1_k^T x_k E_k before X_k and
// G_D1k += v E_k,(k) A_k,(k)^T: two or three further launches (build_drift_stages).  b_k is data: dL/dU
// has no direct term.
// Quadratic gradient terms (gpk_create3_opg, s_k (du/dx_k)^2 + x_jk du/dx_j du/dx_k): axis k is
// gradient-active when g_k, s_k or a pair weight x_jk with k in it is non-zero, and assembles in the
// split mode its other terms imply.  P_k = D1_k x_k A_k per such axis (the V_k launch's position, alpha
// 1); k3_combine_g forms N = sum_k g_k P_k, Gamma and R, and writes Q_k = (g_k U + 2 s_k P_k + sum_j x_jk
// P_j) . R; T_k += D1_k^T x_k Q_k (the dual slot of stage 3), G_D1k = v Q_k,(k) A_k,(k)^T (the convective
// G_D1k launch's position), and dL/dU += v N . R (k3_adam_u_c) (build_gradsq_stages, which stands in
// build_conv_stages' place on such a handle).
// GPK_FLAG3_REFINE: every one of the eight solves (A1, A2, A3, T, S, X1, X2, X3) is followed by
// one refinement step X += K_k^{-1} (B - K_k X) gated on the axis's pst: one fused panel launch
// (refine_panel.hip), or two GEMMs where its panels do not fit LDS (build_refine).
//
// Beyond the step: gpk_predict3 (test-grid predictions, T <- Kmn_k x_k solve(K_k, T) axis after
// axis; its mode-2 products are slab-batched launches, gemm.hip, with no permuted copy),
// gpk_predict_deriv3 (the same with D_x1_kappa / DD_x1_kappa blocks as Kmn_k), gpk_evaluate3 (the
// same quantity at scattered points, chunk by chunk, its axis-2 and axis-3 products contracted
// against fields evaluated on the fly: point_eval.hip), gpk_criterion3 and the Adam state.  (The
// standalone measurements of its pieces, gpk_mode_gemm, gpk_refine_panel and gpk_point_contract,
// are in gpk_diag.cpp.)
#include "gpk_host.h"
#include "gpk_kron3.h"

namespace {
constexpr int K3_LOSS_CAP = 4096;
}  // namespace

// A pair set's eight launches (build_pair_stages) and the refinement of its two solves per pair:
// rst[2 i] / [2 i + 1] the residuals / corrections and rp[i] the fused panels of H_jk (i = 0) and
// Zb_jk (i = 1)
struct PairStages {
  std::vector<std::vector<gpk::GemmDesc>> st, rst;
  std::vector<std::vector<gpk::RefinePanel>> rp;
};

struct gpk_handle3 {
  gpk_problem3 prob{};
  // what the handle solves: gpk_create3_op's operator, or the legacy equation's equivalent
  // (orders 2, weights 1, six faces; legacy_ac keeps Allen-Cahn in its own expression u(u^2 - 1))
  gpk_operator3 op{};
  int legacy_ac = 0;
  // per axis: the assembly's / contraction's mode (op.order[k], or DERIV_BOTH on a mixed axis,
  // where op.order[k] = 0 and op.coef[k] = 1.0, the GEMM weight) and the weights as stated
  int mode[3] = {2, 2, 2};
  double c2[3] = {}, c1[3] = {};
  // gpk_create3_oph: the weights of the order-4 and order-3 fields (zeros: none).  An axis with one
  // of them is entered as a mixed axis and assembles / contracts in DERIV_HIGH, or in DERIV_HIGH_SPLIT
  // where DERIV_SPLIT would stand (its D1_k and G_D1k as there); nothing else knows of them
  double c4[3] = {}, c3[3] = {};
  K3Geom g{};
  int q = 0;
  long nu = 0, nparams = 0;
  int off_kp[3] = {}, off_tau = 0, off_v = 0, nsmall = 0;
  int dev = 0;
  hipStream_t s = nullptr;
  std::vector<void*> allocs;
  double* x[3] = {};
  double *F = nullptr, *bvals = nullptr, *params = nullptr, *grad = nullptr, *m = nullptr,
         *v = nullptr, *Up = nullptr;
  AxisConst* kc = nullptr;
  StepScalars* sc = nullptr;
  int *count = nullptr, *loss_slot = nullptr, *status = nullptr;
  double *losses = nullptr, *diag = nullptr, *bgap = nullptr;
  double *K[3] = {}, *Kb[3] = {}, *D[3] = {}, *piv[3] = {}, *ldet[3] = {}, *pst[3] = {}, *Kinv[3] = {};
  double* Kc[3] = {};  // kept copy of K_k (GPK_FLAG3_REFINE: the refinement residuals), else null
  unsigned int* aflag[3] = {};
  // grid tensors (natural [p1][p2][p3] or, suffix p, mode-2 permuted [p2][p1][p3])
  double *Upp = nullptr, *A1 = nullptr, *A2p = nullptr, *A3 = nullptr, *Tm = nullptr, *Tp = nullptr,
         *Sp = nullptr, *S = nullptr, *Rx = nullptr, *Rz = nullptr, *Ryp = nullptr, *R = nullptr,
         *Rp = nullptr, *T1 = nullptr, *X1 = nullptr, *T2p = nullptr, *X2p = nullptr, *T3 = nullptr,
         *X3 = nullptr, *Y1 = nullptr, *Y2p = nullptr, *Y3 = nullptr;
  // gpk_create3_opv: the fields given (padded, natural layout; null: absent) and, per axis with a
  // field, W_k = a_k R (W[1] permuted).  They are allocations of their own: Rx / Ryp / Rz are the
  // refinement's residual scratch after k3_combine (build_refine).
  double *cf[3] = {}, *rho = nullptr, *W[3] = {};
  // gpk_create3_opn: derivative data on the faces of dfaces (0: none, and nothing below is
  // allocated or launched).  face[k]: axis k's rows d_f, residual planes r_f and partials, all
  // allocations of their own (Rx / Ryp / Rz and T* are refinement scratch at various points);
  // bt: the value gap and the derivative gap of the last step; nd: the derivative faces' entries
  int dfaces = 0;
  double *dvals = nullptr, *bt = nullptr, nd = 0.0;
  K3FaceAxis face[3] = {};
  int fpart[3] = {}, fchunk[3] = {};
  // gpk_create3_opc: the convective weights g_k (conv = 0: none, and nothing below is allocated or
  // launched).  Per axis with g_k != 0: the order-1 block D1_k (the assembly's DERIV_SPLIT), V_k =
  // g_k D1_k x_k A_k (V[1] permuted) and G_D1k = v g_k Q_(k) A_k,(k)^T (GD1); N = sum_k V_k and
  // Q = U . R in the natural layout (Q: axis 1 or 3 convective) and permuted (Qp: axis 2).  All are
  // allocations of their own (Rx / Ryp / Rz and T* are refinement scratch at various points).
  int conv = 0;
  double gconv[3] = {};
  // gpk_create3_opg: the quadratic gradient weights s_k and x_jk (pairs (1,2), (1,3), (2,3)) (gsq = 0:
  // none, and nothing below is allocated or launched).  gact[k]: axis k is gradient-active (g_k, s_k or
  // one of its pair weights non-zero; on every other handle this is g_k != 0).  On such a handle conv
  // is set (the two further launches, N and k3_adam_u_c are the convective handle's), V, Q and Qp stay
  // null, and per gradient-active axis P[k] = D1_k x_k A_k and Qk[k], its reverse operand (both
  // permuted on axis 2), are allocations of their own: nothing aliases build_refine's scratch.
  int gsq = 0;
  double gs[3] = {}, gx[3] = {};
  bool gact[3] = {};
  double *P[3] = {}, *Qk[3] = {};
  double *D1[3] = {}, *GD1[3] = {}, *V[3] = {}, *Nsum = nullptr, *Q = nullptr, *Qp = nullptr;
  // gpk_create3_opm: the cross weights of the pairs (1,2), (1,3), (2,3) (cross = 0: none, and
  // nothing below is allocated or launched).  Pair t = (j, k): Hx[t] = H_jk, Cx[t] = C_jk, Hb[t] =
  // m D1_k^T x_k R and Zb[t] = K_k^{-1} x_k Hb[t], natural for (1,3) and mode-2 permuted for (1,2)
  // and (2,3); Z1 = D1_1 x_1 A_1 natural (Z1p: its permuted copy, pair (1,2)), Z2p = D1_2 x_2 A_2
  // permuted, Zb12 = Zb[0] brought back to the natural layout.  All are allocations of their own;
  // the refinement's scratch of H_jk is Hb[t] (not yet formed) and that of Zb[t] is Cx[t] (read by
  // k3_combine_m before), so nothing here aliases build_refine's scratch.
  int cross = 0;
  double mx[3] = {};
  double *Z1 = nullptr, *Z1p = nullptr, *Z2p = nullptr, *Zb12 = nullptr;
  double *Hx[3] = {}, *Cx[3] = {}, *Hb[3] = {}, *Zb[3] = {};
  // gpk_create3_opq: the weights of the bi-pairs (1,2), (1,3), (2,3) (bi = 0: none, and nothing below
  // is allocated or launched).  Per axis of a present pair: the order-2 block DD_k (D2, the assembly's
  // DERIV_HIGH_D2 / DERIV_HIGH_SPLIT_D2) and its gradient G_DDk (GD2).  The grid tensors are the cross
  // pairs' with DD for D1: Hq[t] = H2_jk, Bq[t] = B_jk, Hbq[t] = q DD_k^T x_k R, Zbq[t] = K_k^{-1} x_k
  // Hbq[t]; Z21 = DD_1 x_1 A_1 (Z21p permuted), Z22p = DD_2 x_2 A_2, Zb212 = Zbq[0] in the natural
  // layout.  All are allocations of their own, so nothing aliases build_refine's scratch.
  int bi = 0;
  double bq[3] = {};
  double *D2[3] = {}, *GD2[3] = {};
  double *Z21 = nullptr, *Z21p = nullptr, *Z22p = nullptr, *Zb212 = nullptr;
  double *Hq[3] = {}, *Bq[3] = {}, *Hbq[3] = {}, *Zbq[3] = {};
  // gpk_create3_opb: the drift fields b_k (drift = 0: none, and nothing below is allocated or
  // launched).  Per axis with a field: bf[k] (padded, natural layout), Zd[k] = D1_k x_k A_k (Zd[1]
  // permuted; Z1 / Z2p themselves where a cross pair already forms them, else an allocation of its
  // own) and Ed[k] = b_k R (Ed[1] permuted), the reverse pass's operand.  None of them aliases
  // build_refine's scratch (Rx / Ryp / Rz, T1 / T2p / T3).
  int drift = 0;
  double *bf[3] = {}, *Zd[3] = {}, *Ed[3] = {};
  double *GK[3] = {}, *GD[3] = {};
  double *red_egap = nullptr, *red_quad = nullptr;
  int nred = 0;
  double *pgpart = nullptr, *pg = nullptr;
  int bpa = 0;
  std::vector<std::vector<GemmDesc>> stages;  // GEMM launches in stream order
  // a convective handle's two further launches: [0] the V_k, after stage 2 and its refinement;
  // [1] the G_D1k, after stage 3 (empty elsewhere)
  std::vector<std::vector<GemmDesc>> cstages;
  // a cross handle's eight further launches (build_pair_stages; empty elsewhere), and a bi-pair
  // handle's eight (qs)
  PairStages xs, qs;
  // a drift handle's further launches (build_drift_stages; empty elsewhere): [0] the Z_k no cross
  // pair forms (may be empty), [1] the sums into T_k, [2] the G_D1k
  std::vector<std::vector<GemmDesc>> dstages;
  // GPK_FLAG3_REFINE: the refinement launches, [2 j] the residuals and [2 j + 1] the corrections
  // that follow stage kRefineAfter[j] (empty without the flag)
  std::vector<std::vector<GemmDesc>> rstages;
  // route 1: one fused panel launch per solve instead (refine_panel.hip), [j] after kRefineAfter[j]
  std::vector<std::vector<RefinePanel>> rpanels;
  int route = 0;
  hipGraphExec_t exec[2] = {nullptr, nullptr};
};

namespace {

// Convective axes (gpk_create3_opc), after build_stages has filled stage 3: T_k becomes the dual
// product D_k^T x_k W_k + g_k D1_k^T x_k Q (same transposes as its first product; no descriptor of
// that batch reads a T_k, which launch_huge's two passes need), and two launches of their own hold
// V_k = g_k D1_k x_k A_k (next to the stage-2 products, whose batch is full) and G_D1k =
// v g_k Q_(k) A_k,(k)^T (next to the G_Dk).  Axis 2 stays in the permuted layout; axis 3 has D1 on
// the right, transposed like D[2].  (An axis is convective where g_k != 0: on a cross handle an axis
// of a pair owns a D1_k without being convective.)
void build_conv_stages(gpk_handle3* h) {
  const int P1 = h->g.p[0], P2 = h->g.p[1], P3 = h->g.p[2];
  const int M1 = P2 * P3, M2 = P1 * P3, M3 = P1 * P2;
  const double* g = h->gconv;
  double* const* D1 = h->D1;
  auto scaled = [](GemmDesc d, double alpha) { d.alpha = alpha; return d; };
  auto dual = [](GemmDesc& d, const double* A2, int lda2, const double* B2, int ldb2, int K2, double alpha2) {
    d.A2 = A2; d.lda2 = lda2; d.ta2 = d.ta; d.B2 = B2; d.ldb2 = ldb2; d.tb2 = d.tb; d.K2 = K2; d.alpha2 = alpha2;
  };
  auto& t = h->stages[3];
  if (g[0] != 0.0) dual(t[0], D1[0], P1, h->Q, M1, P1, g[0]);
  if (g[1] != 0.0) dual(t[1], D1[1], P2, h->Qp, M2, P2, g[1]);
  if (g[2] != 0.0) dual(t[2], h->Q, P3, D1[2], P3, P3, g[2]);
  h->cstages.assign(2, {});
  auto& cv = h->cstages[0];
  auto& cg = h->cstages[1];
  auto vs = [](GemmDesc d) { d.vscale = 1; return d; };
  if (g[0] != 0.0) {
    cv.push_back(scaled(gemm_desc(D1[0], P1, 0, h->A1, M1, 0, h->V[0], M1, P1, M1, P1), g[0]));
    cg.push_back(vs(scaled(gemm_desc(h->Q, M1, 0, h->A1, M1, 1, h->GD1[0], P1, P1, P1, M1), g[0])));
  }
  if (g[1] != 0.0) {
    cv.push_back(scaled(gemm_desc(D1[1], P2, 0, h->A2p, M2, 0, h->V[1], M2, P2, M2, P2), g[1]));
    cg.push_back(vs(scaled(gemm_desc(h->Qp, M2, 0, h->A2p, M2, 1, h->GD1[1], P2, P2, P2, M2), g[1])));
  }
  if (g[2] != 0.0) {
    cv.push_back(scaled(gemm_desc(h->A3, P3, 0, D1[2], P3, 1, h->V[2], P3, M3, P3, P3), g[2]));
    cg.push_back(vs(scaled(gemm_desc(h->Q, P3, 1, h->A3, P3, 0, h->GD1[2], P3, P3, P3, M3), g[2])));
  }
}

// Quadratic gradient terms (gpk_create3_opg), in build_conv_stages' place: per gradient-active axis
// T_k becomes the dual product D_k^T x_k W_k + D1_k^T x_k Q_k (alpha2 = 1: the weights are in Q_k), and
// the two launches hold P_k = D1_k x_k A_k (alpha 1; k3_combine_g applies g_k, s_k and x_jk) and G_D1k =
// v Q_k,(k) A_k,(k)^T.  Layouts and transposes are build_conv_stages' own.
void build_gradsq_stages(gpk_handle3* h) {
  const int P1 = h->g.p[0], P2 = h->g.p[1], P3 = h->g.p[2];
  const int M1 = P2 * P3, M2 = P1 * P3, M3 = P1 * P2;
  double* const* D1 = h->D1;
  auto dual = [](GemmDesc& d, const double* A2, int lda2, const double* B2, int ldb2, int K2) {
    d.A2 = A2; d.lda2 = lda2; d.ta2 = d.ta; d.B2 = B2; d.ldb2 = ldb2; d.tb2 = d.tb; d.K2 = K2; d.alpha2 = 1.0;
  };
  auto& t = h->stages[3];
  if (h->gact[0]) dual(t[0], D1[0], P1, h->Qk[0], M1, P1);
  if (h->gact[1]) dual(t[1], D1[1], P2, h->Qk[1], M2, P2);
  if (h->gact[2]) dual(t[2], h->Qk[2], P3, D1[2], P3, P3);
  h->cstages.assign(2, {});
  auto& cp = h->cstages[0];
  auto& cg = h->cstages[1];
  auto vs = [](GemmDesc d) { d.vscale = 1; return d; };
  if (h->gact[0]) {
    cp.push_back(gemm_desc(D1[0], P1, 0, h->A1, M1, 0, h->P[0], M1, P1, M1, P1));
    cg.push_back(vs(gemm_desc(h->Qk[0], M1, 0, h->A1, M1, 1, h->GD1[0], P1, P1, P1, M1)));
  }
  if (h->gact[1]) {
    cp.push_back(gemm_desc(D1[1], P2, 0, h->A2p, M2, 0, h->P[1], M2, P2, M2, P2));
    cg.push_back(vs(gemm_desc(h->Qk[1], M2, 0, h->A2p, M2, 1, h->GD1[1], P2, P2, P2, M2)));
  }
  if (h->gact[2]) {
    cp.push_back(gemm_desc(h->A3, P3, 0, D1[2], P3, 1, h->P[2], P3, M3, P3, P3));
    cg.push_back(vs(gemm_desc(h->Qk[2], P3, 1, h->A3, P3, 0, h->GD1[2], P3, P3, P3, M3)));
  }
}

// Pairs of axes (j, k), j < k, in the order (1,2), (1,3), (2,3): the mixed partials m_jk d^2u/dx_j dx_k
// (gpk_create3_opm; the block G is D1) and the mixed fourth-order partials q_jk d^4u/dx_j^2 dx_k^2
// (gpk_create3_opq; G is DD).  One builder serves both: a PairSet names the weights, the block per
// axis, its gradient target per axis (add[k]: the target already holds something in the stream) and
// the buffers; it runs after build_stages, build_conv_stages and build_refine.  Pair (1,2) runs on
// the permuted copy of Z_1 and brings Zb_12 back to the natural layout for axis 1's sums; (1,3) is
// natural throughout with K_3^{-1} and G_3 on the right; (2,3) is permuted throughout, mode 3 still
// being the contiguous index there.  Launches, in stream order:
//   [0] Z_j = G_j x_j A_j  [1] H_jk (solves)  [2] C_jk = w G_k x_k H_jk    after stage 2, before the combine
//   [3] Hb_jk = w G_k^T x_k R  [4] Zb_jk (solves)  [5] T_j += G_j^T x_j Zb_jk  [6] dL/dG
//                                                     after stage 3, before stage 4
//   [7] G_Kk -= v Zb_jk,(k) H_jk,(k)^T                after the last stage
// An axis takes at most two pair products into T_j, dL/dG or G_Kk: they share one descriptor (the
// dual-product slot), which adds them to what the target holds (C0 = C, beta = 1: every GEMM kernel
// reads C0 at the element it then writes, in the same thread, as the refinement's in-place
// corrections rely on; launch_huge's first pass does the same and its second reads C alone).  A
// dL/dG that holds nothing yet is written, not added to.  The refinement's scratch of H_jk is Hb_jk
// (not yet formed) and that of Zb_jk is C_jk (the combine kernel has read it).
struct PairSet {
  const double* w;       // [3] pair weights (0: absent)
  double* const* G;      // [3] the block per axis
  double* const* GG;     // [3] dL/dG per axis
  bool add[3];
  double *Z1, *Z1p, *Z2p, *Zb12;
  double* const* Hx; double* const* Cx; double* const* Hb; double* const* Zb;
};

void build_pair_stages(gpk_handle3* h, const PairSet& ps, PairStages& out) {
  const int P1 = h->g.p[0], P2 = h->g.p[1], P3 = h->g.p[2];
  const int M1 = P2 * P3, M2 = P1 * P3, M3 = P1 * P2;
  const double* m = ps.w;
  double* const* Ki = h->Kinv;
  double* const* G = ps.G;
  const bool on[3] = {m[0] != 0.0, m[1] != 0.0, m[2] != 0.0};
  const bool refine = !h->rstages.empty();
  auto scaled = [](GemmDesc d, double alpha) { d.alpha = alpha; return d; };
  auto& xs = out.st;
  xs.assign(8, {});
  out.rst.assign(refine ? 4 : 0, {});
  out.rp.assign(refine ? 2 : 0, {});
  // solve i (0: H_jk, 1: Zb_jk) of a pair against its outer axis a (1: left, permuted; 2: right)
  auto solve = [&](int i, int a, const double* B, double* X, double* W) {
    const bool right = a == 2;
    const int rows = right ? M3 : P2, cols = right ? P3 : M2;
    const RefinedSolve s = refined_solve(right, h->Kc[a], Ki[a], B, X, W, rows, cols, h->pst[a]);
    xs[i ? 4 : 1].push_back(s.solve);
    if (!refine) return;
    out.rst[2 * i].push_back(s.resid);
    out.rst[2 * i + 1].push_back(s.fix);
    out.rp[i].push_back(refine_panel_desc(right, h->Kc[a], Ki[a], B, X, rows, cols, h->pst[a]));
  };
  if (on[0] || on[1]) xs[0].push_back(gemm_desc(G[0], P1, 0, h->A1, M1, 0, ps.Z1, M1, P1, M1, P1));
  if (on[2]) xs[0].push_back(gemm_desc(G[1], P2, 0, h->A2p, M2, 0, ps.Z2p, M2, P2, M2, P2));
  if (on[0]) {  // (1,2), permuted
    solve(0, 1, ps.Z1p, ps.Hx[0], ps.Hb[0]);
    xs[2].push_back(scaled(gemm_desc(G[1], P2, 0, ps.Hx[0], M2, 0, ps.Cx[0], M2, P2, M2, P2), m[0]));
    xs[3].push_back(scaled(gemm_desc(G[1], P2, 1, h->Rp, M2, 0, ps.Hb[0], M2, P2, M2, P2), m[0]));
    solve(1, 1, ps.Hb[0], ps.Zb[0], ps.Cx[0]);
  }
  if (on[1]) {  // (1,3), natural
    solve(0, 2, ps.Z1, ps.Hx[1], ps.Hb[1]);
    xs[2].push_back(scaled(gemm_desc(ps.Hx[1], P3, 0, G[2], P3, 1, ps.Cx[1], P3, M3, P3, P3), m[1]));
    xs[3].push_back(scaled(gemm_desc(h->R, P3, 0, G[2], P3, 0, ps.Hb[1], P3, M3, P3, P3), m[1]));
    solve(1, 2, ps.Hb[1], ps.Zb[1], ps.Cx[1]);
  }
  if (on[2]) {  // (2,3), permuted
    solve(0, 2, ps.Z2p, ps.Hx[2], ps.Hb[2]);
    xs[2].push_back(scaled(gemm_desc(ps.Hx[2], P3, 0, G[2], P3, 1, ps.Cx[2], P3, M3, P3, P3), m[2]));
    xs[3].push_back(scaled(gemm_desc(h->Rp, P3, 0, G[2], P3, 0, ps.Hb[2], P3, M3, P3, P3), m[2]));
    solve(1, 2, ps.Hb[2], ps.Zb[2], ps.Cx[2]);
  }
  // up to two products into one target: the second in the dual slot, each with its own factor
  struct Prod { const double* A; int lda, ta; const double* B; int ldb, tb, K; double alpha; };
  auto sum = [](const std::vector<Prod>& p, double* C, int ldc, int M, int N, bool add, int vs) {
    GemmDesc d = gemm_desc(p[0].A, p[0].lda, p[0].ta, p[0].B, p[0].ldb, p[0].tb, C, ldc, M, N, p[0].K);
    d.alpha = p[0].alpha; d.vscale = vs;
    if (p.size() > 1) {
      d.A2 = p[1].A; d.lda2 = p[1].lda; d.ta2 = p[1].ta; d.B2 = p[1].B; d.ldb2 = p[1].ldb; d.tb2 = p[1].tb;
      d.K2 = p[1].K; d.alpha2 = p[1].alpha; d.vscale2 = vs;
    }
    if (add) { d.beta = 1.0; d.C0 = C; d.ldc0 = ldc; }
    return d;
  };
  // T_1 += G_1^T x_1 (Zb_12 + Zb_13);  T_2 += G_2^T x_2 Zb_23 (permuted)
  {
    std::vector<Prod> t1;
    if (on[0]) t1.push_back({G[0], P1, 1, ps.Zb12, M1, 0, P1, 1.0});
    if (on[1]) t1.push_back({G[0], P1, 1, ps.Zb[1], M1, 0, P1, 1.0});
    if (!t1.empty()) xs[5].push_back(sum(t1, h->T1, M1, P1, M1, true, 0));
    if (on[2]) xs[5].push_back(sum({{G[1], P2, 1, ps.Zb[2], M2, 0, P2, 1.0}}, h->T2p, M2, P2, M2, true, 0));
  }
  // dL/dG per axis: inner products v Zb_(j) A_j^T, outer products v w R_(k) H_(k)^T
  {
    std::vector<Prod> g1, g2, g3;
    if (on[0]) g1.push_back({ps.Zb12, M1, 0, h->A1, M1, 1, M1, 1.0});
    if (on[1]) g1.push_back({ps.Zb[1], M1, 0, h->A1, M1, 1, M1, 1.0});
    if (on[0]) g2.push_back({h->Rp, M2, 0, ps.Hx[0], M2, 1, M2, m[0]});
    if (on[2]) g2.push_back({ps.Zb[2], M2, 0, h->A2p, M2, 1, M2, 1.0});
    if (on[1]) g3.push_back({h->R, P3, 1, ps.Hx[1], P3, 0, M3, m[1]});
    if (on[2]) g3.push_back({h->Rp, P3, 1, ps.Hx[2], P3, 0, M3, m[2]});
    if (!g1.empty()) xs[6].push_back(sum(g1, ps.GG[0], P1, P1, P1, ps.add[0], 1));
    if (!g2.empty()) xs[6].push_back(sum(g2, ps.GG[1], P2, P2, P2, ps.add[1], 1));
    if (!g3.empty()) xs[6].push_back(sum(g3, ps.GG[2], P3, P3, P3, ps.add[2], 1));
  }
  // G_K2 -= v Zb_12,(2) H_12,(2)^T;  G_K3 -= v (Zb_13,(3) H_13,(3)^T + Zb_23,(3) H_23,(3)^T)
  {
    std::vector<Prod> k3;
    if (on[0]) xs[7].push_back(sum({{ps.Zb[0], M2, 0, ps.Hx[0], M2, 1, M2, -1.0}}, h->GK[1], P2, P2, P2, true, 1));
    if (on[1]) k3.push_back({ps.Zb[1], P3, 1, ps.Hx[1], P3, 0, M3, -1.0});
    if (on[2]) k3.push_back({ps.Zb[2], P3, 1, ps.Hx[2], P3, 0, M3, -1.0});
    if (!k3.empty()) xs[7].push_back(sum(k3, h->GK[2], P3, P3, P3, true, 1));
  }
}

// the cross pairs: G = D1, dL/dD1 added to where the axis is convective or gradient-active (its
// G_D1k came first)
void build_cross_stages(gpk_handle3* h) {
  const PairSet ps{h->mx, h->D1, h->GD1, {h->gact[0], h->gact[1], h->gact[2]},
                   h->Z1, h->Z1p, h->Z2p, h->Zb12, h->Hx, h->Cx, h->Hb, h->Zb};
  build_pair_stages(h, ps, h->xs);
}

// the bi-pairs: G = DD, and nothing precedes dL/dDD in the stream (written, beta = 0)
void build_bicross_stages(gpk_handle3* h) {
  const PairSet ps{h->bq, h->D2, h->GD2, {false, false, false},
                   h->Z21, h->Z21p, h->Z22p, h->Zb212, h->Hq, h->Bq, h->Hbq, h->Zbq};
  build_pair_stages(h, ps, h->qs);
}

// Drift fields (gpk_create3_opb), after build_stages, build_conv_stages and the pair stages.
// Axis 2 stays in the permuted layout; axis 3 has D1 on the right, transposed like D[2].  Launches,
// in stream order:
//   [0] Z_k = D1_k x_k A_k of the drift axes no cross pair serves    after stage 2 and the V_k
//   [1] T_k += D1_k^T x_k E_k   [2] G_D1k (+)= v E_k,(k) A_k,(k)^T   after stage 3 and the cross
//                                                                    handle's G_D1, before stage 4
// The stage-3 dual slot (a convective axis) and the cross sums' two slots can all be full on one
// axis, so the sums into T_k are launches of their own under build_pair_stages' aliasing rule
// (C0 = C, beta = 1).  These launches are the last producers of G_D1k in the stream: the convective
// launch writes it, the cross launch writes or adds, and a drift axis adds when either came before
// and writes when it is the first.
void build_drift_stages(gpk_handle3* h) {
  const int P1 = h->g.p[0], P2 = h->g.p[1], P3 = h->g.p[2];
  const int M1 = P2 * P3, M2 = P1 * P3, M3 = P1 * P2;
  double* const* D1 = h->D1;
  const double* m = h->mx;
  // axis k already has a G_D1k in the stream: convective or gradient-active, or an axis of a present pair
  const bool held[3] = {h->gact[0] || m[0] != 0.0 || m[1] != 0.0,
                        h->gact[1] || m[0] != 0.0 || m[2] != 0.0,
                        h->gact[2] || m[1] != 0.0 || m[2] != 0.0};
  auto into = [](GemmDesc d, bool add, int vs) {
    d.vscale = vs;
    if (add) { d.beta = 1.0; d.C0 = d.C; d.ldc0 = d.ldc; }
    return d;
  };
  auto& ds = h->dstages;
  ds.assign(3, {});
  if (h->bf[0]) {
    if (h->Zd[0] != h->Z1) ds[0].push_back(gemm_desc(D1[0], P1, 0, h->A1, M1, 0, h->Zd[0], M1, P1, M1, P1));
    ds[1].push_back(into(gemm_desc(D1[0], P1, 1, h->Ed[0], M1, 0, h->T1, M1, P1, M1, P1), true, 0));
    ds[2].push_back(into(gemm_desc(h->Ed[0], M1, 0, h->A1, M1, 1, h->GD1[0], P1, P1, P1, M1), held[0], 1));
  }
  if (h->bf[1]) {
    if (h->Zd[1] != h->Z2p) ds[0].push_back(gemm_desc(D1[1], P2, 0, h->A2p, M2, 0, h->Zd[1], M2, P2, M2, P2));
    ds[1].push_back(into(gemm_desc(D1[1], P2, 1, h->Ed[1], M2, 0, h->T2p, M2, P2, M2, P2), true, 0));
    ds[2].push_back(into(gemm_desc(h->Ed[1], M2, 0, h->A2p, M2, 1, h->GD1[1], P2, P2, P2, M2), held[1], 1));
  }
  if (h->bf[2]) {
    ds[0].push_back(gemm_desc(h->A3, P3, 0, D1[2], P3, 1, h->Zd[2], P3, M3, P3, P3));
    ds[1].push_back(into(gemm_desc(h->Ed[2], P3, 0, D1[2], P3, 0, h->T3, P3, M3, P3, P3), true, 0));
    ds[2].push_back(into(gemm_desc(h->Ed[2], P3, 1, h->A3, P3, 0, h->GD1[2], P3, P3, P3, M3), held[2], 1));
  }
}

// the step's GEMM launches (stream order; independent products of one launch batched)
void build_stages(gpk_handle3* h) {
  const int P1 = h->g.p[0], P2 = h->g.p[1], P3 = h->g.p[2];
  const int M1 = P2 * P3, M2 = P1 * P3, M3 = P1 * P2;
  const double n1 = h->g.n[0], n2 = h->g.n[1], n3 = h->g.n[2], c = h->prob.logdet;
  double* const* Ki = h->Kinv;
  double* const* D = h->D;
  const double* w = h->op.coef;  // c_k rides on every product with D_k (exact at 1.0)
  auto scaled = [](GemmDesc d, double alpha) { d.alpha = alpha; return d; };
  // the reverse pass's operand of axis k: a_k R on an axis with a field, else R (Rp on axis 2)
  const double* W1 = h->W[0] ? h->W[0] : h->R;
  const double* W2p = h->W[1] ? h->W[1] : h->Rp;
  const double* W3 = h->W[2] ? h->W[2] : h->R;
  auto& st = h->stages;
  st.clear();
  // forward: A1 = K1^{-1} x1 U, A3 = K3^{-1} x3 U
  st.push_back({gemm_desc(Ki[0], P1, 0, h->Up, M1, 0, h->A1, M1, P1, M1, P1),
                gemm_desc(h->Up, P3, 0, Ki[2], P3, 0, h->A3, P3, M3, P3, P3)});
  // (U permuted) A2 = K2^{-1} x2 U;  T = A1 x3 K3^{-1}
  st.push_back({gemm_desc(Ki[1], P2, 0, h->Upp, M2, 0, h->A2p, M2, P2, M2, P2),
                gemm_desc(h->A1, P3, 0, Ki[2], P3, 0, h->Tm, P3, M3, P3, P3)});
  // (T permuted) S = K2^{-1} x2 T;  U_xx = D1 x1 A1, U_yy = D2 x2 A2, U_zz = D3 x3 A3
  st.push_back({gemm_desc(Ki[1], P2, 0, h->Tp, M2, 0, h->Sp, M2, P2, M2, P2),
                scaled(gemm_desc(D[0], P1, 0, h->A1, M1, 0, h->Rx, M1, P1, M1, P1), w[0]),
                scaled(gemm_desc(D[1], P2, 0, h->A2p, M2, 0, h->Ryp, M2, P2, M2, P2), w[1]),
                scaled(gemm_desc(h->A3, P3, 0, D[2], P3, 1, h->Rz, P3, M3, P3, P3), w[2])});
  // (R, S combined) reverse: c_k D_k^T x_k W_k;  G_D1 = v c_1 W1_(1) A1_(1)^T
  {
    GemmDesc gd = scaled(gemm_desc(W1, M1, 0, h->A1, M1, 1, h->GD[0], P1, P1, P1, M1), w[0]);
    gd.vscale = 1;
    st.push_back({scaled(gemm_desc(D[0], P1, 1, W1, M1, 0, h->T1, M1, P1, M1, P1), w[0]),
                  scaled(gemm_desc(D[1], P2, 1, W2p, M2, 0, h->T2p, M2, P2, M2, P2), w[1]),
                  scaled(gemm_desc(W3, P3, 0, D[2], P3, 0, h->T3, P3, M3, P3, P3), w[2]), gd});
  }
  if (h->gsq) build_gradsq_stages(h);
  else if (h->conv) build_conv_stages(h);
  // X_k = K_k^{-1} x_k (c_k D_k^T x_k R) with the side outputs Y_k = S/2 + v X_k;  G_D2
  {
    GemmDesc gd = scaled(gemm_desc(W2p, M2, 0, h->A2p, M2, 1, h->GD[1], P2, P2, P2, M2), w[1]);
    gd.vscale = 1;
    st.push_back({with_side(gemm_desc(Ki[0], P1, 0, h->T1, M1, 0, h->X1, M1, P1, M1, P1), h->Y1, h->S, M1),
                  with_side(gemm_desc(Ki[1], P2, 0, h->T2p, M2, 0, h->X2p, M2, P2, M2, P2), h->Y2p, h->Sp, M2),
                  with_side(gemm_desc(h->T3, P3, 0, Ki[2], P3, 0, h->X3, P3, M3, P3, P3), h->Y3, h->S, P3), gd});
  }
  // G_K_k = c/2 (N / N_k) K_k^{-1} - Y_k,(k) A_k,(k)^T;  G_D3
  {
    GemmDesc g1 = gemm_desc(h->Y1, M1, 0, h->A1, M1, 1, h->GK[0], P1, P1, P1, M1);
    g1.alpha = -1.0; g1.beta = 0.5 * c * n2 * n3; g1.C0 = Ki[0]; g1.ldc0 = P1;
    GemmDesc g2 = gemm_desc(h->Y2p, M2, 0, h->A2p, M2, 1, h->GK[1], P2, P2, P2, M2);
    g2.alpha = -1.0; g2.beta = 0.5 * c * n1 * n3; g2.C0 = Ki[1]; g2.ldc0 = P2;
    GemmDesc g3 = gemm_desc(h->Y3, P3, 1, h->A3, P3, 0, h->GK[2], P3, P3, P3, M3);
    g3.alpha = -1.0; g3.beta = 0.5 * c * n1 * n2; g3.C0 = Ki[2]; g3.ldc0 = P3;
    GemmDesc gd = scaled(gemm_desc(W3, P3, 1, h->A3, P3, 0, h->GD[2], P3, P3, P3, M3), w[2]);
    gd.vscale = 1;
    st.push_back({g1, g2, g3, gd});
  }
}

// Refinement of the solves stage kRefineAfter[j] forms: W = B - Kc_k x_k X, then X += K_k^{-1} x_k W
// in place, both gated on axis k's pst (a closed gate ends every workgroup before any load, so X
// and the scratch keep their values).  W lives in tensors that are free at that point: T1 / T2p /
// T3 until stage 3 writes them, Rx / Ryp / Rz once k3_combine has read them.  Mode 2 stays in
// the permuted layout.  The corrections of X_k rewrite the side output Y_k from the refined X_k.
// Route 1 does each solve's two GEMMs in one fused panel launch (no W tensor).  It measured faster
// at every size it can run, so it is the handle's route whenever every
// padded size is <= REFINE_PANEL_MAX_P (the panels fit LDS); GPK_FLAG3_REFINE_GEMM forces route 0.
constexpr int kRefineAfter[4] = {0, 1, 2, 4};

void build_refine(gpk_handle3* h) {
  const int P1 = h->g.p[0], P2 = h->g.p[1], P3 = h->g.p[2];
  const int M1 = P2 * P3, M2 = P1 * P3, M3 = P1 * P2;
  const int Ps[3] = {P1, P2, P3}, Ms[3] = {M1, M2, M3};
  auto& rs = h->rstages;
  rs.assign(8, {});
  h->rpanels.assign(4, {});
  h->route = !(h->prob.flags & GPK_FLAG3_REFINE_GEMM) && std::max(P1, std::max(P2, P3)) <= REFINE_PANEL_MAX_P;
  // solve X = K_a^{-1} x_a B of axis a (a = 1: permuted operands; a = 2: K on the right), scratch W
  auto add = [&](int j, int a, const double* B, double* X, double* W) {
    const bool right = a == 2;
    const int rows = right ? Ms[a] : Ps[a], cols = right ? Ps[a] : Ms[a];
    const RefinedSolve s = refined_solve(right, h->Kc[a], h->Kinv[a], B, X, W, rows, cols, h->pst[a]);
    rs[2 * j].push_back(s.resid);
    rs[2 * j + 1].push_back(s.fix);
    h->rpanels[j].push_back(refine_panel_desc(right, h->Kc[a], h->Kinv[a], B, X, rows, cols, h->pst[a]));
  };
  add(0, 0, h->Up, h->A1, h->T1);      // A1
  add(0, 2, h->Up, h->A3, h->T3);      // A3
  add(1, 1, h->Upp, h->A2p, h->T2p);   // A2
  add(1, 2, h->A1, h->Tm, h->T3);      // T = A1 x3 K3^{-1}
  add(2, 1, h->Tp, h->Sp, h->T2p);     // S = K2^{-1} x2 T
  add(3, 0, h->T1, h->X1, h->Rx);      // X_k
  add(3, 1, h->T2p, h->X2p, h->Ryp);
  add(3, 2, h->T3, h->X3, h->Rz);
  double* const Y[3] = {h->Y1, h->Y2p, h->Y3};
  const double* const Ys[3] = {h->S, h->Sp, h->S};
  const int ldy[3] = {M1, M2, P3};
  for (int a = 0; a < 3; ++a) {
    rs[7][a] = with_side(rs[7][a], Y[a], Ys[a], ldy[a]);
    h->rpanels[3][a].Y = Y[a]; h->rpanels[3][a].Ys = Ys[a];  // (ldy is X's leading dimension)
  }
}

int launch_descs(gpk_handle3* h, const std::vector<GemmDesc>& d) {
  return check_launch(launch_gemm_sized(d.data(), (int)d.size(), h->sc, h->s),
                      "gemm");
}

// the GEMM kernel a launch of these descriptors runs with (what gpk_stage_variants3 reports)
int stage_variant(const std::vector<GemmDesc>& d) { return gemm_variant(d.data(), (int)d.size(), 0); }

// stage k, then the refinement of its solves when the handle refines
int launch_stage(gpk_handle3* h, int k) {
  TRY(launch_descs(h, h->stages[k]));
  for (int j = 0; j < 4 && !h->rstages.empty(); ++j)
    if (kRefineAfter[j] == k) {
      if (h->route) {
        const auto& f = h->rpanels[j];
        TRY(check_launch(launch_refine_panel(f.data(), (int)f.size(), h->sc, h->s), "refine_panel"));
        continue;
      }
      TRY(launch_descs(h, h->rstages[2 * j]));
      TRY(launch_descs(h, h->rstages[2 * j + 1]));
    }
  return GPK_OK;
}

// a pair set's solves i (0: the H_jk, 1: the Zb_jk), then their refinement when the handle refines
int launch_pair_solves(gpk_handle3* h, const PairStages& p, int i) {
  TRY(launch_descs(h, p.st[i ? 4 : 1]));
  if (p.rst.empty()) return GPK_OK;
  if (h->route) {
    const auto& f = p.rp[i];
    return check_launch(launch_refine_panel(f.data(), (int)f.size(), h->sc, h->s), "refine_panel");
  }
  TRY(launch_descs(h, p.rst[2 * i]));
  return launch_descs(h, p.rst[2 * i + 1]);
}

K3Eq eq_layer(const gpk_handle3* h) {
  const double* r = h->op.react;
  K3Eq e{};
  e.ac = h->legacy_ac;
  e.on = !e.ac && (r[0] != 0.0 || r[1] != 0.0 || r[2] != 0.0);
  e.faces = h->op.faces;
  e.r1 = r[0]; e.r2 = r[1]; e.r3 = r[2];
  return e;
}

// Step constants, K_k and D_k, then K_k^{-1} and log det K_k at the current params: the front of
// the step, and all gpk_predict3 needs of it (apply = 0 leaves the Adam count alone).
int enqueue_inverse3(gpk_handle3* h, int apply) {
  const K3Geom& g = h->g;
  const int q = h->q, kind = h->prob.kind;
  K3Prep P{};
  P.g = g; P.params = h->params; P.q = q;
  for (int a = 0; a < 3; ++a) P.off_kp[a] = h->off_kp[a];
  P.off_tau = h->off_tau; P.off_v = h->off_v;
  P.kc = h->kc; P.sc = h->sc; P.count = h->count; P.apply = apply;
  P.b1 = h->prob.b1; P.b2 = h->prob.b2;
  P.Up = h->Up; P.bvals = h->bvals; P.nb = (int)(2 * ((long)g.n[1] * g.n[2] + (long)g.n[0] * g.n[2] + (long)g.n[0] * g.n[1]));
  P.faces = h->op.faces; P.bgap = h->bgap;
  TRY(check_launch(k3_launch_prep(P, h->s), "k3_prep"));
  // K_k, D_k: the 2-axis assembly kernel (per-pair path), its axis constants from the params
  AssembleArgs aa[3] = {};
  for (int a = 0; a < 3; ++a) {
    aa[a].x = h->x[a]; aa[a].n = g.n[a]; aa[a].p = g.p[a]; aa[a].kc = h->kc + a;
    aa[a].jitter = h->prob.jitter; aa[a].K = h->K[a]; aa[a].Kc = h->Kc[a]; aa[a].D = h->D[a];
    aa[a].deriv = h->mode[a]; aa[a].c2 = h->c2[a]; aa[a].c1 = h->c1[a]; aa[a].D1 = h->D1[a];
    aa[a].c4 = h->c4[a]; aa[a].c3 = h->c3[a]; aa[a].D2 = h->D2[a];
  }
  // (skip = 1: the constants are published by k3_prep; each workgroup derives its axis's own)
  PrepArgs p12{};
  p12.params = h->params; p12.off_kp[0] = h->off_kp[0]; p12.off_kp[1] = h->off_kp[1];
  p12.naxes = 2; p12.skip = 1;
  PrepArgs p3 = p12;
  p3.off_kp[0] = h->off_kp[2];
  p3.naxes = 1;
  // (one derivative mode per launch: axes 1-2 share theirs only when their modes are equal)
  if (h->mode[0] == h->mode[1]) {
    TRY(check_launch(launch_assemble(kind, q, aa, 2, p12, h->s), "assemble"));
  } else {
    PrepArgs p1 = p12, p2 = p12;
    p1.naxes = p2.naxes = 1;
    p2.off_kp[0] = h->off_kp[1];
    TRY(check_launch(launch_assemble(kind, q, aa, 1, p1, h->s), "assemble"));
    TRY(check_launch(launch_assemble(kind, q, aa + 1, 1, p2, h->s), "assemble"));
  }
  TRY(check_launch(launch_assemble(kind, q, aa + 2, 1, p3, h->s), "assemble"));
  // K_k^{-1} and log det K_k (per-sweep Cholesky-Gauss-Jordan inverse; the output buffer of
  // each factor is fixed by its sweep count)
  SpdArgs sa[3] = {};
  for (int a = 0; a < 3; ++a) {
    sa[a].X = h->K[a]; sa[a].Y = h->Kb[a]; sa[a].p = g.p[a]; sa[a].n = g.n[a];
    sa[a].piv = h->piv[a]; sa[a].ldet = h->ldet[a]; sa[a].pst = h->pst[a];
    sa[a].status = h->status; sa[a].flag = h->aflag[a];
  }
  double* fin[3] = {};
  TRY(check_launch(launch_spd_inverse(sa, 2, fin, h->s, false), "spd_inverse"));
  TRY(check_launch(launch_spd_inverse(sa + 2, 1, fin + 2, h->s, false), "spd_inverse"));
  return GPK_OK;
}

int enqueue_step3(gpk_handle3* h, int apply) {
  const K3Geom& g = h->g;
  const int q = h->q, kind = h->prob.kind;
  TRY(enqueue_inverse3(h, apply));
  // forward products
  TRY(launch_stage(h, 0));
  TRY(check_launch(k3_launch_permute(h->Up, h->Upp, g, h->s), "k3_permute"));
  TRY(launch_stage(h, 1));
  // derivative faces: the rows d_f, then g_f and r_f from A_1, A_2 and A_3 (all formed by now)
  if (h->dfaces) {
    K3FaceRows FR{};
    for (int a = 0; a < 3; ++a) {
      FR.x[a] = h->x[a]; FR.n[a] = g.n[a]; FR.p[a] = g.p[a]; FR.row[a] = const_cast<double*>(h->face[a].row);
    }
    FR.kc = h->kc; FR.q = q; FR.dfaces = h->dfaces;
    TRY(check_launch(k3_launch_face_row(kind, FR, h->s), "k3_face_row"));
    for (int a = 0; a < 3; ++a)
      if (h->fpart[a]) TRY(check_launch(k3_launch_face_gap(h->face[a], a == 2, h->s), "k3_face_gap"));
  }
  TRY(check_launch(k3_launch_permute(h->Tm, h->Tp, g, h->s), "k3_permute"));
  TRY(launch_stage(h, 2));
  if (h->conv) TRY(launch_descs(h, h->cstages[0]));  // V_k (gsq: P_k), from the refined A_k
  if (h->drift && !h->dstages[0].empty()) TRY(launch_descs(h, h->dstages[0]));  // Z_k no cross pair forms
  if (h->cross) {  // Z_j from the refined A_j, H_jk (pair (1,2): on the permuted Z_1), C_jk
    TRY(launch_descs(h, h->xs.st[0]));
    if (h->Z1p) TRY(check_launch(k3_launch_permute(h->Z1, h->Z1p, g, h->s), "k3_permute"));
    TRY(launch_pair_solves(h, h->xs, 0));
    TRY(launch_descs(h, h->xs.st[2]));
  }
  if (h->bi) {  // the same with DD: Z2_j, H2_jk (pair (1,2): on the permuted Z2_1), B_jk
    TRY(launch_descs(h, h->qs.st[0]));
    if (h->Z21p) TRY(check_launch(k3_launch_permute(h->Z21, h->Z21p, g, h->s), "k3_permute"));
    TRY(launch_pair_solves(h, h->qs, 0));
    TRY(launch_descs(h, h->qs.st[2]));
  }
  K3Combine C{};
  C.g = g; C.Rx = h->Rx; C.Rz = h->Rz; C.Ryp = h->Ryp; C.F = h->F; C.Up = h->Up; C.Sp = h->Sp;
  C.eq = eq_layer(h); C.R = h->R; C.Rp = h->Rp; C.S = h->S;
  C.red_egap = h->red_egap; C.red_quad = h->red_quad;
  if (h->gsq) {  // k3_combine_q's superset: N from the P_k (no V_k, Q or Qp here), then Gamma
    K3CombineG Gx{};
    K3CombineB& B = Gx.q.b;
    K3CombineC& X = B.m.c;
    X.v.c = C; X.v.rho = h->rho;
    for (int a = 0; a < 3; ++a) {
      X.v.a[a] = h->cf[a]; X.v.W[a] = h->W[a];
      B.m.C[a] = h->Cx[a];
      B.b[a] = h->bf[a]; B.Z[a] = h->Zd[a]; B.E[a] = h->Ed[a];
      Gx.q.B[a] = h->Bq[a];
      Gx.P[a] = h->P[a]; Gx.Qk[a] = h->Qk[a];
      Gx.g[a] = h->gconv[a]; Gx.s[a] = h->gs[a]; Gx.x[a] = h->gx[a];
    }
    X.N = h->Nsum;
    B.m.rp = h->Cx[0] || h->Cx[2] || h->Bq[0] || h->Bq[2];
    TRY(check_launch(k3_launch_combine_g(Gx, h->s), "k3_combine_g"));
  } else if (h->bi) {  // k3_combine_b's superset: every older layer as the handle has it, absent ones null
    K3CombineQ Qx{};
    K3CombineB& B = Qx.b;
    K3CombineC& X = B.m.c;
    X.v.c = C; X.v.rho = h->rho;
    for (int a = 0; a < 3; ++a) {
      X.v.a[a] = h->cf[a]; X.v.W[a] = h->W[a]; X.V[a] = h->V[a];
      B.m.C[a] = h->Cx[a];
      B.b[a] = h->bf[a]; B.Z[a] = h->Zd[a]; B.E[a] = h->Ed[a];
      Qx.B[a] = h->Bq[a];
    }
    X.N = h->Nsum; X.Q = h->Q; X.Qp = h->Qp;
    B.m.rp = h->Cx[0] || h->Cx[2] || h->Bq[0] || h->Bq[2];
    TRY(check_launch(k3_launch_combine_q(Qx, h->s), "k3_combine_q"));
  } else if (h->conv || h->cross || h->drift) {
    K3CombineC X{};
    X.v.c = C; X.v.rho = h->rho;
    for (int a = 0; a < 3; ++a) { X.v.a[a] = h->cf[a]; X.v.W[a] = h->W[a]; X.V[a] = h->V[a]; }
    X.N = h->Nsum; X.Q = h->Q; X.Qp = h->Qp;
    if (h->cross || h->drift) {
      K3CombineM Mx{};
      Mx.c = X;
      Mx.C[0] = h->Cx[0]; Mx.C[1] = h->Cx[1]; Mx.C[2] = h->Cx[2];
      Mx.rp = h->Cx[0] || h->Cx[2];
      if (h->drift) {
        K3CombineB B{};
        B.m = Mx;
        for (int a = 0; a < 3; ++a) { B.b[a] = h->bf[a]; B.Z[a] = h->Zd[a]; B.E[a] = h->Ed[a]; }
        TRY(check_launch(k3_launch_combine_b(B, h->s), "k3_combine_b"));
      } else {
        TRY(check_launch(k3_launch_combine_m(Mx, h->s), "k3_combine_m"));
      }
    } else {
      TRY(check_launch(k3_launch_combine_c(X, h->s), "k3_combine_c"));
    }
  } else if (h->cf[0] || h->cf[1] || h->cf[2] || h->rho) {
    K3CombineV V{};
    V.c = C; V.rho = h->rho;
    for (int a = 0; a < 3; ++a) { V.a[a] = h->cf[a]; V.W[a] = h->W[a]; }
    TRY(check_launch(k3_launch_combine_v(V, h->s), "k3_combine_v"));
  } else {
    TRY(check_launch(k3_launch_combine(C, h->s), "k3_combine"));
  }
  // reverse products and G_K, G_D
  // (T_k takes the derivative faces' term before X_k = K_k^{-1} x_k T_k and its refinement read it)
  for (int k = 3; k < (int)h->stages.size(); ++k) {
    TRY(launch_stage(h, k));
    if (h->conv && k == 3) TRY(launch_descs(h, h->cstages[1]));  // G_D1k
    for (int a = 0; a < 3 && k == 3; ++a)
      if (h->fpart[a])
        TRY(check_launch(k3_launch_face_back(h->face[a], a == 2, h->sc, h->prob.llk_weight, h->s), "k3_face_back"));
    if (h->cross && k == 3) {  // Hb_jk, Zb_jk, then T_j's share before X_j = K_j^{-1} x_j T_j reads it; G_D1
      TRY(launch_descs(h, h->xs.st[3]));
      TRY(launch_pair_solves(h, h->xs, 1));
      if (h->Zb12) TRY(check_launch(k3_launch_unpermute(h->Zb[0], h->Zb12, g, h->s), "k3_permute"));
      TRY(launch_descs(h, h->xs.st[5]));
      TRY(launch_descs(h, h->xs.st[6]));
    }
    if (h->bi && k == 3) {  // Hb2_jk, Zb2_jk, T_j's share, G_DD
      TRY(launch_descs(h, h->qs.st[3]));
      TRY(launch_pair_solves(h, h->qs, 1));
      if (h->Zb212) TRY(check_launch(k3_launch_unpermute(h->Zbq[0], h->Zb212, g, h->s), "k3_permute"));
      TRY(launch_descs(h, h->qs.st[5]));
      TRY(launch_descs(h, h->qs.st[6]));
    }
    if (h->drift && k == 3) {  // T_k's drift share before X_k = K_k^{-1} x_k T_k reads it; G_D1k
      TRY(launch_descs(h, h->dstages[1]));
      TRY(launch_descs(h, h->dstages[2]));
    }
  }
  if (h->cross) TRY(launch_descs(h, h->xs.st[7]));  // G_Kk's share, added to the last stage's G_Kk
  if (h->bi) TRY(launch_descs(h, h->qs.st[7]));     // and the bi-pairs', after it
  // kernel-parameter contraction (the 2-axis kernels: axes 1-2, then axis 3)
  const int fb = h->dfaces ? K3_FACE_TAIL_BLOCKS : 0;  // + blocks of partials per axis: the face rows' (k3_face_tail)
  PGradArgs pg[3] = {};
  for (int a = 0; a < 3; ++a) {
    pg[a].x = h->x[a]; pg[a].n = g.n[a]; pg[a].p = g.p[a]; pg[a].kc = h->kc + a;
    pg[a].GK = h->GK[a]; pg[a].GD = h->GD[a]; pg[a].deriv = h->mode[a];
    pg[a].c2 = h->c2[a]; pg[a].c1 = h->c1[a]; pg[a].GD1 = h->GD1[a];
    pg[a].c4 = h->c4[a]; pg[a].c3 = h->c3[a]; pg[a].GD2 = h->GD2[a];
    pg[a].part = h->pgpart + (size_t)a * (h->bpa + fb) * 3 * QMAX;
  }
  if (h->mode[0] == h->mode[1]) {
    TRY(check_launch(launch_pgrad(kind, q, 0, pg, 2, h->bpa, h->sc, h->s), "pgrad"));
  } else {
    TRY(check_launch(launch_pgrad(kind, q, 0, pg, 1, h->bpa, h->sc, h->s), "pgrad"));
    TRY(check_launch(launch_pgrad(kind, q, 0, pg + 1, 1, h->bpa, h->sc, h->s), "pgrad"));
  }
  TRY(check_launch(launch_pgrad(kind, q, 0, pg + 2, 1, h->bpa, h->sc, h->s), "pgrad"));
  if (fb) {
    K3FaceTail T{};
    for (int a = 0; a < 3; ++a) {
      T.ax[a] = h->face[a]; T.x[a] = h->x[a]; T.npart[a] = h->fpart[a];
      T.out[a] = h->pgpart + ((size_t)a * (h->bpa + fb) + h->bpa) * 3 * QMAX;
      if (h->fchunk[a] > 1) TRY(check_launch(k3_launch_face_colsum(h->face[a], h->fchunk[a], h->s), "k3_face_colsum"));
    }
    T.kc = h->kc; T.sc = h->sc; T.llk_weight = h->prob.llk_weight; T.q = q; T.bgap = h->bgap; T.bt = h->bt;
    TRY(check_launch(k3_launch_face_tail(kind, T, h->s), "k3_face_tail"));
  }
  TRY(check_launch(launch_reduce_parts(h->pgpart, h->bpa + fb, 3, q, h->pg, h->s), "reduce_parts"));
  // loss + small-parameter Adam, then dL/dU + Adam on U (U is read by nothing after this)
  K3Final F{};
  F.g = g; F.hyper = AdamHyper{h->prob.lr, h->prob.b1, h->prob.b2, h->prob.eps};
  F.llk_weight = h->prob.llk_weight; F.logdet = h->prob.logdet; F.apply = apply;
  F.has_cos = kind_cos(kind) ? 1 : 0; F.q = q; F.faces = h->op.faces;
  F.red_quad = h->red_quad; F.red_egap = h->red_egap; F.nred = h->nred;
  for (int a = 0; a < 3; ++a) { F.ldet[a] = h->ldet[a]; F.nldet[a] = g.p[a] / 32; F.off_kp[a] = h->off_kp[a]; }
  F.pg = h->pg; F.kc = h->kc; F.sc = h->sc; F.bgap = h->bgap;
  F.off_tau = h->off_tau; F.off_v = h->off_v; F.off_small = (int)h->nu; F.nsmall = h->nsmall;
  F.params = h->params; F.grad = h->grad; F.m = h->m; F.v = h->v;
  F.losses = h->losses; F.loss_slot = h->loss_slot; F.diag = h->diag; F.nb_extra = h->nd;
  TRY(check_launch(k3_launch_finalize(F, h->s), "k3_finalize"));
  K3AdamU A{};
  A.g = g; A.hyper = F.hyper; A.llk_weight = h->prob.llk_weight; A.apply = apply; A.eq = C.eq;
  A.sc = h->sc; A.S = h->S; A.X1 = h->X1; A.X2p = h->X2p; A.X3 = h->X3; A.R = h->R; A.Up = h->Up;
  A.bvals = h->bvals; A.off_u = 0; A.params = h->params; A.grad = h->grad; A.m = h->m; A.v = h->v;
  if (h->conv) {
    TRY(check_launch(k3_launch_adam_u_c(K3AdamUC{A, h->rho, h->Nsum}, h->s), "k3_adam_u_c"));
  } else if (h->rho) {
    TRY(check_launch(k3_launch_adam_u_v(K3AdamUV{A, h->rho}, h->s), "k3_adam_u_v"));
  } else {
    TRY(check_launch(k3_launch_adam_u(A, h->s), "k3_adam_u"));
  }
  return GPK_OK;
}

int capture3(gpk_handle3* h, int apply) {
  if (h->exec[apply]) return GPK_OK;
  return capture_graph(h->s, &h->exec[apply], [&] { return enqueue_step3(h, apply); });
}

int read_status3(gpk_handle3* h) {
  int st = 0;
  HIPCHK(hipMemcpyAsync(&st, h->status, sizeof(int), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  // (no hand-off waits and no batches here: any status is a non-positive pivot)
  return st ? status_error(st, h->status, h->s, nullptr, false, false) : GPK_OK;
}

// K3Final::diag as the last step or gpk_loss_grad3 left it
int read_diag3(gpk_handle3* h, double diag[8]) {
  HIPCHK(hipMemcpy(diag, h->diag, 8 * sizeof(double), hipMemcpyDeviceToHost));
  return GPK_OK;
}

}  // namespace

extern "C" {

int gpk_destroy3(gpk_handle3* h) {
  if (!h) return GPK_OK;
  DevSwitch ds(h->dev);
  if (h->s) (void)hipStreamSynchronize(h->s);
  for (auto& e : h->exec)
    if (e) (void)hipGraphExecDestroy(e);
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->s) (void)hipStreamDestroy(h->s);
  delete h;
  return GPK_OK;
}

}  // extern "C"

namespace {

// what every create call checks of the problem itself, before any device work
int check_problem3(const gpk_problem3* p) {
  if (p->kind < 0 || p->kind > 3) return fail(GPK_EINVAL, "Invalid Kernel");
  if (p->q <= 0 || p->q > QMAX) return fail(GPK_EINVAL, "Q must be in [1, 64]");
  const int ns[3] = {p->n1, p->n2, p->n3};
  for (int a = 0; a < 3; ++a)
    if (ns[a] < 2 || ns[a] > K3_MAX_N) return fail(GPK_EINVAL, "need 2..1024 collocation points per axis");
  if (!p->x1 || !p->x2 || !p->x3 || !p->src || !p->bvals) return fail(GPK_EINVAL, "NULL problem array");
  return GPK_OK;
}

// gpk_create3 (op = nullptr: the legacy equation p->eq), gpk_create3_op, gpk_create3_opx (opx: op
// is its one-order-per-axis part, a mixed axis entered as order 0 with weight 1.0) and
// gpk_create3_opv (cf: the fields it was given, at least one of them)
int create3(const gpk_problem3* p, const gpk_operator3* op, double freq_scale, gpk_handle3** out,
            const gpk_operator3x* opx = nullptr, const gpk_coef3* cf = nullptr, const gpk_bdata3* bd = nullptr,
            const gpk_conv3* cv = nullptr, const gpk_cross3* mx = nullptr, const gpk_drift3* dr = nullptr,
            const gpk_high3* hi = nullptr, const gpk_bicross3* bq = nullptr, const gpk_gradsq3* gq = nullptr) {
  TRY(check_problem3(p));
  const int ns[3] = {p->n1, p->n2, p->n3};
  TRY(check_device(p->device));
  DevSwitch ds(p->device);
  gpk_handle3* h = new gpk_handle3();
  h->prob = *p;
  h->prob.x1 = h->prob.x2 = h->prob.x3 = h->prob.src = h->prob.bvals = nullptr;
  if (op) {
    h->op = *op;
  } else {
    for (int a = 0; a < 3; ++a) { h->op.order[a] = 2; h->op.coef[a] = 1.0; h->op.react[a] = 0.0; }
    h->op.faces = K3_ALL_FACES;
    h->legacy_ac = p->eq == GPK_ALLENCAHN;
    if (h->legacy_ac) { h->op.react[0] = -1.0; h->op.react[2] = 1.0; }  // what gpk_operator_info3 reports
  }
  for (int a = 0; a < 3; ++a) {
    const bool mixed = h->op.order[a] == 0;
    h->mode[a] = mixed ? DERIV_BOTH : h->op.order[a];
    // a convective axis (entered as a mixed one, whatever its weights): the two-block assembly
    if (cv && cv->g[a] != 0.0) {
      h->gconv[a] = cv->g[a];
      h->conv = 1;
      h->mode[a] = DERIV_SPLIT;
    }
    static const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    h->gact[a] = h->gconv[a] != 0.0;
    // so does a gradient-active axis (it owns D1_k and G_D1k: s_k, or a pair weight x_jk with a in it)
    if (gq) {
      h->gsq = h->conv = 1;
      h->gs[a] = gq->s[a];
      for (int t = 0; t < 3; ++t) {
        h->gx[t] = gq->x[t];
        if (gq->x[t] != 0.0 && (pairs[t][0] == a || pairs[t][1] == a)) h->gact[a] = true;
      }
      if (gq->s[a] != 0.0) h->gact[a] = true;
      if (h->gact[a]) h->mode[a] = DERIV_SPLIT;
    }
    // so does an axis of a pair with a cross weight (it owns D1_k and G_D1k as well)
    for (int t = 0; t < 3 && mx; ++t)
      if (mx->m[t] != 0.0 && (pairs[t][0] == a || pairs[t][1] == a)) {
        h->mx[t] = mx->m[t];
        h->cross = 1;
        h->mode[a] = DERIV_SPLIT;
      }
    // and a drift axis (D1_k and G_D1k likewise)
    if (dr && dr->b[a]) {
      h->drift = 1;
      h->mode[a] = DERIV_SPLIT;
    }
    // a high-order axis (entered as a mixed one): the four-field block, with D1_k alongside where
    // the axis owns one
    if (hi && (hi->c4[a] != 0.0 || hi->c3[a] != 0.0)) {
      h->c4[a] = hi->c4[a];
      h->c3[a] = hi->c3[a];
      h->mode[a] = h->mode[a] == DERIV_SPLIT ? DERIV_HIGH_SPLIT : DERIV_HIGH;
    }
    // an axis of a pair with a bi weight (entered as a mixed one): the four-field block whatever c4
    // and c3 are, with DD_k stored alongside (and D1_k where the axis owns one)
    for (int t = 0; t < 3 && bq; ++t)
      if (bq->q[t] != 0.0 && (pairs[t][0] == a || pairs[t][1] == a)) {
        h->bq[t] = bq->q[t];
        h->bi = 1;
        h->mode[a] = deriv_stores_d1(h->mode[a]) ? DERIV_HIGH_SPLIT_D2 : DERIV_HIGH_D2;
      }
    h->c2[a] = mixed ? opx->c2[a] : h->op.order[a] == 2 ? h->op.coef[a] : 0.0;
    h->c1[a] = mixed ? opx->c1[a] : h->op.order[a] == 1 ? h->op.coef[a] : 0.0;
  }
  h->dev = p->device;
  h->q = p->q;
  for (int a = 0; a < 3; ++a) {
    h->g.n[a] = ns[a];
    h->g.p[a] = pad_up(ns[a]);
  }
  const K3Geom& g = h->g;
  h->nu = g.real();
  for (int a = 0; a < 3; ++a) h->off_kp[a] = (int)h->nu + 3 * p->q * a;
  h->off_tau = (int)h->nu + 9 * p->q;
  h->off_v = h->off_tau + 1;
  h->nsmall = 9 * p->q + 2;
  h->nparams = h->nu + h->nsmall;
  auto bail = [&](int rc) {
    gpk_destroy3(h);
    return rc;
  };
  if (hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(GPK_EHIP, "hipStreamCreate failed"));
  const size_t np = (size_t)g.padded();
  const long nb = 2 * ((long)ns[1] * ns[2] + (long)ns[0] * ns[2] + (long)ns[0] * ns[1]);
  int rc = GPK_OK;
#define A3_(ptr, n) \
  if ((rc = dev_alloc(h->allocs, h->s, &(ptr), (n))) != GPK_OK) return bail(rc)
  for (int a = 0; a < 3; ++a) {
    const int P = g.p[a];
    A3_(h->x[a], P);
    A3_(h->K[a], (size_t)P * P);
    A3_(h->Kb[a], (size_t)P * P);
    A3_(h->D[a], (size_t)P * P);
    A3_(h->piv[a], (size_t)P * 32);
    A3_(h->ldet[a], P / 32);
    A3_(h->pst[a], 2);
    A3_(h->aflag[a], 1);
    A3_(h->GK[a], (size_t)P * P);
    A3_(h->GD[a], (size_t)P * P);
    if (p->flags & GPK_FLAG3_REFINE) A3_(h->Kc[a], (size_t)P * P);
    const int T = P / 32;  // sweep k reads (k even ? K : Kb): T sweeps end in
    h->Kinv[a] = (T & 1) ? h->Kb[a] : h->K[a];
  }
  A3_(h->F, np); A3_(h->bvals, nb);
  A3_(h->params, h->nparams); A3_(h->grad, h->nparams); A3_(h->m, h->nparams); A3_(h->v, h->nparams);
  A3_(h->Up, np);
  A3_(h->kc, 3); A3_(h->sc, 1); A3_(h->count, 1); A3_(h->loss_slot, 1); A3_(h->status, 1);
  A3_(h->losses, K3_LOSS_CAP); A3_(h->diag, 8); A3_(h->bgap, 1);
  double** tens[] = {&h->Upp, &h->A1, &h->A2p, &h->A3, &h->Tm, &h->Tp, &h->Sp, &h->S, &h->Rx,
                     &h->Rz, &h->Ryp, &h->R, &h->Rp, &h->T1, &h->X1, &h->T2p, &h->X2p, &h->T3,
                     &h->X3, &h->Y1, &h->Y2p, &h->Y3};
  for (double** t : tens) A3_(*t, np);
  h->nred = k3_combine_blocks(g);
  A3_(h->red_egap, h->nred); A3_(h->red_quad, h->nred);
  h->bpa = std::max(pgrad_blocks(ns[0]), std::max(pgrad_blocks(ns[1]), pgrad_blocks(ns[2])));
  A3_(h->pgpart, (size_t)3 * (h->bpa + (bd ? K3_FACE_TAIL_BLOCKS : 0)) * 3 * QMAX);
  A3_(h->pg, (size_t)3 * 3 * QMAX);
  // the fields: zero-padded natural-layout tensors, and W_k for each axis that has one
  if (cf) {
    std::vector<double> fp(np);
    const double* given[4] = {cf->a[0], cf->a[1], cf->a[2], cf->rho};
    double** dst[4] = {&h->cf[0], &h->cf[1], &h->cf[2], &h->rho};
    for (int k = 0; k < 4; ++k) {
      if (!given[k]) continue;
      A3_(*dst[k], np);
      if (k < 3) A3_(h->W[k], np);
      std::fill(fp.begin(), fp.end(), 0.0);
      for (int i1 = 0; i1 < ns[0]; ++i1)
        for (int i2 = 0; i2 < ns[1]; ++i2)
          std::memcpy(&fp[g.at(i1, i2, 0)], given[k] + ((size_t)i1 * ns[1] + i2) * ns[2], ns[2] * sizeof(double));
      if (hipMemcpyAsync(*dst[k], fp.data(), np * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess ||
          hipStreamSynchronize(h->s) != hipSuccess)
        return bail(fail(GPK_EHIP, "upload of a coefficient field failed"));
    }
  }
  // derivative data: the six-face array as given (entries of faces outside dfaces are never read),
  // and per axis with such a face the rows, residual planes and partials
  if (bd) {
    static_assert(K3_FACE_MAX_N == K3_MAX_N, "k3_face_tail's LDS rows hold one axis");
    h->dfaces = bd->dfaces;
    A3_(h->dvals, nb); A3_(h->bt, 2);
    if (hipMemcpyAsync(h->dvals, bd->dvals, nb * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess ||
        hipStreamSynchronize(h->s) != hipSuccess)
      return bail(fail(GPK_EHIP, "upload of the derivative data failed"));
    const int pl[3][2] = {{1, 2}, {0, 2}, {0, 1}};  // the face plane's axes
    long off = 0;
    for (int a = 0; a < 3; ++a) {
      K3FaceAxis& F = h->face[a];
      F.nk = ns[a]; F.pk = g.p[a];
      F.na = ns[pl[a][0]]; F.nb = ns[pl[a][1]]; F.pa = g.p[pl[a][0]]; F.pb = g.p[pl[a][1]];
      const long fsz = (long)F.na * F.nb;
      for (int s2 = 0; s2 < 2; ++s2) {
        F.on[s2] = (bd->dfaces >> (2 * a + s2)) & 1;
        F.h[s2] = h->dvals + off + s2 * fsz;
        if (F.on[s2]) h->nd += (double)fsz;
      }
      off += 2 * fsz;
      F.A = a == 0 ? h->A1 : a == 1 ? h->A2p : h->A3;
      F.T = a == 0 ? h->T1 : a == 1 ? h->T2p : h->T3;
      if (!F.on[0] && !F.on[1]) continue;
      h->fpart[a] = k3_face_gap_blocks(F, a == 2);
      h->fchunk[a] = k3_face_back_blocks(F, a == 2);
      double *row = nullptr;
      A3_(row, (size_t)2 * F.pk); A3_(F.r, (size_t)2 * F.pa * F.pb);
      A3_(F.part, h->fpart[a]); A3_(F.gv, (size_t)h->fchunk[a] * 2 * F.pk);
      F.gs = F.gv;  // (one block: its partials are the sums)
      if (h->fchunk[a] > 1) A3_(F.gs, (size_t)2 * F.pk);
      F.row = row;
    }
  }
  // convective axes: D1_k, V_k and G_D1k per axis, N, and Q in the layouts those axes read
  // (and D1_k, G_D1k on the axes of a cross pair)
  for (int a = 0; a < 3 && (h->conv || h->cross || h->drift); ++a) {
    if (!deriv_stores_d1(h->mode[a])) continue;
    const int P = g.p[a];
    A3_(h->D1[a], (size_t)P * P); A3_(h->GD1[a], (size_t)P * P);
    if (h->gsq) {  // P_k and Q_k per gradient-active axis; no V_k, Q or Qp on this handle
      if (h->gact[a]) { A3_(h->P[a], np); A3_(h->Qk[a], np); }
      continue;
    }
    if (h->gconv[a] == 0.0) continue;
    A3_(h->V[a], np);
    if (a == 1) { A3_(h->Qp, np); }
    else if (!h->Q) { A3_(h->Q, np); }
  }
  if (h->conv) A3_(h->Nsum, np);
  // cross pairs: per pair H, C, Hb and Zb; Z_1 / Z_2 for the pairs that start from them, and the
  // two copies pair (1,2) goes through
  for (int t = 0; t < 3 && h->cross; ++t) {
    if (h->mx[t] == 0.0) continue;
    A3_(h->Hx[t], np); A3_(h->Cx[t], np); A3_(h->Hb[t], np); A3_(h->Zb[t], np);
    if (t < 2 && !h->Z1) A3_(h->Z1, np);
    if (t == 0) { A3_(h->Z1p, np); A3_(h->Zb12, np); }
    if (t == 2) A3_(h->Z2p, np);
  }
  // bi-pairs: DD_k and G_DDk per axis of a present pair; per pair H2, B, Hb2 and Zb2; Z2_1 / Z2_2 for
  // the pairs that start from them, and the two copies pair (1,2) goes through
  for (int a = 0; a < 3 && h->bi; ++a) {
    if (!deriv_stores_d2(h->mode[a])) continue;
    const int P = g.p[a];
    A3_(h->D2[a], (size_t)P * P); A3_(h->GD2[a], (size_t)P * P);
  }
  for (int t = 0; t < 3 && h->bi; ++t) {
    if (h->bq[t] == 0.0) continue;
    A3_(h->Hq[t], np); A3_(h->Bq[t], np); A3_(h->Hbq[t], np); A3_(h->Zbq[t], np);
    if (t < 2 && !h->Z21) A3_(h->Z21, np);
    if (t == 0) { A3_(h->Z21p, np); A3_(h->Zb212, np); }
    if (t == 2) A3_(h->Z22p, np);
  }
  // drift axes: the field (zero-padded, natural layout), E_k, and Z_k where no pair forms it
  for (int a = 0; a < 3 && h->drift; ++a) {
    if (!dr->b[a]) continue;
    A3_(h->bf[a], np); A3_(h->Ed[a], np);
    h->Zd[a] = a == 0 ? h->Z1 : a == 1 ? h->Z2p : nullptr;
    if (!h->Zd[a]) A3_(h->Zd[a], np);
    std::vector<double> fp(np, 0.0);
    for (int i1 = 0; i1 < ns[0]; ++i1)
      for (int i2 = 0; i2 < ns[1]; ++i2)
        std::memcpy(&fp[g.at(i1, i2, 0)], dr->b[a] + ((size_t)i1 * ns[1] + i2) * ns[2], ns[2] * sizeof(double));
    if (hipMemcpyAsync(h->bf[a], fp.data(), np * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess ||
        hipStreamSynchronize(h->s) != hipSuccess)
      return bail(fail(GPK_EHIP, "upload of a drift field failed"));
  }
#undef A3_
  // upload: coordinates, the padded source, boundary values, the initial params
  // (model_GP_solver_2d.py:245-261: U = 0, freq = linspace(0,1,Q) freq_scale, log-ls = 0,
  // log-w = log(1/Q), log_tau = log_v = 0)
  const double* xs[3] = {p->x1, p->x2, p->x3};
  for (int a = 0; a < 3; ++a)
    if (hipMemcpyAsync(h->x[a], xs[a], ns[a] * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess)
      return bail(fail(GPK_EHIP, "upload x"));
  {
    std::vector<double> Fp(np, 0.0);
    for (int i1 = 0; i1 < ns[0]; ++i1)
      for (int i2 = 0; i2 < ns[1]; ++i2)
        std::memcpy(&Fp[g.at(i1, i2, 0)], p->src + ((size_t)i1 * ns[1] + i2) * ns[2], ns[2] * sizeof(double));
    std::vector<double> init(h->nparams, 0.0);
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < p->q; ++c) {
        init[h->off_kp[a] + c] = p->q > 1 ? (double)c / (p->q - 1) * freq_scale : 0.0;
        init[h->off_kp[a] + 2 * p->q + c] = std::log(1.0 / p->q);
      }
    if (hipMemcpyAsync(h->F, Fp.data(), np * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess ||
        hipMemcpyAsync(h->bvals, p->bvals, nb * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess ||
        hipMemcpyAsync(h->params, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess ||
        hipStreamSynchronize(h->s) != hipSuccess)
      return bail(fail(GPK_EHIP, "upload failed"));
  }
  build_stages(h);
  if (p->flags & GPK_FLAG3_REFINE) {
    build_refine(h);
    if (h->route && refine_panel_prepare() != hipSuccess) return bail(fail(GPK_EHIP, "refine_panel_prepare failed"));
  }
  if (h->cross) build_cross_stages(h);
  if (h->bi) build_bicross_stages(h);
  if (h->drift) build_drift_stages(h);
  *out = h;
  return GPK_OK;
}

// gpk_operator3x as create3 takes it.  One non-zero weight: that order with that weight
// (gpk_create3_op's handle); none: order 2 with weight 0; both: a mixed axis (order 0), its
// weights in the assembled block and 1.0 on its GEMMs
gpk_operator3 one_order_part(const gpk_operator3x* op) {
  gpk_operator3 o{};
  for (int a = 0; a < 3; ++a) {
    const bool has2 = op->c2[a] != 0.0, has1 = op->c1[a] != 0.0;
    o.order[a] = has2 && has1 ? 0 : has1 ? 1 : 2;
    o.coef[a] = has2 && has1 ? 1.0 : has1 ? op->c1[a] : op->c2[a];
    o.react[a] = op->react[a];
  }
  o.faces = op->faces;
  return o;
}

// the arguments of gpk_create3_opx and gpk_create3_opv (`who`), up to the problem's own checks
int check_operator3x(const gpk_problem3* p, const gpk_operator3x* op, gpk_handle3** out, const char* who) {
  if (!p || !op || !out) return fail(GPK_EINVAL, "NULL argument");
  *out = nullptr;
  const std::string w(who);
  if (p->eq != GPK_POISSON)
    return fail(GPK_EINVAL, w + ": eq must be GPK_POISSON (the operator states the equation)");
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(op->c2[a]) || !std::isfinite(op->c1[a]) || !std::isfinite(op->react[a]))
      return fail(GPK_EINVAL, w + ": c2, c1 and react must be finite");
  if (op->faces < 1 || op->faces > K3_ALL_FACES) return fail(GPK_EINVAL, w + ": faces must be in 1..63");
  return GPK_OK;
}

}  // namespace

extern "C" {

int gpk_create3(const gpk_problem3* p, double freq_scale, gpk_handle3** out) {
  if (!p || !out) return fail(GPK_EINVAL, "NULL argument");
  *out = nullptr;
  if (p->eq != GPK_POISSON && p->eq != GPK_ALLENCAHN)
    return fail(GPK_EINVAL, "equation type not supported for the 3-axis solver");
  return create3(p, nullptr, freq_scale, out);
}

int gpk_create3_op(const gpk_problem3* p, const gpk_operator3* op, double freq_scale, gpk_handle3** out) {
  if (!p || !op || !out) return fail(GPK_EINVAL, "NULL argument");
  *out = nullptr;
  if (p->eq != GPK_POISSON)
    return fail(GPK_EINVAL, "gpk_create3_op: eq must be GPK_POISSON (the operator states the equation)");
  for (int a = 0; a < 3; ++a) {
    if (op->order[a] != 1 && op->order[a] != 2)
      return fail(GPK_EINVAL, "gpk_create3_op: derivative order must be 1 or 2");
    if (!std::isfinite(op->coef[a]) || !std::isfinite(op->react[a]))
      return fail(GPK_EINVAL, "gpk_create3_op: coef and react must be finite");
  }
  if (op->faces < 1 || op->faces > K3_ALL_FACES)
    return fail(GPK_EINVAL, "gpk_create3_op: faces must be in 1..63");
  return create3(p, op, freq_scale, out);
}

int gpk_operator_info3(const gpk_handle3* h, gpk_operator3* out) {
  if (!h || !out) return fail(GPK_EINVAL, "NULL argument");
  for (int a = 0; a < 3; ++a)
    if (deriv_weighted(h->mode[a]))
      return fail(GPK_EINVAL, "gpk_operator_info3: the handle has a mixed-order axis (gpk_operator_info3x states it)");
  *out = h->op;
  return GPK_OK;
}

int gpk_create3_opx(const gpk_problem3* p, const gpk_operator3x* op, double freq_scale, gpk_handle3** out) {
  TRY(check_operator3x(p, op, out, "gpk_create3_opx"));
  const gpk_operator3 o = one_order_part(op);
  return create3(p, &o, freq_scale, out, op);
}

int gpk_operator_info3x(const gpk_handle3* h, gpk_operator3x* out) {
  if (!h || !out) return fail(GPK_EINVAL, "NULL argument");
  for (int a = 0; a < 3; ++a) {
    out->c2[a] = h->c2[a];
    out->c1[a] = h->c1[a];
    out->react[a] = h->op.react[a];
  }
  out->faces = h->op.faces;
  return GPK_OK;
}

int gpk_create3_opv(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf, double freq_scale,
                    gpk_handle3** out) {
  const double* given[4] = {cf ? cf->a[0] : nullptr, cf ? cf->a[1] : nullptr, cf ? cf->a[2] : nullptr,
                            cf ? cf->rho : nullptr};
  if (!given[0] && !given[1] && !given[2] && !given[3]) return gpk_create3_opx(p, op, freq_scale, out);
  TRY(check_operator3x(p, op, out, "gpk_create3_opv"));
  TRY(check_problem3(p));  // (the grid's size, before the fields are read)
  const size_t n = (size_t)p->n1 * p->n2 * p->n3;
  for (const double* f : given)
    if (f && !std::all_of(f, f + n, [](double x) { return std::isfinite(x); }))
      return fail(GPK_EINVAL, "gpk_create3_opv: a coefficient field has a non-finite value");
  const gpk_operator3 o = one_order_part(op);
  return create3(p, &o, freq_scale, out, op, cf);
}

}  // extern "C"

namespace {

// gpk_create3_opn with derivative faces, and gpk_create3_opc with a convective axis (cv; bd may
// then be null or without faces): the argument checks of both, then the handle
int create3_opn(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf, const gpk_bdata3* bd,
                const gpk_conv3* cv, double freq_scale, gpk_handle3** out, const gpk_cross3* mx = nullptr,
                const gpk_drift3* dr = nullptr, const gpk_high3* hi = nullptr, const gpk_bicross3* bq = nullptr,
                const gpk_gradsq3* gq = nullptr) {
  if (!p || !op || !out) return fail(GPK_EINVAL, "NULL argument");
  *out = nullptr;
  if (bd && bd->dfaces == 0) bd = nullptr;
  if (bd && (bd->dfaces < 0 || bd->dfaces > K3_ALL_FACES)) return fail(GPK_EINVAL, "gpk_create3_opn: dfaces must be in 0..63");
  if (bd && !bd->dvals) return fail(GPK_EINVAL, "gpk_create3_opn: dvals is NULL with dfaces != 0");
  // the operator's own checks, with faces = 0 allowed here (data on derivatives alone)
  gpk_operator3x o = *op;
  if (bd && o.faces == 0) o.faces = bd->dfaces;
  TRY(check_operator3x(p, &o, out, gq ? "gpk_create3_opg" : bq ? "gpk_create3_opq" : hi ? "gpk_create3_oph" : dr ? "gpk_create3_opb" : mx ? "gpk_create3_opm" : cv ? "gpk_create3_opc" : "gpk_create3_opn"));
  TRY(check_problem3(p));
  if (bd) {
    const long fs[3] = {(long)p->n2 * p->n3, (long)p->n1 * p->n3, (long)p->n1 * p->n2};
    const double* d = bd->dvals;
    for (int f = 0; f < 6; d += fs[f / 2], ++f)
      if (((bd->dfaces >> f) & 1) && !std::all_of(d, d + fs[f / 2], [](double x) { return std::isfinite(x); }))
        return fail(GPK_EINVAL, "gpk_create3_opn: a derivative value on a face of dfaces is not finite");
  }
  const size_t n = (size_t)p->n1 * p->n2 * p->n3;
  const double* given[4] = {cf ? cf->a[0] : nullptr, cf ? cf->a[1] : nullptr, cf ? cf->a[2] : nullptr,
                            cf ? cf->rho : nullptr};
  bool any = false;
  for (const double* f : given) {
    any = any || f;
    if (f && !std::all_of(f, f + n, [](double x) { return std::isfinite(x); }))
      return fail(GPK_EINVAL, "gpk_create3_opn: a coefficient field has a non-finite value");
  }
  for (int a = 0; a < 3 && dr; ++a)
    if (dr->b[a] && !std::all_of(dr->b[a], dr->b[a] + n, [](double x) { return std::isfinite(x); }))
      return fail(GPK_EINVAL, "gpk_create3_opb: a drift field has a non-finite value");
  gpk_operator3 o1 = one_order_part(op);  // (op's own faces: 0 stays 0)
  // a convective axis assembles D_k = c2_k DD_k + c1_k D1_k whatever the weights are: entered as a
  // mixed axis (order 0, GEMM weight 1.0)
  for (int a = 0; a < 3 && cv; ++a)
    if (cv->g[a] != 0.0) { o1.order[a] = 0; o1.coef[a] = 1.0; }
  // and so are both axes of a pair with a cross weight
  if (mx) {
    const bool in[3] = {mx->m[0] != 0.0 || mx->m[1] != 0.0, mx->m[0] != 0.0 || mx->m[2] != 0.0,
                        mx->m[1] != 0.0 || mx->m[2] != 0.0};
    for (int a = 0; a < 3; ++a)
      if (in[a]) { o1.order[a] = 0; o1.coef[a] = 1.0; }
  }
  // and a drift axis
  for (int a = 0; a < 3 && dr; ++a)
    if (dr->b[a]) { o1.order[a] = 0; o1.coef[a] = 1.0; }
  // and a high-order axis
  for (int a = 0; a < 3 && hi; ++a)
    if (hi->c4[a] != 0.0 || hi->c3[a] != 0.0) { o1.order[a] = 0; o1.coef[a] = 1.0; }
  // and both axes of a pair with a bi weight
  if (bq) {
    const bool in[3] = {bq->q[0] != 0.0 || bq->q[1] != 0.0, bq->q[0] != 0.0 || bq->q[2] != 0.0,
                        bq->q[1] != 0.0 || bq->q[2] != 0.0};
    for (int a = 0; a < 3; ++a)
      if (in[a]) { o1.order[a] = 0; o1.coef[a] = 1.0; }
  }
  // and a gradient-active axis
  if (gq) {
    const bool in[3] = {gq->s[0] != 0.0 || gq->x[0] != 0.0 || gq->x[1] != 0.0,
                        gq->s[1] != 0.0 || gq->x[0] != 0.0 || gq->x[2] != 0.0,
                        gq->s[2] != 0.0 || gq->x[1] != 0.0 || gq->x[2] != 0.0};
    for (int a = 0; a < 3; ++a)
      if (in[a]) { o1.order[a] = 0; o1.coef[a] = 1.0; }
  }
  return create3(p, &o1, freq_scale, out, op, any ? cf : nullptr, bd, cv, mx, dr, hi, bq, gq);
}

// the convective weights as gpk_create3_opc and gpk_create3_opm (`who`) take them: GPK_EINVAL on a
// non-finite g_k, and cv becomes null when all three are zero (no convective axis)
int check_conv3(const gpk_conv3*& cv, const char* who) {
  if (!cv) return GPK_OK;
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(cv->g[a])) return fail(GPK_EINVAL, std::string(who) + ": g must be finite");
  if (cv->g[0] == 0.0 && cv->g[1] == 0.0 && cv->g[2] == 0.0) cv = nullptr;
  return GPK_OK;
}

}  // namespace

extern "C" {

int gpk_create3_opn(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf, const gpk_bdata3* bd,
                    double freq_scale, gpk_handle3** out) {
  if (!bd || bd->dfaces == 0) return gpk_create3_opv(p, op, cf, freq_scale, out);
  return create3_opn(p, op, cf, bd, nullptr, freq_scale, out);
}

int gpk_create3_opc(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf, const gpk_bdata3* bd,
                    const gpk_conv3* cv, double freq_scale, gpk_handle3** out) {
  if (cv && out) *out = nullptr;
  TRY(check_conv3(cv, "gpk_create3_opc"));
  if (!cv) return gpk_create3_opn(p, op, cf, bd, freq_scale, out);
  return create3_opn(p, op, cf, bd, cv, freq_scale, out);
}

int gpk_create3_opm(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf, const gpk_bdata3* bd,
                    const gpk_conv3* cv, const gpk_cross3* mx, double freq_scale, gpk_handle3** out) {
  if (mx) {
    if (out) *out = nullptr;
    for (int t = 0; t < 3; ++t)
      if (!std::isfinite(mx->m[t])) return fail(GPK_EINVAL, "gpk_create3_opm: m must be finite");
  }
  if (!mx || (mx->m[0] == 0.0 && mx->m[1] == 0.0 && mx->m[2] == 0.0))
    return gpk_create3_opc(p, op, cf, bd, cv, freq_scale, out);
  TRY(check_conv3(cv, "gpk_create3_opm"));
  return create3_opn(p, op, cf, bd, cv, freq_scale, out, mx);
}

int gpk_create3_opb(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf, const gpk_bdata3* bd,
                    const gpk_conv3* cv, const gpk_cross3* mx, const gpk_drift3* dr, double freq_scale,
                    gpk_handle3** out) {
  if (!dr || (!dr->b[0] && !dr->b[1] && !dr->b[2])) return gpk_create3_opm(p, op, cf, bd, cv, mx, freq_scale, out);
  if (out) *out = nullptr;
  if (mx) {
    for (int t = 0; t < 3; ++t)
      if (!std::isfinite(mx->m[t])) return fail(GPK_EINVAL, "gpk_create3_opb: m must be finite");
    if (mx->m[0] == 0.0 && mx->m[1] == 0.0 && mx->m[2] == 0.0) mx = nullptr;
  }
  TRY(check_conv3(cv, "gpk_create3_opb"));
  return create3_opn(p, op, cf, bd, cv, freq_scale, out, mx, dr);
}

int gpk_create3_oph(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf, const gpk_bdata3* bd,
                    const gpk_conv3* cv, const gpk_cross3* mx, const gpk_drift3* dr, const gpk_high3* hi,
                    double freq_scale, gpk_handle3** out) {
  bool any = false;
  if (hi) {
    if (out) *out = nullptr;
    for (int a = 0; a < 3; ++a) {
      if (!std::isfinite(hi->c4[a]) || !std::isfinite(hi->c3[a]))
        return fail(GPK_EINVAL, "gpk_create3_oph: c4 and c3 must be finite");
      any = any || hi->c4[a] != 0.0 || hi->c3[a] != 0.0;
    }
  }
  if (!any) return gpk_create3_opb(p, op, cf, bd, cv, mx, dr, freq_scale, out);
  if (mx) {
    for (int t = 0; t < 3; ++t)
      if (!std::isfinite(mx->m[t])) return fail(GPK_EINVAL, "gpk_create3_oph: m must be finite");
    if (mx->m[0] == 0.0 && mx->m[1] == 0.0 && mx->m[2] == 0.0) mx = nullptr;
  }
  TRY(check_conv3(cv, "gpk_create3_oph"));
  if (dr && !dr->b[0] && !dr->b[1] && !dr->b[2]) dr = nullptr;
  return create3_opn(p, op, cf, bd, cv, freq_scale, out, mx, dr, hi);
}

int gpk_create3_opq(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf, const gpk_bdata3* bd,
                    const gpk_conv3* cv, const gpk_cross3* mx, const gpk_drift3* dr, const gpk_high3* hi,
                    const gpk_bicross3* bq, double freq_scale, gpk_handle3** out) {
  if (bq) {
    if (out) *out = nullptr;
    for (int t = 0; t < 3; ++t)
      if (!std::isfinite(bq->q[t])) return fail(GPK_EINVAL, "gpk_create3_opq: q must be finite");
  }
  if (!bq || (bq->q[0] == 0.0 && bq->q[1] == 0.0 && bq->q[2] == 0.0))
    return gpk_create3_oph(p, op, cf, bd, cv, mx, dr, hi, freq_scale, out);
  if (hi) {
    bool any = false;
    for (int a = 0; a < 3; ++a) {
      if (!std::isfinite(hi->c4[a]) || !std::isfinite(hi->c3[a]))
        return fail(GPK_EINVAL, "gpk_create3_opq: c4 and c3 must be finite");
      any = any || hi->c4[a] != 0.0 || hi->c3[a] != 0.0;
    }
    if (!any) hi = nullptr;
  }
  if (mx) {
    for (int t = 0; t < 3; ++t)
      if (!std::isfinite(mx->m[t])) return fail(GPK_EINVAL, "gpk_create3_opq: m must be finite");
    if (mx->m[0] == 0.0 && mx->m[1] == 0.0 && mx->m[2] == 0.0) mx = nullptr;
  }
  TRY(check_conv3(cv, "gpk_create3_opq"));
  if (dr && !dr->b[0] && !dr->b[1] && !dr->b[2]) dr = nullptr;
  return create3_opn(p, op, cf, bd, cv, freq_scale, out, mx, dr, hi, bq);
}

int gpk_create3_opg(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf, const gpk_bdata3* bd,
                    const gpk_conv3* cv, const gpk_cross3* mx, const gpk_drift3* dr, const gpk_high3* hi,
                    const gpk_bicross3* bq, const gpk_gradsq3* gq, double freq_scale, gpk_handle3** out) {
  bool any = false;
  if (gq) {
    if (out) *out = nullptr;
    for (int t = 0; t < 3; ++t) {
      if (!std::isfinite(gq->s[t]) || !std::isfinite(gq->x[t]))
        return fail(GPK_EINVAL, "gpk_create3_opg: s and x must be finite");
      any = any || gq->s[t] != 0.0 || gq->x[t] != 0.0;
    }
  }
  if (!any) return gpk_create3_opq(p, op, cf, bd, cv, mx, dr, hi, bq, freq_scale, out);
  if (bq) {
    for (int t = 0; t < 3; ++t)
      if (!std::isfinite(bq->q[t])) return fail(GPK_EINVAL, "gpk_create3_opg: q must be finite");
    if (bq->q[0] == 0.0 && bq->q[1] == 0.0 && bq->q[2] == 0.0) bq = nullptr;
  }
  if (hi) {
    bool anyh = false;
    for (int a = 0; a < 3; ++a) {
      if (!std::isfinite(hi->c4[a]) || !std::isfinite(hi->c3[a]))
        return fail(GPK_EINVAL, "gpk_create3_opg: c4 and c3 must be finite");
      anyh = anyh || hi->c4[a] != 0.0 || hi->c3[a] != 0.0;
    }
    if (!anyh) hi = nullptr;
  }
  if (mx) {
    for (int t = 0; t < 3; ++t)
      if (!std::isfinite(mx->m[t])) return fail(GPK_EINVAL, "gpk_create3_opg: m must be finite");
    if (mx->m[0] == 0.0 && mx->m[1] == 0.0 && mx->m[2] == 0.0) mx = nullptr;
  }
  TRY(check_conv3(cv, "gpk_create3_opg"));
  if (dr && !dr->b[0] && !dr->b[1] && !dr->b[2]) dr = nullptr;
  return create3_opn(p, op, cf, bd, cv, freq_scale, out, mx, dr, hi, bq, gq);
}

int gpk_gradsq_info3(const gpk_handle3* h, double s[3], double x[3]) {
  if (!h || !s || !x) return fail(GPK_EINVAL, "NULL argument");
  for (int t = 0; t < 3; ++t) {
    s[t] = h->gs[t];
    x[t] = h->gx[t];
  }
  return GPK_OK;
}

int gpk_bicross_info3(const gpk_handle3* h, double q[3]) {
  if (!h || !q) return fail(GPK_EINVAL, "NULL argument");
  for (int t = 0; t < 3; ++t) q[t] = h->bq[t];
  return GPK_OK;
}

int gpk_high_info3(const gpk_handle3* h, double c4[3], double c3[3]) {
  if (!h || !c4 || !c3) return fail(GPK_EINVAL, "NULL argument");
  for (int a = 0; a < 3; ++a) {
    c4[a] = h->c4[a];
    c3[a] = h->c3[a];
  }
  return GPK_OK;
}

int gpk_drift_info3(const gpk_handle3* h, int32_t has[3]) {
  if (!h || !has) return fail(GPK_EINVAL, "NULL argument");
  for (int a = 0; a < 3; ++a) has[a] = h->bf[a] != nullptr;
  return GPK_OK;
}

int gpk_cross_info3(const gpk_handle3* h, double m[3]) {
  if (!h || !m) return fail(GPK_EINVAL, "NULL argument");
  for (int t = 0; t < 3; ++t) m[t] = h->mx[t];
  return GPK_OK;
}

int gpk_conv_info3(const gpk_handle3* h, double g[3]) {
  if (!h || !g) return fail(GPK_EINVAL, "NULL argument");
  for (int a = 0; a < 3; ++a) g[a] = h->gconv[a];
  return GPK_OK;
}

int gpk_bdata_info3(const gpk_handle3* h, int32_t* faces, int32_t* dfaces) {
  if (!h || !faces || !dfaces) return fail(GPK_EINVAL, "NULL argument");
  *faces = h->op.faces;
  *dfaces = h->dfaces;
  return GPK_OK;
}

int gpk_coef_info3(const gpk_handle3* h, int32_t has[4]) {
  if (!h || !has) return fail(GPK_EINVAL, "NULL argument");
  for (int a = 0; a < 3; ++a) has[a] = h->cf[a] != nullptr;
  has[3] = h->rho != nullptr;
  return GPK_OK;
}

int gpk_num_params3(const gpk_handle3* h, int64_t* n) {
  if (!h || !n) return fail(GPK_EINVAL, "NULL argument");
  *n = h->nparams;
  return GPK_OK;
}

int gpk_set_params3(gpk_handle3* h, const double* flat, int64_t n) {
  if (!h || !flat) return fail(GPK_EINVAL, "NULL argument");
  if (n != h->nparams) return fail(GPK_EINVAL, "flat parameter vector has the wrong length");
  DevSwitch ds(h->dev);
  HIPCHK(hipMemcpyAsync(h->params, flat, n * sizeof(double), hipMemcpyHostToDevice, h->s));
  TRY(check_launch(k3_launch_sync_u(h->params, 0, h->g, h->Up, h->s), "k3_sync_u"));
  HIPCHK(hipStreamSynchronize(h->s));
  return GPK_OK;
}

int gpk_get_params3(gpk_handle3* h, double* flat, int64_t n) {
  if (!h || !flat) return fail(GPK_EINVAL, "NULL argument");
  if (n != h->nparams) return fail(GPK_EINVAL, "flat parameter vector has the wrong length");
  DevSwitch ds(h->dev);
  HIPCHK(hipMemcpyAsync(flat, h->params, n * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  return GPK_OK;
}

int gpk_loss_grad3(gpk_handle3* h, double* loss, double* grad_flat) {
  if (!h || !loss) return fail(GPK_EINVAL, "NULL argument");
  DevSwitch ds(h->dev);
  TRY(capture3(h, 0));
  HIPCHK(hipMemsetAsync(h->loss_slot, 0, sizeof(int), h->s));
  HIPCHK(hipGraphLaunch(h->exec[0], h->s));
  TRY(read_status3(h));
  double diag[8];
  TRY(read_diag3(h, diag));
  *loss = diag[0];
  if (grad_flat) HIPCHK(hipMemcpy(grad_flat, h->grad, h->nparams * sizeof(double), hipMemcpyDeviceToHost));
  return GPK_OK;
}

int gpk_step3(gpk_handle3* h, int32_t n_steps, double* losses) {
  if (!h) return fail(GPK_EINVAL, "NULL handle");
  if (n_steps < 0 || n_steps > K3_LOSS_CAP) return fail(GPK_EINVAL, "n_steps must be in [0, 4096]");
  DevSwitch ds(h->dev);
  TRY(capture3(h, 1));
  HIPCHK(hipMemsetAsync(h->loss_slot, 0, sizeof(int), h->s));
  for (int i = 0; i < n_steps; ++i) HIPCHK(hipGraphLaunch(h->exec[1], h->s));
  TRY(read_status3(h));
  if (losses && n_steps > 0)
    HIPCHK(hipMemcpy(losses, h->losses, n_steps * sizeof(double), hipMemcpyDeviceToHost));
  return GPK_OK;
}

int gpk_set_opt_state3(gpk_handle3* h, int64_t count, const double* mu, const double* nu, int64_t n) {
  if (!h || !mu || !nu) return fail(GPK_EINVAL, "NULL argument");
  if (n != h->nparams) return fail(GPK_EINVAL, "parameter count mismatch");
  if (count < 0 || count > 0x7fffffff) return fail(GPK_EINVAL, "bad count");
  DevSwitch ds(h->dev);
  const int c = (int)count;
  HIPCHK(hipMemcpyAsync(h->m, mu, n * sizeof(double), hipMemcpyHostToDevice, h->s));
  HIPCHK(hipMemcpyAsync(h->v, nu, n * sizeof(double), hipMemcpyHostToDevice, h->s));
  HIPCHK(hipMemcpyAsync(h->count, &c, sizeof(int), hipMemcpyHostToDevice, h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  return GPK_OK;
}

int gpk_get_opt_state3(gpk_handle3* h, int64_t* count, double* mu, double* nu, int64_t n) {
  if (!h || !count || !mu || !nu) return fail(GPK_EINVAL, "NULL argument");
  if (n != h->nparams) return fail(GPK_EINVAL, "parameter count mismatch");
  DevSwitch ds(h->dev);
  int c = 0;
  HIPCHK(hipMemcpyAsync(mu, h->m, n * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipMemcpyAsync(nu, h->v, n * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipMemcpyAsync(&c, h->count, sizeof(int), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  *count = c;
  return GPK_OK;
}

int gpk_criterion3(gpk_handle3* h, double* out) {
  if (!h || !out) return fail(GPK_EINVAL, "NULL argument");
  double loss;
  TRY(gpk_loss_grad3(h, &loss, nullptr));
  DevSwitch ds(h->dev);
  double diag[8];
  TRY(read_diag3(h, diag));
  const double n1 = h->g.n[0], n2 = h->g.n[1], n3 = h->g.n[2];
  const double fs[3] = {n2 * n3, n1 * n3, n1 * n2}, Nc = n1 * n2 * n3;
  double Nb = 0.0;  // the active faces' entries
  for (int f = 0; f < 6; ++f)
    if ((h->op.faces >> f) & 1) Nb += fs[f / 2];
  Nb += h->nd;  // (+ the derivative faces', whose gap diag[6] includes)
  *out = diag[6] / Nb + diag[5] / Nc;  // boundary_gap/Nb + eq_gap/Nc (K3Final::diag)
  return GPK_OK;
}

int gpk_boundary_terms3(gpk_handle3* h, double out[4]) {
  if (!h || !out) return fail(GPK_EINVAL, "NULL argument");
  DevSwitch ds(h->dev);
  HIPCHK(hipStreamSynchronize(h->s));
  const double n1 = h->g.n[0], n2 = h->g.n[1], n3 = h->g.n[2];
  const double fs[3] = {n2 * n3, n1 * n3, n1 * n2};
  out[2] = 0.0;
  for (int f = 0; f < 6; ++f)
    if ((h->op.faces >> f) & 1) out[2] += fs[f / 2];
  out[3] = h->nd;
  if (h->dfaces) {
    HIPCHK(hipMemcpy(out, h->bt, 2 * sizeof(double), hipMemcpyDeviceToHost));
  } else {
    double diag[8];
    TRY(read_diag3(h, diag));
    out[0] = diag[6];
    out[1] = 0.0;
  }
  return GPK_OK;
}

int gpk_stage_variants3(gpk_handle3* h, int32_t* out, int32_t cap, int32_t* n) {
  if (!h || !n || cap < 0 || (cap && !out)) return fail(GPK_EINVAL, "NULL argument");
  // stream order: a convective handle's two further launches follow stages 2 and 3; a cross
  // handle's eight follow those (three, four) and the last stage (one); a drift handle's Z_k launch
  // (if any) follows the convective handle's first, its other two the cross handle's after stage 3
  std::vector<const std::vector<GemmDesc>*> order;
  for (size_t k = 0; k < h->stages.size(); ++k) {
    order.push_back(&h->stages[k]);
    if (h->conv && (k == 2 || k == 3)) order.push_back(&h->cstages[k - 2]);
    if (h->drift && k == 2 && !h->dstages[0].empty()) order.push_back(&h->dstages[0]);
    if (h->cross && k == 2) for (int i = 0; i < 3; ++i) order.push_back(&h->xs.st[i]);
    if (h->bi && k == 2) for (int i = 0; i < 3; ++i) order.push_back(&h->qs.st[i]);
    if (h->cross && k == 3) for (int i = 3; i < 7; ++i) order.push_back(&h->xs.st[i]);
    if (h->bi && k == 3) for (int i = 3; i < 7; ++i) order.push_back(&h->qs.st[i]);
    if (h->drift && k == 3) for (int i = 1; i < 3; ++i) order.push_back(&h->dstages[i]);
  }
  if (h->cross) order.push_back(&h->xs.st[7]);
  if (h->bi) order.push_back(&h->qs.st[7]);
  *n = (int32_t)order.size();
  for (int k = 0; k < *n && k < cap; ++k) out[k] = stage_variant(*order[k]);
  return GPK_OK;
}

int gpk_refine_info3(gpk_handle3* h, double bound[3], int32_t open[3], int32_t* route) {
  if (!h || !bound || !open || !route) return fail(GPK_EINVAL, "NULL argument");
  if (h->rstages.empty())
    return fail(GPK_EINVAL, "gpk_refine_info3: the handle was created without GPK_FLAG3_REFINE");
  DevSwitch ds(h->dev);
  HIPCHK(hipStreamSynchronize(h->s));
  for (int a = 0; a < 3; ++a) {
    double pst[2];  // K_00, bits of max diag K^{-1} (gate_open)
    HIPCHK(hipMemcpy(pst, h->pst[a], sizeof(pst), hipMemcpyDeviceToHost));
    bound[a] = pst[0] * pst[1];
    open[a] = bound[a] > REFINE_COND_LB;
  }
  *route = h->route;
  return GPK_OK;
}

int gpk_loss_terms3(gpk_handle3* h, double out[7]) {
  if (!h || !out) return fail(GPK_EINVAL, "NULL argument");
  DevSwitch ds(h->dev);
  HIPCHK(hipStreamSynchronize(h->s));
  double diag[8];
  TRY(read_diag3(h, diag));
  std::copy(diag, diag + 7, out);
  return GPK_OK;
}

}  // extern "C"

namespace {

// K_k with jitter into Kc (the sweeps overwrote the assembled one): the refinement residuals'
// operand of gpk_predict3 and gpk_evaluate3
int cross_kc(gpk_handle3* h, int a, double* Kc) {
  const K3Geom& g = h->g;
  return check_launch(launch_cross(h->prob.kind, h->q, h->x[a], g.n[a], h->x[a], g.n[a], g.p[a], h->kc + a,
                                   h->prob.jitter, 0, Kc, nullptr, h->s), "cross");
}

// Kmn_a^(d) = the d-th derivative of kappa in its first argument at (xt_i, x_a,j), no jitter,
// into the zero-filled block Kmn (leading dimension p_a).  Order 0 is launch_cross's K output;
// above it Kmn takes the D output and K goes to Kd.
int cross_kmn(gpk_handle3* h, int a, const double* xt, int m, int d, double* Kmn, double* Kd) {
  const K3Geom& g = h->g;
  return check_launch(launch_cross(h->prob.kind, h->q, xt, m, h->x[a], g.n[a], g.p[a], h->kc + a, 0.0, d,
                                   d ? Kd : Kmn, d ? Kmn : nullptr, h->s), "cross");
}

struct Solver3 {  // the refined solves of the prediction routes against the call's Kc
  gpk_handle3* h;
  double* const* Kc;
  // X = K_a^{-1} B (a = 0, K on the left) or B K_a^{-1} (a = 2), rows x cols, residual scratch Wr
  int solve(int a, const double* B, double* X, double* Wr, int rows, int cols) const {
    const RefinedSolve s = refined_solve(a == 2, Kc[a], h->Kinv[a], B, X, Wr, rows, cols, nullptr);
    TRY(launch_descs(h, {s.solve}));
    TRY(launch_descs(h, {s.resid}));
    return launch_descs(h, {s.fix});
  }
  // C = alpha A x_2 B + beta C0 over nb slabs of [P2][P3] (A: M x P2)
  int slab(const double* A, int M, const double* B, double* C, double alpha, double beta, const double* C0,
           int nb) const {
    const int P2 = h->g.p[1], P3 = h->g.p[2];
    SlabGemm sg{};
    sg.A = A; sg.B = B; sg.sB = (size_t)P2 * P3; sg.C = C; sg.sC = (size_t)M * P3; sg.C0 = C0; sg.sC0 = sg.sC;
    sg.M = M; sg.N = P3; sg.K = P2; sg.nb = nb; sg.alpha = alpha; sg.beta = beta;
    return check_launch(launch_gemm_slab(sg, h->s), "gemm_slab");
  }
  int slab_solve(const double* B, double* X, double* Wr, int nb) const {
    const int P2 = h->g.p[1];
    TRY(slab(h->Kinv[1], P2, B, X, 1.0, 0.0, nullptr, nb));
    TRY(slab(Kc[1], P2, X, Wr, -1.0, 1.0, B, nb));
    return slab(h->Kinv[1], P2, Wr, X, 1.0, 1.0, X, nb);
  }
};

// gpk_predict3 / gpk_predict_deriv3: the d-th derivatives of the interpolant on a test grid
int predict3_impl(gpk_handle3* h, const double* const xte[3], const int ms[3], const int d[3], double* out) {
  if (!h || !xte[0] || !xte[1] || !xte[2] || !out) return fail(GPK_EINVAL, "NULL argument");
  for (int a = 0; a < 3; ++a) {
    if (ms[a] < 1 || ms[a] > K3_MAX_N) return fail(GPK_EINVAL, "need 1..1024 test points per axis");
    if (d[a] < 0 || d[a] > 2) return fail(GPK_EINVAL, "derivative order must be 0, 1 or 2");
  }
  const int m1 = ms[0], m2 = ms[1], m3 = ms[2];
  DevSwitch ds(h->dev);
  const K3Geom& g = h->g;
  const int P1 = g.p[0], P2 = g.p[1], P3 = g.p[2];
  const int M1p = pad_up(m1), M2p = pad_up(m2), M3p = pad_up(m3);
  const int Mp[3] = {M1p, M2p, M3p};
  // scratch, allocated per call: test coordinates, Kmn_k (zero-padded to Mp_k x P_k), K_k again
  // (the sweeps overwrote it) and three work tensors W that take every intermediate in turn
  CallScratch tmp("gpk_predict3", h->s);
  const size_t N1 = (size_t)P2 * P3, R3 = (size_t)M1p * M2p;
  const size_t big = std::max(std::max((size_t)P1 * N1, (size_t)M1p * N1),
                              std::max(R3 * P3, R3 * M3p));
  double *xt[3], *Kmn[3], *Kc[3], *W[3], *Kd[3] = {};
  for (int a = 0; a < 3; ++a) {
    TRY(tmp.alloc(&xt[a], ms[a], true));
    TRY(tmp.alloc(&Kmn[a], (size_t)Mp[a] * g.p[a], true));
    TRY(tmp.alloc(&Kc[a], (size_t)g.p[a] * g.p[a], true));
    TRY(tmp.alloc(&W[a], big, true));
  }
  for (int a = 0; a < 3; ++a)
    if (d[a]) TRY(tmp.alloc(&Kd[a], (size_t)Mp[a] * g.p[a]));
  for (int a = 0; a < 3; ++a)
    if (hipMemcpyAsync(xt[a], xte[a], ms[a] * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess)
      return fail(GPK_EHIP, "gpk_predict3: upload of the test coordinates failed");
  // K_k^{-1} at the current params (the step's own front), then Kmn_k = kappa^(d_k)(xte_k, x_k)
  // without jitter and K_k with it, for the refinement residuals
  TRY(enqueue_inverse3(h, 0));
  for (int a = 0; a < 3; ++a) {
    TRY(cross_kmn(h, a, xt[a], ms[a], d[a], Kmn[a], Kd[a]));
    TRY(cross_kc(h, a, Kc[a]));
  }
  // T <- Kmn_k x_k solve(K_k, T) for k = 1, 2, 3 from T = U (the reference's 2-axis association,
  // model_GP_solver_2d.py:185-220, axis after axis: every intermediate stays O(|U_pred|)); each
  // solve is A = K^{-1} T, A += K^{-1} (T - K A).  Modes 1 and 3 are GEMMs on the row-major
  // unfoldings; mode 2 of [B][P2][P3] is B slabs of P2 x P3 (launch_gemm_slab: no permuted copy).
  const Solver3 sv{h, Kc};
  const int n1 = (int)N1, r3 = (int)R3;
  TRY(sv.solve(0, h->Up, W[0], W[1], P1, n1));
  TRY(launch_descs(h, {gemm_desc(Kmn[0], P1, 0, W[0], n1, 0, W[1], n1, M1p, n1, P1)}));  // [M1p][P2][P3]
  TRY(sv.slab_solve(W[1], W[0], W[2], M1p));
  TRY(sv.slab(Kmn[1], M2p, W[0], W[1], 1.0, 0.0, nullptr, M1p));                         // [M1p][M2p][P3]
  TRY(sv.solve(2, W[1], W[0], W[2], r3, P3));
  TRY(launch_descs(h, {gemm_desc(W[0], P3, 0, Kmn[2], P3, 1, W[2], M3p, r3, M3p, P3)}));  // [M1p][M2p][M3p]
  for (int i1 = 0; i1 < m1; ++i1)
    if (hipMemcpy2DAsync(out + (size_t)i1 * m2 * m3, m3 * sizeof(double), W[2] + (size_t)i1 * M2p * M3p,
                         M3p * sizeof(double), m3 * sizeof(double), m2, hipMemcpyDeviceToHost, h->s) != hipSuccess)
      return fail(GPK_EHIP, "gpk_predict3: download failed");
  const hipError_t e = hipStreamSynchronize(h->s);
  if (e != hipSuccess) return fail(GPK_EHIP, std::string("gpk_predict3: ") + hipGetErrorString(e));
  return read_status3(h);
}

}  // namespace

extern "C" {

int gpk_predict3(gpk_handle3* h, const double* xte1, int32_t m1, const double* xte2, int32_t m2,
                 const double* xte3, int32_t m3, double* out) {
  const double* const xte[3] = {xte1, xte2, xte3};
  const int ms[3] = {m1, m2, m3}, d[3] = {0, 0, 0};
  return predict3_impl(h, xte, ms, d, out);
}

int gpk_predict_deriv3(gpk_handle3* h, const double* xte1, int32_t m1, const double* xte2, int32_t m2,
                       const double* xte3, int32_t m3, const int32_t d[3], double* out) {
  if (!d) return fail(GPK_EINVAL, "NULL argument");
  const double* const xte[3] = {xte1, xte2, xte3};
  const int ms[3] = {m1, m2, m3}, dd[3] = {d[0], d[1], d[2]};
  return predict3_impl(h, xte, ms, dd, out);
}

// The same quantity at m scattered points, per point in gpk_predict3's association: with
// A1 = K1^{-1} x_1 U (once per call), per chunk of at most EVAL_CHUNK3 points
//   B = Kmn1^(d1) x_1 A1 [M][P2][P3] -> slab solve with K2 -> point contraction over axis 2 with
//   kappa2^(d2)(y_p, .) [M][P3] -> right solve with K3 -> point contraction with kappa3^(d3)(z_p, .)
// No Kmn2 / Kmn3 and no M x M (x M) product.  Each chunk ends in its download and a stream wait,
// so the host staging vectors can be refilled.
int gpk_evaluate3(gpk_handle3* h, const double* pts, int64_t m, const int32_t d[3], double* out) {
  if (!h || !pts || !d || !out) return fail(GPK_EINVAL, "NULL argument");
  if (m < 1) return fail(GPK_EINVAL, "need at least one point");
  for (int a = 0; a < 3; ++a)
    if (d[a] < 0 || d[a] > 2) return fail(GPK_EINVAL, "derivative order must be 0, 1 or 2");
  DevSwitch ds(h->dev);
  const K3Geom& g = h->g;
  const int P1 = g.p[0], P2 = g.p[1], P3 = g.p[2], kind = h->prob.kind;
  const size_t N1 = (size_t)P2 * P3;
  const int chunk = (int)std::min<int64_t>(m, eval3_chunk(N1)), Cp = pad_up(chunk);
  CallScratch tmp("gpk_evaluate3", h->s);
  double *dp[3], *Kc[3], *A1, *WA, *Kmn1, *Kd = nullptr, *W[3], *G, *Nw, *Rn, *res;
  for (int a = 0; a < 3; ++a) {
    TRY(tmp.alloc(&dp[a], chunk));
    TRY(tmp.alloc(&Kc[a], (size_t)g.p[a] * g.p[a], true));
  }
  TRY(tmp.alloc(&A1, (size_t)P1 * N1, true));
  TRY(tmp.alloc(&WA, (size_t)P1 * N1, true));
  TRY(tmp.alloc(&Kmn1, (size_t)Cp * P1));
  if (d[0]) TRY(tmp.alloc(&Kd, (size_t)Cp * P1));
  for (int a = 0; a < 3; ++a) TRY(tmp.alloc(&W[a], (size_t)Cp * N1, true));
  for (double** w : {&G, &Nw, &Rn}) TRY(tmp.alloc(w, (size_t)Cp * P3, true));
  TRY(tmp.alloc(&res, chunk));
  TRY(enqueue_inverse3(h, 0));
  for (int a = 0; a < 3; ++a) TRY(cross_kc(h, a, Kc[a]));
  const Solver3 sv{h, Kc};
  const int n1 = (int)N1;
  TRY(sv.solve(0, h->Up, A1, WA, P1, n1));
  std::vector<double> hp[3];
  for (auto& v : hp) v.resize(chunk);
  for (int64_t k = 0; k < chunk_count(m, chunk); ++k) {
    const int64_t p0 = chunk_begin(k, chunk);
    const int mc = chunk_size(m, k, chunk), mcp = pad_up(mc);
    for (int i = 0; i < mc; ++i)
      for (int a = 0; a < 3; ++a) hp[a][i] = pts[(size_t)(p0 + i) * 3 + a];
    for (int a = 0; a < 3; ++a)
      HIPCHK(hipMemcpyAsync(dp[a], hp[a].data(), mc * sizeof(double), hipMemcpyHostToDevice, h->s));
    // Kmn1^(d1) of the chunk, its padding rows zero (so are those of every product below); G's
    // padding rows are not written by the contraction, so they are cleared as well
    HIPCHK(hipMemsetAsync(Kmn1, 0, (size_t)mcp * P1 * sizeof(double), h->s));
    HIPCHK(hipMemsetAsync(G, 0, (size_t)mcp * P3 * sizeof(double), h->s));
    TRY(cross_kmn(h, 0, dp[0], mc, d[0], Kmn1, Kd));
    TRY(launch_descs(h, {gemm_desc(Kmn1, P1, 0, A1, n1, 0, W[0], n1, mcp, n1, P1)}));  // [mcp][P2][P3]
    TRY(sv.slab_solve(W[0], W[1], W[2], mcp));
    PointContract pc{};
    pc.t = dp[1]; pc.m = mc; pc.x = h->x[1]; pc.n = g.n[1]; pc.kc = h->kc + 1; pc.q = h->q;
    pc.T = W[1]; pc.sp = N1; pc.sj = (size_t)P3; pc.sc = 1; pc.C = P3; pc.out = G;       // [mcp][P3]
    TRY(check_launch(launch_point_contract(kind, d[1], pc, h->s), "point_contract"));
    TRY(sv.solve(2, G, Nw, Rn, mcp, P3));
    pc.t = dp[2]; pc.x = h->x[2]; pc.n = g.n[2]; pc.kc = h->kc + 2;
    pc.T = Nw; pc.sp = (size_t)P3; pc.sj = 1; pc.C = 1; pc.out = res;
    TRY(check_launch(launch_point_contract(kind, d[2], pc, h->s), "point_contract"));
    HIPCHK(hipMemcpyAsync(out + p0, res, mc * sizeof(double), hipMemcpyDeviceToHost, h->s));
    const hipError_t e = hipStreamSynchronize(h->s);
    if (e != hipSuccess) return fail(GPK_EHIP, std::string("gpk_evaluate3: ") + hipGetErrorString(e));
  }
  return read_status3(h);
}

}  // extern "C"

