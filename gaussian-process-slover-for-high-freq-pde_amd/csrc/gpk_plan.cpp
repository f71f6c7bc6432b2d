// gpk_plan.cpp — the 2D step's GEMM plan: the descriptor helpers every host unit builds its
// products with, and build_descs, which lays out the stages gpk_step.cpp launches (and
// gpk_shard.cpp slices by rows).
#include "gpk_host.h"

GemmDesc gemm_desc(const double* A, int lda, int ta, const double* B, int ldb, int tb, double* C,
                   int ldc, int M, int N, int K) {
  GemmDesc g{};
  g.A = A; g.lda = lda; g.ta = ta; g.B = B; g.ldb = ldb; g.tb = tb;
  g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.alpha = 1.0; g.epi = EPI_STORE;
  return g;
}

GemmDesc with_side(GemmDesc g, double* Y, const double* Ys, int ldy) {  // Y = Ys / 2 + v C
  g.Y = Y; g.Ys = Ys; g.ldy = ldy;
  return g;
}

RefinedSolve refined_solve(bool right, const double* Kc, const double* Kinv, const double* B, double* X,
                           double* W, int rows, int cols, const double* gate) {
  const int P = right ? cols : rows;
  auto prod = [&](const double* Km, const double* T, double* C) {
    return right ? gemm_desc(T, cols, 0, Km, P, 0, C, cols, rows, cols, P)
                 : gemm_desc(Km, P, 0, T, cols, 0, C, cols, rows, cols, P);
  };
  RefinedSolve s{prod(Kinv, B, X), prod(Kc, X, W), prod(Kinv, W, X)};
  s.resid.alpha = -1.0; s.resid.beta = 1.0; s.resid.C0 = B; s.resid.ldc0 = cols; s.resid.gate = gate;
  s.fix.beta = 1.0; s.fix.C0 = X; s.fix.ldc0 = cols; s.fix.gate = gate;
  return s;
}

RefinePanel refine_panel_desc(bool right, const double* Kc, const double* Kinv, const double* B, double* X,
                              int rows, int cols, const double* gate) {
  RefinePanel f{};
  f.Kinv = Kinv; f.Kc = Kc; f.B = B; f.X = X; f.right = right; f.gate = gate;
  f.P = right ? cols : rows; f.M = right ? rows : cols;
  f.sp = right ? 1 : (size_t)cols; f.sc = right ? (size_t)cols : 1;
  return f;
}

int gemm_force(int flags) {
  return (flags & GPK_FLAG_FORCE_HUGE_GEMM) ? 2 : (flags & GPK_FLAG_FORCE_BIG_GEMM) ? 1 : 0;
}

int build_descs(gpk_handle* h) {
  const Layout& L = h->L;
  const int P1 = L.p1, P2 = L.p2;
  const double beta = (h->prob.eq == GPK_ADVECTION) ? h->prob.beta : 1.0;
  const int ac = h->prob.eq == GPK_ALLENCAHN;
  std::vector<GemmDesc> d;
  auto begin = [&](int k) { h->st[k].off = (int)d.size(); };
  const int force_big = gemm_force(h->prob.flags);
  auto end = [&](int k) {
    h->st[k].n = (int)d.size() - h->st[k].off;
    for (int i = h->st[k].off; i < (int)d.size(); ++i) d[i].tag = k;
    h->st[k].gated = h->st[k].n > 0;
    for (int i = h->st[k].off; i < (int)d.size(); ++i) h->st[k].gated &= d[i].gate != nullptr;
    h->st[k].variant = gemm_variant(d.data() + h->st[k].off, h->st[k].n, force_big);
  };
  // Every solve against K (JAX: LU solves, model_GP_solver_2d.py:104-105 and the reverse
  // pass) is X = K^{-1} B (MFMA) plus one refinement X += K^{-1}(B - K X), whose two GEMMs are
  // gated on a lower bound of cond(K) (refine_gate_open) (skipped when K is well conditioned, e.g. 256^2).
  const int n1 = L.n1, n2 = L.n2;
  // Refinement GEMMs (X += K^{-1}(B - K X)) are gated on device on a lower bound of cond(K): a
  // closed gate ends each of their workgroups before any load (a launch).  Small factors: every
  // solve is refined.  Large 2D factors (P >= 1600), where each refinement is two N^3 GEMMs
  // (C5: ~2.2 ms each), by default the FORWARD solves A = K1^{-1} U and Bt = U K2^{-1}: the
  // residual R = beta D1 A + Bt D2^T - F differentiates them (D amplifies the unstructured
  // error of an explicit-inverse product) and ||R||^2 feeds the loss and the log_v gradient;
  // GPK_FLAG_REFINE_ALL adds S and X1 / X2, GPK_FLAG_NO_REFINE drops all (round 2's path).
  // Accuracy of each choice against the long-double yardstick: tests/test_gpu_accuracy.py,
  // profiles/r3_parity.json, DESIGN.md §5.
  const int rfl = h->prob.flags;
  const bool ref_fwd = !(rfl & GPK_FLAG_NO_REFINE);
  const bool ref_rev = (!h->bigspd || (rfl & GPK_FLAG_REFINE_ALL)) && !(rfl & GPK_FLAG_NO_REFINE);
  // Large 2D factors, the axis-2 forward solve Bt = U K2^{-1} (round 6): it enters the residual
  // R = beta D1 A + Bt D2^T - F with weight 1 against beta for A, so at beta >= 16 (advection;
  // C5: beta = 200) refining A alone leaves R's error ~1/beta of the unrefined one.  Measured at
  // C5 against the exact-field yardstick (tools/c5_refine_diag.py, profiles/r6_c5_refine_fwd1.txt):
  // log_v (||R||^2) 3.3e-12 with A refined alone, 1.1e-12 with both, 8.3e-9 with neither (the LU
  // oracle: 2.9e-10); every other key within 0.3x of the LU oracle's distance either way -- and
  // the step 37.3 -> 33.5 ms (two 4096^3 products fewer).  GPK_FLAG_REFINE_ALL refines both.
  const bool ref_fwd2 = ref_fwd && !(rfl & GPK_FLAG_REFINE_FWD1_ONLY) &&
                        (!h->bigspd || beta < 16.0 || (rfl & GPK_FLAG_REFINE_ALL));
  bool ref_now = ref_fwd;
  auto pushg = [&](const GemmDesc& g) {
    if (ref_now) d.push_back(g);
  };
  // X1 / X2 producers also write Y = S/2 + v X (GemmDesc::Y): G_K's left operand
  auto side = [&](GemmDesc g, double* Y) { return with_side(g, Y, h->S, P2); };
  // the step's five solves (refined_solve): K1 on the left, K2 on the right, P1 x P2 operands
  auto solve = [&](int a, const double* B, double* X, double* W) {
    return refined_solve(a == 1, h->Kc[a], h->Kinv[a], B, X, W, P1, P2, h->pst[a]);
  };
  const RefinedSolve sA = solve(0, h->Up, h->A, h->W1), sBt = solve(1, h->Up, h->Bt, h->W2),
                     sS = solve(1, h->A, h->S, h->W1), sX1 = solve(0, h->T1, h->X1, h->W1),
                     sX2 = solve(1, h->T2, h->X2, h->W2);
  // Stage A: A = K1^{-1} U, Bt = U K2^{-1}                       (2d.py:104-105)
  // (augmented chain: both come out of the inverse launch itself -- no stage)
  begin(0);
  if (!h->chain_aug) {
    d.push_back(sA.solve);
    d.push_back(sBt.solve);
  }
  end(0);
  // (Measured in C4's training regime, tools/train_regime_parity.py, profiles/r5_train_regime_
  // parity.json: with the gate closed -- cond(K) <= 1.4e3, bound < 21 -- the unrefined step is
  // within 0.45 of the parity bar on its own K and D after 200-2000 Adam steps; refining the
  // forward solves every step took that to 0.05-0.25 for ~12 us per step, so the gate stays.)
  begin(1);  // residuals W1 = U - K1 A, W2 = U - Bt K2
  pushg(sA.resid);
  if (ref_fwd2) pushg(sBt.resid);
  end(1);
  begin(2);  // A += K1^{-1} W1, Bt += W2 K2^{-1}  (in place)
  pushg(sA.fix);
  if (ref_fwd2) pushg(sBt.fix);
  end(2);
  // Stage B: S = A K2^{-1};  R = beta D1 A + Bt D2^T - F (+AC), ||R||^2 and the prior's
  // quadratic term sum(A * Bt) (2d.py:112-143, :161) from the same tile loop
  begin(3);
  {
    d.push_back(sS.solve);
    GemmDesc r = gemm_desc(h->D[0], P1, 0, h->A, P2, 0, h->R, P2, P1, P2, P1);
    r.alpha = beta;
    r.A2 = h->Bt; r.lda2 = P2; r.ta2 = 0; r.B2 = h->D[1]; r.ldb2 = P2; r.tb2 = 1; r.K2 = P2;
    r.alpha2 = 1.0;
    r.epi = EPI_RESID; r.F = h->F; r.U = h->Up; r.ldf = P2; r.ac = ac; r.red = h->red_egap;
    r.red2 = h->red_quad; r.Q1 = h->A; r.Q2 = h->Bt;
    d.push_back(r);
  }
  end(3);
  ref_now = ref_rev;  // (the reverse-pass solves from here on)
  begin(4);  // W1 = A - S K2
  pushg(sS.resid);
  end(4);
  begin(5);  // S += W1 K2^{-1}
  pushg(sS.fix);
  end(5);
  // Stage C: T1 = beta D1^T R, T2 = R D2, G_D1 = v beta R A^T, G_D2 = v R^T Bt  (Appendix A)
  // (augmented chain: X1 = beta (K1^{-1} D1^T) R and X2 = R (K2^{-1} D2^T)^T directly, from the
  // inverse launch's K^{-1} D^T -- stage D's solves fold into this stage)
  begin(6);
  if (h->chain_aug) {
    GemmDesc x1 = gemm_desc(h->PD[0], P1, 0, h->R, P2, 0, h->X1, P2, P1, P2, P1);
    x1.alpha = beta;
    d.push_back(side(x1, h->Y1));
    d.push_back(side(gemm_desc(h->R, P2, 0, h->PD[1], P2, 1, h->X2, P2, P1, P2, P2), h->Y2));
  } else {
    GemmDesc t1 = gemm_desc(h->D[0], P1, 1, h->R, P2, 0, h->T1, P2, P1, P2, P1);
    t1.alpha = beta;
    d.push_back(t1);
    d.push_back(gemm_desc(h->R, P2, 0, h->D[1], P2, 0, h->T2, P2, P1, P2, P2));
  }
  {
    GemmDesc g = gemm_desc(h->R, P2, 0, h->A, P2, 1, h->GD[0], P1, P1, P1, P2);
    g.alpha = beta; g.vscale = 1;
    d.push_back(g);
    GemmDesc g2 = gemm_desc(h->R, P2, 1, h->Bt, P2, 0, h->GD[1], P2, P2, P2, P1);
    g2.vscale = 1;
    d.push_back(g2);
  }
  end(6);
  // Stage D: X1 = K1^{-1} T1, X2 = T2 K2^{-1} (refined)
  begin(7);
  if (!h->chain_aug) {
    d.push_back(side(sX1.solve, h->Y1));
    d.push_back(side(sX2.solve, h->Y2));
  }
  end(7);
  begin(8);  // refinement residuals W1 = beta D1^T R - K1 X1, W2 = R D2 - X2 K2
  if (h->chain_aug) {  // (T1, T2 never formed: dual products, not the solves' own residual form)
    GemmDesc g = gemm_desc(h->D[0], P1, 1, h->R, P2, 0, h->W1, P2, P1, P2, P1);
    g.alpha = beta;
    g.A2 = h->Kc[0]; g.lda2 = P1; g.B2 = h->X1; g.ldb2 = P2; g.K2 = P1; g.alpha2 = -1.0;
    g.gate = h->pst[0];
    pushg(g);
    GemmDesc g2 = gemm_desc(h->R, P2, 0, h->D[1], P2, 0, h->W2, P2, P1, P2, P2);
    g2.A2 = h->X2; g2.lda2 = P2; g2.B2 = h->Kc[1]; g2.ldb2 = P2; g2.K2 = P2; g2.alpha2 = -1.0;
    g2.gate = h->pst[1];
    pushg(g2);
  } else {
    pushg(sX1.resid);
    pushg(sX2.resid);
  }
  end(8);
  begin(9);  // X1 += K1^{-1} W1, X2 += W2 K2^{-1}, Y rewritten from the refined X
  pushg(side(sX1.fix, h->Y1));
  pushg(side(sX2.fix, h->Y2));
  end(9);
  // Stage E: G_K1 = c N2/2 K1^{-1} - Y1 A^T;  G_K2 = c N1/2 K2^{-1} - Y2^T Bt, with
  // Y = S/2 + v X written by the X producers above (one product each instead of two)
  begin(10);
  {
    GemmDesc g = gemm_desc(h->Y1, P2, 0, h->A, P2, 1, h->GK[0], P1, P1, P1, P2);
    g.alpha = -1.0;
    g.beta = 0.5 * h->prob.logdet * n2; g.C0 = h->Kinv[0]; g.ldc0 = P1;
    d.push_back(g);
    GemmDesc g2 = gemm_desc(h->Y2, P2, 1, h->Bt, P2, 0, h->GK[1], P2, P2, P2, P1);
    g2.alpha = -1.0;
    g2.beta = 0.5 * h->prob.logdet * n1; g2.C0 = h->Kinv[1]; g2.ldc0 = P2;
    d.push_back(g2);
  }
  end(10);
  // class tile partials (GemmDesc::cpart) from the G_D (stage C) and G_K (stage E) epilogues
  // when both stages run the 16x16-tile kernel (its epilogue forms them)
  h->cp_on = h->cpK[0] && h->st[6].variant == GEMM_SMALL && h->st[10].variant == GEMM_SMALL;
  if (h->cp_on) {
    for (int k : {6, 10})
      for (int i = h->st[k].off; i < h->st[k].off + h->st[k].n; ++i)
        for (int a = 0; a < 2; ++a) {
          GemmDesc& g = d[i];
          if (g.C != (k == 6 ? h->GD[a] : h->GK[a])) continue;
          g.cpart = k == 6 ? h->cpD[a] : h->cpK[a];
          g.bcid = h->cls[a].cid;
          g.bcbase = h->cls[a].cbase;
          g.bn = axis_n(L, a);
          g.bncls = h->cls[a].ncls;
          g.bsx = (k == 6 && h->prob.eq == GPK_ADVECTION) ? axis_x(h, a) : nullptr;
        }
  }
  {  // the residual descriptor of stage B carries the egap / quad partials: one per tile
    int nq = 0;
    for (int i = h->st[3].off; i < h->st[3].off + h->st[3].n; ++i)
      if (d[i].red) nq = gemm_tiles(d[i], h->st[3].variant);
    h->nquad = h->negap = nq;
  }
  for (int k = 0; k < kGemmStages; ++k)
    if (h->st[k].n > GEMM_MAX_BATCH) return fail(GPK_EINVAL, "internal: GEMM stage batch too large");
  h->hdescs = d;
  return GPK_OK;
}
