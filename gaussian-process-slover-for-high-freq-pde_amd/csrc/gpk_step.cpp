// gpk_step.cpp — the log-joint step of a handle: its argument fillers and enqueue, the 2D GEMM
// plan (build_descs), graph capture, the batch begin / report / rollback protocol, and the entry
// points that run it (gpk_step, gpk_prepare, gpk_loss_grad).  The row-sharded enqueue is in
// gpk_shard.cpp; handle construction in gpk_create.cpp.
#include <sched.h>

#include <atomic>

#include "gpk_host.h"

namespace {
const char* kStageNames1D[] = {"prep", "assemble", "spd_inverse", "gemv_alpha", "gemv_alpha_res",
                               "gemv_alpha_fix", "gemv_resid", "gemv_DtR", "gemv_beta",
                               "gemv_beta_res", "gemv_beta_fix", "pgrad_tail"};
const char* kStageNames2D[] = {"prep", "assemble", "spd_inverse", "gemm_A", "gemm_A_res",
                               "gemm_A_fix", "gemm_B", "gemm_B_res", "gemm_B_fix", "gemm_C",
                               "gemm_D", "gemm_D_res", "gemm_D_fix", "gemm_E", "pgrad_tail"};
}  // namespace

static void mark(gpk_handle* h, int stage) {
  if (h->profiling) (void)hipEventRecord(h->ev[stage + 1], h->s);
}

// ------------------------------------------------------------------------------------------
// the step, in stream order
// ------------------------------------------------------------------------------------------
PrepArgs make_prep(gpk_handle* h, int apply) {
  const Layout& L = h->L;
  PrepArgs P{};
  P.params = h->params;
  P.off_kp[0] = L.off_kp[0];
  P.off_kp[1] = L.off_kp[1];
  P.off_tau = L.off_tau;
  P.off_v = L.off_v;
  P.naxes = L.naxes;
  P.has_cos = (h->prob.kind == GPK_SE_COS || h->prob.kind == GPK_MATERN52_COS) ? 1 : 0;
  P.kc = h->kc;
  P.sc = h->sc;
  P.count = h->count;
  P.apply = apply;
  P.b1 = h->hyper.b1;
  P.b2 = h->hyper.b2;
  P.Up = h->Up; P.bvals = h->bvals; P.bidx = h->bidx; P.nb = h->prob.nb;
  P.dim = L.dim; P.n1 = L.n1; P.n2 = L.n2; P.p2 = L.p2;
  P.bgap = h->bgap;
  P.bgap_parts = h->bgap_parts;
  P.nce_flag = h->nce_flag;
  return P;
}

// Pipelined class values (gpk.h GPK_FLAG_NO_CLASS_PIPE): chain-inverse handles with distance
// classes, unsharded -- the class-value launch is then the step's only user of the kernel
// parameters before the inverse, so it can run at the end of the previous step's parameter-
// gradient launch, which has just updated them.
bool cls_pipe_ok(const gpk_handle* h) {
  return !h->shard && h->chain && h->cls[0].ncls > 0 && h->nce_flag &&
         !(h->prob.flags & GPK_FLAG_NO_CLASS_PIPE);
}

void fill_spd(gpk_handle* h, SpdArgs* sa) {
  const Layout& L = h->L;
  for (int a = 0; a < L.naxes; ++a) {
    sa[a] = SpdArgs{};
    sa[a].X = h->K[a];
    sa[a].Y = h->Kb[a];
    sa[a].p = axis_p(L, a);
    sa[a].n = axis_n(L, a);
    sa[a].piv = h->piv[a];
    sa[a].ldet = h->ldet[a];
    sa[a].status = h->status;
    sa[a].pst = h->pst[a];
    sa[a].flag = h->aflag[a];
    sa[a].wide = h->bigwide ? 1 : 0;
    sa[a].no_quarters = (h->prob.flags & GPK_FLAG_NO_QUARTER_TILES) ? 1 : 0;
    sa[a].qfirst = (h->prob.flags & GPK_FLAG_NO_QUARTER_FIRST) ? 0 : 1;
    sa[a].Z = h->Zp[a];
    sa[a].sched = h->wsched[a];
    sa[a].sched_paired = (h->prob.flags & GPK_FLAG_ONE_SWEEP_UPDATE) ? 0 : 1;
  }
}

// the persistent small-factor inverse; gather: K (+ Kc, D) straight from the distance classes
hipError_t launch_chain(gpk_handle* h, bool gather, double** fin, bool aug, const PrepArgs* prep) {
  const Layout& L = h->L;
  ChainArgs ca[2] = {};
  for (int a = 0; a < L.naxes; ++a) {
    ChainArgs& c = ca[a];
    c.X = h->K[a]; c.PB = h->Kb[a]; c.piv = h->piv[a]; c.ldet = h->ldet[a]; c.pst = h->pst[a];
    c.status = h->status; c.flags = h->cflags[a]; c.gran = h->cgran[a];
    c.PB2 = h->PB2[a]; c.epoch = h->cepoch[a];
    c.lookahead = (h->prob.flags & GPK_FLAG_NO_CHAIN_LOOKAHEAD) ? 0 : 1;
    c.p = axis_p(L, a);
    c.n = axis_n(L, a);
    if (gather) {
      c.cid = h->cls[a].cid; c.kval = h->cls[a].kval; c.dval = h->cls[a].dval;
      c.x = axis_x(h, a); c.jitter = h->prob.jitter; c.Kc = h->Kc[a];
    }
    c.D = h->D[a];  // gather: written; read mode: the augmented D^T columns read it
    if (gather && h->cls_gemv) c.Kc = c.D = nullptr;  // (the GEMVs read them as classes)
    if (h->chain_aug && aug) {  // axis 0: [U | D1^T] -> A, K1^{-1} D1^T;  axis 1: [U^T | D2^T] -> Bt^T, P2
      c.tu = axis_p(L, 1 - a) / 32; c.td = c.p / 32;
      c.Bu = h->Up; c.ldbu = L.p2; c.bu_t = a;
      c.Ou = a ? h->Bt : h->A; c.ldou = L.p2; c.ou_t = a;
      c.Od = h->PD[a]; c.ldod = c.p;
      c.PBa = h->PBa[a]; c.ldpba = L.p1 + L.p2;
    }
    fin[a] = h->K[a];
  }
  if (h->chain_multi) return launch_spd_chain_multi(ca, L.naxes, step_deriv(h), h->s, prep, L.q);
  return launch_spd_chain(ca, L.naxes, step_deriv(h), h->s, prep, L.q);
}

// the SPD inverse of every factor (small: 32-wide sweeps, pivot 0 possibly fused into the
// assembly launch; large: 64-wide panel/update sweeps)
hipError_t launch_inverse(gpk_handle* h, SpdArgs* sa, double** fin, bool pivot0_done) {
  if (h->bigspd) return launch_spd_inverse_big(sa, h->L.naxes, fin, h->s);
  if (h->chain) return launch_chain(h, false, fin, false);  // K^{-1} only (timing, predict)
  return launch_spd_inverse(sa, h->L.naxes, fin, h->s, pivot0_done);
}

// the assembly arguments every caller shares: coordinates, sizes, constants, K and D outputs
void fill_assemble(const gpk_handle* h, AssembleArgs* aa) {
  for (int a = 0; a < h->L.naxes; ++a) {
    aa[a] = AssembleArgs{};
    aa[a].x = axis_x(h, a);
    aa[a].n = axis_n(h->L, a);
    aa[a].p = axis_p(h->L, a);
    aa[a].kc = h->kc + a;
    aa[a].jitter = h->prob.jitter;
    aa[a].K = h->K[a];
    aa[a].D = h->D[a];
    aa[a].deriv = step_deriv(h);
  }
}

// the 2D parameter-contraction arguments every caller shares (no low parts, no class partials)
void fill_pgrad2d(const gpk_handle* h, PGradArgs* pa) {
  for (int a = 0; a < 2; ++a) {
    pa[a] = PGradArgs{};
    pa[a].x = axis_x(h, a);
    pa[a].n = axis_n(h->L, a);
    pa[a].p = axis_p(h->L, a);
    pa[a].kc = h->kc + a;
    pa[a].GK = h->GK[a];
    pa[a].GD = h->GD[a];
    pa[a].deriv = step_deriv(h);
    pa[a].part = h->pgpart + (size_t)a * h->bpa * 3 * QMAX;
    pa[a].cls = h->cls[a];
  }
}

// assemble K, D (+ step constants, + pivot block 0) and invert K: the first part of a step
int enqueue_assemble_inverse(gpk_handle* h, int apply, bool have_cls) {
  const Layout& L = h->L;
  AssembleArgs aa[2] = {};
  fill_assemble(h, aa);
  // the step alone keeps K (refinement residuals), reads the distance classes, and fuses pivot 0
  for (int a = 0; a < L.naxes; ++a) {
    aa[a].Kc = h->Kc[a];
    aa[a].cls = h->cls[a];
    if (!h->bigspd && !h->chain) {  // pivot block 0 factored inside the assembly launch
      aa[a].piv = h->piv[a];
      aa[a].ldet = h->ldet[a];
      aa[a].pst = h->pst[a];
      aa[a].status = h->status;
      aa[a].flag = h->aflag[a];
    }
  }
  // chain + classes: the class values only; the inverse launch gathers K, Kc, D itself and
  // publishes the step constants from one extra workgroup (off the critical path)
  const bool eval_only = h->chain && h->cls[0].ncls > 0;
  PrepArgs prep = make_prep(h, apply), prep_eval = prep;
  prep_eval.skip = eval_only ? 1 : 0;
  if (eval_only && h->fold_begin) {  // the batch begin rides on the chain launch's prep row
    const StepBegin& b = *h->fold_begin;
    prep.snap = b.snap; prep.snap_m = b.m; prep.snap_v = b.v; prep.snap_np = b.np;
    prep.snap_count = b.snap ? b.snap_count : nullptr;
    prep.viol0 = b.viol; prep.slot0 = b.loss_slot;
    h->fold_begin = nullptr;
  }
  // (have_cls: the previous step's parameter-gradient launch evaluated them, cls_pipe_ok)
  if (!(eval_only && have_cls))
    TRY(check_launch(launch_assemble(h->prob.kind, L.q, aa, L.naxes, prep_eval, h->s, eval_only),
                     "assemble"));
  mark(h, 1);
  SpdArgs sa[2];
  fill_spd(h, sa);
  double* fin[2] = {nullptr, nullptr};
  if (h->chain) {
    TRY(check_launch(launch_chain(h, eval_only, fin, true, eval_only ? &prep : nullptr), "spd_chain"));
  } else if (h->split_axis >= 0) {
    // one factor per rank group: invert this rank's factor, then every factor's K^{-1}, log-det
    // blocks and refinement gate from its group's first rank (the other factor's buffers on
    // this rank are overwritten; the sweep path's output buffer is fixed per factor size)
    const int a = h->split_axis;
    double* f1[1] = {nullptr};
    if (h->bigspd)
      TRY(check_launch(launch_spd_inverse_big(sa + a, 1, f1, h->s), "spd_inverse"));
    else
      TRY(check_launch(launch_spd_inverse(sa + a, 1, f1, h->s, true), "spd_inverse"));
    TRY(split_broadcast(h));
    for (int b = 0; b < L.naxes; ++b) fin[b] = h->Kinv[b];
  } else {
    TRY(check_launch(launch_inverse(h, sa, fin, true), "spd_inverse"));
  }
  for (int a = 0; a < L.naxes; ++a) h->Kinv[a] = fin[a];
  mark(h, 2);
  return GPK_OK;
}

// the step tail (loss, small-parameter Adam, dL/dU + Adam on U) fused into the pgrad launch
TailArgs make_tail(gpk_handle* h, int apply, bool refine) {
  const Layout& L = h->L;
  const int ac = h->prob.eq == GPK_ALLENCAHN;
  TailArgs T{};
  T.fused = 1;
  FinalizeArgs& f = T.fin;
  f.L = L; f.hyper = h->hyper; f.llk_weight = h->prob.llk_weight; f.logdet = h->prob.logdet;
  f.apply = apply; f.has_cos = kind_cos(h->prob.kind);
  f.red_quad = h->red_quad; f.nquad = h->nquad; f.red_egap = h->red_egap; f.negap = h->negap;
  for (int a = 0; a < L.naxes; ++a) { f.ldet[a] = h->ldet[a]; f.nldet[a] = h->nldet[a]; }
  f.pg = h->pg; f.kc = h->kc; f.sc = h->sc; f.Up = h->Up; f.bvals = h->bvals;
  f.bidx = h->bidx; f.nb = h->prob.nb;
  f.params = h->params; f.grad = h->grad; f.m = h->m; f.v = h->v;
  f.losses = h->losses; f.loss_slot = h->loss_slot; f.diag = h->diag;
  f.bgap = h->bgap;
  f.bgap_parts = h->bgap_parts;
  if (!refine) {  // fast graph: check that no refinement was needed
    for (int a = 0; a < L.naxes; ++a) f.watch[a] = h->pst[a];
    f.viol = h->viol;
  }
  if (h->fold_report) {
    f.report = 1;
    f.rep = *h->fold_report;
    h->fold_report = nullptr;
  }
  AdamUArgs& au = T.adam;
  au.L = L; au.hyper = h->hyper; au.llk_weight = h->prob.llk_weight; au.apply = apply; au.ac = ac;
  au.sc = h->sc; au.Up = h->Up; au.bvals = h->bvals; au.bidx = h->bidx; au.nb = h->prob.nb;
  au.params = h->params; au.grad = h->grad; au.m = h->m; au.v = h->v;
  if (L.dim == 2) { au.S = h->S; au.X1 = h->X1; au.X2 = h->X2; au.R = h->R; }
  else { au.S = nullptr; au.X1 = h->alpha; au.X2 = h->beta; au.R = h->R; au.U0 = h->uoff; }
  T.gcount = h->tcount; T.top = h->ttop; T.gpart = h->tgpart; T.pg = h->pg;
  T.tg = h->ttg; T.ngpa = h->tngpa;
  T.gpart_lo = h->pg_dd ? h->tgpart_lo : nullptr;
  // the fused tail's Adam block forms pg from the group partials itself (the sharded path's
  // standalone finalize reads pg: enqueue_step_shard clears these)
  f.gpart = T.gpart; f.gpart_lo = T.gpart_lo; f.ngpa = T.ngpa; f.pg_out = h->pg;
  if (h->cls_next && cls_pipe_ok(h)) {  // the next step's class values, after the Adam
    T.nce_flag = h->nce_flag;
    T.nce_status = h->status;
    f.kp_wt = h->nce_kp;
  }
  return T;
}

// A GEMV operand that is Kc or D of axis 0: as class ids + class values on a cls_gemv handle
void gemv_operand(const gpk_handle* h, GemvDesc& g) {
  if (!h->cls_gemv || !(g.A == h->Kc[0] || g.A == h->D[0])) return;
  const bool k = g.A == h->Kc[0];
  g.cid = h->cls[0].cid;
  g.cv = k ? h->cls[0].kval : h->cls[0].dval;
  g.cdiag = k ? h->prob.jitter : 0.0;
  g.ident = k ? 1 : 0;
  g.A = nullptr;
}

hipError_t launch_gemm_stage(gpk_handle* h, int k) {
  return launch_gemm_auto(h->hdescs.data() + h->st[k].off, h->st[k].n, h->sc, h->s, h->st[k].variant);
}

int enqueue_step(gpk_handle* h, int apply, bool refine) {
  if (h->shard) return enqueue_step_shard(h, apply);
  const Layout& L = h->L;
  // pipelined class values: this step's were evaluated by the previous step (have); this step
  // evaluates the next one's when its caller asked for it (cls_next, make_tail)
  const bool have = h->cls_have && cls_pipe_ok(h);
  h->cls_have = false;
  if (h->profiling) (void)hipEventRecord(h->ev[0], h->s);
  mark(h, 0);  // "prep" is fused into the assembly launch (stage kept for the name table)
  TRY(enqueue_assemble_inverse(h, apply, have));
  int stage = 3;
  const char* const* names = L.dim == 2 ? kStageNames2D : kStageNames1D;
  for (int k = 0; k < 3; ++k) h->sname[k] = names[k];
  auto stamp = [&](const char* nm) {  // a launched stage: its name and end event
    if (stage < kMaxStages) {
      h->sname[stage] = nm;
      mark(h, stage++);
    }
  };
  const int ac = h->prob.eq == GPK_ALLENCAHN;
  if (L.dim == 2) {
    for (int k = 0; k < kGemmStages; ++k) {
      if (h->st[k].n == 0 || (!refine && h->st[k].gated)) continue;
      TRY(check_launch(launch_gemm_stage(h, k), "gemm"));
      stamp(kStageNames2D[3 + k]);
    }
    PGradArgs pa[2];
    fill_pgrad2d(h, pa);
    // the unsharded step alone has the double-double low parts (pg_dd) and the class partials
    // its own GEMM epilogues wrote (cp_on)
    for (int a = 0; a < 2; ++a) {
      pa[a].part_lo = h->pg_dd ? h->pgpart_lo + (size_t)a * h->bpa * 3 * QMAX : nullptr;
      if (h->cp_on) {
        pa[a].cpK = h->cpK[a];
        pa[a].cpD = h->cpD[a];
        pa[a].cslots = class_slots(pa[a].p / 16);
      }
    }
    TailArgs tail = make_tail(h, apply, refine);
    TRY(check_launch(launch_pgrad(h->prob.kind, L.q, 0, pa, 2, h->bpa, h->sc, h->s, &tail), "pgrad"));
    h->cls_have = tail.nce_flag != nullptr;
    stamp("pgrad_tail");
  } else {
    const int P = L.p1;
    // every K^{-1} application gets one step of iterative refinement x += K^{-1}(b - K x),
    // gated on a cond(K) lower bound (gemv skips itself when K is well conditioned)
    GemvDesc g{};
    g.lda = P; g.p = P; g.rows = P; g.alpha = 1.0; g.ac = ac; g.F = h->F; g.U = h->Up; g.U0 = h->uoff;
    auto gemv = [&](const char* nm, const double* A, const double* x, double* y, double alpha,
                    const double* C0, double beta, int epi, double* red, bool gated) -> int {
      if (gated && !refine) return GPK_OK;
      GemvDesc q = g;
      q.A = A; q.x = x; q.y = y; q.alpha = alpha; q.C0 = C0; q.beta = beta; q.epi = epi; q.red = red;
      q.gate = gated ? h->pst[0] : nullptr;
      gemv_operand(h, q);
      TRY(check_launch(launch_gemv(q, h->s), "gemv"));
      stamp(nm);
      return GPK_OK;
    };
    // alpha = K^{-1} u (refined), quad = <u, alpha>          (model_GP_solver_1d.py:92,137)
    TRY(gemv("gemv_alpha", h->Kinv[0], h->Up, h->alpha, 1.0, nullptr, 0.0, EPI_STORE, nullptr, false));
    TRY(gemv("gemv_alpha_res", h->Kc[0], h->alpha, h->rvec, -1.0, h->Up, 1.0, EPI_STORE, nullptr, true));
    TRY(gemv("gemv_alpha_fix", h->Kinv[0], h->rvec, h->alpha, 1.0, h->alpha, 1.0, EPI_STORE, nullptr, true));
    // R = D alpha - f (+u(u^2-1)): egap = ||R||^2 and quad = <u, alpha> in one pass
    {
      GemvDesc q = g;
      q.A = h->D[0]; q.x = h->alpha; q.y = h->R; q.epi = EPI_RESID; q.red = h->red_egap;
      q.red2 = h->red_quad; q.Q1 = h->Up; q.Q2 = h->alpha;
      gemv_operand(h, q);
      TRY(check_launch(launch_gemv(q, h->s), "gemv"));
      stamp("gemv_resid");
    }
    // t = D^T R (DD_x1 is bitwise symmetric, so D^T = D)
    TRY(gemv("gemv_DtR", h->D[0], h->R, h->tvec, 1.0, nullptr, 0.0, EPI_STORE, nullptr, false));
    // beta = K^{-1} t (refined)
    TRY(gemv("gemv_beta", h->Kinv[0], h->tvec, h->beta, 1.0, nullptr, 0.0, EPI_STORE, nullptr, false));
    TRY(gemv("gemv_beta_res", h->Kc[0], h->beta, h->rvec, -1.0, h->tvec, 1.0, EPI_STORE, nullptr, true));
    TRY(gemv("gemv_beta_fix", h->Kinv[0], h->rvec, h->beta, 1.0, h->beta, 1.0, EPI_STORE, nullptr, true));
    PGradArgs pa{};
    pa.x = h->x1; pa.n = L.n1; pa.p = P; pa.kc = h->kc;
    pa.Kinv = h->Kinv[0]; pa.alpha = h->alpha; pa.beta = h->beta; pa.R = h->R;
    pa.halfc = 0.5 * h->prob.logdet; pa.deriv = 2; pa.part = h->pgpart; pa.cls = h->cls[0];
    pa.part_lo = h->pg_dd ? h->pgpart_lo : nullptr;
    TailArgs tail = make_tail(h, apply, refine);
    TRY(check_launch(launch_pgrad(h->prob.kind, L.q, 1, &pa, 1, h->bpa, h->sc, h->s, &tail), "pgrad"));
    h->cls_have = tail.nce_flag != nullptr;
    stamp("pgrad_tail");
  }
  h->nstage = stage;
  return GPK_OK;
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
  auto mk = [](const double* A, int lda, int ta, const double* B, int ldb, int tb, double* C,
               int ldc, int M, int N, int K) {
    GemmDesc g{};
    g.A = A; g.lda = lda; g.ta = ta; g.B = B; g.ldb = ldb; g.tb = tb;
    g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.alpha = 1.0; g.epi = EPI_STORE;
    return g;
  };
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
  auto gate = [&](GemmDesc g, int axis) {
    g.gate = h->pst[axis];
    return g;
  };
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
  auto side = [&](GemmDesc g, double* Y) {
    g.Y = Y; g.Ys = h->S; g.ldy = P2;
    return g;
  };
  // Stage A: A = K1^{-1} U, Bt = U K2^{-1}                       (2d.py:104-105)
  // (augmented chain: both come out of the inverse launch itself -- no stage)
  begin(0);
  if (!h->chain_aug) {
    d.push_back(mk(h->Kinv[0], P1, 0, h->Up, P2, 0, h->A, P2, P1, P2, P1));
    d.push_back(mk(h->Up, P2, 0, h->Kinv[1], P2, 0, h->Bt, P2, P1, P2, P2));
  }
  end(0);
  // (Measured in C4's training regime, tools/train_regime_parity.py, profiles/r5_train_regime_
  // parity.json: with the gate closed -- cond(K) <= 1.4e3, bound < 21 -- the unrefined step is
  // within 0.45 of the parity bar on its own K and D after 200-2000 Adam steps; refining the
  // forward solves every step took that to 0.05-0.25 for ~12 us per step, so the gate stays.)
  begin(1);  // residuals W1 = U - K1 A, W2 = U - Bt K2
  {
    GemmDesc g = mk(h->Kc[0], P1, 0, h->A, P2, 0, h->W1, P2, P1, P2, P1);
    g.alpha = -1.0; g.beta = 1.0; g.C0 = h->Up; g.ldc0 = P2;
    pushg(gate(g, 0));
    GemmDesc g2 = mk(h->Bt, P2, 0, h->Kc[1], P2, 0, h->W2, P2, P1, P2, P2);
    g2.alpha = -1.0; g2.beta = 1.0; g2.C0 = h->Up; g2.ldc0 = P2;
    if (ref_fwd2) pushg(gate(g2, 1));
  }
  end(1);
  begin(2);  // A += K1^{-1} W1, Bt += W2 K2^{-1}  (in place)
  {
    GemmDesc g = mk(h->Kinv[0], P1, 0, h->W1, P2, 0, h->A, P2, P1, P2, P1);
    g.beta = 1.0; g.C0 = h->A; g.ldc0 = P2;
    pushg(gate(g, 0));
    GemmDesc g2 = mk(h->W2, P2, 0, h->Kinv[1], P2, 0, h->Bt, P2, P1, P2, P2);
    g2.beta = 1.0; g2.C0 = h->Bt; g2.ldc0 = P2;
    if (ref_fwd2) pushg(gate(g2, 1));
  }
  end(2);
  // Stage B: S = A K2^{-1};  R = beta D1 A + Bt D2^T - F (+AC), ||R||^2 and the prior's
  // quadratic term sum(A * Bt) (2d.py:112-143, :161) from the same tile loop
  begin(3);
  {
    d.push_back(mk(h->A, P2, 0, h->Kinv[1], P2, 0, h->S, P2, P1, P2, P2));
    GemmDesc r = mk(h->D[0], P1, 0, h->A, P2, 0, h->R, P2, P1, P2, P1);
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
  {
    GemmDesc g = mk(h->S, P2, 0, h->Kc[1], P2, 0, h->W1, P2, P1, P2, P2);
    g.alpha = -1.0; g.beta = 1.0; g.C0 = h->A; g.ldc0 = P2;
    pushg(gate(g, 1));
  }
  end(4);
  begin(5);  // S += W1 K2^{-1}
  {
    GemmDesc g = mk(h->W1, P2, 0, h->Kinv[1], P2, 0, h->S, P2, P1, P2, P2);
    g.beta = 1.0; g.C0 = h->S; g.ldc0 = P2;
    pushg(gate(g, 1));
  }
  end(5);
  // Stage C: T1 = beta D1^T R, T2 = R D2, G_D1 = v beta R A^T, G_D2 = v R^T Bt  (Appendix A)
  // (augmented chain: X1 = beta (K1^{-1} D1^T) R and X2 = R (K2^{-1} D2^T)^T directly, from the
  // inverse launch's K^{-1} D^T -- stage D's solves fold into this stage)
  begin(6);
  if (h->chain_aug) {
    GemmDesc x1 = mk(h->PD[0], P1, 0, h->R, P2, 0, h->X1, P2, P1, P2, P1);
    x1.alpha = beta;
    d.push_back(side(x1, h->Y1));
    d.push_back(side(mk(h->R, P2, 0, h->PD[1], P2, 1, h->X2, P2, P1, P2, P2), h->Y2));
  } else {
    GemmDesc t1 = mk(h->D[0], P1, 1, h->R, P2, 0, h->T1, P2, P1, P2, P1);
    t1.alpha = beta;
    d.push_back(t1);
    d.push_back(mk(h->R, P2, 0, h->D[1], P2, 0, h->T2, P2, P1, P2, P2));
  }
  {
    GemmDesc g = mk(h->R, P2, 0, h->A, P2, 1, h->GD[0], P1, P1, P1, P2);
    g.alpha = beta; g.vscale = 1;
    d.push_back(g);
    GemmDesc g2 = mk(h->R, P2, 1, h->Bt, P2, 0, h->GD[1], P2, P2, P2, P1);
    g2.vscale = 1;
    d.push_back(g2);
  }
  end(6);
  // Stage D: X1 = K1^{-1} T1, X2 = T2 K2^{-1} (refined)
  begin(7);
  if (!h->chain_aug) {
    d.push_back(side(mk(h->Kinv[0], P1, 0, h->T1, P2, 0, h->X1, P2, P1, P2, P1), h->Y1));
    d.push_back(side(mk(h->T2, P2, 0, h->Kinv[1], P2, 0, h->X2, P2, P1, P2, P2), h->Y2));
  }
  end(7);
  begin(8);  // refinement residuals W1 = beta D1^T R - K1 X1, W2 = R D2 - X2 K2
  if (h->chain_aug) {  // (T1, T2 never formed: dual products)
    GemmDesc g = mk(h->D[0], P1, 1, h->R, P2, 0, h->W1, P2, P1, P2, P1);
    g.alpha = beta;
    g.A2 = h->Kc[0]; g.lda2 = P1; g.B2 = h->X1; g.ldb2 = P2; g.K2 = P1; g.alpha2 = -1.0;
    pushg(gate(g, 0));
    GemmDesc g2 = mk(h->R, P2, 0, h->D[1], P2, 0, h->W2, P2, P1, P2, P2);
    g2.A2 = h->X2; g2.lda2 = P2; g2.B2 = h->Kc[1]; g2.ldb2 = P2; g2.K2 = P2; g2.alpha2 = -1.0;
    pushg(gate(g2, 1));
  } else {
    GemmDesc g = mk(h->Kc[0], P1, 0, h->X1, P2, 0, h->W1, P2, P1, P2, P1);
    g.alpha = -1.0; g.beta = 1.0; g.C0 = h->T1; g.ldc0 = P2;
    pushg(gate(g, 0));
    GemmDesc g2 = mk(h->X2, P2, 0, h->Kc[1], P2, 0, h->W2, P2, P1, P2, P2);
    g2.alpha = -1.0; g2.beta = 1.0; g2.C0 = h->T2; g2.ldc0 = P2;
    pushg(gate(g2, 1));
  }
  end(8);
  begin(9);
  {
    GemmDesc g = mk(h->Kinv[0], P1, 0, h->W1, P2, 0, h->X1, P2, P1, P2, P1);
    g.beta = 1.0; g.C0 = h->X1; g.ldc0 = P2;
    pushg(side(gate(g, 0), h->Y1));
    GemmDesc g2 = mk(h->W2, P2, 0, h->Kinv[1], P2, 0, h->X2, P2, P1, P2, P2);
    g2.beta = 1.0; g2.C0 = h->X2; g2.ldc0 = P2;
    pushg(side(gate(g2, 1), h->Y2));
  }
  end(9);
  // Stage E: G_K1 = c N2/2 K1^{-1} - Y1 A^T;  G_K2 = c N1/2 K2^{-1} - Y2^T Bt, with
  // Y = S/2 + v X written by the X producers above (one product each instead of two)
  begin(10);
  {
    GemmDesc g = mk(h->Y1, P2, 0, h->A, P2, 1, h->GK[0], P1, P1, P1, P2);
    g.alpha = -1.0;
    g.beta = 0.5 * h->prob.logdet * n2; g.C0 = h->Kinv[0]; g.ldc0 = P1;
    d.push_back(g);
    GemmDesc g2 = mk(h->Y2, P2, 1, h->Bt, P2, 0, h->GK[1], P2, P2, P2, P1);
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

// ------------------------------------------------------------------------------------------
// graph capture and the batch protocol
// ------------------------------------------------------------------------------------------
// Capture what `body` enqueues on `s` into *slot.  A failing body still ends the capture (the
// stream must leave capture mode) and wins over the capture's own error.
int capture_graph(hipStream_t s, hipGraphExec_t* slot, const std::function<int()>& body) {
  hipGraph_t g = nullptr;
  HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  const int rc = body();
  hipError_t e = hipStreamEndCapture(s, &g);
  if (rc != GPK_OK) {
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  if (e != hipSuccess) return fail(GPK_EHIP, std::string("capture: ") + hipGetErrorString(e));
  e = hipGraphInstantiate(slot, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return fail(GPK_EHIP, std::string("instantiate: ") + hipGetErrorString(e));
  return GPK_OK;
}

// `reps` steps back to back, each evaluating the next one's class values (cls_pipe_ok decides);
// fold: the batch report, written by the last step's loss workgroup (make_tail takes it)
static int enqueue_steps(gpk_handle* h, int apply, bool refine, int reps, const StepReport* fold = nullptr) {
  int rc = GPK_OK;
  h->cls_have = false;
  for (int r = 0; r < reps && rc == GPK_OK; ++r) {
    if (fold && r == reps - 1 && !h->shard) h->fold_report = fold;
    h->cls_next = r + 1 < reps;
    rc = enqueue_step(h, apply, refine);
  }
  h->cls_next = h->cls_have = false;
  return rc;
}

constexpr int STEP_GRAPH_REPS = 8;
static int capture(gpk_handle* h, int apply, bool refine = true, int reps = 1, bool batch = false) {
  hipGraphExec_t* slot = batch ? &h->g_batch[refine ? 1 : 0][reps]
                       : reps > 1 ? &h->g_multi[refine ? 1 : 0]
                                  : refine ? &h->g_exec[apply] : &h->g_fast[apply];
  if (*slot) return GPK_OK;
  if (h->shard && !h->comm->capturable())
    return fail(GPK_EINVAL, "handle belongs to an in-process rank group: use gpk_group_step / gpk_group_loss_grad");
  return capture_graph(h->s, slot, [&] { return enqueue_steps(h, apply, refine, reps); });
}

// The begin of a gpk_step batch: every batch takes the snapshot (a failed one is undone,
// read_report), a fast one also clears the violation flag; the loss slot restarts.
StepBegin make_begin(gpk_handle* h, bool fast) {
  StepBegin b{};
  b.snap = h->snap; b.params = h->params; b.m = h->m; b.v = h->v; b.np = (size_t)h->L.nparams;
  b.snap_count = h->snap_count; b.count = h->count;
  if (fast) b.viol = h->viol;
  b.loss_slot = h->loss_slot;
  return b;
}

static StepReport make_report(gpk_handle* h, bool fast, int nloss) {
  StepReport r{};
  r.status = h->status;
  r.viol = fast ? h->viol : nullptr;
  for (int a = 0; a < h->L.naxes; ++a) r.pst[a] = h->pst[a];
  r.out = h->rep_host;
  r.losses = h->losses;
  r.nloss = nloss;
  return r;
}

// Batch begin for the graph being captured: folded into the first step's chain launch when
// that launch publishes the step constants (publish_prep, copy_snapshot), else its own launch.
static int begin_batch(gpk_handle* h, const StepBegin* b) {
  if (!h->shard && h->chain && h->cls[0].ncls > 0) {
    h->fold_begin = b;
    return GPK_OK;
  }
  return check_launch(launch_step_begin(*b, h->s), "step_begin");
}

// Batch end: the last step's loss workgroup wrote the report (make_tail took fold_report), or
// the report kernel runs after it.  Leaves no fold pending (also when the capture failed: rc).
static int end_batch(gpk_handle* h, const StepReport* r, int rc) {
  const bool pending_begin = h->fold_begin != nullptr, pending_report = h->fold_report != nullptr;
  h->fold_begin = nullptr;
  h->fold_report = nullptr;
  if (rc != GPK_OK) return rc;
  if (pending_begin) return fail(GPK_EINVAL, "internal: the batch begin was not folded into a step");
  if (pending_report || h->shard) return check_launch(launch_step_report(*r, h->s), "step_report");
  return GPK_OK;
}

// A whole call as one graph: batch begin (snapshot, counters) + `reps` steps + the pinned-memory
// report -- one step(1) call (g_call, either graph kind), or a fast chunk of a step(n) call
static int capture_whole(gpk_handle* h, hipGraphExec_t* slot, bool fast, int reps) {
  if (*slot) return GPK_OK;
  const StepBegin b = make_begin(h, fast);
  const StepReport rep = make_report(h, fast, reps);
  return capture_graph(h->s, slot, [&] {
    int rc = begin_batch(h, &b);
    if (rc == GPK_OK) rc = enqueue_steps(h, 1, !fast, reps, &rep);
    return end_batch(h, &rep, rc);
  });
}

static int capture_call(gpk_handle* h, bool fast) {
  return capture_whole(h, &h->g_call[fast ? 0 : 1], fast, 1);
}

static int capture_calln(gpk_handle* h, int reps) {
  const int rc = capture_whole(h, &h->g_calln[reps], true, reps);
  if (rc != GPK_OK) h->g_calln.erase(reps);  // (no empty slot left behind)
  return rc;
}

// After a launch whose hand-off wait gave up (status bit 2), a late producer may still have
// stored real words into hand-off slots the consumer had already consumed and reset: restore
// every slot, flag and counter to its create-time state (the stream is synchronised, so every
// launch has drained) before the handle is used again -- stale words would otherwise pass for
// the next launch's inputs.
int reset_handoffs(gpk_handle* h) {
  const Layout& L = h->L;
  for (int a = 0; a < L.naxes; ++a) {
    const size_t P = axis_p(L, a), T = P / 32;
    const size_t nflags = T * (T + (L.p1 + L.p2) / 32) + 2 * T + 1;
    HIPCHK(hipMemsetD32Async(h->cgran[a], CHAIN_SENTINEL32, T * 6144, h->s));
    if (h->PB2[a]) HIPCHK(hipMemsetD32Async(h->PB2[a], CHAIN_SENTINEL32, 4 * chain_half((int)P, h->chain_multi), h->s));
    if (h->cepoch[a]) HIPCHK(hipMemsetAsync(h->cepoch[a], 0, 4 * sizeof(unsigned int), h->s));
    HIPCHK(hipMemsetAsync(h->cflags[a], 0, nflags * sizeof(unsigned int), h->s));
    HIPCHK(hipMemsetAsync(h->aflag[a], 0, (4 + P / 32) * sizeof(unsigned int), h->s));
  }
  HIPCHK(hipMemsetAsync(h->nce_flag, 0, sizeof(unsigned int), h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  return GPK_OK;
}

// A non-zero device status word `st` as the error return.  The word is cleared; handoffs: bit 2
// (a hand-off wait gave up) is told apart and the hand-off slots are reset; undo_batch: the
// handle goes back to the snapshot its batch begin took.  h may be null without either flag
// (the 3-axis solver has its own handle and neither hand-offs nor batches).
int status_error(int st, int* status, hipStream_t s, gpk_handle* h, bool undo_batch, bool handoffs) {
  const bool timeout = handoffs && (st & 2);
  HIPCHK(hipMemsetAsync(status, 0, sizeof(int), s));
  if (timeout) TRY(reset_handoffs(h));
  if (undo_batch) {
    TRY(restore_snapshot(h));
    HIPCHK(hipStreamSynchronize(s));
  }
  const std::string msg =
      timeout ? "SPD inverse: a pivot-chain hand-off timed out (device status 2)"
              : "covariance factor is not positive definite (non-positive pivot in SPD inverse)";
  return fail(GPK_ENOTPD, undo_batch ? msg + "; the batch was undone" : msg);
}

int read_status(gpk_handle* h) {
  int st = 0;
  HIPCHK(hipMemcpyAsync(&st, h->status, sizeof(int), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  return st ? status_error(st, h->status, h->s, h, false, true) : GPK_OK;
}

// End of a batch (one synchronisation): non-positive-definite status, the fast graph's gate
// violation flag, and the refinement gate of the last step, which picks the next batch's graph:
// the fast one once max_a K00 * max diag K_a^{-1} is 2x below REFINE_COND_LB, and it stays
// the fast one while that bound stays below REFINE_COND_LB itself (hysteresis: a fast batch
// that crosses the gate is caught by the check in the fast graph's tail (viol) and rerun, which
// costs one FAST_CHUNK; leaving the fast graph at the margin cost ~15% on every later step of
// C4's training, whose bound drifts to ~21 (tools/train_regime_parity.py): round 4's 8x entry
// margin (12.5) kept a handle that had left the fast graph off it for ~2000 steps).
constexpr double FAST_GRAPH_MARGIN = 2.0;
static int read_report(gpk_handle* h, bool fast, bool* violated);

// params, Adam state and step count back to the snapshot the current batch's begin took (every
// gpk_step batch takes one), U's padded copy rebuilt from params: a fast batch that met an open
// refinement gate is rerun from there, a batch that failed on the device is undone
int restore_snapshot(gpk_handle* h) {
  const size_t np = (size_t)h->L.nparams, nb = np * sizeof(double);
  HIPCHK(hipMemcpyAsync(h->params, h->snap, nb, hipMemcpyDeviceToDevice, h->s));
  HIPCHK(hipMemcpyAsync(h->m, h->snap + np, nb, hipMemcpyDeviceToDevice, h->s));
  HIPCHK(hipMemcpyAsync(h->v, h->snap + 2 * np, nb, hipMemcpyDeviceToDevice, h->s));
  HIPCHK(hipMemcpyAsync(h->count, h->snap_count, sizeof(int), hipMemcpyDeviceToDevice, h->s));
  return check_launch(launch_sync_u(h->params, h->L, h->Up, h->s), "sync_u");
}

static int finish_batch(gpk_handle* h, bool fast, bool* violated) {
  TRY(check_launch(launch_step_report(make_report(h, fast, h->pend_losses ? h->pend_n : 0), h->s),
                   "step_report"));
  HIPCHK(hipStreamSynchronize(h->s));
  return read_report(h, fast, violated);
}

// the report written by step_report_kernel (the stream has been synchronised)
static int read_report(gpk_handle* h, bool fast, bool* violated) {
  if (h->pend_losses) std::memcpy(h->pend_losses, h->rep_host + 8, h->pend_n * sizeof(double));
  h->pend_losses = nullptr;
  h->pend_n = 0;
  const int st = (int)h->rep_host[0];
  const unsigned int vi = (unsigned int)h->rep_host[1];
  double ps[2][2] = {{h->rep_host[2], h->rep_host[3]}, {h->rep_host[4], h->rep_host[5]}};
  *violated = false;
  // undo the batch (its begin took the snapshot), then report
  if (st) return status_error(st, h->status, h->s, h, true, true);
  *violated = fast && vi;
  if (h->fast_ok) {
    double lb = 0.0;  // pst[a][1] holds max diag K^{-1} (positive, atomicMax'd as its bits)
    for (int a = 0; a < h->L.naxes; ++a) lb = std::max(lb, ps[a][0] * ps[a][1]);
    const double margin = (fast && !*violated) ? 1.0 : FAST_GRAPH_MARGIN;
    h->fast_mode = !*violated && lb * margin < REFINE_COND_LB;
  }
  return GPK_OK;
}

int gpk_loss_grad(gpk_handle* h, double* loss, double* grad_flat) {
  if (!h || !loss) return fail(GPK_EINVAL, "NULL argument");
  DevSwitch ds(h->dev);
  h->pend_losses = nullptr;
  bool fast = h->fast_ok && h->fast_mode, viol = false;
  for (int pass = 0; pass < 2; ++pass) {
    TRY(capture(h, 0, !fast));
    {
      StepBegin b{};
      b.viol = fast ? h->viol : nullptr;
      b.loss_slot = h->loss_slot;
      TRY(check_launch(launch_step_begin(b, h->s), "step_begin"));
    }
    HIPCHK(hipGraphLaunch(fast ? h->g_fast[0] : h->g_exec[0], h->s));
    HIPCHK(hipMemcpyAsync(loss, h->diag, sizeof(double), hipMemcpyDeviceToHost, h->s));
    if (grad_flat)
      HIPCHK(hipMemcpyAsync(grad_flat, h->grad, h->L.nparams * sizeof(double), hipMemcpyDeviceToHost, h->s));
    TRY(finish_batch(h, fast, &viol));
    if (!viol) break;
    ++h->rollbacks;  // nothing to restore: apply = 0 leaves params and Adam state alone
    fast = false;
  }
  return GPK_OK;
}

static int run_steps(gpk_handle* h, int n_steps, double* losses, bool fast, bool reset_slot = true) {
  hipGraphExec_t ge = fast ? h->g_fast[1] : h->g_exec[1];
  const bool multi = !h->shard && n_steps >= STEP_GRAPH_REPS;
  if (multi) TRY(capture(h, 1, !fast, STEP_GRAPH_REPS));
  hipGraphExec_t gm = multi ? h->g_multi[fast ? 0 : 1] : nullptr;
  int done = 0;
  while (done < n_steps) {
    const int nb = std::min(LOSS_CAP, n_steps - done);
    if (reset_slot || done > 0) HIPCHK(hipMemsetAsync(h->loss_slot, 0, sizeof(int), h->s));
    int i = 0;
    const auto& bg = h->g_batch[fast ? 0 : 1];
    while (i < nb) {  // prepared batch graphs: the whole rest, else the largest that fits
      auto it = bg.find(nb - i);
      if (it == bg.end() || !it->second) {
        it = bg.upper_bound(nb - i);
        if (it == bg.begin()) break;
        --it;
        if (!it->second || it->first <= STEP_GRAPH_REPS) break;
      }
      HIPCHK(hipGraphLaunch(it->second, h->s));
      i += it->first;
    }
    if (multi)
      for (; i + STEP_GRAPH_REPS <= nb; i += STEP_GRAPH_REPS) HIPCHK(hipGraphLaunch(gm, h->s));
    for (; i < nb; ++i) HIPCHK(hipGraphLaunch(ge, h->s));
    if (losses && done + nb < n_steps) {
      HIPCHK(hipMemcpyAsync(losses + done, h->losses, nb * sizeof(double), hipMemcpyDeviceToHost, h->s));
    } else if (losses) {  // the last batch's losses come back with finish_batch's report
      h->pend_losses = losses + done;
      h->pend_n = nb;
    }
    done += nb;
  }
  return GPK_OK;
}

// Fast batches run in chunks of FAST_CHUNK steps, each checked at its end: a step that met an
// open refinement gate costs a rerun of its chunk only (not of the whole call -- at C3 the
// gate opens mid-training, and a 300-step call used to run twice).
constexpr int FAST_CHUNK = 64;
constexpr int kBatchMax = FAST_CHUNK;  // largest prepared batch graph

// A whole-call graph (capture_call / capture_calln) ends its report with the ready word
// rep_host[7] (stepk_dev.h report_ready): the host waits for that word instead of the stream, so
// gpk_step returns as soon as the call's losses and status are final -- the last step's dL/dU and
// Adam on U may still run, ordered before anything later enqueued on the handle's stream.  The
// wait polls the stream every few thousand reads, so a faulted or finished-without-report stream
// ends it.
static void arm_report(gpk_handle* h) {
  reinterpret_cast<volatile double*>(h->rep_host)[7] = 0.0;
}

static int wait_report(gpk_handle* h) {
  volatile double* ready = reinterpret_cast<volatile double*>(h->rep_host) + 7;
  for (unsigned it = 1;; ++it) {
    if (*ready != 0.0) break;
    // back-off: tight for the first 2^14 reads (a C4 step's report lands within ~100 us), then
    // a pause per read, then a yield per read past 2^20 (a C5 call waits tens of ms: the host
    // core is left to others instead of spinning flat out)
    if (it > (1u << 20)) sched_yield();
    else if (it > (1u << 14)) __builtin_ia32_pause();
    if ((it & 4095u) == 0) {
      const hipError_t e = hipStreamQuery(h->s);
      if (e == hipErrorNotReady) continue;
      if (e != hipSuccess) return fail(GPK_EHIP, std::string("step graph: ") + hipGetErrorString(e));
      if (*ready != 0.0) break;
      return fail(GPK_EHIP, "internal: the step graph finished without its report");
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return GPK_OK;
}

// launch a whole-call graph and read its report: the batch's n losses, status, violation, gate
static int launch_call_graph(gpk_handle* h, hipGraphExec_t g, bool fast, double* losses, int n, bool* viol) {
  arm_report(h);
  HIPCHK(hipGraphLaunch(g, h->s));
  TRY(wait_report(h));
  h->pend_losses = losses;
  h->pend_n = n;
  return read_report(h, fast, viol);
}

// gpk_set_wait_limit_chunk: the poll budget applied while gpk_step runs one chunk of a call
// (tests: a failure in a later chunk leaves the earlier chunks applied)
static std::atomic<int> g_chunk_limit_polls{0}, g_chunk_limit_at{-1};
struct ChunkWaitLimit {
  bool on = false;
  ChunkWaitLimit(gpk_handle* h, int chunk) {
    if (g_chunk_limit_polls.load() <= 0 || chunk != g_chunk_limit_at.load()) return;
    // (the previous chunk's tail may still run: the limit must not reach its waits)
    on = hipStreamSynchronize(h->s) == hipSuccess && gpk_set_wait_limit(g_chunk_limit_polls.load()) == GPK_OK;
  }
  ~ChunkWaitLimit() {
    if (on) gpk_set_wait_limit(0);
  }
};

int gpk_set_wait_limit_chunk(int32_t polls, int32_t chunk) {
  if (polls < 0) return fail(GPK_EINVAL, "polls must be >= 0");
  g_chunk_limit_polls.store(polls);
  g_chunk_limit_at.store(polls > 0 ? chunk : -1);
  return GPK_OK;
}

int gpk_step(gpk_handle* h, int32_t n_steps, double* losses) {
  if (!h) return fail(GPK_EINVAL, "NULL handle");
  if (n_steps < 0) return fail(GPK_EINVAL, "n_steps < 0");
  DevSwitch ds(h->dev);
  h->pend_losses = nullptr;  // (a failed earlier call may have left one)
  int done = 0;
  if (n_steps == 1 && !h->shard) {  // one graph launch per call (a rollback takes the path below)
    const bool fast = h->fast_ok && h->fast_mode;
    bool viol = false;
    TRY(capture_call(h, fast));
    TRY(launch_call_graph(h, h->g_call[fast ? 0 : 1], fast, losses, 1, &viol));
    if (!viol) return GPK_OK;
    ++h->rollbacks;  // restore the snapshot the call graph took and rerun with the full graph
    TRY(restore_snapshot(h));
    TRY(capture_call(h, false));
    return launch_call_graph(h, h->g_call[1], false, losses, 1, &viol);
  }
  for (int chunk = 0; done < n_steps; ++chunk) {
    ChunkWaitLimit chunk_limit(h, chunk);  // (tests: gpk_set_wait_limit_chunk)
    // (both graphs run in FAST_CHUNK chunks while the fast graph is available, so the mode is
    // re-decided every 64 steps: a long first call on the full graph used to keep its whole
    // length there, and the training that followed, until the gate bound fell below the entry
    // margin -- round 4's W = 200 line at 8100 it/s)
    const bool fast = h->fast_ok && h->fast_mode;
    const int n = h->fast_ok ? std::min(FAST_CHUNK, n_steps - done) : n_steps - done;
    double* lo = losses ? losses + done : nullptr;
    bool viol = false;
    auto cg = fast && !h->shard ? h->g_calln.find(n) : h->g_calln.end();
    if (cg != h->g_calln.end() && cg->second) {  // a prepared whole-chunk graph
      TRY(launch_call_graph(h, cg->second, true, lo, n, &viol));
    } else {
      TRY(capture(h, 1, !fast));
      // the snapshot of everything a fast batch carries forward (Up is rebuilt from params), the
      // violation flag and the loss slot: one launch
      TRY(check_launch(launch_step_begin(make_begin(h, fast), h->s), "step_begin"));
      TRY(run_steps(h, n, lo, fast, false));
      TRY(finish_batch(h, fast, &viol));
    }
    if (viol) {  // a step of the chunk needed refinement: roll back and rerun with the full graph
      ++h->rollbacks;
      TRY(restore_snapshot(h));
      TRY(capture(h, 1, true));
      TRY(run_steps(h, n, lo, false));
      TRY(finish_batch(h, false, &viol));
    }
    done += n;
  }
  return GPK_OK;
}

int gpk_prepare(gpk_handle* h, int32_t n_steps) {
  if (!h) return fail(GPK_EINVAL, "NULL handle");
  if (n_steps < 0) return fail(GPK_EINVAL, "n_steps < 0");
  if (h->shard && !h->comm->capturable()) return GPK_OK;  // in-process groups run eagerly
  DevSwitch ds(h->dev);
  for (int refine = 0; refine < 2; ++refine) {
    if (!refine && !h->fast_ok) continue;
    TRY(capture(h, 1, refine != 0));
    if (!h->shard) TRY(capture_call(h, refine == 0));
    if (!h->shard && n_steps >= STEP_GRAPH_REPS) TRY(capture(h, 1, refine != 0, STEP_GRAPH_REPS));
    // the chunks of a call of n_steps: FAST_CHUNK-step chunks + the remainder whenever the fast
    // graph exists (fast_ok), on either graph -- each chunk is a batch of its own (snapshot,
    // report, undo on failure); without a fast graph the whole call is one batch, run as
    // kBatchMax-step graphs + the remainder.  One graph each
    if (!h->shard && n_steps > STEP_GRAPH_REPS) {
      const int full = std::min(n_steps, kBatchMax), rest = n_steps % kBatchMax;
      TRY(capture(h, 1, refine != 0, full, true));
      if (rest > STEP_GRAPH_REPS && rest != full) TRY(capture(h, 1, refine != 0, rest, true));
    }
    // fast chunks as whole-call graphs (begin + steps + report)
    if (!refine && !h->shard && n_steps > 1) {
      const int full = std::min(n_steps, FAST_CHUNK), rest = n_steps % FAST_CHUNK;
      TRY(capture_calln(h, full));
      if (rest > 1 && rest != full) TRY(capture_calln(h, rest));
    }
  }
  HIPCHK(hipStreamSynchronize(h->s));
  return GPK_OK;
}

int gpk_set_wait_limit(int32_t polls) {
  if (polls < 0) return fail(GPK_EINVAL, "polls must be >= 0");
  const unsigned v = polls > 0 ? (unsigned)polls : SPIN_CAP;
  if (wait_limit_spdinv(v) != hipSuccess || wait_limit_spdbig(v) != hipSuccess ||
      wait_limit_assemble(v) != hipSuccess || wait_limit_pgrad(v) != hipSuccess)
    return fail(GPK_EHIP, "set the wait limit");
  return GPK_OK;
}
