// gpk_step.cpp — one log-joint step of a handle in stream order: its argument fillers, the SPD
// inverse launches and enqueue_step.  The 2D GEMM plan it launches is built in gpk_plan.cpp; the
// graphs and batches it runs in are gpk_batch.cpp's; the row-sharded enqueue is in gpk_shard.cpp.
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
int enqueue_assemble_inverse(gpk_handle* h, const StepCtx& c, StepDone* done) {
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
  PrepArgs prep = make_prep(h, c.apply), prep_eval = prep;
  prep_eval.skip = eval_only ? 1 : 0;
  if (eval_only && c.begin) {  // the batch begin rides on the chain launch's prep row
    const StepBegin& b = *c.begin;
    prep.snap = b.snap; prep.snap_m = b.m; prep.snap_v = b.v; prep.snap_np = b.np;
    prep.snap_count = b.snap ? b.snap_count : nullptr;
    prep.viol0 = b.viol; prep.slot0 = b.loss_slot;
    if (done) done->begin = true;
  }
  // (have_cls: the previous step's parameter-gradient launch evaluated them, cls_pipe_ok)
  if (!(eval_only && c.have_cls))
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
TailArgs make_tail(gpk_handle* h, const StepCtx& c) {
  const Layout& L = h->L;
  const int ac = h->prob.eq == GPK_ALLENCAHN;
  TailArgs T{};
  T.fused = 1;
  FinalizeArgs& f = T.fin;
  f.L = L; f.hyper = h->hyper; f.llk_weight = h->prob.llk_weight; f.logdet = h->prob.logdet;
  f.apply = c.apply; f.has_cos = kind_cos(h->prob.kind);
  f.red_quad = h->red_quad; f.nquad = h->nquad; f.red_egap = h->red_egap; f.negap = h->negap;
  for (int a = 0; a < L.naxes; ++a) { f.ldet[a] = h->ldet[a]; f.nldet[a] = h->nldet[a]; }
  f.pg = h->pg; f.kc = h->kc; f.sc = h->sc; f.Up = h->Up; f.bvals = h->bvals;
  f.bidx = h->bidx; f.nb = h->prob.nb;
  f.params = h->params; f.grad = h->grad; f.m = h->m; f.v = h->v;
  f.losses = h->losses; f.loss_slot = h->loss_slot; f.diag = h->diag;
  f.bgap = h->bgap;
  f.bgap_parts = h->bgap_parts;
  if (!c.refine) {  // fast graph: check that no refinement was needed
    for (int a = 0; a < L.naxes; ++a) f.watch[a] = h->pst[a];
    f.viol = h->viol;
  }
  if (c.report) {  // the loss workgroup writes the batch report
    f.report = 1;
    f.rep = *c.report;
  }
  AdamUArgs& au = T.adam;
  au.L = L; au.hyper = h->hyper; au.llk_weight = h->prob.llk_weight; au.apply = c.apply; au.ac = ac;
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
  if (c.next_cls && cls_pipe_ok(h)) {  // the next step's class values, after the Adam
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

// what the step's last launch carried (make_tail decided): the next step's class values, the report
static void tail_done(const TailArgs& tail, StepDone* done) {
  if (!done) return;
  done->next_cls = tail.nce_flag != nullptr;
  done->report = tail.fin.report != 0;
}

int enqueue_step(gpk_handle* h, const StepCtx& c, StepDone* done) {
  if (h->shard) return enqueue_step_shard(h, c.apply);
  const Layout& L = h->L;
  if (h->profiling) (void)hipEventRecord(h->ev[0], h->s);
  mark(h, 0);  // "prep" is fused into the assembly launch (stage kept for the name table)
  TRY(enqueue_assemble_inverse(h, c, done));
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
      if (h->st[k].n == 0 || (!c.refine && h->st[k].gated)) continue;
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
    TailArgs tail = make_tail(h, c);
    TRY(check_launch(launch_pgrad(h->prob.kind, L.q, 0, pa, 2, h->bpa, h->sc, h->s, &tail), "pgrad"));
    tail_done(tail, done);
    stamp("pgrad_tail");
  } else {
    const int P = L.p1;
    // every K^{-1} application gets one step of iterative refinement x += K^{-1}(b - K x),
    // gated on a cond(K) lower bound (gemv skips itself when K is well conditioned)
    GemvDesc g{};
    g.lda = P; g.p = P; g.rows = P; g.alpha = 1.0; g.ac = ac; g.F = h->F; g.U = h->Up; g.U0 = h->uoff;
    auto gemv = [&](const char* nm, const double* A, const double* x, double* y, double alpha,
                    const double* C0, double beta, int epi, double* red, bool gated) -> int {
      if (gated && !c.refine) return GPK_OK;
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
    TailArgs tail = make_tail(h, c);
    TRY(check_launch(launch_pgrad(h->prob.kind, L.q, 1, &pa, 1, h->bpa, h->sc, h->s, &tail), "pgrad"));
    tail_done(tail, done);
    stamp("pgrad_tail");
  }
  h->nstage = stage;
  return GPK_OK;
}
