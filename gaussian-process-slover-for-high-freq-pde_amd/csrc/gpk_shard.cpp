// gpk_shard.cpp — the row-sharded 2D step: its collective backends (RCCL, and an in-process
// group of handles), the shard plan (build_shard), its enqueue, and the gpk_create_sharded /
// gpk_group_* entry points.  The only translation unit that includes RCCL.
#include <rccl/rccl.h>

#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

#include "gpk_host.h"

// ------------------------------------------------------------------------------------------
// row-sharded multi-GPU step (the reference has no multi-GPU path)
//
// Every rank holds the whole problem, assembles and inverts both Kronecker factors itself
// (replicated: O(N^2 Q) + O(N^3) per factor), and computes rows [r*h, (r+1)*h) of every
// product of the step -- the GEMM stages are ~26 N^3 of the ~28 N^3 flops (C5: 1.9 TFLOP).
// A row slice of C = op(A) op(B) needs only the same rows of op(A); every operand a later
// stage reads beyond its own rows (a B operand, or an A operand read transposed) is completed
// by an in-place all-gather of its row blocks.  The kernel-parameter contraction runs over a
// 1/P share of the pair tiles; its partials, the per-tile loss partials (||R||^2, <A,Bt>) and
// nothing else are all-reduced (6Q+2 tile vectors); the loss and the small-parameter Adam are
// then identical on every rank; Adam on U updates the rank's rows, which are all-gathered.
// Collectives: RCCL in the handle's stream (captured into the step's hipGraph), or -- for tests
// on one GPU -- an in-process group of handles, one host thread per rank.
// ------------------------------------------------------------------------------------------
namespace {

int nccl_check(ncclResult_t r, const char* what) {
  return r == ncclSuccess ? GPK_OK : fail(GPK_ERCCL, std::string(what) + ": " + ncclGetErrorString(r));
}

struct RcclComm : ShardComm {
  ncclComm_t c = nullptr;
  ~RcclComm() override {
    if (c) (void)ncclCommDestroy(c);
  }
  int allgather(gpk_handle* h, double* buf, size_t chunk) override {
    return nccl_check(ncclAllGather(buf + (size_t)h->rank * chunk, buf, chunk, ncclDouble, c, h->s), "ncclAllGather");
  }
  int allreduce(gpk_handle* h, double* buf, size_t n) override {
    return nccl_check(ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, c, h->s), "ncclAllReduce");
  }
  int broadcast(gpk_handle* h, double* buf, size_t n, int root) override {
    return nccl_check(ncclBroadcast(buf, buf, n, ncclDouble, root, c, h->s), "ncclBroadcast");
  }
  bool capturable() const override { return true; }
};

// In-process group (one device, one host thread per rank): collectives meet at a host barrier;
// rank 0 moves the blocks with device copies (and sums in rank order: deterministic).
struct LocalGroup {
  int n = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  long gen = 0;
  bool broken = false;
  std::vector<double*> slot;
  bool barrier() {  // false if another rank failed
    std::unique_lock<std::mutex> lk(mu);
    if (broken) return false;
    const long g = gen;
    if (++arrived == n) {
      arrived = 0;
      ++gen;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != g || broken; });
    }
    return !broken;
  }
  void abort() {
    std::lock_guard<std::mutex> lk(mu);
    broken = true;
    cv.notify_all();
  }
};

struct LocalComm : ShardComm {
  std::shared_ptr<LocalGroup> g;
  // One collective: drain this rank's stream, publish its buffer, meet; rank 0 does `work` (its
  // failure message, or null) on every rank's buffer and drains; meet again.
  template <class Work>
  int rendezvous(gpk_handle* h, double* buf, const char* sync_msg, Work work) {
    HIPCHK(hipStreamSynchronize(h->s));
    g->slot[h->rank] = buf;
    if (!g->barrier()) return fail(GPK_EHIP, "rank group aborted");
    int rc = GPK_OK;
    if (h->rank == 0) {
      rc = work();
      if (hipStreamSynchronize(h->s) != hipSuccess) rc = fail(GPK_EHIP, sync_msg);
    }
    if (!g->barrier()) return fail(GPK_EHIP, "rank group aborted");
    return rc;
  }
  int copy(gpk_handle* h, double* dst, const double* src, size_t n, const char* msg) {
    return hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToDevice, h->s) == hipSuccess
               ? GPK_OK : fail(GPK_EHIP, msg);
  }
  int allgather(gpk_handle* h, double* buf, size_t chunk) override {
    return rendezvous(h, buf, "group all-gather sync", [&] {
      int rc = GPK_OK;
      for (int src = 0; src < g->n && rc == GPK_OK; ++src)
        for (int dst = 0; dst < g->n; ++dst)
          if (dst != src && copy(h, g->slot[dst] + (size_t)src * chunk, g->slot[src] + (size_t)src * chunk,
                                 chunk, "group all-gather copy") != GPK_OK)
            rc = GPK_EHIP;
      return rc;
    });
  }
  int allreduce(gpk_handle* h, double* buf, size_t n) override {
    return rendezvous(h, buf, "group all-reduce sync", [&] {
      int rc = GPK_OK;
      for (int src = 1; src < g->n && rc == GPK_OK; ++src)
        rc = check_launch(launch_add_into(g->slot[0], g->slot[src], n, h->s), "add_into");
      for (int dst = 1; dst < g->n && rc == GPK_OK; ++dst)
        rc = copy(h, g->slot[dst], g->slot[0], n, "group all-reduce copy");
      return rc;
    });
  }
  int broadcast(gpk_handle* h, double* buf, size_t n, int root) override {
    return rendezvous(h, buf, "group broadcast sync", [&] {
      int rc = GPK_OK;
      for (int dst = 0; dst < g->n && rc == GPK_OK; ++dst)
        if (dst != root) rc = copy(h, g->slot[dst], g->slot[root], n, "group broadcast copy");
      return rc;
    });
  }
  bool capturable() const override { return false; }
};

int tile_cols_count(const GemmDesc& d, int variant) {
  const int tc = gemm_tile_dim(variant);
  return (d.N + tc - 1) / tc;
}

// rows [r0, r0 + rows) of C = op(A) op(B) [+ dual] with every row-indexed operand offset
GemmDesc slice_rows(const GemmDesc& d, int r0, int rows, int variant) {
  GemmDesc s = d;
  s.M = rows;
  s.A = d.ta ? d.A + r0 : d.A + (size_t)r0 * d.lda;
  if (d.K2) s.A2 = d.ta2 ? d.A2 + r0 : d.A2 + (size_t)r0 * d.lda2;
  s.C = d.C + (size_t)r0 * d.ldc;
  if (d.C0) s.C0 = d.C0 + (size_t)r0 * d.ldc0;
  if (d.F) s.F = d.F + (size_t)r0 * d.ldf;
  if (d.U) s.U = d.U + (size_t)r0 * d.ldf;
  if (d.Q1) s.Q1 = d.Q1 + (size_t)r0 * d.ldf;
  if (d.Q2) s.Q2 = d.Q2 + (size_t)r0 * d.ldf;
  if (d.Y) {
    s.Y = d.Y + (size_t)r0 * d.ldy;
    s.Ys = d.Ys + (size_t)r0 * d.ldy;
  }
  const size_t toff = (size_t)(r0 / gemm_tile_dim(variant)) * tile_cols_count(d, variant);
  if (d.red) s.red = d.red + toff;
  if (d.red2) s.red2 = d.red2 + toff;
  return s;
}

// rows [r0, r0 + rows) of the CONTRACTION index of C = op(A) op(B) (single product): this rank's
// partial of a full-size C, summed over ranks only through the linear parameter contraction.
// The C0 term is carried by rank 0 alone.
GemmDesc slice_k(const GemmDesc& d, int r0, int rows, int rank) {
  GemmDesc s = d;
  s.K = rows;
  s.A = d.ta ? d.A + (size_t)r0 * d.lda : d.A + r0;
  s.B = d.tb ? d.B + r0 : d.B + (size_t)r0 * d.ldb;
  if (rank != 0) {
    s.C0 = nullptr;
    s.beta = 0.0;
  }
  return s;
}

}  // namespace

// GPK_FLAG_SPLIT_FACTORS: factor b's K^{-1}, log-det blocks and gate from its group's first rank
int split_broadcast(gpk_handle* h) {
  for (int b = 0; b < 2; ++b) {
    const int P = axis_p(h->L, b), root = b ? h->nranks / 2 : 0;
    TRY(h->comm->broadcast(h, h->Kinv[b], (size_t)P * P, root));
    TRY(h->comm->broadcast(h, h->ldet[b], (size_t)P / 32, root));
    TRY(h->comm->broadcast(h, h->pst[b], 2, root));
  }
  return GPK_OK;
}

// Row slices of the step's GEMM stages for this rank, the variant per stage (its tile rows must
// divide the slice height so that the per-tile loss partials land in the full-grid slots), and
// the all-gathers after each stage: exactly the outputs a later stage reads beyond its rows.
// Every descriptor runs in one of three modes: 'r' its output rows [r h, (r + 1) h) (slice_rows),
// 'k' this rank's share of its contraction index (slice_k: G_K2, G_D2, summed through the
// linear parameter contraction) or 'f' whole (replicated on every rank).  The plan -- modes per
// stage, then the collectives -- is kept as text (gpk_shard_plan) and restated by gpk/shard.py
// shard_plan(), whose host stand-in runs it across gloo processes (tests/test_shard.py).
//   augmented chain (small factors, C4): every rank's inverse launch yields the whole A, Bt and
//   K^{-1} D^T, so the forward refinement (stages 1, 2: the gate's two GEMMs) and X1 =
//   beta (K1^{-1} D1^T) R with its refinement (stages 6, 8, 9: one P1^3 product each, cheap at
//   these sizes) run whole: the step's collectives are the R gather, ONE all-reduce and the U
//   gather.
//   otherwise (large factors, C5; the factor split): A is gathered after stage 0 and 2 (W1
//   after the refinement's residual), R, T1 (and X1 / W1 of the reverse refinement) after their
//   stages -- each a 4096^2 row block exchange instead of a replicated 4096^3 product.
int build_shard(gpk_handle* h) {
  const Layout& L = h->L;
  const int P1 = L.p1, P2 = L.p2;
  h->h1 = P1 / h->nranks;
  h->h2 = P2 / h->nranks;
  const int force = gemm_force(h->prob.flags);
  const bool aug = h->chain_aug;
  h->sdescs.clear();
  auto mode_of = [&](int k, const GemmDesc& d) -> char {
    // G_K2 = c N1/2 K2^{-1} - Y2^T Bt and G_D2 = v R^T Bt contract over the P1 rows: each rank
    // forms the full matrix from its own rows of Y2 / R and Bt (no all-gather of those operands)
    if (d.C == h->GK[1] || d.C == h->GD[1]) return 'k';
    if (aug && (k == 1 || k == 2)) return 'f';
    if (aug && (k == 6 || k == 8 || k == 9) && (d.C == h->X1 || d.C == h->W1)) return 'f';
    return 'r';
  };
  auto slice = [&](char mode, const GemmDesc& d, int variant) {
    const int rows = d.M == P1 ? h->h1 : h->h2;
    if (mode == 'k') return slice_k(d, h->rank * h->h1, h->h1, h->rank);
    if (mode == 'f') return d;
    return slice_rows(d, h->rank * rows, rows, variant);
  };
  for (int k = 0; k < kGemmStages; ++k) {
    const GemmDesc* full = h->hdescs.data() + h->st[k].off;
    const int n = h->st[k].n;
    std::vector<GemmDesc> tmp;
    for (int i = 0; i < n; ++i) {
      const GemmDesc& d = full[i];
      if (d.M != P1 && d.M != P2) return fail(GPK_EINVAL, "shard: unexpected GEMM row count");
      tmp.push_back(slice(mode_of(k, d), d, GEMM_SMALL));
    }
    int variant = gemm_variant(tmp.data(), n, force);
    for (int i = 0; i < n; ++i)
      while (mode_of(k, full[i]) == 'r' && (full[i].M == P1 ? h->h1 : h->h2) % gemm_tile_dim(variant) != 0)
        variant = variant == GEMM_HUGE ? GEMM_BIG : GEMM_SMALL;
    h->sst[k].off = (int)h->sdescs.size();
    h->sst[k].n = n;
    h->sst[k].variant = variant;
    for (int i = 0; i < n; ++i) {
      h->sdescs.push_back(slice(mode_of(k, full[i]), full[i], variant));
      if (full[i].red) h->nquad = h->negap = gemm_tiles(full[i], variant);
    }
  }
  // All-gathers: exactly the operands a later product reads beyond this rank's rows.  G_K / G_D
  // are never gathered: axis 1's are row slices (the other rows stay zero on this rank), axis
  // 2's this rank's partials (slice_k); the parameter contraction is linear in them, so every
  // rank contracts what it holds and the partials are all-reduced (enqueue_step_shard).
  auto g1 = [&](double* b) { return ShardGather{b, (size_t)h->h1 * P2}; };
  for (auto& v : h->sgather) v.clear();
  std::string gplan[kGemmStages];
  auto gather = [&](int k, double* b, const char* name) {
    h->sgather[k].push_back(g1(b));
    gplan[k] += std::string(" g") + name;
  };
  if (aug) {
    gather(3, h->R, "R");                                      // X1 = beta P1 R, T = D1^T R (W1)
  } else {
    // (the refinement stages this handle has: build_descs, GPK_FLAG_REFINE_ALL / NO_REFINE)
    if (h->st[1].n > 0) {
      gather(0, h->A, "A");                                    // A_res: K1 A
      gather(1, h->W1, "W1");                                  // A_fix: K1^{-1} W1
    }
    gather(2, h->A, "A");                                      // R: D1 A;  G_K1 = Y1 A^T
    gather(3, h->R, "R");                                      // T1 = D1^T R
    gather(6, h->T1, "T1");                                    // X1 = K1^{-1} T1
    if (h->st[8].n > 0) {
      gather(7, h->X1, "X1");                                  // D_res: K1 X1
      gather(8, h->W1, "W1");                                  // D_fix: K1^{-1} W1
    }
  }
  // the plan: per stage its descriptors' modes, then the gathers that follow it
  std::string out;
  for (int k = 0; k < kGemmStages; ++k) {
    const GemmDesc* full = h->hdescs.data() + h->st[k].off;
    if (h->st[k].n) {
      out += (out.empty() ? "" : " ") + std::string("s") + std::to_string(k) + ":";
      for (int i = 0; i < h->st[k].n; ++i) out += mode_of(k, full[i]);
    }
    out += gplan[k];
  }
  h->splan = out + " ar gU";  // + the step's one all-reduce and the U rows after Adam
  return GPK_OK;
}

int enqueue_step_shard(gpk_handle* h, int apply) {
  const Layout& L = h->L;
  StepCtx ctx;  // (a full step that folds nothing: the batch begin and report are launches)
  ctx.apply = apply;
  TRY(enqueue_assemble_inverse(h, ctx));  // replicated: K, D, K^{-1}, log det, step constants
  for (int k = 0; k < kGemmStages; ++k) {
    if (h->sst[k].n)  // (empty: a refinement stage of a path without refinement)
      TRY(check_launch(launch_gemm_auto(h->sdescs.data() + h->sst[k].off, h->sst[k].n, h->sc, h->s,
                                        h->sst[k].variant), "gemm"));
    for (const ShardGather& g : h->sgather[k]) TRY(h->comm->allgather(h, g.buf, g.chunk));
  }
  // the base arguments only: a sharded handle has neither low parts (pg_dd) nor class partials
  PGradArgs pa[2];
  fill_pgrad2d(h, pa);
  // every rank contracts its own G_K / G_D rows (axis 1) and partials (axis 2) in full
  TRY(check_launch(launch_pgrad(h->prob.kind, L.q, 0, pa, 2, h->bpa, h->sc, h->s, nullptr), "pgrad"));
  TRY(check_launch(launch_reduce_parts(h->pgpart, h->bpa, 2, L.q, h->pg, h->s), "reduce_parts"));
  // the step's one all-reduce: [status bits | parameter-contraction partials | per-tile ||R||^2 |
  // per-tile <A, Bt>], contiguous (h->sred).  The status rides in it: a failed inverse (or a
  // rank-local hand-off timeout) fails every rank's batch before the loss is formed -- every rank
  // runs the same collectives whatever its status, so none waits alone
  TRY(check_launch(launch_status_f64(h->status, h->stat_x, 0, h->s), "status_pack"));
  TRY(h->comm->allreduce(h, h->sred, (size_t)(h->red_quad + h->nquad - h->sred)));
  TRY(check_launch(launch_status_f64(h->status, h->stat_x, 1, h->s), "status_unpack"));
  TailArgs T = make_tail(h, ctx);
  T.fin.gpart = T.fin.gpart_lo = nullptr;  // (pg all-reduced above)
  T.fin.pg_out = nullptr;
  TRY(check_launch(launch_finalize(T.fin, h->s), "finalize"));
  // this rank's tile slots are rewritten next step; the summed copies must not leak into it
  HIPCHK(hipMemsetAsync(h->red_egap, 0, (size_t)h->negap * sizeof(double), h->s));
  HIPCHK(hipMemsetAsync(h->red_quad, 0, (size_t)h->nquad * sizeof(double), h->s));
  AdamUArgs au = T.adam;
  const int r0 = h->rank * h->h1, r1 = std::min(L.n1, r0 + h->h1);
  const int nu = L.n1 * L.n2;
  au.e0 = r0 < r1 ? r0 * L.n2 : nu;
  au.e1 = r0 < r1 ? r1 * L.n2 : nu;
  TRY(check_launch(launch_adam_u(au, h->s), "adam_u"));
  TRY(h->comm->allgather(h, h->Up, (size_t)h->h1 * L.p2));
  return GPK_OK;
}

int gpk_comm_unique_id(uint8_t* out, int32_t len) {
  if (!out || len < (int32_t)sizeof(ncclUniqueId)) return fail(GPK_EINVAL, "need a 128-byte buffer");
  ncclUniqueId id;
  TRY(nccl_check(ncclGetUniqueId(&id), "ncclGetUniqueId"));
  std::memcpy(out, &id, sizeof(id));
  return GPK_OK;
}

int gpk_create_sharded(const gpk_problem* p, double freq_scale, int32_t rank, int32_t nranks,
                       const uint8_t* comm_id, gpk_handle** out) {
  if (!p || !out || !comm_id) return fail(GPK_EINVAL, "NULL argument");
  if (p->dim != 2) return fail(GPK_EINVAL, "row-sharded handles are 2D (Kronecker) only");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(GPK_EINVAL, "bad rank / nranks");
  gpk_handle* h = nullptr;
  TRY(create_impl(p, freq_scale, rank, nranks, true, &h));
  DevSwitch ds(h->dev);
  RcclComm* c = new RcclComm();
  ncclUniqueId id;
  std::memcpy(&id, comm_id, sizeof(id));
  const int rc = nccl_check(ncclCommInitRank(&c->c, nranks, id, rank), "ncclCommInitRank");
  if (rc != GPK_OK) {
    delete c;
    gpk_destroy(h);  // (leaves the error message alone)
    return rc;
  }
  h->comm = c;
  *out = h;
  return GPK_OK;
}

int gpk_group_create(const gpk_problem* p, double freq_scale, int32_t nranks, gpk_handle** out) {
  if (!p || !out) return fail(GPK_EINVAL, "NULL argument");
  if (p->dim != 2) return fail(GPK_EINVAL, "row-sharded handles are 2D (Kronecker) only");
  if (nranks < 1 || nranks > 64) return fail(GPK_EINVAL, "nranks must be in [1, 64]");
  auto g = std::make_shared<LocalGroup>();
  g->n = nranks;
  g->slot.assign(nranks, nullptr);
  for (int r = 0; r < nranks; ++r) out[r] = nullptr;
  for (int r = 0; r < nranks; ++r) {
    int rc = create_impl(p, freq_scale, r, nranks, true, &out[r], true);
    if (rc != GPK_OK) {
      for (int k = 0; k < r; ++k) gpk_destroy(out[k]);
      return rc;
    }
    LocalComm* c = new LocalComm();
    c->g = g;
    out[r]->comm = c;
  }
  return GPK_OK;
}

// one host thread per rank, eager launches (an in-process group cannot be graph-captured)
static int group_run(gpk_handle** hs, int nranks, int apply, int n_steps) {
  if (!hs || nranks < 1) return fail(GPK_EINVAL, "bad group");
  for (int r = 0; r < nranks; ++r)
    if (!hs[r] || !hs[r]->shard || hs[r]->comm->capturable() || hs[r]->rank != r || hs[r]->nranks != nranks)
      return fail(GPK_EINVAL, "not the handles of one gpk_group_create group, in rank order");
  std::vector<int> rcs(nranks, GPK_OK);
  std::vector<std::string> errs(nranks);
  std::vector<std::thread> th;
  for (int r = 0; r < nranks; ++r)
    th.emplace_back([&, r]() {
      gpk_handle* h = hs[r];
      DevSwitch ds(h->dev);
      // the batch begin: loss slot reset and the snapshot a failed batch is undone to
      int rc = check_launch(launch_step_begin(make_begin(h, false), h->s), "step_begin");
      for (int i = 0; i < n_steps && rc == GPK_OK; ++i) rc = enqueue_step_shard(h, apply);
      if (rc == GPK_OK && hipStreamSynchronize(h->s) != hipSuccess) rc = fail(GPK_EHIP, "group step sync");
      if (rc != GPK_OK) {
        errs[r] = gpk_last_error();  // (this thread's)
        static_cast<LocalComm*>(h->comm)->g->abort();
      }
      rcs[r] = rc;
    });
  for (auto& t : th) t.join();
  for (int r = 0; r < nranks; ++r)
    if (rcs[r] != GPK_OK) return fail(rcs[r], "rank " + std::to_string(r) + ": " + errs[r]);
  // every rank's status: the step makes it group-wide (its one all-reduce), so ranks that disagree
  // are an internal error.  A failed batch (non-PD factor, or a hand-off timeout: bit 2, raised by
  // one rank's wait and summed over the group) fails the whole group with GPK_ENOTPD; every rank
  // resets its hand-off slots and restores the batch's snapshot.
  std::vector<int> st(nranks, 0);
  int any = 0, bad = 0;
  for (int r = 0; r < nranks; ++r) {
    DevSwitch ds(hs[r]->dev);
    HIPCHK(hipMemcpy(&st[r], hs[r]->status, sizeof(int), hipMemcpyDeviceToHost));
    any |= st[r];
    bad += st[r] != 0;
  }
  if (!any) return GPK_OK;
  for (int r = 0; r < nranks; ++r) {  // every rank undoes the batch (gpk.h: failed batches are undone)
    DevSwitch ds(hs[r]->dev);
    TRY(status_recover(any, hs[r]->status, hs[r]->s, hs[r], true, true));
  }
  int r0 = 0;  // the first rank whose wait gave up
  while ((any & 2) && !(st[r0] & 2)) ++r0;
  if (!(any & 2) && bad != nranks)
    return fail(GPK_EINVAL, "internal: device status differs across the ranks of the group (" +
                                std::to_string(bad) + " of " + std::to_string(nranks) + ")");
  return fail(GPK_ENOTPD, status_message(any, true, r0));
}

int gpk_group_step(gpk_handle** hs, int32_t nranks, int32_t n_steps, double* losses) {
  if (n_steps < 0 || n_steps > LOSS_CAP) return fail(GPK_EINVAL, "n_steps must be in [0, 4096]");
  TRY(group_run(hs, nranks, 1, n_steps));
  if (losses && n_steps > 0) {
    DevSwitch ds(hs[0]->dev);
    HIPCHK(hipMemcpy(losses, hs[0]->losses, n_steps * sizeof(double), hipMemcpyDeviceToHost));
  }
  return GPK_OK;
}

int gpk_group_loss_grad(gpk_handle** hs, int32_t nranks, double* loss, double* grad_flat) {
  if (!loss) return fail(GPK_EINVAL, "NULL argument");
  TRY(group_run(hs, nranks, 0, 1));
  const Layout& L = hs[0]->L;
  DevSwitch ds(hs[0]->dev);
  HIPCHK(hipMemcpy(loss, hs[0]->diag, sizeof(double), hipMemcpyDeviceToHost));
  if (grad_flat) {  // small params from rank 0 (identical on every rank), U rows from their owner
    HIPCHK(hipMemcpy(grad_flat, hs[0]->grad, L.nparams * sizeof(double), hipMemcpyDeviceToHost));
    for (int r = 1; r < nranks; ++r) {
      const int r0 = r * hs[r]->h1, r1 = std::min(L.n1, r0 + hs[r]->h1);
      if (r0 >= r1) continue;
      HIPCHK(hipMemcpy(grad_flat + L.off_u + (size_t)r0 * L.n2, hs[r]->grad + L.off_u + (size_t)r0 * L.n2,
                       (size_t)(r1 - r0) * L.n2 * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  return GPK_OK;
}

int gpk_shard_plan(const gpk_handle* h, char* out, int64_t cap) {
  if (!h || !out || cap < 1) return fail(GPK_EINVAL, "NULL argument");
  if (!h->shard) return fail(GPK_EINVAL, "gpk_shard_plan: not a row-sharded handle");
  if ((int64_t)h->splan.size() + 1 > cap) return fail(GPK_EINVAL, "gpk_shard_plan: cap too small");
  std::memcpy(out, h->splan.c_str(), h->splan.size() + 1);
  return GPK_OK;
}

int gpk_shard_info(const gpk_handle* h, int32_t* rank, int32_t* nranks, int32_t* row0, int32_t* rows) {
  if (!h || !rank || !nranks || !row0 || !rows) return fail(GPK_EINVAL, "NULL argument");
  *rank = h->rank;
  *nranks = h->nranks;
  if (!h->shard) {
    *row0 = 0;
    *rows = h->L.n1;
    return GPK_OK;
  }
  *row0 = h->rank * h->h1;
  *rows = std::max(0, std::min(h->L.n1, *row0 + h->h1) - *row0);
  return GPK_OK;
}
