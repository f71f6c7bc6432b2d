// gpk_batch.cpp — how a handle's steps run: the graph cache and capture, the batch begin /
// report / rollback protocol, device status as an error, and the entry points on top of them
// (gpk_step, gpk_prepare, gpk_loss_grad, gpk_set_wait_limit[_chunk]).  What one step enqueues is
// gpk_step.cpp's.
#include <sched.h>

#include <atomic>

#include "gpk_host.h"

// ------------------------------------------------------------------------------------------
// graph capture
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

constexpr int STEP_GRAPH_REPS = 8;
// Fast batches run in chunks of FAST_CHUNK steps, each checked at its end: a step that met an
// open refinement gate costs a rerun of its chunk only (not of the whole call -- at C3 the
// gate opens mid-training, and a 300-step call used to run twice).  Also the largest prepared
// graph.
constexpr int FAST_CHUNK = 64;

static GraphKey plain_key(bool fast, int apply, int reps) { return GraphKey{false, !fast, apply, reps}; }
static GraphKey whole_key(bool fast, int reps) { return GraphKey{true, !fast, 1, reps}; }

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

// `reps` steps back to back, each evaluating the next one's class values (cls_pipe_ok decides).
// begin / report: folded into the first / last step where the step can carry them; *folded says
// which were.
static int enqueue_steps(gpk_handle* h, int apply, bool refine, int reps, const StepBegin* begin,
                         const StepReport* report, StepDone* folded) {
  StepCtx c;
  c.apply = apply;
  c.refine = refine;
  for (int r = 0; r < reps; ++r) {
    c.next_cls = r + 1 < reps;
    c.begin = r == 0 ? begin : nullptr;
    c.report = r == reps - 1 ? report : nullptr;
    StepDone d;
    TRY(enqueue_step(h, c, &d));
    c.have_cls = d.next_cls;
    folded->begin |= d.begin;
    folded->report |= d.report;
  }
  return GPK_OK;
}

// A whole call: the batch begin (folded into the first step's chain launch when that launch
// publishes the step constants -- publish_prep, copy_snapshot -- else its own launch), `reps`
// steps, and the report (written by the last step's loss workgroup, else by its own launch after
// it: a sharded step).
static int enqueue_call(gpk_handle* h, const StepBegin& b, const StepReport& rep, bool refine, int reps) {
  const bool fold = !h->shard && h->chain && h->cls[0].ncls > 0;
  if (!fold) TRY(check_launch(launch_step_begin(b, h->s), "step_begin"));
  StepDone folded;
  TRY(enqueue_steps(h, 1, refine, reps, fold ? &b : nullptr, &rep, &folded));
  if (fold && !folded.begin) return fail(GPK_EINVAL, "internal: the batch begin was not folded into a step");
  if (!folded.report) return check_launch(launch_step_report(rep, h->s), "step_report");
  return GPK_OK;
}

// The executable of graph k, captured on first use.  It enters the cache only once it has been
// instantiated, so a failed capture leaves nothing behind and every entry can be launched.
static int step_graph(gpk_handle* h, const GraphKey& k, hipGraphExec_t* out = nullptr) {
  auto it = h->graphs.find(k);
  if (it == h->graphs.end()) {
    if (h->shard && !h->comm->capturable())
      return fail(GPK_EINVAL, "handle belongs to an in-process rank group: use gpk_group_step / gpk_group_loss_grad");
    hipGraphExec_t g = nullptr;
    TRY(capture_graph(h->s, &g, [&] {
      if (k.whole)
        return enqueue_call(h, make_begin(h, !k.refine), make_report(h, !k.refine, k.reps), k.refine, k.reps);
      StepDone none;
      return enqueue_steps(h, k.apply, k.refine, k.reps, nullptr, nullptr, &none);
    }));
    it = h->graphs.emplace(k, g).first;
  }
  if (out) *out = it->second;
  return GPK_OK;
}

// ------------------------------------------------------------------------------------------
// device status
// ------------------------------------------------------------------------------------------
// After a launch whose hand-off wait gave up (status bit 2), a late producer may still have
// stored real words into hand-off slots the consumer had already consumed and reset: restore
// every slot, flag and counter to its create-time state (the stream is synchronised, so every
// launch has drained) before the handle is used again -- stale words would otherwise pass for
// the next launch's inputs.
static int reset_handoffs(gpk_handle* h) {
  const Layout& L = h->L;
  for (int a = 0; a < L.naxes; ++a) {
    const size_t P = axis_p(L, a), T = P / 32;
    const size_t nflags = T * (T + (L.p1 + L.p2) / 32) + 2 * T + 1;
    HIPCHK(hipMemsetD32Async(h->cgran[a], CHAIN_SENTINEL32, T * 6144, h->s));
    if (h->PB2[a]) HIPCHK(hipMemsetD32Async(h->PB2[a], CHAIN_SENTINEL32, 4 * chain_half((int)P, h->chain_multi), h->s));
    if (h->cepoch[a]) HIPCHK(hipMemsetAsync(h->cepoch[a], 0, CHAIN_EPOCH_WORDS * sizeof(unsigned int), h->s));
    HIPCHK(hipMemsetAsync(h->cflags[a], 0, nflags * sizeof(unsigned int), h->s));
    HIPCHK(hipMemsetAsync(h->aflag[a], 0, (4 + P / 32) * sizeof(unsigned int), h->s));
  }
  HIPCHK(hipMemsetAsync(h->nce_flag, 0, sizeof(unsigned int), h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  return GPK_OK;
}

// params, Adam state and step count back to the snapshot the current batch's begin took (every
// gpk_step batch takes one), U's padded copy rebuilt from params: a fast batch that met an open
// refinement gate is rerun from there, a batch that failed on the device is undone
static int restore_snapshot(gpk_handle* h) {
  const size_t np = (size_t)h->L.nparams, nb = np * sizeof(double);
  HIPCHK(hipMemcpyAsync(h->params, h->snap, nb, hipMemcpyDeviceToDevice, h->s));
  HIPCHK(hipMemcpyAsync(h->m, h->snap + np, nb, hipMemcpyDeviceToDevice, h->s));
  HIPCHK(hipMemcpyAsync(h->v, h->snap + 2 * np, nb, hipMemcpyDeviceToDevice, h->s));
  HIPCHK(hipMemcpyAsync(h->count, h->snap_count, sizeof(int), hipMemcpyDeviceToDevice, h->s));
  return check_launch(launch_sync_u(h->params, h->L, h->Up, h->s), "sync_u");
}

// A non-zero device status word `st` in words.  handoffs: bit 2 (a hand-off wait gave up) is
// told apart; rank >= 0: the rank of a group that raised it.
std::string status_message(int st, bool handoffs, int rank) {
  if (!(handoffs && (st & 2)))
    return "covariance factor is not positive definite (non-positive pivot in SPD inverse)";
  return "SPD inverse: a pivot-chain hand-off timed out (device status 2" +
         (rank >= 0 ? ", rank " + std::to_string(rank) : std::string()) + ")";
}

// ... and the handle made usable again: the word is cleared; on bit 2 the hand-off slots are
// reset; undo_batch: the handle goes back to the snapshot its batch begin took.  h may be null
// without either flag (the 3-axis solver has its own handle and neither hand-offs nor batches).
int status_recover(int st, int* status, hipStream_t s, gpk_handle* h, bool undo_batch, bool handoffs) {
  HIPCHK(hipMemsetAsync(status, 0, sizeof(int), s));
  if (handoffs && (st & 2)) TRY(reset_handoffs(h));
  if (undo_batch) {
    TRY(restore_snapshot(h));
    HIPCHK(hipStreamSynchronize(s));
  }
  return GPK_OK;
}

// ... both: the status word as the error return
int status_error(int st, int* status, hipStream_t s, gpk_handle* h, bool undo_batch, bool handoffs) {
  TRY(status_recover(st, status, s, h, undo_batch, handoffs));
  const std::string msg = status_message(st, handoffs);
  return fail(GPK_ENOTPD, undo_batch ? msg + "; the batch was undone" : msg);
}

int read_status(gpk_handle* h) {
  int st = 0;
  HIPCHK(hipMemcpyAsync(&st, h->status, sizeof(int), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  return st ? status_error(st, h->status, h->s, h, false, true) : GPK_OK;
}

// ------------------------------------------------------------------------------------------
// the batch protocol
// ------------------------------------------------------------------------------------------
// End of a batch (one synchronisation): non-positive-definite status, the fast graph's gate
// violation flag, and the refinement gate of the last step, which picks the next batch's graph:
// the fast one once max_a K00 * max diag K_a^{-1} is 2x below REFINE_COND_LB, and it stays
// the fast one while that bound stays below REFINE_COND_LB itself (hysteresis: a fast batch
// that crosses the gate is caught by the check in the fast graph's tail (viol) and rerun, which
// costs one FAST_CHUNK; leaving the fast graph at the margin cost ~15% on every later step of
// C4's training, whose bound drifts to ~21 (tools/train_regime_parity.py): round 4's 8x entry
// margin (12.5) kept a handle that had left the fast graph off it for ~2000 steps).
constexpr double FAST_GRAPH_MARGIN = 2.0;

// the report written by step_report_kernel (the host has seen it complete); its first n losses
// go to `losses` (nullable)
static int read_report(gpk_handle* h, bool fast, double* losses, int n, bool* violated) {
  if (losses) std::memcpy(losses, h->rep_host + 8, n * sizeof(double));
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

static int finish_batch(gpk_handle* h, bool fast, double* losses, int n, bool* violated) {
  TRY(check_launch(launch_step_report(make_report(h, fast, losses ? n : 0), h->s), "step_report"));
  HIPCHK(hipStreamSynchronize(h->s));
  return read_report(h, fast, losses, n, violated);
}

// n training steps as plain graphs, in pieces of LOSS_CAP (the device loss buffer).  Every piece
// but the last copies its losses out itself; the last one's come back with the batch report:
// *last, *nlast.  reset_slot: the first piece restarts the loss slot (a batch begin has not).
static int run_steps(gpk_handle* h, int n_steps, double* losses, bool fast, bool reset_slot,
                     double** last, int* nlast) {
  if (!h->shard && n_steps >= STEP_GRAPH_REPS) TRY(step_graph(h, plain_key(fast, 1, STEP_GRAPH_REPS)));
  for (int done = 0; done < n_steps;) {
    const int nb = std::min(LOSS_CAP, n_steps - done);
    if (reset_slot || done > 0) HIPCHK(hipMemsetAsync(h->loss_slot, 0, sizeof(int), h->s));
    // the largest graph that fits what is left: a prepared size, STEP_GRAPH_REPS, one step (the
    // single-step graph exists: run_batch, so the walk stays among this mode's graphs and ends)
    for (int r = nb; r > 0;) {
      const auto it = std::prev(h->graphs.upper_bound(plain_key(fast, 1, r)));
      HIPCHK(hipGraphLaunch(it->second, h->s));
      r -= it->first.reps;
    }
    if (losses && done + nb < n_steps) {
      HIPCHK(hipMemcpyAsync(losses + done, h->losses, nb * sizeof(double), hipMemcpyDeviceToHost, h->s));
    } else if (losses) {
      *last = losses + done;
      *nlast = nb;
    }
    done += nb;
  }
  return GPK_OK;
}

// A whole-call graph ends its report with the ready word rep_host[7] (stepk_dev.h report_ready):
// the host waits for that word instead of the stream, so gpk_step returns as soon as the call's
// losses and status are final -- the last step's dL/dU and Adam on U may still run, ordered
// before anything later enqueued on the handle's stream.  The wait polls the stream every few
// thousand reads, so a faulted or finished-without-report stream ends it.
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

// One batch as its caller sees it: n training steps and their losses (nullable), or, apply = 0,
// the loss and gradient of the current parameters (n = 1).
struct Batch {
  int apply, n;
  double* losses;   // apply = 1: [n]
  bool whole_call;  // a gpk_step(1) call on an unsharded handle: one graph launch, one wait
  double *loss, *grad;  // apply = 0 (grad nullable)
};

// Run batch b on the fast or the full graph; *violated: a fast step met an open refinement gate,
// so nothing the batch did counts.  rerun: the batch follows a violated run of itself.
static int run_batch(gpk_handle* h, const Batch& b, bool fast, bool rerun, bool* violated) {
  // one whole-call graph: a one-step call (either graph, captured on first use), or a fast chunk
  // of the size gpk_prepare captured (a one-step chunk of a longer call is not such a chunk)
  hipGraphExec_t g = nullptr;
  if (b.whole_call) {
    TRY(step_graph(h, whole_key(fast, 1), &g));
  } else if (b.apply && fast && !h->shard && b.n > 1) {
    const auto it = h->graphs.find(whole_key(true, b.n));
    if (it != h->graphs.end()) g = it->second;
  }
  if (g) {
    reinterpret_cast<volatile double*>(h->rep_host)[7] = 0.0;  // (wait_report's ready word)
    HIPCHK(hipGraphLaunch(g, h->s));
    TRY(wait_report(h));
    return read_report(h, fast, b.losses, b.n, violated);
  }
  TRY(step_graph(h, plain_key(fast, b.apply, 1), &g));
  double* last = nullptr;
  int nlast = 0;
  if (b.apply) {
    // the snapshot of everything a batch carries forward (Up is rebuilt from params), the
    // violation flag and the loss slot: one launch.  A rerun keeps it (its steps start from the
    // restored snapshot) and restarts the loss slot alone
    if (!rerun) TRY(check_launch(launch_step_begin(make_begin(h, fast), h->s), "step_begin"));
    TRY(run_steps(h, b.n, b.losses, fast, rerun, &last, &nlast));
  } else {  // nothing is applied, so nothing to snapshot: the violation flag and the loss slot
    StepBegin sb{};
    sb.viol = fast ? h->viol : nullptr;
    sb.loss_slot = h->loss_slot;
    TRY(check_launch(launch_step_begin(sb, h->s), "step_begin"));
    HIPCHK(hipGraphLaunch(g, h->s));
    HIPCHK(hipMemcpyAsync(b.loss, h->diag, sizeof(double), hipMemcpyDeviceToHost, h->s));
    if (b.grad)
      HIPCHK(hipMemcpyAsync(b.grad, h->grad, h->L.nparams * sizeof(double), hipMemcpyDeviceToHost, h->s));
  }
  return finish_batch(h, fast, last, nlast, violated);
}

// ... in the handle's current mode; a fast batch that needed refinement is rolled back (training
// steps: to the snapshot its begin took; apply = 0 leaves params and Adam state alone) and rerun
// with the full graph
static int run_rolled_back(gpk_handle* h, const Batch& b) {
  bool viol = false;
  TRY(run_batch(h, b, h->fast_ok && h->fast_mode, false, &viol));
  if (!viol) return GPK_OK;
  ++h->rollbacks;
  if (b.apply) TRY(restore_snapshot(h));
  return run_batch(h, b, false, true, &viol);
}

int gpk_loss_grad(gpk_handle* h, double* loss, double* grad_flat) {
  if (!h || !loss) return fail(GPK_EINVAL, "NULL argument");
  DevSwitch ds(h->dev);
  return run_rolled_back(h, Batch{/*apply=*/0, 1, nullptr, false, loss, grad_flat});
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
  if (n_steps == 1 && !h->shard) return run_rolled_back(h, Batch{1, 1, losses, /*whole_call=*/true});
  int done = 0;
  for (int chunk = 0; done < n_steps; ++chunk) {
    ChunkWaitLimit chunk_limit(h, chunk);  // (tests: gpk_set_wait_limit_chunk; spans a rerun)
    // (both graphs run in FAST_CHUNK chunks while the fast graph is available, so the mode is
    // re-decided every 64 steps: a long first call on the full graph used to keep its whole
    // length there, and the training that followed, until the gate bound fell below the entry
    // margin -- round 4's W = 200 line at 8100 it/s.  Without a fast graph the call is one batch)
    const int n = h->fast_ok ? std::min(FAST_CHUNK, n_steps - done) : n_steps - done;
    TRY(run_rolled_back(h, Batch{1, n, losses ? losses + done : nullptr, false}));
    done += n;
  }
  return GPK_OK;
}

// Every graph a gpk_step(n_steps) call can launch, on either graph kind, captured ahead of it.
int gpk_prepare(gpk_handle* h, int32_t n_steps) {
  if (!h) return fail(GPK_EINVAL, "NULL handle");
  if (n_steps < 0) return fail(GPK_EINVAL, "n_steps < 0");
  if (h->shard && !h->comm->capturable()) return GPK_OK;  // in-process groups run eagerly
  DevSwitch ds(h->dev);
  for (const bool fast : {true, false}) {
    if (fast && !h->fast_ok) continue;
    TRY(step_graph(h, plain_key(fast, 1, 1)));
    if (h->shard) continue;  // (no multi-step and no whole-call graphs)
    TRY(step_graph(h, whole_key(fast, 1)));
    if (n_steps >= STEP_GRAPH_REPS) TRY(step_graph(h, plain_key(fast, 1, STEP_GRAPH_REPS)));
    // the chunks of the call: FAST_CHUNK-step chunks + the remainder whenever the fast graph
    // exists (fast_ok), on either graph -- each chunk is a batch of its own (snapshot, report,
    // undo on failure); without a fast graph the whole call is one batch, run as FAST_CHUNK-step
    // graphs + the remainder.  One plain graph each above STEP_GRAPH_REPS; fast chunks also as
    // whole-call graphs (begin + steps + report: one launch and one wait per chunk)
    for (const int reps : {std::min(n_steps, FAST_CHUNK), n_steps % FAST_CHUNK}) {
      if (reps > STEP_GRAPH_REPS) TRY(step_graph(h, plain_key(fast, 1, reps)));
      if (fast && reps > 1) TRY(step_graph(h, whole_key(true, reps)));
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
