// gpk_host.h — what the host translation units of libgpk share (never included by device code):
// the solver handle, the error helpers, and the functions that cross translation units.
//   gpk_api.cpp     errors, device check, standalone kernels, predict / predict_deriv / evaluate,
//                   getters and setters
//   gpk_create.cpp  handle construction (validate, choose path, allocate, classes, upload), state
//   gpk_plan.cpp    the 2D step's GEMM plan (build_descs) and the descriptor helpers every unit
//                   shares: gemm_desc, with_side, refined_solve, refine_panel_desc
//   gpk_step.cpp    one step in stream order: argument fillers, the inverse, enqueue_step
//   gpk_batch.cpp   graph cache and capture, batch begin / report / rollback, status handling,
//                   gpk_step, gpk_prepare, gpk_loss_grad
//   gpk_shard.cpp   the row-sharded step and its collective backends (the only user of RCCL)
//   gpk_diag.cpp    measurement and diagnostic entry points (reached from no solver entry point),
//                   gpk_mode_gemm, gpk_refine_panel, gpk_point_contract and gpk_assemble_pairs among them
//   gpk_kron3.cpp   the 3-axis solver (step, predictions, scattered points, criterion, Adam state)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/gpk.h"
#include "eval_chunk.h"
#include "gpk_internal.h"
#include "stepk.h"

using namespace gpk;

// helpers and cross-unit functions stay out of the library's dynamic symbol table
#pragma GCC visibility push(hidden)
int fail(int code, const std::string& msg);  // sets gpk_last_error, returns code (gpk_api.cpp)
int check_launch(hipError_t e, const char* what);
int check_device(int dev);
// the axis constants of host kernel parameters, as the device derives them (gpk_api.cpp)
void host_axis_const(const double* logw, const double* logls, const double* freq, int q, AxisConst* kc);
#pragma GCC visibility pop

#define HIPCHK(x)                                                                      \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess)                                                              \
      return fail(e_ == hipErrorOutOfMemory ? GPK_ENOMEM : GPK_EHIP,                   \
                  std::string(#x) + ": " + hipGetErrorString(e_));                     \
  } while (0)

constexpr int LOSS_CAP = 4096;
constexpr int kMaxStages = 18;
constexpr int kGemmStages = 11;  // A, A_res, A_fix, B, B_res, B_fix, C, D, D_res, D_fix, E
constexpr int K3_MAX_N = 1024;   // 3-axis solver, per axis (the per-sweep inverse; 1024^3 is 8 GB)

// restore the caller's current device on scope exit
struct __attribute__((visibility("hidden"))) DevSwitch {
  int prev = -1;
  explicit DevSwitch(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~DevSwitch() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

struct Stage {
  int off = 0, n = 0, variant = 0;
  bool gated = false;  // every descriptor is a refinement GEMM (left out of the fast graph)
};

struct gpk_handle;
// collective backend of a row-sharded handle (RCCL, or an in-process group: gpk_shard.cpp)
struct ShardComm {
  virtual ~ShardComm() {}
  virtual int allgather(gpk_handle* h, double* buf, size_t chunk) = 0;  // in place
  virtual int allreduce(gpk_handle* h, double* buf, size_t n) = 0;      // in place, sum
  virtual int broadcast(gpk_handle* h, double* buf, size_t n, int root) = 0;  // in place
  virtual bool capturable() const = 0;
};
struct ShardGather {
  double* buf;
  size_t chunk;     // doubles per rank (a block of rows), rank r's block at buf + r * chunk
};

// A captured graph of the step: `reps` steps back to back with (refine, apply) -- or, whole, a
// call of its own: batch begin (snapshot, counters) + those steps + the pinned-memory report.
// Ordered so that the graphs of one (whole, refine, apply) are neighbours in ascending reps.
struct GraphKey {
  bool whole, refine;
  int apply, reps;
  bool operator<(const GraphKey& o) const {
    return std::tie(whole, refine, apply, reps) < std::tie(o.whole, o.refine, o.apply, o.reps);
  }
};

// What one enqueued step is asked to do beyond the step itself, and (StepDone) what it did.
struct StepCtx {
  int apply = 1;
  bool refine = true;     // false: the fast step (refinement stages left out, gates watched)
  // pipelined class values (TailArgs::nce_flag, cls_pipe_ok): the parameter-gradient launch of
  // step s of a captured batch evaluates step s + 1's class values after the kernel-parameter Adam
  bool have_cls = false;  // the previous enqueued step evaluated this one's: no class-value launch
  bool next_cls = false;  // this step evaluates the next one's
  const StepBegin* begin = nullptr;    // batch begin to fold into the chain launch (chain + classes)
  const StepReport* report = nullptr;  // batch report to fold into the loss workgroup
};
struct StepDone {
  bool next_cls = false, begin = false, report = false;
};

struct gpk_handle {
  gpk_problem prob{};
  double freq_scale = 0.0;
  Layout L{};
  AdamHyper hyper{};
  int dev = 0;
  hipStream_t s = nullptr;
  std::vector<void*> allocs;

  double *x1 = nullptr, *x2 = nullptr, *F = nullptr, *bvals = nullptr;
  int* bidx = nullptr;
  double *params = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr, *Up = nullptr;
  AxisConst* kc = nullptr;
  StepScalars* sc = nullptr;
  int *count = nullptr, *loss_slot = nullptr, *status = nullptr;
  double *losses = nullptr, *diag = nullptr;
  double* stat_x = nullptr;  // [2] status bits as doubles (split-factor group all-reduce)

  double *K[2] = {}, *Kb[2] = {}, *D[2] = {}, *Kinv[2] = {}, *piv[2] = {}, *ldet[2] = {};
  int nldet[2] = {0, 0};
  // 2D work
  double *A = nullptr, *Bt = nullptr, *S = nullptr, *R = nullptr, *T1 = nullptr, *T2 = nullptr,
         *X1 = nullptr, *X2 = nullptr, *W1 = nullptr, *W2 = nullptr;  // W: refinement residuals
  double *Y1 = nullptr, *Y2 = nullptr;  // S/2 + v X1, S/2 + v X2 (the G_K operands)
  double *GK[2] = {}, *GD[2] = {};
  // 2D class path: class tile partials of G_K / G_D written by their GEMM epilogues
  // ([class_slots(P/16)][ncls] per axis; GemmDesc::cpart); cp_on: the stages use them
  double *cpK[2] = {}, *cpD[2] = {};
  bool cp_on = false;
  // 1D work
  double *alpha = nullptr, *tvec = nullptr, *beta = nullptr;
  double *red_quad = nullptr, *red_egap = nullptr;
  int nquad = 0, negap = 0;
  double *pgpart = nullptr, *pg = nullptr;
  double *pgpart_lo = nullptr, *tgpart_lo = nullptr;  // DD contraction (pg_dd): low parts
  bool pg_dd = false;                 // kernel-parameter contraction in double-double
  int bpa = 0;
  // fused step tail (pgrad launch): group counters / partials, boundary gap
  unsigned int *tcount = nullptr, *ttop = nullptr;
  double *tgpart = nullptr, *bgap = nullptr;
  int bgap_parts = 1;                 // PrepArgs::bgap_parts
  int ttg = 0, tngpa = 0;
  std::vector<GemmDesc> hdescs;  // per-stage GEMM descriptors (kernel arguments)
  Stage st[kGemmStages];
  double *Kc[2] = {}, *pst[2] = {};  // kept K (refinement residuals), pivot stats (gate)
  unsigned int* aflag[2] = {};        // assembly -> pivot-0 hand-off counters (small path) /
                                      // update -> pivot hand-off counters (large path)
  bool bigspd = false;                // large-factor SPD inverse (spdinv_big.hip)
  bool bigwide = false;               // ... with 128-wide sweeps
  bool chain_multi = false;           // persistent inverse on macro tiles (large 1D factors)
  // large 1D factors with distance classes: the GEMVs read Kc and D as class ids + class values
  // (GemvDesc::cid), so the inverse launch's gather writes neither matrix (64 MB at C2)
  bool cls_gemv = false;
  double* Zp[2] = {};                 // ... its panel buffers [3][128][P] (by sweep mod 3)
  unsigned* wsched[2] = {};           // ... its update schedule (wide_schedule; unpaired under GPK_FLAG_ONE_SWEEP_UPDATE)
  bool chain = false;                 // small factors: persistent one-launch inverse (chain_kernel)
  bool chain_aug = false;             // ... which also solves A, Bt^T and K^{-1} D^T (2D, unsharded)
  unsigned int* cflags[2] = {};       // its hand-off flags [T*(T+taug) + 2T + 1] per factor
  double* cgran[2] = {};              // its pivot-chain input slots [T][3][1024] per factor
  double* PB2[2] = {};                // chain_multi: panel slots [2][P*P] by launch parity
  unsigned int* cepoch[2] = {};       // launch counter + arrival count per factor [CHAIN_EPOCH_WORDS]
  double *PD[2] = {}, *PBa[2] = {};   // K_a^{-1} D_a^T; augmented panel buffers
  ClassArgs cls[2] = {};              // distance classes per axis (ncls = 0: per-pair path)
  double* rvec = nullptr;            // 1D refinement residual
  double* uoff = nullptr;            // 1D Allen-Cahn offset (gpk_problem.uoff), or null
  // predict scratch
  GemmDesc* pdescs = nullptr;

  // row-sharded step: this rank computes rows [rank*h, (rank+1)*h) of every GEMM output
  bool shard = false;
  int rank = 0, nranks = 1;
  int split_axis = -1;                // GPK_FLAG_SPLIT_FACTORS: the factor this rank inverts
  int h1 = 0, h2 = 0;                 // row-block heights of the P1- and P2-row outputs
  ShardComm* comm = nullptr;
  std::vector<GemmDesc> sdescs;       // row slices of hdescs
  Stage sst[kGemmStages];
  std::vector<ShardGather> sgather[kGemmStages];
  // the one per-step all-reduce of a sharded handle: [status (2) | pg | egap | quad] contiguous
  double* sred = nullptr;
  std::string splan;                  // the step's shard plan (gpk_shard_plan; gpk/shard.py)

  // every captured graph of this handle (gpk_batch.cpp step_graph: captured on first use, or by
  // gpk_prepare).  Plain graphs exist at reps 1, at STEP_GRAPH_REPS (one host launch per group of
  // steps: a graph launch boundary costs ~5-9 us of idle GPU) and at the chunk sizes of a prepared
  // call; whole-call graphs at reps 1 (one step(1) call as one launch and one wait: the
  // reference's one-call-per-iteration loop shape) and, fast only, at the prepared chunk sizes.
  std::map<GraphKey, hipGraphExec_t> graphs;
  bool fast_ok = false;    // the fast graph exists for this handle (not row-sharded)
  int fast_mode = 0;       // next step(s) run the fast graph (gate closed with margin last time)
  long long rollbacks = 0;
  double* snap = nullptr;  // [3 * nparams] params, m, v at the start of a fast batch
  int* snap_count = nullptr;
  unsigned int* viol = nullptr;  // the fast graph met an open refinement gate
  unsigned int* nce_flag = nullptr;  // raised by the Adam block, reset by the next publish_prep
  double* nce_kp = nullptr;          // [nsmall] the kernel parameters it hands over (sc1)
  double* rep_host = nullptr;    // [8 + LOSS_CAP] pinned: status, viol, gates, losses (step_report)
  hipEvent_t ev[kMaxStages + 1] = {};
  bool profiling = false;
  int nstage = 0;
  const char* sname[kMaxStages] = {};  // name of each launched (profiled) stage
};

#define TRY(x)                  \
  do {                          \
    int r_ = (x);               \
    if (r_ != GPK_OK) return r_; \
  } while (0)

// zero-filled device memory, freed with its handle (every pointer in `allocs`)
template <class T>
int dev_alloc(std::vector<void*>& allocs, hipStream_t s, T** p, size_t count) {
  void* q = nullptr;
  const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return fail(GPK_ENOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  e = hipMemsetAsync(q, 0, bytes, s);
  if (e != hipSuccess) return fail(GPK_EHIP, hipGetErrorString(e));
  allocs.push_back(q);
  *p = static_cast<T*>(q);
  return GPK_OK;
}

// Device scratch of one call (handle lifetime: dev_alloc).  Every block is freed on scope exit,
// whichever return ends the scope -- after `s` has drained when the call enqueues work on a stream
// (what it enqueued may still read the blocks).  Both methods return the library's status, with
// gpk_last_error set and GPK_ENOMEM for an allocation the device cannot serve.
class __attribute__((visibility("hidden"))) CallScratch {
 public:
  explicit CallScratch(const char* who, hipStream_t s = nullptr) : who_(who), s_(s) {}
  CallScratch(const CallScratch&) = delete;
  CallScratch& operator=(const CallScratch&) = delete;
  ~CallScratch() {
    if (s_) (void)hipStreamSynchronize(s_);
    for (void* p : mem_) (void)hipFree(p);
  }
  // n elements (at least 16 bytes), zero-filled in the order of `s` when asked
  template <class T>
  int alloc(T** p, size_t n, bool zero = false) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(n * sizeof(T), 16);
    const hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(e == hipErrorOutOfMemory ? GPK_ENOMEM : GPK_EHIP,
                  std::string(who_) + ": hipMalloc failed: " + hipGetErrorString(e));
    }
    mem_.push_back(q);
    *p = static_cast<T*>(q);
    return zero ? check_launch(hipMemsetAsync(q, 0, bytes, s_), who_) : GPK_OK;
  }
  // n elements copied from the host array before the call returns
  template <class T>
  int upload(T** p, const T* src, size_t n) {
    TRY(alloc(p, n));
    return check_launch(hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice), who_);
  }

 private:
  const char* who_;
  hipStream_t s_;
  std::vector<void*> mem_;
};

// padded size, size and coordinates of axis a (0 or 1)
inline int axis_p(const Layout& L, int a) { return a ? L.p2 : L.p1; }
inline int axis_n(const Layout& L, int a) { return a ? L.n2 : L.n1; }
inline const double* axis_x(const gpk_handle* h, int a) { return a ? h->x2 : h->x1; }
inline int step_deriv(const gpk_handle* h) { return h->prob.eq == GPK_ADVECTION ? 1 : 2; }

#pragma GCC visibility push(hidden)
// gpk_create.cpp
bool build_classes(const double* x, int n, int P, std::vector<double>& dist, std::vector<int>& cid,
                   std::vector<int>& cbase, int& vmax);
int create_impl(const gpk_problem* p, double freq_scale, int rank, int nranks, bool shard,
                gpk_handle** out, bool local_group = false);
// gpk_plan.cpp
GemmDesc gemm_desc(const double* A, int lda, int ta, const double* B, int ldb, int tb, double* C,
                   int ldc, int M, int N, int K);  // C = op(A) op(B), stored
GemmDesc with_side(GemmDesc g, double* Y, const double* Ys, int ldy);  // + Y = Ys / 2 + v C
// One solve against K with its refinement step, X and B rows x cols and K of order rows (K on the
// left, right = 0: X = K^{-1} B) or cols (right = 1: X = B K^{-1}); every operand row-major and
// contiguous.  solve: X = K^{-1} B;  resid: W = B - Kc X;  fix: X += K^{-1} W in place -- the
// last two gated on `gate` (nullable: always run).
struct RefinedSolve {
  GemmDesc solve, resid, fix;
};
RefinedSolve refined_solve(bool right, const double* Kc, const double* Kinv, const double* B, double* X,
                           double* W, int rows, int cols, const double* gate);
// the same refinement step as one fused panel launch (refine_panel.hip; P <= REFINE_PANEL_MAX_P)
RefinePanel refine_panel_desc(bool right, const double* Kc, const double* Kinv, const double* B, double* X,
                              int rows, int cols, const double* gate);
int gemm_force(int flags);
int build_descs(gpk_handle* h);
// gpk_step.cpp: argument fillers and the enqueue of one step
PrepArgs make_prep(gpk_handle* h, int apply);
bool cls_pipe_ok(const gpk_handle* h);
void fill_spd(gpk_handle* h, SpdArgs* sa);
void fill_assemble(const gpk_handle* h, AssembleArgs* aa);  // base fields: callers add their own
void fill_pgrad2d(const gpk_handle* h, PGradArgs* pa);       // base fields: callers add their own
hipError_t launch_chain(gpk_handle* h, bool gather, double** fin, bool aug = true,
                        const PrepArgs* prep = nullptr);
hipError_t launch_inverse(gpk_handle* h, SpdArgs* sa, double** fin, bool pivot0_done);
hipError_t launch_gemm_stage(gpk_handle* h, int k);  // stage k of the unsharded 2D plan
int enqueue_assemble_inverse(gpk_handle* h, const StepCtx& c, StepDone* done = nullptr);
TailArgs make_tail(gpk_handle* h, const StepCtx& c);
void gemv_operand(const gpk_handle* h, GemvDesc& g);
int enqueue_step(gpk_handle* h, const StepCtx& c, StepDone* done = nullptr);
// gpk_batch.cpp: capture, the batch protocol, device status
int capture_graph(hipStream_t s, hipGraphExec_t* slot, const std::function<int()>& body);
StepBegin make_begin(gpk_handle* h, bool fast);
std::string status_message(int st, bool handoffs, int rank = -1);
int status_recover(int st, int* status, hipStream_t s, gpk_handle* h, bool undo_batch, bool handoffs);
int status_error(int st, int* status, hipStream_t s, gpk_handle* h, bool undo_batch, bool handoffs);
int read_status(gpk_handle* h);
// gpk_shard.cpp
int build_shard(gpk_handle* h);
int split_broadcast(gpk_handle* h);
int enqueue_step_shard(gpk_handle* h, int apply);
#pragma GCC visibility pop
