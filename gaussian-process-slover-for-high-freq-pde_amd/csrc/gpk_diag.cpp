// gpk_diag.cpp — measurement and diagnostic entry points: per-stage and per-kernel timing, the
// forward fields, the standalone GEMM (plain and with the step's epilogues), GEMV, mode-k product
// and refinement step, the trace hooks.  No
// solver entry point (gpk_create, gpk_step, gpk_prepare, gpk_loss_grad, gpk_predict, gpk_*3)
// reaches this file, and it reaches the step only through the functions gpk_host.h declares.
#include "gpk_host.h"
#include "gpk_kron3.h"
#include "gpk_trace.h"
#include "fields_dd.h"

namespace {

// gpk_fields_dd: one thread per distance, the call pgrad_kernel's DD loop makes (pgrad.hip);
// row e of hi / lo = the high / low parts of (f_w, f_l, f_f, d_w, d_l, d_f)
template <bool MATERN, bool COS, int DERIV>
__global__ void fields_dd_kernel(const double* __restrict__ d, int n, double a, double om, double oml,
                                 double* __restrict__ hi, double* __restrict__ lo) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  dd::D F[6];
  fields_dd<MATERN, COS, DERIV>(d[e], a, om, oml, F[0], F[1], F[2], F[3], F[4], F[5]);
#pragma unroll
  for (int x = 0; x < 6; ++x) {
    hi[(size_t)e * 6 + x] = F[x].h;
    lo[(size_t)e * 6 + x] = F[x].l;
  }
}

template <bool MATERN, bool COS>
hipError_t launch_fields_dd(int deriv, const double* d, int n, double a, double om, double oml, double* hi,
                            double* lo) {
  const dim3 grid((n + 63) / 64), block(64);
  if (deriv == 2)
    hipLaunchKernelGGL((fields_dd_kernel<MATERN, COS, 2>), grid, block, 0, 0, d, n, a, om, oml, hi, lo);
  else
    hipLaunchKernelGGL((fields_dd_kernel<MATERN, COS, 1>), grid, block, 0, 0, d, n, a, om, oml, hi, lo);
  return hipGetLastError();
}

struct EventPair {  // two HIP events, destroyed on every path
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  hipError_t create() {
    const hipError_t e = hipEventCreate(&e0);
    return e != hipSuccess ? e : hipEventCreate(&e1);
  }
  hipError_t elapsed_us(double* us) {  // waits for e1
    float ms = 0.f;
    hipError_t e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    *us = ms * 1000.0;
    return e;
  }
};

// `warm` untimed launches, then `iters` launches back to back between two events: their average
hipError_t time_launches(hipStream_t s, int iters, int warm, const std::function<hipError_t()>& body,
                         double* avg_us) {
  EventPair ev;
  hipError_t e = ev.create();
  for (int it = 0; it < warm && e == hipSuccess; ++it) e = body();
  if (e == hipSuccess) e = hipEventRecord(ev.e0, s);
  for (int it = 0; it < iters && e == hipSuccess; ++it) e = body();
  if (e == hipSuccess) e = hipEventRecord(ev.e1, s);
  double us = 0.0;
  if (e == hipSuccess) e = ev.elapsed_us(&us);
  if (e == hipSuccess) *avg_us = us / iters;  // (untouched on failure)
  return e;
}

// `warm` + `iters` rounds of an untimed `prime` and a `timed` region between two events, one
// synchronisation per round: the total of the last `iters` timed regions
int time_each(hipStream_t s, int iters, int warm, const std::function<int()>& prime,
              const std::function<int()>& timed, double* total_us) {
  EventPair ev;
  HIPCHK(ev.create());
  *total_us = 0.0;
  for (int it = 0; it < warm + iters; ++it) {
    TRY(prime());
    HIPCHK(hipEventRecord(ev.e0, s));
    TRY(timed());
    HIPCHK(hipEventRecord(ev.e1, s));
    double us = 0.0;
    HIPCHK(ev.elapsed_us(&us));
    if (it >= warm) *total_us += us;
  }
  return GPK_OK;
}

}  // namespace

int gpk_trace_reset(void) {
  trace_reset_assemble();
  trace_reset_spdinv();
  trace_reset_pgrad();
  trace_reset_gemm();
  trace_reset_spdbig();
  return GPK_OK;
}

int gpk_trace_read(uint64_t* lo, uint64_t* hi, int32_t n) {
  if (!lo || !hi || n < TRACE_SLOTS) return fail(GPK_EINVAL, "need TRACE_SLOTS (256) slots");
  uint64_t l[5][TRACE_SLOTS], h[5][TRACE_SLOTS];
  trace_fetch_assemble(l[0], h[0]);
  trace_fetch_spdinv(l[1], h[1]);
  trace_fetch_pgrad(l[2], h[2]);
  trace_fetch_gemm(l[3], h[3]);
  trace_fetch_spdbig(l[4], h[4]);
  for (int i = 0; i < TRACE_SLOTS; ++i) {
    lo[i] = l[0][i];
    hi[i] = h[0][i];
    for (int u = 1; u < 5; ++u) {
      lo[i] = std::min(lo[i], l[u][i]);
      hi[i] = std::max(hi[i], h[u][i]);
    }
  }
#ifdef GPK_TRACE
  return GPK_OK;
#else
  return fail(GPK_EINVAL, "built without GPK_TRACE (make trace -> libgpk_trace.so)");
#endif
}

int gpk_profile_stages(gpk_handle* h, int32_t iters, double* out_us, int32_t cap, int32_t* n) {
  if (!h || !out_us || !n || iters <= 0) return fail(GPK_EINVAL, "bad argument");
  DevSwitch ds(h->dev);
  std::vector<double> acc(kMaxStages, 0.0);
  // run on a copy of the state: save params + opt state, restore afterwards
  const int64_t np = h->L.nparams;
  std::vector<double> p(np), mu(np), nu(np);
  int64_t cnt = 0;
  TRY(gpk_get_params(h, p.data(), np));
  TRY(gpk_get_opt_state(h, &cnt, mu.data(), nu.data(), np));
  h->profiling = true;
  for (int it = 0; it < iters; ++it) {
    HIPCHK(hipMemsetAsync(h->loss_slot, 0, sizeof(int), h->s));
    int rc = enqueue_step(h, StepCtx{});  // (a full step with apply = 1 that folds nothing)
    if (rc) { h->profiling = false; return rc; }
    HIPCHK(hipStreamSynchronize(h->s));
    for (int k = 0; k < h->nstage; ++k) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
      acc[k] += ms * 1000.0;
    }
  }
  h->profiling = false;
  TRY(gpk_set_params(h, p.data(), np));
  TRY(gpk_set_opt_state(h, cnt, mu.data(), nu.data(), np));
  const int ns = std::min<int>(h->nstage, cap);
  for (int k = 0; k < ns; ++k) out_us[k] = acc[k] / iters;
  *n = ns;
  return read_status(h);
}

const char* gpk_stage_name(const gpk_handle* h, int32_t stage) {
  if (!h || stage < 0) return "?";
  if (stage >= h->nstage || stage >= kMaxStages || !h->sname[stage]) return "?";
  return h->sname[stage];
}

// the per-pair assembly of K and D into the handle's buffers (no kept copy, no classes)
static int assemble_plain(gpk_handle* h, const AssembleArgs* aa) {
  return check_launch(launch_assemble(h->prob.kind, h->L.q, aa, h->L.naxes, make_prep(h, 0), h->s), "assemble");
}

int gpk_time_spd_inverse(gpk_handle* h, int32_t iters, double* avg_us) {
  if (!h || !avg_us || iters <= 0) return fail(GPK_EINVAL, "bad argument");
  DevSwitch ds(h->dev);
  AssembleArgs aa[2] = {};
  SpdArgs sa[2];
  fill_assemble(h, aa);
  fill_spd(h, sa);
  double total = 0.0;
  // re-assemble K (the inverse consumes it), time only the inverse
  TRY(time_each(h->s, iters, 0, [&] { return assemble_plain(h, aa); },
                [&] {
                  double* fin[2];
                  return check_launch(launch_inverse(h, sa, fin, false), "spd_inverse");
                },
                &total));
  *avg_us = total / iters;
  return read_status(h);
}

int gpk_forward_field(gpk_handle* h, int32_t what, double* out, int64_t n) {
  if (!h || !out) return fail(GPK_EINVAL, "NULL argument");
  const Layout& L = h->L;
  const int64_t n1 = L.n1, n2 = L.n2;
  int64_t want;
  if (L.dim == 2) {
    const int64_t sizes[26] = {n1 * n1, n2 * n2, n1 * n2, n2 * n1, n1 * n2, n1 * n2,
                               n1 * n1, n1 * n1, n2 * n2, n2 * n2, n1 * n1, n2 * n2,
                               n1 * n1, n2 * n2, n1 * n2, n1 * n2, n1 * n2, n1 * n2,
                               n1 * n1, n2 * n2, n1 * n1, n2 * n2, n1 * n1, n2 * n2, n1 * n1, n2 * n2};
    if (what < 0 || what > 25) return fail(GPK_EINVAL, "what must be 0..25 (2D)");
    if (what >= 22 && h->cls[0].ncls <= 0) return fail(GPK_EINVAL, "this handle does not use distance classes");
    if ((what == 18 || what == 19) && !h->Kc[what - 18])
      return fail(GPK_EINVAL, "this handle keeps no copy of K");
    if ((what == 12 || what == 13) && !h->PD[what - 12])
      return fail(GPK_EINVAL, "K^{-1} D^T is formed on the augmented chain path only");
    want = sizes[what];
  } else {
    if (what != 0 && what != 2 && what != 4 && what != 6 && what != 7)
      return fail(GPK_EINVAL, "what must be 0, 2, 4, 6 or 7 (1D)");
    want = (what == 0 || what >= 6) ? n1 * n1 : n1;
  }
  if (n != want) return fail(GPK_EINVAL, "output size mismatch");
  DevSwitch ds(h->dev);
  std::vector<double> host;
  CallScratch scratch("gpk_forward_field", h->s);
  double* tmp = nullptr;
  if (what <= 1) {  // K factor: assemble at the current params (kappa + jitter I)
    const int a = what;
    const int na = axis_n(L, a);
    TRY(check_launch(launch_prep2(h->params, L, h->kc, h->sc, h->count, 0, h->hyper.b1, h->hyper.b2, h->s), "prep"));
    TRY(scratch.alloc(&tmp, (size_t)na * na));
    const double* xa = axis_x(h, a);
    TRY(check_launch(launch_cross(h->prob.kind, L.q, xa, na, xa, na, na, h->kc + a, h->prob.jitter,
                                  0, tmp, nullptr, h->s), "cross"));
    if (hipMemcpyAsync(out, tmp, n * sizeof(double), hipMemcpyDeviceToHost, h->s) != hipSuccess)
      return fail(GPK_EHIP, "copy");
    if (hipStreamSynchronize(h->s) != hipSuccess) return fail(GPK_EHIP, "sync");
    return GPK_OK;
  }
  double loss = 0.0;
  TRY(gpk_loss_grad(h, &loss, nullptr));  // device buffers now hold the forward quantities
  if (L.dim == 1 && what >= 6) {  // the step's K (6) and D (7), as its last step assembled them
    const int P = L.p1, na = L.n1;
    const ClassArgs& C = h->cls[0];
    if (C.ncls > 0) {  // class ids + class values (K and D are never materialised on this path)
      std::vector<int> cid((size_t)P * P);
      std::vector<double> cv(C.ncls);
      HIPCHK(hipMemcpy(cid.data(), C.cid, cid.size() * sizeof(int), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(cv.data(), what == 6 ? C.kval : C.dval, cv.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (int i = 0; i < na; ++i)
        for (int j = 0; j < na; ++j) {
          double v = cv[cid[(size_t)i * P + j]];
          if (what == 6 && i == j) v += h->prob.jitter;  // (the gather adds it per element)
          out[(size_t)i * na + j] = v;
        }
      return GPK_OK;
    }
    const double* m = what == 6 ? h->Kc[0] : h->D[0];
    if (!m) return fail(GPK_EINVAL, "this handle keeps no copy of K / D");
    host.resize((size_t)P * P);
    HIPCHK(hipMemcpy(host.data(), m, host.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < na; ++i)
      for (int j = 0; j < na; ++j) out[(size_t)i * na + j] = host[(size_t)i * P + j];
    return GPK_OK;
  }
  if (L.dim == 1) {
    const int P = L.p1;
    const double* src = h->alpha;
    if (what == 4) {  // u_xx = D alpha
      TRY(scratch.alloc(&tmp, P));
      GemvDesc g{};
      g.A = h->D[0]; g.lda = P; g.x = h->alpha; g.y = tmp; g.p = P; g.rows = P; g.alpha = 1.0;
      g.epi = EPI_STORE;
      gemv_operand(h, g);
      TRY(check_launch(launch_gemv(g, h->s), "gemv"));
      src = tmp;
    }
    hipError_t e = hipMemcpyAsync(out, src, n * sizeof(double), hipMemcpyDeviceToHost, h->s);
    if (e == hipSuccess) e = hipStreamSynchronize(h->s);
    if (e != hipSuccess) return fail(GPK_EHIP, hipGetErrorString(e));
    return GPK_OK;
  }
  const int P1 = L.p1, P2 = L.p2;
  if (what >= 22) {  // K (22, 23) / D (24, 25) expanded on the host from the class table (cid + values)
    const int a = (what == 22 || what == 24) ? 0 : 1;
    const ClassArgs& C = h->cls[a];
    const int P = axis_p(L, a), na = axis_n(L, a);
    std::vector<int> cid((size_t)P * P);
    std::vector<double> cv(C.ncls), x(na);
    HIPCHK(hipMemcpy(cid.data(), C.cid, cid.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cv.data(), what <= 23 ? C.kval : C.dval, cv.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(x.data(), axis_x(h, a), na * sizeof(double), hipMemcpyDeviceToHost));
    const bool sgn = what >= 24 && h->prob.eq == GPK_ADVECTION;  // D_x1: s_ij (JAX abs'(0) = +1)
    for (int i = 0; i < na; ++i)
      for (int j = 0; j < na; ++j) {
        double v = cv[cid[(size_t)i * P + j]];
        if (what <= 23 && i == j) v += h->prob.jitter;
        if (sgn && !(x[i] - x[j] >= 0.0)) v = -v;
        out[(size_t)i * na + j] = v;
      }
    return GPK_OK;
  }
  if ((what >= 6 && what <= 13) || what >= 18) {  // work matrices, K^{-1}, K^{-1} D^T, Kc, D (P x P)
    const int a = (what == 6 || what == 7 || what == 10 || what == 12 || what == 18 || what == 20) ? 0 : 1;
    const int P = axis_p(L, a), na = axis_n(L, a);
    const double* m = what >= 20 ? h->D[a] : what >= 18 ? h->Kc[a] : what >= 12 ? h->PD[a]
                    : what >= 10 ? h->Kinv[a] : (what == 6 || what == 8) ? h->GK[a] : h->GD[a];
    host.resize((size_t)P * P);
    hipError_t e = hipMemcpyAsync(host.data(), m, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->s);
    if (e == hipSuccess) e = hipStreamSynchronize(h->s);
    if (e != hipSuccess) return fail(GPK_EHIP, hipGetErrorString(e));
    for (int i = 0; i < na; ++i)
      for (int j = 0; j < na; ++j) out[(size_t)i * na + j] = host[(size_t)i * P + j];
    return GPK_OK;
  }
  if (what >= 14) {  // grid work matrices R, X1, X2, S (P1 x P2)
    const double* m = what == 14 ? h->R : what == 15 ? h->X1 : what == 16 ? h->X2 : h->S;
    host.resize((size_t)P1 * P2);
    hipError_t e = hipMemcpyAsync(host.data(), m, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->s);
    if (e == hipSuccess) e = hipStreamSynchronize(h->s);
    if (e != hipSuccess) return fail(GPK_EHIP, hipGetErrorString(e));
    for (int64_t i = 0; i < n1; ++i)
      for (int64_t j = 0; j < n2; ++j) out[i * n2 + j] = host[(size_t)i * P2 + j];
    return GPK_OK;
  }
  const double* src = (what == 3) ? h->Bt : h->A;
  if (what >= 4) {  // U_xx = D1 A  /  U_yy = Bt D2^T
    TRY(scratch.alloc(&tmp, (size_t)P1 * P2));
    GemmDesc g{};
    if (what == 4) {
      g.A = h->D[0]; g.lda = P1; g.B = h->A; g.ldb = P2; g.K = P1;
    } else {
      g.A = h->Bt; g.lda = P2; g.B = h->D[1]; g.ldb = P2; g.tb = 1; g.K = P2;
    }
    g.C = tmp; g.ldc = P2; g.M = P1; g.N = P2; g.alpha = 1.0; g.epi = EPI_STORE;
    hipError_t e = launch_gemm_sized(&g, 1, h->sc, h->s, gemm_force(h->prob.flags));
    if (e != hipSuccess) return fail(GPK_EHIP, hipGetErrorString(e));
    src = tmp;
  }
  host.resize((size_t)P1 * P2);
  hipError_t e = hipMemcpyAsync(host.data(), src, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->s);
  if (e == hipSuccess) e = hipStreamSynchronize(h->s);
  if (e != hipSuccess) return fail(GPK_EHIP, hipGetErrorString(e));
  for (int64_t i = 0; i < n1; ++i)
    for (int64_t j = 0; j < n2; ++j) {
      const double v = host[(size_t)i * P2 + j];
      if (what == 3)
        out[j * n1 + i] = v;  // K2inv_Ut = (U K2^{-1})^T
      else
        out[i * n2 + j] = v;
    }
  return GPK_OK;
}

int gpk_fields_dd(int32_t kind, int32_t deriv, const double* d, int32_t n, double a, double freq,
                  double* hi, double* lo) {
  if (kind < 0 || kind > 3) return fail(GPK_EINVAL, "Invalid Kernel");
  if (deriv != 1 && deriv != 2) return fail(GPK_EINVAL, "deriv must be 1 or 2");
  if (n <= 0 || !d || !hi || !lo) return fail(GPK_EINVAL, "bad argument");
  for (int e = 0; e < n; ++e)
    if (!(d[e] >= 0.0)) return fail(GPK_EINVAL, "distances must be >= 0");
  int dev = 0;
  (void)hipGetDevice(&dev);
  TRY(check_device(dev));
  const double om = TWO_PI * freq, oml = om_low(freq, om);  // (gpk_api.cpp host_axis_const)
  const size_t nb = (size_t)n * sizeof(double);
  CallScratch tmp("fields_dd");
  double *dd_, *dh, *dl;
  TRY(tmp.upload(&dd_, d, (size_t)n));
  TRY(tmp.alloc(&dh, (size_t)6 * n));
  TRY(tmp.alloc(&dl, (size_t)6 * n));
  hipError_t e =
      kind == SE_COS           ? launch_fields_dd<false, true>(deriv, dd_, n, a, om, oml, dh, dl)
        : kind == MATERN52_COS ? launch_fields_dd<true, true>(deriv, dd_, n, a, om, oml, dh, dl)
        : kind == SE           ? launch_fields_dd<false, false>(deriv, dd_, n, a, om, oml, dh, dl)
                               : launch_fields_dd<true, false>(deriv, dd_, n, a, om, oml, dh, dl);
  if (e == hipSuccess) e = hipMemcpy(hi, dh, 6 * nb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(lo, dl, 6 * nb, hipMemcpyDeviceToHost);
  return check_launch(e, "fields_dd");
}

// large path: a freshly assembled K with pivot block 0 factored and (panel) sweep 0's panel formed
static int prime_big_inverse(gpk_handle* h, const AssembleArgs* aa, SpdArgs* sa, bool panel = true) {
  TRY(assemble_plain(h, aa));
  TRY(check_launch(launch_spd_big_stage(sa, h->L.naxes, -1, h->s), "pivot_init"));
  if (panel) TRY(check_launch(launch_spd_big_stage(sa, h->L.naxes, 0, h->s), "panel"));
  return GPK_OK;
}

// class path: the gather's arguments (classes, the kept copy Kc) and freshly evaluated class values
static int prime_gather(gpk_handle* h, AssembleArgs* aa) {
  const Layout& L = h->L;
  if (h->cls[0].ncls <= 0) return fail(GPK_EINVAL, "gather: this handle does not use distance classes");
  for (int a = 0; a < L.naxes; ++a) {
    aa[a].cls = h->cls[a];
    aa[a].Kc = h->Kc[a];
  }
  return check_launch(launch_assemble(h->prob.kind, L.q, aa, L.naxes, make_prep(h, 0), h->s, true), "class_eval");
}

// The K-assembly launch of the class path (the large-factor step's, gpk_step.cpp
// enqueue_assemble_inverse): K (+ jitter), its kept copy Kc (when the handle keeps one) and D
// written, the class id of every element read (its variant byte ClassArgs::vidx where the
// handle built them, p >= 1024; else the int32 id) -- the bytes it really moves; the class
// values and cbase entries are L2-resident gathers and not counted
static double gather_bytes(const gpk_handle* h) {
  double bytes = 0.0;
  for (int a = 0; a < h->L.naxes; ++a) {
    const double P = axis_p(h->L, a);
    bytes += P * P * ((h->cls[a].vidx ? 1.0 : 4.0) + 8.0 + (h->Kc[a] ? 8.0 : 0.0) + (step_deriv(h) ? 8.0 : 0.0));
  }
  return bytes;
}

int gpk_bench_kernel(gpk_handle* h, const char* name, int32_t iters, double* avg_us,
                     double* alg_flops, double* alg_bytes) {
  if (!h || !name || !avg_us || !alg_flops || !alg_bytes || iters <= 0)
    return fail(GPK_EINVAL, "bad argument");
  const std::string nm(name);
  const Layout& L = h->L;
  // one full step (no update) so every kernel's inputs are valid
  double loss = 0.0;
  TRY(gpk_loss_grad(h, &loss, nullptr));
  DevSwitch ds(h->dev);
  AssembleArgs aa[2] = {};
  SpdArgs sa[2];
  fill_assemble(h, aa);
  fill_spd(h, sa);
  // a case either sets `launch` (warmed once, then timed `iters` times back to back) or times
  // each iteration itself into `total`, `per` launches per timed region
  std::function<hipError_t()> launch;
  double flops = 0.0, bytes = 0.0, total = 0.0;
  int per = 1;
  const double n1 = L.n1, n2 = L.dim == 2 ? L.n2 : 0.0, nn[2] = {n1, n2};
  const size_t grid_bytes = (size_t)L.p1 * L.p2 * sizeof(double);
  auto copy_twice = [&]() -> int {  // an HBM-bound copy of other buffers
    for (int c = 0; c < 2; ++c) HIPCHK(hipMemcpyAsync(h->S, h->R, grid_bytes, hipMemcpyDeviceToDevice, h->s));
    return GPK_OK;
  };
  if (nm == "spd_chain") {
    // the step's persistent inverse launch as the step runs it (gather mode after the class
    // values; idempotent: it rebuilds K from the classes each time)
    if (!h->chain) return fail(GPK_EINVAL, "spd_chain: this handle does not use the chain inverse");
    const bool gather = h->cls[0].ncls > 0;
    for (int a = 0; a < L.naxes; ++a) aa[a].cls = h->cls[a];
    TRY(check_launch(launch_assemble(h->prob.kind, L.q, aa, L.naxes, make_prep(h, 0), h->s, gather),
                     "assemble"));
    launch = [&, gather]() {
      double* fin[2];
      return launch_chain(h, gather, fin);
    };
    // potrf + potri = n^3 per factor; each augmented column a triangular solve pair, 2 n^2
    // bytes: K^{-1}, Kc, D written (24 n^2), augmented outputs written (8 n m), U read
    for (int a = 0; a < L.naxes; ++a) {
      const double n = nn[a], m = h->chain_aug ? n1 + n2 : 0.0;
      flops += n * n * n + 2.0 * n * n * m;
      bytes += 24.0 * n * n + 8.0 * n * m + (h->chain_aug ? 8.0 * n1 * n2 : 0.0);
    }
  } else if (nm == "sweep" && h->bigspd) {
    // large path: time the update launch of sweep 0 (in place, so every timed launch gets a
    // freshly assembled K, pivot 0 and panel 0 first; only the update is between the events)
    TRY(time_each(h->s, iters, 0, [&] { return prime_big_inverse(h, aa, sa); },
                  [&] { return check_launch(launch_spd_big_stage(sa, L.naxes, 1, h->s), "update"); }, &total));
    // the MFMA work launch 0 schedules (its tile lists: under the two-sweep schedule launch 0
    // updates only its own parity class + the eager row / column, all at K = 128), + the next
    // pivot and panel; HBM: read + write the lower triangle
    flops = spd_big_update_flops(sa, L.naxes, 0, true);
    for (int a = 0; a < L.naxes; ++a) bytes += 8.0 * nn[a] * nn[a];
  } else if (nm == "spd_tiles" && h->bigspd) {
    // the update launch's tile work alone (no pivot workgroup), sweep 0; idempotent enough for
    // timing (each launch re-reads X and Z; values drift but stay finite over a few launches)
    TRY(prime_big_inverse(h, aa, sa));
    launch = [&]() { return launch_spd_big_tiles(sa, L.naxes, 0, h->s); };
    // the tile products launch 0's lists schedule (no pivot workgroup) -- the work actually done
    flops = spd_big_update_flops(sa, L.naxes, 0, false);
    for (int a = 0; a < L.naxes; ++a) bytes += 8.0 * nn[a] * nn[a];
  } else if (nm == "spd_updates" && h->bigspd) {
    // every update launch of one inverse (sweeps 0 .. last, each with its fused next pivot and
    // panel; the final mirror left out), between two events after pivot 0 and panel 0: the
    // average update launch as the step runs it, even and odd launches of the two-sweep schedule
    // alike, credited with the work their tile lists schedule (spd_big_update_flops)
    int nsw = 0;
    for (int a = 0; a < L.naxes; ++a) nsw = std::max(nsw, spd_big_sweeps(axis_p(L, a), h->bigwide));
    for (int k = 0; k < nsw; ++k) flops += spd_big_update_flops(sa, L.naxes, k, true);
    TRY(time_each(h->s, iters, 0, [&] { return prime_big_inverse(h, aa, sa); },
                  [&]() -> int {
                    for (int k = 0; k < nsw; ++k)
                      TRY(check_launch(launch_spd_big_stage(sa, L.naxes, 2 * k + 1, h->s, false), "update"));
                    return GPK_OK;
                  },
                  &total));
    for (int a = 0; a < L.naxes; ++a)  // read + write the lower triangle per sweep
      bytes += 8.0 * nn[a] * nn[a] * spd_big_sweeps(axis_p(L, a), h->bigwide);
    per = nsw;  // time, flops and bytes per update launch
  } else if ((nm == "spd_pivot" || nm == "spd_panel") && h->bigspd) {
    // large path pieces (idempotent): the 64-pivot factorisation of block 0, the panel of sweep 0
    TRY(prime_big_inverse(h, aa, sa, false));
    const int stage = nm == "spd_pivot" ? -1 : 0;
    launch = [&, stage]() { return launch_spd_big_stage(sa, L.naxes, stage, h->s); };
  } else if (nm == "sweep") {
    // re-assemble K and factor pivot 0, then time sweep 0 (idempotent: X -> Y, piv[1]).
    TRY(assemble_plain(h, aa));
    TRY(check_launch(launch_spd_stage(sa, L.naxes, -1, h->s), "pivot_init"));
    launch = [&]() { return launch_spd_stage(sa, L.naxes, 0, h->s); };
    // potrf+potri-equivalent flops (n^3 per factor) spread over the T = p/32 sweeps;
    // HBM bytes: read X + write Y per factor
    for (int a = 0; a < L.naxes; ++a) {
      flops += nn[a] * nn[a] * nn[a] / (axis_p(L, a) / 32);
      bytes += 16.0 * nn[a] * nn[a];
    }
  } else if (nm == "gather") {
    TRY(prime_gather(h, aa));
    launch = [&]() { return launch_gather_only(aa, L.naxes, h->s); };
    bytes = gather_bytes(h);
  } else if ((nm == "write_stream" || nm == "write_stream_after_copy") && L.dim == 2) {
    // a pure write stream of the gather's bytes (hipMemsetD32 of K, Kc, D of both factors),
    // back to back or right after an HBM-bound copy of other buffers: whether the gather's
    // in-step rate is the write-heavy HBM rate once the memory-side cache holds other lines
    const bool after = nm == "write_stream_after_copy";
    TRY(time_each(h->s, iters, 1, [&]() -> int { return after ? copy_twice() : GPK_OK; },
                  [&]() -> int {
                    for (int a = 0; a < L.naxes; ++a) {
                      const size_t P = axis_p(L, a);
                      for (double* q : {h->K[a], h->Kc[a], h->D[a]}) HIPCHK(hipMemsetD32Async(q, 0, 2 * P * P, h->s));
                    }
                    return GPK_OK;
                  },
                  &total));
    for (int a = 0; a < L.naxes; ++a) bytes += 24.0 * axis_p(L, a) * (double)axis_p(L, a);
  } else if ((nm == "gather_after_gemm" || nm == "gather_after_copy") && L.dim == 2) {
    // the gather timed alone (events around it) right after a C5-size GEMM stage (gemm_B: an
    // MFMA-bound launch writing 2 x 134 MB) or after an HBM-bound copy of the same bytes: which
    // state makes the in-step gather run at half its back-to-back rate
    TRY(prime_gather(h, aa));
    const bool gemm = nm == "gather_after_gemm";
    TRY(time_each(h->s, iters, 1,  // (the first round is a warm-up)
                  [&]() -> int {
                    if (!gemm) return copy_twice();
                    HIPCHK(launch_gemm_stage(h, 3));
                    return GPK_OK;
                  },
                  [&]() -> int {
                    HIPCHK(launch_gather_only(aa, L.naxes, h->s));
                    return GPK_OK;
                  },
                  &total));
    bytes = gather_bytes(h);
  } else if (nm == "class_eval") {
    // the class-value launch (every field at every class distance + the step constants): it
    // reads the U class distances and writes K and D values per class (24 B per class and axis)
    if (h->cls[0].ncls <= 0) return fail(GPK_EINVAL, "class_eval: this handle does not use distance classes");
    for (int a = 0; a < L.naxes; ++a) aa[a].cls = h->cls[a];
    launch = [&]() {
      return launch_assemble(h->prob.kind, L.q, aa, L.naxes, make_prep(h, 0), h->s, true);
    };
    for (int a = 0; a < L.naxes; ++a) bytes += 24.0 * h->cls[a].ncls;
  } else if (nm == "assemble") {
    // the step's assembly launch(es): class values only when the chain gathers K itself
    const bool eval_only = h->chain && h->cls[0].ncls > 0;
    for (int a = 0; a < L.naxes; ++a) aa[a].cls = h->cls[a];
    launch = [&, eval_only]() {
      return launch_assemble(h->prob.kind, L.q, aa, L.naxes, make_prep(h, 0), h->s, eval_only);
    };
    // the bytes the launch really moves: with classes and the chain, the class values (24 B per
    // class: distance read, K and D value written); otherwise K and D written per element (P^2
    // per axis, 8 B each); flops not counted (transcendental-bound)
    for (int a = 0; a < L.naxes; ++a) {
      const double P = axis_p(L, a);
      bytes += eval_only ? 24.0 * h->cls[a].ncls : 16.0 * P * P;
    }
  } else if (nm == "gemm_B" && L.dim == 2) {
    launch = [&]() { return launch_gemm_stage(h, 3); };
    // S = A K2^{-1} (2 n1 n2^2); R = D1 A + Bt D2^T (2 n1^2 n2 + 2 n1 n2^2)
    flops = 2 * n1 * n2 * n2 + 2 * n1 * n1 * n2 + 2 * n1 * n2 * n2;
    // reads A, K2^{-1}, D1, Bt, D2, F, U; writes S, R
    bytes = 8.0 * (n1 * n2 + n2 * n2 + n1 * n1 + n1 * n2 + n2 * n2 + 2 * n1 * n2 + 2 * n1 * n2);
  } else if (nm == "pgrad" && L.dim == 2) {
    // the base arguments only, without the step tail: partials as the per-pair / class path
    // forms them (no low parts, no class partials from the GEMM epilogues)
    PGradArgs pa[2];
    fill_pgrad2d(h, pa);
    launch = [&, pa]() mutable { return launch_pgrad(h->prob.kind, L.q, 0, pa, 2, h->bpa, h->sc, h->s); };
    bytes = 16.0 * (n1 * n1 + n2 * n2);  // G_K, G_D read
  } else {
    return fail(GPK_EINVAL, "unknown kernel name (spd_chain | sweep | assemble | gemm_B | pgrad[2D])");
  }
  if (launch) {
    HIPCHK(time_launches(h->s, iters, 1, launch, avg_us));
  } else {
    *avg_us = total / iters / per;
  }
  *alg_flops = flops / per;
  *alg_bytes = bytes / per;
  return read_status(h);
}

int gpk_dgemm(int32_t variant, int32_t M, int32_t N, int32_t K, double alpha, const double* A,
              int32_t lda, int32_t ta, const double* B, int32_t ldb, int32_t tb, int32_t K2,
              double alpha2, const double* A2, int32_t lda2, int32_t ta2, const double* B2,
              int32_t ldb2, int32_t tb2, double beta, const double* C0, double* C, int32_t ldc,
              int32_t iters, double* avg_us) {
  if (variant < 0 || variant > 3 || M <= 0 || N <= 0 || K <= 0 || K2 < 0 || (M | N | K | K2) & 31 ||
      !A || !B || !C || (K2 && (!A2 || !B2)) || iters < 0 || (iters && !avg_us))
    return fail(GPK_EINVAL, "gpk_dgemm: bad argument (M, N, K, K2 multiples of 32)");
  // stored extents of op(A) = M x K etc.: rows x row length, each row length <= its ld
  auto ext = [](int rows, int cols, int t, int ld, size_t* n) {
    const int r = t ? cols : rows, c = t ? rows : cols;
    *n = (size_t)(r - 1) * ld + c;
    return ld >= c;
  };
  size_t na = 0, nb = 0, na2 = 0, nb2 = 0, nc = 0;
  if (!ext(M, K, ta, lda, &na) || !ext(K, N, tb, ldb, &nb) || !ext(M, N, 0, ldc, &nc) ||
      (K2 && (!ext(M, K2, ta2, lda2, &na2) || !ext(K2, N, tb2, ldb2, &nb2))))
    return fail(GPK_EINVAL, "gpk_dgemm: leading dimension shorter than a row");
  TRY(check_device(0));
  DevSwitch dsw(0);
  CallScratch tmp("gpk_dgemm");
  GemmDesc d{};
  double *dA = nullptr, *dB = nullptr, *dA2 = nullptr, *dB2 = nullptr, *dC = nullptr, *dC0 = nullptr;
  TRY(tmp.upload(&dA, A, na));
  TRY(tmp.upload(&dB, B, nb));
  if (K2) TRY(tmp.upload(&dA2, A2, na2));
  if (K2) TRY(tmp.upload(&dB2, B2, nb2));
  TRY(C0 == C ? tmp.upload(&dC, C, nc) : tmp.alloc(&dC, nc));
  if (C0 && C0 != C) TRY(tmp.upload(&dC0, C0, nc));
  d.A = dA; d.lda = lda; d.ta = ta ? 1 : 0; d.B = dB; d.ldb = ldb; d.tb = tb ? 1 : 0;
  d.A2 = dA2; d.lda2 = lda2; d.ta2 = ta2 ? 1 : 0; d.B2 = dB2; d.ldb2 = ldb2; d.tb2 = tb2 ? 1 : 0;
  d.alpha = alpha; d.alpha2 = alpha2; d.K2 = K2;
  d.beta = C0 ? beta : 0.0; d.C0 = C0 ? (C0 == C ? dC : dC0) : nullptr; d.ldc0 = ldc;
  d.C = dC; d.ldc = ldc; d.M = M; d.N = N; d.K = K; d.epi = EPI_STORE;
  const int v = variant ? variant : gemm_variant(&d, 1, 0);
  auto launch = [&]() { return launch_gemm_auto(&d, 1, nullptr, 0, v); };
  // (an in-place C0 == C update is checked once; timed launches then repeat it on their own output)
  hipError_t e = launch();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(C, dC, nc * 8, hipMemcpyDeviceToHost);
  // (timing only: with C0 == C every timed launch updates dC in place, so each one reads the
  // previous launch's output as its C0 -- same shapes and work, different values; the result
  // copied back above is the first launch's)
  if (e == hipSuccess && iters) e = time_launches(0, iters, 1, launch, avg_us);
  return check_launch(e, "gpk_dgemm");
}

namespace {

// elements a row-major rows x cols block with leading dimension ld spans; 0 when ld is shorter
// than a row or odd (the kernels' 16-byte operand loads)
size_t block_extent(int rows, int cols, int ld) {
  return (ld >= cols && !(ld & 1)) ? (size_t)(rows - 1) * ld + cols : 0;
}

// the two gate words (gate_open: open when gate[0] * gate[1] > REFINE_COND_LB; a product equal to
// the bound is closed) of a gate selector, uploaded; GPK_GATE_NONE leaves *gate null
int upload_gate(CallScratch& tmp, int sel, const double** gate) {
  *gate = nullptr;
  if (sel == GPK_GATE_NONE) return GPK_OK;
  const double w[2] = {1.0, sel == GPK_GATE_OPEN ? 2.0 * REFINE_COND_LB : REFINE_COND_LB};
  double* d = nullptr;
  TRY(tmp.upload(&d, w, 2));
  *gate = d;
  return GPK_OK;
}

// a host array (nullable) uploaded for a descriptor's const operand
int upload_opt(CallScratch& tmp, const double* src, size_t n, const double** dst) {
  *dst = nullptr;
  if (!src) return GPK_OK;
  double* d = nullptr;
  TRY(tmp.upload(&d, src, n));
  *dst = d;
  return GPK_OK;
}

// no output of a call may be one of its inputs or another output; `inplace` lists the outputs
// that one input each may equal (C0 == C)
bool outputs_alias(const std::vector<const void*>& in, const std::vector<const void*>& out,
                   const std::vector<const void*>& inplace) {
  for (size_t o = 0; o < out.size(); ++o) {
    for (size_t q = o + 1; q < out.size(); ++q)
      if (out[o] == out[q]) return true;
    size_t same = 0, allowed = 0;
    for (const void* p : in) same += p == out[o];
    for (const void* p : inplace) allowed += p == out[o];
    if (same > allowed) return true;
  }
  return false;
}

}  // namespace

int gpk_dgemm_epi(int32_t variant, int32_t ndesc, gpk_gemm_case* cases, double v) {
  if (variant < GEMM_SMALL || variant > GEMM_HUGE || ndesc < 1 || ndesc > GEMM_MAX_BATCH || !cases ||
      !std::isfinite(v))
    return fail(GPK_EINVAL, "gpk_dgemm_epi: variant 1..3, 1..4 descriptors, finite v");
  struct Ext { size_t a, b, a2, b2, c, c0, f, y; };
  Ext ex[GEMM_MAX_BATCH] = {};
  std::vector<const void*> in, out, inplace;
  for (int i = 0; i < ndesc; ++i) {
    gpk_gemm_case& g = cases[i];
    Ext& e = ex[i];
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || g.K2 < 0 || ((g.M | g.N | g.K | g.K2) & 31))
      return fail(GPK_EINVAL, "gpk_dgemm_epi: M, N, K, K2 must be multiples of 32");
    GemmDesc shape{};
    shape.M = g.M; shape.N = g.N;
    g.tiles = gemm_tiles(shape, variant);
    if (!g.A || !g.B || !g.C || (g.K2 && (!g.A2 || !g.B2)))
      return fail(GPK_EINVAL, "gpk_dgemm_epi: NULL operand");
    if (g.epi < GPK_EPI_STORE || g.epi > GPK_EPI_QUAD || g.gate < GPK_GATE_NONE || g.gate > GPK_GATE_CLOSED)
      return fail(GPK_EINVAL, "gpk_dgemm_epi: epi must be 0..2 and gate 0..2");
    if (!std::isfinite(g.alpha) || !std::isfinite(g.alpha2) || !std::isfinite(g.beta))
      return fail(GPK_EINVAL, "gpk_dgemm_epi: alpha, alpha2 and beta must be finite");
    e.a = g.ta ? block_extent(g.K, g.M, g.lda) : block_extent(g.M, g.K, g.lda);
    e.b = g.tb ? block_extent(g.N, g.K, g.ldb) : block_extent(g.K, g.N, g.ldb);
    e.c = block_extent(g.M, g.N, g.ldc);
    bool ok = e.a && e.b && e.c;
    if (g.K2) {
      e.a2 = g.ta2 ? block_extent(g.K2, g.M, g.lda2) : block_extent(g.M, g.K2, g.lda2);
      e.b2 = g.tb2 ? block_extent(g.N, g.K2, g.ldb2) : block_extent(g.K2, g.N, g.ldb2);
      ok = ok && e.a2 && e.b2;
    }
    if (g.C0) {
      e.c0 = block_extent(g.M, g.N, g.ldc0);
      ok = ok && e.c0 && (g.C0 != g.C || g.ldc0 == g.ldc);
    }
    const bool side = g.Y != nullptr, epi_ops = g.F || g.U || g.Q1 || g.Q2;
    if (epi_ops) {
      e.f = block_extent(g.M, g.N, g.ldf);
      ok = ok && e.f;
    }
    if (side || g.Ys) {
      e.y = block_extent(g.M, g.N, g.ldy);
      ok = ok && e.y;
    }
    if (!ok) return fail(GPK_EINVAL, "gpk_dgemm_epi: a leading dimension is odd or shorter than a row");
    if (g.beta != 0.0 && !g.C0) return fail(GPK_EINVAL, "gpk_dgemm_epi: beta != 0 needs C0");
    if (side && (g.epi != GPK_EPI_STORE || !g.Ys))
      return fail(GPK_EINVAL, "gpk_dgemm_epi: Y is the STORE epilogue's side output and needs Ys");
    if ((g.epi == GPK_EPI_RESID && (!g.F || (g.ac && !g.U))) || (g.epi == GPK_EPI_QUAD && !g.U))
      return fail(GPK_EINVAL, "gpk_dgemm_epi: RESID needs F (and U with ac), QUAD needs U");
    if ((g.red && g.epi == GPK_EPI_STORE) || (g.red2 && (g.epi != GPK_EPI_RESID || !g.Q1 || !g.Q2)))
      return fail(GPK_EINVAL, "gpk_dgemm_epi: red is formed by RESID and QUAD, red2 by RESID from Q1 and Q2");
    if ((g.red || g.red2) && g.red_cap < g.tiles)
      return fail(GPK_EINVAL, "gpk_dgemm_epi: red_cap is below the variant's tile count");
    for (const void* p : {(const void*)g.A, (const void*)g.B, (const void*)g.A2, (const void*)g.B2,
                          (const void*)g.C0, (const void*)g.F, (const void*)g.U, (const void*)g.Q1,
                          (const void*)g.Q2, (const void*)g.Ys})
      if (p) in.push_back(p);
    for (const void* p : {(const void*)g.C, (const void*)g.Y, (const void*)g.red, (const void*)g.red2})
      if (p) out.push_back(p);
    if (g.C0 == g.C) inplace.push_back(g.C);
  }
  if (outputs_alias(in, out, inplace))
    return fail(GPK_EINVAL, "gpk_dgemm_epi: an output is also an input (other than C0 == C) or another output");
  TRY(check_device(0));
  DevSwitch dsw(0);
  CallScratch tmp("gpk_dgemm_epi");
  const StepScalars hsc{1.0, v, 1.0, 1.0};
  StepScalars* sc = nullptr;
  TRY(tmp.upload(&sc, &hsc, 1));
  GemmDesc d[GEMM_MAX_BATCH] = {};
  for (int i = 0; i < ndesc; ++i) {
    const gpk_gemm_case& g = cases[i];
    const Ext& e = ex[i];
    GemmDesc& x = d[i];
    TRY(upload_opt(tmp, g.A, e.a, &x.A));
    TRY(upload_opt(tmp, g.B, e.b, &x.B));
    if (g.K2) TRY(upload_opt(tmp, g.A2, e.a2, &x.A2));
    if (g.K2) TRY(upload_opt(tmp, g.B2, e.b2, &x.B2));
    TRY(tmp.upload(&x.C, g.C, e.c));
    if (g.C0 == g.C)
      x.C0 = x.C;
    else
      TRY(upload_opt(tmp, g.C0, e.c0, &x.C0));
    TRY(upload_opt(tmp, g.F, e.f, &x.F));
    TRY(upload_opt(tmp, g.U, e.f, &x.U));
    TRY(upload_opt(tmp, g.Q1, e.f, &x.Q1));
    TRY(upload_opt(tmp, g.Q2, e.f, &x.Q2));
    if (g.Y) TRY(upload_opt(tmp, g.Ys, e.y, &x.Ys));
    if (g.Y) TRY(tmp.upload(&x.Y, g.Y, e.y));
    if (g.red) TRY(tmp.upload(&x.red, g.red, (size_t)g.red_cap));
    if (g.red2) TRY(tmp.upload(&x.red2, g.red2, (size_t)g.red_cap));
    TRY(upload_gate(tmp, g.gate, &x.gate));
    x.lda = g.lda; x.ta = g.ta ? 1 : 0; x.ldb = g.ldb; x.tb = g.tb ? 1 : 0;
    x.lda2 = g.lda2; x.ta2 = g.ta2 ? 1 : 0; x.ldb2 = g.ldb2; x.tb2 = g.tb2 ? 1 : 0;
    x.alpha = g.alpha; x.alpha2 = g.alpha2; x.beta = g.beta; x.ldc0 = g.ldc0; x.ldc = g.ldc;
    x.M = g.M; x.N = g.N; x.K = g.K; x.K2 = g.K2; x.epi = g.epi; x.ac = g.ac ? 1 : 0;
    x.ldf = g.ldf; x.vscale = g.vscale ? 1 : 0; x.vscale2 = g.vscale2 ? 1 : 0; x.ldy = g.ldy;
  }
  hipError_t e = launch_gemm_auto(d, ndesc, sc, 0, variant);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  for (int i = 0; i < ndesc && e == hipSuccess; ++i) {
    const gpk_gemm_case& g = cases[i];
    e = hipMemcpy(g.C, d[i].C, ex[i].c * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && g.Y) e = hipMemcpy(g.Y, d[i].Y, ex[i].y * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && g.red) e = hipMemcpy(g.red, d[i].red, (size_t)g.red_cap * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && g.red2) e = hipMemcpy(g.red2, d[i].red2, (size_t)g.red_cap * 8, hipMemcpyDeviceToHost);
  }
  return check_launch(e, "gpk_dgemm_epi");
}

int gpk_dgemv_epi(int32_t p, int32_t rows, const double* A, const int32_t* cid, const double* cv,
                  int32_t ncls, double cdiag, int32_t ident, int32_t lda, const double* x, double alpha,
                  const double* C0, double beta, int32_t epi, int32_t ac, const double* F, const double* U,
                  const double* U0, const double* Q1, const double* Q2, double* red, double* red2,
                  int32_t gate, double* y) {
  if (p <= 0 || (p & 31) || lda < p || (lda & 31) || rows < 1 || rows > p)
    return fail(GPK_EINVAL, "gpk_dgemv_epi: p and lda multiples of 32, lda >= p, 1 <= rows <= p");
  if (!x || !y || (!A && (!cid || !cv || ncls < 1)) || (A && cid))
    return fail(GPK_EINVAL, "gpk_dgemv_epi: needs x, y and either A or the class form (cid, cv, ncls >= 1)");
  if (epi < GPK_EPI_STORE || epi > GPK_EPI_QUAD || gate < GPK_GATE_NONE || gate > GPK_GATE_CLOSED)
    return fail(GPK_EINVAL, "gpk_dgemv_epi: epi must be 0..2 and gate 0..2");
  if (!std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(cdiag))
    return fail(GPK_EINVAL, "gpk_dgemv_epi: alpha, beta and cdiag must be finite");
  if (beta != 0.0 && !C0) return fail(GPK_EINVAL, "gpk_dgemv_epi: beta != 0 needs C0");
  if ((epi == GPK_EPI_RESID && (!F || (ac && !U))) || (epi == GPK_EPI_QUAD && !U))
    return fail(GPK_EINVAL, "gpk_dgemv_epi: RESID needs F (and U with ac), QUAD needs U");
  if ((red && epi == GPK_EPI_STORE) || (red2 && (!Q1 || !Q2)))
    return fail(GPK_EINVAL, "gpk_dgemv_epi: red is formed by RESID and QUAD, red2 from Q1 and Q2");
  const size_t nm = (size_t)(rows - 1) * lda + p;
  if (cid)
    for (int i = 0; i < rows; ++i)
      for (int j = 0; j < p; ++j)
        if (cid[(size_t)i * lda + j] >= ncls) return fail(GPK_EINVAL, "gpk_dgemv_epi: class id >= ncls");
  std::vector<const void*> in, out, inplace;
  for (const void* q : {(const void*)A, (const void*)cv, (const void*)x, (const void*)C0, (const void*)F,
                        (const void*)U, (const void*)U0, (const void*)Q1, (const void*)Q2})
    if (q) in.push_back(q);
  for (const void* q : {(const void*)y, (const void*)red, (const void*)red2})
    if (q) out.push_back(q);
  if (C0 == y) inplace.push_back(y);
  if (outputs_alias(in, out, inplace) || (const void*)cid == (const void*)y)
    return fail(GPK_EINVAL, "gpk_dgemv_epi: an output is also an input (other than C0 == y) or another output");
  TRY(check_device(0));
  DevSwitch dsw(0);
  CallScratch tmp("gpk_dgemv_epi");
  GemvDesc d{};
  const int nblk = gemv_blocks(rows);
  TRY(upload_opt(tmp, A, nm, &d.A));
  if (cid) {
    int* dcid = nullptr;
    TRY(tmp.upload(&dcid, reinterpret_cast<const int*>(cid), nm));
    d.cid = dcid;
    TRY(upload_opt(tmp, cv, (size_t)ncls, &d.cv));
  }
  TRY(upload_opt(tmp, x, (size_t)p, &d.x));
  TRY(tmp.upload(&d.y, y, (size_t)rows));
  if (C0 == y)
    d.C0 = d.y;
  else
    TRY(upload_opt(tmp, C0, (size_t)rows, &d.C0));
  TRY(upload_opt(tmp, F, (size_t)rows, &d.F));
  TRY(upload_opt(tmp, U, (size_t)rows, &d.U));
  TRY(upload_opt(tmp, U0, (size_t)rows, &d.U0));
  TRY(upload_opt(tmp, Q1, (size_t)rows, &d.Q1));
  TRY(upload_opt(tmp, Q2, (size_t)rows, &d.Q2));
  if (red) TRY(tmp.upload(&d.red, red, (size_t)nblk));
  if (red2) TRY(tmp.upload(&d.red2, red2, (size_t)nblk));
  TRY(upload_gate(tmp, gate, &d.gate));
  d.lda = lda; d.p = p; d.rows = rows; d.alpha = alpha; d.beta = beta; d.epi = epi; d.ac = ac ? 1 : 0;
  d.cdiag = cdiag; d.ident = ident ? 1 : 0;
  hipError_t e = launch_gemv(d, 0);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(y, d.y, (size_t)rows * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && red) e = hipMemcpy(red, d.red, (size_t)nblk * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && red2) e = hipMemcpy(red2, d.red2, (size_t)nblk * 8, hipMemcpyDeviceToHost);
  return check_launch(e, "gpk_dgemv_epi");
}

int gpk_mode_gemm(int32_t variant, int32_t k, int32_t d1, int32_t d2, int32_t d3, int32_t m, double alpha,
                  const double* Mat, const double* T, double beta, const double* C0, double* C,
                  int32_t iters, double* avg_us) {
  if (variant < 0 || variant > 3 || k < 1 || k > 3 || d1 <= 0 || d2 <= 0 || d3 <= 0 || m <= 0 ||
      ((d1 | d2 | d3 | m) & 31) || !Mat || !T || !C || iters < 0 || (iters && !avg_us))
    return fail(GPK_EINVAL, "gpk_mode_gemm: bad argument (k in 1..3, sizes multiples of 32)");
  if (k == 2 && d1 > 65535) return fail(GPK_EINVAL, "gpk_mode_gemm: mode 2 takes at most 65535 slabs");
  const int dk = k == 1 ? d1 : k == 2 ? d2 : d3;
  const size_t nt = (size_t)d1 * d2 * d3, nc = nt / dk * m, nm = (size_t)m * dk;
  if (nt / dk > 0x7fffffff / 2) return fail(GPK_EINVAL, "gpk_mode_gemm: tensor too large");
  TRY(check_device(0));
  DevSwitch dsw(0);
  CallScratch tmp("gpk_mode_gemm");
  const bool permute = k == 2 && variant == 1;
  double *dM = nullptr, *dT = nullptr, *dC = nullptr, *dC0 = nullptr, *dTp = nullptr, *dCp = nullptr,
         *dC0p = nullptr;
  TRY(tmp.upload(&dM, Mat, nm));
  TRY(tmp.upload(&dT, T, nt));
  TRY(C0 == C ? tmp.upload(&dC, C, nc) : tmp.alloc(&dC, nc));
  if (C0 && C0 != C) TRY(tmp.upload(&dC0, C0, nc));
  if (permute) TRY(tmp.alloc(&dTp, nt));
  if (permute) TRY(tmp.alloc(&dCp, nc));
  if (permute && C0) TRY(tmp.alloc(&dC0p, nc));
  const double* c0 = C0 ? (C0 == C ? dC : dC0) : nullptr;
  const double be = C0 ? beta : 0.0;
  auto one = [&](GemmDesc d, const double* c0_) {
    d.alpha = alpha;
    if (c0_) { d.beta = be; d.C0 = c0_; d.ldc0 = d.ldc; }
    return launch_gemm_sized(&d, 1, nullptr, 0);
  };
  const int n23 = d2 * d3, n13 = d1 * d3, n12 = d1 * d2;
  auto launch = [&]() -> hipError_t {
    if (k == 1) return one(gemm_desc(dM, d1, 0, dT, n23, 0, dC, n23, m, n23, d1), c0);
    if (k == 3) return one(gemm_desc(dT, d3, 0, dM, d3, 1, dC, m, n12, m, d3), c0);
    if (!permute) {  // the slab kernel (variant 2 / 3: its 32 / 64 tile forced)
      SlabGemm sg{};
      sg.A = dM; sg.B = dT; sg.sB = (size_t)n23; sg.C = dC; sg.sC = (size_t)m * d3; sg.C0 = c0; sg.sC0 = sg.sC;
      sg.M = m; sg.N = d3; sg.K = d2; sg.nb = d1; sg.alpha = alpha; sg.beta = be;
      return launch_gemm_slab(sg, 0, variant == 2 ? 32 : variant == 3 ? 64 : 0);
    }
    // the step's route: permuted copy [d2][d1][d3], one GEMM on its rows, permuted back
    K3Geom gi{}, go{};
    gi.p[0] = gi.n[0] = d1; gi.p[1] = gi.n[1] = d2; gi.p[2] = gi.n[2] = d3;
    go.p[0] = go.n[0] = m; go.p[1] = go.n[1] = d1; go.p[2] = go.n[2] = d3;   // [m][d1][d3] -> [d1][m][d3]
    K3Geom gc = go;
    gc.p[0] = gc.n[0] = d1; gc.p[1] = gc.n[1] = m;                             // [d1][m][d3] -> [m][d1][d3]
    hipError_t r = k3_launch_permute(dT, dTp, gi, 0);
    if (r == hipSuccess && c0) r = k3_launch_permute(c0, dC0p, gc, 0);
    if (r == hipSuccess) r = one(gemm_desc(dM, d2, 0, dTp, n13, 0, dCp, n13, m, n13, d2), c0 ? dC0p : nullptr);
    if (r == hipSuccess) r = k3_launch_permute(dCp, dC, go, 0);
    return r;
  };
  // (as gpk_dgemm: C receives the checked launch's result; with C0 == C the timed launches keep
  // updating the device copy in place -- same work, each on the last one's output)
  hipError_t e = launch();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(C, dC, nc * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && iters) e = time_launches(0, iters, 1, launch, avg_us);
  return check_launch(e, "gpk_mode_gemm");
}

int gpk_refine_panel(int32_t route, int32_t side, int32_t P, int32_t M, const double* Kinv, const double* Kc,
                     const double* B, double* X, int32_t iters, double* avg_us) {
  if (route < 0 || route > 1 || side < 0 || side > 1 || P < 32 || (P & 31) || M < 32 || (M & 31) ||
      P > K3_MAX_N || !Kinv || !Kc || !B || !X || iters < 0 || (iters && !avg_us))
    return fail(GPK_EINVAL, "gpk_refine_panel: bad argument (route, side in 0..1, sizes multiples of 32)");
  if (route == 1 && P > REFINE_PANEL_MAX_P)
    return fail(GPK_EINVAL, "gpk_refine_panel: the fused route holds two P x 16 panels in LDS: P <= 512");
  if ((size_t)P * M > 0x7fffffff / 2) return fail(GPK_EINVAL, "gpk_refine_panel: tensor too large");
  TRY(check_device(0));
  DevSwitch dsw(0);
  const size_t nt = (size_t)P * M, nm = (size_t)P * P;
  CallScratch tmp("gpk_refine_panel");
  double *dKi = nullptr, *dKc = nullptr, *dB = nullptr, *dX = nullptr, *dW = nullptr;
  TRY(tmp.upload(&dKi, Kinv, nm));
  TRY(tmp.upload(&dKc, Kc, nm));
  TRY(tmp.upload(&dB, B, nt));
  TRY(tmp.upload(&dX, X, nt));
  TRY(tmp.alloc(&dW, nt));
  if (route == 1) TRY(check_launch(refine_panel_prepare(), "gpk_refine_panel"));
  // the step's refinement of one solve (gpk_kron3.cpp build_refine), ungated: X is P x M (side 0,
  // K on the left) or M x P (side 1)
  const int rows = side ? M : P, cols = side ? P : M;
  const RefinePanel f = refine_panel_desc(side, dKc, dKi, dB, dX, rows, cols, nullptr);
  const RefinedSolve g = refined_solve(side, dKc, dKi, dB, dX, dW, rows, cols, nullptr);
  auto launch = [&]() -> hipError_t {
    if (route == 1) return launch_refine_panel(&f, 1, nullptr, 0);
    hipError_t rc = launch_gemm_sized(&g.resid, 1, nullptr, 0);
    return rc == hipSuccess ? launch_gemm_sized(&g.fix, 1, nullptr, 0) : rc;
  };
  // (X receives the checked launch's result; the timed launches keep refining the device copy)
  hipError_t e = launch();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(X, dX, nt * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && iters) e = time_launches(0, iters, 1, launch, avg_us);
  return check_launch(e, "gpk_refine_panel");
}

int gpk_point_contract(int32_t kind, int32_t deriv, const double* t, int32_t m, const double* x, int32_t n,
                       const double* logw, const double* logls, const double* freq, int32_t q,
                       const double* T, int64_t sp, int64_t sj, int64_t sc, int32_t C,
                       double* out, int32_t iters, double* avg_us) {
  if (kind < 0 || kind > 3) return fail(GPK_EINVAL, "Invalid Kernel");
  if (deriv < 0 || deriv > 2) return fail(GPK_EINVAL, "deriv must be 0, 1 or 2");
  if (m <= 0 || n <= 0 || C <= 0 || q <= 0 || q > QMAX || iters < 0)
    return fail(GPK_EINVAL, "gpk_point_contract: bad sizes (m, n, C >= 1, 0 < q <= 64)");
  if (!t || !x || !logw || !logls || !freq || !T || !out || (iters && !avg_us))
    return fail(GPK_EINVAL, "gpk_point_contract: NULL pointer argument");
  if (C > 1 && n > POINT_MAX_N)
    return fail(GPK_EINVAL, "gpk_point_contract: C > 1 holds a point's n field values in LDS: n <= 4096");
  const size_t nT = point_contract_extent(m, n, C, sp, sj, sc);
  if (!nT) return fail(GPK_EINVAL, "gpk_point_contract: strides need sp >= 0, sj >= 1, sc >= 1");
  TRY(check_device(0));
  DevSwitch dsw(0);
  AxisConst hk;
  host_axis_const(logw, logls, freq, q, &hk);
  CallScratch tmp("gpk_point_contract");
  double *dt = nullptr, *dx = nullptr, *dT = nullptr, *dout = nullptr;
  AxisConst* dkc = nullptr;
  TRY(tmp.upload(&dt, t, (size_t)m));
  TRY(tmp.upload(&dx, x, (size_t)n));
  TRY(tmp.upload(&dT, T, nT));
  TRY(tmp.alloc(&dout, (size_t)m * C));
  TRY(tmp.upload(&dkc, &hk, 1));
  PointContract pc{};
  pc.t = dt; pc.m = m; pc.x = dx; pc.n = n; pc.kc = dkc; pc.q = q;
  pc.T = dT; pc.sp = (size_t)sp; pc.sj = (size_t)sj; pc.sc = (size_t)sc; pc.C = C; pc.out = dout;
  auto launch = [&]() { return launch_point_contract(kind, deriv, pc, 0); };
  hipError_t e = launch();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)m * C * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && iters) e = time_launches(0, iters, 1, launch, avg_us);
  return check_launch(e, "gpk_point_contract");
}

// gpk_assemble_pairs (K_out, D_out; iters = 0) and gpk_assemble_pairs_time (iters > 0, no outputs;
// split: modes 2 and 1 as two launches per iteration, each into a block of its own)
static int assemble_pairs_impl(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                               const double* freq, int32_t q, double jitter, double c2, double c1,
                               double* K_out, double* D_out, int32_t split, int32_t iters, double* avg_us) {
  if (kind < 0 || kind > 3) return fail(GPK_EINVAL, "Invalid Kernel");
  if (n < 1 || n > K3_MAX_N || q <= 0 || q > QMAX || iters < 0)
    return fail(GPK_EINVAL, "gpk_assemble_pairs: bad sizes (1 <= n <= 1024, 0 < q <= 64)");
  if (!x || !logw || !logls || !freq || (iters ? !avg_us : (!K_out || !D_out)))
    return fail(GPK_EINVAL, "gpk_assemble_pairs: NULL pointer argument");
  if (!std::isfinite(c2) || !std::isfinite(c1) || !std::isfinite(jitter))
    return fail(GPK_EINVAL, "gpk_assemble_pairs: c2, c1 and jitter must be finite");
  TRY(check_device(0));
  DevSwitch dsw(0);
  const int P = pad_up(n);
  // the kernel derives its axis constants from flat params laid out (freq, log-ls, log-w)
  std::vector<double> kp(3 * (size_t)q);
  std::copy(freq, freq + q, kp.begin());
  std::copy(logls, logls + q, kp.begin() + q);
  std::copy(logw, logw + q, kp.begin() + 2 * q);
  CallScratch tmp("gpk_assemble_pairs");
  double *dx = nullptr, *dkp = nullptr, *dK = nullptr, *dD = nullptr, *dD1 = nullptr;
  TRY(tmp.alloc(&dx, (size_t)P, true));
  TRY(check_launch(hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice), "gpk_assemble_pairs"));
  TRY(tmp.upload(&dkp, kp.data(), kp.size()));
  TRY(tmp.alloc(&dK, (size_t)P * P, true));
  TRY(tmp.alloc(&dD, (size_t)P * P, true));
  if (split) TRY(tmp.alloc(&dD1, (size_t)P * P, true));
  AssembleArgs aa{};
  aa.x = dx; aa.n = n; aa.p = P; aa.jitter = jitter; aa.K = dK; aa.D = dD;
  aa.deriv = c1 == 0.0 ? 2 : c2 == 0.0 ? 1 : DERIV_BOTH;
  aa.c2 = c2; aa.c1 = c1;
  PrepArgs prep{};
  prep.params = dkp; prep.naxes = 1; prep.skip = 1;  // (no step constants to publish)
  auto launch = [&]() {
    if (!split) return launch_assemble(kind, q, &aa, 1, prep, 0);
    AssembleArgs a2 = aa, a1 = aa;
    a2.deriv = 2;
    a1.deriv = 1; a1.D = dD1;
    const hipError_t e2 = launch_assemble(kind, q, &a2, 1, prep, 0);
    return e2 != hipSuccess ? e2 : launch_assemble(kind, q, &a1, 1, prep, 0);
  };
  hipError_t e = launch();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  const size_t row = (size_t)n * sizeof(double);
  if (e == hipSuccess && K_out) e = hipMemcpy2D(K_out, row, dK, (size_t)P * sizeof(double), row, n, hipMemcpyDeviceToHost);
  if (e == hipSuccess && D_out) e = hipMemcpy2D(D_out, row, dD, (size_t)P * sizeof(double), row, n, hipMemcpyDeviceToHost);
  if (e == hipSuccess && iters) e = time_launches(0, iters, 1, launch, avg_us);
  return check_launch(e, "gpk_assemble_pairs");
}

int gpk_assemble_pairs(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                       const double* freq, int32_t q, double jitter, double c2, double c1,
                       double* K_out, double* D_out) {
  if (!K_out || !D_out) return fail(GPK_EINVAL, "gpk_assemble_pairs: NULL pointer argument");
  return assemble_pairs_impl(kind, x, n, logw, logls, freq, q, jitter, c2, c1, K_out, D_out, 0, 0, nullptr);
}

// The two-block mode (DERIV_SPLIT, a convective axis's assembly): K, D = c2 DD + c1 D1 and D1, at
// any weights, zeros included
int gpk_assemble_pairs2(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                        const double* freq, int32_t q, double jitter, double c2, double c1,
                        double* K_out, double* D_out, double* D1_out) {
  if (kind < 0 || kind > 3) return fail(GPK_EINVAL, "Invalid Kernel");
  if (n < 1 || n > K3_MAX_N || q <= 0 || q > QMAX)
    return fail(GPK_EINVAL, "gpk_assemble_pairs2: bad sizes (1 <= n <= 1024, 0 < q <= 64)");
  if (!x || !logw || !logls || !freq || !K_out || !D_out || !D1_out)
    return fail(GPK_EINVAL, "gpk_assemble_pairs2: NULL pointer argument");
  if (!std::isfinite(c2) || !std::isfinite(c1) || !std::isfinite(jitter))
    return fail(GPK_EINVAL, "gpk_assemble_pairs2: c2, c1 and jitter must be finite");
  TRY(check_device(0));
  DevSwitch dsw(0);
  const int P = pad_up(n);
  std::vector<double> kp(3 * (size_t)q);  // flat params laid out (freq, log-ls, log-w)
  std::copy(freq, freq + q, kp.begin());
  std::copy(logls, logls + q, kp.begin() + q);
  std::copy(logw, logw + q, kp.begin() + 2 * q);
  CallScratch tmp("gpk_assemble_pairs2");
  double *dx = nullptr, *dkp = nullptr, *dK = nullptr, *dD = nullptr, *dD1 = nullptr;
  TRY(tmp.alloc(&dx, (size_t)P, true));
  TRY(check_launch(hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice), "gpk_assemble_pairs2"));
  TRY(tmp.upload(&dkp, kp.data(), kp.size()));
  TRY(tmp.alloc(&dK, (size_t)P * P, true));
  TRY(tmp.alloc(&dD, (size_t)P * P, true));
  TRY(tmp.alloc(&dD1, (size_t)P * P, true));
  AssembleArgs aa{};
  aa.x = dx; aa.n = n; aa.p = P; aa.jitter = jitter; aa.K = dK; aa.D = dD; aa.D1 = dD1;
  aa.deriv = DERIV_SPLIT; aa.c2 = c2; aa.c1 = c1;
  PrepArgs prep{};
  prep.params = dkp; prep.naxes = 1; prep.skip = 1;  // (no step constants to publish)
  hipError_t e = launch_assemble(kind, q, &aa, 1, prep, 0);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  const size_t row = (size_t)n * sizeof(double);
  for (auto [dst, src] : {std::pair<double*, double*>{K_out, dK}, {D_out, dD}, {D1_out, dD1}})
    if (e == hipSuccess) e = hipMemcpy2D(dst, row, src, (size_t)P * sizeof(double), row, n, hipMemcpyDeviceToHost);
  return check_launch(e, "gpk_assemble_pairs2");
}

// The high-order modes (DERIV_HIGH; DERIV_HIGH_SPLIT when D1_out is given): K, D = c4 D4 + c3 D3 + c2 DD
// + c1 D1 and, in the two-block mode, D1, at any weights, zeros included
int gpk_assemble_pairs4(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                        const double* freq, int32_t q, double jitter, double c4, double c3, double c2,
                        double c1, double* K_out, double* D_out, double* D1_out) {
  if (kind < 0 || kind > 3) return fail(GPK_EINVAL, "Invalid Kernel");
  if (n < 1 || n > K3_MAX_N || q <= 0 || q > QMAX)
    return fail(GPK_EINVAL, "gpk_assemble_pairs4: bad sizes (1 <= n <= 1024, 0 < q <= 64)");
  if (!x || !logw || !logls || !freq || !K_out || !D_out)
    return fail(GPK_EINVAL, "gpk_assemble_pairs4: NULL pointer argument");
  if (!std::isfinite(c4) || !std::isfinite(c3) || !std::isfinite(c2) || !std::isfinite(c1) || !std::isfinite(jitter))
    return fail(GPK_EINVAL, "gpk_assemble_pairs4: c4, c3, c2, c1 and jitter must be finite");
  TRY(check_device(0));
  DevSwitch dsw(0);
  const int P = pad_up(n);
  std::vector<double> kp(3 * (size_t)q);  // flat params laid out (freq, log-ls, log-w)
  std::copy(freq, freq + q, kp.begin());
  std::copy(logls, logls + q, kp.begin() + q);
  std::copy(logw, logw + q, kp.begin() + 2 * q);
  CallScratch tmp("gpk_assemble_pairs4");
  double *dx = nullptr, *dkp = nullptr, *dK = nullptr, *dD = nullptr, *dD1 = nullptr;
  TRY(tmp.alloc(&dx, (size_t)P, true));
  TRY(check_launch(hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice), "gpk_assemble_pairs4"));
  TRY(tmp.upload(&dkp, kp.data(), kp.size()));
  TRY(tmp.alloc(&dK, (size_t)P * P, true));
  TRY(tmp.alloc(&dD, (size_t)P * P, true));
  if (D1_out) TRY(tmp.alloc(&dD1, (size_t)P * P, true));
  AssembleArgs aa{};
  aa.x = dx; aa.n = n; aa.p = P; aa.jitter = jitter; aa.K = dK; aa.D = dD; aa.D1 = dD1;
  aa.deriv = D1_out ? DERIV_HIGH_SPLIT : DERIV_HIGH;
  aa.c4 = c4; aa.c3 = c3; aa.c2 = c2; aa.c1 = c1;
  PrepArgs prep{};
  prep.params = dkp; prep.naxes = 1; prep.skip = 1;  // (no step constants to publish)
  hipError_t e = launch_assemble(kind, q, &aa, 1, prep, 0);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  const size_t row = (size_t)n * sizeof(double);
  for (auto [dst, src] : {std::pair<double*, double*>{K_out, dK}, {D_out, dD}, {D1_out, dD1}})
    if (e == hipSuccess && dst) e = hipMemcpy2D(dst, row, src, (size_t)P * sizeof(double), row, n, hipMemcpyDeviceToHost);
  return check_launch(e, "gpk_assemble_pairs4");
}

// The bi-pair modes (DERIV_HIGH_D2; DERIV_HIGH_SPLIT_D2 when D1_out is given): gpk_assemble_pairs5's
// blocks and the plain order-2 block D2
int gpk_assemble_pairs5(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                        const double* freq, int32_t q, double jitter, double c4, double c3, double c2,
                        double c1, double* K_out, double* D_out, double* D1_out, double* D2_out) {
  if (kind < 0 || kind > 3) return fail(GPK_EINVAL, "Invalid Kernel");
  if (n < 1 || n > K3_MAX_N || q <= 0 || q > QMAX)
    return fail(GPK_EINVAL, "gpk_assemble_pairs5: bad sizes (1 <= n <= 1024, 0 < q <= 64)");
  if (!x || !logw || !logls || !freq || !K_out || !D_out || !D2_out)
    return fail(GPK_EINVAL, "gpk_assemble_pairs5: NULL pointer argument");
  if (!std::isfinite(c4) || !std::isfinite(c3) || !std::isfinite(c2) || !std::isfinite(c1) || !std::isfinite(jitter))
    return fail(GPK_EINVAL, "gpk_assemble_pairs5: c4, c3, c2, c1 and jitter must be finite");
  TRY(check_device(0));
  DevSwitch dsw(0);
  const int P = pad_up(n);
  std::vector<double> kp(3 * (size_t)q);  // flat params laid out (freq, log-ls, log-w)
  std::copy(freq, freq + q, kp.begin());
  std::copy(logls, logls + q, kp.begin() + q);
  std::copy(logw, logw + q, kp.begin() + 2 * q);
  CallScratch tmp("gpk_assemble_pairs5");
  double *dx = nullptr, *dkp = nullptr, *dK = nullptr, *dD = nullptr, *dD1 = nullptr, *dD2 = nullptr;
  TRY(tmp.alloc(&dx, (size_t)P, true));
  TRY(check_launch(hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice), "gpk_assemble_pairs5"));
  TRY(tmp.upload(&dkp, kp.data(), kp.size()));
  TRY(tmp.alloc(&dK, (size_t)P * P, true));
  TRY(tmp.alloc(&dD, (size_t)P * P, true));
  if (D1_out) TRY(tmp.alloc(&dD1, (size_t)P * P, true));
  TRY(tmp.alloc(&dD2, (size_t)P * P, true));
  AssembleArgs aa{};
  aa.x = dx; aa.n = n; aa.p = P; aa.jitter = jitter; aa.K = dK; aa.D = dD; aa.D1 = dD1; aa.D2 = dD2;
  aa.deriv = D1_out ? DERIV_HIGH_SPLIT_D2 : DERIV_HIGH_D2;
  aa.c4 = c4; aa.c3 = c3; aa.c2 = c2; aa.c1 = c1;
  PrepArgs prep{};
  prep.params = dkp; prep.naxes = 1; prep.skip = 1;  // (no step constants to publish)
  hipError_t e = launch_assemble(kind, q, &aa, 1, prep, 0);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  const size_t row = (size_t)n * sizeof(double);
  for (auto [dst, src] : {std::pair<double*, double*>{K_out, dK}, {D_out, dD}, {D1_out, dD1}, {D2_out, dD2}})
    if (e == hipSuccess && dst) e = hipMemcpy2D(dst, row, src, (size_t)P * sizeof(double), row, n, hipMemcpyDeviceToHost);
  return check_launch(e, "gpk_assemble_pairs5");
}

int gpk_assemble_pairs_time(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                            const double* freq, int32_t q, double c2, double c1, int32_t split,
                            int32_t iters, double* avg_us) {
  if (iters < 1 || !avg_us) return fail(GPK_EINVAL, "gpk_assemble_pairs_time: iters >= 1 and avg_us");
  return assemble_pairs_impl(kind, x, n, logw, logls, freq, q, 0.0, c2, c1, nullptr, nullptr, split, iters, avg_us);
}
