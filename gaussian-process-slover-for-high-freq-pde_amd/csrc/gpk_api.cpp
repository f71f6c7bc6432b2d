// gpk_api.cpp — C ABI of libgpk (include/gpk.h): solver handles, device buffers, the
// captured HIP graph of one log-joint step, and the standalone entry points.
//
// One handle = the reference's solver object (GP_solver_1d_single / GP_solver_2d_single /
// GP_solver_2d_single_advection, code/model_GP_solver_{1d,2d,advection}.py) with its params
// and optax state resident in HBM.  step() (model_GP_solver_2d.py:176-183) is one replay of
// a hipGraph that holds every kernel of the step in stream order:
//   prep -> assemble K,D -> SPD inverse (+logdet) -> GEMM stages A..E (2D) | GEMVs (1D)
//   -> hyperparameter-gradient contraction -> deterministic reduction -> loss + Adam.
// A row-sharded handle (gpk_create_sharded / gpk_group_create) runs the 2D step across ranks:
// see "row-sharded multi-GPU step" in gpk_shard.cpp.
//
// This file: the error state, the device check, the standalone kernels, predict with its
// derivative and scattered-point forms, and the small getters and setters; gpk_host.h lists the
// other host translation units.
#include "gpk_host.h"

static thread_local std::string g_err;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int check_launch(hipError_t e, const char* what) {
  if (e != hipSuccess) return fail(GPK_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  return GPK_OK;
}

int gpk_abi_version(void) { return GPK_ABI_VERSION; }

const char* gpk_last_error(void) { return g_err.c_str(); }

int gpk_device_count(int32_t* n) {
  if (!n) return fail(GPK_EINVAL, "n is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) c = 0;
  *n = c;
  return GPK_OK;
}

int check_device(int dev) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess || c == 0) return fail(GPK_ENODEV, "no HIP device visible");
  if (dev < 0 || dev >= c) return fail(GPK_EINVAL, "device ordinal out of range");
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, dev));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(GPK_ENODEV, std::string("libgpk is built for gfx950, device is ") + prop.gcnArchName);
  return GPK_OK;
}

void host_axis_const(const double* logw, const double* logls, const double* freq, int q,
                     AxisConst* kc) {
  std::memset(kc, 0, sizeof(AxisConst));
  for (int c = 0; c < q; ++c) {
    kc->w[c] = std::exp(logw[c]);
    kc->a[c] = std::exp(logls[c]);
    kc->om[c] = TWO_PI * freq[c];
    kc->oml[c] = om_low(freq[c], kc->om[c]);
  }
}

int gpk_kernel_matrices(int32_t kind, int32_t deriv, const double* x1, int32_t n1,
                        const double* x2, int32_t n2, const double* logw, const double* logls,
                        const double* freq, int32_t q, double jitter, double* K_out,
                        double* D_out) {
  if (kind < 0 || kind > 3) return fail(GPK_EINVAL, "Invalid Kernel");
  if (deriv < 0 || deriv > 2) return fail(GPK_EINVAL, "deriv must be 0, 1 or 2");
  if (n1 <= 0 || n2 <= 0 || q <= 0 || q > QMAX) return fail(GPK_EINVAL, "bad sizes (0 < q <= 64)");
  if (!x1 || !x2 || !logw || !logls || !freq || !K_out || (deriv && !D_out))
    return fail(GPK_EINVAL, "NULL pointer argument");
  int dev = 0;
  (void)hipGetDevice(&dev);
  TRY(check_device(dev));
  AxisConst hk;
  host_axis_const(logw, logls, freq, q, &hk);
  CallScratch tmp("gpk_kernel_matrices");
  double *dx1, *dx2, *dK, *dD = nullptr;
  AxisConst* dkc;
  size_t nn = (size_t)n1 * n2;
  TRY(tmp.upload(&dx1, x1, n1));
  TRY(tmp.upload(&dx2, x2, n2));
  TRY(tmp.alloc(&dK, nn));
  if (deriv) TRY(tmp.alloc(&dD, nn));
  TRY(tmp.upload(&dkc, &hk, 1));
  TRY(check_launch(launch_cross(kind, q, dx1, n1, dx2, n2, n2, dkc, jitter, deriv, dK, dD, 0), "cross"));
  HIPCHK(hipMemcpy(K_out, dK, nn * sizeof(double), hipMemcpyDeviceToHost));
  if (deriv) HIPCHK(hipMemcpy(D_out, dD, nn * sizeof(double), hipMemcpyDeviceToHost));
  return GPK_OK;
}

int gpk_kernel_pairs(int32_t kind, int32_t deriv, const double* x1, const double* x2, int64_t n,
                     const double* logw, const double* logls, const double* freq, int32_t q,
                     double* out) {
  if (kind < 0 || kind > 3) return fail(GPK_EINVAL, "Invalid Kernel");
  if (deriv < 0 || deriv > 2) return fail(GPK_EINVAL, "deriv must be 0, 1 or 2");
  if (n <= 0 || q <= 0 || q > QMAX) return fail(GPK_EINVAL, "bad sizes (0 < q <= 64)");
  if (!x1 || !x2 || !logw || !logls || !freq || !out) return fail(GPK_EINVAL, "NULL pointer argument");
  int dev = 0;
  (void)hipGetDevice(&dev);
  TRY(check_device(dev));
  AxisConst hk;
  host_axis_const(logw, logls, freq, q, &hk);
  CallScratch tmp("kernel_pairs");
  double *d1, *d2, *dout;
  AxisConst* dkc;
  TRY(tmp.upload(&d1, x1, (size_t)n));
  TRY(tmp.upload(&d2, x2, (size_t)n));
  TRY(tmp.alloc(&dout, (size_t)n));
  TRY(tmp.upload(&dkc, &hk, 1));
  TRY(check_launch(launch_pairs(kind, q, d1, d2, n, dkc, deriv, dout, 0), "kernel_pairs"));
  return check_launch(hipMemcpy(out, dout, (size_t)n * sizeof(double), hipMemcpyDeviceToHost), "kernel_pairs");
}

int gpk_sync(gpk_handle* h) {
  if (!h) return fail(GPK_EINVAL, "NULL handle");
  DevSwitch ds(h->dev);
  HIPCHK(hipStreamSynchronize(h->s));
  return GPK_OK;
}

int gpk_distance_classes(const double* x, int32_t n, int32_t* ncls, int32_t* vmax) {
  if (!x || n <= 0 || !ncls) return fail(GPK_EINVAL, "bad argument");
  std::vector<double> dist;
  std::vector<int> cid, cbase;
  int vm = 0;
  const bool ok = build_classes(x, n, pad_up(n), dist, cid, cbase, vm);
  *ncls = ok ? (int32_t)dist.size() : 0;
  if (vmax) *vmax = ok ? vm : CLS_VMAX + 1;
  return GPK_OK;
}

int gpk_class_count(const gpk_handle* h, int32_t axis, int32_t* ncls) {
  if (!h || !ncls || axis < 0 || axis >= h->L.naxes) return fail(GPK_EINVAL, "bad argument");
  *ncls = h->cls[axis].ncls;
  return GPK_OK;
}

int gpk_class_sum_path(const gpk_handle* h, int32_t* epilogue) {
  if (!h || !epilogue) return fail(GPK_EINVAL, "bad argument");
  *epilogue = h->cp_on ? 1 : 0;
  return GPK_OK;
}

int gpk_class_pipe(const gpk_handle* h, int32_t* on) {
  if (!h || !on) return fail(GPK_EINVAL, "bad argument");
  *on = cls_pipe_ok(h) ? 1 : 0;
  return GPK_OK;
}

int gpk_set_spd_big_workgroups(int32_t workgroups) {
  if (workgroups < 0) return fail(GPK_EINVAL, "workgroups must be >= 0");
  spd_big_set_workgroups(workgroups);
  return GPK_OK;
}

int gpk_inverse_path(const gpk_handle* h, int32_t* path) {
  if (!h || !path) return fail(GPK_EINVAL, "NULL argument");
  *path = h->bigspd ? (h->bigwide ? GPK_INV_BIG_WIDE : GPK_INV_BIG)
          : h->chain_multi ? GPK_INV_CHAIN_MULTI
          : h->chain_aug ? GPK_INV_CHAIN_AUG : h->chain ? GPK_INV_CHAIN : GPK_INV_SWEEP;
  return GPK_OK;
}

int gpk_graph_mode(const gpk_handle* h, int32_t* fast, int64_t* rollbacks) {
  if (!h) return fail(GPK_EINVAL, "NULL handle");
  if (fast) *fast = (h->fast_ok && h->fast_mode) ? 1 : 0;
  if (rollbacks) *rollbacks = h->rollbacks;
  return GPK_OK;
}

int gpk_criterion(gpk_handle* h, double* out) {
  if (!h || !out) return fail(GPK_EINVAL, "NULL argument");
  double loss;
  TRY(gpk_loss_grad(h, &loss, nullptr));
  DevSwitch ds(h->dev);
  double diag[8];
  HIPCHK(hipMemcpy(diag, h->diag, sizeof(diag), hipMemcpyDeviceToHost));
  const Layout& L = h->L;
  const double Nb = (double)h->prob.nb;
  const double Nc = L.dim == 2 ? (double)L.n1 * L.n2 : (double)L.n1;
  *out = diag[5] / Nb + diag[4] / Nc;  // boundary_gap/Nb + eq_gap/Nc
  return GPK_OK;
}

namespace {

// K^{-1} at the current params: the step's own front (apply = 0), unprofiled
int inverse_front(gpk_handle* h) {
  const bool prof = h->profiling;
  h->profiling = false;
  const int rc = enqueue_assemble_inverse(h, StepCtx{0});
  h->profiling = prof;
  return rc;
}

// Kmn^(d) = the d-th derivative of kappa in its first argument at (xte_i, x_j) of `axis`, no
// jitter, into the zero-filled mp x P block Kmn.  Order 0 is launch_cross's K output and nothing
// else is launched or allocated; above it Kmn takes the D output and K goes to a block of `tmp`.
int cross_deriv(gpk_handle* h, CallScratch& tmp, int axis, const double* dx, int m, int mp, int d,
                double* Kmn) {
  const Layout& L = h->L;
  const int P = axis_p(L, axis);
  double* Kd = nullptr;
  if (d) TRY(tmp.alloc(&Kd, (size_t)mp * P));
  return check_launch(launch_cross(h->prob.kind, L.q, dx, m, axis_x(h, axis), axis_n(L, axis), P, h->kc + axis,
                                   0.0, d, d ? Kd : Kmn, d ? Kmn : nullptr, h->s), "cross");
}

// y = al A x + be C0 over the P1 x P1 factor (the operand as the step reads it: gemv_operand)
int predict_gemv(gpk_handle* h, const double* A, const double* x, double* y, int rows, double al,
                 const double* C0, double be) {
  GemvDesc g{};
  g.A = A; g.lda = h->L.p1; g.x = x; g.y = y; g.p = h->L.p1; g.rows = rows; g.alpha = al;
  g.C0 = C0; g.beta = be; g.epi = EPI_STORE;
  gemv_operand(h, g);
  return check_launch(launch_gemv(g, h->s), "gemv");
}

// alpha = K^{-1} u with one refinement step (matches solve() accuracy; 1d.py:176-179)
int solve_alpha(gpk_handle* h, double* alpha, double* rv) {
  TRY(predict_gemv(h, h->Kinv[0], h->Up, alpha, h->L.p1, 1.0, nullptr, 0.0));
  TRY(predict_gemv(h, h->Kc[0], alpha, rv, h->L.p1, -1.0, h->Up, 1.0));
  return predict_gemv(h, h->Kinv[0], rv, alpha, h->L.p1, 1.0, alpha, 1.0);
}

int launch_gemms(gpk_handle* h, const GemmDesc* d, int n) {
  const int force_big = gemm_force(h->prob.flags);
  for (int i = 0; i < n; ++i)
    TRY(check_launch(launch_gemm_sized(d + i, 1, h->sc, h->s, force_big), "gemm"));
  return GPK_OK;
}

bool order_ok(int d) { return d >= 0 && d <= 2; }

// gpk_predict / gpk_predict_deriv: the (d1, d2) derivative of the interpolant on a test grid
int predict_impl(gpk_handle* h, const double* xte1, int32_t m1, const double* xte2, int32_t m2,
                 int d1, int d2, double* out) {
  if (!h || !xte1 || !out || m1 <= 0) return fail(GPK_EINVAL, "bad argument");
  const Layout& L = h->L;
  if (L.dim == 2 && (!xte2 || m2 <= 0)) return fail(GPK_EINVAL, "2D predict needs xte2");
  if (!order_ok(d1) || (L.dim == 2 && !order_ok(d2))) return fail(GPK_EINVAL, "derivative order must be 0, 1 or 2");
  DevSwitch ds(h->dev);
  TRY(inverse_front(h));
  const int M1p = pad_up(m1), P1 = L.p1;
  CallScratch tmp("predict", h->s);  // (zero-filled: the padding of Kmn and of every product)
  double *dx1, *Kmn1, *res;
  TRY(tmp.alloc(&dx1, m1, true));
  TRY(tmp.alloc(&Kmn1, (size_t)M1p * P1, true));
  HIPCHK(hipMemcpyAsync(dx1, xte1, m1 * sizeof(double), hipMemcpyHostToDevice, h->s));
  // Kmn = kappa(xte_i, x_j) (no jitter), zero-padded to M1p x P1   (model_GP_solver_2d.py:198-202)
  TRY(cross_deriv(h, tmp, 0, dx1, m1, M1p, d1, Kmn1));
  if (L.dim == 1) {
    double *alpha, *rv;
    TRY(tmp.alloc(&alpha, P1, true));
    TRY(tmp.alloc(&res, M1p, true));
    TRY(tmp.alloc(&rv, P1, true));
    TRY(solve_alpha(h, alpha, rv));
    TRY(predict_gemv(h, Kmn1, alpha, res, m1, 1.0, nullptr, 0.0));  // preds = Kmn K^{-1} u
    HIPCHK(hipMemcpyAsync(out, res, m1 * sizeof(double), hipMemcpyDeviceToHost, h->s));
  } else {
    // U_pred = Kmn2 (K2^{-1} (Kmn1 K1^{-1} U)^T), associated exactly as the reference does
    // (model_GP_solver_2d.py:185-220: M1 = Kmn K1inv_U, M2 = solve(K2, M1^T), Kmn2 M2): every
    // intermediate stays O(|U_pred|) after its Kmn product.  (Forming S = K1^{-1} U K2^{-1}
    // first, as rounds 1-2 did, builds entries ~ |U| / jitter^2 whose cancellation in
    // Kmn1 S Kmn2^T cost up to 0.37 relative L2 at C5 with a random field.)
    const int M2p = pad_up(m2), P2 = L.p2;
    double *dx2, *Kmn2, *Aw, *Rw, *Mw, *Nw, *Rm;
    TRY(tmp.alloc(&dx2, m2, true));
    TRY(tmp.alloc(&Kmn2, (size_t)M2p * P2, true));
    for (double** w : {&Aw, &Rw}) TRY(tmp.alloc(w, (size_t)P1 * P2, true));
    for (double** w : {&Mw, &Nw, &Rm}) TRY(tmp.alloc(w, (size_t)M1p * P2, true));
    TRY(tmp.alloc(&res, (size_t)M1p * M2p, true));
    HIPCHK(hipMemcpyAsync(dx2, xte2, m2 * sizeof(double), hipMemcpyHostToDevice, h->s));
    TRY(cross_deriv(h, tmp, 1, dx2, m2, M2p, d2, Kmn2));
    // A = K1^{-1} U and N = M1 K2^{-1} = M2^T, each with one refinement step (solve() accuracy)
    const RefinedSolve sA = refined_solve(false, h->Kc[0], h->Kinv[0], h->Up, Aw, Rw, P1, P2, nullptr),
                       sN = refined_solve(true, h->Kc[1], h->Kinv[1], Mw, Nw, Rm, M1p, P2, nullptr);
    const GemmDesc d[8] = {sA.solve, sA.resid, sA.fix,
                           gemm_desc(Kmn1, P1, 0, Aw, P2, 0, Mw, P2, M1p, P2, P1),  // M1 = Kmn1 A
                           sN.solve, sN.resid, sN.fix,
                           gemm_desc(Nw, P2, 0, Kmn2, P2, 1, res, M2p, M1p, M2p, P2)};  // U_pred = N Kmn2^T
    TRY(launch_gemms(h, d, 8));
    for (int i = 0; i < m1; ++i)
      HIPCHK(hipMemcpyAsync(out + (size_t)i * m2, res + (size_t)i * M2p, m2 * sizeof(double),
                            hipMemcpyDeviceToHost, h->s));
  }
  const hipError_t e = hipStreamSynchronize(h->s);
  if (e != hipSuccess) return fail(GPK_EHIP, std::string("predict: ") + hipGetErrorString(e));
  return read_status(h);
}

}  // namespace

int gpk_predict(gpk_handle* h, const double* xte1, int32_t m1, const double* xte2, int32_t m2,
                double* out) {
  return predict_impl(h, xte1, m1, xte2, m2, 0, 0, out);
}

int gpk_predict_deriv(gpk_handle* h, const double* xte1, int32_t m1, const double* xte2, int32_t m2,
                      int32_t d1, int32_t d2, double* out) {
  return predict_impl(h, xte1, m1, xte2, m2, d1, d2, out);
}

// The same quantity at scattered points, in the reference's association per point: 1D
// sum_j kappa^(d)(x_p, x_j) alpha_j; 2D sum_j kappa2^(d2)(y_p, x2_j) N[p][j] with
// N = (Kmn1^(d1) K1^{-1} U) K2^{-1} -- no Kmn2 and no M x M product.  alpha / A = K1^{-1} U are
// formed once; the points go in chunks of EVAL_CHUNK (the scratch is bounded whatever m), each
// ending in its download and a stream wait, so the host staging vectors can be refilled.
int gpk_evaluate(gpk_handle* h, const double* pts, int64_t m, int32_t d1, int32_t d2, double* out) {
  if (!h || !pts || !out || m <= 0) return fail(GPK_EINVAL, "bad argument");
  const Layout& L = h->L;
  if (!order_ok(d1) || (L.dim == 2 && !order_ok(d2))) return fail(GPK_EINVAL, "derivative order must be 0, 1 or 2");
  DevSwitch ds(h->dev);
  TRY(inverse_front(h));
  const int P1 = L.p1, P2 = L.p2, kind = h->prob.kind;
  const int chunk = (int)std::min<int64_t>(m, EVAL_CHUNK), Cp = pad_up(chunk);
  CallScratch tmp("gpk_evaluate", h->s);
  double *dxp, *dyp = nullptr, *res, *alpha = nullptr, *rv = nullptr, *Kmn1 = nullptr, *Kd = nullptr,
         *Aw = nullptr, *Rw = nullptr, *Mw = nullptr, *Nw = nullptr, *Rm = nullptr;
  TRY(tmp.alloc(&dxp, chunk));
  TRY(tmp.alloc(&res, chunk));
  std::vector<double> hx(chunk), hy(L.dim == 2 ? chunk : 0);
  RefinedSolve sN{};
  GemmDesc gM{};
  if (L.dim == 1) {
    TRY(tmp.alloc(&alpha, P1, true));
    TRY(tmp.alloc(&rv, P1, true));
    TRY(solve_alpha(h, alpha, rv));
  } else {
    TRY(tmp.alloc(&dyp, chunk));
    TRY(tmp.alloc(&Kmn1, (size_t)Cp * P1));
    if (d1) TRY(tmp.alloc(&Kd, (size_t)Cp * P1));
    for (double** w : {&Aw, &Rw}) TRY(tmp.alloc(w, (size_t)P1 * P2, true));
    for (double** w : {&Mw, &Nw, &Rm}) TRY(tmp.alloc(w, (size_t)Cp * P2, true));
    const RefinedSolve sA = refined_solve(false, h->Kc[0], h->Kinv[0], h->Up, Aw, Rw, P1, P2, nullptr);
    const GemmDesc d[3] = {sA.solve, sA.resid, sA.fix};
    TRY(launch_gemms(h, d, 3));
  }
  for (int64_t k = 0; k < chunk_count(m, chunk); ++k) {
    const int64_t p0 = chunk_begin(k, chunk);
    const int mc = chunk_size(m, k, chunk), mcp = pad_up(mc);
    for (int i = 0; i < mc; ++i) {
      hx[i] = pts[(size_t)(p0 + i) * L.dim];
      if (L.dim == 2) hy[i] = pts[(size_t)(p0 + i) * 2 + 1];
    }
    HIPCHK(hipMemcpyAsync(dxp, hx.data(), mc * sizeof(double), hipMemcpyHostToDevice, h->s));
    PointContract pc{};
    pc.m = mc; pc.kc = h->kc; pc.q = L.q; pc.sj = 1; pc.sc = 1; pc.C = 1; pc.out = res;
    if (L.dim == 1) {
      pc.t = dxp; pc.x = h->x1; pc.n = L.n1; pc.T = alpha; pc.sp = 0;
      TRY(check_launch(launch_point_contract(kind, d1, pc, h->s), "point_contract"));
    } else {
      HIPCHK(hipMemcpyAsync(dyp, hy.data(), mc * sizeof(double), hipMemcpyHostToDevice, h->s));
      // Kmn1^(d1) of the chunk, its padding rows zero (so are those of every product below)
      HIPCHK(hipMemsetAsync(Kmn1, 0, (size_t)mcp * P1 * sizeof(double), h->s));
      TRY(check_launch(launch_cross(kind, L.q, dxp, mc, h->x1, L.n1, P1, h->kc, 0.0, d1, d1 ? Kd : Kmn1,
                                    d1 ? Kmn1 : nullptr, h->s), "cross"));
      sN = refined_solve(true, h->Kc[1], h->Kinv[1], Mw, Nw, Rm, mcp, P2, nullptr);
      gM = gemm_desc(Kmn1, P1, 0, Aw, P2, 0, Mw, P2, mcp, P2, P1);  // G = Kmn1 A
      const GemmDesc d[4] = {gM, sN.solve, sN.resid, sN.fix};       // N = G K2^{-1}, refined
      TRY(launch_gemms(h, d, 4));
      pc.t = dyp; pc.x = h->x2; pc.n = L.n2; pc.kc = h->kc + 1; pc.T = Nw; pc.sp = (size_t)P2;
      TRY(check_launch(launch_point_contract(kind, d2, pc, h->s), "point_contract"));
    }
    HIPCHK(hipMemcpyAsync(out + p0, res, mc * sizeof(double), hipMemcpyDeviceToHost, h->s));
    const hipError_t e = hipStreamSynchronize(h->s);
    if (e != hipSuccess) return fail(GPK_EHIP, std::string("gpk_evaluate: ") + hipGetErrorString(e));
  }
  return read_status(h);
}

int gpk_wide_schedule(int32_t T2, int32_t paired, uint32_t* out, int64_t cap) {
  if (T2 < 1 || T2 > 255 || !out) return fail(GPK_EINVAL, "gpk_wide_schedule: T2 in [1, 255], out non-null");
  std::vector<unsigned> tab;
  wide_schedule(T2, paired != 0, tab);
  if ((int64_t)tab.size() > cap) return fail(GPK_EINVAL, "gpk_wide_schedule: cap too small");
  std::memcpy(out, tab.data(), tab.size() * sizeof(unsigned));
  return GPK_OK;
}
