/*
 * gpk.h — C ABI of libgpk, the MI355X-native (gfx950, HIP) hot path of the GP-PDE solver.
 *
 * The reference (xuangu-fang/Gaussian-Process-Slover-for-High-Freq-PDE, pure Python + JAX)
 * has no FFI: its "operator surface" is a handful of Python methods.  Each entry point
 * below replaces one of them; the Python mirror in
 * gaussian-process-slover-for-high-freq-pde_amd/gpk/ binds them with ctypes
 * (INTEGRATION.md shows the binding).  References are to /root/reference/code/.
 *
 * Conventions
 *   - every function returns an int status (GPK_OK = 0); on failure gpk_last_error()
 *     returns a thread-local message.  No C++ exception crosses the ABI.
 *   - all pointers are HOST pointers unless a name ends in _dev; the library copies.
 *   - matrices are row-major; x1 indexes rows (kernel_matrix.py:26).
 *   - fp64 throughout (kernel_matrix.py:6-7 enables jax x64).
 *   - one handle = one HIP device + one HIP stream; calls on a handle are synchronous on
 *     return and not re-entrant; distinct handles are independent.
 */
#ifndef GPK_H_
#define GPK_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPK_ABI_VERSION 2  /* 2: gpk_problem.uoff (extra-GP second phase) */

/* status codes */
enum {
  GPK_OK = 0,
  GPK_EINVAL = 1,  /* bad argument (reference: assert / raise Exception('Invalid Kernel')) */
  GPK_ENOTPD = 2,  /* a covariance factor lost positive definiteness in the SPD inverse   */
  GPK_EHIP = 3,    /* HIP runtime error                                                    */
  GPK_ERCCL = 4,   /* RCCL error (sharded handles)                                         */
  GPK_ENOMEM = 5,  /* device allocation failed                                             */
  GPK_ENODEV = 6   /* no gfx950 device visible                                             */
};

/* kernel kinds: kernel_matrix.py:107-193 */
enum { GPK_SE_COS = 0, GPK_MATERN52_COS = 1, GPK_SE = 2, GPK_MATERN52 = 3 };

/* equation families: model_GP_solver_1d.py:108-116, model_GP_solver_2d.py:131-141,
 * model_GP_solver_advection.py:132-134 */
enum { GPK_POISSON = 0, GPK_ALLENCAHN = 1, GPK_ADVECTION = 2 };

/* Problem description = the solver constructor's arguments + trick_paras.
 *   1D (GP_solver_1d_single.__init__, model_GP_solver_1d.py:38-47):
 *       dim=1, n1=N_col, x1=X_col, src=src_col [n1], bvals=y [nb], bidx=Xind [nb]
 *   2D / advection (GP_solver_2d_single.__init__, model_GP_solver_2d.py:40-48):
 *       dim=2, x1=X_col[0] [n1], x2=X_col[1] [n2], src=src_vals [n1*n2],
 *       bvals=hstack(U[0,:],U[-1,:],U[:,0],U[:,-1]) [2*n2+2*n1], bidx=NULL
 */
typedef struct gpk_problem {
  int32_t dim;          /* 1 or 2 */
  int32_t eq;           /* GPK_POISSON | GPK_ALLENCAHN | GPK_ADVECTION (dim 2 only) */
  int32_t kind;         /* GPK_SE_COS .. GPK_MATERN52 */
  int32_t n1, n2;       /* collocation points per axis (n2 ignored for dim 1) */
  int32_t q;            /* mixture components Q (1..64) */
  const double* x1;
  const double* x2;
  const double* src;
  const double* bvals;
  const int32_t* bidx;  /* dim 1 only */
  int32_t nb;           /* dim 1: len(Xind); dim 2: ignored (2*n1+2*n2) */
  double jitter;        /* 1e-6 in the reference (model_GP_solver_2d.py:432) */
  double llk_weight;    /* trick_paras['llk_weight'] */
  double logdet;        /* trick_paras['logdet'] (1.0 / 0.0) */
  double beta;          /* advection speed (advection-sin.yaml:16); ignored otherwise */
  double lr, b1, b2, eps; /* optax.adam(lr) defaults b1=.9, b2=.999, eps=1e-8 */
  int32_t device;       /* HIP device ordinal */
  int32_t flags;        /* GPK_FLAG_* bits, normally 0 */
  /* dim 1 only, nullable [n1]: a frozen field u0 added to u inside the Allen-Cahn term,
   * (u+u0)((u+u0)^2-1) -- the extra GP's second phase, where the first GP's u is frozen
   * (model_GP_solver_1d_extra.py:86-98).  Its u_xx and u0[Xind] enter as shifted src / bvals. */
  const double* uoff;
} gpk_problem;

/* gpk_problem.flags bits */
#define GPK_FLAG_FORCE_BIG_GEMM 1 /* use the 64x64 throughput GEMM at every size (tests/tuning) */
#define GPK_FLAG_FORCE_BIG_SPD 2  /* use the 64-wide panel/update SPD inverse at every size */
#define GPK_FLAG_FORCE_SMALL_SPD 4 /* use the 32-wide sweep SPD inverse at every size */
#define GPK_FLAG_FORCE_HUGE_GEMM 8 /* use the 128x128 throughput GEMM at every size (tests/tuning) */
/* gpk_step / gpk_loss_grad run one of two captured step graphs: the full one, whose iterative-
 * refinement GEMM stages check a device-side cond(K) gate and skip themselves when it is closed,
 * or a fast one without those stages, chosen while the last observed gate value is 2x below its
 * threshold.  The fast graph checks the gate every step; a step that needed refinement makes the
 * call roll its batch back (params, Adam state) and rerun it with the full graph, so results are
 * bitwise those of the full graph. */
#define GPK_FLAG_NO_FAST_GRAPH 16  /* always run the full graph */
#define GPK_FLAG_FAST_FIRST 32     /* start in fast-graph mode (tests: exercises the rollback) */
/* The step evaluates the covariance fields once per distinct pair distance |x_i - x_j| of each
 * axis (exact fp64 classes, built at gpk_create; ~5n classes on a linspace grid instead of n^2
 * pairs) and contracts the hyper-parameter gradient per class.  K and D are bitwise the per-pair
 * evaluation's; the gradient sums differ only in summation order.  Grids with more than 32
 * distinct distances on one diagonal |i - j| = k fall back to the per-pair kernels. */
#define GPK_FLAG_NO_DCLASS 64      /* always use the per-pair kernels */
/* Small factors (sum of (p/32)^2 over the factors <= 256) are inverted by ONE persistent
 * launch whose workgroups order the pivot sweeps through flags; bitwise the per-sweep launches. */
#define GPK_FLAG_NO_CHAIN 128      /* one launch per pivot sweep instead */
/* 2D, unsharded, chain-sized: the inverse launch also carries U, U^T and D^T as augmented
 * columns of the sweep operator and ends with A = K1^{-1} U, Bt = U K2^{-1} and K^{-1} D^T,
 * which replace the step's first GEMM stage and fold the X1/X2 solves into the G_D stage. */
#define GPK_FLAG_NO_CHAIN_AUG 256  /* the chain inverts K only */
/* Large factors (the panel/update inverse): 128-wide sweeps from a padded size of 3072 (the update
 * is MFMA-bound instead of bound by the matrix traffic), 64-wide below (shorter serial pivots). */
#define GPK_FLAG_FORCE_WIDE_SPD 512   /* 128-wide sweeps at every size (with FORCE_BIG_SPD: tests) */
#define GPK_FLAG_FORCE_NARROW_SPD 1024 /* 64-wide sweeps at every size */
/* Row-sharded handles (nranks >= 2): the first half of the ranks inverts K1 only, the second half
 * K2 only, and the inverses (+ their log-det blocks and refinement gates) are broadcast from
 * ranks 0 and nranks/2 -- one Kronecker factor per rank group instead of both on every rank. */
#define GPK_FLAG_SPLIT_FACTORS 2048
/* 1D factors of padded size >= 1600 (the large-factor range): the persistent chain inverse on
 * 64-row macro tiles of the lower triangle, when its grid is co-resident (p <= 2048 on a full
 * MI355X); GPK_FLAG_NO_CHAIN or GPK_FLAG_FORCE_BIG_SPD select the launch-per-sweep path. */
#define GPK_FLAG_FORCE_CHAIN_MULTI 4096 /* the macro-tile chain at every 1D size (tests) */
/* Large 2D factors (P >= 1600): which solves get one (cond-gated) refinement step.  Default: the
 * forward solves A = K1^{-1} U, Bt = U K2^{-1}; REFINE_ALL: also S and X1 / X2 (every solve, as
 * the small-factor path, whose forward solves are refined on every step, ungated); NO_REFINE:
 * none at any size (explicit-inverse products only; accuracy studies). */
#define GPK_FLAG_REFINE_ALL 8192
#define GPK_FLAG_NO_REFINE 16384
/* Large 1D factors on the macro-tile chain: the inverse launch writes Kc and D as matrices and the
 * GEMVs read them (round-2 form; default: the GEMVs read class ids + class values and the
 * inverse writes neither). Bitwise the same results. */
#define GPK_FLAG_MATRIX_GEMV 32768
/* 128-wide SPD inverse: keep the update's last round of tiles whole (default: quarter tiles when
 * that round would leave most workgroups idle). Bitwise the same results. */
#define GPK_FLAG_NO_QUARTER_TILES 65536
/* Kernel-parameter contraction (distance classes): the derivative fields and every sum after
 * them in double-double (default only for factors of >= 3072 points, where the contraction's
 * cancellation amplifies the fields' fp64 rounding ~1e8-fold), at any size (DD_CONTRACTION) or
 * never (NO_DD_CONTRACTION). */
#define GPK_FLAG_DD_CONTRACTION 131072
#define GPK_FLAG_NO_DD_CONTRACTION 262144
/* 128-wide SPD inverse (factors >= 3072): the handle uploads the unpaired update schedule
 * (gpk_wide_schedule with paired = 0), so every lower tile takes every sweep in its own pass
 * (default: the paired one -- tiles take sweeps in pairs, K = 256 per pass, half the tiles per
 * launch).  Same update kernel either way. */
#define GPK_FLAG_ONE_SWEEP_UPDATE 524288
/* 128-wide SPD inverse: a tile workgroup with a quarter item works it after its whole tiles
 * (default: first, unless its first whole tile is in the next panel's row / column; A/B only).
 * Bitwise the same results. */
#define GPK_FLAG_NO_QUARTER_FIRST 1048576
/* Large 2D factors: refine only the axis-1 forward solve A = K1^{-1} U (not Bt = U K2^{-1}), as
 * the default does when beta >= 16 (advection); diagnostics (tools/c5_refine_diag.py). */
#define GPK_FLAG_REFINE_FWD1_ONLY 2097152
/* 2D factors with distance classes: the class sums of G_K / G_D by a class-sum launch over their
 * rows (default: the 16x16-tile GEMMs that produce them sum each output tile per class in their
 * epilogue, and the contraction adds those partials -- one launch fewer per step). */
#define GPK_FLAG_NO_CLASS_BINS 4194304
/* Chain-inverse handles with distance classes: every step of a multi-step batch evaluates its
 * class values in a launch of its own (default: step s + 1's class values are evaluated at the
 * end of step s's parameter-gradient launch, right after the kernel-parameter Adam, so steps
 * 2.. of a batch start with the inverse launch).  Bitwise the same results; A/B only. */
#define GPK_FLAG_NO_CLASS_PIPE 8388608
/* Persistent chain inverse on 32x32 tiles: the pivot workgroup receives each pivot's two input
 * tiles from their owners (default: it keeps a two-block window and forms them itself while one
 * of its waves factors the previous pivot, from tiles handed over one sweep earlier).  Bitwise
 * the same results; A/B only. */
#define GPK_FLAG_NO_CHAIN_LOOKAHEAD 16777216

typedef struct gpk_handle gpk_handle;

int gpk_abi_version(void);
const char* gpk_last_error(void);
int gpk_device_count(int32_t* n);

/* Kernel_matrix.get_kernel_matrix (kernel_matrix.py:21-30) and the vmap'd derivative
 * covariances (model_GP_solver_2d.py:107-117, model_GP_solver_advection.py:107-117).
 * K_out[n1*n2] = kappa(x1_i, x2_j) + jitter*[i==j]  (pass jitter=0 for the rectangular
 * cross-covariance of preds, model_GP_solver_2d.py:198-202).
 * deriv 1: D_out = D_x1_kappa (kernel_matrix.py:49-52); deriv 2: DD_x1_kappa (:54-57);
 * deriv 0: D_out unused (may be NULL). */
int gpk_kernel_matrices(int32_t kind, int32_t deriv, const double* x1, int32_t n1,
                        const double* x2, int32_t n2, const double* logw, const double* logls,
                        const double* freq, int32_t q, double jitter, double* K_out,
                        double* D_out);

/* vmap(kappa) / vmap(D_x1_kappa) / vmap(DD_x1_kappa) over n elementwise pairs
 * (x1[e], x2[e]) -- the reference's per-pair kernel calls (kernel_matrix.py:26,
 * model_GP_solver_2d.py:107-117): out[e] for deriv 0 / 1 / 2.  No jitter. */
int gpk_kernel_pairs(int32_t kind, int32_t deriv, const double* x1, const double* x2, int64_t n,
                     const double* logw, const double* logls, const double* freq, int32_t q,
                     double* out);

/* Diagnostic: the six double-double derivative fields of ONE mixture component, as the
 * double-double kernel-parameter contraction (GPK_FLAG_DD_CONTRACTION) evaluates them on the
 * device, at n distances d[e] >= 0.  a = e^{log-ls} is taken as given (no device exp); the
 * angular frequency is 2*pi*freq as the exact pair (om, om_low).  deriv 1 or 2.
 * hi / lo [n*6], row e = (f_w, f_l, f_f, d_w, d_l, d_f): the high and low parts of
 * kappa_c / w_c, its d/dlog-ls and d/dfreq, and the same three of D_x1_kappa (deriv 1, unsigned)
 * or DD_x1_kappa (deriv 2). */
int gpk_fields_dd(int32_t kind, int32_t deriv, const double* d, int32_t n, double a, double freq,
                  double* hi, double* lo);

/* Solver object: copies the problem to device memory; params start at the reference init
 * (train(), model_GP_solver_2d.py:245-261 / model_GP_solver_1d.py:203-213) with zero Adam
 * state.  freq_scale sets the initial frequencies linspace(0,1,Q)*freq_scale. */
int gpk_create(const gpk_problem* prob, double freq_scale, gpk_handle** out);
int gpk_destroy(gpk_handle* h);

/* SPD inverse path a handle's step uses (chosen at gpk_create from the factor sizes, the flags
 * and the device): 32-wide per-sweep launches, the persistent chain (K^{-1} only / augmented
 * with the first solves), or the large-factor path. */
enum { GPK_INV_SWEEP = 0, GPK_INV_CHAIN = 1, GPK_INV_CHAIN_AUG = 2, GPK_INV_BIG = 3, GPK_INV_BIG_WIDE = 4,
       GPK_INV_CHAIN_MULTI = 5 };
int gpk_inverse_path(const gpk_handle* h, int32_t* path);
/* The chain's workgroups wait on one another, so gpk_create uses it only when its grid fits the
 * device's co-resident capacity (hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs).  This
 * overrides that capacity for handles created afterwards (workgroups > 0; 0 restores the device
 * query) -- tests use it to force the per-sweep fallback. */
int gpk_set_chain_capacity(int32_t workgroups);
/* Tile workgroups per factor of the large-factor inverse's update launch (0: the default, two per
 * CU).  Applies to every later launch; tests use a few to give each workgroup long tile runs. */
int gpk_set_spd_big_workgroups(int32_t workgroups);
/* Poll budget of every inter-workgroup wait of later launches on the current device (polls > 0;
 * 0 restores the default 2^22).  A wait that spends it -- a hand-off that never arrives, e.g. a
 * persistent grid that is not co-resident -- gives up instead of hanging the device, and every
 * other wait of the handle then gives up within 64 polls: the call returns GPK_ENOTPD ("hand-off
 * timed out") and a gpk_step batch is undone (see gpk_step).  Tests force that path with 1 (every
 * wait whose first poll fails gives up). */
int gpk_set_wait_limit(int32_t polls);
/* Tests: apply the poll budget only while gpk_step runs chunk `chunk` (0-based, 64-step chunks)
 * of a later call; polls = 0 clears it. */
int gpk_set_wait_limit_chunk(int32_t polls, int32_t chunk);

/* Graph selection state (see GPK_FLAG_NO_FAST_GRAPH): *fast = 1 if the next gpk_step uses the
 * fast graph, *rollbacks = batches rerun with the full graph so far.  Either pointer may be NULL. */
int gpk_graph_mode(const gpk_handle* h, int32_t* fast, int64_t* rollbacks);

/* Distance classes (GPK_FLAG_NO_DCLASS) of one coordinate axis x[n], host only (no device):
 * *ncls = classes (distinct |x_i - x_j| per diagonal |i - j|), *vmax = the most on one diagonal;
 * *ncls = 0 when that exceeds 32 (the step then uses the per-pair kernels).
 * gpk_class_count: the classes a handle's step uses on axis 0 / 1 (0 = per-pair kernels). */
int gpk_distance_classes(const double* x, int32_t n, int32_t* ncls, int32_t* vmax);
int gpk_class_count(const gpk_handle* h, int32_t axis, int32_t* ncls);
/* How a 2D class-path step sums G_K / G_D per class: *epilogue = 1 when the GEMMs that produce
 * them write class tile partials (GPK_FLAG_NO_CLASS_BINS off, <= 16 variants per diagonal,
 * 16x16-tile GEMM stages, unsharded), 0 when a class-sum launch reads the matrices. */
int gpk_class_sum_path(const gpk_handle* h, int32_t* epilogue);
/* *on = 1 when a multi-step batch evaluates step s + 1's class values at the end of step s's
 * parameter-gradient launch (chain-inverse handles with distance classes, unsharded,
 * GPK_FLAG_NO_CLASS_PIPE off), 0 when every step launches its own class-value evaluation. */
int gpk_class_pipe(const gpk_handle* h, int32_t* on);

/* Latency-tuning probes (libgpk_trace.so, `make trace`; the product library returns GPK_EINVAL):
 * per timeline slot (csrc/gpk_trace.h) the first-arrival / last-departure device clock
 * (100 MHz) since the last gpk_trace_reset.  n >= 128. */
int gpk_trace_reset(void);
int gpk_trace_read(uint64_t* lo, uint64_t* hi, int32_t n);

/* Flat parameter layout = jax's pytree leaf order (dict keys sorted):
 *   2D: [U (n1*n2, row-major), k1.freq[Q], k1.log-ls[Q], k1.log-w[Q],
 *        k2.freq[Q], k2.log-ls[Q], k2.log-w[Q], log_tau, log_v]
 *   1D: [freq[Q], log-ls[Q], log-w[Q], log_tau, log_v, u[n1]]                       */
int gpk_num_params(const gpk_handle* h, int64_t* n);
int gpk_set_params(gpk_handle* h, const double* flat, int64_t n);
int gpk_get_params(gpk_handle* h, double* flat, int64_t n);
/* Adam state (optax ScaleByAdamState: count, mu, nu), same flat layout */
int gpk_set_opt_state(gpk_handle* h, int64_t count, const double* mu, const double* nu, int64_t n);
int gpk_get_opt_state(gpk_handle* h, int64_t* count, double* mu, double* nu, int64_t n);

/* value_and_grad(loss) at the current params (model_GP_solver_2d.py:145-174,179);
 * grad_flat may be NULL. */
int gpk_loss_grad(gpk_handle* h, double* loss, double* grad_flat);

/* n_steps x step() (model_GP_solver_2d.py:176-183): loss + full gradient + Adam update,
 * params and Adam state device-resident.  losses[n_steps] receives the loss evaluated
 * BEFORE each update (as step() returns it); may be NULL.  Returns once the losses and the
 * device status of the call are final: the last step's U update may still be running, like
 * the reference's asynchronously dispatched jax step; every later call on the handle is ordered
 * after it, and gpk_sync waits for it.  Batches: when the handle has a fast graph (every handle
 * but the row-sharded ones and the large 2D factors), a call is split into 64-step chunks + the
 * remainder, on the fast and on the full (refining) graph alike, and every chunk is a batch of
 * its own; otherwise the whole call is one batch.  A batch that fails on the device -- GPK_ENOTPD:
 * a non-positive pivot or a hand-off timeout -- is undone: params, Adam state and step count are
 * restored from the snapshot the batch took at its start.  Earlier chunks of the same call stay
 * applied (their losses are written), so a failed call may have advanced the handle by a
 * multiple of 64 steps. */
int gpk_step(gpk_handle* h, int32_t n_steps, double* losses);

/* Wait until every launch enqueued on the handle has finished (timing). */
int gpk_sync(gpk_handle* h);

/* Capture and instantiate every step graph a gpk_step(n_steps) call can launch (full and fast,
 * single-step and multi-step) without running a step: graph construction is a one-time host
 * cost of the first call otherwise.  Params and Adam state are untouched. */
int gpk_prepare(gpk_handle* h, int32_t n_steps);

/* preds (model_GP_solver_2d.py:185-220 / model_GP_solver_1d.py:160-180) at the current
 * params: 2D out[m1*m2] (row-major, x-test indexes rows); 1D out[m1] (xte2 ignored). */
int gpk_predict(gpk_handle* h, const double* xte1, int32_t m1, const double* xte2, int32_t m2,
                double* out);

/* d^d1/dx^d1 d^d2/dy^d2 of the interpolant u(x*) = kappa(x*, X) K^{-1} u on the test grid
 * xte1 x xte2 at the current params; d1, d2 in {0, 1, 2}; out as gpk_predict.  The derivative is
 * taken in the test point (kappa's first argument): Kmn_k is D_x1_kappa / DD_x1_kappa in place of
 * kappa, the D block of gpk_kernel_matrices(deriv = d_k, xte_k, x_k), with its sign and JAX's
 * abs'(0) = +1; the solves are gpk_predict's.  1D handles: xte2 / m2 / d2 ignored.  (0, 0) is
 * gpk_predict, bit for bit.  Handles, status codes and side effects (none on params or Adam state)
 * as gpk_predict; GPK_EINVAL on an order outside 0..2. */
int gpk_predict_deriv(gpk_handle* h, const double* xte1, int32_t m1, const double* xte2, int32_t m2,
                      int32_t d1, int32_t d2, double* out);

/* The same quantity at m >= 1 scattered points: pts [m][dim] row-major (dim = the handle's, 1 or
 * 2), out [m].  Per point in the reference's association (model_GP_solver_2d.py:185-220): 1D
 * sum_j kappa^(d1)(x_p, x_j) (K^{-1} u)_j; 2D sum_j kappa2^(d2)(y_p, x2_j) N[p][j] with
 * N = (Kmn1^(d1) K1^{-1} U) K2^{-1}, the kernel fields evaluated on the fly -- O(m (P1 + P2)) memory
 * instead of the m x m grid whose diagonal this is.  The points are walked in chunks of 4096, so
 * the scratch (allocated for the call, freed on return) is bounded whatever m. */
int gpk_evaluate(gpk_handle* h, const double* pts, int64_t m, int32_t d1, int32_t d2, double* out);

/* compute_early_stopping (model_GP_solver_2d.py:222-233): bgap/Nb + egap/Nc */
int gpk_criterion(gpk_handle* h, double* out);

/* value_and_grad_kernel (model_GP_solver_2d.py:87-121 / model_GP_solver_1d.py:80-99) at the
 * current params, computed on the device; `what` selects one field, out gets it unpadded:
 *   2D: 0 K1 [n1*n1], 1 K2 [n2*n2], 2 K1inv_U [n1*n2], 3 K2inv_Ut [n2*n1], 4 U_xx [n1*n2],
 *       5 U_yy [n1*n2]   (advection: U_x, U_y); the reverse pass's kernel-parameter operands
 *       (diagnostics): 6 G_K1, 7 G_D1 [n1*n1], 8 G_K2, 9 G_D2 [n2*n2] (the weights of
 *       sum_ij G_K dK/dtheta + G_D dD/dtheta), 10 K1^{-1} [n1*n1], 11 K2^{-1} [n2*n2],
 *       12 K1^{-1} D1^T [n1*n1], 13 K2^{-1} D2^T [n2*n2] (augmented chain path only), 14 R,
 *       15 X1, 16 X2, 17 S [n1*n2] (model_GP_solver_2d.py:133 residual),
 *       18 Kc1, 19 Kc2 (the step's kept copy of K, refinement residuals), 20 D1, 21 D2 (the
 *       step's derivative blocks) -- the matrices as the last step assembled them; 22 K1,
 *       23 K2, 24 D1, 25 D2 expanded on the host from the distance-class table (class ids +
 *       class values; handles with classes), the gathers' reference
 *   1D: 0 K [n*n], 2 Kinv_u [n], 4 u_xx [n]; 6 K, 7 D [n*n] as the last step assembled them                                                */
int gpk_forward_field(gpk_handle* h, int32_t what, double* out, int64_t n);

/* Per-stage device timings (HIP events on the handle's stream) of one step, averaged over
 * `iters` eager (non-graph) steps run on a saved copy of the state: out_us[stage], names via
 * gpk_stage_name(h, stage).  Returns #stages in *n. */
int gpk_profile_stages(gpk_handle* h, int32_t iters, double* out_us, int32_t cap, int32_t* n);
const char* gpk_stage_name(const gpk_handle* h, int32_t stage);

/* Standalone SPD factor+inverse of the assembled K factor(s) at the current params,
 * `iters` times on the handle's stream; returns average microseconds per call. */
int gpk_time_spd_inverse(gpk_handle* h, int32_t iters, double* avg_us);

/* One kernel of the step, launched `iters` times back to back on the handle's stream
 * between two HIP events (after one full step so its inputs are valid; every listed kernel
 * is idempotent).  name: "assemble" | "sweep" | "gemm_B" | "pgrad" | "spd_chain" | "gather";
 * large-factor inverse: "sweep" / "spd_tiles" (update launch 0 with / without its pivot
 * workgroup), "spd_updates" (every update launch of one inverse, averaged per launch),
 * "spd_pivot" | "spd_panel".  Returns the average device time per launch and the kernel's
 * ALGORITHMIC work per launch (flops, HBM bytes; DESIGN.md §Measurement defines them; the
 * large-factor update launches are credited the tile products their lists schedule). */
int gpk_bench_kernel(gpk_handle* h, const char* name, int32_t iters, double* avg_us,
                     double* alg_flops, double* alg_bytes);

/* The step's fp64 MFMA GEMM kernels on host operands (row-major, device 0), for tests and
 * rate measurements: C = alpha op(A) op(B) + alpha2 op(A2) op(B2) + beta C0, op = transpose
 * when ta / tb / ta2 / tb2; K2 = 0 drops the second product; C0 may equal C (in-place
 * update) or be NULL.  variant: 0 auto (the step's size rule), 1 16x16 latency tiles, 2 64x64
 * tiles, 3 the 128x128 pipelined tile (model_GP_solver_2d.py:104-119's solves and products
 * are these GEMMs here).  M, N, K, K2 multiples of 32 (the step's padding contract); lda etc.
 * in elements.  iters > 0 times that many back-to-back launches with HIP events after the
 * checked one and returns the average microseconds in *avg_us (may be NULL when iters = 0;
 * written only on success).  C receives the checked launch's result; with C0 == C the timed
 * launches keep updating the device copy in place (same work, each on the last one's output). */
int gpk_dgemm(int32_t variant, int32_t M, int32_t N, int32_t K, double alpha, const double* A,
              int32_t lda, int32_t ta, const double* B, int32_t ldb, int32_t tb, int32_t K2,
              double alpha2, const double* A2, int32_t lda2, int32_t ta2, const double* B2,
              int32_t ldb2, int32_t tb2, double beta, const double* C0, double* C, int32_t ldc,
              int32_t iters, double* avg_us);

/* One descriptor of gpk_dgemm_epi: the product of gpk_dgemm with one of the step's fused
 * epilogues.  Everything is a host array, row-major; M, N, K, K2 multiples of 32 (K2 = 0: no
 * second product, A2 / B2 unused), leading dimensions even and at least a row long.
 *   epi GPK_EPI_STORE  C = alpha P1 + alpha2 P2 + beta C0
 *       GPK_EPI_RESID  C = alpha P1 + alpha2 P2 - F [+ u (u^2 - 1), u = U, when ac];
 *                      red[tile] = sum C^2, red2[tile] = sum Q1 Q2  (beta is not applied)
 *       GPK_EPI_QUAD   C = alpha P1 + alpha2 P2 + beta C0; red[tile] = sum C U
 *   vscale / vscale2   alpha / alpha2 multiplied by v (gpk_dgemm_epi's argument)
 *   Y (STORE only)     Y = 0.5 Ys + v C, C the stored value
 *   gate               GPK_GATE_NONE, GPK_GATE_OPEN (identical to none) or GPK_GATE_CLOSED: the
 *                      launch writes nothing, every output keeps what it was uploaded with
 * C0 is NULL (beta must be 0) or has C's shape with ldc0; C0 == C (ldc0 == ldc) is the in-place
 * update.  F, U, Q1, Q2 are M x N with ldf; Ys, Y with ldy.  red / red2 (NULL: not formed) hold
 * red_cap entries; tile t of the variant's square tiles in row-major order (edge tiles sum rows
 * < M and columns < N only) goes to entry t.  C, Y, red and red2 are uploaded before the launch
 * and copied back after it, so entries the launch does not write keep the caller's values.
 * tiles (output) is the variant's tile count of M x N, set whenever variant, M and N are valid. */
enum { GPK_EPI_STORE = 0, GPK_EPI_RESID = 1, GPK_EPI_QUAD = 2 };
enum { GPK_GATE_NONE = 0, GPK_GATE_OPEN = 1, GPK_GATE_CLOSED = 2 };
typedef struct gpk_gemm_case {
  int32_t M, N, K, K2;
  const double* A; const double* B; const double* A2; const double* B2;
  int32_t lda, ldb, lda2, ldb2;
  int32_t ta, tb, ta2, tb2;
  double alpha, alpha2, beta;
  const double* C0; double* C;
  int32_t ldc0, ldc;
  int32_t epi, ac;
  const double* F; const double* U; const double* Q1; const double* Q2;
  const double* Ys; double* Y;
  int32_t ldf, ldy;
  int32_t vscale, vscale2;
  int32_t gate, red_cap;
  double* red; double* red2;
  int32_t tiles;  /* output */
} gpk_gemm_case;

/* One launch of ndesc (1..4) descriptors on GEMM variant 1, 2 or 3 (gpk_dgemm's numbers; the
 * 128x128 tile runs a dual product as two passes and groups the batch by transpose signature),
 * on device 0, for tests: the epilogues, partial slots, edge tiles, gate and batching exactly as
 * the step launches them.  v is the step scalar e^{log v} that vscale, vscale2 and Y read.
 * Every argument is validated before any device work.  Refused with GPK_EINVAL, because the
 * kernels do not support it: Y with an epilogue other than STORE; red with STORE or red2 without
 * RESID; partials with red_cap below the tile count; sizes that are not multiples of 32; odd
 * leading dimensions; beta != 0 without C0; an output (C, Y, red, red2) that is also an input
 * of the batch (other than C0 == C) or another output of it. */
int gpk_dgemm_epi(int32_t variant, int32_t ndesc, gpk_gemm_case* cases, double v);

/* One launch of the step's GEMV (the 1D solver's products) on host operands, device 0, for
 * tests: y = alpha A x + beta C0 with gpk_gemm_case's epilogues on vectors --
 * RESID y -= F [+ u (u^2 - 1), u = U + U0 (U0 nullable)], red[b] = sum y^2; QUAD red[b] = sum y U;
 * red2[b] = sum Q1 Q2 (any epilogue); b = the block of 4 consecutive rows, red / red2 (nullable)
 * hold (rows + 3) / 4 entries.  The operand is the matrix A (rows x p, leading dimension lda), or,
 * when A is NULL, the class form: A[i][j] = cv[cid[i lda + j]] for ids 0 <= id < ncls, 0 for
 * negative (pad) ids, and on the diagonal + cdiag (pads: 1) when ident = 1.  p and lda multiples
 * of 32, lda >= p, 1 <= rows <= p.  C0 (NULL: beta must be 0) may equal y.  y, red and red2 are
 * uploaded before the launch; a closed gate (GPK_GATE_CLOSED) leaves y as uploaded (the
 * partials are formed regardless).  Refused with GPK_EINVAL: red with STORE, a class id >=
 * ncls, y or a partial array that is also an input (other than C0 == y). */
int gpk_dgemv_epi(int32_t p, int32_t rows, const double* A, const int32_t* cid, const double* cv,
                  int32_t ncls, double cdiag, int32_t ident, int32_t lda, const double* x, double alpha,
                  const double* C0, double beta, int32_t epi, int32_t ac, const double* F, const double* U,
                  const double* U0, const double* Q1, const double* Q2, double* red, double* red2,
                  int32_t gate, double* y);

/* The 128-wide SPD inverse's two-sweep update schedule (host only, no device): for T2 128-tiles
 * per dimension, T2 rows of wide_sched_stride(T2) = 2 + T2 (T2 + 1) / 2 words -- per sweep k the
 * tile count, the next pivot tile's entry, then the entries J | I << 8 | two << 16 | c0 << 18 |
 * c1 << 20 | c2 << 22 (coefficient codes 0, 1 = +1, 3 = -1; the tile's new value is
 * c0 X + c1 Z_{k-1}^T Z_{k-1} + c2 Z_k^T Z_k).  paired = 0: the one-sweep form.  Writes at most
 * cap words; returns GPK_EINVAL when cap is too small.  For tests and tools. */
int gpk_wide_schedule(int32_t T2, int32_t paired, uint32_t* out, int64_t cap);

/* ---- Row-sharded 2D step across GPUs (the reference has no multi-GPU path).
 * Every rank holds the problem, forms both Kronecker factors' K, D, K^{-1} itself, and computes
 * its block of rows of every product of the step (model_GP_solver_2d.py:87-183 /
 * advection :87-179); operands read beyond a rank's rows are completed by in-place all-gathers,
 * the kernel-parameter partials and per-tile loss partials by all-reduces.  Loss, gradients of
 * the small params and their Adam update are identical on every rank; Adam on U updates the
 * rank's rows (gathered after the step).  gpk_step / gpk_loss_grad run this step on a sharded
 * handle; gpk_loss_grad's U gradient is valid on the rank's rows only (gpk_shard_info). */

/* 128-byte RCCL communicator id: rank 0 creates it, every rank passes the same bytes. */
int gpk_comm_unique_id(uint8_t* out, int32_t len);
/* One rank (one process, device = problem.device) of an RCCL (xGMI) group of nranks. */
int gpk_create_sharded(const gpk_problem* p, double freq_scale, int32_t rank, int32_t nranks,
                       const uint8_t* comm_id, gpk_handle** out);
/* nranks handles on ONE device in this process, exchanging through device copies (the same
 * sharded step without RCCL: tests on a single GPU).  Driven by gpk_group_step /
 * gpk_group_loss_grad (one host thread per rank); gpk_step on them returns GPK_EINVAL. */
int gpk_group_create(const gpk_problem* p, double freq_scale, int32_t nranks, gpk_handle** out);
int gpk_group_step(gpk_handle** hs, int32_t nranks, int32_t n_steps, double* losses);
/* loss and the FULL flat gradient (U rows collected from their owners) */
int gpk_group_loss_grad(gpk_handle** hs, int32_t nranks, double* loss, double* grad_flat);
/* this handle's rank, group size and rows [row0, row0 + rows) of U it owns */
int gpk_shard_info(const gpk_handle* h, int32_t* rank, int32_t* nranks, int32_t* row0, int32_t* rows);
/* the sharded step's plan as text (NUL-terminated, <= cap bytes): per GEMM stage "s<k>:" and one
 * mode letter per product -- r = this rank's output rows, k = its share of the contraction
 * index, f = whole (replicated) -- then " g<buffer>" for each all-gather after that stage; the
 * step ends with "ar" (its one all-reduce: status, contraction partials, loss partials) and "gU"
 * (U rows after Adam).  gpk/shard.py shard_plan restates it (tests/test_shard.py). */
int gpk_shard_plan(const gpk_handle* h, char* out, int64_t cap);

/* ---- 3-axis Kronecker solver (the d > 2 generalisation) ------------
 * The reference's GP_solver_2d_single log joint (model_GP_solver_2d.py:87-183) with
 * K = K1 (x) K2 (x) K3 on a tensor grid: prior -1/2 c sum_k (prod_{j!=k} N_j) logdet K_k -
 * 1/2 <U, K^{-1} U> (the 2-axis weights :157-162), residual sum_k (D_k K_k^{-1}) x_k U - F
 * [+ U(U^2-1)], boundary on the six faces.  Flat params (sorted-key pytree order): U
 * [n1*n2*n3 row-major], k1.{freq, log-ls, log-w}[Q], k2..., k3..., log_tau, log_v. */
typedef struct gpk_problem3 {
  int32_t eq;           /* GPK_POISSON | GPK_ALLENCAHN */
  int32_t kind;         /* GPK_SE_COS .. GPK_MATERN52 */
  int32_t n1, n2, n3;   /* collocation points per axis */
  int32_t q;            /* mixture components Q (1..64) */
  const double* x1;
  const double* x2;
  const double* x3;
  const double* src;    /* [n1*n2*n3] row-major */
  const double* bvals;  /* faces U[0], U[-1], U[:,0], U[:,-1], U[:,:,0], U[:,:,-1], each row-major:
                         * [2(n2 n3 + n1 n3 + n1 n2)] */
  double jitter, llk_weight, logdet;
  double lr, b1, b2, eps;
  int32_t device;
  int32_t flags;        /* GPK_FLAG3_* bits, normally 0 */
} gpk_problem3;
/* One refinement step X += K_k^{-1} (B - K_k X) after each of the step's eight solves (A1, A2, A3,
 * T = A1 x_3 K3^{-1}, S, X1, X2, X3), as the 2-axis step has: each is gated on the
 * device on its own axis's bound K_00 max diag K_k^{-1} (> 100 opens it), placed directly after
 * the launch that forms the solve, so every later product reads the corrected value.  The handle
 * keeps a copy of each K_k (written by the assembly launch).  With the bit clear the handle
 * allocates, captures and launches exactly the unrefined step.  With it set and every gate
 * closed the results equal the unrefined step's bit for bit.  (Its own bit space: the 2-axis
 * GPK_FLAG_* values mean nothing here.) */
#define GPK_FLAG3_REFINE 1
/* The refinement's kernels (with GPK_FLAG3_REFINE).  Default: the fused panel kernel (one launch
 * per solve, the X and residual panels in LDS; it measured faster at every size it runs at)
 * whenever every padded size is <= 512 (both panels fit LDS), else two gated GEMMs per solve.
 * GPK_FLAG3_REFINE_GEMM forces the two GEMMs (tests, A/B). */
#define GPK_FLAG3_REFINE_GEMM 2

typedef struct gpk_handle3 gpk_handle3;
int gpk_create3(const gpk_problem3* p, double freq_scale, gpk_handle3** out);
int gpk_destroy3(gpk_handle3* h);

/* The same solver for a stated operator instead of one of the two built-in equations: one
 * derivative order and one weight per axis, a constant-coefficient reaction polynomial, and the
 * set of faces that carry boundary data (an initial-value problem leaves its final-time face
 * open).  Residual on the grid
 *     R = sum_k c_k (D_k^(o_k) K_k^{-1}) x_k U - F + r1 U + r2 U^2 + r3 U^3,
 * D_k^(1) = D_x1_kappa, D_k^(2) = DD_x1_kappa of axis k (gpk_kernel_matrices deriv 1 / 2); the log
 * joint is gpk_create3's with this R, and its boundary term, Nb (in the loss, in d/d log_tau, in
 * gpk_criterion3 and gpk_loss_terms3's boundary_gap) run over the active faces only.  An edge
 * shared by two active faces counts twice, as on a legacy handle; an edge between an active and
 * an open face counts once.  Examples with the third axis as time: heat u_t - nu (u_xx + u_yy):
 * order (2,2,1), coef (-nu,-nu,1), faces 31; transport b1 u_x + b2 u_y + u_t: order (1,1,1), coef
 * (b1,b2,1); Helmholtz: order (2,2,2), coef (1,1,1), react (k^2,0,0); Allen-Cahn in time:
 * order (2,2,1), coef (-eps,-eps,1), react (-1,0,1), faces 31.
 * Two orders on one axis (a d^2 + b d) are stated with gpk_operator3x / gpk_create3_opx below.
 * Coefficients that vary over the grid are stated with gpk_coef3 / gpk_create3_opv below.
 * Derivative (Neumann / initial-velocity) boundary data is stated with gpk_bdata3 / gpk_create3_opn. */
typedef struct gpk_operator3 {
  int32_t order[3];  /* 1 or 2: the derivative taken along axis k (D_x1_kappa / DD_x1_kappa block) */
  double  coef[3];   /* its weight c_k, any finite value (0 drops that axis's term)               */
  double  react[3];  /* r1, r2, r3: + r1 u + r2 u^2 + r3 u^3 in the residual                      */
  int32_t faces;     /* bit f set: face f carries boundary data; f in gpk_problem3.bvals order:
                        0: i1=0, 1: i1=n1-1, 2: i2=0, 3: i2=n2-1, 4: i3=0, 5: i3=n3-1.  1..63    */
} gpk_operator3;
/* p->eq must be GPK_POISSON (the operator says everything else); p->flags as on gpk_create3, both
 * GPK_FLAG3_REFINE bits included.  p->bvals keeps the six-face layout and length whatever the
 * mask: entries of open faces are never read and may be NaN.  GPK_EINVAL on a NULL op, an order
 * outside {1, 2}, a non-finite coef or react, faces outside 1..63, or eq != GPK_POISSON.  Every
 * other gpk_*3 call works on such a handle unchanged (predictions, derivatives and scattered
 * points depend on K_k only).  order (2,2,2), coef (1,1,1), react 0, faces 63 is gpk_create3's
 * Poisson handle bit for bit; react (-1,0,1) is its Allen-Cahn handle up to rounding (the legacy
 * handle evaluates u(u^2 - 1)). */
int gpk_create3_op(const gpk_problem3* p, const gpk_operator3* op, double freq_scale, gpk_handle3** out);
/* What the handle runs: gpk_create3_op's operator, or a gpk_create3 handle's equivalent (orders 2,
 * weights 1, faces 63, react 0 for Poisson and (-1,0,1) for Allen-Cahn).  GPK_EINVAL on a
 * gpk_create3_opx handle with a mixed-order axis: this struct cannot state it (gpk_operator_info3x
 * works on every 3-axis handle). */
int gpk_operator_info3(const gpk_handle3* h, gpk_operator3* out);

/* Operators with a second- and a first-order term on the same axis (convection-diffusion,
 * u_t + beta . grad u - nu lap u + r(u) = f).  Residual on the grid
 *     R = sum_k (c2_k D_k^(2) + c1_k D_k^(1)) K_k^{-1} x_k U - F + r1 U + r2 U^2 + r3 U^3;
 * the log joint, boundary term, Nb, criterion and loss terms as on a gpk_create3_op handle.  Per
 * axis: exactly one non-zero weight is gpk_operator3's order 2 or 1 with that weight, both zero is
 * order 2 with weight 0 -- a handle without a mixed axis equals the gpk_create3_op handle of the
 * same operator bit for bit.  Both non-zero is a mixed axis: its assembled block is
 * D_k = c2_k DD_x1_kappa + c1_k D_x1_kappa (neither symmetric nor antisymmetric; both fields from
 * one evaluation per pair and mixture component) and every product with D_k has weight exactly 1.
 * Example, third axis time: u_t + b1 u_x + b2 u_y - nu (u_xx + u_yy): c2 (-nu,-nu,0), c1 (b1,b2,1),
 * faces 31.  The 1- and 2-axis handles and sharded handles take no such operator. */
typedef struct gpk_operator3x {
  double  c2[3];    /* weight of d^2/dx_k^2 (DD_x1_kappa block) */
  double  c1[3];    /* weight of d/dx_k     (D_x1_kappa block)  */
  double  react[3]; /* r1, r2, r3 as in gpk_operator3           */
  int32_t faces;    /* as in gpk_operator3, 1..63               */
} gpk_operator3x;
/* p as on gpk_create3_op.  GPK_EINVAL on a NULL op, a non-finite c2, c1 or react, faces outside
 * 1..63, or eq != GPK_POISSON.  Every other gpk_*3 call works on such a handle unchanged. */
int gpk_create3_opx(const gpk_problem3* p, const gpk_operator3x* op, double freq_scale, gpk_handle3** out);
/* What any 3-axis handle runs, in this form: a gpk_create3 or gpk_create3_op handle reports its
 * equivalent (the weight under c2 or c1 by its order, the other 0). */
int gpk_operator_info3x(const gpk_handle3* h, gpk_operator3x* out);

/* Coefficients that vary over the grid: a field a_k(x) on axis k's term and a field rho(x) on the
 * linear reaction term (Helmholtz in a medium, lap u + k(x)^2 u; heat in a heterogeneous
 * conductor, u_t - nu(x,y) (u_xx + u_yy); transport in a non-uniform flow; a potential V(x) u).
 * With T_k = (c2_k D_k^(2) + c1_k D_k^(1)) K_k^{-1} x_k U exactly as on the gpk_create3_opx handle
 * of the same `op` (constant weights included), the residual on the grid is
 *     R = a_1 . T_1 + a_2 . T_2 + a_3 . T_3 - F + (r1 + rho) . U + r2 U^2 + r3 U^3
 * ( . elementwise); the log joint, boundary term, Nb, criterion and loss terms are those of the
 * opx handle with this R.  The fields are problem data like src: given at the collocation points,
 * copied at creation, never part of the parameter vector.  One field serves both terms of a
 * mixed-order axis; r2 and r3 stay constants.  Not expressible: two different fields on the two
 * terms of one axis (divergence form -div(a grad u)). */
typedef struct gpk_coef3 {
  const double* a[3]; /* per axis: NULL (identically 1) or n1*n2*n3 values, row-major [i1][i2][i3] like src */
  const double* rho;  /* NULL (identically 0) or the same layout: + rho . u in the residual               */
} gpk_coef3;
/* p and op as on gpk_create3_opx, with its GPK_EINVAL cases; also GPK_EINVAL on a non-finite value
 * in a given field.  cf == NULL, or all four pointers NULL, is gpk_create3_opx itself: the same
 * handle, graph and kernels.  gpk_operator_info3x / gpk_operator_info3 report the constant part,
 * as for the opx handle of the same op.  Every other gpk_*3 call works on such a handle unchanged. */
int gpk_create3_opv(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf,
                    double freq_scale, gpk_handle3** out);
/* has[0..2]: axis k has a field; has[3]: rho is present.  Any 3-axis handle; all zeros on a handle
 * of gpk_create3, gpk_create3_op or gpk_create3_opx. */
int gpk_coef_info3(const gpk_handle3* h, int32_t has[4]);

/* Data on the derivative of u on faces (Neumann walls; the initial velocity u_t(., 0) of the wave
 * equation u_tt - c^2 lap u = f, third axis time, next to u(., 0) on the same face).  Face
 * f = 2k + s belongs to axis k (gpk_operator3.faces' bit order) at index i_f = 0 or n_k - 1.  The
 * data is d u / d x_k ALONG THE COORDINATE x_k, not along the outward normal: on a face with s = 0
 * the outward normal derivative is its negative.  The model's value on face f is
 *     g_f = d_f ._k (K_k^{-1} x_k U),   d_f[j] = D_x1_kappa_k(x_{i_f}, x_j)
 * (row i_f of gpk_kernel_matrices' deriv 1 block, whatever orders the operator has on axis k), and
 * dgap = sum_f ||g_f - h_f||^2 over the faces of dfaces, Nd = their entries.  The log joint is the
 * gpk_create3_opv handle's with boundary_gap + dgap and Nb + Nd in place of boundary_gap and Nb:
 * in the loss, in d/d log_tau, in gpk_criterion3 and in gpk_loss_terms3's boundary_gap.  A face may
 * carry both kinds of data: each of its entries then counts once in Nb and once in Nd; no edge
 * gets special treatment.  One precision tau serves both kinds.  Not built: tangential or oblique
 * derivatives, Robin data, and derivative data on sharded, 1-axis and 2-axis handles or on the
 * class path. */
typedef struct gpk_bdata3 {
  int32_t dfaces;       /* bit f set: face f carries d u / d x_k data (k = f / 2); 0..63 */
  const double* dvals;  /* gpk_problem3.bvals' six-face layout; entries of faces outside dfaces are never read */
} gpk_bdata3;
/* p, op and cf as on gpk_create3_opv (cf may be NULL).  bd == NULL or dfaces == 0 is
 * gpk_create3_opv(p, op, cf, ...) itself: the same stage list, launches and bits.  With
 * dfaces != 0, op->faces may be 0 (derivative data alone; the operator then needs a reaction term
 * to pin the constant).  GPK_EINVAL, before any device work, on dfaces outside 0..63, dvals NULL
 * with dfaces != 0, or a non-finite value on a face of dfaces. */
int gpk_create3_opn(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf,
                    const gpk_bdata3* bd, double freq_scale, gpk_handle3** out);
/* The faces that carry values and derivatives; dfaces is 0 on every older kind of 3-axis handle. */
int gpk_bdata_info3(const gpk_handle3* h, int32_t* faces, int32_t* dfaces);
/* out: value gap, derivative gap, Nb, Nd as the last gpk_step3 or gpk_loss_grad3 left them (the
 * gaps at the parameters before that step's update).  Any 3-axis handle; derivative gap and Nd
 * are 0 on the older kinds. */
int gpk_boundary_terms3(gpk_handle3* h, double out[4]);

/* Convective terms (viscous and inviscid Burgers: u_t + u (u_x + u_y) - nu lap u = f).  Axis k adds
 *     g_k . u . d u / d x_k
 * to the equation of a gpk_create3_opn handle; with A_k = K_k^{-1} x_k U and D1_k the plain order-1
 * block of axis k, V_k = g_k D1_k x_k A_k, N = sum_k V_k and the residual is the opn handle's plus
 * U . N.  g_k is a CONSTANT: the gpk_coef3 fields multiply the linear terms of their axis only,
 * never this one.  An axis may have c2_k = c1_k = 0 with g_k != 0 (inviscid).  Everything else --
 * the log joint, the boundary and derivative-boundary terms, gpk_criterion3, gpk_loss_terms3,
 * gpk_boundary_terms3, the Adam update -- keeps its formula on the new residual; predictions
 * depend on K_k only.  Not built: the sharded, 1-axis and 2-axis handles, a field on the
 * convective term, systems of equations, the conservative form d(u^2 / 2) / dx_k. */
typedef struct gpk_conv3 { double g[3]; } gpk_conv3;
/* p, op, cf and bd as on gpk_create3_opn (cf and bd may be NULL).  cv == NULL or all three
 * g_k == 0.0 is gpk_create3_opn(p, op, cf, bd, ...) itself: the same stage list, launches and bits.
 * GPK_EINVAL, before any device work, on a non-finite g_k, and on everything gpk_create3_opn,
 * gpk_create3_opv and gpk_create3_opx reject. */
int gpk_create3_opc(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf,
                    const gpk_bdata3* bd, const gpk_conv3* cv, double freq_scale, gpk_handle3** out);
/* The convective weights; zeros on every older kind of 3-axis handle. */
int gpk_conv_info3(const gpk_handle3* h, double g[3]);

/* Mixed partials (a rotated or sheared anisotropic medium, -div(A grad u) with off-diagonal A; an
 * equation in non-orthogonal coordinates).  The pair (j, k), j < k, adds
 *     m_jk . d^2 u / d x_j d x_k
 * to the equation of a gpk_create3_opc handle; m holds the weights of the pairs (1,2), (1,3), (2,3)
 * in that order.  With A_j = K_j^{-1} x_j U and D1_k the plain order-1 block of axis k,
 *     Z_j = D1_j x_j A_j,   H_jk = K_k^{-1} x_k Z_j,   C_jk = m_jk D1_k x_k H_jk,
 * and the residual is the opc handle's plus C_13 + C_12 + C_23 (that order, each only where its
 * weight is non-zero).  m_jk is a CONSTANT: the gpk_coef3 fields multiply the linear terms of their
 * own axis only, never a cross term.  A pair's axes may have c2 = c1 = 0.  Everything else -- the
 * log joint, the boundary and derivative-boundary terms, gpk_criterion3, gpk_loss_terms3,
 * gpk_boundary_terms3, the Adam update -- keeps its formula on the new residual; predictions depend
 * on K_k only.  gpk_stage_variants3 reports eight further GEMM launches on a handle with any pair
 * set, whichever pairs they are: three after the convective handle's first (Z_j; H_jk; C_jk), four
 * after its second (the reverse products D1_k^T x_k R; their solves; the sums into T_j; the G_D1)
 * and one at the end (the sums into G_Kk).  Not built: the sharded, 1-axis and 2-axis handles, a
 * field on a cross weight, mixed terms of total order above two. */
typedef struct gpk_cross3 { double m[3]; } gpk_cross3;
/* p, op, cf, bd and cv as on gpk_create3_opc (cf, bd and cv may be NULL).  mx == NULL or all three
 * m == 0.0 is gpk_create3_opc(p, op, cf, bd, cv, ...) itself: the same stage list, launches and
 * bits.  GPK_EINVAL, before any device work, on a non-finite m, and on everything gpk_create3_opc,
 * gpk_create3_opn, gpk_create3_opv and gpk_create3_opx reject. */
int gpk_create3_opm(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf,
                    const gpk_bdata3* bd, const gpk_conv3* cv, const gpk_cross3* mx, double freq_scale,
                    gpk_handle3** out);
/* The cross weights (1,2), (1,3), (2,3); zeros on every older kind of 3-axis handle. */
int gpk_cross_info3(const gpk_handle3* h, double m[3]);

/* Drift fields (divergence form -div(a grad u) = -a lap u - grad a . grad u: Darcy flow, heat in
 * conservation form; convection-diffusion with a variable velocity and a constant viscosity;
 * Fokker-Planck / Ornstein-Uhlenbeck drifts).  Axis k adds
 *     b_k(x) . d u / d x_k
 * ( . elementwise) to the equation of a gpk_create3_opm handle: with A_k = K_k^{-1} x_k U and D1_k
 * the plain order-1 block of axis k, Z_k = D1_k x_k A_k and the residual is the opm handle's plus
 * b_1 . Z_1 + b_3 . Z_3 + b_2 . Z_2 (that order, after the cross terms, each only where its field
 * is given).  b_k is problem data like the gpk_coef3 fields: given at the collocation points,
 * copied at creation, never part of the parameter vector.  It is a field of its own: THE gpk_coef3
 * FIELDS a_k DO NOT MULTIPLY THE DRIFT TERM (a_k serves c2_k d^2 + c1_k d of its axis, b_k stands
 * alone), which is what divergence form needs: c2_k a on the second derivative and c2_k da/dx_k as
 * b_k on the first.  A drift axis may have c2_k = c1_k = g_k = 0.  Everything else -- the log
 * joint, the boundary and derivative-boundary terms, gpk_criterion3, gpk_loss_terms3,
 * gpk_boundary_terms3, the Adam update -- keeps its formula on the new residual; predictions depend
 * on K_k only.  gpk_stage_variants3 reports two or three further GEMM launches on a handle with any
 * drift field: one after the convective handle's first launch (the Z_k; absent when every drift
 * axis's Z_k is already a cross pair's: axis 1 of the pairs (1,2) and (1,3), axis 2 of (2,3)), and
 * two after the cross handle's G_D1 launch, before the X_k (the sums into T_k; the G_D1k).  Not
 * built: fields on g_k and on m_jk, the sharded, 1-axis and 2-axis handles, the class path. */
typedef struct gpk_drift3 {
  const double* b[3]; /* per axis: NULL (no drift term) or n1*n2*n3 values, row-major [i1][i2][i3] like src */
} gpk_drift3;
/* p, op, cf, bd, cv and mx as on gpk_create3_opm (cf, bd, cv and mx may be NULL).  dr == NULL or
 * all three pointers NULL is gpk_create3_opm(p, op, cf, bd, cv, mx, ...) itself: the same stage
 * list, launches and bits.  GPK_EINVAL, before any device work, on a non-finite value in a given
 * drift field, and on everything gpk_create3_opm, gpk_create3_opc, gpk_create3_opn, gpk_create3_opv
 * and gpk_create3_opx reject. */
int gpk_create3_opb(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf,
                    const gpk_bdata3* bd, const gpk_conv3* cv, const gpk_cross3* mx, const gpk_drift3* dr,
                    double freq_scale, gpk_handle3** out);
/* has[k]: axis k has a drift field; zeros on every older kind of 3-axis handle. */
int gpk_drift_info3(const gpk_handle3* h, int32_t has[3]);

/* Third- and fourth-order terms (KdV u_t + u u_x + delta u_xxx; Kuramoto-Sivashinsky u_t + u u_x +
 * u_xx + nu u_xxxx axis-wise; the Euler-Bernoulli beam u_tt + kappa u_xxxx with clamped ends; the
 * linear part of Cahn-Hilliard).  Axis k adds
 *     c4_k d^4 u / d x_k^4 + c3_k d^3 u / d x_k^3
 * to the linear operator of a gpk_create3_opb handle: the assembled block of that axis becomes
 *     D_k = c4_k D4_k + c3_k D3_k + c2_k DD_k + c1_k D1_k,
 * Dn_k[i][j] the n-th derivative in the first argument of kappa_k at (x_i, x_j): per mixture
 * component sum_m C(n, m) m_m(d) c_{n-m}(d) with c_0..c_4 = C, -om S, -om^2 C, om^3 S, om^4 C and the
 * radial derivatives m_3, m_4 in closed form.  Odd orders carry the sign s_ij of x_i - x_j (s = +1
 * at 0; their diagonal is exactly 0), even orders are symmetric.  Such an axis is entered like a
 * mixed-order one: every product with its D_k has GEMM weight exactly 1.0.  The gpk_coef3 field a_k
 * multiplies the whole term of its axis, all four orders.  Convective terms, cross pairs, drift
 * terms and derivative face data on the same axis keep using the plain order-1 block D1_k.  Nothing
 * else in the log joint changes: the boundary and derivative-boundary terms, gpk_criterion3,
 * gpk_loss_terms3 and gpk_boundary_terms3 keep their formulas; the stage list, the refinement and the
 * face kernels are those of the same handle without the high-order weights.
 * ORDER 4 IS THE CEILING: the Matern-5/2 radial factor has a continuous fourth derivative with a
 * kink at d = 0 and no fifth derivative, and both kernel families stop there.
 * Not built: orders above four; boundary data on second derivatives (simply supported ends); the sharded, 1-axis and
 * 2-axis handles; the class path; derivatives above 2 in gpk_predict_deriv3 and gpk_evaluate3, which
 * keep rejecting 3. */
typedef struct gpk_high3 {
  double c4[3]; /* weight of d^4 u / d x_k^4 */
  double c3[3]; /* weight of d^3 u / d x_k^3 */
} gpk_high3;
/* p, op, cf, bd, cv, mx and dr as on gpk_create3_opb (cf, bd, cv, mx and dr may be NULL).  hi == NULL
 * or all six weights 0.0 is gpk_create3_opb(p, op, cf, bd, cv, mx, dr, ...) itself: the same stage
 * list, launches and bits.  GPK_EINVAL, before any device work, on a non-finite weight, and on
 * everything the older create calls reject. */
int gpk_create3_oph(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf,
                    const gpk_bdata3* bd, const gpk_conv3* cv, const gpk_cross3* mx, const gpk_drift3* dr,
                    const gpk_high3* hi, double freq_scale, gpk_handle3** out);
/* The high-order weights; zeros on every older kind of 3-axis handle.  gpk_operator_info3x keeps
 * reporting c2 and c1; gpk_operator_info3 returns GPK_EINVAL on a handle with a high-order axis, as
 * it does for a mixed axis. */
int gpk_high_info3(const gpk_handle3* h, double c4[3], double c3[3]);

/* Mixed fourth-order partials (the Kirchhoff plate u_tt + kappa Delta^2 u, the true biharmonic
 * Delta^2, Swift-Hohenberg, the linear part of Cahn-Hilliard in two space dimensions).  A pair
 * (j, k), j < k, of weight q_jk != 0 adds
 *     q_jk d^4 u / d x_j^2 d x_k^2
 * (u_xxyy for the pair (1,2)) to the equation of a gpk_create3_oph handle.  q_jk is a constant, like m_jk: the gpk_coef3 fields
 * a_k do not multiply it, and the reverse pass reads R itself, never W_k.  Everything is fp64.  With
 * A_j, T_j, K_k^{-1} and R as on the oph handle and DD_k the plain, unweighted second-derivative
 * block of axis k (the block gpk_assemble_pairs assembles at c1 = 0), per present pair:
 *     Z2_j  = DD_j x_j A_j                    (shared by the pairs (1,2) and (1,3))
 *     H2_jk = K_k^{-1} x_k Z2_j               (a solve)
 *     B_jk  = q_jk DD_k x_k H2_jk
 *     R     = [the oph handle's R, drift terms included] + B_13 + B_12 + B_23   (that fixed order)
 *     Hb2_jk = q_jk DD_k^T x_k R,   Zb2_jk = K_k^{-1} x_k Hb2_jk   (a solve)
 *     G_DDk += v q_jk R_(k) H2_jk,(k)^T,   G_Kk -= v Zb2_jk,(k) H2_jk,(k)^T        (outer axis)
 *     G_DDj += v Zb2_jk,(j) A_j,(j)^T,     T_j += DD_j^T x_j Zb2_jk before X_j = K_j^{-1} x_j T_j
 * The drift outputs E_k = b_k R are formed on the final R; eq_gap, the log joint, the boundary and
 * derivative-boundary terms, gpk_criterion3, gpk_loss_terms3, gpk_boundary_terms3 and the Adam
 * kernels keep their formulas on the new R; predictions depend on K_k only.  Both axes of a pair
 * are entered like mixed-order ones and may have every other weight zero; they always assemble and
 * contract with the four-field evaluation.  Under GPK_FLAG3_REFINE both solves of a pair are refined
 * on both routes, gated on the outer axis.  gpk_stage_variants3 reports eight further launches.
 * The per-axis ceiling of order four is untouched: Delta^2 needs only the second derivative of each
 * factor, which Matern-5/2 has.
 * Not built: fields on q; pairs of other orders such as u_xxxy or u_xyy; boundary data on second
 * derivatives; the sharded, 1-axis and 2-axis handles; the class path. */
typedef struct gpk_bicross3 {
  double q[3]; /* pairs (1,2), (1,3), (2,3) */
} gpk_bicross3;
/* p, op, cf, bd, cv, mx, dr and hi as on gpk_create3_oph (all but p and op may be NULL).  bq == NULL
 * or q = (0, 0, 0) is gpk_create3_oph(p, op, cf, bd, cv, mx, dr, hi, ...) itself: the same stage list,
 * launches and bits.  GPK_EINVAL, before any device work, on a non-finite q, and on everything the
 * older create calls reject. */
int gpk_create3_opq(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf,
                    const gpk_bdata3* bd, const gpk_conv3* cv, const gpk_cross3* mx, const gpk_drift3* dr,
                    const gpk_high3* hi, const gpk_bicross3* bq, double freq_scale, gpk_handle3** out);
/* The bi-pair weights; zeros on every older kind of 3-axis handle. */
int gpk_bicross_info3(const gpk_handle3* h, double q[3]);

/* Quadratic gradient terms (eikonal and viscous eikonal |grad u|^2 - eps lap u = f, Hamilton-Jacobi
 * u_t + |grad u|^2 / 2 - nu lap u = f, KPZ, the anisotropic and level-set forms grad u^T S grad u with
 * off-diagonal S, Kuramoto-Sivashinsky in its integral form).  The handle adds
 *     sum_k s_k (d u / d x_k)^2 + sum_{j<k} x_jk (d u / d x_j) (d u / d x_k)
 * to the equation of a gpk_create3_opq handle; x holds the weights of the pairs (1,2), (1,3), (2,3) in
 * that order.  Axis k is gradient-active when g_k != 0 (gpk_conv3), s_k != 0 or a pair with k in it
 * has x_jk != 0.  With A_k = K_k^{-1} x_k U and D1_k the plain order-1 block of axis k, on a handle
 * with any non-zero weight here:
 *     P_k   = D1_k x_k A_k                                   (once per gradient-active axis)
 *     N     = g_1 P_1 + g_3 P_3 + g_2 P_2
 *     Gamma = s_1 P_1^2 + s_3 P_3^2 + s_2 P_2^2 + x_13 P_1 P_3 + x_12 P_1 P_2 + x_23 P_2 P_3
 *     R     = [the opq handle's R, u . N included] + Gamma   (Gamma last)
 *     Q_k   = (g_k U + 2 s_k P_k + sum_{j != k} x_jk P_j) . R
 *     T_k  += D1_k^T x_k Q_k,    G_D1k = v Q_k,(k) A_k,(k)^T,    dL/dU += v N . R
 * ( . elementwise, every sum in that fixed order, present terms only).  THE WEIGHTS ARE CONSTANTS:
 * the gpk_coef3 fields a_k multiply the linear terms of their own axis only, never this term, and
 * the drift fields b_k stand alone as before.  A gradient-active axis is entered like a mixed-order
 * one and may have c4 = c3 = c2 = c1 = g = 0 (inviscid eikonal).  The drift outputs E_k = b_k R and
 * the W_k are formed on the final R; eq_gap, the log joint, the boundary and derivative-boundary
 * terms, gpk_criterion3, gpk_loss_terms3, gpk_boundary_terms3 and the Adam kernels keep their formulas
 * on the new R; predictions depend on K_k only.  No solve is added.  gpk_stage_variants3 reports
 * exactly the entries of a convective handle with the same other terms.
 * Not built: fields on s and x; terms cubic in grad u; products with second derivatives; the
 * conservative form; the sharded, 1-axis and 2-axis handles; the class path. */
typedef struct gpk_gradsq3 {
  double s[3]; /* s_k (du/dx_k)^2 */
  double x[3]; /* pairs (1,2), (1,3), (2,3): x_jk du/dx_j du/dx_k */
} gpk_gradsq3;
/* p, op, cf, bd, cv, mx, dr, hi and bq as on gpk_create3_opq (all but p and op may be NULL).  gq ==
 * NULL or all six weights 0.0 is gpk_create3_opq(p, op, cf, bd, cv, mx, dr, hi, bq, ...) itself: the
 * same stage list, launches and bits.  GPK_EINVAL, before any device work, on a non-finite weight,
 * and on everything the older create calls reject. */
int gpk_create3_opg(const gpk_problem3* p, const gpk_operator3x* op, const gpk_coef3* cf,
                    const gpk_bdata3* bd, const gpk_conv3* cv, const gpk_cross3* mx, const gpk_drift3* dr,
                    const gpk_high3* hi, const gpk_bicross3* bq, const gpk_gradsq3* gq, double freq_scale,
                    gpk_handle3** out);
/* The quadratic gradient weights; zeros on every older kind of 3-axis handle. */
int gpk_gradsq_info3(const gpk_handle3* h, double s[3], double x[3]);

int gpk_num_params3(const gpk_handle3* h, int64_t* n);
int gpk_set_params3(gpk_handle3* h, const double* flat, int64_t n);
int gpk_get_params3(gpk_handle3* h, double* flat, int64_t n);
/* loss and full gradient at the current params (no update) */
int gpk_loss_grad3(gpk_handle3* h, double* loss, double* grad_flat);
/* n_steps of loss + gradient + Adam, device-resident; losses[n_steps] nullable */
int gpk_step3(gpk_handle3* h, int32_t n_steps, double* losses);
/* Adam state of a 3-axis handle: the step count and the first / second moments, each in the
 * flat params' layout (n = gpk_num_params3). */
int gpk_set_opt_state3(gpk_handle3* h, int64_t count, const double* mu, const double* nu, int64_t n);
int gpk_get_opt_state3(gpk_handle3* h, int64_t* count, double* mu, double* nu, int64_t n);
/* Predictions on the test grid xte1 x xte2 x xte3 at the current params: out[m1*m2*m3] row-major.
 * The reference's 2-axis association (model_GP_solver_2d.py:185-220) axis after axis,
 * T <- Kmn_k x_k solve(K_k, T) for k = 1, 2, 3 from T = U, each solve through K_k^{-1} with one
 * refinement step.  1 <= m_k <= 1024.  Scratch is allocated for the call and freed before it
 * returns (GPK_ENOMEM when it does not fit); GPK_ENOTPD on a non-positive pivot.  Params and Adam
 * state are untouched. */
int gpk_predict3(gpk_handle3* h, const double* xte1, int32_t m1, const double* xte2, int32_t m2,
                 const double* xte3, int32_t m3, double* out);
/* gpk_predict3 with the d[k]-th derivative (0, 1 or 2) along axis k, taken in the test point as
 * in gpk_predict_deriv: Kmn_k is the D block of gpk_kernel_matrices(deriv = d[k], xte_k, x_k).
 * d = {0, 0, 0} is gpk_predict3, bit for bit; sizes, status codes and side effects are its own. */
int gpk_predict_deriv3(gpk_handle3* h, const double* xte1, int32_t m1, const double* xte2, int32_t m2,
                       const double* xte3, int32_t m3, const int32_t d[3], double* out);
/* The same quantity at m >= 1 scattered points, pts [m][3] row-major, out [m]: gpk_predict3's
 * association per point, with the axis-2 and axis-3 products contracted against kernel fields
 * evaluated on the fly (no m x m x m grid, and no limit of 1024 on m).  The points are walked in
 * chunks of at most 1024 (fewer on grids whose chunk x P2 x P3 intermediate would pass 2 GiB); the
 * solve K1^{-1} x_1 U is done once per call.  A point's result does not depend on the chunks
 * before it.  Scratch, status codes and side effects as gpk_predict3. */
int gpk_evaluate3(gpk_handle3* h, const double* pts, int64_t m, const int32_t d[3], double* out);
/* compute_early_stopping (model_GP_solver_2d.py:222-233) on three axes: boundary_gap / Nb +
 * eq_gap / Nc at the current params, Nb = 2 (n2 n3 + n1 n3 + n1 n2), Nc = n1 n2 n3 (operator handles: boundary_gap
 * and Nb over the active faces). */
int gpk_criterion3(gpk_handle3* h, double* out);
/* The GEMM kernel each of the step's GEMM launches takes, in stream order (gpk_dgemm's variant
 * numbers: 1 the 16x16, 2 the 64x64, 3 the 128x128 kernel): *n launches, the first
 * min(*n, cap) of them in out.  Fixed by the grid; nothing is launched. */
int gpk_stage_variants3(gpk_handle3* h, int32_t* out, int32_t cap, int32_t* n);
/* The terms of the last gpk_loss_grad3's loss: out = {loss, log det K1, log det K2, log det K3,
 * <U, K^{-1} U>, eq_gap, boundary_gap} (read back; nothing is launched). */
int gpk_loss_terms3(gpk_handle3* h, double out[7]);
/* Refinement gates of a GPK_FLAG3_REFINE handle as the last graph run (gpk_loss_grad3 / gpk_step3)
 * left them: bound[k] = K_00 max diag K_k^{-1} of axis k (a lower bound of cond K_k), open[k] = 1
 * when that run refined axis k's solves (bound > 100), *route the refinement's kernels (0: two
 * gated GEMMs per solve, 1: the fused panel kernel).  Read back; nothing is launched.  GPK_EINVAL on a handle created
 * without the flag.  The step's GEMM launches proper stay the six of gpk_stage_variants3. */
int gpk_refine_info3(gpk_handle3* h, double bound[3], int32_t open[3], int32_t* route);

/* One mode-k product on host operands (tests, A/B timing; the counterpart of gpk_dgemm):
 *   C = alpha (Mat x_k T) + beta C0,   T [d1][d2][d3] row-major, Mat m x d_k row-major,
 * C and C0 shaped as T with d_k replaced by m; every size a multiple of 32; C0 may be NULL or
 * equal C.  Modes 1 and 3 are single GEMMs on the row-major unfoldings under every variant.
 * Mode 2: variant 0 the slab-batched kernel (one launch over the d1 slabs of d2 x d3, no copy;
 * 2 / 3 the same with its 32x32 / 64x64 tile forced), variant 1 the step's route (permuted
 * copy, one GEMM, permuted back).  iters > 0 times that many back-to-back runs of the whole
 * route with HIP events after the checked one; *avg_us as gpk_dgemm. */
int gpk_mode_gemm(int32_t variant, int32_t k, int32_t d1, int32_t d2, int32_t d3, int32_t m, double alpha,
                  const double* Mat, const double* T, double beta, const double* C0, double* C,
                  int32_t iters, double* avg_us);

/* One refinement step X <- X + Kinv (B - Kc X) on host operands, no gate (tests, A/B timing; the
 * counterpart of gpk_mode_gemm).  side 0: X and B are P x M row-major and the matrices act on
 * rows; side 1: X and B are M x P and the step is X + (B - X Kc) Kinv.  route 0: the step's two
 * GEMMs; route 1: the fused panel kernel (P <= 512, else GPK_EINVAL).  P, M multiples of 32,
 * P <= 1024; Kinv and Kc P x P, any values.  X is overwritten with the result.  iters as
 * gpk_mode_gemm (the timed launches keep refining the device copy of X). */
int gpk_refine_panel(int32_t route, int32_t side, int32_t P, int32_t M, const double* Kinv, const double* Kc,
                     const double* B, double* X, int32_t iters, double* avg_us);

/* The scattered-point contraction on host operands (tests, timing; the counterpart of
 * gpk_mode_gemm / gpk_refine_panel):
 *   out[p * C + c] = sum_{j < n} field(t[p], x[j]) * T[p * sp + j * sj + c * sc],  p < m, c < C,
 * field = kappa / D_x1_kappa / DD_x1_kappa for deriv 0 / 1 / 2 (first argument = the point), the
 * values of gpk_kernel_matrices(kind, deriv, t, x, ...), evaluated on the fly.  sp = 0 broadcasts
 * one T to all points; sp >= 0, sj >= 1, sc >= 1, and T holds (m-1) sp + (n-1) sj + (C-1) sc + 1
 * doubles, of which only the addressed ones are used (padding may hold anything).  C = 1: one
 * wave per point; C > 1: the point's field values in LDS, n <= 4096 (else GPK_EINVAL).  The sum's
 * order depends on (n, C) only.  iters > 0 times that many back-to-back launches with HIP events
 * after the checked one; *avg_us as gpk_dgemm. */
int gpk_point_contract(int32_t kind, int32_t deriv, const double* t, int32_t m, const double* x, int32_t n,
                       const double* logw, const double* logls, const double* freq, int32_t q,
                       const double* T, int64_t sp, int64_t sj, int64_t sc, int32_t C,
                       double* out, int32_t iters, double* avg_us);

/* The step's per-pair assembly kernel on one axis of host operands (tests; the counterpart of
 * gpk_point_contract): K_out = kappa(x_i, x_j) + jitter on the diagonal and D_out, both n x n
 * row-major, as the 3-axis step assembles them before the inverse.  c1 == 0: D_out = DD_x1_kappa
 * (mode 2); c2 == 0 (and c1 != 0): D_out = D_x1_kappa (mode 1) -- both unweighted, as in the step,
 * where the weight rides on the GEMMs; otherwise the mixed block c2 DD_x1_kappa + c1 D_x1_kappa.
 * 1 <= n <= 1024, 1 <= q <= 64, c2 and c1 finite. */
int gpk_assemble_pairs(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                       const double* freq, int32_t q, double jitter, double c2, double c1,
                       double* K_out, double* D_out);
/* The same launch timed (A/B; no outputs): *avg_us is the mean over iters >= 1 back-to-back
 * launches between two HIP events, after a checked and a warm-up one.  split != 0 runs mode 2 and
 * mode 1 as two launches per iteration, each into a block of its own -- what forming the two
 * fields of a mixed axis separately would cost -- whatever c2 and c1 are. */
int gpk_assemble_pairs_time(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                            const double* freq, int32_t q, double c2, double c1, int32_t split,
                            int32_t iters, double* avg_us);

/* The two-block mode of gpk_assemble_pairs' kernel, which a convective axis (gpk_create3_opc) assembles in:
 * K_out, D_out = c2 DD_x1_kappa + c1 D_x1_kappa at any c2 and c1 (zeros included) and D1_out =
 * D_x1_kappa alone, each n x n row-major. */
int gpk_assemble_pairs2(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                        const double* freq, int32_t q, double jitter, double c2, double c1,
                        double* K_out, double* D_out, double* D1_out);

/* The high-order modes of the same kernel, which an axis with c4_k or c3_k non-zero (gpk_create3_oph)
 * assembles in: K_out and D_out = c4 D4 + c3 D3 + c2 DD_x1_kappa + c1 D_x1_kappa at any weights
 * (zeros included; D4, D3 the fourth and the signed third derivative in the first argument), each
 * n x n row-major.  D1_out == NULL: the plain mode; otherwise the two-block mode, which also stores
 * D1_out = D_x1_kappa alone.  At c4 = c3 = 0 the blocks are gpk_assemble_pairs2's, bit for bit.
 * 1 <= n <= 1024, 1 <= q <= 64, weights and jitter finite. */
int gpk_assemble_pairs4(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                        const double* freq, int32_t q, double jitter, double c4, double c3, double c2,
                        double c1, double* K_out, double* D_out, double* D1_out);

/* The modes an axis of a bi-pair (gpk_create3_opq) assembles in: gpk_assemble_pairs4's K_out, D_out and
 * D1_out, bit for bit, and D2_out = DD_x1_kappa alone (required), the block gpk_assemble_pairs4 gives
 * as D_out at (c4, c3, c2, c1) = (0, 0, 1, 0), n x n row-major and symmetric to the bit.  D1_out == NULL:
 * the mode without D1. */
int gpk_assemble_pairs5(int32_t kind, const double* x, int32_t n, const double* logw, const double* logls,
                        const double* freq, int32_t q, double jitter, double c4, double c3, double c2,
                        double c1, double* K_out, double* D_out, double* D1_out, double* D2_out);

#ifdef __cplusplus
}
#endif
#endif /* GPK_H_ */
