// gpk_create.cpp — building and destroying a handle: problem validation, the inverse-path
// policy, buffer allocation, distance classes, the problem upload; parameter and optimizer-state
// get / set.  create_impl runs these as named phases, in this order.
#include <atomic>

#include "gpk_host.h"

static std::atomic<int> g_chain_cap{0};  // gpk_set_chain_capacity override (0: query the device)

// Distance classes of one axis (gpk_internal.h ClassArgs): per diagonal k the distinct exact
// values of d = |x_{j+k} - x_j| (= |x_j - x_{j+k}| bitwise), in order of first appearance.
// false: some diagonal has more than CLS_VMAX of them (the step keeps the per-pair kernels).
bool build_classes(const double* x, int n, int P, std::vector<double>& dist, std::vector<int>& cid,
                   std::vector<int>& cbase, int& vmax) {
  cid.assign((size_t)P * P, -1);
  cbase.assign((size_t)n + 1, 0);
  dist.clear();
  vmax = 0;
  double vals[CLS_VMAX];
  for (int k = 0; k < n; ++k) {
    int nv = 0;
    cbase[k] = (int)dist.size();
    for (int j = 0; j + k < n; ++j) {
      const double d = std::fabs(x[j + k] - x[j]);
      int v = 0;
      while (v < nv && !(vals[v] == d)) ++v;
      if (v == nv) {
        if (nv == CLS_VMAX) return false;
        vals[nv++] = d;
        dist.push_back(d);
      }
      const int c = cbase[k] + v;
      cid[(size_t)(j + k) * P + j] = c;
      cid[(size_t)j * P + j + k] = c;
    }
    vmax = std::max(vmax, nv);
  }
  cbase[n] = (int)dist.size();
  return true;
}

// padm: padding multiple of the matrix dimensions (32; 32 * nranks for a row-sharded handle so
// that every rank's row block is a whole number of 32-row tiles)
static Layout make_layout(const gpk_problem* p, int padm = PADM) {
  auto pad_up = [padm](int n) { return (n + padm - 1) / padm * padm; };
  Layout L{};
  L.dim = p->dim;
  L.q = p->q;
  L.n1 = p->n1;
  L.p1 = pad_up(p->n1);
  if (p->dim == 2) {
    L.naxes = 2;
    L.n2 = p->n2;
    L.p2 = pad_up(p->n2);
    const int nu = p->n1 * p->n2;
    L.off_u = 0;
    L.off_kp[0] = nu;
    L.off_kp[1] = nu + 3 * p->q;
    L.off_tau = nu + 6 * p->q;
    L.off_v = L.off_tau + 1;
    L.off_small = nu;
    L.nsmall = 6 * p->q + 2;
    L.nparams = (int64_t)nu + 6 * p->q + 2;
  } else {
    L.naxes = 1;
    L.n2 = 1;
    L.p2 = 1;
    L.off_kp[0] = 0;
    L.off_kp[1] = 0;
    L.off_tau = 3 * p->q;
    L.off_v = 3 * p->q + 1;
    L.off_u = 3 * p->q + 2;
    L.off_small = 0;
    L.nsmall = 3 * p->q + 2;
    L.nparams = (int64_t)p->n1 + 3 * p->q + 2;
  }
  return L;
}

static std::vector<double> init_params(const gpk_problem* p, const Layout& L, double freq_scale) {
  // train(): log_tau = log_v = 0; log-w = log(1/Q); log-ls = 0; freq = linspace(0,1,Q)*fs; U = 0
  std::vector<double> h((size_t)L.nparams, 0.0);
  const int q = p->q;
  for (int a = 0; a < L.naxes; ++a) {
    const int off = L.off_kp[a];
    for (int c = 0; c < q; ++c) {
      const double lin = (q == 1) ? 0.0 : (double)c / (double)(q - 1);  // np.linspace(0,1,Q)
      h[off + c] = lin * freq_scale;
      h[off + q + c] = 0.0;
      h[off + 2 * q + c] = std::log(1.0 / q);
    }
  }
  return h;
}

// phase 1: the problem as given
static int validate_problem(const gpk_problem* p) {
  if (p->dim != 1 && p->dim != 2) return fail(GPK_EINVAL, "dim must be 1 or 2");
  if (p->kind < 0 || p->kind > 3) return fail(GPK_EINVAL, "Invalid Kernel");
  if (p->eq < 0 || p->eq > 2 || (p->eq == GPK_ADVECTION && p->dim != 2))
    return fail(GPK_EINVAL, "equation type not supported for this dimension");
  if (p->q <= 0 || p->q > QMAX) return fail(GPK_EINVAL, "Q must be in [1, 64]");
  if (p->n1 < 2 || (p->dim == 2 && p->n2 < 2)) return fail(GPK_EINVAL, "need >= 2 collocation points per axis");
  if (!p->x1 || !p->src || !p->bvals || (p->dim == 2 && !p->x2) || (p->dim == 1 && (!p->bidx || p->nb <= 0)))
    return fail(GPK_EINVAL, "NULL problem array");
  if (p->dim == 1)
    for (int k = 0; k < p->nb; ++k)
      if (p->bidx[k] < 0 || p->bidx[k] >= p->n1) return fail(GPK_EINVAL, "Xind out of range");
  return GPK_OK;
}

// phase 2: the SPD inverse the step uses (gpk_inverse_path reports it)
static void choose_inverse_path(gpk_handle* h, const gpk_problem* p, bool local_group) {
  const Layout& L = h->L;
  const bool shard = h->shard;
  const int rank = h->rank, nranks = h->nranks;
  const int pmax = std::max(L.p1, L.dim == 2 ? L.p2 : 0);
  h->bigspd = (p->flags & GPK_FLAG_FORCE_BIG_SPD) != 0 ||
              (!(p->flags & GPK_FLAG_FORCE_SMALL_SPD) && pmax >= SPD_BIG_MIN);
  h->bigwide = h->bigspd && !(p->flags & GPK_FLAG_FORCE_NARROW_SPD) &&
               ((p->flags & GPK_FLAG_FORCE_WIDE_SPD) || pmax >= SPD_WIDE_MIN);
  // The persistent chain inverse needs its whole grid co-resident: the grid (workgroups of
  // every factor's row, the widest row times the factors) must fit the device's capacity for
  // the chain variant the step launches (occupancy per CU x CUs, so a CU-partitioned device
  // falls back to the per-sweep launches), and handles of an in-process rank group -- which
  // launch concurrently on one device from several host threads -- never use it.
  const int pp[2] = {L.p1, L.p2};
  const int deriv = p->eq == GPK_ADVECTION ? 1 : 2;
  int cap = g_chain_cap.load();
  if (cap <= 0) {
    DevSwitch dsw(p->device);
    const bool gather = !(p->flags & GPK_FLAG_NO_DCLASS);  // (gather mode needs classes; the
    cap = std::min(spd_chain_capacity(deriv, gather),       //  per-pair mode's footprint is
                   spd_chain_capacity(deriv, false));        //  bounded by the same check)
  }
  cap = std::min(cap, CHAIN_MAX_BLOCKS);
  auto grid_blocks = [&](bool aug) {  // launch_spd_chain's grid: (max_a T_a TC_a + 1) x factors
    const int cols = (L.p1 + (L.naxes == 2 ? L.p2 : 0)) / 32;
    int wide = 0;
    for (int a = 0; a < L.naxes; ++a) wide = std::max(wide, (pp[a] / 32) * (pp[a] / 32 + (aug ? cols : 0)) + 1);
    return wide * L.naxes;
  };
  const bool in_group = shard && local_group && nranks > 1;
  if (shard && nranks >= 2 && (p->flags & GPK_FLAG_SPLIT_FACTORS)) h->split_axis = rank < nranks / 2 ? 0 : 1;
  // (the chain inverts every factor in one launch: a split rank inverts one, per sweep)
  // (an in-process group's ranks launch their chains concurrently on the one device: all of
  // them must be co-resident together -- the 2-rank group is how the tests exercise the exact
  // chain + row-sharded step an RCCL rank runs)
  const int chains_on_device = in_group ? nranks : 1;
  h->chain = !h->bigspd && h->split_axis < 0 && !(p->flags & GPK_FLAG_NO_CHAIN) &&
             grid_blocks(false) * chains_on_device <= cap;
  // (row-sharded handles too: the augmented chain gives every rank the whole A, Bt and
  // K^{-1} D^T from its replicated inverse, so the forward solves need no all-gather -- the
  // sharded step's plan, build_shard)
  h->chain_aug = h->chain && L.dim == 2 && !(p->flags & GPK_FLAG_NO_CHAIN_AUG) &&
                 grid_blocks(true) * chains_on_device <= cap;
  // large 1D factors: the persistent inverse on 64-row macro tiles (chain_multi_kernel), when
  // its grid is co-resident (else the 64/128-wide launch-per-sweep path)
  if (L.dim == 1 && !in_group && h->split_axis < 0 &&
      !(p->flags & (GPK_FLAG_NO_CHAIN | GPK_FLAG_FORCE_BIG_SPD | GPK_FLAG_FORCE_SMALL_SPD)) &&
      (pmax >= SPD_BIG_MIN || (p->flags & GPK_FLAG_FORCE_CHAIN_MULTI))) {
    int mcap = g_chain_cap.load();
    if (mcap <= 0) {
      DevSwitch dsw(p->device);
      const bool gather = !(p->flags & GPK_FLAG_NO_DCLASS);
      mcap = std::min(spd_chain_multi_capacity(deriv, gather), spd_chain_multi_capacity(deriv, false));
    }
    if (spd_chain_multi_blocks(pp, L.naxes) <= mcap) {
      h->chain_multi = h->chain = true;
      h->chain_aug = h->bigspd = h->bigwide = false;
    }
  }
}

#define A_(ptr, n) TRY(dev_alloc(h->allocs, h->s, &(ptr), (n)))  // zero-filled, freed by gpk_destroy

// phase 3: problem, parameter, factor and work buffers
static int allocate_buffers(gpk_handle* h, const gpk_problem* p) {
  const Layout& L = h->L;
  const bool shard = h->shard;
  const int P1 = L.p1, P2 = L.p2;
  const size_t nup = (size_t)P1 * P2;
  A_(h->x1, P1);
  A_(h->x2, std::max(P2, 1));
  A_(h->F, nup);
  A_(h->bvals, h->prob.nb);
  A_(h->bidx, std::max(p->nb, 1));
  A_(h->params, L.nparams);
  A_(h->grad, L.nparams);
  A_(h->m, L.nparams);
  A_(h->v, L.nparams);
  A_(h->Up, nup);
  A_(h->kc, 2);
  A_(h->sc, 1);
  A_(h->count, 1);
  A_(h->loss_slot, 1);
  A_(h->status, 1);
  A_(h->stat_x, 2);
  A_(h->losses, LOSS_CAP);
  A_(h->diag, 8);
  for (int a = 0; a < L.naxes; ++a) {
    const int P = axis_p(L, a);
    A_(h->K[a], (size_t)P * P);
    A_(h->Kb[a], (size_t)P * P);
    A_(h->D[a], (size_t)P * P);
    A_(h->piv[a], spd_big_piv_doubles(P));  // large path: W x W L^{-1} + 128-pivot scratch
    A_(h->ldet[a], P / 32);
    A_(h->Kc[a], (size_t)P * P);
    A_(h->pst[a], 2);
    A_(h->aflag[a], 4 + P / 32);  // + the 128-wide update's per-sweep panel tickets
    if (h->bigspd) A_(h->Zp[a], (size_t)3 * 128 * P);
    if (h->bigspd && h->bigwide) {  // (fill_spd: SpdArgs::sched_paired names the same table)
      const int T2 = (int)((P + 127) / 128);
      std::vector<unsigned> tab;
      wide_schedule(T2, !(p->flags & GPK_FLAG_ONE_SWEEP_UPDATE), tab);
      A_(h->wsched[a], tab.size());
      if (hipMemcpyAsync(h->wsched[a], tab.data(), tab.size() * sizeof(unsigned), hipMemcpyHostToDevice, h->s) != hipSuccess ||
          hipStreamSynchronize(h->s) != hipSuccess)
        return fail(GPK_EHIP, "upload the update schedule");
    }
    A_(h->cflags[a], (size_t)(P / 32) * (P / 32 + (P1 + P2) / 32) + 2 * (P / 32) + 1);
    A_(h->cgran[a], (size_t)(P / 32) * 3072);  // [T][3][1024]
    // every hand-off slot starts unwritten (spdinv.hip chain_master / chain_multi_kernel)
    if (hipMemsetD32Async(h->cgran[a], CHAIN_SENTINEL32, (size_t)(P / 32) * 6144, h->s) != hipSuccess)
      return fail(GPK_EHIP, "initialise the pivot-chain input slots");
    if (h->chain) {  // chain_multi: panel + L^{-1} slots; chain_kernel: the L^{-1} slots
      A_(h->PB2[a], 2 * chain_half(P, h->chain_multi));
      A_(h->cepoch[a], CHAIN_EPOCH_WORDS);  // launch counter, arrival count (each its own line)
      if (hipMemsetD32Async(h->PB2[a], CHAIN_SENTINEL32, 4 * chain_half(P, h->chain_multi), h->s) != hipSuccess)
        return fail(GPK_EHIP, "initialise the panel slots");
    }
    if (h->chain_aug) {
      A_(h->PD[a], (size_t)P * P);
      A_(h->PBa[a], (size_t)P * (P1 + P2));
    }
    h->nldet[a] = P / 32;
  }
  if (L.dim == 2) {
    A_(h->A, nup); A_(h->Bt, nup); A_(h->S, nup); A_(h->R, nup);
    A_(h->T1, nup); A_(h->T2, nup); A_(h->X1, nup); A_(h->X2, nup);
    A_(h->W1, nup); A_(h->W2, nup); A_(h->Y1, nup); A_(h->Y2, nup);
    for (int a = 0; a < 2; ++a) {
      const int P = axis_p(L, a);
      A_(h->GK[a], (size_t)P * P);
      A_(h->GD[a], (size_t)P * P);
    }
    h->nquad = h->negap = (P1 / 16) * (P2 / 16);  // upper bound (16x16 tiles); set in build_descs
  } else {
    A_(h->alpha, P1); A_(h->R, P1); A_(h->tvec, P1); A_(h->beta, P1); A_(h->rvec, P1);
    if (p->uoff) A_(h->uoff, P1);
    h->nquad = h->negap = gemv_blocks(P1);
  }
  if (shard) {  // one all-reduce per sharded step: [status | pg | egap | quad] (enqueue_step_shard)
    const size_t npg = (size_t)L.naxes * 3 * QMAX;
    A_(h->sred, 2 + npg + (size_t)h->negap + (size_t)h->nquad);
    h->stat_x = h->sred;
    h->pg = h->sred + 2;
    h->red_egap = h->pg + npg;
    h->red_quad = h->red_egap + h->negap;
  } else {
    A_(h->red_quad, h->nquad);
    A_(h->red_egap, h->negap);
  }
  return GPK_OK;
}

// phase 4: distance classes and the buffers sized by them
static int build_upload_classes(gpk_handle* h, const gpk_problem* p) {
  const Layout& L = h->L;
  const bool shard = h->shard;
  const int P1 = L.p1, P2 = L.p2;
  // distance classes (both axes or none), uploaded once: the coordinates never change
  std::vector<double> cdist[2];
  std::vector<int> ccid[2], cbase[2];
  bool use_cls = !(p->flags & GPK_FLAG_NO_DCLASS);
  int vmax[2] = {0, 0};
  for (int a = 0; a < L.naxes && use_cls; ++a)
    use_cls = build_classes(a ? p->x2 : p->x1, axis_n(L, a), axis_p(L, a),
                            cdist[a], ccid[a], cbase[a], vmax[a]);
  if (use_cls) {
    for (int a = 0; a < L.naxes; ++a) {
      const int P = axis_p(L, a), U = (int)cdist[a].size();
      ClassArgs& c = h->cls[a];
      double *dist = nullptr, *kval = nullptr, *dval = nullptr, *part = nullptr;
      int *cid = nullptr, *cb = nullptr;
      // class-sum row chunks: <= 64 chunks of >= 16 rows (one 4-row group per wave and pass);
      // with the LDS bins (> 8 variants per diagonal: 70 KB per workgroup, two per CU) <= 32
      // chunks -- C2: 0.693 -> 0.688 ms/step (64 rows; 128 the same, 256 slower)
      const int n = axis_n(L, a);
      const int maxchunks = vmax[a] > 8 ? 32 : 64;
      const int rb = std::max(16, (n + maxchunks - 1) / maxchunks + 15) / 16 * 16;
      const int nchunk = (n + rb - 1) / rb;
      A_(dist, U); A_(kval, U); A_(dval, U); A_(part, (size_t)2 * nchunk * U);
      A_(cid, (size_t)P * P); A_(cb, cbase[a].size());
      if (hipMemcpyAsync(dist, cdist[a].data(), U * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess ||
          hipMemcpyAsync(cid, ccid[a].data(), ccid[a].size() * sizeof(int), hipMemcpyHostToDevice, h->s) != hipSuccess ||
          hipMemcpyAsync(cb, cbase[a].data(), cbase[a].size() * sizeof(int), hipMemcpyHostToDevice, h->s) != hipSuccess)
        return fail(GPK_EHIP, "upload distance classes");
      c.ncls = U; c.vmax = vmax[a]; c.dist = dist; c.cid = cid; c.cbase = cb;
      c.kval = kval; c.dval = dval; c.nchunk = nchunk; c.rb = rb; c.part = part;
      // the large-factor gather's variant bytes (ClassArgs::vidx), for EVERY axis once the
      // largest one takes gather_wide_kernel (assemble.hip: (P/32)^2 >= GW_WIDE_MIN_TILES, i.e.
      // max P >= 1024) -- that launch assembles all axes at once
      if (std::max(P1, L.naxes == 2 ? P2 : 0) >= 1024) {
        std::vector<unsigned char> vb((size_t)P * P, 0xff);
        for (int i = 0; i < n; ++i)
          for (int j = 0; j < n; ++j) {
            const int u = ccid[a][(size_t)i * P + j];
            if (u >= 0) vb[(size_t)i * P + j] = (unsigned char)(u - cbase[a][std::abs(i - j)]);
          }
        unsigned char* dv = nullptr;
        if (hipMalloc(&dv, vb.size()) != hipSuccess) return fail(GPK_ENOMEM, "hipMalloc (class variants)");
        h->allocs.push_back(dv);
        if (hipMemcpyAsync(dv, vb.data(), vb.size(), hipMemcpyHostToDevice, h->s) != hipSuccess ||
            hipStreamSynchronize(h->s) != hipSuccess)
          return fail(GPK_EHIP, "upload class variants");
        c.vidx = dv;
      }
    }
    h->bpa = std::max(pgrad_class_blocks(h->cls[0].ncls), L.dim == 2 ? pgrad_class_blocks(h->cls[1].ncls) : 0);
    // 2D, <= CB_VMAX variants per diagonal, unsharded: the G_K / G_D GEMMs sum their tiles per
    // class (build_descs turns it on when both stages take the 16x16-tile kernel)
    if (L.dim == 2 && !shard && !(p->flags & GPK_FLAG_NO_CLASS_BINS) && vmax[0] <= CB_VMAX &&
        vmax[1] <= CB_VMAX) {
      for (int a = 0; a < 2; ++a) {
        const size_t ns = (size_t)h->cls[a].ncls * class_slots(axis_p(L, a) / 16);
        A_(h->cpK[a], ns);
        A_(h->cpD[a], ns);
      }
    }
    h->cls_gemv = h->chain_multi && L.dim == 1 && !(p->flags & GPK_FLAG_MATRIX_GEMV);
  } else {
    h->bpa = std::max(pgrad_blocks(L.n1), L.dim == 2 ? pgrad_blocks(L.n2) : 0);
  }
  return GPK_OK;
}

// ... then the contraction partials, the step tail, the snapshot and the pinned report
static int allocate_step_tail(gpk_handle* h, const gpk_problem* p) {
  const Layout& L = h->L;
  const bool shard = h->shard;
  const int P1 = L.p1, P2 = L.p2;
  A_(h->pgpart, (size_t)L.naxes * h->bpa * 3 * QMAX);
  if (!shard) A_(h->pg, (size_t)L.naxes * 3 * QMAX);
  h->ttg = std::max(16, (int)std::ceil(std::sqrt((double)h->bpa)));  // one 16-load batch per level at C4
  h->tngpa = (h->bpa + h->ttg - 1) / h->ttg;
  A_(h->tcount, (size_t)L.naxes * h->tngpa);
  A_(h->ttop, 1);
  A_(h->tgpart, (size_t)L.naxes * h->tngpa * 3 * QMAX);
  // The kernel-parameter contraction in double-double on the large 2D factors (C5): there the
  // sum over classes cancels ~1e8-fold and the fp64 rounding of the derivative fields sets its
  // accuracy; at C4 it would cost the latency-bound step ~1 us and buys nothing
  h->pg_dd = h->cls[0].ncls > 0 && !shard && !(p->flags & GPK_FLAG_NO_DD_CONTRACTION) &&
             ((L.dim == 2 && std::max(P1, P2) >= SPD_WIDE_MIN) || (p->flags & GPK_FLAG_DD_CONTRACTION));
  if (h->pg_dd) {
    A_(h->pgpart_lo, (size_t)L.naxes * h->bpa * 3 * QMAX);
    A_(h->tgpart_lo, (size_t)L.naxes * h->tngpa * 3 * QMAX);
  }
  // boundary-gap parts (PrepArgs::bgap): one per BGAP_CHUNK entries of a 2D boundary
  h->bgap_parts = L.dim == 2 ? std::min(BGAP_PARTS_MAX, std::max(1, (2 * L.n1 + 2 * L.n2 + BGAP_CHUNK - 1) / BGAP_CHUNK)) : 1;
  A_(h->bgap, BGAP_PARTS_MAX);
  A_(h->snap, (size_t)3 * L.nparams);
  A_(h->snap_count, 1);
  A_(h->viol, 1);
  A_(h->nce_flag, 1);
  A_(h->nce_kp, (size_t)L.nsmall);
  if (hipHostMalloc(reinterpret_cast<void**>(&h->rep_host), (8 + LOSS_CAP) * sizeof(double),
                    hipHostMallocCoherent) != hipSuccess)
    return fail(GPK_ENOMEM, "hipHostMalloc (step report)");
  std::memset(h->rep_host, 0, (8 + LOSS_CAP) * sizeof(double));
  return GPK_OK;
}

#undef A_
// phase 5: upload the problem and the initial parameters
static int upload_problem(gpk_handle* h, const gpk_problem* p, double freq_scale) {
  const Layout& L = h->L;
  const int P2 = L.p2;
  if (hipMemcpyAsync(h->x1, p->x1, L.n1 * sizeof(double), hipMemcpyHostToDevice, h->s) != hipSuccess)
    return fail(GPK_EHIP, "upload x1");
  if (L.dim == 2) {
    (void)hipMemcpyAsync(h->x2, p->x2, L.n2 * sizeof(double), hipMemcpyHostToDevice, h->s);
    for (int i = 0; i < L.n1; ++i)
      (void)hipMemcpyAsync(h->F + (size_t)i * P2, p->src + (size_t)i * L.n2, L.n2 * sizeof(double),
                           hipMemcpyHostToDevice, h->s);
  } else {
    (void)hipMemcpyAsync(h->F, p->src, L.n1 * sizeof(double), hipMemcpyHostToDevice, h->s);
    (void)hipMemcpyAsync(h->bidx, p->bidx, p->nb * sizeof(int), hipMemcpyHostToDevice, h->s);
    if (p->uoff)
      (void)hipMemcpyAsync(h->uoff, p->uoff, L.n1 * sizeof(double), hipMemcpyHostToDevice, h->s);
  }
  (void)hipMemcpyAsync(h->bvals, p->bvals, h->prob.nb * sizeof(double), hipMemcpyHostToDevice, h->s);
  std::vector<double> init = init_params(p, L, freq_scale);
  (void)hipMemcpyAsync(h->params, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice, h->s);
  if (hipStreamSynchronize(h->s) != hipSuccess) return fail(GPK_EHIP, "upload failed");
  return GPK_OK;
}

int create_impl(const gpk_problem* p, double freq_scale, int rank, int nranks, bool shard,
                gpk_handle** out, bool local_group) {
  if (!p || !out) return fail(GPK_EINVAL, "NULL argument");
  *out = nullptr;
  TRY(validate_problem(p));
  TRY(check_device(p->device));
  DevSwitch ds(p->device);
  gpk_handle* h = new gpk_handle();
  h->prob = *p;
  h->prob.x1 = h->prob.x2 = h->prob.src = h->prob.bvals = nullptr;
  h->prob.bidx = nullptr;
  h->prob.uoff = nullptr;
  if (p->dim == 2) h->prob.nb = 2 * p->n1 + 2 * p->n2;
  h->freq_scale = freq_scale;
  h->dev = p->device;
  h->shard = shard;
  h->rank = rank;
  h->nranks = nranks;
  h->L = make_layout(p, shard ? PADM * nranks : PADM);
  h->hyper = AdamHyper{p->lr, p->b1, p->b2, p->eps};
  const Layout& L = h->L;
  choose_inverse_path(h, p, local_group);
  auto bail = [&](int rc) {
    gpk_destroy(h);
    return rc;
  };
  if (hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(GPK_EHIP, "hipStreamCreate failed"));
  int rc = GPK_OK;
  if ((rc = allocate_buffers(h, p)) != GPK_OK || (rc = build_upload_classes(h, p)) != GPK_OK ||
      (rc = allocate_step_tail(h, p)) != GPK_OK || (rc = upload_problem(h, p, freq_scale)) != GPK_OK)
    return bail(rc);
  for (int k = 0; k <= kMaxStages; ++k)
    if (hipEventCreate(&h->ev[k]) != hipSuccess) return bail(fail(GPK_EHIP, "hipEventCreate"));
  // Kinv buffer identity is static (parity of the sweep count): resolve it by a dry enqueue
  // of the inverse into a throwaway capture is unnecessary -- compute it directly.
  for (int a = 0; a < L.naxes; ++a) {
    const int T = axis_p(L, a) / 32;
    h->Kinv[a] = (h->bigspd || h->chain) ? h->K[a] : ((T & 1) ? h->Kb[a] : h->K[a]);
  }
  if (L.dim == 2 && (rc = build_descs(h)) != GPK_OK) return bail(rc);
  if (shard && (rc = build_shard(h)) != GPK_OK) return bail(rc);
  // (the 2D large-factor path has no refinement stages: its one graph is the fast one)
  h->fast_ok = !shard && !(h->bigspd && L.dim == 2) && !(p->flags & GPK_FLAG_NO_FAST_GRAPH);
  h->fast_mode = h->fast_ok && (p->flags & GPK_FLAG_FAST_FIRST);
  *out = h;
  return GPK_OK;
}

int gpk_create(const gpk_problem* p, double freq_scale, gpk_handle** out) {
  return create_impl(p, freq_scale, 0, 1, false, out);
}

int gpk_destroy(gpk_handle* h) {
  if (!h) return GPK_OK;
  DevSwitch ds(h->dev);
  if (h->s) (void)hipStreamSynchronize(h->s);
  for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second);
  for (int k = 0; k <= kMaxStages; ++k)
    if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
  if (h->rep_host) (void)hipHostFree(h->rep_host);
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->s) (void)hipStreamDestroy(h->s);
  delete h->comm;
  delete h;
  return GPK_OK;
}

int gpk_num_params(const gpk_handle* h, int64_t* n) {
  if (!h || !n) return fail(GPK_EINVAL, "NULL argument");
  *n = h->L.nparams;
  return GPK_OK;
}

int gpk_set_params(gpk_handle* h, const double* flat, int64_t n) {
  if (!h || !flat) return fail(GPK_EINVAL, "NULL argument");
  if (n != h->L.nparams) return fail(GPK_EINVAL, "parameter count mismatch");
  DevSwitch ds(h->dev);
  HIPCHK(hipMemcpyAsync(h->params, flat, n * sizeof(double), hipMemcpyHostToDevice, h->s));
  TRY(check_launch(launch_sync_u(h->params, h->L, h->Up, h->s), "sync_u"));
  HIPCHK(hipStreamSynchronize(h->s));
  // new parameters: the next batch runs the full graph until their gate value has been seen
  h->fast_mode = h->fast_ok && (h->prob.flags & GPK_FLAG_FAST_FIRST);
  return GPK_OK;
}

int gpk_get_params(gpk_handle* h, double* flat, int64_t n) {
  if (!h || !flat) return fail(GPK_EINVAL, "NULL argument");
  if (n != h->L.nparams) return fail(GPK_EINVAL, "parameter count mismatch");
  DevSwitch ds(h->dev);
  if (h->shard)  // U rows are gathered into Up each step; the flat params hold only this rank's
    TRY(check_launch(launch_params_from_up(h->Up, h->L, h->params, h->s), "params_from_up"));
  HIPCHK(hipMemcpyAsync(flat, h->params, n * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  return GPK_OK;
}

int gpk_set_opt_state(gpk_handle* h, int64_t count, const double* mu, const double* nu, int64_t n) {
  if (!h || !mu || !nu) return fail(GPK_EINVAL, "NULL argument");
  if (n != h->L.nparams) return fail(GPK_EINVAL, "parameter count mismatch");
  if (count < 0 || count > 0x7fffffff) return fail(GPK_EINVAL, "bad count");
  DevSwitch ds(h->dev);
  int c = (int)count;
  HIPCHK(hipMemcpyAsync(h->m, mu, n * sizeof(double), hipMemcpyHostToDevice, h->s));
  HIPCHK(hipMemcpyAsync(h->v, nu, n * sizeof(double), hipMemcpyHostToDevice, h->s));
  HIPCHK(hipMemcpyAsync(h->count, &c, sizeof(int), hipMemcpyHostToDevice, h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  return GPK_OK;
}

int gpk_get_opt_state(gpk_handle* h, int64_t* count, double* mu, double* nu, int64_t n) {
  if (!h || !count || !mu || !nu) return fail(GPK_EINVAL, "NULL argument");
  if (n != h->L.nparams) return fail(GPK_EINVAL, "parameter count mismatch");
  DevSwitch ds(h->dev);
  int c = 0;
  HIPCHK(hipMemcpyAsync(mu, h->m, n * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipMemcpyAsync(nu, h->v, n * sizeof(double), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipMemcpyAsync(&c, h->count, sizeof(int), hipMemcpyDeviceToHost, h->s));
  HIPCHK(hipStreamSynchronize(h->s));
  *count = c;
  return GPK_OK;
}

int gpk_set_chain_capacity(int32_t workgroups) {
  g_chain_cap.store(workgroups > 0 ? workgroups : 0);
  return GPK_OK;
}
