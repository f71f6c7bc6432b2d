// spdinv.hip — SPD inverse + log-determinant of the covariance factors (gfx950, fp64 MFMA).
//
// Replaces jnp.linalg.solve (LU getrf/getrs) and jnp.linalg.slogdet (a second LU) of
//   code/model_GP_solver_1d.py:92,135-137 and code/model_GP_solver_2d.py:104-105,157-162.
// The step needs K^{-1} explicitly anyway (the log-det gradient is K^{-1}), so every solve
// becomes an MFMA GEMM against K^{-1} and the log-det falls out of the Cholesky pivots.
//
// Algorithm: blocked Cholesky-Gauss-Jordan sweep, 32x32 pivot blocks.  For pivot block P
// (the current Schur complement S = X_PP = L L^T, Cholesky-factored in LDS by one workgroup):
//     V   = L^{-1} X_P.                  (panel "TRSM" by MFMA against L^{-1})
//     X_RR -= V_R^T V_R                  (symmetric rank-32 update, like SYRK)
//     X_PR  = L^{-T} V_R,  X_RP = X_PR^T,  X_PP = -L^{-T} L^{-1}
// After every block is swept X = -K^{-1}; the last sweep flips the sign.  Using L^{-1}
// (not X_PP^{-1}) for the update keeps the accuracy of a Cholesky-based inverse: a plain
// block Gauss-Jordan with explicit X_PP^{-1} lost ~4 digits at cond(K) = 1e7.
// log det K = sum_k 2 sum_i log L_ii over pivot blocks.  A non-positive pivot raises
// GPK_ENOTPD through *status.
//
// Three forms of the same arithmetic, bitwise equal to one another:
//   * sweep_kernel: one launch per pivot block (ping-pong X -> Y, no intra-launch hazards); a
//     256-thread workgroup owns one 32x32 output tile (4 waves x 16x16 v_mfma_f64_16x16x4
//     quadrants) and recomputes the two 32x32 panel pieces it needs; the workgroup that produces
//     the NEXT pivot tile factors it in its tail, so the next launch finds L^{-1} ready: N/32
//     launches, batched over both Kronecker factors.  The reference of the other two.
//   * chain_kernel: every sweep in ONE launch, a workgroup per tile, ordered by flags and
//     self-validating words; one workgroup per factor runs the pivot chain (chain_master, with a
//     two-block look-ahead in chain_master_la).
//   * chain_multi_kernel: the same with a macro tile per workgroup, for large 1D factors.
// sweep_kernel and chain_kernel share the accumulator layout (q_row, q_col, q_elem), the
// quadrant product (mma_f) and the four-case tile update (sweep_update), and chain_kernel's
// gather sites share gather_k / gather_d; the host side has one batch builder and one (deriv,
// gather) dispatch for both chain launches.  chain_multi_kernel, the two pivot-chain masters
// and ChainFactor keep their own text: folded, the C2 step measured slower.
#include <algorithm>

#include "gpk_internal.h"
#include "spd_pivot.h"
#include "gpk_trace.h"
#include "prep_dev.h"

namespace gpk {

GPK_WAIT_LIMIT_SETTER(wait_limit_spdinv)  // gpk_set_wait_limit

GPK_TRACE_TU(spdinv)

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int SA = 34;  // LDS row stride for A-role tiles (conflict-free ds_read_b64 A[i][k])
constexpr int SB = 48;  // LDS row stride for B-role tiles (conflict-free B[k][j])
struct SpdBatch {
  double* X[2];   // buffer holding the assembled K (even sweeps read it)
  double* Y[2];   // pong buffer (odd sweeps read it)
  int p[2];
  int T[2];       // p / 32
  double* piv[2]; // [T][32*32] L^{-1} of each pivot block
  double* ldet[2];
  double* pst[2];  // refinement gate [2]: K_00, bits of max diag K^{-1} (gate_open)
  int n[2];        // true size: padded rows (identity) are left out of pst
  int* status[2];
};

__global__ __launch_bounds__(256) void pivot_init_kernel(SpdBatch b) {
  const int m = blockIdx.x;
  __shared__ double A[32 * SP], M[32 * SP], pv[32];
  const int t = threadIdx.x;
  const double* X = b.X[m];
  const int p = b.p[m];
  for (int e = t; e < 1024; e += 256) A[(e >> 5) * SP + (e & 31)] = X[(size_t)(e >> 5) * p + (e & 31)];
  __syncthreads();
  const double ls = pivot_chol_inv_1w(A, M, pv, t, b.status[m]);
  double* piv = b.piv[m];
  for (int e = t; e < 1024; e += 256) piv[e] = M[(e >> 5) * SP + (e & 31)];
  if (t == 0) {
    b.ldet[m][0] = ls;
    b.pst[m][0] = X[0];  // K_00 = max diag K (stationary kernel + jitter)
    b.pst[m][1] = 0.0;   // max diag K^{-1}: atomicMax'd by the last sweep
  }
}

// The MFMA accumulator layout: element r of wave quadrant (wr, wc) of a 32x32 tile is the tile's
// row q_row(wr, lane, r), column q_col(wc, lane).
__device__ __forceinline__ int q_row(int wr, int lane, int r) { return 16 * wr + (lane >> 4) + 4 * r; }
__device__ __forceinline__ int q_col(int wc, int lane) { return 16 * wc + (lane & 15); }
// ... and element 32 row + col of the tile stored densely (the pivot chain's input slots)
__device__ __forceinline__ int q_elem(int wr, int wc, int lane, int r) {
  return q_row(wr, lane, r) * 32 + q_col(wc, lane);
}

// The one 32-deep quadrant product: acc += A B, this wave's 16x16 quadrant (wr, wc); fa(i, k),
// fb(k, j) give the operands.  The k order (4 kk + lk) and the operand roles are what keeps the
// three inverse paths (sweep, chain, multi-tile chain) bitwise equal.
template <class FA, class FB>
__device__ __forceinline__ d4 mma_f(FA fa, FB fb, int wr, int wc, int lane, d4 acc) {
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    const int k = 4 * kk + lk;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa(16 * wr + li, k), fb(k, 16 * wc + li), acc, 0, 0, 0);
  }
  return acc;
}
// ... with A (i, k) at a[i*sai + k*sak] and B (k, j) at bm[k*sbk + j*sbj]: strides let one LDS
// image serve transposed reads
__device__ __forceinline__ d4 mma_t(const double* a, int sai, int sak, const double* bm, int sbk,
                                    int sbj, int wr, int wc, int lane, d4 acc) {
  return mma_f([&](int i, int k) { return a[i * sai + k * sak]; },
               [&](int k, int j) { return bm[k * sbk + j * sbj]; }, wr, wc, lane, acc);
}

// One sweep's update of tile (I, J) by pivot block P, this wave's quadrant (ip: I == P, jp:
// J == P).  lt = L^{-T} (i, k), l = L^{-1} (k, j), vit = V_I^T (i, k), vj = V_J (k, j); x: the
// tile before the sweep.  Every product is accumulated from zero and then negated / subtracted.
template <class LT, class L, class VIT, class VJ>
__device__ __forceinline__ d4 sweep_update(bool ip, bool jp, LT lt, L l, VIT vit, VJ vj, int wr,
                                           int wc, int lane, d4 x) {
  const d4 zero = {0.0, 0.0, 0.0, 0.0};
  if (ip && jp) return -mma_f(lt, l, wr, wc, lane, zero);  // -L^{-T} L^{-1}
  if (ip) return mma_f(lt, vj, wr, wc, lane, zero);        // L^{-T} V_J
  if (jp) return mma_f(vit, l, wr, wc, lane, zero);        // V_I^T L^{-1}
  return x - mma_f(vit, vj, wr, wc, lane, zero);           // x - V_I^T V_J
}

// ... with L^{-1} in sL [32][SA] and V_I, V_J in sVI, sVJ [32][SB] (sweep_kernel, chain_kernel)
__device__ __forceinline__ d4 sweep_update_lds(bool ip, bool jp, const double* sL, const double* sVI,
                                               const double* sVJ, int wr, int wc, int lane, d4 x) {
  return sweep_update(
      ip, jp, [&](int i, int k) { return sL[k * SA + i]; }, [&](int k, int j) { return sL[k * SA + j]; },
      [&](int i, int k) { return sVI[k * SB + i]; }, [&](int k, int j) { return sVJ[k * SB + j]; }, wr, wc,
      lane, x);
}

__device__ __forceinline__ void store_quad(double* s, int ld, int wr, int wc, int lane, d4 v) {
#pragma unroll
  for (int r = 0; r < 4; ++r) s[q_row(wr, lane, r) * ld + q_col(wc, lane)] = v[r];
}

__global__ __launch_bounds__(256) void sweep_kernel(SpdBatch b, int k) {
  // grid (nmat, tiles): the factors are interleaved in dispatch order, and tile numbering starts
  // at the tile that factors the next pivot (the critical path of the launch): it is dispatched
  // first instead of after up to 2 T^2 other workgroups
  const int m = blockIdx.x;
  const int p = b.p[m];
  const int T = b.T[m];
  if (k >= T) return;  // this factor is already inverted
  const int last = (k == T - 1);
  if ((int)blockIdx.y >= T * T) return;
  const int tile = (int)(blockIdx.y + (last ? 0 : (k + 1) * (T + 1))) % (T * T);
  const int I = tile / T, J = tile % T;
  // probes: the block that factors the next pivot (tile (0,0) of factor 0 in the last sweep)
  const bool trb = threadIdx.x == 0 && m == 0 && k < 16 && blockIdx.y == 0;
  if (trb) TR_LO(SLOT_SWEEP + k);
  const double* X = (k & 1) ? b.Y[m] : b.X[m];
  double* Y = (k & 1) ? b.X[m] : b.Y[m];
  const double* Li = b.piv[m] + (size_t)k * 1024;  // L^{-1} of pivot block k

  __shared__ double sL[32 * SA];                 // L^{-1}
  __shared__ double sXI[32 * SB], sXJ[32 * SB];  // X_PI, X_PJ, then V_I, V_J
  __shared__ double sP[32 * SP], sM[32 * SP], pv[32];  // next-pivot scratch
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int tx = t & 31, ty = t >> 5;
  const int P = k;

  // prefetch this wave's quadrant of X_IJ (consumed only in the epilogue)
  d4 xij = {0.0, 0.0, 0.0, 0.0};
  if (I != P && J != P) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      xij[r] = X[(size_t)(I * 32 + q_row(wr, lane, r)) * p + J * 32 + q_col(wc, lane)];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = ty + 8 * r;
    sL[row * SA + tx] = Li[row * 32 + tx];
    if (I != P) sXI[row * SB + tx] = X[(size_t)(P * 32 + row) * p + I * 32 + tx];
    if (J != P && J != I) sXJ[row * SB + tx] = X[(size_t)(P * 32 + row) * p + J * 32 + tx];
  }
  __syncthreads();
  const double* sVJ = (J == I) ? sXI : sXJ;
  // V_I = L^{-1} X_PI, V_J = L^{-1} X_PJ (in place, after everyone has read the inputs)
  d4 vi = {0.0, 0.0, 0.0, 0.0}, vj = {0.0, 0.0, 0.0, 0.0};
  if (I != P) vi = mma_t(sL, SA, 1, sXI, SB, 1, wr, wc, lane, vi);
  if (J != P && J != I) vj = mma_t(sL, SA, 1, sXJ, SB, 1, wr, wc, lane, vj);
  __syncthreads();
  if (I != P) store_quad(sXI, SB, wr, wc, lane, vi);
  if (J != P && J != I) store_quad(sXJ, SB, wr, wc, lane, vj);
  __syncthreads();

  const d4 acc = sweep_update_lds(I == P, J == P, sL, sXI, sVJ, wr, wc, lane, xij);

  const double fin = last ? -1.0 : 1.0;
  const bool nextpiv = (!last) && I == k + 1 && J == k + 1;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = q_row(wr, lane, r), col = q_col(wc, lane);
    const size_t o = (size_t)(I * 32 + row) * p + J * 32 + col;
    const double y = acc[r];
    Y[o] = y * fin;
    if (nextpiv) sP[row * SP + col] = y;
    if (last && I == J && row == col) pv[row] = (I * 32 + row < b.n[m]) ? y * fin : 0.0;
  }
  if (last && I == J) {  // block-uniform: refinement gate, max_i (K^{-1})_ii of this block
    __syncthreads();
    if (t == 0) {
      double mx = 0.0;
      for (int j = 0; j < 32; ++j) mx = fmax(mx, pv[j]);
      // positive doubles order like their bit patterns
      atomicMax(reinterpret_cast<unsigned long long*>(b.pst[m] + 1),
                (unsigned long long)__double_as_longlong(mx));
    }
    if (trb) TR_HI(SLOT_SWEEP + k);
    return;
  }
  if (!nextpiv) {  // block-uniform
    if (trb) TR_HI(SLOT_SWEEP + k);
    return;
  }
  __syncthreads();
  if (trb) TR_LO(SLOT_SWEEP_PIVOT + k);
  const double ls = pivot_chol_inv_1w(sP, sM, pv, t, b.status[m]);
  double* piv = b.piv[m] + (size_t)(k + 1) * 1024;
  for (int e = t; e < 1024; e += 256) piv[e] = sM[(e >> 5) * SP + (e & 31)];
  if (t == 0) b.ldet[m][k + 1] = ls;
  if (trb) TR_HI(SLOT_SWEEP_PIVOT + k);
  if (trb) TR_HI(SLOT_SWEEP + k);
}

// ---- persistent dataflow form ("chain"): every sweep in ONE launch ------------------------
// The sweep above pays a launch boundary per pivot block: the pivot workgroup's pre-pivot work
// (~4 us of loads + two MFMA passes) plus the inter-kernel gap (~1.7 us) on top of the 5.4-us
// factorisation, 8 times at 256^2 (tools/timeline.py).  Here one workgroup per tile owns its
// tile for the whole inverse (in MFMA accumulators) and sweeps are ordered by flags:
//   * tile (I, J) is read by other workgroups only as the panel of sweep I; its owner publishes
//     it once, after sweep I-1, into the panel buffer PB (write-once, no ping-pong hazard);
//   * L^{-1} of pivot k is published once into piv[k] by the owner of (k, k);
//   * hand-offs follow MI355X_MICROARCH.md's sc1 row: payload stored sc1 by every wave, each
//     wave's vmcnt(0), a barrier, one lane's sc1 flag store; the consumer polls the flag with an
//     sc1 load, a barrier, then sc1 loads of the payload.
// The per-sweep critical path is the pivot owner's hop (poll + loads + two MFMA passes) plus its
// factorisation.  All workgroups wait on one another, so the grid must be co-resident: used
// only when the grid fits the device's co-resident capacity (spd_chain_capacity: occupancy per CU
// x CUs; two per CU on a full MI355X) and at most CHAIN_MAX_BLOCKS.  The arithmetic is the
// sweep kernel's operation for operation: the results are bitwise equal.

struct ChainFactor {
  double* X;            // in: assembled K (read mode); out: K^{-1}
  double* PB;           // panel buffer [p*p]: tile (I, J) as it is after sweep I-1
  double* piv;          // [T][32*32] L^{-1} of each pivot block
  double* ldet;         // [T]
  double* pst;          // refinement gate [2]
  int* status;
  // [T*TC] panel ready (chain_kernel); the 2T + 1 words after them (once the pivot-ready flags, a
  // gap and the done counter) keep their place in the ABI's allocation; chain_kernel uses none of
  // them, chain_multi_kernel (no flags) still counts its exits on the last, at T*T + 2T.  A flag
  // carries the TAG of the launch that raised it, epoch + 1 (chain_tag), and no kernel ever clears
  // one: a waiter spins until the word EQUALS its own launch's tag, and a word left by any earlier
  // launch of the factor differs from it -- also when that launch laid the buffer out for another
  // TC (the step's augmented launch, TC = T + tu + td, and the K^{-1}-only launch, TC = T, share
  // it: the tag is unique per launch of the factor, whatever its layout) and in the create-time /
  // reset_handoffs state (all zero, epoch 0: the first tag is 1).  The epoch advances by exactly
  // one per launch and wraps at 2^32 like the tag; equality needs no order, so the wrap itself is
  // harmless.  A stale word could pass only if it was last written exactly 2^32 launches of the
  // factor ago -- or never since the reset, at the one launch whose tag is 0 -- and every launch
  // rewrites every word it waits on in its own layout.
  unsigned int* flags;
  double* gran;              // the pivot chain's input slots [T][3][1024] (chain_master)
  int la;                    // chain_kernel: two-block look-ahead in the pivot chain (chain_master)
  double* PB2;               // hand-off slots [2][chain_half] by launch parity (self-validating)
  // [CHAIN_EPOCH_WORDS] launch counter: its parity selects the PB2 half, epoch + 1 tags the flags.
  // One 128-byte line further (CHAIN_STARTED) chain_kernel's `started` count: every active
  // workgroup of the factor adds one after its last read of the epoch (chain_arrive), and the pivot
  // chain's workgroup, the first to finish, zeroes it and advances the epoch once all have
  // (chain_advance).  chain_multi_kernel advances the epoch from its last workgroup to exit.
  unsigned int* epoch;
  int piv_off;               // T * TC (once the offset of the pivot-ready flags; unused)
  int p, n, T;
  // gather mode: K from the distance classes (+ jitter), kept copy Kc and D written on the way
  const int* cid; const double* kval; const double* dval; const double* x; double jitter;
  double* Kc; double* D;
  // augmented right-hand sides: tile columns T.. of the sweep operator's upper-right block end
  // as K^{-1} [B_u | D^T]  (gpk_internal.h ChainArgs)
  int tu, td;
  const double* Bu; int ldbu, bu_t;
  double* Ou; int ldou, ou_t;
  double* Od; int ldod;
  double* PBa; int ldpba;
};
struct ChainBatch {
  ChainFactor f[2];
  int nmat;
  PrepArgs prep;  // published by workgroup (0, nmat) when the grid has that extra row
  int q;
  int mpos;       // chain_multi_kernel: linear index of the pivot chain's workgroup
};

__device__ __forceinline__ void st_sc1(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_sc1(const double* p) {
  return __hip_atomic_load(const_cast<double*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The launch's tag: what its flags hold once raised (ChainFactor::flags).  ep: the epoch word as
// this workgroup loaded it at its start.
__device__ __forceinline__ unsigned chain_tag(unsigned ep) { return ep + 1u; }
// bounded (spd_pivot.h spin_until_eq): a flag that never takes this launch's tag sets status bit 2
__device__ __forceinline__ void wait_flag(unsigned int* f, unsigned tag, int* status) {
  (void)spin_until_eq<1>(f, tag, status);
}
// every wave drained its sc1 stores -> barrier -> one lane raises the flag
__device__ __forceinline__ void signal_flag(unsigned int* f, unsigned tag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(f, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A workgroup's arrival on the factor's `started` count: ONE non-returning agent-scope add by one
// thread, which nothing in the workgroup waits for.  The epoch may advance as soon as the count is
// full, so NO THREAD OF THE WORKGROUP MAY READ THE EPOCH WORD AFTER THIS IS ISSUED -- and an add
// is not ordered behind another wave's outstanding load.  chain_kernel's tile workgroups
// therefore issue it in sweep 0 behind the barrier that
// follows the LDS stores of L_0^{-1}: every thread loads those words through an address formed
// from its own copy of the epoch (the PB2 half) and stores them to LDS before that barrier, so
// every wave reaches it only with its epoch load returned.  The pivot chain's workgroup arrives
// in chain_advance.
__device__ __forceinline__ void chain_arrive(const ChainFactor& F) {
  (void)__hip_atomic_fetch_add(F.epoch + CHAIN_STARTED, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The pivot chain's workgroup, after its last L^{-1} and ldet are stored (it is the first of the
// factor to finish: the tiles' last sweep is still ahead, ~3 us at C4): its own arrival, then one
// thread polls `started` until all `active` workgroups of the factor have arrived -- they did
// tens of microseconds ago, so this is one load round trip under the tiles' last sweep -- zeroes
// it and advances the epoch for the next launch.  Nothing waits at the launch's end any more:
// a tile workgroup exits after its output stores.  The barrier: every thread of this workgroup
// has stored L^{-1} words through its own copy of the epoch before it (chain_arrive's condition).
// Bounded like every wait; a poll that gives up (status bit 2) leaves both words alone -- the
// host resets them (reset_handoffs), and until then the later launches of a captured batch see a
// count that never fits and give up within 64 polls.
__device__ __forceinline__ void chain_advance(const ChainFactor& F, unsigned ep, unsigned active, bool tr) {
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned int* started = F.epoch + CHAIN_STARTED;
  chain_arrive(F);
  if (!spin_until_eq<1>(started, active, F.status)) return;
  __hip_atomic_store(started, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(F.epoch, ep + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tr) TR_HI(SLOT_CHAIN_BUMP);
}

// The pivot chain's inputs travel as self-validating words (MI355X_MICROARCH.md hand-off row
// handoff-1to1; cdna_hip_programming.md Guideline 16 R2 with the data as its own flag): every
// fp64 element is ONE 8-byte sc1 store into a slot that holds a sentinel (a signalling-NaN bit
// pattern, which no floating-point operation produces: results are quieted) until it is
// written.  The producer neither drains its stores nor raises a flag; the pivot chain, the
// slot's only reader, loads the words, re-loads any that still hold the sentinel, and after
// consuming a slot writes the sentinel back (ready for the next launch; the buffer is
// initialised to the sentinel at create, gpk_create.cpp).  Slot k (hop k, the inputs of pivot
// k+1): [0] panel tile (k, k+1), [1] diagonal tile (k+1, k+1), both after sweep k-1; element
// e = 32 row + col of the tile.  Look-ahead mode (chain_master, below) hands over the tiles one
// sweep older instead: slot h (read while pivot h+1 is factored): [0] tile (h, h+2),
// [1] tile (h+1, h+2), [2] tile (h+2, h+2), all after sweep h-1.
__device__ __forceinline__ double* gran_at(const ChainFactor& F, int slot, int which, int e) {
  return F.gran + (size_t)(2 * slot + which) * 1024 + e;
}
__device__ __forceinline__ double* gran3_at(const ChainFactor& F, int slot, int which, int e) {
  return F.gran + (size_t)(3 * slot + which) * 1024 + e;
}
__device__ __forceinline__ bool gran_ok(double v) {
  return __double_as_longlong(v) != (long long)CHAIN_SENTINEL;
}
// The one gather.  D(i, j) of distance class u (zero on the pads, u < 0; advection, DERIV 1: signed
// by x_i - x_j) ...
template <int DERIV>
__device__ __forceinline__ double class_d(const ChainFactor& F, int u, int i, int j) {
  double dv = u >= 0 ? F.dval[u] : 0.0;
  if (DERIV == 1 && u >= 0 && !(F.x[i] - F.x[j] >= 0.0)) dv = -dv;  // JAX abs'(0) = +1
  return dv;
}
// ... D(i, j) from the class tables, or the stored D in read mode (the augmented D^T columns)
template <int DERIV, bool GATHER>
__device__ __forceinline__ double gather_d(const ChainFactor& F, int i, int j) {
  const size_t o = (size_t)i * F.p + j;
  return GATHER ? class_d<DERIV>(F, F.cid[o], i, j) : F.D[o];
}
// K(i, j) from the distance classes (+ jitter on the diagonal; identity on the pads), or from X in
// read mode.  write (gather mode): the kept copy Kc and D are stored on the way.
template <int DERIV, bool GATHER>
__device__ __forceinline__ double gather_k(const ChainFactor& F, int i, int j, bool write) {
  const size_t o = (size_t)i * F.p + j;
  if (!GATHER) return F.X[o];
  const int u = F.cid[o];
  double kv, dv;
  if (u >= 0) {  // (both table reads in one branch: they are in flight together)
    kv = F.kval[u];
    if (i == j) kv += F.jitter;
    dv = class_d<DERIV>(F, u, i, j);
  } else {
    kv = (i == j) ? 1.0 : 0.0;
    dv = 0.0;
  }
  if (write) {
    if (F.Kc) F.Kc[o] = kv;
    if (DERIV && F.D) F.D[o] = dv;
  }
  return kv;
}

// one 16x16 quadrant product with both operands in registers: a[kk] = A(i, 4 kk + lk),
// b[kk] = B(4 kk + lk, j) of lane (li, lk) -- mma_t's operation sequence
__device__ __forceinline__ d4 mma_r(const double (&a)[8], const double (&b)[8], d4 acc) {
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk], acc, 0, 0, 0);
  return acc;
}
// ... with A from LDS (element (i, k) at a[i * sai + k * sak], i = 16 wr + li)
__device__ __forceinline__ d4 mma_lr(const double* a, int sai, int sak, const double (&b)[8], int wr,
                                     int lane, d4 acc) {
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < 8; ++kk)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[(16 * wr + li) * sai + (4 * kk + lk) * sak], b[kk], acc, 0, 0, 0);
  return acc;
}

struct NoTileSource {  // (chain_multi_kernel: no look-ahead)
  __device__ double operator()(int, int) const { return 0.0; }
};

// The pivot chain with a two-block window (chain_kernel, ChainFactor::la).  The plain form below
// receives pivot h+1's inputs -- tiles (h, h+1) and (h+1, h+1) after sweep h-1 -- from their
// owners, who can start them only when L_{h-1}^{-1} is visible: that path (L^{-1} words landing,
// loads, LDS, three barriers and MFMAs, stores landing, re-load) is longer than this
// workgroup's own period (hop + factorisation), so every hop began with a 0.4-0.6 us wait
// (C4, profiles/r7_c4_timeline.txt).  Here the
// workgroup forms those inputs itself: while wave 0 factors pivot h+1 (the one-wave form), waves
// 1-3 apply sweep h to the 2x2 window's remaining tiles with the L_h^{-1} and V1 = L_h^{-1}
// X_{h,h+1} that are still in LDS,
//     V2 = L_h^{-1} P2,   Q' = Q - V1^T V2,   D2' = D2 - V2^T V2,
// where P2, Q, D2 = tiles (h, h+2), (h+1, h+2), (h+2, h+2) after sweep h-1 are what the owners
// hand over (slot h, self-validating words): one sweep older than before, i.e. a whole period
// more slack.  Q' and D2' are tiles (h+1, h+2) and (h+2, h+2) after sweep h: the next hop's
// inputs, left in LDS before the factorisation's closing barrier.  Hop 0's own inputs, tiles
// (0, 1) and (1, 1), are K itself: read through `kf` (class tables or X) like tile (0, 0), by
// waves 1-3 while pivot 0 is factored; slot 0 holds K's tiles (0, 2), (1, 2), (2, 2).
// Every product is the owner's own operation sequence (mma_t's operand roles and k order, the
// product accumulated from zero and then subtracted): the pivots receive bit for bit the inputs
// they receive in the plain form.
// Waves 1-3 must not meet at the workgroup barrier (wave 0 is factoring), so each is
// self-sufficient, operands in registers: wave 1 + c (c = 0, 1) forms the 16-column half c of V2
// (its C-layout quadrants ARE the B operand of V1^T V2 and both operands of V2^T V2), that half
// of Q' and the diagonal quadrant (c, c) of D2'; wave 3 forms both halves of V2 again and the two
// mixed quadrants of D2'.  About 40 (48) MFMAs per wave against a 4.3-us factorisation.
// L_h^{-1} must survive factorisation h+1: the factorisations alternate between sM and sM2; the
// panel tile alternates between sX and sX2 (V1 is read while Q' is written).
// Consumed slots get the sentinel back after the closing barrier (P2's words are read by two
// waves).  LDS: sX, sX2 [32][SB]; sP, sM, sM2, sD [32][SP]; pv [32].
template <class KF>
__device__ __forceinline__ void chain_master_la(const ChainFactor& F, int T, d4 acc, double* sX,
                                                double* sX2, double* sP, double* sM, double* sM2,
                                                double* sD, double* pv, bool trm, bool trla,
                                                double* lw, KF kf) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  // (the lane's row / column, re-derived from an opaque copy of the lane id wherever the
  // look-ahead forms addresses: hoisted out of the hop loop, its element offsets would stay live
  // across the factorisation, which is the kernel's register peak -- they spilled)
  int li = lane & 15, lk = lane >> 4;
  int wq = __builtin_amdgcn_readfirstlane(wv), c = 0, nw = 0;  // wave, its column half, its words
  auto fresh_lane = [&]() {
    int l = lane, w = __builtin_amdgcn_readfirstlane(wv);
    asm volatile("" : "+v"(l), "+s"(w));
    li = l & 15;
    lk = l >> 4;
    wq = w;
    c = wq == 2 ? 1 : 0;
    nw = wq == 3 ? 24 : 20;
  };
  __builtin_amdgcn_s_setprio(3);
  const double snan = __longlong_as_double((long long)CHAIN_SENTINEL);
  // word i of this wave's look-ahead inputs, as an offset into the slot's three tiles (0: P2,
  // 1: Q, 2: D2; element e = 32 row + col) from the lane's own 32 lk + li -- wave-uniform.
  // Waves 1, 2 (c = wv - 1): 0..7 P2 as B operand of column half c, 8..15 Q's quadrants (0, c),
  // (1, c), 16..19 D2's quadrant (c, c).  Wave 3: 0..15 P2 as B operand of both halves, 16..19
  // D2's quadrant (0, 1), 20..23 its quadrant (1, 0).
  auto woff = [&](int i) -> int {
    if (i < 8) return 128 * i + 16 * c;
    if (i < 16) return wq == 3 ? 16 + 128 * (i - 8) : 1024 + 512 * ((i - 8) >> 2) + 128 * (i & 3) + 16 * c;
    if (i < 20) return 2048 + 128 * (i & 3) + (wq == 3 ? 16 : 528 * c);
    return 2048 + 512 + 128 * (i & 3);
  };
  // waves 1-3, during factorisation h+1: the window's sweep h (h + 2 < T)
  auto lookahead = [&](int h) {
    double* sV1 = (h & 1) ? sX2 : sX;   // V1 (this hop's panel tile)
    double* sQn = (h & 1) ? sX : sX2;   // <- Q': the next hop's panel tile
    const double* Lh = (h & 1) ? sM2 : sM;
    fresh_lane();
    const double* g = gran3_at(F, h, 0, 32 * lk + li);
    double w[24];
    // (per lane) words not yet written hold the sentinel: load again.  Bounded like every
    // hand-off wait.
    for (unsigned spins = 0;; ++spins) {
      bool ok = true;
#pragma unroll
      for (int i = 0; i < 24; ++i) {
        w[i] = i < nw ? ld_sc1(g + woff(i)) : 0.0;
        ok = ok && gran_ok(w[i]);
      }
#ifdef GPK_TRACE
      const bool late = spins == 0 && __any(!ok);  // (some word of this wave was not there yet)
      if (trla && late) { TR_LO(SLOT_LOOKAHEAD_LATE); TR_HI(SLOT_LOOKAHEAD_LATE); }
#endif
      if (ok || spin_give_up(spins, F.status)) break;
      __builtin_amdgcn_s_sleep(1);
    }
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    double pa[8], va[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) pa[i] = w[i];
    // V2, column half c (wave 3: half 0): quadrants (0, c), (1, c); as an operand, k = 4 kk + lk
    // is row lk + 4 (kk & 3) of quadrant row kk >> 2
    const d4 v0 = mma_lr(Lh, SP, 1, pa, 0, lane, zero), v1 = mma_lr(Lh, SP, 1, pa, 1, lane, zero);
#pragma unroll
    for (int i = 0; i < 4; ++i) { va[i] = v0[i]; va[4 + i] = v1[i]; }
    if (wq != 3) {
      d4 q0 = {w[8], w[9], w[10], w[11]}, q1 = {w[12], w[13], w[14], w[15]};
      d4 d2 = {w[16], w[17], w[18], w[19]};
      q0 = q0 - mma_lr(sV1, 1, SB, va, 0, lane, zero);  // Q - V1^T V2
      q1 = q1 - mma_lr(sV1, 1, SB, va, 1, lane, zero);
      d2 = d2 - mma_r(va, va, zero);                     // D2 - V2^T V2
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sQn[(lk + 4 * r) * SB + 16 * c + li] = q0[r];
        sQn[(16 + lk + 4 * r) * SB + 16 * c + li] = q1[r];
        sD[(16 * c + lk + 4 * r) * SP + 16 * c + li] = d2[r];
      }
    } else {
      double pb[8], vb[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) pb[i] = w[8 + i];
      const d4 u0 = mma_lr(Lh, SP, 1, pb, 0, lane, zero), u1 = mma_lr(Lh, SP, 1, pb, 1, lane, zero);
#pragma unroll
      for (int i = 0; i < 4; ++i) { vb[i] = u0[i]; vb[4 + i] = u1[i]; }
      d4 d01 = {w[16], w[17], w[18], w[19]}, d10 = {w[20], w[21], w[22], w[23]};
      d01 = d01 - mma_r(va, vb, zero);
      d10 = d10 - mma_r(vb, va, zero);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sD[(lk + 4 * r) * SP + 16 + li] = d01[r];
        sD[(16 + lk + 4 * r) * SP + li] = d10[r];
      }
    }
  };
  // slot h consumed: the sentinel back for the next launch (waves 1, 2: their words; wave 3: its
  // D2 quadrants -- P2's words are waves 1 and 2's)
  auto rearm = [&](int h) {
    fresh_lane();
    double* g = gran3_at(F, h, 0, 32 * lk + li);
#pragma unroll
    for (int i = 0; i < 24; ++i)
      if (i < nw && !(wq == 3 && i < 16)) st_sc1(g + woff(i), snan);
  };
  auto factor = [&](int kp) {
    if (trm && kp > 0 && kp < 17) TR_HI(SLOT_SWEEP + kp - 1);
    store_quad(sP, SP, wr, wc, lane, acc);
    __syncthreads();
    if (trm && kp > 0 && kp < 17) TR_LO(SLOT_SWEEP_PIVOT + kp - 1);
    if (trm && kp == 0) TR_LO(SLOT_PIVOT0);
    double* Mk = (kp & 1) ? sM2 : sM;
    if (wv > 0) {  // (wave 0 goes straight to the factorisation)
      if (kp >= 2) rearm(kp - 2);  // the slot read during factorisation kp - 1
      if (kp == 0 && T > 1) {
        // hop 0's inputs: tiles (0, 1) and (1, 1) of K.  (From an opaque copy of the thread id,
        // as fresh_lane: this branch now sits in the pivot loop, and its 11 element offsets,
        // hoisted out of the loop, would stay live across every factorisation -- they spilled)
        int t0 = t;
        asm volatile("" : "+v"(t0));
#pragma unroll
        for (int it = 0; it < 11; ++it) {
          const int e = t0 - 64 + 192 * it;
          if (e >= 2048) continue;
          const int row = (e >> 5) & 31, col = e & 31;
          if (e < 1024) sX[row * SB + col] = kf(row, 32 + col);
          else sD[row * SP + col] = kf(32 + row, 32 + col);
        }
      } else if (kp > 0 && kp + 1 < T) {
        lookahead(kp - 1);
      }
    }
    const double ls = pivot_chol_inv_1w<double*, NoPivotHook>(sP, Mk, pv, t, F.status);
    double* ldst = lw + (size_t)kp * 1024;
    for (int e = t; e < 1024; e += 256) st_sc1(ldst + e, Mk[(e >> 5) * SP + (e & 31)]);
    if (t == 0) F.ldet[kp] = ls;
    if (trm && kp > 0 && kp < 17) TR_HI(SLOT_SWEEP_PIVOT + kp - 1);
    if (trm && kp == 0) TR_HI(SLOT_PIVOT0);
  };
  if (t == 0) {  // refinement gate (as the plain form)
    st_sc1(F.pst, acc[0]);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(F.pst + 1), 0ull, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the zeroing, before any L^{-1} word: below)
  // ONE call site of factor(): the unrolled factorisation (~10 KB) is inlined once, so pivot 0
  // runs the loop's copy and leaves it warm in the instruction cache for pivot 1 (with a call
  // ahead of the loop, pivot 0 ran a copy used once per launch and pivot 1 the loop's copy cold)
  for (int kp = 0; kp < T; ++kp) {
    if (kp > 0) {  // hop kp - 1: acc = tile (kp, kp) after sweep kp - 1
      const int h = kp - 1;
      if (trm && h < 16) TR_LO(SLOT_SWEEP + h);
      double* sXh = (h & 1) ? sX2 : sX;
      const double* Lh = (h & 1) ? sM2 : sM;
      // (q_row / q_col's layout with the opaque li, lk of fresh_lane: formed from `lane`, these
      // offsets are hoisted out of the hop loop and stay live across the factorisation -- above)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = sD[(16 * wr + lk + 4 * r) * SP + 16 * wc + li];
      d4 vj = {0.0, 0.0, 0.0, 0.0};
      vj = mma_t(Lh, SP, 1, sXh, SB, 1, wr, wc, lane, vj);  // V1 = L_h^{-1} X_{h,h+1}
      __syncthreads();
      store_quad(sXh, SB, wr, wc, lane, vj);
      __syncthreads();
      d4 prod = {0.0, 0.0, 0.0, 0.0};
      prod = mma_t(sXh, 1, SB, sXh, SB, 1, wr, wc, lane, prod);  // V1^T V1
      acc = acc - prod;
    }
    factor(kp);
  }
}

// The pivot chain of one factor (chain_kernel, chain_multi_kernel): one workgroup factors every
// pivot block in order.  acc: this wave's quadrant of tile (0, 0) of K.  LDS: sXJ [32][SB],
// sP / sM [32][SP], pv [32].  LOOKAHEAD (chain_kernel): the two-block window above when the
// launch asks for it (ChainFactor::la), with its extra LDS (win) and K's tiles (kf).
struct ChainWindow {
  double *sX2, *sM2, *sD;
  bool trla;  // probes: lane 0 of wave 1, factor 0
};
template <bool ONEWAVE, bool LOOKAHEAD = false, class KF = NoTileSource>
__device__ __forceinline__ void chain_master(const ChainFactor& F, int T, d4 acc, double* sXJ,
                                             double* sP, double* sM, double* pv, bool trm,
                                             bool early_flag, double* lw = nullptr,
                                             ChainWindow win = ChainWindow(), KF kf = KF()) {
  if constexpr (LOOKAHEAD) {
    if (F.la) {  // (launch-uniform)
      chain_master_la(F, T, acc, sXJ, win.sX2, sP, sM, win.sM2, win.sD, pv, trm, win.trla, lw, kf);
      return;
    }
  }
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int tx = t & 31, ty = t >> 5;
  __shared__ int s_pflag;  // pivot_chol_inv_1w's "wave 0 passed block step 5" flag
    // (issue priority over the tile workgroup that may share its CU: this one is the chain)
  __builtin_amdgcn_s_setprio(3);
  // The pivot chain, kept in one workgroup: after factoring pivot k it holds L_k^{-1} in LDS,
  // so pivot k+1's Schur complement X_{k+1,k+1} - V^T V (V = L_k^{-1} X_{k,k+1}) needs no hop
  // for L_k^{-1}; its two inputs (the panel tile (k, k+1) and the diagonal tile (k+1, k+1)
  // after sweep k-1) are handed over (self-validating words, above) by their owners while this
  // workgroup is still factoring pivot k.  Same operations as the owner's update of that tile:
  // bitwise equal.  Their loads are issued inside that factorisation (PivotPrefetch, after block
  // step 5) and checked after it; words that were not yet written are re-loaded.
  // element of this thread: panel tile (LDS-staging layout: row ty + 8r, column tx) and the
  // diagonal tile (MFMA quadrant layout)
  auto ex = [&](int r) { return (ty + 8 * r) * 32 + tx; };
  auto ed = [&](int r) { return (16 * wr + (lane >> 4) + 4 * r) * 32 + 16 * wc + (lane & 15); };
  double gx[4], gd[4];
  auto issue = [&](int k) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      gx[r] = ld_sc1(gran_at(F, k, 0, ex(r)));
      gd[r] = ld_sc1(gran_at(F, k, 1, ed(r)));
    }
  };
  struct PivotPrefetch {
    __device__ constexpr bool waves() const { return true; }  // every thread issues its own words
    decltype(issue)* f;
    int k, T;
    __device__ void early() {}
    __device__ void pre() {}
    __device__ void post() {
      if (k + 1 < T) (*f)(k);
    }
  };
  // L^{-1}_kp is stored right after its factorisation, as self-validating words: no drain, no
  // flag -- the chain does not stall on the write-back of any pivot
  auto factor = [&](int kp) {
    if (trm && kp > 0 && kp < 17) TR_HI(SLOT_SWEEP + kp - 1);  // (inputs in: the hop ends)
    store_quad(sP, SP, wr, wc, lane, acc);
    __syncthreads();
    if (trm && kp > 0 && kp < 17) TR_LO(SLOT_SWEEP_PIVOT + kp - 1);
    if (trm && kp == 0) TR_LO(SLOT_PIVOT0);
    PivotPrefetch hook{&issue, kp, T};
    // ONEWAVE (chain_kernel): the one-wave factorisation (spd_pivot.h pivot_chol_inv_1w, 4.3 vs
    // 5.0 us), waves 1-3 issuing their prefetch words when wave 0 passes block step 5;
    // chain_multi_kernel keeps the four-wave form (its tile path is at the register limit: the
    // one-wave form's accumulators would spill there)
    double ls;
    if (ONEWAVE)
      ls = pivot_chol_inv_1w<double*, PivotPrefetch>(sP, sM, pv, t, F.status, &s_pflag, hook);
    else
      ls = pivot_chol_inv_block<4, double*, PivotPrefetch>(sP, sM, pv, t, F.status, hook);
    // L^{-1}_kp as self-validating words in this launch's slots (lw), no flag
    double* ldst = lw + (size_t)kp * 1024;
    for (int e = t; e < 1024; e += 256) st_sc1(ldst + e, sM[(e >> 5) * SP + (e & 31)]);
    if (t == 0) F.ldet[kp] = ls;
    if (trm && kp > 0 && kp < 17) TR_HI(SLOT_SWEEP_PIVOT + kp - 1);
    if (trm && kp == 0) TR_HI(SLOT_PIVOT0);
  };
  // refinement gate: K_00 = max diag K (stationary kernel + jitter), and max diag K^{-1}
  // zeroed here
  if (t == 0) {
    st_sc1(F.pst, acc[0]);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(F.pst + 1), 0ull, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  if (t == 0) s_pflag = 0;  // (the barrier inside factor(0) orders it before the pivot)
  // the zeroing above completes before any L^{-1} word is stored (every diagonal tile's atomicMax
  // comes after it has read L^{-1}_0's words)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // ONE call site of factor() (one inlined copy of the factorisation, as in chain_master_la):
  // pivot 0 factors acc = tile (0, 0) of K, gathered above; pivot kp > 0 follows hop kp - 1
  for (int kp = 0; kp < T; ++kp) {
    if (kp > 0) {
      const int k = kp - 1;
      // (early_flag, chain_multi: the barrier of the pivot-ready flag this hop once raised; L_k^{-1}
      // travels as self-validating words now, the barrier keeps the hop's schedule)
      if (early_flag) __syncthreads();
      bool ok = true;
#pragma unroll
      for (int r = 0; r < 4; ++r) ok = ok && gran_ok(gx[r]) && gran_ok(gd[r]);
      if (trm && !ok) { TR_LO(SLOT_PREFETCH_MISS); TR_HI(SLOT_PREFETCH_MISS); }  // (thread 0's words)
      // (per lane) words not yet written when they were loaded: load them again.  Bounded: a
      // hand-off that never arrives flags the status word (the step reports an error) instead of
      // hanging the device.
      for (unsigned spins = 0; !ok; ++spins) {
        if (spin_give_up(spins, F.status)) break;
        __builtin_amdgcn_s_sleep(1);
        issue(k);
        ok = true;
#pragma unroll
        for (int r = 0; r < 4; ++r) ok = ok && gran_ok(gx[r]) && gran_ok(gd[r]);
      }
      if (trm && k < 16) TR_LO(SLOT_SWEEP + k);
#pragma unroll
      for (int r = 0; r < 4; ++r) {  // prefetched during pivot k's factorisation
        sXJ[(ty + 8 * r) * SB + tx] = gx[r];
        acc[r] = gd[r];
        // consumed: the sentinel back into the slot for the next launch
        st_sc1(gran_at(F, k, 0, ex(r)), __longlong_as_double((long long)CHAIN_SENTINEL));
        st_sc1(gran_at(F, k, 1, ed(r)), __longlong_as_double((long long)CHAIN_SENTINEL));
      }
      __syncthreads();
      d4 vj = {0.0, 0.0, 0.0, 0.0};
      vj = mma_t(sM, SP, 1, sXJ, SB, 1, wr, wc, lane, vj);  // V = L_k^{-1} X_{k,k+1}
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // L^{-1}_k's stores (long drained)
      __syncthreads();
      store_quad(sXJ, SB, wr, wc, lane, vj);
      __syncthreads();
      d4 prod = {0.0, 0.0, 0.0, 0.0};
      prod = mma_t(sXJ, 1, SB, sXJ, SB, 1, wr, wc, lane, prod);  // V^T V
      acc = acc - prod;
    }
    factor(kp);
  }
}

template <int DERIV, bool GATHER>
__global__ __launch_bounds__(256, 2) void chain_kernel(ChainBatch b) {
  const int m = blockIdx.y;
  if (m == b.nmat) {  // the step constants (+ a folded batch begin), off the critical path
    if (blockIdx.x == 0) publish_prep(b.prep, b.q);
    copy_snapshot(b.prep, blockIdx.x, gridDim.x);
    return;
  }
  const ChainFactor& F = b.f[m];
  const int T = F.T, p = F.p;
  const int TC = T + F.tu + F.td;  // tile columns: K, then the augmented B_u, D^T columns
  if ((int)blockIdx.x > T * TC) return;
  // the pivot chain's own workgroup (below) is tile index T*TC; it and the tiles feeding it are
  // dispatched in the grid's middle, alone on their CUs (gpk_internal.h chain_role)
  const int tile = chain_role(m, (int)blockIdx.x, T, TC);
  const bool master = tile == T * TC;
  const int I = master ? 0 : tile / TC, J = master ? 0 : tile % TC;
  const bool aug = J >= T;
  const int ja = J - T;  // augmented tile column
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int tx = t & 31, ty = t >> 5;
  unsigned int* panel_rdy = F.flags;
  // panel tile (row k) of column J: K part in PB, augmented part in PBa
  auto panel_ptr = [&](int k, int row, int col) -> double* {
    return J < T ? F.PB + (size_t)(k * 32 + row) * p + J * 32 + col
                 : F.PBa + (size_t)(k * 32 + row) * F.ldpba + ja * 32 + col;
  };
  __shared__ double sL[32 * SA];
  __shared__ double sXI[32 * SB], sXJ[32 * SB];
  __shared__ double sP[32 * SP], sM[32 * SP], pv[32];
  __shared__ double sD[32 * SP];  // the pivot chain's look-ahead: its next diagonal tile
  // L_k^{-1} as self-validating words (chain_multi_kernel's form) in this launch's half of the
  // L^{-1} slots (PB2, launch parity; the other half is reset by the tile workgroups): the tile
  // workgroups see L_k^{-1} as soon as its stores land, with no flag of the pivot chain's.
  // The epoch: read here by every thread and never again (chain_arrive); its parity selects the
  // half, epoch + 1 tags this launch's panel flags.
  const unsigned ep = __hip_atomic_load(F.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned tag = chain_tag(ep);
  double* PLc = F.PB2 + (size_t)(ep & 1u) * chain_half(p, false);

  // own tile, this wave's quadrant
  d4 acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = I * 32 + q_row(wr, lane, r);
    if (!aug) {  // (the pivot chain's copy of tile (0, 0) leaves Kc and D to the tile's owner)
      acc[r] = gather_k<DERIV, GATHER>(F, i, J * 32 + q_col(wc, lane), !master);
      continue;
    }
    // B_u[i][j'] or D^T[i][j'] = D[j'][i] (j' = column inside the part)
    const int jl = ja * 32 + q_col(wc, lane);
    if (ja < F.tu)
      acc[r] = F.bu_t ? F.Bu[(size_t)(jl) * F.ldbu + i] : F.Bu[(size_t)i * F.ldbu + jl];
    else
      acc[r] = gather_d<DERIV, GATHER>(F, jl - 32 * F.tu, i);
  }
  auto publish_tile = [&](void) {  // panel tile (I, J) <- acc, then its flag
#pragma unroll
    for (int r = 0; r < 4; ++r) st_sc1(panel_ptr(I, q_row(wr, lane, r), q_col(wc, lane)), acc[r]);
    signal_flag(panel_rdy + I * TC + J, tag);
  };
  // the pivot chain's inputs of hop kk (after sweep kk-1): panel tile (kk, kk+1) and diagonal
  // tile (kk+1, kk+1) as granules (chain_master), before any other store of the tile
  // Look-ahead mode (F.la): the chain forms those two itself and takes the window's other tiles,
  // one sweep older: (kk, kk+2), (kk+1, kk+2), (kk+2, kk+2) after sweep kk-1 into slot kk
  auto chain_inputs = [&](int kk) {
    int which;
    if (F.la) {
      which = (J != kk + 2 || kk + 2 >= T) ? -1 : I - kk;
      if (which < 0 || which > 2) return;
    } else {
      which = (I == kk && J == kk + 1) ? 0 : (I == J && I == kk + 1) ? 1 : -1;
      if (which < 0 || kk + 1 >= T) return;
    }
    double* slot = F.la ? gran3_at(F, kk, which, 0) : gran_at(F, kk, which, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      st_sc1(slot + q_elem(wr, wc, lane, r), acc[r]);
  };
  // K's element (i, j) as the gather above forms it (the pivot chain's hop-0 tiles)
  auto k_at = [&](int i, int j) -> double { return gather_k<DERIV, GATHER>(F, i, j, false); };
  const bool trm = t == 0 && m == 0;  // probes (gpk_trace.h): factor 0's pivot owners
  if (master) {
    // (a tile workgroup's sL and sXI are free here: the second L^{-1} and panel buffers)
    const ChainWindow win{sXI, sL, sD, t == 64 && m == 0};
    chain_master<true, true>(F, T, acc, sXJ, sP, sM, pv, trm, false, PLc, win, k_at);
    if (t == 0 && m == 1) TR_HI(SLOT_CHAIN_M1);
    if (t == 0 && m == 1) TR_LO(SLOT_CHAIN_M1);
    chain_advance(F, ep, (unsigned)(T * TC + 1), trm);  // T*TC tiles + this workgroup
    return;
  }
  if (trm && tile == 0) TR_LO(SLOT_GATHER);
  chain_inputs(0);                       // tiles (0, 1) and (1, 1) as they are before sweep 0
  if (I == 0 && J != 0) publish_tile();  // row 0 is the panel of sweep 0
  {  // this tile's share of the other half's L^{-1} slots (last launch's) -> sentinel
    double* PLo = F.PB2 + (size_t)((ep & 1u) ^ 1u) * chain_half(p, false);
    const int share = (T * 1024 + T * TC - 1) / (T * TC);
    const int e1 = min(T * 1024, (tile + 1) * share);
    for (int e = tile * share + t; e < e1; e += 256) PLo[e] = __longlong_as_double((long long)CHAIN_SENTINEL);
  }

  for (int k = 0; k < T; ++k) {
    const bool needI = I != k, needJ = J != k && J != I;
    // issue priority over the CU's other workgroup when this tile feeds sweep k+1's panel or
    // the pivot chain
    if (I == k + 1 || (I == k + 2 && J == k + 2)) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(0);
    // the panel tiles are usually published long before the pivot: fetch them first, then
    // wait for L^{-1}_k
    if (t == 0) {
      if (needI) wait_flag(panel_rdy + k * TC + I, tag, F.status);
      if (needJ) wait_flag(panel_rdy + k * TC + J, tag, F.status);
    }
    __syncthreads();
    double xi[4], xj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ty + 8 * r;
      xi[r] = needI ? ld_sc1(F.PB + (size_t)(k * 32 + row) * p + I * 32 + tx) : 0.0;
      xj[r] = needJ ? ld_sc1(panel_ptr(k, row, tx)) : 0.0;
    }
    const bool trl = t == 0 && m == 0 && k == T - 1 && I == T - 1 && J == T - 1;
    double lv[4];
    {
      // one thread polls one word of L_k^{-1} (the polling traffic of a flag), then every thread
      // loads its words and re-loads those still holding the sentinel (bounded)
      const double* Lw = PLc + (size_t)k * 1024;
      if (t == 0) {
        for (unsigned spins = 0; !gran_ok(ld_sc1(Lw + 1023)); ++spins) {
          if (spin_give_up(spins, F.status)) break;
          __builtin_amdgcn_s_sleep(1);
        }
      }
      __syncthreads();
      if (trl) TR_HI(SLOT_LAST_FLAG);
#pragma unroll
      for (int r = 0; r < 4; ++r) lv[r] = ld_sc1(Lw + (ty + 8 * r) * 32 + tx);
      for (unsigned spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int r = 0; r < 4; ++r) ok = ok && gran_ok(lv[r]);
        if (ok) break;
        if (spin_give_up(spins, F.status)) break;
        __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (!gran_ok(lv[r])) lv[r] = ld_sc1(Lw + (ty + 8 * r) * 32 + tx);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ty + 8 * r;
      sL[row * SA + tx] = lv[r];
      if (needI) sXI[row * SB + tx] = xi[r];
      if (needJ) sXJ[row * SB + tx] = xj[r];
    }
    __syncthreads();
    // (every thread's L_0^{-1} words came through its own copy of the epoch and are in LDS:
    // chain_arrive's condition holds from here on)
    if (k == 0 && t == 0) chain_arrive(F);
    if (trl) TR_HI(SLOT_LAST_LDS);
    const double* sVJ = (J == I) ? sXI : sXJ;
    d4 vi = {0.0, 0.0, 0.0, 0.0}, vj = {0.0, 0.0, 0.0, 0.0};
    if (needI) vi = mma_t(sL, SA, 1, sXI, SB, 1, wr, wc, lane, vi);
    if (needJ) vj = mma_t(sL, SA, 1, sXJ, SB, 1, wr, wc, lane, vj);
    __syncthreads();
    if (needI) store_quad(sXI, SB, wr, wc, lane, vi);
    if (needJ) store_quad(sXJ, SB, wr, wc, lane, vj);
    __syncthreads();
    acc = sweep_update_lds(I == k, J == k, sL, sXI, sVJ, wr, wc, lane, acc);
    // panel of sweep k + 1 (the diagonal tile's panel slot is the pivot chain's: nobody reads
    // a (k, k) panel tile)
    chain_inputs(k + 1);  // tiles (k+1, k+2), (k+2, k+2) after sweep k: pivot k+2's inputs
    if (k + 1 < T && I == k + 1 && J != I) publish_tile();
    if (trl) TR_HI(SLOT_LAST_MMA);
    __syncthreads();  // LDS is refilled next sweep
  }
  if (aug) {  // upper-right block: +K^{-1} B (B_u part possibly stored transposed)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // (q_row / q_col written out: called here they cost chain_kernel 4 VGPRs, 250 -> 254, which
      // <0, false> does not have -- see DESIGN section 5)
      const int i = I * 32 + 16 * wr + (lane >> 4) + 4 * r, jl = ja * 32 + 16 * wc + (lane & 15);
      if (ja < F.tu) {
        if (F.ou_t) F.Ou[(size_t)jl * F.ldou + i] = acc[r];
        else F.Ou[(size_t)i * F.ldou + jl] = acc[r];
      } else {
        F.Od[(size_t)i * F.ldod + jl - 32 * F.tu] = acc[r];
      }
    }
  }
  // K^{-1} = -X after the last sweep
#pragma unroll
  for (int r = 0; r < 4 && !aug; ++r) {
    const int row = q_row(wr, lane, r), col = q_col(wc, lane);
    const double y = -acc[r];
    F.X[(size_t)(I * 32 + row) * p + J * 32 + col] = y;
    if (I == J && row == col) pv[row] = (I * 32 + row < F.n) ? y : 0.0;
  }
  __syncthreads();
  if (I == J && t == 0) {  // refinement gate: max_i (K^{-1})_ii of this block
    double mx = 0.0;
    for (int j = 0; j < 32; ++j) mx = fmax(mx, pv[j]);
    atomicMax(reinterpret_cast<unsigned long long*>(F.pst + 1), (unsigned long long)__double_as_longlong(mx));
  }
  if (trm && tile == 0) TR_HI(SLOT_GATHER);
  // A tile workgroup ends here: nothing is counted at the exit and no flag is cleared (the flags
  // are tagged, the epoch is advanced by the pivot chain's workgroup: chain_advance).
#ifdef GPK_TRACE
  // probes: thread 0's stores drained (wave 0's share of the outputs; its atomicMax returned) in
  // tile (T-1, T-1) and the last augmented tile of factor 0, and -- SLOT_CHAIN_END, an estimate of
  // the launch's last exit from a sample -- in up to four tiles per factor of row max(T-2, 0),
  // which are among the heaviest of the last sweep (two panel products and the update; their
  // augmented outputs possibly stored transposed)
  const bool tr_out = t == 0 && m == 0 && I == T - 1 && J == T - 1;
  const bool tr_aug = t == 0 && m == 0 && I == T - 1 && J == TC - 1;
  const bool tr_end = t == 0 && I == (T > 1 ? T - 2 : 0) && J >= TC - 4;
  if (tr_out || tr_aug || tr_end) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (tr_out) TR_HI(SLOT_LAST_OUT);
  if (tr_aug) TR_HI(SLOT_LAST_AUG);
  if (tr_end) TR_HI(SLOT_CHAIN_END);
#endif
}

// ---- multi-tile chain: large factors (1D, p up to 2048) -------------------------------------
// chain_kernel owns one 32x32 tile per workgroup (T^2 workgroups: p <= ~700).  Here a workgroup
// owns a LOWER macro tile -- rows {2R, 2R+1} x one pair of 32-column tiles {2C, 2C+1}, C < R --
// and up to one tile of its macro row's diagonal 2x2 block (multi_role: the three lower tiles
// go to three different workgroups of the row from R = 3 on, so no workgroup updates more than
// five tiles per sweep) -- so p = 2048 needs 1 + 32*31/2 = 497 workgroups + the pivot chain
// (two per CU).  The pivot chain is chain_kernel's (chain_master); per sweep k a
// tile workgroup:
//   * waits for the panel tiles of its row / column pairs and L_k^{-1}, loads them (sc1);
//   * forms V = L_k^{-1} X_{k,.} for its (up to) four tile rows / columns (MFMA, LDS);
//   * updates its (up to) five tiles (seven in macro row 1) with chain_kernel's operations -- first the tiles that
//     feed the next sweep's panel or the pivot chain, published together (one drain + barrier),
//     then the rest.
// Storage is the lower triangle: panel slot (k, J) of PB holds X_{k,J} after sweep k-1; for J > k
// it is the transpose of lower tile (J, k), published transposed by its owner.  The same
// operation sequence per tile as chain_kernel (bitwise equal results); K^{-1} is written to both
// triangles at the end.  V tiles are XOR-swizzled in LDS (element (k, j) at 32k + (j ^ 16(k&1)):
// conflict-free fragment reads without padding), so the workgroup needs 42 KB.
__device__ __forceinline__ int vsw(int k, int j) { return 32 * k + (j ^ ((k & 1) << 4)); }

// slot s of a macro-tile workgroup: s < 4 the column pair c0 (rows 2R + (s >> 1), column
// 2 c0 + (s & 1)), s = 4..6 the diagonal block (2R,2R), (2R+1,2R), (2R+1,2R+1)
__host__ __device__ inline void multi_slot(int s, int R, int c0, int& I, int& J) {
  if (s < 4) {
    I = 2 * R + (s >> 1);
    J = 2 * c0 + (s & 1);
  } else {
    I = 2 * R + (s == 4 ? 0 : 1);
    J = 2 * R + (s == 6 ? 1 : 0);
  }
}

// macro-tile workgroup g (0-based) -> macro row R, its column pair c0 (-1: none) and the tiles of
// the diagonal 2x2 block it holds (dmask bit s - 4 for slot s).  Row 0: the diagonal block only;
// row R >= 1: R workgroups c0 = 0 .. R-1.  The pivot chain's inputs after sweep k are tiles
// (k+2, k+1) and (k+2, k+2), and every workgroup updates all of its tiles in every sweep, so the
// workgroup holding an input tile must not be slowed by extra tiles: (2R+1, 2R+1) goes to c0 =
// R-1, (2R, 2R) to R-2 and (2R+1, 2R) to R-3 (rows 1, 2: to c0 = 0 where those do not exist).
// Round 2's form gave the whole block to c0 = R-1: seven tiles, four of them in the critical
// pass of sweep 2R-1, which set the C2 sweep cycle.
__host__ __device__ inline void multi_role(int g, int& R, int& c0, int& dmask) {
  if (g == 0) {
    R = 0; c0 = -1; dmask = 7;
    return;
  }
  int r = 1, first = 1;  // first workgroup of macro row r: 1 + r(r-1)/2
  while (first + r <= g) { first += r; ++r; }
  R = r;
  c0 = g - first;
  const int o4 = r >= 2 ? r - 2 : 0, o5 = r >= 3 ? r - 3 : 0, o6 = r - 1;
  dmask = (c0 == o4 ? 1 : 0) | (c0 == o5 ? 2 : 0) | (c0 == o6 ? 4 : 0);
}

__host__ __device__ inline int multi_workgroups(int T) {  // per factor, + the pivot chain
  const int MT = (T + 1) / 2;
  return 1 + MT * (MT - 1) / 2 + 1;
}

template <int DERIV, bool GATHER>
__global__ __launch_bounds__(256, 2) void chain_multi_kernel(ChainBatch b) {
  const int m = blockIdx.y;
  if (m == b.nmat) {  // the step constants (+ a folded batch begin), off the critical path
    if (blockIdx.x == 0) publish_prep(b.prep, b.q);
    copy_snapshot(b.prep, blockIdx.x, gridDim.x);
    return;
  }
  const ChainFactor& F = b.f[m];
  const int T = F.T, p = F.p;
  const int nwg = multi_workgroups(T);
  if ((int)blockIdx.x >= nwg) return;
  // the pivot chain's workgroup sits at linear index mpos (host: a CU the dispatcher's second
  // pass over the CUs does not double up), the tile workgroups around it
  const int mpos = b.mpos < nwg ? b.mpos : 0;
  const bool master = (int)blockIdx.x == mpos;
  if (master && threadIdx.x == 0 && m == 0) TR_WHO(SLOT_MCP_MPOS, blockIdx.x);
  int R = 0, c0 = -1, dmask = 0;
  if (!master) multi_role((int)blockIdx.x - ((int)blockIdx.x > mpos ? 1 : 0), R, c0, dmask);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int tx = t & 31, ty = t >> 5;
  // panel hand-off: self-validating words (chain_master's inputs, above) in the PB2 half of this
  // launch's parity; the other half (last launch's) is reset to the sentinel meanwhile, a chunk
  // per tile workgroup and sweep, off the critical path.  No flags, no drains.
  // L_k^{-1} travels the same way (PLc, after the panel slots in each half; no pivot flags): it
  // is normally written before the panel row it goes with, so it arrives with the panel's loads
  unsigned int* done = F.flags + T * T + 2 * T;
  const unsigned ep = __hip_atomic_load(F.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const size_t hs = multi_half(p);
  double* PBc = F.PB2 + (size_t)(ep & 1u) * hs;
  double* PBo = F.PB2 + (size_t)((ep & 1u) ^ 1u) * hs;
  double* PLc = PBc + (size_t)p * p;
  // LDS: L_k^{-1} [32][SA] + four swizzled V tiles; the pivot chain's sXJ / sP / sM alias them
  __shared__ double pool[32 * SA + 4 * 1024];
  __shared__ double pv[32];
  __shared__ unsigned int s_last;
  __shared__ double sQ[4 * 16 * 17];  // per-wave transposition blocks (publish_stores)
  double* sL = pool;
  double* sV = pool + 32 * SA;

  auto valid = [&](int s) {
    if (master) return false;
    if (s < 4 && c0 < 0) return false;
    if (s >= 4 && !((dmask >> (s - 4)) & 1)) return false;
    int I, J;
    multi_slot(s, R, c0, I, J);
    return I < T && J <= I;
  };
  // gathered / read K value (and Kc, D written) at (i, j)
  auto kval_at = [&](int i, int j, bool write) -> double {
    const size_t o = (size_t)i * p + j;
    if (GATHER) {
      const int u = F.cid[o];
      double kv, dv;
      if (u >= 0) {
        kv = F.kval[u];
        if (i == j) kv += F.jitter;
        dv = F.dval[u];
        if (DERIV == 1 && !(F.x[i] - F.x[j] >= 0.0)) dv = -dv;  // JAX abs'(0) = +1
      } else {
        kv = (i == j) ? 1.0 : 0.0;
        dv = 0.0;
      }
      if (write) {
        if (F.Kc) F.Kc[o] = kv;
        if (DERIV && F.D) F.D[o] = dv;
      }
      return kv;
    }
    return F.X[o];
  };
  d4 acc[7];
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    acc[s] = d4{0.0, 0.0, 0.0, 0.0};
    if (!valid(s)) continue;
    int I, J;
    multi_slot(s, R, c0, I, J);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = I * 32 + 16 * wr + (lane >> 4) + 4 * r, j = J * 32 + 16 * wc + (lane & 15);
      acc[s][r] = kval_at(i, j, true);
      if (GATHER && I != J && (F.Kc || (DERIV && F.D))) (void)kval_at(j, i, true);  // mirrored Kc / D
    }
  }
  const bool trm = t == 0 && m == 0;
  if (master) {
    d4 a0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      a0[r] = kval_at(16 * wr + (lane >> 4) + 4 * r, 16 * wc + (lane & 15), false);
    double* sXJ = pool;             // [32][SB]
    double* sP = pool + 32 * SB;    // [32][SP]
    double* sM = sP + 32 * SP;      // [32][SP]
    chain_master<false>(F, T, a0, sXJ, sP, sM, pv, trm, true, PLc);
  }

  // hand-offs after sweep kk - 1 (kk = k + 1; kk = 0: before sweep 0): panel row kk -- tile
  // (kk, J), J < kk as is, tile (I, kk), I > kk transposed (stores of every publishing tile of
  // the pass, one drain + barrier, flags) -- and, as granules first, the pivot chain's inputs of
  // hop kk: tile (kk+1, kk) (= panel tile (kk, kk+1) transposed) and the diagonal tile
  // (kk+1, kk+1)
  auto publishes = [&](int s, int kk) {
    int I, J;
    multi_slot(s, R, c0, I, J);
    return kk < T && ((I == kk && J < kk) || (J == kk && I > kk));
  };
  auto chain_in = [&](int s, int kk) {
    int I, J;
    multi_slot(s, R, c0, I, J);
    return kk + 1 < T && I == kk + 1 && (J == kk || J == I);
  };
  // a wave's 16x16 quadrant stored transposed -- element (row, col) of the tile to
  // dst[col * ld + row] -- through its own LDS block (no workgroup barrier): each store
  // instruction then writes 4 whole 128-B column segments instead of 16 lines x 32 B
  auto put_transposed = [&](double* dst, size_t ld, const d4& a) {
    double* q = sQ + wv * (16 * 17);
#pragma unroll
    for (int r = 0; r < 4; ++r) q[((lane >> 4) + 4 * r) * 17 + (lane & 15)] = a[r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int e = lane + 64 * r, c = e >> 4, rr = e & 15;  // quadrant column c, row rr
      st_sc1(dst + (size_t)(16 * wc + c) * ld + 16 * wr + rr, q[rr * 17 + c]);
    }
    __builtin_amdgcn_wave_barrier();
  };
  // stores of the publishing tiles (sc1, not waited for here): which = 0 the pivot chain's input
  // tiles (granules, and their panel slots when they publish), 1 the other publishing tiles
  auto publish_stores = [&](int kk, int which) {
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      if (which != 0 || !valid(s) || !chain_in(s, kk)) continue;
      int I, J;
      multi_slot(s, R, c0, I, J);
      if (I == J) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * wr + (lane >> 4) + 4 * r, col = 16 * wc + (lane & 15);
          st_sc1(gran_at(F, kk, 1, row * 32 + col), acc[s][r]);
        }
      } else {  // (kk+1, kk) -> element (col, row) of panel tile (kk, kk+1)
        put_transposed(gran_at(F, kk, 0, 0), 32, acc[s]);
      }
    }
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      if (!valid(s) || !publishes(s, kk) || chain_in(s, kk) != (which == 0)) continue;
      int I, J;
      multi_slot(s, R, c0, I, J);
      if (I == kk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * wr + (lane >> 4) + 4 * r, col = 16 * wc + (lane & 15);
          st_sc1(PBc + (size_t)(kk * 32 + row) * p + J * 32 + col, acc[s][r]);
        }
      } else {  // (I, kk) -> slot (kk, I) transposed
        put_transposed(PBc + (size_t)(kk * 32) * p + I * 32, (size_t)p, acc[s]);
      }
    }
  };
  if (!master) {
    publish_stores(0, 0);
    publish_stores(0, 1);
  }
  // this workgroup's share of the other half's reset: [rs0, rs1), a chunk per sweep
  const size_t ntot = hs;
  const int gidx = (int)blockIdx.x - ((int)blockIdx.x > mpos ? 1 : 0);
  const size_t share = (ntot + (nwg - 2)) / (nwg - 1);
  const size_t rs0 = std::min(ntot, (size_t)gidx * share), rs1 = std::min(ntot, rs0 + share);
  const size_t rchunk = (share + T - 1) / T;

  __shared__ unsigned s_lword_;  // sweep k + 1 once thread 0 has seen a word of L_k^{-1}
  volatile unsigned* s_lword = &s_lword_;
  if (t == 0) *s_lword = 0u;
  __syncthreads();
  // V slots: 0, 1 = rows 2R, 2R+1; 2, 3 = the plain column pair's columns 2c0, 2c0+1
  auto vslot_of_col = [&](int s) { return s < 4 ? 2 + (s & 1) : (s == 6 ? 1 : 0); };
  for (int k = 0; k < T && !master; ++k) {
    // probes (gpk_trace.h SLOT_MC_*): the workgroup owning tile (k+2, k+2), factor 0
    const bool trc = t == 0 && m == 0 && k < 16 &&
                     ((k + 2 == 2 * R && (dmask & 1)) || (k + 2 == 2 * R + 1 && (dmask & 4)));
    // issue priority: the sweep's front half (loads, V, the pass-0 tiles that feed sweep k+1 and
    // the pivot chain) over the pass-1 products of the workgroup sharing this CU
    __builtin_amdgcn_s_setprio(2);
    bool need[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int idx = v < 2 ? 2 * R + v : 2 * c0 + (v - 2);
      need[v] = (v < 2 || c0 >= 0) && idx < T && idx != k;
    }
    // panel tiles of sweep k: load, re-load the words still holding the sentinel (bounded)
    double xv[4][4];
    auto load_panel = [&]() {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int idx = v < 2 ? 2 * R + v : 2 * c0 + (v - 2);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          xv[v][r] = need[v] ? ld_sc1(PBc + (size_t)(k * 32 + ty + 8 * r) * p + idx * 32 + tx) : 0.0;
      }
    };
    auto panel_ok = [&]() {
      bool ok = true;
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int r = 0; r < 4; ++r) ok = ok && gran_ok(xv[v][r]);
      return ok;
    };
    // re-load while waiting: only each tile's first word (r = 0) until those are in, then the
    // words still holding the sentinel -- a quarter of the polling traffic of ~500 waiting
    // workgroups, which otherwise delays the very stores they wait for
    auto reload_panel = [&]() {
      bool head = true;
#pragma unroll
      for (int v = 0; v < 4; ++v) head = head && gran_ok(xv[v][0]);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int idx = v < 2 ? 2 * R + v : 2 * c0 + (v - 2);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (need[v] && !gran_ok(xv[v][r]) && (r == 0 || head))
            xv[v][r] = ld_sc1(PBc + (size_t)(k * 32 + ty + 8 * r) * p + idx * 32 + tx);
      }
    };
    // L_k^{-1}'s words (row ty + 8r, column tx), loaded with the panel's; only the words still
    // holding the sentinel are loaded again
    const double* Li = PLc + (size_t)k * 1024;
    double lv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) lv[r] = __longlong_as_double((long long)CHAIN_SENTINEL);
    auto load_l = [&]() {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (!gran_ok(lv[r])) lv[r] = ld_sc1(Li + (ty + 8 * r) * 32 + tx);
    };
    auto l_ok = [&]() {
      bool ok = true;
#pragma unroll
      for (int r = 0; r < 4; ++r) ok = ok && gran_ok(lv[r]);
      return ok;
    };
    // L_k^{-1}: while the panel is awaited, thread 0 polls ONE of its words (a flag's polling
    // traffic); once that word is in, every thread issues its own words with its next panel
    // re-load, so they arrive under the panel wait instead of one round trip after it.  Polling
    // all of L_k^{-1}'s words with the panel had ~500 workgroups re-loading the same 8 KB while
    // the pivot was being factored (measured: C2 0.638 -> 0.676 ms), and so did loading them
    // once with the panel's first attempt (0.614 -> 0.677 ms): no thread touches the slots
    // before that one word is in.
    load_panel();
    if (t == 0) lv[0] = ld_sc1(Li);  // (thread 0's first word is the one polled)
    bool lissued = false;
    for (unsigned spins = 0; !panel_ok(); ++spins) {
      if (spin_give_up(spins, F.status)) break;
      if (!lissued) {
        if (t == 0 && gran_ok(lv[0])) *s_lword = k + 1;
        if (*s_lword == (unsigned)(k + 1)) {
          load_l();
          lissued = true;
        }
      }
      __builtin_amdgcn_s_sleep(1);
      reload_panel();
      if (t == 0 && !lissued) lv[0] = ld_sc1(Li);
    }
    if (trc) TR_HI(SLOT_MC_PANEL + k);
    load_l();  // (the words not yet loaded, or still holding the sentinel)
    for (unsigned spins = 0; !l_ok(); ++spins) {
      if (spin_give_up(spins, F.status)) break;
      __builtin_amdgcn_s_sleep(1);
      load_l();
    }
    if (trc) TR_HI(SLOT_MC_PIV + k);
    // probes (trace build): every workgroup that publishes panel row k + 1 in this sweep's pass 0,
    // [first, last] of its inputs-in and of its publication (SLOT_MCP_IN / SLOT_MCP_OUT)
    [[maybe_unused]] bool pubk = false;
#ifdef GPK_TRACE
#pragma unroll
    for (int s = 0; s < 7; ++s) pubk = pubk || (valid(s) && publishes(s, k + 1));
    pubk = pubk && t == 0 && m == 0 && k < 16;
    if (pubk) { TR_LO(SLOT_MCP_IN + k); TR_HI(SLOT_MCP_IN + k); TR_WHO(SLOT_MCP_WHO_IN + k, blockIdx.x); }
#endif
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ty + 8 * r;
      sL[row * SA + tx] = lv[r];
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (need[v]) sV[v * 1024 + vsw(row, tx)] = xv[v][r];
    }
    __syncthreads();
    if (trc) TR_HI(SLOT_MC_LDS + k);
    d4 vv[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      vv[v] = d4{0.0, 0.0, 0.0, 0.0};
      if (!need[v]) continue;
      const double* X = sV + v * 1024;
      vv[v] = mma_f([&](int i, int kq) { return sL[i * SA + kq]; }, [&](int kq, int j) { return X[vsw(kq, j)]; },
                    wr, wc, lane, vv[v]);  // V = L_k^{-1} X_{k,idx}
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (!need[v]) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        sV[v * 1024 + vsw(16 * wr + (lane >> 4) + 4 * r, 16 * wc + (lane & 15))] = vv[v][r];
    }
    __syncthreads();
    if (trc) TR_HI(SLOT_MC_V + k);
    // the tiles that publish after this sweep (and the pivot chain's inputs) first, their
    // stores, then the rest.  (Forming V_I^T V_J as P_I^T (M_k P_J), M_k = L_k^{-T} L_k^{-1},
    // halves the V products but moved no sweep: the critical merged workgroups keep 4 products,
    // and the 5-step C2 trajectory drifted past the oracle budget -- measured, reverted.)
    // pass 0: the pivot chain's input tiles (its next hop waits on them), stored at once; pass 1:
    // the other tiles that publish panel row k + 1; pass 2: the rest.  (A loop: unrolled three
    // times it spilled 108 B per lane.)
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
#pragma unroll
      for (int s = 0; s < 7; ++s) {
        if (!valid(s)) continue;
        const int ps = chain_in(s, k + 1) ? 0 : publishes(s, k + 1) ? 1 : 2;
        if (ps != pass) continue;
        int I, J;
        multi_slot(s, R, c0, I, J);
        const double* VI = sV + (s < 4 ? (s >> 1) : (s == 4 ? 0 : 1)) * 1024;
        const double* VJ = sV + vslot_of_col(s) * 1024;
        auto lt = [&](int i, int kq) { return sL[kq * SA + i]; };  // L^T (i, k) = L (k, i)
        auto lk = [&](int kq, int j) { return sL[kq * SA + j]; };
        auto vit = [&](int i, int kq) { return VI[vsw(kq, i)]; };  // V_I^T
        auto vj = [&](int kq, int j) { return VJ[vsw(kq, j)]; };
        d4 prod = {0.0, 0.0, 0.0, 0.0};
        if (I == k && J == k) {
          prod = mma_f(lt, lk, wr, wc, lane, prod);  // L^{-T} L^{-1}
          acc[s] = -prod;
        } else if (I == k) {
          acc[s] = mma_f(lt, vj, wr, wc, lane, prod);  // L^{-T} V_J
        } else if (J == k) {
          acc[s] = mma_f(vit, lk, wr, wc, lane, prod);  // V_I^T L^{-1}
        } else {
          prod = mma_f(vit, vj, wr, wc, lane, prod);  // V_I^T V_J
          acc[s] = acc[s] - prod;
        }
      }
      if (pass == 1 && trc) TR_HI(SLOT_MC_PROD + k);
      if (pass < 2 && k + 1 < T) publish_stores(k + 1, pass);
      if (pass == 1 && trc) TR_HI(SLOT_MC_PUB + k);
      if (pass == 1 && pubk) { TR_LO(SLOT_MCP_OUT + k); TR_HI(SLOT_MCP_OUT + k); TR_WHO(SLOT_MCP_WHO_OUT + k, blockIdx.x); }
      if (pass == 1) __builtin_amdgcn_s_setprio(0);
    }
    {  // reset chunk k of this workgroup's share of the other half
      const size_t b0 = rs0 + (size_t)k * rchunk, b1 = std::min(rs1, b0 + rchunk);
      for (size_t e = b0 + t; e < b1; e += 256)
        PBo[e] = __longlong_as_double((long long)CHAIN_SENTINEL);
    }
    __syncthreads();  // LDS is refilled next sweep
    if (trc) TR_HI(SLOT_MC_DONE + k);
  }
  // K^{-1} = -X, both triangles; refinement gate over the diagonal tiles
  double mx = 0.0;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    if (!valid(s)) continue;
    int I, J;
    multi_slot(s, R, c0, I, J);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wr + (lane >> 4) + 4 * r, col = 16 * wc + (lane & 15);
      const double y = -acc[s][r];
      F.X[(size_t)(I * 32 + row) * p + J * 32 + col] = y;
      if (I != J) F.X[(size_t)(J * 32 + col) * p + I * 32 + row] = y;
      else if (row == col && I * 32 + row < F.n) mx = fmax(mx, y);
    }
  }
  if (dmask & 5) {  // holds a diagonal tile
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if (lane == 0 && mx > 0.0)
      atomicMax(reinterpret_cast<unsigned long long*>(F.pst + 1), (unsigned long long)__double_as_longlong(mx));
  }
  // The last workgroup of this factor advances the epoch.  This kernel keeps the arrival count at
  // its exit: it raises no flags (nothing to tag or re-arm), the count is ~1 % of its launch, and
  // with chain_kernel's start-side arrival (chain_arrive / chain_advance) the 1D step measured
  // 0.9 % slower.  The count is the word behind chain_kernel's flag layout.
  __syncthreads();
  if (t == 0) s_last = atomicAdd(done, 1u) == (unsigned)(nwg - 1);
  __syncthreads();
  if (s_last && t == 0) {
    __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(F.epoch, ep + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The (deriv, gather) instance of chain_kernel / chain_multi_kernel (multi): the one dispatch of
// both launches and both capacity queries.
using ChainKernel = void (*)(ChainBatch);
static ChainKernel chain_instance(bool multi, int deriv, bool gather) {
  if (!gather) return multi ? chain_multi_kernel<0, false> : chain_kernel<0, false>;
  if (deriv == 1) return multi ? chain_multi_kernel<1, true> : chain_kernel<1, true>;
  return multi ? chain_multi_kernel<2, true> : chain_kernel<2, true>;
}

// Workgroups of a chain kernel instance the current device keeps resident at once:
// occupancy per CU (its VGPR / LDS footprint) x the CUs this device (or partition) exposes.
static int chain_capacity(ChainKernel kern) {
  int dev = 0, cus = 0, per = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, 256, 0) == hipSuccess ? per * cus : 0;
}
int spd_chain_capacity(int deriv, bool gather) { return chain_capacity(chain_instance(false, deriv, gather)); }
int spd_chain_multi_capacity(int deriv, bool gather) {
  return chain_capacity(chain_instance(true, deriv, gather));
}

int spd_chain_multi_blocks(const int* p, int nmat) {
  int w = 0;
  for (int m = 0; m < nmat; ++m) w = std::max(w, multi_workgroups(p[m] / 32));
  return w * nmat;
}

int spd_chain_blocks(const int* p, int nmat, bool aug) {
  int blocks = 0, cols = 0;
  for (int m = 0; m < nmat; ++m) cols += p[m] / 32;
  for (int m = 0; m < nmat; ++m) blocks += (p[m] / 32) * (p[m] / 32 + (aug ? cols : 0)) + 1;
  return blocks;
}

// The launch's batch: every factor's ChainArgs copied into ChainFactor's own layout (kept: the
// kernels' argument layout is part of what C2's speed was measured with), T and piv_off derived,
// and the step constants.
// False when the factors mix gather and read mode or lack the pivot chain's input slots; each
// launcher adds its own argument checks.
static bool chain_batch(ChainBatch& b, const ChainArgs* a, int nmat, const PrepArgs* prep, int q) {
  b.nmat = nmat;
  if (prep) {
    b.prep = *prep;
    b.q = q;
  }
  for (int m = 0; m < nmat; ++m) {
    ChainFactor& f = b.f[m];
    f.X = a[m].X; f.PB = a[m].PB; f.piv = a[m].piv; f.ldet = a[m].ldet; f.pst = a[m].pst;
    f.status = a[m].status; f.flags = a[m].flags; f.p = a[m].p; f.n = a[m].n; f.T = a[m].p / 32;
    f.cid = a[m].cid; f.kval = a[m].kval; f.dval = a[m].dval; f.x = a[m].x; f.jitter = a[m].jitter;
    f.Kc = a[m].Kc; f.D = a[m].D;
    f.tu = a[m].tu; f.td = a[m].td; f.Bu = a[m].Bu; f.ldbu = a[m].ldbu; f.bu_t = a[m].bu_t;
    f.Ou = a[m].Ou; f.ldou = a[m].ldou; f.ou_t = a[m].ou_t; f.Od = a[m].Od; f.ldod = a[m].ldod;
    f.PBa = a[m].PBa; f.ldpba = a[m].ldpba;
    f.gran = a[m].gran; f.la = a[m].lookahead;
    f.PB2 = a[m].PB2; f.epoch = a[m].epoch;  // (both required by both launchers)
    f.piv_off = f.T * (f.T + f.tu + f.td);
    if ((f.cid != nullptr) != (a[0].cid != nullptr) || !f.gran) return false;
  }
  return true;
}
static hipError_t chain_launch(bool multi, const ChainBatch& b, int width, int deriv, bool prep,
                               hipStream_t s) {
  const dim3 grid(width, b.nmat + (prep ? 1 : 0));
  hipLaunchKernelGGL(chain_instance(multi, deriv, b.f[0].cid != nullptr), grid, dim3(256), 0, s, b);
  return hipGetLastError();
}

hipError_t launch_spd_chain(const ChainArgs* a, int nmat, int deriv, hipStream_t s,
                            const PrepArgs* prep, int q) {
  ChainBatch b{};
  if (!chain_batch(b, a, nmat, prep, q)) return hipErrorInvalidValue;
  int Tmax = 0;
  for (int m = 0; m < nmat; ++m) {
    const ChainFactor& f = b.f[m];
    if (!f.PB2 || !f.epoch) return hipErrorInvalidValue;  // (the tag, the parity, the L^{-1} slots)
    Tmax = std::max(Tmax, f.piv_off + 1);  // + the pivot chain's workgroup
  }
  return chain_launch(false, b, Tmax, deriv, prep != nullptr, s);
}

hipError_t launch_spd_chain_multi(const ChainArgs* a, int nmat, int deriv, hipStream_t s,
                                  const PrepArgs* prep, int q) {
  ChainBatch b{};
  if (!chain_batch(b, a, nmat, prep, q)) return hipErrorInvalidValue;
  int wmax = 0;
  for (int m = 0; m < nmat; ++m) {
    const ChainFactor& f = b.f[m];
    if (f.tu || f.td || !f.PB2 || !f.epoch) return hipErrorInvalidValue;
    wmax = std::max(wmax, multi_workgroups(f.T));
  }
  // one factor: the pivot chain in the middle of the CUs that hold a single workgroup (the
  // dispatcher deals the first `cus` workgroups one per CU, the rest double up the first CUs
  // again; placement only -- the flags order everything)
  b.mpos = 0;
  int dev = 0, cus = 0;
  if (nmat == 1 && hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
      wmax > cus && wmax < 2 * cus)
    b.mpos = wmax - cus + (2 * cus - wmax) / 2;
  return chain_launch(true, b, wmax, deriv, prep != nullptr, s);
}

// The sweep form's batch; Tmax: the largest factor's tiles per dimension
static SpdBatch spd_batch(const SpdArgs* a, int nmat, int& Tmax) {
  SpdBatch b{};
  Tmax = 0;
  for (int m = 0; m < nmat; ++m) {
    b.X[m] = a[m].X; b.Y[m] = a[m].Y; b.p[m] = a[m].p; b.T[m] = a[m].p / 32;
    b.piv[m] = a[m].piv; b.ldet[m] = a[m].ldet; b.status[m] = a[m].status;
    b.pst[m] = a[m].pst; b.n[m] = a[m].n;
    Tmax = std::max(Tmax, b.T[m]);
  }
  return b;
}

// One launch of the inverse: stage -1 = pivot_init, stage k >= 0 = sweep k (bench/profiling).
hipError_t launch_spd_stage(SpdArgs* a, int nmat, int stage, hipStream_t s) {
  int Tmax;
  const SpdBatch b = spd_batch(a, nmat, Tmax);
  if (stage < 0)
    hipLaunchKernelGGL(pivot_init_kernel, dim3(nmat), dim3(256), 0, s, b);
  else
    hipLaunchKernelGGL(sweep_kernel, dim3(nmat, Tmax * Tmax), dim3(256), 0, s, b, stage);
  return hipGetLastError();
}

hipError_t launch_spd_inverse(SpdArgs* a, int nmat, double** final_out, hipStream_t s,
                              bool pivot0_done) {
  int Tmax;
  const SpdBatch b = spd_batch(a, nmat, Tmax);
  // sweep k reads (k even ? X : Y) and writes the other; T sweeps end in:
  for (int m = 0; m < nmat; ++m) final_out[m] = (b.T[m] & 1) ? a[m].Y : a[m].X;
  if (!pivot0_done) hipLaunchKernelGGL(pivot_init_kernel, dim3(nmat), dim3(256), 0, s, b);
  for (int k = 0; k < Tmax; ++k)
    hipLaunchKernelGGL(sweep_kernel, dim3(nmat, Tmax * Tmax), dim3(256), 0, s, b, k);
  return hipGetLastError();
}

}  // namespace gpk
