// refine_panel.hip — the fused refinement step of one mode solve (gpk_internal.h RefinePanel):
//   X += K^{-1} (B - Kc X)
// One 256-thread workgroup owns a panel of 16 unfolding columns for all P mode indices.  It loads
// the X panel into LDS, forms W = B - Kc X tile row by tile row on v_mfma_f64_16x16x4 (Kc from
// L2, straight into registers; the 16-row tiles dealt to the four waves) into a second LDS panel,
// and after one barrier forms X + K^{-1} W from the two panels and stores it (with the side
// output Y = Ys / 2 + v X).  The panel's X is read once and written once and B read once: three
// tensor passes.  Independent solves of one stage share a launch (blockIdx.y).  LDS: 2 panels x P x PL doubles (PL = 17: the right form's panel load writes
// consecutive p, 17 doubles apart, to distinct banks), 136 KiB at P = 512 of the CU's 160 KiB.
#include "gpk_internal.h"

namespace gpk {

typedef double d4r __attribute__((ext_vector_type(4)));

namespace {
constexpr int PL = 17;  // panel row stride (doubles)

// O = op(Mat)[16 rows from i0][0..P) x panel[0..P)[16]: lane (li, lk) holds op(Mat)[i0 + li][k + lk]
// and panel[k + lk][li]; 8 k-substeps of Mat loads in flight.  Left form (tr = 0): acc = O, lane
// value q is O[lk + 4 q][li].  Right form (tr = 1: op = transpose): the operands swap places,
// acc = O^T, lane value q is O[li][lk + 4 q] -- consecutive lanes hold consecutive mode indices,
// which are contiguous in that form's tensors.
__device__ __forceinline__ d4r panel_product(const double* __restrict__ Mat, int P, int tr, int i0,
                                             const double* panel, int lane) {
  const int li = lane & 15, lk = lane >> 4;
  d4r acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < P; k0 += 32) {  // P is a multiple of 32
    double a[8], b[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int k = k0 + 4 * s + lk;
      a[s] = tr ? Mat[(size_t)k * P + i0 + li] : Mat[(size_t)(i0 + li) * P + k];
      b[s] = panel[k * PL + li];
    }
#pragma unroll
    for (int s = 0; s < 8; ++s)
      acc = tr ? __builtin_amdgcn_mfma_f64_16x16x4f64(b[s], a[s], acc, 0, 0, 0)
               : __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s], acc, 0, 0, 0);
  }
  return acc;
}
}  // namespace

__global__ __launch_bounds__(256) void refine_panel_kernel(RefinePanelBatch batch,
                                                           const StepScalars* __restrict__ sc) {
  const RefinePanel& r = batch.d[blockIdx.y];
  if ((int)blockIdx.x >= r.M / 16) return;  // (the grid is as wide as the batch's largest solve)
  if (!gate_open(r.gate)) return;  // refinement not needed (uniform; before any load)
  extern __shared__ double lds[];
  double* Xs = lds;
  double* Ws = lds + (size_t)r.P * PL;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int P = r.P;
  const size_t c0 = (size_t)blockIdx.x * 16;  // first unfolding column of the panel (< M)
  // the X panel: consecutive threads along the contiguous direction of the form
  for (int idx = t; idx < P * 16; idx += 256) {
    const int p = r.right ? idx % P : idx >> 4, c = r.right ? idx / P : idx & 15;
    Xs[p * PL + c] = r.X[(size_t)p * r.sp + (c0 + c) * r.sc];
  }
  __syncthreads();
  const int li = lane & 15, lk = lane >> 4;
  // W = B - Kc X
  for (int rt = wv; rt < P / 16; rt += 4) {
    const d4r acc = panel_product(r.Kc, P, r.right, rt * 16, Xs, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = rt * 16 + (r.right ? li : lk + 4 * q), c = r.right ? lk + 4 * q : li;
      Ws[p * PL + c] = r.B[(size_t)p * r.sp + (c0 + c) * r.sc] - acc[q];
    }
  }
  __syncthreads();
  // X + K^{-1} W
  const double vv = r.Y ? sc->v : 0.0;
  for (int rt = wv; rt < P / 16; rt += 4) {
    const d4r acc = panel_product(r.Kinv, P, r.right, rt * 16, Ws, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = rt * 16 + (r.right ? li : lk + 4 * q), c = r.right ? lk + 4 * q : li;
      const size_t o = (size_t)p * r.sp + (c0 + c) * r.sc;
      const double x = Xs[p * PL + c] + acc[q];
      r.X[o] = x;
      if (r.Y) r.Y[o] = 0.5 * r.Ys[o] + vv * x;
    }
  }
}

static size_t panel_lds_bytes(int P) { return (size_t)2 * P * PL * sizeof(double); }

hipError_t refine_panel_prepare() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(refine_panel_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)panel_lds_bytes(REFINE_PANEL_MAX_P));
}

hipError_t launch_refine_panel(const RefinePanel* rs, int n, const StepScalars* sc, hipStream_t s) {
  if (n < 1 || n > REFINE_MAX_BATCH) return hipErrorInvalidValue;
  RefinePanelBatch b{};
  int pmax = 0, panels = 0;
  for (int i = 0; i < n; ++i) {
    const RefinePanel& r = rs[i];
    if (r.P < 32 || (r.P & 31) || r.P > REFINE_PANEL_MAX_P || r.M < 16 || (r.M & 15) || (r.Y && !sc))
      return hipErrorInvalidValue;
    b.d[i] = r;
    pmax = std::max(pmax, r.P);
    panels = std::max(panels, r.M / 16);
  }
  hipLaunchKernelGGL(refine_panel_kernel, dim3(panels, n), dim3(256), panel_lds_bytes(pmax), s, b, sc);
  return hipGetLastError();
}

}  // namespace gpk
