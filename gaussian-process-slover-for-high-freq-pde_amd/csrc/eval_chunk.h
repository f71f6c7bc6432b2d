// eval_chunk.h — host-side index arithmetic of the scattered-point calls (gpk_evaluate,
// gpk_evaluate3, gpk_point_contract).  Plain C++, no device header: a stand-alone host program can
// include it (tests/test_evaluate_host.py builds one with the address and undefined sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>

// gpk_evaluate / gpk_evaluate3 walk their points in chunks of at most this many (bounded scratch:
// five chunk x P2 blocks on two axes, three chunk x P2 x P3 tensors on three)
constexpr int EVAL_CHUNK = 4096, EVAL_CHUNK3 = 1024;
// ... and on three axes of at most EVAL_TENSOR_CAP / (P2 P3) points, a multiple of 32 and at least
// 32, so that one chunk x P2 x P3 tensor stays within 2 GiB on the largest grids
constexpr size_t EVAL_TENSOR_CAP = (size_t)1 << 28;  // doubles

inline int eval3_chunk(size_t slab /* P2 * P3 */) {
  size_t c = EVAL_TENSOR_CAP / (slab ? slab : 1) / 32 * 32;
  if (c < 32) c = 32;
  return c > (size_t)EVAL_CHUNK3 ? EVAL_CHUNK3 : (int)c;
}

// chunk k of m points in chunks of `chunk`: its first point and its size (0 past the end)
inline int64_t chunk_begin(int64_t k, int chunk) { return k * (int64_t)chunk; }
inline int chunk_size(int64_t m, int64_t k, int chunk) {
  const int64_t left = m - chunk_begin(k, chunk);
  return left <= 0 ? 0 : left < chunk ? (int)left : chunk;
}
inline int64_t chunk_count(int64_t m, int chunk) { return (m + chunk - 1) / chunk; }

// doubles of T that out[p][c] = sum_j f * T[p sp + j sj + c sc] can touch (p < m, j < n, c < C):
// one past the largest index; 0 when a size is not positive or the extent overflows size_t / 8
inline size_t point_contract_extent(int64_t m, int64_t n, int64_t C, int64_t sp, int64_t sj, int64_t sc) {
  if (m < 1 || n < 1 || C < 1 || sp < 0 || sj < 1 || sc < 1) return 0;
  const unsigned __int128 last = (unsigned __int128)(m - 1) * sp + (unsigned __int128)(n - 1) * sj +
                                 (unsigned __int128)(C - 1) * sc;
  const unsigned __int128 cap = (unsigned __int128)1 << 60;
  return last >= cap ? 0 : (size_t)last + 1;
}
