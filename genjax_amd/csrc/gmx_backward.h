// Backward simulation over a sweep's history (include/genmi.h "Row-wise exact-integer draws"): ONE multinomial draw per
// row of a [rows, n] matrix of logits, each row through the two-level block-floating-point integer CDF of the
// resamplers (tiles of 1024 columns) and the exact 128-bit threshold of gmx_ancestors(GMX_RESAMPLE_MULTINOMIAL).
//   k_pick_stats   per (row, tile): m_b = max logit, A_b = sum floor(exp(x - k_b ln 2) * 2^shift)      (reads rows x n x 4 B once)
//   k_pick_row     one workgroup per row: M, K and the total from the row's tile statistics; the threshold from the row's
//                  key; the tile the threshold falls into (a scan of the scaled tile sums, 256 tiles per round); that
//                  tile's 1024 terms rebuilt in registers; the number of its columns whose CDF value is below the threshold
// No n-entry CDF array.  Everything after the per-element exp is integer arithmetic, so the index is the one
// gmx_weight_cdf + gmx_ancestors give for the row, whatever the grid.
// Under hipcc: the two kernels and the device pieces the whole row-wise family is put together from (gmx_resample_rows.h
// includes this file): pick_threshold, pick_group_offsets, rows_store4 and the three phases of the pick of a row of one tile
// (pick1_*), each stated once, at its definition; the four fixed-point weights of a thread are gmx_block.h's
// gmx_tile_fixed4.  Included by gmx_kernels.hip only (not among the headers embedded for hiprtc).  Under a
// plain host compiler: the two ENTRY POINTS, the draw as a sequential loop over rows calling gmx_weight_cdf and
// gmx_ancestors (both declared in genmi.h and exported by a CPU build of the C-ABI; gmx_vm.h includes this file there).
// That loop validates its arguments as the HIP entry point does and leaves its message (gmx_sizes.h: the checks, gmx_fail).
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "gmx_sizes.h"                 /* gmx_pick_rows_bytes_, gmx_pick_rows_shift_, gmx_pick_rows_refusal_ */

#define GMX_PICK_TILE GMX_TILE          /* one definition tile of the CDF */

#if defined(__HIPCC__)
#include "gmx_resample.h"              /* gmx_block.h, gmx_rng.h, u128 / mul64 */

#define GMX_PICK_BLOCK 256

// four consecutive logits of a row, columns base .. base + 3; columns >= n read as -inf (weight 0).  A row starts at
// any 4-byte boundary (ld is arbitrary): one 16-byte load where the address allows, four 4-byte loads otherwise.
__device__ __forceinline__ void pick_load4(const float* __restrict__ row, int64_t base, int64_t n, float x[4]) {
  if (base + 4 <= n && (((uintptr_t)(row + base)) & 15u) == 0u) {
    const float4 v = *reinterpret_cast<const float4*>(row + base);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = (base + c < n) ? row[base + c] : -gmx_inf();
  }
}

// sum of a u64 over the 256 threads, to every thread (every thread of the workgroup calls it)
__device__ __forceinline__ uint64_t pick_block_sum(uint64_t v, uint64_t* lds8) {
  v = wave_sum_u64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds8[threadIdx.x >> 6] = v;
  __syncthreads();
  return (lds8[0] + lds8[1]) + (lds8[2] + lds8[3]);
}

// ---- the pieces every row-wise draw is put together from (this file's kernels and gmx_resample_rows.h's).  None of them
// holds a barrier: a kernel calls them between its own. ----

// The multinomial slot's threshold: Thr = ceil(total (2^23 - u) / 2^23) for a 23-bit uniform u, k_ancestors_mn's integer
// form of cdf_i 2^23 >= total (2^23 - u).  In [1, total] (0 without mass).
__device__ __forceinline__ uint64_t pick_threshold(uint64_t total, uint64_t u) {
  const u128 P = mul64(total, (1ull << 23) - u);                 // >= 1 with mass
  const uint64_t plo = P.lo + ((1ull << 23) - 1ull);
  const uint64_t phi = P.hi + (plo < P.lo ? 1ull : 0ull);
  return (phi << 41) | (plo >> 23);                              // ceil(P / 2^23)
}
// ... of the row's key at counter j
__device__ __forceinline__ uint64_t pick_threshold(const uint32_t* __restrict__ keys, int64_t r, uint64_t j, uint64_t total) {
  gmx_key key; key.k0 = keys[2 * r]; key.k1 = keys[2 * r + 1];
  return pick_threshold(total, (uint64_t)(gmx_bits32(key, j) >> 9));
}

// A row held by waves grp * W .. grp * W + W - 1 of the workgroup, each wave's inclusive sum in s[wave]: the sum of the
// group's waves before `wave`, and the row's total
template <int W>
__device__ __forceinline__ void pick_group_offsets(const uint64_t* s, int grp, int wave, uint64_t& woff, uint64_t& total) {
  woff = 0; total = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const uint64_t v = s[grp * W + w];
    total += v;
    woff += (grp * W + w < wave) ? v : 0ull;
  }
}

// One 16-byte store of four consecutive elements base .. base + 3 of a row of n where the address allows, else four
// guarded stores
template <typename T> struct rows_quad;
template <> struct rows_quad<int32_t> { typedef int4 type; };
template <> struct rows_quad<float> { typedef float4 type; };
template <typename T>
__device__ __forceinline__ void rows_store4(T* row, int64_t base, int64_t n, const T v[4]) {
  if (base + 4 <= n && (((uintptr_t)(row + base)) & 15u) == 0u) {
    typename rows_quad<T>::type q4;
    q4.x = v[0]; q4.y = v[1]; q4.z = v[2]; q4.w = v[3];
    *reinterpret_cast<typename rows_quad<T>::type*>(row + base) = q4;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (base + c < n) row[base + c] = v[c];
  }
}

// ---- the pick of a row of ONE tile (n <= 1024) held W waves to the row, 4 / W rows to the workgroup, four columns to the
// thread: k_pick_row's answer with K = k_b and nothing below the tile, #{ i : cdf_i < Thr }, cdf_i the row's inclusive
// sum.  Three phases, one barrier of the caller's after each; LDS: s_max, s_scan and s_cnt, four words each. ----
// 1: the wave's maximum into s_max
__device__ __forceinline__ void pick1_put_max(const float x[4], float* s_max, int lane, int wave) {
  const float m = wave_max(gmx_rmax(gmx_rmax(x[0], x[1]), gmx_rmax(x[2], x[3])));
  if (lane == 0) s_max[wave] = m;
}
// 2: the row's maximum M, the fixed-point weights against its reference, their wave scan (returned) into s_scan
template <int W>
__device__ __forceinline__ uint64_t pick1_put_scan(const float x[4], int64_t base, int64_t n, float scale, const float* s_max,
                                                   uint64_t* s_scan, int grp, int lane, int wave, float& M, uint64_t q[4],
                                                   uint64_t& run) {
  M = s_max[grp * W];
#pragma unroll
  for (int w = 1; w < W; ++w) M = gmx_rmax(M, s_max[grp * W + w]);
  const float ref = gmx_tile_ref(gmx_tile_exp(M));       // one tile: K = k_b, cdf_i = the tile-local inclusive sum
  run = gmx_tile_fixed4(x, base, n, false, ref, scale, q);
  const uint64_t inc = wave_scan_u64(run);
  if (lane == 63) s_scan[wave] = inc;
  return inc;
}
// 3: the row's total (returned), the threshold of keys[r] at counter 0, the wave's count of columns below it into s_cnt
template <int W>
__device__ __forceinline__ uint64_t pick1_put_count(const uint32_t* __restrict__ keys, int64_t r, int64_t base, int64_t n,
                                                    const uint64_t q[4], uint64_t run, uint64_t inc, const uint64_t* s_scan,
                                                    uint32_t* s_cnt, int grp, int lane, int wave) {
  uint64_t woff, total;
  pick_group_offsets<W>(s_scan, grp, wave, woff, total);
  const uint64_t loc = woff + (inc - run);
  const uint64_t Thr = pick_threshold(keys, r, 0ull, total);
  uint64_t lower = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) lower += (base + c < n && loc + q[c] < Thr) ? 1ull : 0ull;
  lower = wave_sum_u64(lower);
  if (lane == 0) s_cnt[wave] = (uint32_t)lower;
  return total;
}
// ... and after the third barrier: the column (a row without mass: the caller's business)
template <int W>
__device__ __forceinline__ uint32_t pick1_index(const uint32_t* s_cnt, int grp, int64_t n) {
  uint32_t cnt = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) cnt += s_cnt[grp * W + w];
  return cnt < (uint32_t)n ? cnt : (uint32_t)n - 1u;
}

// blockIdx.x: the tile, blockIdx.y: the row (row0 + y).  k_tile_stats with a row stride; every offset is 64-bit.
__global__ void __launch_bounds__(GMX_PICK_BLOCK)
k_pick_stats(const float* __restrict__ logits, int64_t n, int64_t ld, int64_t n_tiles, int64_t row0, float scale,
             float* __restrict__ tmax, uint64_t* __restrict__ agg) {
  __shared__ float lds4[4];
  __shared__ uint64_t lds8[4];
  const int64_t r = row0 + (int64_t)blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * GMX_PICK_TILE + (int64_t)threadIdx.x * 4;
  float x[4];
  pick_load4(logits + r * ld, base, n, x);
  float m = gmx_rmax(gmx_rmax(x[0], x[1]), gmx_rmax(x[2], x[3]));
  m = block_max(m, lds4);
  uint64_t q[4];
  const uint64_t run = pick_block_sum(gmx_tile_fixed4(x, base, n, false, gmx_tile_ref(gmx_tile_exp(m)), scale, q), lds8);
  if (threadIdx.x == 0) {
    tmax[r * n_tiles + blockIdx.x] = m;
    agg[r * n_tiles + blockIdx.x] = run;
  }
}

// One workgroup per row.  cdf_i = below(tile of i) + ((tile-local inclusive sum) >> (K - k_b)), as k_weight_cdf writes
// it; the draw is the first i with cdf_i >= Thr (pick_threshold).  cdf is non-decreasing, so that i = #{ i : cdf_i < Thr }:
// the tiles whose inclusive prefix is below Thr are counted first, then the columns of the one tile that reaches it.
// Row r's answer, plus r * index_stride, goes to out[r * out_stride + out_offset] (gmx_pick_rows: 1, 0 and no stride;
// gmx_resample_rows_as: slot n - 1 of row r of the ancestor matrix).
__global__ void __launch_bounds__(GMX_PICK_BLOCK)
k_pick_row(const uint32_t* __restrict__ keys, const float* __restrict__ logits, int64_t n, int64_t ld, int64_t n_tiles,
           float scale, const float* __restrict__ tmax, const uint64_t* __restrict__ agg, int32_t* __restrict__ out,
           int64_t out_stride, int64_t out_offset, int64_t index_stride, unsigned long long* __restrict__ status) {
  __shared__ float lds4[4];
  __shared__ uint64_t lds8[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = (int64_t)blockIdx.x;
  const float* __restrict__ tm = tmax + r * n_tiles;
  const uint64_t* __restrict__ ta = agg + r * n_tiles;
  int32_t* __restrict__ dst = out + (r * out_stride + out_offset);
  const int32_t add = (int32_t)(r * index_stride);
  float M = -gmx_inf();
  for (int64_t t = tid; t < n_tiles; t += GMX_PICK_BLOCK) M = gmx_rmax(M, tm[t]);
  M = block_max(M, lds4);
  const int32_t K = gmx_tile_exp(M);
  uint64_t part = 0;
  for (int64_t t = tid; t < n_tiles; t += GMX_PICK_BLOCK) part += gmx_tile_scale(ta[t], gmx_tile_exp(tm[t]), K);   // (K - k_b may pass 63)
  const uint64_t total = pick_block_sum(part, lds8);
  if (total == 0ull) {                   // no mass at all: the last column, as gmx_ancestors answers, and counted
    if (tid == 0) { *dst = (int32_t)(n - 1) + add; atomicAdd(status, 1ull); }
    return;
  }
  const uint64_t Thr = pick_threshold(keys, r, 0ull, total);
  // ---- the tile: 256 tiles per round, the rounds chained by `carry` (uniform) ----
  uint64_t carry = 0, below = 0, cnt = 0;
  for (int64_t c0 = 0; c0 < n_tiles && carry < Thr; c0 += GMX_PICK_BLOCK) {
    const int64_t t = c0 + tid;
    const uint64_t G = t < n_tiles ? gmx_tile_scale(ta[t], gmx_tile_exp(tm[t]), K) : 0ull;
    const uint64_t inc = wave_scan_u64(G);
    __syncthreads();
    if (lane == 63) lds8[wave] = inc;
    __syncthreads();
    uint64_t woff, round;
    pick_group_offsets<4>(lds8, 0, wave, woff, round);
    if (t < n_tiles && carry + woff + inc < Thr) { cnt += 1ull; below += G; }
    carry += round;
  }
  cnt = pick_block_sum(cnt, lds8);
  below = pick_block_sum(below, lds8);
  int64_t b = (int64_t)cnt;              // < n_tiles: the last inclusive prefix is total >= Thr
  if (b > n_tiles - 1) b = n_tiles - 1;
  // ---- that tile's 1024 terms, rebuilt in registers ----
  const int32_t k_b = gmx_tile_exp(tm[b]);
  const int64_t base = b * GMX_PICK_TILE + (int64_t)tid * 4;
  float x[4];
  pick_load4(logits + r * ld, base, n, x);
  uint64_t q[4];
  const uint64_t run = gmx_tile_fixed4(x, base, n, false, gmx_tile_ref(k_b), scale, q);
  const uint64_t inc = wave_scan_u64(run);
  __syncthreads();
  if (lane == 63) lds8[wave] = inc;
  __syncthreads();
  uint64_t woff, tile_sum;
  pick_group_offsets<4>(lds8, 0, wave, woff, tile_sum);
  const uint64_t loc = woff + (inc - run);
  uint64_t lower = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    lower += (base + c < n && below + gmx_tile_scale(loc + q[c], k_b, K) < Thr) ? 1ull : 0ull;
  lower = pick_block_sum(lower, lds8);
  if (tid == 0) {
    int64_t i = b * GMX_PICK_TILE + (int64_t)lower;
    if (i > n - 1) i = n - 1;
    *dst = (int32_t)i + add;
  }
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)
#include <vector>
#include "genmi.h"
#include "gmx_math.h"
// (`used`: emitted, and so exported by a shared library, although nothing in the translation unit calls them)

extern "C" __attribute__((used)) inline size_t gmx_pick_rows_workspace(int64_t rows, int64_t n) { return gmx_pick_rows_bytes_(rows, n); }

extern "C" __attribute__((used)) inline int gmx_pick_rows(const uint32_t* keys_d, const float* logits_d, int64_t rows, int64_t n, int64_t ld,
                                    int32_t* out_d, int64_t* status_d, void* workspace_d, gmx_stream stream) {
  const gmx_refusal no = gmx_pick_rows_refusal_(!keys_d || !logits_d || !out_d || !status_d || !workspace_d, rows, n, ld);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_pick_rows", no.v);
  const int shift = gmx_pick_rows_shift_(n);
  std::vector<uint64_t> cdf((size_t)n);
  std::vector<float> row((size_t)n);                             // (gmx_weight_cdf may ask for an aligned row)
  for (int64_t r = 0; r < rows; ++r) {
    const float* src = logits_d + r * ld;
    float M = -gmx_inf();
    for (int64_t i = 0; i < n; ++i) { row[(size_t)i] = src[i]; M = gmx_rmax(M, src[i]); }
    uint64_t total = 0;
    if (gmx_weight_cdf(row.data(), n, shift, nullptr, 0, &M, cdf.data(), &total, workspace_d, stream)) return 1;
    if (gmx_ancestors(GMX_RESAMPLE_MULTINOMIAL, keys_d + 2 * r, cdf.data(), n, 0, &total, 1, 0, 1, out_d + r, stream)) return 1;
    if (total == 0) status_d[0] += 1;
  }
  return 0;
}
#endif
