// Weighted quantiles of many independent rows (include/genmi.h "Row-wise weighted quantiles": gmx_rows_quantiles): per row r
// of a [rows, n] matrix of log-weights (plus, optionally, `carry` — ONE float32 add, as in gmx_rows_moments) and a
// struct-of-arrays [D, x_ld] state store addressed as gmx_rows_moments addresses it, with q_i the row's fixed-point weights
// (the increments of gmx_weight_cdf of the row alone: one tile, shift = 62 - ceil(log2 n)), total = sum q_i and, per level,
// T = max(1, ceil(level_q32 total / 2^32)):
//     out[r, d, j] = the state word x of component d with the smallest key(x) such that sum { q_i : key(x_i) <= key(x) } >= T
// key: the monotone map of a float's bits (gmx_qnt_key), a total order on bit patterns.  Everything after the per-column
// exp is integer arithmetic and the order is total, so the device, the mirror and a reference in Python integers agree bit
// for bit.  A row without mass writes NaN.  Nothing is written into the inputs.
//   n <= 1024   k_rows_quantiles_small<W>: ONE launch, no workspace.  The packing of rows_small_body / k_rows_moments_small:
//               a thread holds 4 consecutive columns (one 16-byte load), a row takes W = 1, 2 or 4 waves, a 256-thread
//               workgroup holds 4 / W rows; a group past the last row redoes the last row and writes nothing.
//     weights, once per row   the weight, carry and first component loads leave before the first wait; the maximum and the
//               fixed-point weights are mom_row_max and gmx_tile_fixed4 (what pick1_put_scan calls); a thread's four q are
//               parked in LDS BY COLUMN (s_q: 8 bytes x 1024 columns per workgroup at every W); the Q thresholds are
//               computed once per row by Q threads of its group and parked too.  Three barriers.
//     sort, once per component   a bitonic network over the 256 W words (key << 32 | column) of the row: the column makes
//               ties strict, so the network is deterministic; columns >= n carry the largest key and weigh 0.  Element
//               distances 1 and 2 are compare-exchanges between a thread's own four registers; distances 4 .. 128 are lane
//               xor 1 .. 32 inside the wave (DPP quad permutes for 1 and 2, __shfl_xor for 4, 8, 16, v_permlane32_swap for
//               32); only distances >= 256 go through LDS with a barrier: none for W = 1 — a row of <= 256 particles sorts
//               inside one wave — one step for W = 2, three for W = 4.  The exchange buffer is doubled (2 x 8 KB) and the
//               steps alternate between the halves, so a step needs ONE barrier: the barrier of step s + 1 stands between
//               the reads of step s and the writes of step s + 2.  Component d + 1 is loaded before component d is sorted.
//     select   a thread gathers the weights of its four sorted positions from s_q by column, scans them (wave_scan_u64 and,
//               W > 1, pick_group_offsets<W> behind one barrier, its four words doubled like the exchange buffer); for each
//               level the ONE thread whose positions hold the crossing C_{k-1} < T <= C_k stores the word.
//     Barriers per launch: 3 + D (steps + 1) with steps = 0, 1, 3 for W = 1, 2, 4 and no select barrier for W = 1.  LDS:
//               8 KB of weights, 16 KB of exchange for W > 1, 0.7 KB of thresholds and scan words.  No float arithmetic
//               after the weights; the one float add is written as the instruction (mom_add); vector stores only.
//   n > 1024    refused: a quantile past one tile needs the two-level block-floating-point weights and a selection across
//               tiles (gmx_sizes.h, gmx_rows_quantiles_refusal_).
// Under hipcc: the kernel, included by gmx_kernels.hip only (not among the headers embedded for hiprtc).  Under a plain
// host compiler: the ENTRY POINT as the definition written literally — a sequential loop over rows: sort (key, column)
// pairs, cumulate in uint64 — with the same refusals (gmx_sizes.h); gmx_vm.h includes this file there.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "gmx_moments.h"               /* gmx_math.h; hipcc: gmx_backward.h, mom_row_max; the mirror: gmx_mom_row_ */

// the order: bits ^ 0x80000000 for a non-negative float, ~bits for a negative one (-NaN first, -0 < +0, +NaN last)
GMX_HD uint32_t gmx_qnt_key(uint32_t bits) { return (bits >> 31) ? ~bits : (bits ^ 0x80000000u); }
GMX_HD uint32_t gmx_qnt_bits(uint32_t key) { return (key >> 31) ? (key ^ 0x80000000u) : ~key; }
#define GMX_QNT_ONE (1ull << 32)       /* the level of probability 1 */

#if defined(__HIPCC__)

#define GMX_QNT_BLOCK 256
static_assert(GMX_ROWS_QUANTILES_MAX_Q <= 64, "the thresholds of a row are computed by the first Q threads of its group");
static_assert(GMX_PICK_TILE == 4 * GMX_QNT_BLOCK && GMX_PICK_TILE <= 1024, "a column is the low 10 bits of a sort word");

// T = max(1, ceil(level total / 2^32)), level <= 2^32: in [1, total] with mass
__device__ __forceinline__ uint64_t qnt_threshold(uint64_t level, uint64_t total) {
  const u128 P = mul64(level, total);                            // below 2^94
  const uint64_t plo = P.lo + (GMX_QNT_ONE - 1ull);
  const uint64_t phi = P.hi + (plo < P.lo ? 1ull : 0ull);
  const uint64_t T = (phi << 32) | (plo >> 32);
  return T > 0ull ? T : 1ull;
}
// lane l receives lane (l xor M)'s word, M = 1 .. 32
template <int M>
__device__ __forceinline__ uint64_t qnt_lane_xor_c(uint64_t v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  if (M == 1) {                                                  // quad_perm [1, 0, 3, 2]
    lo = gmx_dpp<0xB1, 0xf>(lo, lo);
    hi = gmx_dpp<0xB1, 0xf>(hi, hi);
  } else if (M == 2) {                                           // quad_perm [2, 3, 0, 1]
    lo = gmx_dpp<0x4E, 0xf>(lo, lo);
    hi = gmx_dpp<0x4E, 0xf>(hi, hi);
  } else if (M == 32) {                // (v, v) swapped: in every lane one result is the lane's own word, the other lane
    const auto slo = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);       // (l xor 32)'s: own ^ other ^ own
    const auto shi = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    lo = (uint32_t)slo[0] ^ (uint32_t)slo[1] ^ lo;
    hi = (uint32_t)shi[0] ^ (uint32_t)shi[1] ^ hi;
  } else {
    lo = (uint32_t)__shfl_xor((int)lo, M, GMX_WAVE);
    hi = (uint32_t)__shfl_xor((int)hi, M, GMX_WAVE);
  }
  return ((uint64_t)hi << 32) | lo;
}
// ... for an m the unrolled network knows at compile time
__device__ __forceinline__ uint64_t qnt_lane_xor(uint64_t v, int m) {
  switch (m) {
    case 1: return qnt_lane_xor_c<1>(v);
    case 2: return qnt_lane_xor_c<2>(v);
    case 4: return qnt_lane_xor_c<4>(v);
    case 8: return qnt_lane_xor_c<8>(v);
    case 16: return qnt_lane_xor_c<16>(v);
    default: return qnt_lane_xor_c<32>(v);
  }
}
// the compare-exchange of the network on the side that holds `mine`: the smaller word when keep_min (words are distinct)
__device__ __forceinline__ uint64_t qnt_keep(uint64_t mine, uint64_t other, bool keep_min) {
  return ((mine < other) == keep_min) ? mine : other;
}

// The bitonic network over the N = 256 W words of a row, ascending: thread gt of the row's group holds elements 4 gt ..
// 4 gt + 3 in v[0 .. 3].  Stage k, distance j: element e meets e xor j, and the pair is put in ascending order iff
// (e & k) == 0 — for k >= 4 a property of the thread, (gt & (k / 4)) == 0, and always true in the last stage.  W > 1: every
// thread of the workgroup calls it (a barrier per step of distance >= 256); `flip`: the half of s_x the next such step
// writes, carried from call to call.
template <int W>
__device__ __forceinline__ void qnt_sort(uint64_t v[4], int tid, int gt, int lane, uint64_t* s_x, int& flip) {
  constexpr int N = 256 * W;
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
    const bool asc_t = (gt & (k >> 2)) == 0;                     // (k >= 4)
#pragma unroll
    for (int j = k >> 1; j >= 1; j >>= 1) {
      if (W > 1 && j >= 256) {                                   // another wave of the group: through LDS
        const int m = j >> 2;
        uint64_t* buf = s_x + flip * GMX_PICK_TILE;
#pragma unroll
        for (int c = 0; c < 4; ++c) buf[tid * 4 + c] = v[c];
        __syncthreads();
        const bool keep_min = ((gt & m) == 0) == asc_t;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = qnt_keep(v[c], buf[(tid ^ m) * 4 + c], keep_min);
        flip ^= 1;
      } else if (j >= 4) {                                       // another lane of the wave
        const bool keep_min = ((lane & (j >> 2)) == 0) == asc_t;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = qnt_keep(v[c], qnt_lane_xor(v[c], j >> 2), keep_min);
      } else {                                                   // the thread's own registers
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if ((c & j) != 0) continue;
          const bool asc = k == 2 ? (c & 2) == 0 : asc_t;
          const uint64_t a = v[c], b = v[c | j];
          const bool swap = (a > b) == asc;
          v[c] = swap ? b : a;
          v[c | j] = swap ? a : b;
        }
      }
    }
  }
}

// n <= 1024: W waves per row, 4 / W rows per workgroup; thread gt of a row's group holds columns 4 gt .. 4 gt + 3, and after
// a sort the sorted positions 4 gt .. 4 gt + 3.  Every thread reaches every barrier (the header counts them).
template <int W>
__global__ void __launch_bounds__(GMX_QNT_BLOCK)
k_rows_quantiles_small(const float* __restrict__ lw, const float* __restrict__ carry, int64_t rows, int64_t n, int64_t ld,
                       const float* __restrict__ x, int32_t D, int64_t x_ld, int64_t x_row_stride,
                       const uint64_t* __restrict__ level, int32_t Q, float scale, float* __restrict__ out, int64_t out_ld) {
  static_assert(W == 1 || W == 2 || W == 4, "waves per row");
  constexpr int RPW = 4 / W, GT = 64 * W;
  __shared__ float s_max[4];
  __shared__ uint64_t s_scan[4];
  __shared__ uint64_t s_sel[2][4];
  __shared__ uint64_t s_thr[4][GMX_ROWS_QUANTILES_MAX_Q];
  __shared__ uint64_t s_q[GMX_PICK_TILE];
  __shared__ uint64_t s_x[W > 1 ? 2 * GMX_PICK_TILE : 1];                  // (W = 1: no exchange through LDS)
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = tid / GT, gt = tid % GT;
  const int64_t r_ = (int64_t)blockIdx.x * RPW + grp;
  const bool live = r_ < rows;
  const int64_t r = live ? r_ : rows - 1;
  const int64_t base = (int64_t)gt * 4;
  const float* __restrict__ xrow = x + r * x_row_stride;
  float a[4], cy[4], xn[4];
  pick_load4(lw + r * ld, base, n, a);
  if (carry != nullptr) pick_load4(carry + r * ld, base, n, cy);       // (every load below is out before the first wait)
  pick_load4(xrow, base, n, xn);
  // ---- the row's fixed-point weights, parked by column; its thresholds ----
  const float M = mom_row_max<W>(a, cy, carry != nullptr, s_max, grp, lane, wave);
  uint64_t* qrow = s_q + grp * (GT * 4);
  {
    uint64_t q[4];
    const uint64_t run = gmx_tile_fixed4(a, base, n, false, gmx_tile_ref(gmx_tile_exp(M)), scale, q);
    qrow[base] = q[0];
#pragma unroll
    for (int c = 1; c < 4; ++c) qrow[base + c] = q[c] - q[c - 1];
    const uint64_t wsum = wave_sum_u64(run);
    if (lane == 0) s_scan[wave] = wsum;
  }
  __syncthreads();
  uint64_t total = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) total += s_scan[grp * W + w];
  if (gt < Q) {
    const uint64_t lv = level[gt];
    s_thr[grp][gt] = qnt_threshold(lv < GMX_QNT_ONE ? lv : GMX_QNT_ONE, total);
  }
  __syncthreads();
  // ---- per component: sort, then select ----
  uint32_t* __restrict__ orow = reinterpret_cast<uint32_t*>(out) + r * out_ld;
  int flip = 0;
  for (int32_t d = 0; d < D; ++d) {
    uint64_t v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t key = (base + c < n) ? gmx_qnt_key(gmx_f2u(xn[c])) : 0xffffffffu;
      v[c] = ((uint64_t)key << 32) | (uint64_t)(uint32_t)(base + c);
    }
    if (d + 1 < D) pick_load4(xrow + (int64_t)(d + 1) * x_ld, base, n, xn);      // (out before this component's sort)
    qnt_sort<W>(v, tid, gt, lane, s_x, flip);
    uint64_t w[4], run = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      w[c] = qrow[(uint32_t)v[c] & (uint32_t)(GMX_PICK_TILE - 1)];
      run += w[c];
    }
    const uint64_t inc = wave_scan_u64(run);
    uint64_t woff = 0;
    if (W > 1) {
      uint64_t all;
      if (lane == 63) s_sel[d & 1][wave] = inc;
      __syncthreads();
      pick_group_offsets<W>(s_sel[d & 1], grp, wave, woff, all);
    }
    const uint64_t lo = woff + (inc - run);                      // the mass before the thread's four positions
    if (!live) continue;
    uint32_t* __restrict__ dst = orow + (int64_t)d * Q;
    if (total == 0ull) {                                         // no mass: NaN for every level
      if (gt < Q) dst[gt] = GMX_NAN_BITS;
      continue;
    }
    for (int32_t j = 0; j < Q; ++j) {
      const uint64_t T = s_thr[grp][j];
      if (!(lo < T && T <= lo + run)) continue;                  // exactly one thread of the group passes
      uint64_t C = lo;
      uint32_t word = 0;
      bool found = false;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        C += w[c];
        const bool here = !found && T <= C;
        word = here ? gmx_qnt_bits((uint32_t)(v[c] >> 32)) : word;
        found = found || here;
      }
      dst[j] = word;
    }
  }
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)
#include <algorithm>
#include <vector>
#include "genmi.h"
#include "gmx_sizes.h"
// (`used`: emitted, and so exported by a shared library, although nothing in the translation unit calls it)

// the definition, literally: the row's weights, then per component the (key, column) pairs sorted and cumulated
extern "C" __attribute__((used)) inline int gmx_rows_quantiles(const float* lw_d, const float* carry_d, int64_t rows, int64_t n, int64_t ld,
                                                            const float* x_d, int32_t D, int64_t x_ld, int64_t x_row_stride,
                                                            const uint64_t* level_q32_d, int32_t Q, float* out_d, int64_t out_ld,
                                                            gmx_stream stream) {
  (void)stream;
  const gmx_refusal no = gmx_rows_quantiles_refusal_(!lw_d || !x_d || !level_q32_d || !out_d, rows, n, ld, D, x_ld, x_row_stride, Q,
                                                     out_ld, level_q32_d);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_rows_quantiles", no.v);
  const int shift = gmx_pick_rows_shift_(n);
  std::vector<float> a((size_t)n);
  std::vector<uint64_t> q((size_t)n), word((size_t)n), T((size_t)Q);
  uint32_t* out = reinterpret_cast<uint32_t*>(out_d);
  for (int64_t r = 0; r < rows; ++r) {
    const float M = gmx_mom_row_(lw_d + r * ld, carry_d ? carry_d + r * ld : nullptr, n, a.data());
    const float ref = gmx_tile_ref(gmx_tile_exp(M));             // one tile: the row's reference is the tile's
    uint64_t total = 0;
    for (int64_t i = 0; i < n; ++i) total += q[(size_t)i] = gmx_exp_fixed(a[(size_t)i] - ref, shift);
    for (int32_t j = 0; j < Q; ++j) {
      const unsigned __int128 P = (unsigned __int128)level_q32_d[j] * total + (GMX_QNT_ONE - 1);
      T[(size_t)j] = std::max<uint64_t>((uint64_t)(P >> 32), 1);
    }
    for (int32_t d = 0; d < D; ++d) {
      const float* xs = x_d + (int64_t)d * x_ld + r * x_row_stride;
      for (int64_t i = 0; i < n; ++i) {
        uint32_t bits;
        __builtin_memcpy(&bits, xs + i, 4);
        word[(size_t)i] = ((uint64_t)gmx_qnt_key(bits) << 32) | (uint64_t)i;
      }
      std::sort(word.begin(), word.end());
      for (int32_t j = 0; j < Q; ++j) {
        uint32_t res = GMX_NAN_BITS;                             // (a row without mass)
        uint64_t C = 0;
        for (int64_t k = 0; k < n && total != 0; ++k) {
          C += q[(size_t)(word[(size_t)k] & 0xffffffffull)];
          if (C >= T[(size_t)j]) { res = gmx_qnt_bits((uint32_t)(word[(size_t)k] >> 32)); break; }
        }
        out[r * out_ld + (int64_t)d * Q + j] = res;
      }
    }
  }
  return 0;
}
#endif
