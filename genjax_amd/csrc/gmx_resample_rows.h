// Resampling of many independent rows (include/genmi.h "Row-wise exact-integer draws": gmx_resample_rows): row r of a
// [rows, n] matrix of log-weights is resampled under keys[r] exactly as gmx_resample resamples it alone — the two-level
// block-floating-point integer CDF over tiles of 1024 columns OF THE ROW, shift = 62 - ceil(log2 n), 23-bit uniforms, 128-bit
// comparisons.  Everything after the per-element exp is integer arithmetic and every slot is decided by the DEFINITION
// (the first column whose CDF value passes the slot's threshold: a binary search over the tile's CDF in LDS), so the
// ancestors do not depend on the grid or on the form.
//   n <= 1024   k_rows_small<kind, W>: ONE launch, no workspace traffic.  A row is one CDF tile: its maximum, its weights,
//               their scan and the slot searches stay in registers / LDS.  PACKING: a thread holds 4 consecutive columns
//               (one 16-byte load), so a row takes W = 1, 2 or 4 waves (n <= 256, <= 512, <= 1024) and a 256-thread
//               workgroup holds 4 / W rows: four rows of up to 256 columns, two of up to 512, one of up to 1024.
//   n > 1024    k_pick_stats (gmx_backward.h) per (row, tile), then k_rows_tile<kind>, one workgroup per (row, tile): the
//               row's tile prefixes, total and (M, K) from its <= 2048 tile statistics (gmx_tile_prefix_block, into LDS),
//               the tile's 1024 CDF values rebuilt into LDS, and — systematic / stratified — the slots the tile owns,
//               [f(prefix_b), f(prefix_b + G_b)), f(c) = #{ j : P_j < c D }, searched in that LDS tile.  No CDF array.
//   iid multinomial past one tile: a slot's threshold falls anywhere in the row, so k_rows_tile writes the row's CDF into
//               the workspace ([rows, n] u64) and k_rows_mn searches it per slot (a third launch).
//   pinned (gmx_resample_rows_pinned, conditional SMC): the iid multinomial with column n - 1 of every row replaced by a
//               retained particle's weight (written back), its D state words written into the caller's store, and slot
//               n - 1 answering n - 1.  n <= 1024: k_rows_small_pinned<W>, the same body with the pin compiled in — still
//               ONE launch; n > 1024: k_rows_pin writes the pins first, then the chain above with k_rows_mn<true>.
//   pins alone (gmx_rows_pin): k_rows_pin, which can also broadcast a second [D, rows] state over every particle of its
//               row (ancestor sampling: the NEXT retained state as a per-particle leaf).
//   ancestor sampling (gmx_resample_rows_as): the iid multinomial, then slot n - 1 of every row re-drawn from a second matrix
//               of logits as gmx_pick_rows draws it.  n <= 1024: k_rows_small_as<W>, the same body with that draw compiled
//               in — still ONE launch, no barrier added; n > 1024: the chain above, then k_pick_stats and k_pick_row
//               (gmx_backward.h) on the second matrix, k_pick_row writing slot n - 1 of the row.
//   adaptive (gmx_resample_rows_ess, n <= 1024 only): a second matrix `carry` is added to the weights (one float32 add,
//               written back), and the row is resampled only when the effective sample size of its fixed-point weights is
//               below ess_q8 / 256 — an exact integer predicate; a row that is not keeps its accumulated weights in
//               `carry` and gets identity ancestors.  k_rows_small_ess<kind, W>, the same body with the decision compiled in:
//               still ONE launch, no barrier added.
//   pick and take (gmx_pick_rows_take, backward simulation): gmx_pick_rows' one draw per row, then the picked particle's
//               weight and D state words taken, and the state broadcast over every particle of the row for the next step's
//               densities.  n <= 1024: k_rows_small_take<W>, the packing above around the draw alone — ONE launch, three
//               barriers, 64 bytes of LDS, no CDF tile; n > 1024: k_pick_stats and k_pick_row (gmx_backward.h) writing the
//               offset index, then k_rows_take, the gather and the broadcast in k_rows_pin's shape.
// Under hipcc: the kernels, included by gmx_kernels.hip only (not among the headers embedded for hiprtc).  Under a plain
// host compiler: the ENTRY POINTS as a sequential loop over rows calling the per-row path (gmx_resample; for the iid
// multinomial gmx_weight_cdf + gmx_ancestors, which is what gmx_resample does with that kind), as gmx_backward.h does
// for gmx_pick_rows; gmx_vm.h includes this file there.  That loop validates its arguments as the HIP entry point does
// and leaves its message (gmx_sizes.h: the checks, gmx_fail).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "gmx_backward.h"              /* gmx_sizes.h, GMX_PICK_TILE; under hipcc k_pick_stats, pick_load4 */

// (workspace size, refusals, GMX_ROWS_MAX_N, GMX_ROWS_PIN_MAX_D: gmx_sizes.h)

#if defined(__HIPCC__)
#include "gmx_resample.h"              /* gmx_block.h, gmx_rng.h, u128 / mul64 / slot_threshold */

#define GMX_ROWS_BLOCK 256

// Slot j's ancestor inside ONE ascending run of CDF values cdf[0 .. cnt): the first i whose value passes the slot's
// threshold, cnt when none does.  systematic / stratified: cdf_i D > P_j = (j 2^23 + u_j) total, D = n 2^23 (k_offspring's
// predicate); multinomial: cdf_i >= pick_threshold(total, u_j) (gmx_backward.h).  total >= 1.
template <int KIND>
__device__ __forceinline__ int32_t rows_slot_search(const uint64_t* cdf, int32_t cnt, gmx_key key, uint64_t u0, int64_t j,
                                                    uint64_t total, uint64_t D) {
  int32_t lo = 0, hi = cnt;
  if (KIND == GMX_RESAMPLE_MULTINOMIAL) {
    const uint64_t Thr = pick_threshold(total, (uint64_t)(gmx_bits32(key, (uint64_t)j) >> 9));
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (cdf[mid] >= Thr) hi = mid; else lo = mid + 1;
    }
  } else {
    const u128 P = slot_threshold(KIND, key, u0, j, total);
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (gt128(mul64(cdf[mid], D), P)) hi = mid; else lo = mid + 1;
    }
  }
  return lo;
}

// f(c) = #{ j in [0, n) : P_j < c D } for the ordered kinds (P_j increases with j): the exact predicate, bisected
template <int KIND>
__device__ __forceinline__ int64_t rows_slots_below(gmx_key key, uint64_t u0, uint64_t c, uint64_t D, uint64_t total, int64_t n) {
  const u128 X = mul64(c, D);
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (gt128(X, slot_threshold(KIND, key, u0, mid, total))) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// (four ancestors or four floats of consecutive slots of a row: rows_store4, gmx_backward.h)

// What gmx_resample_rows_pinned adds to a row (conditional SMC: slot n - 1 of every row is the retained particle)
struct rows_pin {
  const float* lw;      // [rows]: row r's column n - 1 takes lw[r] (written back into the matrix)
  const float* x;       // [D, rows]: ... and its D state words, into
  float* x_out;         //   x_out[d * x_ld + r * x_row_stride + n - 1]
  int32_t D;
  int64_t x_ld, x_row_stride;
};
// What gmx_resample_rows_as adds to a row (ancestor sampling: slot n - 1 of every row is one draw from a second matrix)
struct rows_as {
  const uint32_t* keys;          // [rows, 2]: row r's draw is under keys[r], counter 0
  const float* lw;               // the ancestor logits, rows ld elements apart
  int64_t ld;
  unsigned long long* status;    // counts the rows whose ancestor logits carry no mass
};
// What gmx_resample_rows_ess adds to a row (adaptive resampling: the row is resampled only when its ESS is low)
struct rows_ess {
  float* carry;                  // the log-weights carried since the row's last resampling: the matrix's layout, rows ld apart
  uint32_t ess_q8;               // resample iff ESS < ess_q8 / 256
  int32_t* resampled;            // [rows]: the decision
};
// sum of squares of the truncated weights as (hi, lo) += v^2 split at bit 32; V2 = (hi << 32) + lo, every part exact in u64
__device__ __forceinline__ u128 rows_ess_v2(uint64_t hi, uint64_t lo) {
  u128 r;
  r.lo = (hi << 32) + lo;
  r.hi = (hi >> 32) + (r.lo < lo ? 1ull : 0ull);
  return r;
}
// a row of the matrix as the kernel reads it: nothing else writes it — unless the kernel itself writes into it
template <bool PIN> struct rows_row_ptr { typedef const float* __restrict__ type; };
template <> struct rows_row_ptr<true> { typedef const float* type; };

// n <= 1024: W waves per row, 4 / W rows per workgroup; thread gt of a row's group holds columns (and slots) 4 gt .. 4 gt + 3.
// Every thread reaches every barrier (a group past the last row works on the last row again and writes nothing).
// PIN (the iid multinomial only): the thread that holds column n - 1 takes the pinned weight into its registers before the
// row's maximum is reduced, writes it back into the matrix and answers n - 1 for slot n - 1 whatever the search found; the
// row's group writes the D pinned state words.  No barrier and no LDS of its own; without PIN nothing of it is compiled.
// AS (the iid multinomial only, never with PIN): the row's group also holds the row's four-per-thread ancestor logits
// (loaded with the weights: one wait) and runs the three phases of the one-tile pick (pick1_*, gmx_backward.h) on them
// beside the weights' — the same three barriers; the thread that holds slot n - 1 stores that pick instead of its search.
// 64 bytes of LDS of its own; without AS nothing of it is compiled.
// ESS (any kind, never with PIN or AS): the row's group also loads the row of `carry` (with the weights: one wait), adds it
// — x = lw + carry, ONE float32 add, written back into the matrix — and everything above runs on x.  Each thread truncates
// its four fixed-point weights to v = w >> (shift - 30) (at most 2^30) and sums v, and v^2 in two halves split at bit 32;
// the three wave sums go to LDS packed in two words beside s_scan, before the barrier that follows it.  After that barrier
// every thread of the group holds V1 = sum v and V2 = sum v^2 exactly and evaluates V1^2 * 256 < ess_q8 * V2 in 128 bits
// (V1^2 <= 2^80, ess_q8 V2 < 2^102).  A resampled row: the searches as always, carry = 0.  Any other: no search, identity
// ancestors, carry = x.  No barrier and 64 bytes of LDS of its own; without ESS nothing of it is compiled.
template <int KIND, int W, bool PIN, bool AS = false, bool ESS = false>
__device__ __forceinline__ void rows_small_body(const uint32_t* __restrict__ keys, typename rows_row_ptr<PIN || ESS>::type lw,
                                                int64_t rows, int64_t n, int64_t ld, int64_t index_stride, float scale,
                                                float* __restrict__ max_out, uint64_t* __restrict__ total_out,
                                                int32_t* __restrict__ anc, unsigned long long* __restrict__ status,
                                                const rows_pin& pin, const rows_as& as = rows_as{},
                                                const rows_ess& ess = rows_ess{}) {
  static_assert(W == 1 || W == 2 || W == 4, "waves per row");
  static_assert(!PIN || KIND == GMX_RESAMPLE_MULTINOMIAL, "forcing a slot is a conditional draw under iid slots only");
  static_assert(!AS || (KIND == GMX_RESAMPLE_MULTINOMIAL && !PIN), "re-drawing a slot: iid slots only; the pin is in the matrix");
  static_assert(!ESS || (!PIN && !AS), "the adaptive form is the plain resampler's");
  constexpr int RPW = 4 / W, GT = 64 * W;
  __shared__ float s_max[4];
  __shared__ uint64_t s_scan[4];
  __shared__ uint64_t s_cdf[GMX_PICK_TILE];
  __shared__ float s_amax[AS ? 4 : 1];                   // (AS only: unused arrays take no LDS)
  __shared__ uint64_t s_ascan[AS ? 4 : 1];
  __shared__ uint32_t s_acnt[AS ? 4 : 1];
  __shared__ uint64_t s_ess[ESS ? 8 : 1];                // (ESS only) per wave: V2's low word | V2's high byte + V1 << 8
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = tid / GT, gt = tid % GT;
  const int64_t r_ = (int64_t)blockIdx.x * RPW + grp;
  const bool live = r_ < rows;
  const int64_t r = live ? r_ : rows - 1;
  typename rows_row_ptr<PIN || ESS>::type row = lw + r * ld;
  const int64_t base = (int64_t)gt * 4;
  float x[4];
  float p = 0.0f;
  float px = 0.0f;
  if (PIN) {                                             // (issued ahead of the row's load: one wait for all of them)
    p = pin.lw[r];
    if (live && gt < pin.D) px = pin.x[(int64_t)gt * rows + r];
  }
  pick_load4(row, base, n, x);
  float a[4];
  if (AS) pick_load4(as.lw + r * as.ld, base, n, a);     // (both matrices' loads are out before the first wait)
  if (ESS) {                                             // (likewise) x = lw + carry, written back
    float cy[4];
    pick_load4(ess.carry + r * ld, base, n, cy);
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = x[c] + cy[c];
    if (live) rows_store4(const_cast<float*>(lw) + r * ld, base, n, x);
  }
  if (PIN && live) {                                     // the D state words, by the row's thread group
    const int64_t at = r * pin.x_row_stride + n - 1;
    if (gt < pin.D) pin.x_out[(int64_t)gt * pin.x_ld + at] = px;
    for (int32_t d = gt + GT; d < pin.D; d += GT) pin.x_out[(int64_t)d * pin.x_ld + at] = pin.x[(int64_t)d * rows + r];
  }
  if (PIN && base <= n - 1 && n - 1 < base + 4) {        // the one thread of the group that holds column n - 1
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (base + c == n - 1) x[c] = p;
    if (live) const_cast<float*>(lw)[r * ld + n - 1] = p;
  }
  pick1_put_max(x, s_max, lane, wave);
  if (AS) pick1_put_max(a, s_amax, lane, wave);
  __syncthreads();
  float M;
  uint64_t q[4], run;
  const uint64_t inc = pick1_put_scan<W>(x, base, n, scale, s_max, s_scan, grp, lane, wave, M, q, run);
  if (ESS) {                                             // v = w >> (shift - 30); sum v, sum v^2 (its halves apart), per wave
    const int down = (int)(gmx_f2u(scale) >> 23) - 127 - 30;
    uint64_t v1 = 0, lo2 = 0, hi2 = 0, prev = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint64_t v = (q[c] - prev) >> down;
      prev = q[c];
      const uint64_t sq = v * v;
      v1 += v;
      lo2 += sq & 0xffffffffull;
      hi2 += sq >> 32;
    }
    v1 = wave_sum_u64(v1);
    lo2 = wave_sum_u64(lo2);
    hi2 = wave_sum_u64(hi2);
    if (lane == 63) {
      const u128 v2 = rows_ess_v2(hi2, lo2);             // below 2^72 per wave; V1 below 2^56
      s_ess[2 * wave] = v2.lo;
      s_ess[2 * wave + 1] = v2.hi | (v1 << 8);
    }
  }
  uint64_t qa[4], run_a = 0, inc_a = 0;
  if (AS) {                                              // the ancestor logits: one tile, their own reference
    float MA;
    inc_a = pick1_put_scan<W>(a, base, n, scale, s_amax, s_ascan, grp, lane, wave, MA, qa, run_a);
  }
  __syncthreads();
  uint64_t woff, total;
  pick_group_offsets<W>(s_scan, grp, wave, woff, total);
  const uint64_t loc = woff + (inc - run);
  uint64_t* cdf = s_cdf + grp * (GT * 4);
#pragma unroll
  for (int c = 0; c < 4; ++c) cdf[base + c] = loc + q[c];
  uint64_t total_a = 0;
  if (AS) total_a = pick1_put_count<W>(as.keys, r, base, n, qa, run_a, inc_a, s_ascan, s_acnt, grp, lane, wave);
  __syncthreads();
  if (!live) return;                                     // (no barrier follows)
  if (gt == 0) {
    max_out[r] = M;
    total_out[r] = total;
    if (total == 0ull) atomicAdd(status, 1ull);
  }
  if (ESS) {                                             // the decision, by every thread of the row's group alike
    u128 V2; V2.hi = 0ull; V2.lo = 0ull;
    uint64_t V1 = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const uint64_t a0 = s_ess[2 * (grp * W + w)], a1 = s_ess[2 * (grp * W + w) + 1];
      V2.lo += a0;
      V2.hi += (a1 & 0xffull) + (V2.lo < a0 ? 1ull : 0ull);
      V1 += a1 >> 8;
    }
    const u128 lhs = mul64(V1, V1 << 8);                 // V1^2 * 256 <= 2^88
    const u128 m_lo = mul64(V2.lo, (uint64_t)ess.ess_q8);
    u128 rhs; rhs.lo = m_lo.lo; rhs.hi = m_lo.hi + V2.hi * (uint64_t)ess.ess_q8;      // ess_q8 * V2 < 2^102
    const bool go = total != 0ull && ((int64_t)ess.ess_q8 > 256 * n || gt128(rhs, lhs));
    if (gt == 0) ess.resampled[r] = go ? 1 : 0;
    float* crow = ess.carry + r * ld;
    if (!go) {                                           // carried forward: identity ancestors, the weights kept
      const int32_t first = (int32_t)(r * index_stride) + (int32_t)base;
      const int32_t idn[4] = {first, first + 1, first + 2, first + 3};
      rows_store4(anc + r * n, base, n, idn);
      rows_store4(crow, base, n, x);
      return;
    }
    const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    rows_store4(crow, base, n, zero);
  }
  gmx_key key; key.k0 = keys[2 * r]; key.k1 = keys[2 * r + 1];
  const uint64_t u0 = KIND == GMX_RESAMPLE_SYSTEMATIC ? (uint64_t)(gmx_bits32(key, 0ull) >> 9) : 0ull;
  const uint64_t D = (uint64_t)n << 23;
  const int32_t add = (int32_t)(r * index_stride);
  int32_t out[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int32_t i = (int32_t)n - 1;                          // no mass at all: the last column, as gmx_resample answers
    if (total != 0ull && base + c < n) {
      i = rows_slot_search<KIND>(cdf, (int32_t)n, key, u0, base + c, total, D);
      i = i < (int32_t)n ? i : (int32_t)n - 1;
    }
    if (PIN && base + c == n - 1) i = (int32_t)n - 1;    // slot n - 1 descends from slot n - 1 (its uniform is its own)
    if (AS && base + c == n - 1) {                       // slot n - 1: the draw from the ancestor logits
      i = (int32_t)pick1_index<W>(s_acnt, grp, n);
      if (total_a == 0ull) {                             // no mass: the plain pin, and counted
        i = (int32_t)n - 1;
        atomicAdd(as.status, 1ull);
      }
    }
    out[c] = i + add;
  }
  rows_store4(anc + r * n, base, n, out);
}

template <int KIND, int W>
__global__ void __launch_bounds__(GMX_ROWS_BLOCK)
k_rows_small(const uint32_t* __restrict__ keys, const float* __restrict__ lw, int64_t rows, int64_t n, int64_t ld,
             int64_t index_stride, float scale, float* __restrict__ max_out, uint64_t* __restrict__ total_out,
             int32_t* __restrict__ anc, unsigned long long* __restrict__ status) {
  rows_small_body<KIND, W, false>(keys, lw, rows, n, ld, index_stride, scale, max_out, total_out, anc, status, rows_pin{});
}

// (`lw` is read and written: not __restrict__)
template <int W>
__global__ void __launch_bounds__(GMX_ROWS_BLOCK)
k_rows_small_pinned(const uint32_t* __restrict__ keys, float* lw, int64_t rows, int64_t n, int64_t ld, int64_t index_stride,
                    float scale, float* __restrict__ max_out, uint64_t* __restrict__ total_out, int32_t* __restrict__ anc,
                    unsigned long long* __restrict__ status, rows_pin pin) {
  rows_small_body<GMX_RESAMPLE_MULTINOMIAL, W, true>(keys, lw, rows, n, ld, index_stride, scale, max_out, total_out, anc,
                                                     status, pin);
}

// (`lw` holds the pin already: only read)
template <int W>
__global__ void __launch_bounds__(GMX_ROWS_BLOCK)
k_rows_small_as(const uint32_t* __restrict__ keys, const float* __restrict__ lw, int64_t rows, int64_t n, int64_t ld,
                int64_t index_stride, float scale, float* __restrict__ max_out, uint64_t* __restrict__ total_out,
                int32_t* __restrict__ anc, unsigned long long* __restrict__ status, rows_as as) {
  rows_small_body<GMX_RESAMPLE_MULTINOMIAL, W, false, true>(keys, lw, rows, n, ld, index_stride, scale, max_out, total_out, anc,
                                                            status, rows_pin{}, as);
}

// (`lw` and `carry` are read and written: not __restrict__)
template <int KIND, int W>
__global__ void __launch_bounds__(GMX_ROWS_BLOCK)
k_rows_small_ess(const uint32_t* __restrict__ keys, float* lw, int64_t rows, int64_t n, int64_t ld, int64_t index_stride,
                 float scale, float* __restrict__ max_out, uint64_t* __restrict__ total_out, int32_t* __restrict__ anc,
                 unsigned long long* __restrict__ status, rows_ess ess) {
  rows_small_body<KIND, W, false, false, true>(keys, lw, rows, n, ld, index_stride, scale, max_out, total_out, anc, status,
                                               rows_pin{}, rows_as{}, ess);
}

// One value per row, value_of(r), over every particle of the row in dst[r * n + i], i < n: the threads (g of `step`) stride
// over the quads of the rows * n particles — four consecutive particles per thread, one store (rows_store4); a quad may
// span rows (n is arbitrary), the value is read again only where the row changes.
template <class F>
__device__ __forceinline__ void rows_spread(float* __restrict__ dst, int64_t rows, int64_t n, int64_t g, int64_t step, F value_of) {
  const int64_t cols = rows * n, quads = (cols + 3) / 4;
  for (int64_t qd = g; qd < quads; qd += step) {
    const int64_t base = qd * 4;
    int64_t r = base / n, k = base - r * n;              // particle `base` is column k of row r
    float cur = value_of(r);                             // (base < cols: r < rows)
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = cur;
      if (++k == n) {
        k = 0; ++r;
        if (r < rows) cur = value_of(r);
      }
    }
    rows_store4(dst, base, cols, v);
  }
}

// The pins into the matrix and the state store (gmx_rows_pin; gmx_resample_rows_pinned past one tile, before the row's
// statistics are taken).  blockIdx.y: the state word d < D, or (y = D) the weight; the threads of a y stride over the rows.
// next_x ([D, rows], may be null): state word d of row r also goes to every particle of the row in a second store,
// next[d * next_ld + r * n + i], i < n (rows_spread).
__global__ void __launch_bounds__(GMX_ROWS_BLOCK)
k_rows_pin(float* __restrict__ lw, int64_t rows, int64_t n, int64_t ld, rows_pin pin, const float* __restrict__ next_x,
           float* __restrict__ next, int64_t next_ld) {
  const int64_t g = (int64_t)blockIdx.x * GMX_ROWS_BLOCK + (int64_t)threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * GMX_ROWS_BLOCK;
  const int32_t d = (int32_t)blockIdx.y;
  for (int64_t r = g; r < rows; r += step) {
    if (d == pin.D) lw[r * ld + n - 1] = pin.lw[r];
    else pin.x_out[(int64_t)d * pin.x_ld + r * pin.x_row_stride + n - 1] = pin.x[(int64_t)d * rows + r];
  }
  if (next_x == nullptr || d == pin.D) return;
  const float* __restrict__ src = next_x + (int64_t)d * rows;
  rows_spread(next + (int64_t)d * next_ld, rows, n, g, step, [&](int64_t r) { return src[r]; });
}

// What gmx_pick_rows_take adds to a row's pick (backward simulation: what was picked, taken and handed on)
struct rows_take {
  const float* lw;      // the weights, rows lw_ld elements apart (may be the logits themselves): lw_out[r] = lw[r * lw_ld + k]
  int64_t lw_ld;
  const float* x;       // [D, x_ld]: x_out[d * rows + r] = x[d * x_ld + r * x_row_stride + k]
  int32_t D;
  int64_t x_ld, x_row_stride;
  int64_t index_stride; // idx_out[r] = k + r * index_stride
  int32_t* idx_out;     // [rows]
  float* lw_out;        // [rows]
  float* x_out;         // [D, rows]
  float* next;          // [D, next_ld] or null: next[d * next_ld + r * n + i] = x_out[d * rows + r], i < n
  int64_t next_ld;
};

// gmx_pick_rows_take, n <= 1024: k_rows_small's packing (W waves per row, 4 / W rows per workgroup, thread gt of a row's
// group holds columns 4 gt .. 4 gt + 3) around the one-tile pick (pick1_*, gmx_backward.h) on its own.  Three barriers, 64
// bytes of LDS, no CDF in LDS: nothing is searched.  After the third barrier every thread of the group knows k: thread 0
// writes the three outputs, every thread reads the one word x[.. + k] per state word (one address per group) and stores
// its four columns of the broadcast.  Every thread reaches every barrier (a group past the last row works on the last
// row again and writes nothing).
template <int W>
__global__ void __launch_bounds__(GMX_ROWS_BLOCK)
k_rows_small_take(const uint32_t* __restrict__ keys, const float* __restrict__ logits, int64_t rows, int64_t n, int64_t ld,
                  float scale, unsigned long long* __restrict__ status, rows_take tk) {
  static_assert(W == 1 || W == 2 || W == 4, "waves per row");
  constexpr int RPW = 4 / W, GT = 64 * W;
  __shared__ float s_max[4];
  __shared__ uint64_t s_scan[4];
  __shared__ uint32_t s_cnt[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = tid / GT, gt = tid % GT;
  const int64_t r_ = (int64_t)blockIdx.x * RPW + grp;
  const bool live = r_ < rows;
  const int64_t r = live ? r_ : rows - 1;
  const int64_t base = (int64_t)gt * 4;
  float a[4];
  pick_load4(logits + r * ld, base, n, a);
  pick1_put_max(a, s_max, lane, wave);
  __syncthreads();
  float M;
  uint64_t q[4], run;
  const uint64_t inc = pick1_put_scan<W>(a, base, n, scale, s_max, s_scan, grp, lane, wave, M, q, run);
  __syncthreads();
  const uint64_t total = pick1_put_count<W>(keys, r, base, n, q, run, inc, s_scan, s_cnt, grp, lane, wave);
  __syncthreads();
  if (!live) return;                                     // (no barrier follows)
  int64_t k = (int64_t)pick1_index<W>(s_cnt, grp, n);
  if (total == 0ull) k = n - 1;                          // no mass at all: the last column, as gmx_pick_rows answers, and counted
  if (gt == 0) {
    if (total == 0ull) atomicAdd(status, 1ull);
    tk.idx_out[r] = (int32_t)k + (int32_t)(r * tk.index_stride);
    tk.lw_out[r] = tk.lw[r * tk.lw_ld + k];
  }
  const float* __restrict__ src = tk.x + (r * tk.x_row_stride + k);
  for (int32_t d = 0; d < tk.D; ++d) {
    const float v = src[(int64_t)d * tk.x_ld];           // (one address per group)
    if (gt == 0) tk.x_out[(int64_t)d * rows + r] = v;
    if (tk.next != nullptr) {
      const float v4[4] = {v, v, v, v};
      rows_store4(tk.next + ((int64_t)d * tk.next_ld + r * n), base, n, v4);
    }
  }
}

// gmx_pick_rows_take past one tile, after k_pick_row wrote idx_out: the gather and the broadcast, modelled on k_rows_pin.
// blockIdx.y: the state word d < D, or (y = D) the weight; the threads of a y stride over the rows, then (d < D, with a
// broadcast) over the quads of the rows * n particles.  Row r's pick is idx_out[r] - r * index_stride; the broadcast reads
// the store through it, not x_out (which this launch writes).
__global__ void __launch_bounds__(GMX_ROWS_BLOCK)
k_rows_take(int64_t rows, int64_t n, rows_take tk) {
  const int64_t g = (int64_t)blockIdx.x * GMX_ROWS_BLOCK + (int64_t)threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * GMX_ROWS_BLOCK;
  const int32_t d = (int32_t)blockIdx.y;
  const int32_t* __restrict__ idx = tk.idx_out;
  for (int64_t r = g; r < rows; r += step) {
    const int64_t k = (int64_t)(idx[r] - (int32_t)(r * tk.index_stride));
    if (d == tk.D) tk.lw_out[r] = tk.lw[r * tk.lw_ld + k];
    else tk.x_out[(int64_t)d * rows + r] = tk.x[(int64_t)d * tk.x_ld + r * tk.x_row_stride + k];
  }
  if (tk.next == nullptr || d == tk.D) return;
  const float* __restrict__ src = tk.x + (int64_t)d * tk.x_ld;
  rows_spread(tk.next + (int64_t)d * tk.next_ld, rows, n, g, step, [&](int64_t r) {
    return src[r * tk.x_row_stride + (int64_t)(idx[r] - (int32_t)(r * tk.index_stride))];
  });
}

// n > 1024: blockIdx.x the tile, blockIdx.y the row (row0 + y).  tmax / agg: k_pick_stats' [rows, n_tiles] statistics.
// cdf_i = prefix_b + ((tile-local inclusive sum) >> (K - k_b)), as k_weight_cdf writes it.
template <int KIND>
__global__ void __launch_bounds__(GMX_ROWS_BLOCK)
k_rows_tile(const uint32_t* __restrict__ keys, const float* __restrict__ lw, int64_t n, int64_t ld, int n_tiles, int64_t row0,
            int64_t index_stride, float scale, const float* __restrict__ tmax, const uint64_t* __restrict__ agg,
            float* __restrict__ max_out, uint64_t* __restrict__ total_out, int32_t* __restrict__ anc,
            uint64_t* __restrict__ cdf_out, unsigned long long* __restrict__ status) {
  __shared__ float lds4[4];
  __shared__ uint64_t lds8[4];
  __shared__ uint64_t s_pref[GMX_TP_MAX_TILES + 16];
  __shared__ uint64_t s_cdf[GMX_PICK_TILE];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = (int)blockIdx.x;
  const int64_t r = row0 + (int64_t)blockIdx.y;
  const float* __restrict__ tm = tmax + r * n_tiles;
  const int64_t col0 = (int64_t)b * GMX_PICK_TILE, base = col0 + (int64_t)tid * 4;
  float x[4];
  pick_load4(lw + r * ld, base, n, x);
  const float tmax_mine = tm[b];
  gmx_tile_prefix_block(tm, agg + r * n_tiles, n_tiles, s_pref, lds4, lds8);
  const int32_t k_b = gmx_tile_exp(tmax_mine);
  const float ref_b = gmx_tile_ref(k_b);
  uint64_t q[4];
  const uint64_t run = gmx_tile_fixed4(x, base, n, false, ref_b, scale, q);
  const uint64_t inc = wave_scan_u64(run);
  __syncthreads();                                       // s_pref is written; lds8 has been read
  if (lane == 63) lds8[wave] = inc;
  __syncthreads();
  uint64_t woff, tile_sum;
  pick_group_offsets<4>(lds8, 0, wave, woff, tile_sum);
  const uint64_t loc = woff + (inc - run);
  const uint64_t prefix = s_pref[b], total = s_pref[n_tiles], mk = s_pref[n_tiles + 1];
  const int32_t K = (int32_t)(uint32_t)(mk >> 32);
#pragma unroll
  for (int c = 0; c < 4; ++c) s_cdf[tid * 4 + c] = prefix + gmx_tile_scale(loc + q[c], k_b, K);
  __syncthreads();
  if (b == 0 && tid == 0) {
    max_out[r] = gmx_u2f((uint32_t)mk);
    total_out[r] = total;
    if (total == 0ull) atomicAdd(status, 1ull);
  }
  const int32_t add = (int32_t)(r * index_stride);
  int32_t* __restrict__ arow = anc + r * n;
  if (KIND == GMX_RESAMPLE_MULTINOMIAL) {                // the row's CDF for k_rows_mn (a row without mass: all zero)
    uint64_t* __restrict__ crow = cdf_out + r * n;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (base + c < n) crow[base + c] = s_cdf[tid * 4 + c];
    return;
  }
  if (total == 0ull) {                                   // no mass at all: every slot maps to the last column
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (base + c < n) arow[base + c] = (int32_t)(n - 1) + add;
    return;
  }
  gmx_key key; key.k0 = keys[2 * r]; key.k1 = keys[2 * r + 1];
  const uint64_t u0 = KIND == GMX_RESAMPLE_SYSTEMATIC ? (uint64_t)(gmx_bits32(key, 0ull) >> 9) : 0ull;
  const uint64_t D = (uint64_t)n << 23;
  const uint64_t upper = s_cdf[GMX_PICK_TILE - 1];      // prefix_b + G_b (columns past n carry nothing)
  if (upper == prefix) return;                           // an empty tile owns no slot
  const int64_t T0 = rows_slots_below<KIND>(key, u0, prefix, D, total, n);
  const int64_t T1 = rows_slots_below<KIND>(key, u0, upper, D, total, n);
  const int64_t left = n - col0;
  const int32_t cnt = left < GMX_PICK_TILE ? (int32_t)left : GMX_PICK_TILE;
  for (int64_t j = T0 + tid; j < T1; j += GMX_ROWS_BLOCK) {
    int32_t i = rows_slot_search<KIND>(s_cdf, cnt, key, u0, j, total, D);
    i = i < cnt ? i : cnt - 1;
    arow[j] = (int32_t)col0 + i + add;
  }
}

// iid multinomial past one tile: slot j of row r searches the row's CDF array.  blockIdx.x: 256 slots, blockIdx.y: the row.
// PIN: slot n - 1 answers n - 1 (gmx_resample_rows_pinned).
template <bool PIN>
__global__ void __launch_bounds__(GMX_ROWS_BLOCK)
k_rows_mn(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ cdf, int64_t n, int64_t row0, int64_t index_stride,
          const uint64_t* __restrict__ total_in, int32_t* __restrict__ anc) {
  const int64_t r = row0 + (int64_t)blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * GMX_ROWS_BLOCK + (int64_t)threadIdx.x;
  if (j >= n) return;
  const uint64_t total = total_in[r];
  int32_t i = (int32_t)n - 1;
  if (total != 0ull && !(PIN && j == n - 1)) {
    gmx_key key; key.k0 = keys[2 * r]; key.k1 = keys[2 * r + 1];
    i = rows_slot_search<GMX_RESAMPLE_MULTINOMIAL>(cdf + r * n, (int32_t)n, key, 0ull, j, total, 0ull);
    i = i < (int32_t)n ? i : (int32_t)n - 1;
  }
  anc[r * n + j] = i + (int32_t)(r * index_stride);
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)
#include <vector>
#include "genmi.h"
#include "gmx_math.h"
// (`used`: emitted, and so exported by a shared library, although nothing in the translation unit calls them)

extern "C" __attribute__((used)) inline size_t gmx_resample_rows_workspace(int kind, int64_t rows, int64_t n) {
  return gmx_resample_rows_bytes_(kind, rows, n);
}

extern "C" __attribute__((used)) inline int gmx_resample_rows(int kind, const uint32_t* keys_d, const float* lw_d, int64_t rows, int64_t n,
                                        int64_t ld, int64_t index_stride, float* max_d, uint64_t* total_d, int32_t* ancestors_d,
                                        int64_t* status_d, void* workspace_d, gmx_stream stream) {
  const gmx_refusal no = gmx_resample_rows_refusal_(!keys_d || !lw_d || !max_d || !total_d || !ancestors_d || !status_d || !workspace_d,
                                                    kind, rows, n, ld, index_stride);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_resample_rows", no.v);
  const int shift = gmx_pick_rows_shift_(n);
  std::vector<float> row((size_t)n);                             // (the per-row path asks for an aligned row)
  std::vector<uint64_t> cdf(kind == GMX_RESAMPLE_MULTINOMIAL ? (size_t)n : 0);
  std::vector<uint64_t> ws((gmx_resample_workspace(n) + 7) / 8 + 2);
  for (int64_t r = 0; r < rows; ++r) {
    const float* src = lw_d + r * ld;
    float M = -gmx_inf();
    for (int64_t i = 0; i < n; ++i) { row[(size_t)i] = src[i]; M = gmx_rmax(M, src[i]); }
    uint64_t total = 0;
    int32_t* out = ancestors_d + r * n;
    if (kind == GMX_RESAMPLE_MULTINOMIAL) {
      if (gmx_weight_cdf(row.data(), n, shift, nullptr, 0, &M, cdf.data(), &total, ws.data(), stream)) return 1;
      if (gmx_ancestors(kind, keys_d + 2 * r, cdf.data(), n, 0, &total, n, 0, n, out, stream)) return 1;
    } else if (gmx_resample(kind, keys_d + 2 * r, row.data(), n, shift, nullptr, 0, &M, &total, out, ws.data(), stream)) {
      return 1;
    }
    max_d[r] = M;
    total_d[r] = total;
    if (total == 0) status_d[0] += 1;
    const int32_t add = (int32_t)(r * index_stride);
    for (int64_t i = 0; i < n; ++i) out[i] += add;
  }
  return 0;
}

// the definition, in order: the pins into the matrix and the store, the unconditional draw on the pinned weights, slot n - 1
extern "C" __attribute__((used)) inline int gmx_resample_rows_pinned(const uint32_t* keys_d, float* lw_d, int64_t rows, int64_t n, int64_t ld,
                                               int64_t index_stride, const float* pin_lw_d, const float* pin_x_d, float* x_d,
                                               int32_t D, int64_t x_ld, int64_t x_row_stride, float* max_d, uint64_t* total_d,
                                               int32_t* ancestors_d, int64_t* status_d, void* workspace_d, gmx_stream stream) {
  const char* who = "gmx_resample_rows_pinned";
  const gmx_refusal no = gmx_resample_rows_pinned_refusal_(
      !keys_d || !lw_d || !pin_lw_d || !max_d || !total_d || !ancestors_d || !status_d || !workspace_d, rows, n, ld, index_stride,
      D, x_ld, x_row_stride, !pin_x_d, !x_d);
  if (no.fmt) return gmx_fail(no.fmt, who, no.v);
  for (int64_t r = 0; r < rows; ++r) {
    lw_d[r * ld + n - 1] = pin_lw_d[r];
    for (int64_t d = 0; d < D; ++d) x_d[d * x_ld + r * x_row_stride + n - 1] = pin_x_d[d * rows + r];
  }
  if (gmx_resample_rows(GMX_RESAMPLE_MULTINOMIAL, keys_d, lw_d, rows, n, ld, index_stride, max_d, total_d, ancestors_d,
                        status_d, workspace_d, stream)) return 1;
  for (int64_t r = 0; r < rows; ++r) ancestors_d[r * n + n - 1] = (int32_t)(n - 1 + r * index_stride);
  return 0;
}

// steps 1 and 2 of the above as a call of their own, and the broadcast of a second state over every particle of its row
extern "C" __attribute__((used)) inline int gmx_rows_pin(float* lw_d, int64_t rows, int64_t n, int64_t ld, const float* pin_lw_d,
                                   const float* pin_x_d, float* x_d, int32_t D, int64_t x_ld, int64_t x_row_stride,
                                   const float* next_x_d, float* next_d, int64_t next_ld, gmx_stream stream) {
  const char* who = "gmx_rows_pin";
  (void)stream;
  const gmx_refusal no = gmx_rows_pin_refusal_(!lw_d || !pin_lw_d, rows, n, ld, D, x_ld, x_row_stride, next_x_d != nullptr,
                                               next_ld, !pin_x_d, !x_d, !next_d);
  if (no.fmt) return gmx_fail(no.fmt, who, no.v);
  for (int64_t r = 0; r < rows; ++r) {
    lw_d[r * ld + n - 1] = pin_lw_d[r];
    for (int64_t d = 0; d < D; ++d) x_d[d * x_ld + r * x_row_stride + n - 1] = pin_x_d[d * rows + r];
    if (next_x_d)
      for (int64_t d = 0; d < D; ++d)
        for (int64_t i = 0; i < n; ++i) next_d[d * next_ld + r * n + i] = next_x_d[d * rows + r];
  }
  return 0;
}

extern "C" __attribute__((used)) inline size_t gmx_resample_rows_as_workspace(int64_t rows, int64_t n) {
  return gmx_resample_rows_as_bytes_(rows, n);
}

// the definition, in order: the unconditional draw, one draw per row from the ancestor logits, that draw into slot n - 1
extern "C" __attribute__((used)) inline int gmx_resample_rows_as(const uint32_t* keys_d, const float* lw_d, int64_t rows, int64_t n, int64_t ld,
                                           int64_t index_stride, const uint32_t* as_keys_d, const float* as_lw_d, int64_t as_ld,
                                           float* max_d, uint64_t* total_d, int32_t* ancestors_d, int64_t* status_d,
                                           void* workspace_d, gmx_stream stream) {
  const char* who = "gmx_resample_rows_as";
  const gmx_refusal no = gmx_resample_rows_as_refusal_(
      !keys_d || !lw_d || !as_keys_d || !as_lw_d || !max_d || !total_d || !ancestors_d || !status_d || !workspace_d, rows, n, ld,
      index_stride, as_ld);
  if (no.fmt) return gmx_fail(no.fmt, who, no.v);
  if (gmx_resample_rows(GMX_RESAMPLE_MULTINOMIAL, keys_d, lw_d, rows, n, ld, index_stride, max_d, total_d, ancestors_d,
                        status_d, workspace_d, stream)) return 1;
  std::vector<int32_t> tmp((size_t)rows);
  std::vector<uint64_t> ws((gmx_resample_workspace(n) + 7) / 8 + 2);       // (what the per-row path may ask for)
  if (gmx_pick_rows(as_keys_d, as_lw_d, rows, n, as_ld, tmp.data(), status_d + 1, ws.data(), stream)) return 1;
  for (int64_t r = 0; r < rows; ++r) ancestors_d[r * n + n - 1] = tmp[(size_t)r] + (int32_t)(r * index_stride);
  return 0;
}

extern "C" __attribute__((used)) inline size_t gmx_resample_rows_ess_workspace(int kind, int64_t rows, int64_t n) {
  return gmx_resample_rows_ess_bytes_(kind, rows, n);
}

// the definition, in order: the sum into the matrix, the unconditional draw on it, the integer predicate, the gating
extern "C" __attribute__((used)) inline int gmx_resample_rows_ess(int kind, const uint32_t* keys_d, float* lw_d, float* carry_d, int64_t rows,
                                            int64_t n, int64_t ld, int64_t index_stride, uint32_t ess_q8, float* max_d,
                                            uint64_t* total_d, int32_t* resampled_d, int32_t* ancestors_d, int64_t* status_d,
                                            void* workspace_d, gmx_stream stream) {
  const char* who = "gmx_resample_rows_ess";
  const gmx_refusal no = gmx_resample_rows_ess_refusal_(
      !keys_d || !lw_d || !carry_d || !max_d || !total_d || !resampled_d || !ancestors_d || !status_d || !workspace_d, kind, rows,
      n, ld, index_stride);
  if (no.fmt) return gmx_fail(no.fmt, who, no.v);
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t i = 0; i < n; ++i) lw_d[r * ld + i] = lw_d[r * ld + i] + carry_d[r * ld + i];
  if (gmx_resample_rows(kind, keys_d, lw_d, rows, n, ld, index_stride, max_d, total_d, ancestors_d, status_d, workspace_d,
                        stream)) return 1;
  const int shift = gmx_pick_rows_shift_(n);
  for (int64_t r = 0; r < rows; ++r) {
    const float ref = gmx_tile_ref(gmx_tile_exp(max_d[r]));      // one tile: the row's reference is the tile's
    unsigned __int128 V1 = 0, V2 = 0;
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t v = gmx_exp_fixed(lw_d[r * ld + i] - ref, shift) >> (shift - 30);
      V1 += v;
      V2 += (unsigned __int128)v * v;
    }
    const bool go = total_d[r] != 0 && (ess_q8 > gmx_ess_always_(n) || V1 * V1 * 256 < (unsigned __int128)ess_q8 * V2);
    resampled_d[r] = go ? 1 : 0;
    for (int64_t i = 0; i < n; ++i) {
      carry_d[r * ld + i] = go ? 0.0f : lw_d[r * ld + i];
      if (!go) ancestors_d[r * n + i] = (int32_t)(i + r * index_stride);
    }
  }
  return 0;
}

extern "C" __attribute__((used)) inline size_t gmx_pick_rows_take_workspace(int64_t rows, int64_t n) {
  return gmx_pick_rows_take_bytes_(rows, n);
}

// the definition, in order: one draw per row from the logits, what it picked copied out, the picked state over the row
extern "C" __attribute__((used)) inline int gmx_pick_rows_take(const uint32_t* keys_d, const float* logits_d, int64_t rows, int64_t n, int64_t ld,
                                         const float* lw_d, int64_t lw_ld, const float* x_d, int32_t D, int64_t x_ld,
                                         int64_t x_row_stride, int64_t index_stride, int32_t* idx_out_d, float* lw_out_d,
                                         float* x_out_d, float* next_d, int64_t next_ld, int64_t* status_d, void* workspace_d,
                                         gmx_stream stream) {
  const char* who = "gmx_pick_rows_take";
  const gmx_refusal no = gmx_pick_rows_take_refusal_(
      !keys_d || !logits_d || !lw_d || !idx_out_d || !lw_out_d || !status_d || !workspace_d, rows, n, ld, lw_ld, D, x_ld,
      x_row_stride, index_stride, next_d != nullptr, next_ld, !x_d, !x_out_d);
  if (no.fmt) return gmx_fail(no.fmt, who, no.v);
  std::vector<int32_t> k((size_t)rows);
  std::vector<uint64_t> ws((gmx_resample_workspace(n) + 7) / 8 + 2);       // (what the per-row path may ask for)
  if (gmx_pick_rows(keys_d, logits_d, rows, n, ld, k.data(), status_d, ws.data(), stream)) return 1;
  for (int64_t r = 0; r < rows; ++r) {
    const int64_t kr = k[(size_t)r];
    idx_out_d[r] = (int32_t)(kr + r * index_stride);
    lw_out_d[r] = lw_d[r * lw_ld + kr];
    for (int64_t d = 0; d < D; ++d) x_out_d[d * rows + r] = x_d[d * x_ld + r * x_row_stride + kr];
    if (next_d)
      for (int64_t d = 0; d < D; ++d)
        for (int64_t i = 0; i < n; ++i) next_d[d * next_ld + r * n + i] = x_out_d[d * rows + r];
  }
  return 0;
}
#endif
