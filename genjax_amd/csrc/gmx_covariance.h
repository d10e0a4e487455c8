// Weighted mean and FULL covariance of many independent rows (include/genmi.h "Row-wise weighted covariance":
// gmx_rows_covariance): weights and state addressed as gmx_rows_moments addresses them, and exactly its weights — a_i = lw_i
// (+ carry_i, ONE float32 add: mom_add), M the row's gmx_rmax, e_i = (double) gmx_mom_weight(a_i, M).  With z_0 = 1 and
// z_d = (double) x_{d-1,i}, 1 <= d <= D <= 15, the row's Gram matrix G = Z^T diag(e) Z, in float64:
//     G_jk = sum_i (e_i z_j) z_k      S0 = G_00      mean_d = G_0d / S0      cov_jk = G_jk / S0 - mean_j mean_k
//     out[r, d] = mean_d      out[r, D + j D + k] = out[r, D + k D + j] = cov_jk (j <= k computed once, stored twice; the
//     diagonal clamped at 0 as gmx_mom_mean_var clamps the variance)
// A row without mass (S0 = 0) writes NaN everywhere.  Nothing is written into the inputs.  The summation order is fixed —
// a matrix instruction's four columns, the blocks of 16 columns of a wave in order, the waves in order, the tiles in order —
// so a row's result depends on n alone, not on rows, the grid or the row's position.
// WHY A MATRIX INSTRUCTION.  1 + D <= 16, so G is ONE 16 x 16 accumulator tile of v_mfma_f64_16x16x4_f64: S0, the D first
// moments and the D (D + 1) / 2 second moments at once, against D (D + 1) / 2 pairs of 64-lane butterflies (120 at D = 15)
// had mom_reduce been extended.  The instruction computes C += A B for A [16 x 4], B [4 x 16]; per lane l, with c = l mod 16
// and q = l / 16, ONE double of each: A's element (c, q) and B's element (q, c).  Taking the 4 as four consecutive columns
// (particles) i = base + q and the 16 as the components, lane l supplies B = z_c of particle base + q and A = e z_c of the
// same particle: both operands from one loaded word.  THE ACCUMULATOR (AMD's matrix instruction calculator for gfx90a and
// later; the same as composable_kernel's mfma_f64_16x16x4f64: groups of ONE row, four groups a lane, four rows apart):
// double v (0..3) of lane l holds C[4 v + q][c] — row 4 v + l / 16, column l mod 16.  (The f32 16x16x4 form holds
// C[4 q + v][c]: the two differ by exactly the wrong 4-row block a test with D >= 3 distinct components shows.)
//   n <= 1024   k_rows_cov_small<W>: ONE launch, no workspace traffic, the packing of rows_small_body — W = 1, 2 or 4 waves
//               per row, 4 / W rows per 256-thread workgroup.  Phase 1, as k_rows_moments_small: a thread loads its four
//               columns of lw (and carry), the row's maximum is gmx_moments.h's mom_row_max (4 LDS words), and the thread
//               parks its four e_i in LDS by column as the float32 values they are (4 KB a workgroup; columns >= n: 0).
//               Phase 2: a wave owns 256 consecutive columns, 16 to a block: lane (c, q) with 1 <= c <= D issues ONE
//               16-byte load of component c - 1 at columns blk + 4 q .. + 3 (c = 0 holds 1, c > D holds 0 and loads
//               nothing), reads its four e from LDS — the 16 lanes of a k-slot read the same 16 bytes: a broadcast —
//               and the block is four MFMAs, k-step j taking column blk + 4 q + j of every k-slot.  The loads of ALL of
//               the wave's (up to 16) blocks are issued before the first wait, 64 VGPRs: the wave pays one memory latency,
//               where loading one block ahead paid sixteen in a row (measured: +10.2 us per step of a captured sweep
//               at R = 256, n = 1024 against +7.3 us so).  Phase 3: each wave parks its
//               256 accumulator doubles in LDS (W x 2 KB a row); ONE barrier; the threads of the row's group take the
//               entries j <= k, add the W waves in wave order — S0 and the two first moments the same way — and store.
//   n > 1024    k_rows_cov_part, one workgroup per (row, tile of 1024 columns): the body above at W = 4 relative to the
//               tile's own maximum m_b; m_b and the 136 upper-triangle doubles per (row, tile) into the workspace (a tile
//               without mass: zeros and m_b = -inf).  Then k_rows_cov_finish, one workgroup per row: M = max_b m_b, thread
//               t < 136 sums its entry over the tiles in ascending order under s_b = exp(m_b - M), taken in FLOAT64 for
//               the reason gmx_moments.h gives (s_b parked in LDS, 8 bytes a tile), and the outputs as above.  No MFMA.
// Under hipcc: the kernels, included by gmx_kernels.hip only (not among the headers embedded for hiprtc).  Under a plain
// host compiler: the ENTRY POINTS as a sequential loop over rows implementing the definition literally, sums in column
// order, with the same refusals (gmx_sizes.h); gmx_vm.h includes this file there.
#pragma once
#include "gmx_moments.h"               /* gmx_mom_weight, gmx_mom_tile_scale; under hipcc mom_row_max, pick_load4 */

// entry (i <= j) of the 16 x 16 upper triangle, rows in order: 0 .. 135
GMX_HD int gmx_cov_tri(int i, int j) { return 16 * i - i * (i - 1) / 2 + (j - i); }
// what entry (i <= j) of a row's Gram matrix writes: g = G_ij, g0i = G_0i, g0j = G_0j, S0 = G_00
GMX_HD void gmx_cov_store(double S0, double g0i, double g0j, double g, int i, int j, int32_t D, double* out) {
  const bool mass = S0 > 0.0;
  if (i == 0) {
    if (j > 0) out[j - 1] = mass ? g / S0 : (double)gmx_nan();
    return;
  }
  const double v = mass ? g / S0 - (g0i / S0) * (g0j / S0) : (double)gmx_nan();
  const double w = (i == j && v < 0.0) ? 0.0 : v;                // (false for NaN)
  out[(int64_t)D + (int64_t)(i - 1) * D + (j - 1)] = w;
  out[(int64_t)D + (int64_t)(j - 1) * D + (i - 1)] = w;
}

#if defined(__HIPCC__)

#define GMX_COV_BLOCK 256
static_assert(GMX_COV_REC == 16 * 17 / 2 && GMX_COV_MAX_D + 1 == 16, "one 16 x 16 accumulator tile");
static_assert(GMX_PICK_TILE == 4 * GMX_COV_BLOCK, "a workgroup's threads hold one tile, four columns each");
typedef double cov_d4 __attribute__((ext_vector_type(4)));

// LDS of the Gram phase: the waves' maxima, the tile's e by column, the waves' accumulator tiles
struct cov_lds {
  float max[4];
  __attribute__((aligned(16))) float e[GMX_PICK_TILE];
  double acc[4][256];
};

// The Gram matrix of columns col0 .. col0 + 256 W - 1 (those below n) of one row, held by waves grp * W .. grp * W + W - 1,
// relative to the maximum of those columns (returned): on return s.acc[grp * W + w] holds wave w's share, entry (i, j) at
// 16 i + j, and every thread of the workgroup has passed the barrier after it.  gt: the thread within the row's group.
// Every thread of the workgroup calls it (three barriers).
template <int W>
__device__ __forceinline__ float cov_gram(const float* __restrict__ lw, const float* __restrict__ carry,
                                          const float* __restrict__ xrow, int32_t D, int64_t x_ld, int64_t col0, int64_t n,
                                          int grp, int gt, int lane, int wave, cov_lds& s) {
  constexpr int GT = 64 * W;
  const int c = lane & 15, q = lane >> 4;
  const int64_t base = col0 + (int64_t)gt * 4;                  // phase 1: this thread's four columns
  const int64_t w0 = col0 + (int64_t)(wave - grp * W) * 256;    // phase 2: this wave's 256 columns, w0 .. wend - 1
  const int64_t wend = w0 + 256 < n ? w0 + 256 : n;
  const float* __restrict__ zrow = (c >= 1 && c <= D) ? xrow + (int64_t)(c - 1) * x_ld : nullptr;
  // every component's words at a multiple of four columns are 16-byte aligned (uniform over the wave, as w0 and wend are)
  const bool quads = __builtin_amdgcn_readfirstlane((int)(((uintptr_t)xrow | ((uintptr_t)x_ld << 2)) & 15u)) == 0;
  float a[4], cy[4], z[16][4];
  pick_load4(lw, base, n, a);
  if (carry != nullptr) pick_load4(carry, base, n, cy);
  // Lane (c, q)'s operand words of block b, columns cb .. cb + 3: component c - 1 for 1 <= c <= D, the constant 1 for c = 0,
  // 0 for c > D.  A block whole below n in an aligned row is ONE 16-byte load; the ragged last block, or a row that is not
  // aligned, is up to four guarded loads.  The choice is uniform and each load is a plain guarded one — no select, no
  // two-sided branch on the loaded registers — so nothing waits here: every load is out before the first wait.
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    const int64_t cb = w0 + 16 * b + 4 * q;
#pragma unroll
    for (int k = 0; k < 4; ++k) z[b][k] = c == 0 ? 1.0f : 0.0f;
    if (quads && w0 + 16 * b + 16 <= wend) {
      if (zrow != nullptr) {
        const float4 v = *reinterpret_cast<const float4*>(zrow + cb);
        z[b][0] = v.x; z[b][1] = v.y; z[b][2] = v.z; z[b][3] = v.w;
      }
    } else if (w0 + 16 * b < wend) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (zrow != nullptr && cb + k < n) z[b][k] = zrow[cb + k];
    }
  }
  const float M = mom_row_max<W>(a, cy, carry != nullptr, s.max, grp, lane, wave);
  float4 e4;                                                     // (a column >= n was loaded as -inf: weight 0)
  e4.x = gmx_mom_weight(a[0], M); e4.y = gmx_mom_weight(a[1], M);
  e4.z = gmx_mom_weight(a[2], M); e4.w = gmx_mom_weight(a[3], M);
  float* __restrict__ se = s.e + grp * GT * 4;                  // the row's columns, from col0
  *reinterpret_cast<float4*>(se + gt * 4) = e4;
  __syncthreads();
  cov_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    if (w0 + 16 * b >= wend) break;                              // (uniform over the wave: the MFMAs run with every lane)
    const float4 eb = *reinterpret_cast<const float4*>(se + (w0 - col0) + 16 * b + 4 * q);
    const float e[4] = {eb.x, eb.y, eb.z, eb.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double zk = (w0 + 16 * b + 4 * q + k < n) ? (double)z[b][k] : 0.0;       // (a column >= n: A = B = 0)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)e[k] * zk, zk, acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) s.acc[wave][16 * (4 * v + q) + c] = acc[v];      // C[4 v + q][c] (the header says why)
  __syncthreads();
  return M;
}
// entry (i, j) of the row's Gram matrix: the W waves in wave order
template <int W>
__device__ __forceinline__ double cov_entry(const cov_lds& s, int grp, int i, int j) {
  double g = s.acc[grp * W][16 * i + j];
#pragma unroll
  for (int w = 1; w < W; ++w) g += s.acc[grp * W + w][16 * i + j];
  return g;
}

// n <= 1024: W waves per row, 4 / W rows per workgroup.  Every thread reaches every barrier (a group past the last row
// works on the last row again and writes nothing).
template <int W>
__global__ void __launch_bounds__(GMX_COV_BLOCK)
k_rows_cov_small(const float* __restrict__ lw, const float* __restrict__ carry, int64_t rows, int64_t n, int64_t ld,
                 const float* __restrict__ x, int32_t D, int64_t x_ld, int64_t x_row_stride, double* __restrict__ out,
                 int64_t out_ld) {
  static_assert(W == 1 || W == 2 || W == 4, "waves per row");
  constexpr int RPW = 4 / W, GT = 64 * W;
  __shared__ cov_lds s;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (uniform, and known so)
  const int grp = wave / W, gt = tid - grp * GT;
  const int64_t r_ = (int64_t)blockIdx.x * RPW + grp;
  const bool live = r_ < rows;
  const int64_t r = live ? r_ : rows - 1;
  cov_gram<W>(lw + r * ld, carry != nullptr ? carry + r * ld : nullptr, x + r * x_row_stride, D, x_ld, 0, n, grp, gt, lane,
              wave, s);
  if (!live) return;
  const double S0 = cov_entry<W>(s, grp, 0, 0);
  for (int t = gt; t < 256; t += GT) {                           // entry (i, j) = (t / 16, t mod 16), the upper triangle
    const int i = t >> 4, j = t & 15;
    if (i > j || j > D) continue;
    gmx_cov_store(S0, cov_entry<W>(s, grp, 0, i), cov_entry<W>(s, grp, 0, j), cov_entry<W>(s, grp, i, j), i, j, D,
                  out + r * out_ld);
  }
}

// n > 1024, first launch: blockIdx.x the tile, blockIdx.y the row (row0 + y); cell = r * n_tiles + b
__global__ void __launch_bounds__(GMX_COV_BLOCK)
k_rows_cov_part(const float* __restrict__ lw, const float* __restrict__ carry, int64_t n, int64_t ld, int64_t n_tiles,
                int64_t row0, const float* __restrict__ x, int32_t D, int64_t x_ld, int64_t x_row_stride,
                double* __restrict__ rec, float* __restrict__ tmax) {
  __shared__ cov_lds s;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t r = row0 + (int64_t)blockIdx.y;
  const int64_t cell = r * n_tiles + (int64_t)blockIdx.x;
  const float m = cov_gram<4>(lw + r * ld, carry != nullptr ? carry + r * ld : nullptr, x + r * x_row_stride, D, x_ld,
                              (int64_t)blockIdx.x * GMX_PICK_TILE, n, 0, tid, lane, wave, s);
  if (tid == 0) tmax[cell] = m;
  const int i = tid >> 4, j = tid & 15;
  if (i <= j) rec[cell * GMX_COV_REC + gmx_cov_tri(i, j)] = cov_entry<4>(s, 0, i, j);
}

// n > 1024, second launch: one workgroup per row
__global__ void __launch_bounds__(GMX_COV_BLOCK)
k_rows_cov_finish(const double* __restrict__ rec, const float* __restrict__ tmax, int64_t n_tiles, int32_t D,
                  double* __restrict__ out, int64_t out_ld) {
  __shared__ float lds4[4];
  __shared__ double s_scale[GMX_TP_MAX_TILES];
  __shared__ double s_g[GMX_COV_REC];
  const int tid = (int)threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x;
  const float* __restrict__ tm = tmax + r * n_tiles;
  float M = -gmx_inf();
  for (int64_t t = tid; t < n_tiles; t += GMX_COV_BLOCK) M = gmx_rmax(M, tm[t]);
  M = block_max(M, lds4);
  for (int64_t t = tid; t < n_tiles; t += GMX_COV_BLOCK) s_scale[t] = gmx_mom_tile_scale(tm[t], M);
  __syncthreads();
  if (tid < GMX_COV_REC) {
    const double* __restrict__ mine = rec + r * n_tiles * GMX_COV_REC + tid;
    double g = 0.0;
    for (int64_t b = 0; b < n_tiles; ++b) g += s_scale[b] * mine[b * GMX_COV_REC];
    s_g[tid] = g;
  }
  __syncthreads();
  const int i = tid >> 4, j = tid & 15;
  if (i <= j && j <= D)
    gmx_cov_store(s_g[0], s_g[gmx_cov_tri(0, i)], s_g[gmx_cov_tri(0, j)], s_g[gmx_cov_tri(i, j)], i, j, D, out + r * out_ld);
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)
// (`used`: emitted, and so exported by a shared library, although nothing in the translation unit calls them)

extern "C" __attribute__((used)) inline size_t gmx_rows_covariance_workspace(int64_t rows, int64_t n, int32_t D) {
  return gmx_rows_cov_bytes_(rows, n, D);
}

// the definition, literally: the Gram matrix of a row in column order
extern "C" __attribute__((used)) inline int gmx_rows_covariance(const float* lw_d, const float* carry_d, int64_t rows, int64_t n,
                                                             int64_t ld, const float* x_d, int32_t D, int64_t x_ld,
                                                             int64_t x_row_stride, double* out_d, int64_t out_ld,
                                                             void* workspace_d, gmx_stream stream) {
  (void)stream;
  const gmx_refusal no = gmx_rows_cov_refusal_(!lw_d || !out_d || !workspace_d, rows, n, ld, D, x_ld, x_row_stride, out_ld, !x_d);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_rows_covariance", no.v);
  std::vector<float> a((size_t)n);
  for (int64_t r = 0; r < rows; ++r) {
    const float M = gmx_mom_row_(lw_d + r * ld, carry_d ? carry_d + r * ld : nullptr, n, a.data());
    double G[16][16] = {}, z[16];
    z[0] = 1.0;
    for (int64_t i = 0; i < n; ++i) {
      const double e = (double)gmx_mom_weight(a[(size_t)i], M);
      for (int32_t d = 0; d < D; ++d) z[1 + d] = (double)x_d[(int64_t)d * x_ld + r * x_row_stride + i];
      for (int j = 0; j <= D; ++j)
        for (int k = j; k <= D; ++k) G[j][k] += (e * z[j]) * z[k];
    }
    for (int j = 0; j <= D; ++j)
      for (int k = j; k <= D; ++k) gmx_cov_store(G[0][0], G[0][j], G[0][k], G[j][k], j, k, D, out_d + r * out_ld);
  }
  return 0;
}
#endif
