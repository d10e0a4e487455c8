// Lag-one smoothed pair moments of many independent rows (include/genmi.h "Fixed-lag smoothed pair moments":
// gmx_rows_lag_pairs): the joint second moments of the CONSECUTIVE states x_s, x_{s+1} given y_1..t, s = t - l, for the lags l
// of [lag_lo, lag_hi], 1 <= lag_lo — the sufficient statistics of fixed-lag EM for a state-space model (Olsson, Cappe, Douc
// and Moulines 2008); for an LGSSM what the RTS smoother returns as P_{s|T} and P_{s,s+1|T}.  The call is made for step t
// AFTER gmx_rows_lag_moments has recorded step t into the rings hist_x and hist_a; it reads them and writes nothing but out.
// Per row r, with e_i exactly gmx_rows_moments' weights (gmx_mom_weight of lw (+ carry) against the row's maximum: the same
// bits) and b_l(i) the walk of gmx_lag.h (b_0(i) = i, b_l(i) = gmx_lag_col(a_{t-l}[b_{l-1}(i)]), a_{t-l} in slot t - l + 1):
//     u_i = x_{t-l}[b_l(i)]   (time s)        v_i = x_{t-l+1}[b_{l-1}(i)]   (time s + 1; both from the rings, lag 1's v too)
// and in float64, with zu = (1, u), zv = (1, v) of length 1 + D <= 16, three Gram matrices that share the operand e zu:
//     Guu = Zu^T diag(e) Zu        Guv = Zu^T diag(e) Zv        Gvv = Zv^T diag(e) Zv        S0 = Guu_00
// From them 2 D + 3 D^2 doubles at out[l * out_lag_stride + r * out_ld + ...] (a signed stride, as gmx_rows_lag_moments'):
//     [mean_s : D][mean_next : D][cov_s : D x D][cross : D x D][cov_next : D x D]
//     mean_s[j] = Guu_0,j+1 / S0     mean_next[k] = Gvv_0,k+1 / S0     cross[j][k] = Guv_j+1,k+1 / S0 - mean_s[j] mean_next[k]
// cov_s and cov_next as gmx_cov_store forms them (j <= k computed once and stored twice, the diagonal clamped at 0); cross is
// not symmetric and not clamped.  A row without mass writes NaN everywhere.  lag_lo > lag_hi: nothing is launched.
// The summation order is gmx_covariance.h's (a matrix instruction's four columns, a wave's blocks of 16 columns in order, the
// waves in order, the tiles in order): a row's result depends on n alone, and a lag's bits not on the range it came in.
// WHY A KERNEL OF ITS OWN.  gmx_lag.h reduces one component at a time (3 D^2 / 2 butterflies here); gmx_covariance.h feeds both
// operands of v_mfma_f64_16x16x4_f64 from one contiguously loaded word of the current step.  Here the operands are GATHERED
// along the walk, and A and B come from different times: per block of 16 columns and k-step, lane (c, q) supplies
//     A = e zu_c, B = zu_c -> Guu        A = e zu_c, B = zv_c -> Guv        A = e zv_c, B = zv_c -> Gvv
// three instructions into three accumulator tiles, in the layout gmx_covariance.h documents (double v of lane l holds
// C[4 v + l / 16][l mod 16]).  The 16 columns of block b of a wave are the four columns each of lanes 4 b .. 4 b + 3 (the
// packing of the walk), so lane (c, q) takes e and the two columns of its four particles from lane 4 b + q by cross-lane
// reads (ds_bpermute: no LDS space, no barrier) and gathers its words 4 bytes at a time from hist_x — lanes 1 <= c <= D only;
// c = 0 holds the constant 1, c > D holds 0.  v of lag l is u of lag l - 1: its 64 registers are kept, not gathered again.
//   n <= 1024   k_rows_pairs_small<W>: ONE launch in the packing of k_rows_lag_small (4 consecutive columns per thread, W = 1,
//               2 or 4 waves per row, 4 / W rows per 256-thread workgroup).  Phase 1 is that kernel's: the weight, carry and
//               table loads first, hop 1 the thread's own words of slot t (registers), hops 2 .. lag_hi parked in DYNAMIC LDS
//               as 16-bit row-relative columns (2 KB a table), the row's maximum through mom_row_max — whose barrier publishes
//               the tables — and a thread's four chains walked side by side.  Phase 2 per lag: the gathers of ALL of the
//               wave's (up to 16) blocks are issued before the first wait (128 VGPRs of operand words for a first lag, 64 new
//               ones after), then 3 x 4 MFMAs a block.  Phase 3 per lag: barrier, each wave parks its three tiles (6 KB) in
//               LDS, barrier, the threads of the row's group add the W waves in order and store.  LDS: the accumulators are
//               24 KB a workgroup and the tables up to 62 KB, so for ONE lag (every step but the last) the accumulators
//               REUSE the tables' space — dead after the last hop, and the first barrier of phase 3 is behind it — and a
//               launch asks for max(24 KB, 2 KB (lag_hi - 1)) <= 62 KB; for a range of lags the walk goes on after a lag's
//               Gram, the two live side by side, and the entry point cuts the range so that 2 KB (lag_hi - 1) + 24 KB stays
//               within 64 KB: lags up to 20 in one launch, each later lag (a flush with L > 20 only) in a launch of its own.
//   n > 1024    k_rows_pairs_part, one workgroup per (row, tile of 1024 columns): the walk through hist_a in GLOBAL memory as
//               k_rows_lag_part does, the body above at W = 4 relative to the tile's own maximum m_b; m_b and, per lag, the
//               upper triangles of Guu and Gvv (136 doubles each) and all of Guv (256) into the workspace.  Then
//               k_rows_pairs_finish, one workgroup per row: the tiles in ascending order under s_b = exp(m_b - M) in FLOAT64
//               (gmx_mom_tile_scale, for gmx_moments.h's reason), lag by lag.  No MFMA there.
// Under hipcc: the kernels, included by gmx_kernels.hip only (not among the headers embedded for hiprtc).  Under a plain
// host compiler: the ENTRY POINTS as a sequential loop over rows implementing the definition literally, sums in column
// order, with the same refusals (gmx_sizes.h); gmx_vm.h includes this file there.
#pragma once
#include "gmx_lag.h"                   /* gmx_lag_col, gmx_lag_slot; under hipcc lag_load4i and gmx_moments.h's weight head */
#include "gmx_covariance.h"            /* gmx_cov_tri; under hipcc cov_d4 */

// one second-moment output from its Gram entry g and the two first-moment entries ga, gb (S0 = G_00); clamp: a diagonal
GMX_HD double gmx_pairs_moment(double S0, double ga, double gb, double g, bool clamp) {
  if (!(S0 > 0.0)) return (double)gmx_nan();
  const double v = g / S0 - (ga / S0) * (gb / S0);
  return (clamp && v < 0.0) ? 0.0 : v;                           // (false for NaN)
}
// What entry (i, j), 0 <= i, j <= D, of a row's three Gram matrices writes into the row's 2 D + 3 D^2 outputs: uu, uv, vv are
// the entries (i, j); u0i, u0j = Guu_0i, Guu_0j; v0i, v0j = Gvv_0i, Gvv_0j; S0 = Guu_00.  Column 0 writes nothing.
GMX_HD void gmx_pairs_store(double S0, double u0i, double u0j, double v0i, double v0j, double uu, double uv, double vv, int i,
                            int j, int32_t D, double* out) {
  if (j == 0) return;
  const bool mass = S0 > 0.0;
  const int64_t DD = (int64_t)D * D;
  if (i == 0) {
    out[j - 1] = mass ? uu / S0 : (double)gmx_nan();
    out[(int64_t)D + j - 1] = mass ? vv / S0 : (double)gmx_nan();
    return;
  }
  double* cov_s = out + 2 * (int64_t)D;
  cov_s[DD + (int64_t)(i - 1) * D + (j - 1)] = gmx_pairs_moment(S0, u0i, v0j, uv, false);
  if (i > j) return;
  const double cs = gmx_pairs_moment(S0, u0i, u0j, uu, i == j), cn = gmx_pairs_moment(S0, v0i, v0j, vv, i == j);
  cov_s[(int64_t)(i - 1) * D + (j - 1)] = cs;
  cov_s[(int64_t)(j - 1) * D + (i - 1)] = cs;
  cov_s[2 * DD + (int64_t)(i - 1) * D + (j - 1)] = cn;
  cov_s[2 * DD + (int64_t)(j - 1) * D + (i - 1)] = cn;
}

#if defined(__HIPCC__)

#define GMX_PAIRS_BLOCK 256
static_assert(GMX_PAIRS_ACC_BYTES == 4 * 3 * 256 * 8, "three accumulator tiles per wave, four waves a workgroup");
static_assert(GMX_PAIRS_REC == 2 * GMX_COV_REC + 256, "two upper triangles and one full tile per (row, tile, lag)");
static_assert((GMX_ROWS_LAG_MAX - 1) * GMX_LAG_TABLE_BYTES + 16 <= 65536, "one lag: the accumulators reuse the tables' space");
static_assert((GMX_PAIRS_RANGE_MAX - 1) * GMX_LAG_TABLE_BYTES + GMX_PAIRS_ACC_BYTES + 16 <= 65536, "a range: tables and accumulators side by side");

// a wave's three accumulator tiles of one lag, entry (i, j) at 16 i + j
struct pairs_acc { double uu[256], uv[256], vv[256]; };

// Lane (c, q)'s operand words of the wave's blocks: for block b and k-step k the particle of lane 4 b + q's k-th chain, standing
// at column col[k] there — component c - 1 of slab `src` (hist_x at the slot of the operand's time, the row's offset added)
// for 1 <= c <= D, the constant 1 for c = 0, 0 for c > D — and 0 in every lane for a particle >= n, so that the Gram loop
// needs no mask of its own.  Every gather is a plain guarded load and
// nothing here reads a loaded register: all of them are out before the first wait.  Every lane of the wave calls it.
__device__ __forceinline__ void pairs_gather(const int32_t col[4], const float* src, int64_t hx_ld, int32_t D, int64_t w0,
                                             int64_t n, int c, int q, float z[16][4]) {
  const float* zrow = (c >= 1 && c <= D) ? src + (int64_t)(c - 1) * hx_ld : nullptr;
#pragma unroll
  for (int b = 0; b < 16; ++b) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int32_t at = __shfl(col[k], 4 * b + q, GMX_WAVE);
      const bool in = w0 + 16 * b + 4 * q + k < n;                // (a column >= n: every operand 0, the constant too)
      z[b][k] = (c == 0 && in) ? 1.0f : 0.0f;
      if (zrow != nullptr && in) z[b][k] = zrow[at];
    }
  }
}

// The three Gram matrices of one lag over the wave's columns w0 .. min(w0 + 256, n) - 1, parked in `mine`.  e: the lane's own
// four weights (its chains' particles).  Every lane of the wave calls it: the matrix instructions run with every lane.
__device__ __forceinline__ void pairs_gram(const float e[4], const float zu[16][4], const float zv[16][4], int64_t w0, int64_t n,
                                           int c, int q, pairs_acc& mine) {
  const int64_t wend = w0 + 256 < n ? w0 + 256 : n;
  cov_d4 uu = {0.0, 0.0, 0.0, 0.0}, uv = {0.0, 0.0, 0.0, 0.0}, vv = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    if (w0 + 16 * b >= wend) break;                              // (uniform over the wave)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double ek = (double)__shfl(e[k], 4 * b + q, GMX_WAVE);
      const double zuk = (double)zu[b][k], zvk = (double)zv[b][k];
      const double au = ek * zuk, av = ek * zvk;
      uu = __builtin_amdgcn_mfma_f64_16x16x4f64(au, zuk, uu, 0, 0, 0);
      uv = __builtin_amdgcn_mfma_f64_16x16x4f64(au, zvk, uv, 0, 0, 0);
      vv = __builtin_amdgcn_mfma_f64_16x16x4f64(av, zvk, vv, 0, 0, 0);
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {                                  // C[4 v + q][c] (gmx_covariance.h says why)
    mine.uu[16 * (4 * v + q) + c] = uu[v];
    mine.uv[16 * (4 * v + q) + c] = uv[v];
    mine.vv[16 * (4 * v + q) + c] = vv[v];
  }
}

// The lags lag_lo .. lag_hi of the columns col0 .. col0 + 256 W - 1 (those below n) of one row, held by waves grp * W ..
// grp * W + W - 1: per lag every wave parks its tiles in acc[wave] and done(l) is called by every thread between two
// barriers.  b: the thread's four chains at lag 0 (row-relative columns; 0 for a column >= n);
// hop(h, b) moves them through table h.  slab(tau): hist_x at step tau's slot, the row's offset added.  Every thread of the
// workgroup calls it (two barriers per lag; the first is also behind the last hop of a one-lag call, whose tables `acc` may lie in).
template <class H, class S, class O>
__device__ __forceinline__ void pairs_lags(const float e[4], int32_t b[4], H hop, S slab, int64_t hx_ld, int32_t D, int64_t t,
                                           int32_t lag_lo, int32_t lag_hi, int64_t w0, int64_t n, int lane, int wave,
                                           pairs_acc* acc, O done) {
  const int c = lane & 15, q = lane >> 4;
  float zu[16][4], zv[16][4];
  for (int32_t h = 1; h < lag_lo; ++h) hop(h, b);
  pairs_gather(b, slab(t - lag_lo + 1), hx_ld, D, w0, n, c, q, zv);        // the first lag's v: out together with its u below
  for (int32_t l = lag_lo; l <= lag_hi; ++l) {
    if (l > lag_lo) {                                            // v of lag l is u of lag l - 1 (arrived: its Gram has run)
#pragma unroll
      for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) zv[i][k] = zu[i][k];
    }
    hop(l, b);
    pairs_gather(b, slab(t - l), hx_ld, D, w0, n, c, q, zu);
    __syncthreads();                                             // lag l - 1's readers are done; a one-lag call's tables are dead
    pairs_gram(e, zu, zv, w0, n, c, q, acc[wave]);
    __syncthreads();
    done(l);
  }
}
// entry k of a tile of the row's Gram matrices: the W waves in wave order (tile: a member of pairs_acc)
template <int W>
__device__ __forceinline__ double pairs_entry(const pairs_acc* acc, double (pairs_acc::*tile)[256], int k) {
  double g = (acc[0].*tile)[k];
#pragma unroll
  for (int w = 1; w < W; ++w) g += (acc[w].*tile)[k];
  return g;
}

// n <= 1024: W waves per row, 4 / W rows per workgroup; thread gt of a row's group holds columns 4 gt .. 4 gt + 3.  Every
// thread reaches every barrier (a group past the last row works on the last row again and writes nothing).  Dynamic LDS:
// the tables of hops 2 .. lag_hi from byte 0, the accumulators from byte acc_off (0: they reuse the tables' space).
template <int W>
__global__ void __launch_bounds__(GMX_PAIRS_BLOCK)
k_rows_pairs_small(const float* __restrict__ lw, const float* __restrict__ carry, int64_t rows, int64_t n, int64_t ld, int32_t D,
                   int64_t x_row_stride, int64_t index_stride, int64_t t, int32_t L, int32_t lag_lo, int32_t lag_hi,
                   const float* __restrict__ hist_x, int64_t hx_ld, const int32_t* __restrict__ hist_a, int64_t ha_ld,
                   double* __restrict__ out, int64_t out_ld, int64_t out_lag_stride, uint32_t acc_off) {
  static_assert(W == 1 || W == 2 || W == 4, "waves per row");
  constexpr int RPW = 4 / W, GT = 64 * W;
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  __shared__ float s_max[4];
  uint16_t* s_tab = reinterpret_cast<uint16_t*>(s_dyn);         // [lag_hi - 1][1024]: hops 2 .. lag_hi
  pairs_acc* s_acc = reinterpret_cast<pairs_acc*>(s_dyn + acc_off);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave / W, gt = tid - grp * GT;
  const int64_t r_ = (int64_t)blockIdx.x * RPW + grp;
  const bool live = r_ < rows;
  const int64_t r = live ? r_ : rows - 1;
  const int64_t base = (int64_t)gt * 4, off = r * index_stride, row_off = r * x_row_stride;
  const int64_t ha_slot = rows * ha_ld, hx_slot = (int64_t)D * hx_ld;
  float a[4], cy[4];
  int32_t a0[4];
  pick_load4(lw + r * ld, base, n, a);
  if (carry != nullptr) pick_load4(carry + r * ld, base, n, cy);
  lag_load4i(hist_a + gmx_lag_slot(t, L) * ha_slot + r * ha_ld, base, n, a0);      // hop 1: what step t recorded
  uint16_t* tab = s_tab + grp * GT * 4;                          // the row's columns of every table
#pragma unroll 8
  for (int32_t h = 2; h <= lag_hi; ++h) {
    int32_t q4[4];
    lag_load4i(hist_a + gmx_lag_slot(t - h + 1, L) * ha_slot + r * ha_ld, base, n, q4);
    ushort4 c4;
    c4.x = (uint16_t)gmx_lag_col(q4[0], off, n); c4.y = (uint16_t)gmx_lag_col(q4[1], off, n);
    c4.z = (uint16_t)gmx_lag_col(q4[2], off, n); c4.w = (uint16_t)gmx_lag_col(q4[3], off, n);
    *reinterpret_cast<ushort4*>(tab + (int64_t)(h - 2) * GMX_PICK_TILE + base) = c4;
  }
  // (its barrier also publishes the tables written above)
  const float M = mom_row_max<W>(a, cy, carry != nullptr, s_max, grp, lane, wave);
  float e[4];
  int32_t b[4];
  bool in[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e[k] = gmx_mom_weight(a[k], M);                              // (a column >= n was loaded as -inf: weight 0)
    in[k] = base + k < n;
    b[k] = in[k] ? (int32_t)base + k : 0;
  }
  auto hop = [&](int32_t h, int32_t bb[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      bb[k] = h == 1 ? (in[k] ? gmx_lag_col(a0[k], off, n) : 0) : (int32_t)tab[(int64_t)(h - 2) * GMX_PICK_TILE + bb[k]];
  };
  auto slab = [&](int64_t tau) { return hist_x + gmx_lag_slot(tau, L) * hx_slot + row_off; };
  const pairs_acc* mine = s_acc + grp * W;
  pairs_lags(e, b, hop, slab, hx_ld, D, t, lag_lo, lag_hi, (int64_t)(wave - grp * W) * 256, n, lane, wave, s_acc, [&](int32_t l) {
    if (!live) return;
    const double S0 = pairs_entry<W>(mine, &pairs_acc::uu, 0);
    double* o = out + (int64_t)l * out_lag_stride + r * out_ld;
    for (int k = gt; k < 256; k += GT) {                         // entry (i, j) = (k / 16, k mod 16)
      const int i = k >> 4, j = k & 15;
      if (i > D || j > D) continue;
      gmx_pairs_store(S0, pairs_entry<W>(mine, &pairs_acc::uu, i), pairs_entry<W>(mine, &pairs_acc::uu, j),
                      pairs_entry<W>(mine, &pairs_acc::vv, i), pairs_entry<W>(mine, &pairs_acc::vv, j),
                      pairs_entry<W>(mine, &pairs_acc::uu, k), pairs_entry<W>(mine, &pairs_acc::uv, k),
                      pairs_entry<W>(mine, &pairs_acc::vv, k), i, j, D, o);
    }
  });
}

// n > 1024, first launch: blockIdx.x the tile, blockIdx.y the row (row0 + y); cell = r * n_tiles + b, nl * GMX_PAIRS_REC
// doubles a cell: per lag [Guu's triangle 136][Gvv's triangle 136][Guv 256]
__global__ void __launch_bounds__(GMX_PAIRS_BLOCK)
k_rows_pairs_part(const float* __restrict__ lw, const float* __restrict__ carry, int64_t rows, int64_t n, int64_t ld, int64_t n_tiles,
                  int64_t row0, int32_t D, int64_t x_row_stride, int64_t index_stride, int64_t t, int32_t L, int32_t lag_lo,
                  int32_t lag_hi, const float* __restrict__ hist_x, int64_t hx_ld, const int32_t* __restrict__ hist_a,
                  int64_t ha_ld, double* __restrict__ rec, float* __restrict__ tmax) {
  __shared__ pairs_acc s_acc[4];
  __shared__ float lds4[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t r = row0 + (int64_t)blockIdx.y;
  const int64_t col0 = (int64_t)blockIdx.x * GMX_PICK_TILE, base = col0 + (int64_t)tid * 4;
  const int64_t cell = r * n_tiles + (int64_t)blockIdx.x;
  const int64_t off = r * index_stride, row_off = r * x_row_stride;
  const int64_t ha_slot = rows * ha_ld, hx_slot = (int64_t)D * hx_ld;
  float a[4], cy[4];
  int32_t a0[4];
  pick_load4(lw + r * ld, base, n, a);
  if (carry != nullptr) pick_load4(carry + r * ld, base, n, cy);
  lag_load4i(hist_a + gmx_lag_slot(t, L) * ha_slot + r * ha_ld, base, n, a0);
  const float m = mom_tile_max(a, cy, carry != nullptr, lds4, tmax + cell, tid);
  float e[4];
  int32_t b[4];
  bool in[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e[k] = gmx_mom_weight(a[k], m);
    in[k] = base + k < n;
    b[k] = in[k] ? (int32_t)(base + k) : 0;
  }
  auto hop = [&](int32_t h, int32_t bb[4]) {
    const int32_t* tabh = hist_a + gmx_lag_slot(t - h + 1, L) * ha_slot + r * ha_ld;
    int32_t q4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q4[k] = h == 1 ? a0[k] : tabh[bb[k]];
#pragma unroll
    for (int k = 0; k < 4; ++k) bb[k] = in[k] ? gmx_lag_col(q4[k], off, n) : 0;
  };
  auto slab = [&](int64_t tau) { return hist_x + gmx_lag_slot(tau, L) * hx_slot + row_off; };
  const int64_t nl = (int64_t)lag_hi - lag_lo + 1;
  pairs_lags(e, b, hop, slab, hx_ld, D, t, lag_lo, lag_hi, col0 + (int64_t)wave * 256, n, lane, wave, s_acc, [&](int32_t l) {
    double* __restrict__ mine = rec + (cell * nl + (l - lag_lo)) * GMX_PAIRS_REC;
    const int i = tid >> 4, j = tid & 15;
    if (i <= j) {
      mine[gmx_cov_tri(i, j)] = pairs_entry<4>(s_acc, &pairs_acc::uu, tid);
      mine[GMX_COV_REC + gmx_cov_tri(i, j)] = pairs_entry<4>(s_acc, &pairs_acc::vv, tid);
    }
    mine[2 * GMX_COV_REC + tid] = pairs_entry<4>(s_acc, &pairs_acc::uv, tid);
  });
}

// n > 1024, second launch: one workgroup per row, lag by lag
__global__ void __launch_bounds__(GMX_PAIRS_BLOCK)
k_rows_pairs_finish(const double* __restrict__ rec, const float* __restrict__ tmax, int64_t n_tiles, int32_t D, int32_t lag_lo,
                    int32_t lag_hi, double* __restrict__ out, int64_t out_ld, int64_t out_lag_stride) {
  __shared__ float lds4[4];
  __shared__ double s_scale[GMX_TP_MAX_TILES];
  __shared__ double s_g[GMX_PAIRS_REC];
  const int tid = (int)threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x;
  const float* __restrict__ tm = tmax + r * n_tiles;
  float M = -gmx_inf();
  for (int64_t b = tid; b < n_tiles; b += GMX_PAIRS_BLOCK) M = gmx_rmax(M, tm[b]);
  M = block_max(M, lds4);
  for (int64_t b = tid; b < n_tiles; b += GMX_PAIRS_BLOCK) s_scale[b] = gmx_mom_tile_scale(tm[b], M);
  const int64_t nl = (int64_t)lag_hi - lag_lo + 1;
  const int i = tid >> 4, j = tid & 15;
  for (int32_t l = lag_lo; l <= lag_hi; ++l) {
    __syncthreads();                                             // the scales; the last lag's readers
    for (int k = tid; k < GMX_PAIRS_REC; k += GMX_PAIRS_BLOCK) {
      const double* __restrict__ mine = rec + (r * n_tiles * nl + (l - lag_lo)) * GMX_PAIRS_REC + k;
      double g = 0.0;
      for (int64_t b = 0; b < n_tiles; ++b) g += s_scale[b] * mine[b * nl * GMX_PAIRS_REC];
      s_g[k] = g;
    }
    __syncthreads();
    if (i > D || j > D) continue;
    const double* uu = s_g, * vv = s_g + GMX_COV_REC, * uv = s_g + 2 * GMX_COV_REC;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    gmx_pairs_store(uu[0], uu[gmx_cov_tri(0, i)], uu[gmx_cov_tri(0, j)], vv[gmx_cov_tri(0, i)], vv[gmx_cov_tri(0, j)],
                    uu[gmx_cov_tri(lo, hi)], uv[tid], vv[gmx_cov_tri(lo, hi)], i, j, D,
                    out + (int64_t)l * out_lag_stride + r * out_ld);
  }
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)

extern "C" __attribute__((used)) inline size_t gmx_rows_lag_pairs_workspace(int64_t rows, int64_t n, int32_t D, int32_t L) {
  return gmx_rows_pairs_bytes_(rows, n, D, L);
}

// the definition, literally: per row the walk lag by lag and the three Gram matrices of a lag in column order
extern "C" __attribute__((used)) inline int gmx_rows_lag_pairs(
    const float* lw_d, const float* carry_d, int64_t rows, int64_t n, int64_t ld, const float* x_d, int32_t D, int64_t x_ld,
    int64_t x_row_stride, int64_t index_stride, int64_t t, int32_t L, int32_t lag_lo, int32_t lag_hi, const float* hist_x_d,
    int64_t hist_x_ld, const int32_t* hist_a_d, int64_t hist_a_ld, double* out_d, int64_t out_ld, int64_t out_lag_stride,
    void* workspace_d, gmx_stream stream) {
  (void)stream; (void)x_d;
  const gmx_refusal no = gmx_rows_lag_pairs_refusal_(!lw_d || !hist_x_d || !hist_a_d || !out_d || !workspace_d, rows, n, ld, D, x_ld,
                                                     x_row_stride, index_stride, t, L, lag_lo, lag_hi, hist_x_ld, hist_a_ld, out_ld);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_rows_lag_pairs", no.v);
  if (lag_lo > lag_hi) return 0;
  const int64_t ha_slot = rows * hist_a_ld, hx_slot = (int64_t)D * hist_x_ld;
  std::vector<float> a((size_t)n);
  std::vector<double> e((size_t)n);
  std::vector<int64_t> b((size_t)n), bp((size_t)n);
  for (int64_t r = 0; r < rows; ++r) {
    const int64_t off = r * index_stride, row_off = r * x_row_stride;
    const float M = gmx_mom_row_(lw_d + r * ld, carry_d ? carry_d + r * ld : nullptr, n, a.data());
    for (int64_t i = 0; i < n; ++i) {
      e[(size_t)i] = (double)gmx_mom_weight(a[(size_t)i], M);
      b[(size_t)i] = i;
    }
    for (int32_t l = 1; l <= lag_hi; ++l) {
      const int32_t* tab = hist_a_d + gmx_lag_slot(t - l + 1, L) * ha_slot + r * hist_a_ld;       // a_{t-l}: recorded at t - l + 1
      bp = b;
      for (int64_t i = 0; i < n; ++i) b[(size_t)i] = gmx_lag_col(tab[bp[(size_t)i]], off, n);
      if (l < lag_lo) continue;
      const float* us = hist_x_d + gmx_lag_slot(t - l, L) * hx_slot + row_off;
      const float* vs = hist_x_d + gmx_lag_slot(t - l + 1, L) * hx_slot + row_off;
      double Guu[16][16] = {}, Guv[16][16] = {}, Gvv[16][16] = {}, zu[16], zv[16];
      zu[0] = zv[0] = 1.0;
      for (int64_t i = 0; i < n; ++i) {
        for (int32_t d = 0; d < D; ++d) {
          zu[1 + d] = (double)us[(int64_t)d * hist_x_ld + b[(size_t)i]];
          zv[1 + d] = (double)vs[(int64_t)d * hist_x_ld + bp[(size_t)i]];
        }
        for (int j = 0; j <= D; ++j)
          for (int k = 0; k <= D; ++k) {
            Guu[j][k] += (e[(size_t)i] * zu[j]) * zu[k];
            Guv[j][k] += (e[(size_t)i] * zu[j]) * zv[k];
            Gvv[j][k] += (e[(size_t)i] * zv[j]) * zv[k];
          }
      }
      for (int j = 0; j <= D; ++j)
        for (int k = 0; k <= D; ++k)
          gmx_pairs_store(Guu[0][0], Guu[0][j], Guu[0][k], Gvv[0][j], Gvv[0][k], Guu[j][k], Guv[j][k], Gvv[j][k], j, k, D,
                          out_d + (int64_t)l * out_lag_stride + r * out_ld);
    }
  }
  return 0;
}
#endif
