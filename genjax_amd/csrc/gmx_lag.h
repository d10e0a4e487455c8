// Fixed-lag smoothed moments of many independent rows (include/genmi.h "Fixed-lag smoothed moments": gmx_rows_lag_moments):
// E[x_{t-l} | y_1..t] and its variance per row, for the lags l of [lag_lo, lag_hi], from a ring of the last L + 1 state slabs
// and ancestor tables that the call itself keeps.  ONE call per step t does three things:
//   record     step t's state words x_t and the current ancestor rows (a_{t-1}: the column of x_{t-1} each particle of x_t
//              extends; none at t = 0) are copied into slot t mod (L + 1) of hist_x [L + 1, D, hist_x_ld] and
//              hist_a [L + 1, rows, hist_a_ld];
//   walk       b_0(i) = i, b_l(i) = col(a_{t-l}[b_{l-1}(i)]) for l = 1 .. lag_hi, col(a) = a - r * index_stride clamped into
//              [0, n - 1] (gmx_lag_col: an ancestor word outside its row cannot take the walk out of the row) — the column of
//              x_{t-l} particle i descends from;
//   summarise  with e_i exactly gmx_rows_moments' weights (gmx_mom_weight of lw (+ carry) against the row's maximum: the same
//              bits), in float64 S0 = sum e_i and, per lag l in [lag_lo, lag_hi] and component d, A = sum e_i x_{t-l,d}[b_l(i)],
//              B = sum e_i x^2; gmx_mom_mean_var's mean and clamped variance go to
//              out[l * out_lag_stride + r * out_ld + d] and [... + D + d] (a signed stride: lag l can land in the record of
//              time t - l).  A row without mass writes NaN.  The empty range (0, -1) records only.
// Nothing is written into lw, carry, x or the ancestors.  The summation order is gmx_rows_moments' (a thread's four columns
// in order, a wave butterfly, the waves in order, the tiles in order): lag 0 is that kernel's mean and variance bit for bit.
//   n <= 1024   k_rows_lag_small<W>: ONE launch in the packing of k_rows_moments_small (4 consecutive columns per thread,
//               W = 1, 2 or 4 waves per row, 4 / W rows per 256-thread workgroup, always 1024 columns per workgroup).
//               ALL TABLES IN LDS, the form the sketch names first, kept because the walk then has no barrier of its own:
//               hop 1 is the thread's own ancestor words (registers), hops 2 .. lag_hi are parked once as 16-bit
//               row-relative columns, 2 KB per table of DYNAMIC LDS sized by the call's lag_hi — 14 KB in the steady state
//               of L = 8, so eight workgroups still fit a CU's 160 KB, where a static 64 KB would leave two; at most
//               31 tables = 62 KB, which with the 1 KB of the reduction stays inside the 64 KB a launch may ask for without
//               an attribute (why hop 1 stays in registers and GMX_LAG_C is 8, not gmx_moments.h's 16).  The streamed form
//               (a doubled 4 KB slab, one barrier per hop) would cost lag_hi barriers against none and was not built.
//               The weight, carry, ancestor and table loads are issued first (the tables in groups of 8: 32 registers),
//               then the D record copies.  The walk is lag_hi dependent LDS reads per particle, a thread's four chains
//               side by side; only lags in [lag_lo, lag_hi] gather state words from hist_x (lag 0: from x), the gather of
//               pair p + 1 issued before pair p is reduced.  Steady state lag_lo = lag_hi = L: L hops, D gathers, one
//               batch.  BARRIERS: 1 (the row maxima and the tables) + ceil((1 + D * lags) / 8) (mom_reduce); 0 for an
//               empty range.
//   n > 1024    k_rows_lag_part, one workgroup per (row, tile of 1024 columns): records its columns, walks through hist_a
//               in GLOBAL memory (a row's table is up to 8 MB: no LDS form), four chains side by side, and writes the tile's
//               maximum m_b and its 1 + D * lags pairs of sums relative to it into the workspace; then k_rows_lag_finish, one
//               workgroup per row, combines the tiles in ascending order under s_b = exp(m_b - M) taken in float64, as
//               k_rows_moments_finish does and for its reason.  Hop 1 reads the call's own ancestors, every further hop and
//               every gather a slot an EARLIER call wrote, so no workgroup reads what another writes in the same launch.
//               An empty range launches the first kernel alone.
// SHARED with gmx_moments.h: the weights, the weight heads, the reduction (at C = GMX_LAG_C), the tile scales, the outputs'
// arithmetic and the mirror's row head are that header's; only a pair's place, which depends on its lag, is stated here.
// Under hipcc: the kernels, included by gmx_kernels.hip only (not among the headers embedded for hiprtc).  Under a plain
// host compiler: the ENTRY POINTS as a sequential loop over rows implementing the definition literally, sums in column
// order, with the same refusals (gmx_sizes.h); gmx_vm.h includes this file there.
#pragma once
#include "gmx_moments.h"               /* gmx_mom_weight, gmx_mom_mean_var; under hipcc the helpers listed above */

// the row-relative column an ancestor word of row offset `off` names, clamped into the row
GMX_HD int32_t gmx_lag_col(int32_t a, int64_t off, int64_t n) {
  const int64_t c = (int64_t)a - off;
  return (int32_t)(c < 0 ? 0 : (c >= n ? n - 1 : c));
}
// the ring slot of step tau >= 0
GMX_HD int64_t gmx_lag_slot(int64_t tau, int32_t L) { return tau % ((int64_t)L + 1); }

#if defined(__HIPCC__)

#define GMX_LAG_BLOCK 256
#define GMX_LAG_C 8                    /* pairs of sums per barrier: 2 buffers x 4 waves x 16 doubles = 1 KB */
#define GMX_LAG_TABLE_BYTES (GMX_PICK_TILE * 2)
static_assert(GMX_PICK_TILE == 4 * GMX_LAG_BLOCK && GMX_PICK_TILE <= 65536, "a workgroup holds one tile; a column fits 16 bits");
static_assert((GMX_ROWS_LAG_MAX - 1) * GMX_LAG_TABLE_BYTES + 2 * 4 * 2 * GMX_LAG_C * 8 + 16 <= 65536, "the tables and the reduction in 64 KB");
static_assert(GMX_TP_MAX_TILES == 8 * GMX_LAG_BLOCK, "k_rows_lag_finish holds a thread's scale factors in 8 registers");

// four consecutive ancestor words of a row, columns base .. base + 3; columns >= n read as 0
__device__ __forceinline__ void lag_load4i(const int32_t* row, int64_t base, int64_t n, int32_t v[4]) {
  if (base + 4 <= n && (((uintptr_t)(row + base)) & 15u) == 0u) {
    const int4 q = *reinterpret_cast<const int4*>(row + base);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = (base + c < n) ? row[base + c] : 0;
  }
}

// What a thread carries along its four chains: the columns b_cur of its particles, advanced lag by lag.  hop(h, b) moves the
// four columns through table h; the pairs are visited in order, so the walk only ever goes forward.
struct lag_walk {
  int32_t b[4];
  int32_t cur, l, d;                   // the lag b stands at; the (lag, component) of the next pair to gather
};
// the state words of pair (w.l, w.d) at the thread's four chains into xg (0 for a column >= n), then the pair after it
template <class H>
__device__ __forceinline__ void lag_gather(lag_walk& w, H hop, const float* __restrict__ x, int64_t x_ld, const float* hist_x,
                                           int64_t hx_ld, int64_t row_off, int32_t D, int64_t t, int32_t L, const bool in[4],
                                           float xg[4]) {
  while (w.cur < w.l) hop(++w.cur, w.b);
  const float* src = w.l == 0 ? x + (int64_t)w.d * x_ld + row_off
                              : hist_x + (gmx_lag_slot(t - w.l, L) * D + w.d) * hx_ld + row_off;
#pragma unroll
  for (int c = 0; c < 4; ++c) xg[c] = in[c] ? src[w.b[c]] : 0.0f;
  if (++w.d == D) { w.d = 0; ++w.l; }
}
// the writer's place for pair p >= 1 of a row: (lag, component) counted as the pairs come
struct lag_place { int32_t l, d; double S0; };

// step t's state words and ancestor words of columns base .. base + 3 of row r into the rings' slot (a0: loaded by the caller)
__device__ __forceinline__ void lag_record(const float* __restrict__ xrow, int32_t D, int64_t x_ld, int64_t base, int64_t n,
                                           float* hx_row, int64_t hx_ld, int32_t* ha_row, const int32_t a0[4], bool has_anc) {
  if (has_anc) rows_store4<int32_t>(ha_row, base, n, a0);
#pragma unroll 4
  for (int32_t d = 0; d < D; ++d) {
    float xd[4];
    mom_load4(xrow + (int64_t)d * x_ld, base, n, xd);
    rows_store4<float>(hx_row + (int64_t)d * hx_ld, base, n, xd);
  }
}

// n <= 1024: W waves per row, 4 / W rows per workgroup; thread gt of a row's group holds columns 4 gt .. 4 gt + 3.  Every
// thread reaches every barrier (a group past the last row works on the last row again and writes nothing).
template <int W>
__global__ void __launch_bounds__(GMX_LAG_BLOCK)
k_rows_lag_small(const float* __restrict__ lw, const float* __restrict__ carry, int64_t rows, int64_t n, int64_t ld,
                 const float* __restrict__ x, int32_t D, int64_t x_ld, int64_t x_row_stride, const int32_t* __restrict__ anc,
                 int64_t a_ld, int64_t index_stride, int64_t t, int32_t L, int32_t lag_lo, int32_t lag_hi, float* hist_x,
                 int64_t hx_ld, int32_t* hist_a, int64_t ha_ld, double* __restrict__ out, int64_t out_ld, int64_t out_lag_stride) {
  static_assert(W == 1 || W == 2 || W == 4, "waves per row");
  constexpr int RPW = 4 / W, GT = 64 * W;
  extern __shared__ __attribute__((aligned(16))) uint16_t s_tab[];       // [lag_hi - 1][1024]: hops 2 .. lag_hi
  __shared__ float s_max[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = tid / GT, gt = tid % GT;
  const int64_t r_ = (int64_t)blockIdx.x * RPW + grp;
  const bool live = r_ < rows;
  const int64_t r = live ? r_ : rows - 1;
  const int64_t base = (int64_t)gt * 4, off = r * index_stride, row_off = r * x_row_stride;
  const int64_t ha_slot = rows * ha_ld, hx_slot = (int64_t)D * hx_ld;
  const bool sums = lag_hi >= 0;
  float a[4], cy[4];
  int32_t a0[4] = {0, 0, 0, 0};
  if (sums) {
    pick_load4(lw + r * ld, base, n, a);
    if (carry != nullptr) pick_load4(carry + r * ld, base, n, cy);
  }
  if (anc != nullptr) lag_load4i(anc + r * a_ld, base, n, a0);
  uint16_t* tab = s_tab + grp * GT * 4;                          // the row's columns of every table
#pragma unroll 8
  for (int32_t h = 2; h <= lag_hi; ++h) {
    int32_t q[4];
    lag_load4i(hist_a + gmx_lag_slot(t - h + 1, L) * ha_slot + r * ha_ld, base, n, q);
    ushort4 c4;
    c4.x = (uint16_t)gmx_lag_col(q[0], off, n); c4.y = (uint16_t)gmx_lag_col(q[1], off, n);
    c4.z = (uint16_t)gmx_lag_col(q[2], off, n); c4.w = (uint16_t)gmx_lag_col(q[3], off, n);
    *reinterpret_cast<ushort4*>(tab + (int64_t)(h - 2) * GMX_PICK_TILE + base) = c4;
  }
  if (live)
    lag_record(x + row_off, D, x_ld, base, n, hist_x + gmx_lag_slot(t, L) * hx_slot + row_off, hx_ld,
               hist_a + gmx_lag_slot(t, L) * ha_slot + r * ha_ld, a0, anc != nullptr);
  if (!sums) return;                                             // (uniform: before any barrier)
  // (its barrier also publishes the tables written above: they stay before this call)
  const float M = mom_row_max<W>(a, cy, carry != nullptr, s_max, grp, lane, wave);
  double e[4];
  bool in[4];
  lag_walk wk;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    e[c] = (double)gmx_mom_weight(a[c], M);
    in[c] = base + c < n;
    wk.b[c] = in[c] ? (int32_t)base + c : 0;
  }
  wk.cur = 0; wk.l = lag_lo; wk.d = 0;
  auto hop = [&](int32_t h, int32_t b[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      b[c] = h == 1 ? (in[c] ? gmx_lag_col(a0[c], off, n) : 0) : (int32_t)tab[(int64_t)(h - 2) * GMX_PICK_TILE + b[c]];
  };
  const int32_t P = 1 + D * (lag_hi - lag_lo + 1);
  float xn[4];
  lag_gather(wk, hop, x, x_ld, hist_x, hx_ld, row_off, D, t, L, in, xn);
  lag_place at = {lag_lo, 0, 0.0};
  mom_reduce<W, GMX_LAG_C>(P, [&](int32_t p, double& u, double& v) {
    if (p == 0) { u = ((e[0] + e[1]) + e[2]) + e[3]; v = 0.0; return; }
    float xc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) xc[c] = xn[c];
    if (p + 1 < P) lag_gather(wk, hop, x, x_ld, hist_x, hx_ld, row_off, D, t, L, in, xn);    // (out before this pair's reduction)
    mom_pair(e, xc, u, v);
  }, [&](int32_t p, double u, double v) {
    if (p == 0) { at.S0 = u; return; }
    double* o = out + (int64_t)at.l * out_lag_stride + r * out_ld;
    gmx_mom_mean_var(at.S0, u, v, o + at.d, o + (int64_t)D + at.d);
    if (++at.d == D) { at.d = 0; ++at.l; }
  }, grp, lane, wave, live && gt == 0);
}

// n > 1024, first launch: blockIdx.x the tile, blockIdx.y the row (row0 + y); cell = r * n_tiles + b, 2 P doubles a cell
__global__ void __launch_bounds__(GMX_LAG_BLOCK)
k_rows_lag_part(const float* __restrict__ lw, const float* __restrict__ carry, int64_t rows, int64_t n, int64_t ld, int64_t n_tiles,
                int64_t row0, const float* __restrict__ x, int32_t D, int64_t x_ld, int64_t x_row_stride,
                const int32_t* __restrict__ anc, int64_t a_ld, int64_t index_stride, int64_t t, int32_t L, int32_t lag_lo,
                int32_t lag_hi, float* hist_x, int64_t hx_ld, int32_t* hist_a, int64_t ha_ld, double* __restrict__ rec,
                float* __restrict__ tmax) {
  __shared__ float lds4[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = row0 + (int64_t)blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * GMX_PICK_TILE + (int64_t)tid * 4;
  const int64_t cell = r * n_tiles + (int64_t)blockIdx.x;
  const int64_t off = r * index_stride, row_off = r * x_row_stride;
  const int64_t ha_slot = rows * ha_ld, hx_slot = (int64_t)D * hx_ld;
  const bool sums = lag_hi >= 0;
  float a[4], cy[4];
  int32_t a0[4] = {0, 0, 0, 0};
  if (sums) {
    pick_load4(lw + r * ld, base, n, a);
    if (carry != nullptr) pick_load4(carry + r * ld, base, n, cy);
  }
  if (anc != nullptr) lag_load4i(anc + r * a_ld, base, n, a0);
  lag_record(x + row_off, D, x_ld, base, n, hist_x + gmx_lag_slot(t, L) * hx_slot + row_off, hx_ld,
             hist_a + gmx_lag_slot(t, L) * ha_slot + r * ha_ld, a0, anc != nullptr);
  if (!sums) return;
  const float m = mom_tile_max(a, cy, carry != nullptr, lds4, tmax + cell, tid);
  double e[4];
  bool in[4];
  lag_walk wk;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    e[c] = (double)gmx_mom_weight(a[c], m);
    in[c] = base + c < n;
    wk.b[c] = in[c] ? (int32_t)(base + c) : 0;
  }
  wk.cur = 0; wk.l = lag_lo; wk.d = 0;
  auto hop = [&](int32_t h, int32_t b[4]) {
    const int32_t* tabh = hist_a + gmx_lag_slot(t - h + 1, L) * ha_slot + r * ha_ld;      // (h >= 2: an earlier call's slot)
    int32_t q[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = h == 1 ? a0[c] : tabh[b[c]];
#pragma unroll
    for (int c = 0; c < 4; ++c) b[c] = in[c] ? gmx_lag_col(q[c], off, n) : 0;
  };
  const int32_t P = 1 + D * (lag_hi - lag_lo + 1);
  double* __restrict__ mine = rec + cell * 2 * (int64_t)P;
  float xn[4];
  lag_gather(wk, hop, x, x_ld, hist_x, hx_ld, row_off, D, t, L, in, xn);
  mom_reduce<4, GMX_LAG_C>(P, [&](int32_t p, double& u, double& v) {
    if (p == 0) { u = ((e[0] + e[1]) + e[2]) + e[3]; v = 0.0; return; }
    float xc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) xc[c] = xn[c];
    if (p + 1 < P) lag_gather(wk, hop, x, x_ld, hist_x, hx_ld, row_off, D, t, L, in, xn);
    mom_pair(e, xc, u, v);
  }, [&](int32_t p, double u, double v) {
    mine[2 * (int64_t)p] = u;
    mine[2 * (int64_t)p + 1] = v;
  }, 0, lane, wave, tid == 0);
}

// n > 1024, second launch: one workgroup per row.  Thread t takes tiles t, t + 256, ... in ascending order.
__global__ void __launch_bounds__(GMX_LAG_BLOCK)
k_rows_lag_finish(const double* __restrict__ rec, const float* __restrict__ tmax, int64_t n_tiles, int32_t D, int32_t lag_lo,
                  int32_t lag_hi, double* __restrict__ out, int64_t out_ld, int64_t out_lag_stride) {
  __shared__ float lds4[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = (int64_t)blockIdx.x;
  const float* __restrict__ tm = tmax + r * n_tiles;
  float M = -gmx_inf();
  for (int64_t b = tid; b < n_tiles; b += GMX_LAG_BLOCK) M = gmx_rmax(M, tm[b]);
  M = block_max(M, lds4);
  double s[8];
  mom_tile_scales(tm, n_tiles, M, tid, s);
  const int32_t P = 1 + D * (lag_hi - lag_lo + 1);
  const int64_t stride = 2 * (int64_t)P;
  const double* __restrict__ mine = rec + (r * n_tiles + tid) * stride;
  lag_place at = {lag_lo, 0, 0.0};
  mom_reduce<4, GMX_LAG_C>(P, [&](int32_t p, double& u, double& v) {
    u = 0.0; v = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if ((int64_t)tid + (int64_t)j * GMX_LAG_BLOCK < n_tiles) {
        const double* __restrict__ q = mine + (int64_t)j * GMX_LAG_BLOCK * stride + 2 * (int64_t)p;
        u += s[j] * q[0];
        v += s[j] * q[1];
      }
    }
  }, [&](int32_t p, double u, double v) {
    if (p == 0) { at.S0 = u; return; }
    double* o = out + (int64_t)at.l * out_lag_stride + r * out_ld;
    gmx_mom_mean_var(at.S0, u, v, o + at.d, o + (int64_t)D + at.d);
    if (++at.d == D) { at.d = 0; ++at.l; }
  }, 0, lane, wave, tid == 0);
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)
#include <vector>
#include "genmi.h"
#include "gmx_sizes.h"

extern "C" __attribute__((used)) inline size_t gmx_rows_lag_moments_workspace(int64_t rows, int64_t n, int32_t D, int32_t L) {
  return gmx_rows_lag_bytes_(rows, n, D, L);
}

// the definition, literally: record, then per row the walk lag by lag and the sums of a lag in column order
extern "C" __attribute__((used)) inline int gmx_rows_lag_moments(
    const float* lw_d, const float* carry_d, int64_t rows, int64_t n, int64_t ld, const float* x_d, int32_t D, int64_t x_ld,
    int64_t x_row_stride, const int32_t* ancestors_d, int64_t a_ld, int64_t index_stride, int64_t t, int32_t L, int32_t lag_lo,
    int32_t lag_hi, float* hist_x_d, int64_t hist_x_ld, int32_t* hist_a_d, int64_t hist_a_ld, double* out_d, int64_t out_ld,
    int64_t out_lag_stride, void* workspace_d, gmx_stream stream) {
  (void)stream;
  const gmx_refusal no = gmx_rows_lag_moments_refusal_(!lw_d || !hist_x_d || !hist_a_d || !out_d || !workspace_d, rows, n, ld, D, x_ld,
                                                       x_row_stride, a_ld, index_stride, t, L, lag_lo, lag_hi, hist_x_ld, hist_a_ld,
                                                       out_ld, !x_d, !ancestors_d);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_rows_lag_moments", no.v);
  const int64_t ha_slot = rows * hist_a_ld, hx_slot = (int64_t)D * hist_x_ld;
  std::vector<float> a((size_t)n);
  std::vector<double> e((size_t)n);
  std::vector<int64_t> b((size_t)n);
  for (int64_t r = 0; r < rows; ++r) {
    const int64_t off = r * index_stride, row_off = r * x_row_stride;
    for (int64_t i = 0; i < n; ++i) {
      if (ancestors_d) hist_a_d[gmx_lag_slot(t, L) * ha_slot + r * hist_a_ld + i] = ancestors_d[r * a_ld + i];
      for (int32_t d = 0; d < D; ++d)
        hist_x_d[gmx_lag_slot(t, L) * hx_slot + (int64_t)d * hist_x_ld + row_off + i] = x_d[(int64_t)d * x_ld + row_off + i];
    }
    if (lag_hi < 0) continue;
    const float M = gmx_mom_row_(lw_d + r * ld, carry_d ? carry_d + r * ld : nullptr, n, a.data());
    double S0 = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      e[(size_t)i] = (double)gmx_mom_weight(a[(size_t)i], M);
      S0 += e[(size_t)i];
      b[(size_t)i] = i;
    }
    for (int32_t l = 0; l <= lag_hi; ++l) {
      const int32_t* tab = hist_a_d + gmx_lag_slot(t - l + 1, L) * ha_slot + r * hist_a_ld;       // a_{t-l}: recorded at t - l + 1
      for (int64_t i = 0; l > 0 && i < n; ++i) b[(size_t)i] = gmx_lag_col(tab[b[(size_t)i]], off, n);
      if (l < lag_lo) continue;
      double* out = out_d + (int64_t)l * out_lag_stride + r * out_ld;
      for (int32_t d = 0; d < D; ++d) {
        const float* src = hist_x_d + gmx_lag_slot(t - l, L) * hx_slot + (int64_t)d * hist_x_ld + row_off;
        double A = 0.0, B = 0.0;
        for (int64_t i = 0; i < n; ++i) {
          const double xv = (double)src[b[(size_t)i]];
          A += e[(size_t)i] * xv;
          B += e[(size_t)i] * (xv * xv);
        }
        gmx_mom_mean_var(S0, A, B, out + d, out + D + d);
      }
    }
  }
  return 0;
}
#endif
