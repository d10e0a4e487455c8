// Weighted moments of many independent rows (include/genmi.h "Row-wise weighted moments": gmx_rows_moments): per row r of a
// [rows, n] matrix of log-weights (plus, optionally, a second matrix `carry` — ONE float32 add, the one gmx_resample_rows_ess
// performs, so the moments are those of exactly the weights that resampler acts on) and a struct-of-arrays [D, x_ld] state
// store addressed as gmx_rows_pin addresses it, with M the row's maximum (gmx_rmax) and e_i = (double) exp(a_i - M) taken in
// float32 (gmx_mom_weight below: device and host compute the same e_i bit for bit):
//     S0 = sum e_i    S2 = sum e_i^2    A_d = sum e_i x_{d,i}    B_d = sum e_i x_{d,i}^2          (all sums in float64)
//     out[r, 0] = S0^2 / S2 (ESS)    out[r, 1 + d] = A_d / S0    out[r, 1 + D + d] = max(B_d / S0 - (A_d / S0)^2, 0)
// A row without mass (S0 = 0: no finite weight) writes ESS = 0 and NaN means and variances.  Nothing is written into the
// inputs.  The summation order is fixed — a thread's four columns in order, a wave butterfly, the waves in order, the tiles
// in order — so a row's result depends on n alone, not on rows, the grid or the row's position.
//   n <= 1024   k_rows_moments_small<W>: ONE launch, no workspace traffic.  The packing of rows_small_body
//               (gmx_resample_rows.h): a thread holds 4 consecutive columns (one 16-byte load), a row takes W = 1, 2 or 4
//               waves and a 256-thread workgroup holds 4 / W rows.  The weight, carry and first state loads are issued before
//               the first wait; the row's maximum goes through a wave reduction and 4 LDS words; e stays in registers (4
//               doubles) for the whole kernel; component d + 1 is loaded before component d is reduced.
//   n > 1024    k_rows_moments_part, one workgroup per (row, tile of 1024 columns): the tile's own maximum m_b and its sums
//               relative to it — m_b and 2 + 2 D doubles per (row, tile) into the workspace (a tile with no finite weight:
//               zeros and m_b = -inf); then k_rows_moments_finish, one workgroup per row: M = max_b m_b, the tiles in
//               ascending order under s_b = exp(m_b - M) (s_b^2 for S2), threads strided over the <= 2048 tiles.  s_b is
//               taken in FLOAT64 (the difference of two floats is exact there): a float32 s_b carries the rounding of
//               m_b - M, up to half an ulp of the difference — 2.4e-7 relative at a difference of 4 — on EVERY weight of
//               the tile alike, so it does not average out over the row as the per-weight roundings do (measured on the
//               device with a float32 s_b: 1.95e-7 on the ESS of a two-tile row, against 3.1e-8 for the one-tile form).
//               exp(fl(a - m_b)) exp(m_b - M) is still not the definition's exp(fl(a - M)) bit for bit — the float32
//               subtraction rounds elsewhere — so the tiled form is held to the float64 reference with a tolerance, not
//               bit for bit to the definition the one-tile form follows.
// THE REDUCTION (mom_reduce, all three kernels and gmx_lag.h's at C = 8): the D + 1 pairs — (S0, S2), then (A_d, B_d) —
// are handed over by a pair_of callback and reduced in batches of C = GMX_MOM_C = 16 pairs, the writer's results going to
// an emit callback (a tile's record, or mom_row_out: the row's outputs): each wave sums a pair across its lanes by
// cross-lane moves and lane 0 parks it in LDS; ONE barrier per batch; one thread of the row's group then adds the W waves
// in order and writes the batch's outputs.  The
// batches alternate between two LDS buffers, so the writer reads batch k while the waves fill batch k + 1 and no second
// barrier is needed.  C by LDS budget: a buffer is 4 waves x 2 C doubles, 2 x 1 KB for C = 16 — far below what would limit
// the eight 256-thread workgroups a CU can hold (160 KB / 8), while D <= 15 (every state this project's sweeps carry) still
// finishes in one batch; a larger C only buys fewer barriers for D >= 16.
// Under hipcc: the kernels, included by gmx_kernels.hip only (not among the headers embedded for hiprtc).  Under a plain
// host compiler: the ENTRY POINTS as a sequential loop over rows implementing the definition literally, sums in column
// order, with the same refusals (gmx_sizes.h); gmx_vm.h includes this file there.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "gmx_math.h"

// e_i as a float: exp(a - M) in float32, 0 where a - M is NaN (a = M = -inf, a NaN weight, a = M = +inf) — the entries the
// resamplers' fixed-point weights count as nothing
GMX_HD float gmx_mom_weight(float a, float M) {
  const float d = a - M;
  return d == d ? gmx_expf_nonpos(d) : 0.0f;
}
// row r's outputs from its sums: the ESS, then (mean, var) per component
GMX_HD double gmx_mom_ess(double S0, double S2) { return S0 > 0.0 ? S0 * S0 / S2 : 0.0; }
GMX_HD void gmx_mom_mean_var(double S0, double A, double B, double* mean, double* var) {
  const double m = S0 > 0.0 ? A / S0 : (double)gmx_nan();
  const double v = S0 > 0.0 ? B / S0 - m * m : (double)gmx_nan();
  *mean = m;
  *var = v < 0.0 ? 0.0 : v;                              // (false for NaN)
}

// a tile's scale s_b = exp(m_b - M) in FLOAT64 (the header says why); 0 for a tile without mass under a row without
// (-inf - -inf)
GMX_HD double gmx_mom_tile_scale(float m_b, float M) {
  const double dm = (double)m_b - (double)M;
  return dm == dm ? exp(dm) : 0.0;
}

#if defined(__HIPCC__)
#include "gmx_backward.h"              /* gmx_sizes.h, gmx_block.h, pick_load4, pick1_put_max */

#define GMX_MOM_BLOCK 256
#define GMX_MOM_C 16                   /* pairs of sums per barrier */
static_assert(GMX_TP_MAX_TILES == 8 * GMX_MOM_BLOCK, "k_rows_moments_finish holds a thread's scale factors in 8 registers");

// sum of a double over the wave, to every lane: the butterfly (its order is part of the definition)
__device__ __forceinline__ double mom_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, GMX_WAVE);
  return v;
}
// lw + carry, ONE float32 add per column, written as the instruction: left to the compiler, the four adds of a thread are
// paired into packed adds, which the chain's kernels are kept free of (third accounting); the same bits
__device__ __forceinline__ float mom_add(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// four consecutive state words of a row, columns base .. base + 3; columns >= n read as 0 (their weight is 0)
__device__ __forceinline__ void mom_load4(const float* __restrict__ row, int64_t base, int64_t n, float x[4]) {
  pick_load4(row, base, n, x);
#pragma unroll
  for (int c = 0; c < 4; ++c) x[c] = (base + c < n) ? x[c] : 0.0f;
}
// a thread's share of (S0, S2) and of (A_d, B_d): its four columns in order
__device__ __forceinline__ void mom_pair0(const double e[4], double& u, double& v) {
  u = ((e[0] + e[1]) + e[2]) + e[3];
  v = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3];
}
__device__ __forceinline__ void mom_pair(const double e[4], const float x[4], double& u, double& v) {
  double p[4], q[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double xc = (double)x[c];
    p[c] = e[c] * xc;
    q[c] = e[c] * (xc * xc);                             // (xc^2 is exact in float64)
  }
  u = ((p[0] + p[1]) + p[2]) + p[3];
  v = ((q[0] + q[1]) + q[2]) + q[3];
}

// P pairs of sums of a row held by waves grp * W .. grp * W + W - 1, C pairs per barrier: every thread calls
// pair_of(p, u, v) for p = 0 .. P - 1 in order (its share of pair p); `writer`, the one thread of the group that adds the
// waves in order, calls emit(p, u, v) in the same order.  Every thread of the workgroup calls it (the header says why one
// barrier per batch is enough).
template <int W, int C, class F, class O>
__device__ __forceinline__ void mom_reduce(int32_t P, F pair_of, O emit, int grp, int lane, int wave, bool writer) {
  __shared__ double s_buf[2][4][2 * C];
  int k = 0;
  for (int32_t p0 = 0; p0 < P; p0 += C, k ^= 1) {
    const int32_t p1 = p0 + C < P ? p0 + C : P;
    for (int32_t p = p0; p < p1; ++p) {
      double u, v;
      pair_of(p, u, v);
      u = mom_wave_sum(u);
      v = mom_wave_sum(v);
      if (lane == 0) {
        s_buf[k][wave][2 * (p - p0)] = u;
        s_buf[k][wave][2 * (p - p0) + 1] = v;
      }
    }
    __syncthreads();
    if (!writer) continue;
    for (int32_t p = p0; p < p1; ++p) {
      double u = s_buf[k][grp * W][2 * (p - p0)], v = s_buf[k][grp * W][2 * (p - p0) + 1];
#pragma unroll
      for (int w = 1; w < W; ++w) {
        u += s_buf[k][grp * W + w][2 * (p - p0)];
        v += s_buf[k][grp * W + w][2 * (p - p0) + 1];
      }
      emit(p, u, v);
    }
  }
}

// THE WEIGHT HEAD of a one-tile kernel, after the caller has issued its loads: a (+ cy when with_carry: mom_add), the W
// wave maxima through s_max [4], ONE barrier — which also publishes whatever the caller wrote to LDS before the call —
// and the row's maximum M to every thread of the row's group.  Every thread of the workgroup calls it.
template <int W>
__device__ __forceinline__ float mom_row_max(float a[4], const float cy[4], bool with_carry, float* s_max, int grp, int lane, int wave) {
  if (with_carry) {
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = mom_add(a[c], cy[c]);
  }
  pick1_put_max(a, s_max, lane, wave);
  __syncthreads();
  float M = s_max[grp * W];
#pragma unroll
  for (int w = 1; w < W; ++w) M = gmx_rmax(M, s_max[grp * W + w]);
  return M;
}
// ... of a tiled kernel's first launch: the tile's maximum m_b to every thread, and into *tmax_cell by thread 0
__device__ __forceinline__ float mom_tile_max(float a[4], const float cy[4], bool with_carry, float* lds4, float* tmax_cell, int tid) {
  if (with_carry) {
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = mom_add(a[c], cy[c]);
  }
  const float m = block_max(gmx_rmax(gmx_rmax(a[0], a[1]), gmx_rmax(a[2], a[3])), lds4);
  if (tid == 0) *tmax_cell = m;
  return m;
}
// a finish kernel's eight scale factors of thread tid: tiles tid, tid + 256, ... (0 past the last tile)
__device__ __forceinline__ void mom_tile_scales(const float* __restrict__ tm, int64_t n_tiles, float M, int tid, double s[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t t = (int64_t)tid + (int64_t)j * GMX_MOM_BLOCK;
    s[j] = t < n_tiles ? gmx_mom_tile_scale(tm[t], M) : 0.0;
  }
}
// the emit of a row's outputs: pair 0 is (S0, S2) -> the ESS, pair 1 + d is (A_d, B_d) -> mean and variance of component d
struct mom_row_out {
  double* dst; int32_t D; double S0;
  __device__ __forceinline__ void operator()(int32_t p, double u, double v) {
    if (p == 0) { S0 = u; dst[0] = gmx_mom_ess(u, v); }
    else gmx_mom_mean_var(S0, u, v, dst + p, dst + (int64_t)D + p);
  }
};

// n <= 1024: W waves per row, 4 / W rows per workgroup; thread gt of a row's group holds columns 4 gt .. 4 gt + 3.  Every
// thread reaches every barrier (a group past the last row works on the last row again and writes nothing).
template <int W>
__global__ void __launch_bounds__(GMX_MOM_BLOCK)
k_rows_moments_small(const float* __restrict__ lw, const float* __restrict__ carry, int64_t rows, int64_t n, int64_t ld,
                     const float* __restrict__ x, int32_t D, int64_t x_ld, int64_t x_row_stride, double* __restrict__ out,
                     int64_t out_ld) {
  static_assert(W == 1 || W == 2 || W == 4, "waves per row");
  constexpr int RPW = 4 / W, GT = 64 * W;
  __shared__ float s_max[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = tid / GT, gt = tid % GT;
  const int64_t r_ = (int64_t)blockIdx.x * RPW + grp;
  const bool live = r_ < rows;
  const int64_t r = live ? r_ : rows - 1;
  const int64_t base = (int64_t)gt * 4;
  const float* __restrict__ xrow = D > 0 ? x + r * x_row_stride : nullptr;
  float a[4], cy[4], xn[4];
  pick_load4(lw + r * ld, base, n, a);
  if (carry != nullptr) pick_load4(carry + r * ld, base, n, cy);     // (every load below is out before the first wait)
  if (D > 0) mom_load4(xrow, base, n, xn);
  const float M = mom_row_max<W>(a, cy, carry != nullptr, s_max, grp, lane, wave);
  double e[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) e[c] = (double)gmx_mom_weight(a[c], M);
  mom_reduce<W, GMX_MOM_C>(D + 1, [&](int32_t p, double& u, double& v) {
    if (p == 0) { mom_pair0(e, u, v); return; }
    float xc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) xc[c] = xn[c];
    if (p < D) mom_load4(xrow + (int64_t)p * x_ld, base, n, xn);               // (out before this component's reduction)
    mom_pair(e, xc, u, v);
  }, mom_row_out{out + r * out_ld, D, 0.0}, grp, lane, wave, live && gt == 0);
}

// n > 1024, first launch: blockIdx.x the tile, blockIdx.y the row (row0 + y); cell = r * n_tiles + b
__global__ void __launch_bounds__(GMX_MOM_BLOCK)
k_rows_moments_part(const float* __restrict__ lw, const float* __restrict__ carry, int64_t n, int64_t ld, int64_t n_tiles,
                    int64_t row0, const float* __restrict__ x, int32_t D, int64_t x_ld, int64_t x_row_stride,
                    double* __restrict__ rec, float* __restrict__ tmax) {
  __shared__ float lds4[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = row0 + (int64_t)blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * GMX_PICK_TILE + (int64_t)tid * 4;
  const int64_t cell = r * n_tiles + (int64_t)blockIdx.x;
  const float* __restrict__ xrow = D > 0 ? x + r * x_row_stride : nullptr;
  float a[4], cy[4], xn[4];
  pick_load4(lw + r * ld, base, n, a);
  if (carry != nullptr) pick_load4(carry + r * ld, base, n, cy);
  if (D > 0) mom_load4(xrow, base, n, xn);
  const float m = mom_tile_max(a, cy, carry != nullptr, lds4, tmax + cell, tid);
  double e[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) e[c] = (double)gmx_mom_weight(a[c], m);
  double* __restrict__ mine = rec + cell * (2 + 2 * (int64_t)D);
  mom_reduce<4, GMX_MOM_C>(D + 1, [&](int32_t p, double& u, double& v) {
    if (p == 0) { mom_pair0(e, u, v); return; }
    float xc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) xc[c] = xn[c];
    if (p < D) mom_load4(xrow + (int64_t)p * x_ld, base, n, xn);
    mom_pair(e, xc, u, v);
  }, [&](int32_t p, double u, double v) {
    mine[2 * (int64_t)p] = u;
    mine[2 * (int64_t)p + 1] = v;
  }, 0, lane, wave, tid == 0);
}

// n > 1024, second launch: one workgroup per row.  Thread t takes tiles t, t + 256, ... in ascending order.
__global__ void __launch_bounds__(GMX_MOM_BLOCK)
k_rows_moments_finish(const double* __restrict__ rec, const float* __restrict__ tmax, int64_t n_tiles, int32_t D,
                      double* __restrict__ out, int64_t out_ld) {
  __shared__ float lds4[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = (int64_t)blockIdx.x;
  const float* __restrict__ tm = tmax + r * n_tiles;
  float M = -gmx_inf();
  for (int64_t t = tid; t < n_tiles; t += GMX_MOM_BLOCK) M = gmx_rmax(M, tm[t]);
  M = block_max(M, lds4);
  double s[8];
  mom_tile_scales(tm, n_tiles, M, tid, s);
  const int64_t stride = 2 + 2 * (int64_t)D;
  const double* __restrict__ mine = rec + (r * n_tiles + tid) * stride;
  mom_reduce<4, GMX_MOM_C>(D + 1, [&](int32_t p, double& u, double& v) {
    u = 0.0; v = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if ((int64_t)tid + (int64_t)j * GMX_MOM_BLOCK < n_tiles) {
        const double* __restrict__ q = mine + (int64_t)j * GMX_MOM_BLOCK * stride + 2 * (int64_t)p;
        u += s[j] * q[0];
        v += (p == 0 ? s[j] * s[j] : s[j]) * q[1];
      }
    }
  }, mom_row_out{out + r * out_ld, D, 0.0}, 0, lane, wave, tid == 0);
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)
#include <vector>
#include "genmi.h"
#include "gmx_sizes.h"
// (`used`: emitted, and so exported by a shared library, although nothing in the translation unit calls them)

extern "C" __attribute__((used)) inline size_t gmx_rows_moments_workspace(int64_t rows, int64_t n, int32_t D) {
  return gmx_rows_moments_bytes_(rows, n, D);
}

// a row's a_i = lw_i (+ carry_i: ONE float32 add) into a[0 .. n), and their maximum M — how every row summary's mirror
// (gmx_rows_moments, _covariance, _quantiles, _lag_moments) starts a row
inline float gmx_mom_row_(const float* lw, const float* carry, int64_t n, float* a) {
  float M = -gmx_inf();
  for (int64_t i = 0; i < n; ++i) {
    a[i] = carry ? lw[i] + carry[i] : lw[i];
    M = gmx_rmax(M, a[i]);
  }
  return M;
}

// the definition, literally: the sums of a row in column order
extern "C" __attribute__((used)) inline int gmx_rows_moments(const float* lw_d, const float* carry_d, int64_t rows, int64_t n, int64_t ld,
                                                          const float* x_d, int32_t D, int64_t x_ld, int64_t x_row_stride,
                                                          double* out_d, int64_t out_ld, void* workspace_d, gmx_stream stream) {
  (void)stream;
  const gmx_refusal no = gmx_rows_moments_refusal_(!lw_d || !out_d || !workspace_d, rows, n, ld, D, x_ld, x_row_stride, out_ld, !x_d);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_rows_moments", no.v);
  std::vector<float> a((size_t)n);
  std::vector<double> A((size_t)D), B((size_t)D);
  for (int64_t r = 0; r < rows; ++r) {
    const float M = gmx_mom_row_(lw_d + r * ld, carry_d ? carry_d + r * ld : nullptr, n, a.data());
    double S0 = 0.0, S2 = 0.0;
    for (int32_t d = 0; d < D; ++d) A[(size_t)d] = B[(size_t)d] = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      const double e = (double)gmx_mom_weight(a[(size_t)i], M);
      S0 += e;
      S2 += e * e;
      for (int32_t d = 0; d < D; ++d) {
        const double x = (double)x_d[(int64_t)d * x_ld + r * x_row_stride + i];
        A[(size_t)d] += e * x;
        B[(size_t)d] += e * (x * x);
      }
    }
    double* out = out_d + r * out_ld;
    out[0] = gmx_mom_ess(S0, S2);
    for (int32_t d = 0; d < D; ++d) gmx_mom_mean_var(S0, A[(size_t)d], B[(size_t)d], out + 1 + d, out + 1 + D + d);
  }
  return 0;
}
#endif
