// The dense step of the marginal particle smoother (include/genmi.h "Backward smoothing": gmx_smooth_back): forward filtering,
// backward smoothing (Doucet, Godsill and Andrieu 2000) needs, per recorded step, the smoothed weights of step t + 1 carried
// through the row-normalised backward kernel — a [C, K] x softmax_rows([K, n]) product whose right factor is never stored:
//     M_k = max_i A[k, i] (gmx_rmax: a NaN is ignored)          e[k, i] = gmx_mom_weight(A[k, i], M_k)   (float32, the moments' e)
//     S_k = sum_i (double) e[k, i]                                G[c, i] (+)= sum_k u[c, k] e[k, i] / S_k      (float64)
// A: float32 logits [K, n], rows ld apart at ANY 4-byte boundary (smc._backward_logits writes rows n apart); u: float64 [C, K],
// C <= 16 (row 0 the smoothed weights v, row d the first moments v x_d); G: float64 [C, n].  A row without mass (S_k = 0: all
// -inf / NaN, or a +inf) contributes exactly nothing and is counted into *status_d.  Nothing is written into A or u.
//   k_smooth_rows<W>   pass 1, a row's M_k and 1 / S_k into the workspace.  W = 1 (n <= 1024): one wave per row, four rows a
//                      workgroup, no barrier; W = 4: one workgroup per row.  A thread holds 4 quads of columns (16 VGPRs), all
//                      four loads out before the first wait; a row longer than that batch (1024 W columns) is swept twice, the
//                      second time out of cache.  The maximum through the DPP wave reduction (wave_max), the float64 sum through
//                      mom_wave_sum's butterfly, the waves in order.
//   k_smooth_contract  pass 2, one workgroup per (strip of 64 columns, run of split_rows rows): gmx_sizes.h's plan, a function of
//                      (K, n) alone.  Per k-step of 4 rows lane l = (c, q) = (l mod 16, l / 16) issues ONE 16-byte load — row
//                      k + q, columns i0 + 4 c .. + 3, so a row of the strip is one 256-byte run (pick_load4: four 4-byte loads
//                      where the row's address does not allow it) — forms its four e and feeds them as the B operand of four
//                      v_mfma_f64_16x16x4_f64: tile t takes column i0 + 4 j + t as its column j, so that in the accumulator
//                      layout gmx_covariance.h documents double v of tile t of lane l is G[4 v + q][i0 + 4 c + t] — a lane ends
//                      with four CONSECUTIVE columns of four rows of G.  The A operand is u[c, k + q] / S_{k+q}, read with
//                      M_{k+q} from an LDS table the workgroup stages per chunk of 64 rows ([64][17] doubles: the pad keeps
//                      the coalesced fill at two lanes a bank); rows c >= C, rows past the run and columns >= n feed zeros.  The
//                      16 k-steps of a chunk go round the four waves, a wave's four loads are out before the chunk's barrier,
//                      and two tables alternate, so a chunk costs ONE barrier.  Four accumulator tiles (32 registers), no LDS
//                      traffic for A.  Then the waves' tiles through LDS (32 KB, the tables' space reused), added in wave order,
//                      each thread storing four consecutive doubles of one row of the run's partial tile.
//   k_smooth_finish    G[c, i] (+)= the runs' partial tiles in run order; its first workgroup counts the rows with 1 / S = 0 and
//                      ONE thread adds the count to *status_d.  No atomics anywhere: a result is the same bits on every run.
// Under hipcc: the kernels, included by gmx_kernels.hip only (not among the headers embedded for hiprtc).  Under a plain host
// compiler: the ENTRY POINTS implementing the definition literally, rows then columns in order, with the same refusals
// (gmx_sizes.h); gmx_vm.h includes this file there.
#pragma once
#include "gmx_covariance.h"            /* gmx_moments.h: gmx_mom_weight; under hipcc mom_wave_sum, pick_load4, cov_d4 */

#if defined(__HIPCC__)

#define GMX_SMOOTH_BLOCK 256
#define GMX_SMOOTH_TAB (GMX_SMOOTH_CHUNK * 17)          /* doubles of one staged table of u / S */
static_assert(GMX_SMOOTH_CHUNK == 64 && GMX_SMOOTH_STRIP == 64 && GMX_SMOOTH_MAX_C == 16, "16 k-steps a chunk, four tiles a strip");
static_assert(2 * GMX_SMOOTH_TAB + GMX_SMOOTH_CHUNK <= 4096, "two tables of u / S and of M inside the waves' 32 KB of tiles");

// pass 1: W waves per row, 4 / W rows per workgroup; thread gt of a row's group holds quads gt, gt + 64 W, ... of a batch
template <int W>
__global__ void __launch_bounds__(GMX_SMOOTH_BLOCK)
k_smooth_rows(const float* __restrict__ A, int64_t K, int64_t n, int64_t ld, double* __restrict__ inv, float* __restrict__ mx) {
  static_assert(W == 1 || W == 4, "a wave or the workgroup per row");
  constexpr int RPW = 4 / W, GT = 64 * W;
  __shared__ float s_max[4];
  __shared__ double s_sum[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave / W, gt = tid - grp * GT;
  const int64_t r_ = (int64_t)blockIdx.x * RPW + grp;
  const bool live = r_ < K;
  const float* __restrict__ row = A + (live ? r_ : K - 1) * ld;
  const int64_t span = (int64_t)GT * 16;
  float a[4][4];
  float m = -gmx_inf();
  for (int64_t b0 = 0; b0 < n; b0 += span) {
#pragma unroll
    for (int j = 0; j < 4; ++j) pick_load4(row, b0 + ((int64_t)j * GT + gt) * 4, n, a[j]);       // (all out before the first wait)
#pragma unroll
    for (int j = 0; j < 4; ++j) m = gmx_rmax(m, gmx_rmax(gmx_rmax(a[j][0], a[j][1]), gmx_rmax(a[j][2], a[j][3])));
  }
  float M = wave_max(m);
  if (W > 1) {
    if (lane == 0) s_max[wave] = M;
    __syncthreads();
    M = gmx_rmax(gmx_rmax(s_max[0], s_max[1]), gmx_rmax(s_max[2], s_max[3]));
  }
  double s = 0.0;
  for (int64_t b0 = 0; b0 < n; b0 += span) {
    if (n > span) {                                              // (one batch: the registers of the first sweep)
#pragma unroll
      for (int j = 0; j < 4; ++j) pick_load4(row, b0 + ((int64_t)j * GT + gt) * 4, n, a[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) s += (double)gmx_mom_weight(a[j][c], M);       // (a column >= n was loaded as -inf: 0)
  }
  double S = mom_wave_sum(s);
  if (W > 1) {
    if (lane == 0) s_sum[wave] = S;
    __syncthreads();
    S = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
  }
  if (live && gt == 0) {
    mx[r_] = M;
    inv[r_] = S > 0.0 ? 1.0 / S : 0.0;
  }
}

// pass 2: blockIdx.x the strip, blockIdx.y the run of rows; part: [runs, C, np]
__global__ void __launch_bounds__(GMX_SMOOTH_BLOCK)
k_smooth_contract(const float* __restrict__ A, int64_t K, int64_t n, int64_t ld, const double* __restrict__ u, int32_t C,
                  int64_t u_ld, const double* __restrict__ inv, const float* __restrict__ mx, int64_t split_rows, int64_t np,
                  double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double s_raw[4096];
  float* const s_m = reinterpret_cast<float*>(s_raw + 2 * GMX_SMOOTH_TAB);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int64_t i0 = (int64_t)blockIdx.x * GMX_SMOOTH_STRIP, col = i0 + 4 * c;
  const int64_t kb = (int64_t)blockIdx.y * split_rows, ke = kb + split_rows < K ? kb + split_rows : K;
  cov_d4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = cov_d4{0.0, 0.0, 0.0, 0.0};
  int b = 0;
  for (int64_t k0 = kb; k0 < ke; k0 += GMX_SMOOTH_CHUNK, b ^= 1) {
    float a[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {                                // this wave's k-steps wave, wave + 4, ... of the chunk
      const int64_t k = k0 + 4 * (wave + 4 * s) + q;
      pick_load4(A + (k < ke ? k : ke - 1) * ld, col, k < ke ? n : 0, a[s]);      // (a row past the run: -inf, nothing loaded)
    }
    double* const tab = s_raw + b * GMX_SMOOTH_TAB;
    float* const tm = s_m + b * GMX_SMOOTH_CHUNK;
    for (int idx = tid; idx < GMX_SMOOTH_MAX_C * GMX_SMOOTH_CHUNK; idx += GMX_SMOOTH_BLOCK) {
      const int cc = idx >> 6, kk = idx & 63;
      double v = 0.0;
      if (cc < C && k0 + kk < ke) {
        const double r = inv[k0 + kk];
        v = r > 0.0 ? u[(int64_t)cc * u_ld + k0 + kk] * r : 0.0;
      }
      tab[kk * 17 + cc] = v;
    }
    if (tid < GMX_SMOOTH_CHUNK) tm[tid] = k0 + tid < ke ? mx[k0 + tid] : 0.0f;
    __syncthreads();                                             // (the table two chunks back was read before the last barrier)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kk = 4 * (wave + 4 * s) + q;
      const float m = tm[kk];
      const double ua = tab[kk * 17 + c];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, (double)gmx_mom_weight(a[s][t], m), acc[t], 0, 0, 0);
    }
  }
  __syncthreads();                                               // the last table's readers are done: its space takes the tiles
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) s_raw[(wave * 16 + v * 4 + t) * 64 + lane] = acc[t][v];
  __syncthreads();
  const int cc = tid >> 4, jj = tid & 15;                        // row cc of G, columns i0 + 4 jj .. + 3: lane 16 (cc mod 4) + jj's
  if (cc >= C) return;
  const int at = ((cc >> 2) * 4) * 64 + 16 * (cc & 3) + jj;
  double* __restrict__ dst = part + ((int64_t)blockIdx.y * C + cc) * np + i0 + 4 * jj;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    double g = s_raw[at + t * 64];
#pragma unroll
    for (int w = 1; w < 4; ++w) g += s_raw[w * 1024 + at + t * 64];
    dst[t] = g;
  }
}

// the last stage: blockIdx.x the 256 columns, blockIdx.y the row of G
__global__ void __launch_bounds__(GMX_SMOOTH_BLOCK)
k_smooth_finish(const double* __restrict__ part, int64_t splits, int32_t C, int64_t n, int64_t np, double* __restrict__ G,
                int64_t g_ld, int accumulate, const double* __restrict__ inv, int64_t K, int64_t* __restrict__ status) {
  __shared__ int32_t s_dead[GMX_SMOOTH_BLOCK];
  const int tid = (int)threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * GMX_SMOOTH_BLOCK + tid, c = (int64_t)blockIdx.y;
  if (i < n) {
    double g = part[c * np + i];
    for (int64_t y = 1; y < splits; ++y) g += part[(y * C + c) * np + i];
    double* __restrict__ dst = G + c * g_ld + i;
    *dst = accumulate ? *dst + g : g;
  }
  if (blockIdx.x != 0 || blockIdx.y != 0) return;                // (uniform over the workgroup)
  int32_t dead = 0;
  for (int64_t k = tid; k < K; k += GMX_SMOOTH_BLOCK) dead += inv[k] > 0.0 ? 0 : 1;
  s_dead[tid] = dead;
  __syncthreads();
  if (tid != 0) return;
  int64_t all = 0;
  for (int t = 0; t < GMX_SMOOTH_BLOCK; ++t) all += s_dead[t];
  if (all) *status += all;
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)

extern "C" __attribute__((used)) inline size_t gmx_smooth_back_workspace(int64_t K, int64_t n, int32_t C) {
  return gmx_smooth_back_bytes_(K, n, C);
}

// the definition, literally: rows in order, then columns in order
extern "C" __attribute__((used)) inline int gmx_smooth_back(const float* A_d, int64_t K, int64_t n, int64_t ld, const double* u_d,
                                                         int32_t C, int64_t u_ld, double* G_d, int64_t g_ld, int accumulate,
                                                         int64_t* status_d, void* workspace_d, gmx_stream stream) {
  (void)stream;
  const gmx_refusal no = gmx_smooth_back_refusal_(!A_d || !u_d || !G_d || !status_d || !workspace_d, K, n, ld, C, u_ld, g_ld, u_d, G_d);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_smooth_back", no.v);
  if (!accumulate)
    for (int32_t c = 0; c < C; ++c)
      for (int64_t i = 0; i < n; ++i) G_d[c * g_ld + i] = 0.0;
  std::vector<float> e((size_t)n);
  for (int64_t k = 0; k < K; ++k) {
    const float* row = A_d + k * ld;
    float M = -gmx_inf();
    for (int64_t i = 0; i < n; ++i) M = gmx_rmax(M, row[i]);
    double S = 0.0;
    for (int64_t i = 0; i < n; ++i) S += (double)(e[(size_t)i] = gmx_mom_weight(row[i], M));
    if (!(S > 0.0)) {
      *status_d += 1;
      continue;
    }
    for (int32_t c = 0; c < C; ++c)
      for (int64_t i = 0; i < n; ++i) G_d[c * g_ld + i] += u_d[c * u_ld + k] * (double)e[(size_t)i] / S;
  }
  return 0;
}
#endif
