// Particle marginal Metropolis-Hastings over a bank of filters (include/genmi.h "Particle marginal Metropolis-Hastings";
// Andrieu, Doucet & Holenstein 2010, section 2.4.2): R independent chains, chain r driving filter r of a BootstrapBank.
// One iteration is  gmx_pmmh_propose | the prior's log-density program | the bank's sweep | gmx_pmmh_accept,  with the
// iteration count kept in two device words, so nothing in it reads a device value on the host.
//   k_pmmh_propose   one workgroup per 1024 consecutive particles of the flat [R * n] axis.  The (chain, parameter) draws
//                    of the chains its span touches are computed once, by the first lanes, and parked in LDS (P floats per
//                    chain, <= 32 KB); the (t, r) rows of the bank's two key tables are derived by a grid-stride loop over
//                    the same grid; ONE barrier; then each thread stores four consecutive entries of every parameter leaf,
//                    16 bytes at a time where the address allows (rows_store4).  Block 0 writes it[1] = it[0] + 1.
//   k_pmmh_accept    one thread per chain: the evidence of the chain's sweep summed in float64 over its T terms (the
//                    written-out gmx_log64 below: the same bits on the device and on a host), the Metropolis-Hastings
//                    decision, the chain's state and its record row.  Block 0 writes it[0] = it[1].
// No workgroup reads an iteration word another workgroup of the same launch writes.
// The span of a workgroup, the fill of the key tables and the broadcast through LDS are device helpers (gmx_pmmh_span_of,
// gmx_pmmh_put_keys, gmx_pmmh_broadcast) that k_pg_open of gmx_pgibbs.h, which includes this file, runs on as well.
// The arithmetic — the key schedule, the draw, gmx_log64, the evidence term, the decision — is stated ONCE, in the shared
// part below, as GMX_HD functions: the kernels (hipcc; included by gmx_kernels.hip only, not among the headers embedded
// for hiprtc) and the two ENTRY POINTS a plain host compiler gets (sequential loops over chains; gmx_vm.h includes this
// file there) call the same ones.  Both builds use -ffp-contract=off, and float64 add / mul / div and the u64 -> f64
// conversion are correctly rounded on gfx950 and on x86-64, so every decision is the same on both.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "gmx_backward.h"              /* gmx_sizes.h: GMX_PMMH_*, the refusals; under hipcc rows_store4 */
#include "gmx_dist.h"                  /* gmx_normal_sample, gmx_uniform_sample; gmx_rng.h, gmx_math.h */

GMX_HD double gmx_u2d(uint64_t u) { union { uint64_t u; double d; } c; c.u = u; return c.d; }
GMX_HD uint64_t gmx_d2u(double d) { union { uint64_t u; double d; } c; c.d = d; return c.u; }

// Natural log of an integer v >= 1 in float64, with a fixed operation sequence (no platform log: the device's and a
// host libm's differ in the last bit).  x = (double)v = 2^e m; m in [sqrt(1/2), sqrt 2) by the exponent split of the
// conversion's bits; f = m - 1 (exact), s = f / (2 + f), z = s^2:  log m = 2 s + s z (2/3 + 2/5 z + ... + 2/23 z^10),
// z <= 0.0295, the first dropped term below 2^-60 of the result; log v = e ln2_hi + ((e ln2_lo + s z Q) + 2 s), ln2_hi
// with 21 trailing zero bits (e ln2_hi is exact).  v = 1 gives +0, v = 2^k gives k ln 2 rounded once.  Measured against
// numpy's log over the totals of tests/pmmh_checks.py: DESIGN.md section 4.  v = 0 is the caller's business.
GMX_HD double gmx_log64(uint64_t v) {
  const uint64_t bits = gmx_d2u((double)v);
  const uint64_t frac = bits & 0x000FFFFFFFFFFFFFull;
  const int up = frac >= 0x0006A09E667F3BCDull;                  // m >= sqrt 2: halve it
  const double e = (double)((int32_t)(bits >> 52) - 1023 + up);
  const double m = gmx_u2d(frac | (up ? 0x3FE0000000000000ull : 0x3FF0000000000000ull));
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s;
  double q = 2.0 / 23.0;
  q = q * z + 2.0 / 21.0;
  q = q * z + 2.0 / 19.0;
  q = q * z + 2.0 / 17.0;
  q = q * z + 2.0 / 15.0;
  q = q * z + 2.0 / 13.0;
  q = q * z + 2.0 / 11.0;
  q = q * z + 2.0 / 9.0;
  q = q * z + 2.0 / 7.0;
  q = q * z + 2.0 / 5.0;
  q = q * z + 2.0 / 3.0;
  const double lo = e * 1.90821492927058770002e-10 + s * (z * q);
  return e * 6.93147180369123816490e-01 + (lo + 2.0 * s);
}

// The keys of iteration j under the run key: k_it = fold_in(key, j); (bank, prop, acc) = split(k_it, 3)
struct gmx_pmmh_keys { gmx_key bank, prop, acc; };
GMX_HD gmx_pmmh_keys gmx_pmmh_iter_keys(gmx_key key, uint32_t j) {
  const gmx_key k_it = gmx_fold_in(key, j);
  gmx_pmmh_keys K;
  K.bank = gmx_split_child(k_it, 0);
  K.prop = gmx_split_child(k_it, 1);
  K.acc = gmx_split_child(k_it, 2);
  return K;
}
// Row (t, r) of the bank's key tables under split(k_bank, R)[r] (BootstrapBank._key_tables): children 0 and 1 of the
// step key fold_in(., t); `last` given: also child 2 (ConditionalBank's ancestor draws)
GMX_HD void gmx_pmmh_step_keys(gmx_key k_bank, uint32_t r, uint32_t t, gmx_key* prop, gmx_key* res, gmx_key* last = nullptr) {
  const gmx_key k_step = gmx_fold_in(gmx_split_child(k_bank, r), t);
  *prop = gmx_split_child(k_step, 0);
  *res = gmx_split_child(k_step, 1);
  if (last) *last = gmx_split_child(k_step, 2);
}
// A random-walk step of parameter p of chain r under split(split(k_prop, R)[r], P)[p] — gmx_normal_sample: z * scale
// rounded, then + theta rounded
GMX_HD float gmx_pmmh_walk(gmx_key k_prop, uint32_t r, uint32_t p, float theta, float scale) {
  return gmx_normal_sample(gmx_split_child(gmx_split_child(k_prop, r), p), 0, theta, scale);
}
// theta'[p, r]: iteration 0 evaluates the start; after it the step
GMX_HD float gmx_pmmh_proposal(gmx_key k_prop, uint32_t j, uint32_t r, uint32_t p, float theta, float scale) {
  const float v = gmx_pmmh_walk(k_prop, r, p, theta, scale);
  return j == 0u ? theta : v;
}

// What gmx_pmmh_accept works on (the entry point's arguments, sizes as the kernels index them)
struct gmx_pmmh_chains {
  const float* maxs; const uint64_t* totals; const int32_t* flags;          // [T, R]; flags may be null
  int32_t T, R, P;
  double shift_ln2, log_n;
  const float* lp_prop; const float* theta_prop;                            // [R], [P, R]
  float* theta; double* ll; float* lp;                                      // the chains' state: [P, R], [R], [R]
  float* rec_theta; double* rec_ll; uint8_t* rec_acc;                       // [cap, P, R], [cap, R], [cap, R]
};
// (the struct from the entry point's arguments: every build fills it alike)
static inline gmx_pmmh_chains gmx_pmmh_chains_of_(const float* maxs_d, const uint64_t* totals_d, const int32_t* flags_d, int32_t T,
                                                  int64_t R, int32_t P, double shift_ln2, double log_n, const float* lp_prop_d,
                                                  float* theta_d, double* ll_d, float* lp_d, const float* theta_prop_d,
                                                  float* rec_theta_d, double* rec_ll_d, uint8_t* rec_acc_d) {
  gmx_pmmh_chains C;
  C.maxs = maxs_d; C.totals = totals_d; C.flags = flags_d; C.T = T; C.R = (int32_t)R; C.P = P;
  C.shift_ln2 = shift_ln2; C.log_n = log_n; C.lp_prop = lp_prop_d; C.theta_prop = theta_prop_d;
  C.theta = theta_d; C.ll = ll_d; C.lp = lp_d; C.rec_theta = rec_theta_d; C.rec_ll = rec_ll_d; C.rec_acc = rec_acc_d;
  return C;
}
// The evidence of chain r's sweep: the counted terms (flag set, and step T - 1 always) summed in ascending t, each
// ((ref(M) + log total) - shift ln 2) - log n in float64; -inf when a counted total is 0
GMX_HD double gmx_pmmh_evidence(const gmx_pmmh_chains& C, int32_t r) {
  double acc = 0.0;
  int dead = 0;
  for (int32_t t = 0; t < C.T; ++t) {
    const int64_t at = (int64_t)t * C.R + r;
    const int counted = C.flags == nullptr || t == C.T - 1 || C.flags[at] != 0;
    const uint64_t total = C.totals[at];
    if (!counted) continue;
    if (total == 0ull) { dead = 1; continue; }
    const double ref = (double)gmx_tile_ref(gmx_tile_exp(C.maxs[at]));
    acc = acc + (((ref + gmx_log64(total)) - C.shift_ln2) - C.log_n);
  }
  return dead ? -(double)gmx_inf() : acc;
}
// Chain r of iteration j: the decision (gmx_mh_accept's rule on the float32 log_alpha; NaN rejects), the state, and row
// `row` of the record
GMX_HD void gmx_pmmh_accept_chain(const gmx_pmmh_chains& C, gmx_key k_acc, int64_t row, int32_t r) {
  const double ll_new = gmx_pmmh_evidence(C, r);
  const double ll_old = C.ll[r];
  const float lp_new = C.lp_prop[r], lp_old = C.lp[r];
  const float log_alpha = (float)((ll_new - ll_old) + ((double)lp_new - (double)lp_old));
  const float u = gmx_uniform_sample(gmx_split_child(k_acc, (uint64_t)r), 0, 0.0f, 1.0f);
  const int take = gmx_logf(u) < log_alpha ? 1 : 0;
  const double ll = take ? ll_new : ll_old;
  C.ll[r] = ll;
  C.lp[r] = take ? lp_new : lp_old;
  C.rec_ll[row * C.R + r] = ll;
  C.rec_acc[row * C.R + r] = (uint8_t)take;
  for (int32_t p = 0; p < C.P; ++p) {
    const int64_t at = (int64_t)p * C.R + r;
    const float th = take ? C.theta_prop[at] : C.theta[at];
    C.theta[at] = th;
    C.rec_theta[(row * C.P + p) * C.R + r] = th;
  }
}

#if defined(__HIPCC__)

// What a workgroup of the span form works on — k_pmmh_propose and k_pg_open (gmx_pgibbs.h) —: blockIdx.x is the span of
// GMX_PMMH_SPAN consecutive particles of the flat [R * n] axis, chains r0 .. r0 + nch - 1 are those it touches, and the
// dynamic LDS holds [P, nch] floats (gmx_pmmh_lds_bytes_).  R * n < 2^31 and T * R < 2^31 (the refusal): 32-bit indices
// throughout.
struct gmx_pmmh_span { uint32_t N, base, r0, nch; };
__device__ __forceinline__ gmx_pmmh_span gmx_pmmh_span_of(uint32_t R, uint32_t n) {
  gmx_pmmh_span S;
  S.N = R * n;
  S.base = blockIdx.x * GMX_PMMH_SPAN;                            // < N
  const uint32_t last = S.N - S.base > GMX_PMMH_SPAN ? S.base + (GMX_PMMH_SPAN - 1) : S.N - 1;
  S.r0 = S.base / n;
  S.nch = last / n - S.r0 + 1;
  return S;
}
// the bank's key tables under k_bank, spread over the grid; keys_as (the third child's table) may be null
__device__ __forceinline__ void gmx_pmmh_put_keys(gmx_key k_bank, uint32_t T, uint32_t R, uint32_t* __restrict__ keys_prop,
                                                  uint32_t* __restrict__ keys_res, uint32_t* __restrict__ keys_as) {
  for (uint32_t i = blockIdx.x * GMX_PMMH_BLOCK + threadIdx.x; i < T * R; i += gridDim.x * GMX_PMMH_BLOCK) {
    const uint32_t t = i / R;
    gmx_key kp, kr, ka;
    gmx_pmmh_step_keys(k_bank, i - t * R, t, &kp, &kr, keys_as ? &ka : nullptr);
    reinterpret_cast<uint2*>(keys_prop)[i] = make_uint2(kp.k0, kp.k1);
    reinterpret_cast<uint2*>(keys_res)[i] = make_uint2(kr.k0, kr.k1);
    if (keys_as) reinterpret_cast<uint2*>(keys_as)[i] = make_uint2(ka.k0, ka.k1);
  }
}
// after the barrier: four consecutive particles per thread, each reading its chain's value from s_val [P, nch]
__device__ __forceinline__ void gmx_pmmh_broadcast(const float* s_val, const gmx_pmmh_span& S, uint32_t P, uint32_t n,
                                                   float* const* __restrict__ leaves) {
  const uint32_t i0 = S.base + threadIdx.x * 4u;
  if (i0 >= S.N) return;
  uint32_t c = i0 / n - S.r0;
  uint32_t rem = i0 - (c + S.r0) * n;
  uint32_t cc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cc[k] = c < S.nch ? c : S.nch - 1;                             // (past the last particle: not stored)
    if (++rem == n) { rem = 0; ++c; }
  }
  for (uint32_t p = 0; p < P; ++p) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = s_val[p * S.nch + cc[k]];
    rows_store4(leaves[p], (int64_t)i0, (int64_t)S.N, v);
  }
}

__global__ void __launch_bounds__(GMX_PMMH_BLOCK)
k_pmmh_propose(uint32_t k0, uint32_t k1, uint32_t* __restrict__ it, const float* __restrict__ theta,
               const float* __restrict__ scale, uint32_t P, uint32_t R, uint32_t n, uint32_t T, uint32_t* __restrict__ keys_prop,
               uint32_t* __restrict__ keys_res, float* const* __restrict__ leaves, float* __restrict__ theta_prop) {
  extern __shared__ float s_draw[];
  const uint32_t tid = threadIdx.x;
  const uint32_t j = it[0];
  gmx_key key; key.k0 = k0; key.k1 = k1;
  const gmx_pmmh_keys K = gmx_pmmh_iter_keys(key, j);
  const gmx_pmmh_span S = gmx_pmmh_span_of(R, n);
  // the draws of the span's chains, once per workgroup; the workgroup holding a chain's first particle stores them
  for (uint32_t q = tid; q < S.nch * P; q += GMX_PMMH_BLOCK) {
    const uint32_t p = q / S.nch, c = q - p * S.nch, r = S.r0 + c;
    const float v = gmx_pmmh_proposal(K.prop, j, r, p, theta[p * R + r], scale[p]);
    s_draw[q] = v;
    if (r * n >= S.base) theta_prop[p * R + r] = v;
  }
  gmx_pmmh_put_keys(K.bank, T, R, keys_prop, keys_res, nullptr);
  if (blockIdx.x == 0 && tid == 0) it[1] = j + 1u;
  __syncthreads();
  gmx_pmmh_broadcast(s_draw, S, P, n, leaves);
}

// one thread per chain.  The record row is j - rec_base[0]; outside [0, cap) no chain is touched and block 0 counts the
// launch in status[0].
__global__ void __launch_bounds__(GMX_PMMH_BLOCK)
k_pmmh_accept(uint32_t k0, uint32_t k1, uint32_t* __restrict__ it, gmx_pmmh_chains C, const int64_t* __restrict__ rec_base,
              int64_t cap, unsigned long long* __restrict__ status) {
  const uint32_t next = it[1];
  const uint32_t j = next - 1u;
  const int64_t row = (int64_t)j - rec_base[0];
  const bool inside = row >= 0 && row < cap;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    it[0] = next;
    if (!inside) status[0] += 1ull;
  }
  const uint32_t r = blockIdx.x * GMX_PMMH_BLOCK + threadIdx.x;
  if (!inside || r >= (uint32_t)C.R) return;
  gmx_key key; key.k0 = k0; key.k1 = k1;
  gmx_pmmh_accept_chain(C, gmx_pmmh_iter_keys(key, j).acc, row, (int32_t)r);
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)
#include "genmi.h"
// (`used`: emitted, and so exported by a shared library, although nothing in the translation unit calls them)

extern "C" __attribute__((used)) inline int gmx_pmmh_propose(const uint32_t key[2], uint32_t* it_d, const float* theta_d, const float* scale_d,
                                       int32_t P, int64_t R, int64_t n, int32_t T, uint32_t* keys_prop_d, uint32_t* keys_res_d,
                                       float* const* leaves_d, float* theta_prop_d, gmx_stream stream) {
  (void)stream;
  const gmx_refusal no = gmx_pmmh_propose_refusal_(
      !key || !it_d || !theta_d || !scale_d || !keys_prop_d || !keys_res_d || !leaves_d || !theta_prop_d, P, R, n, T);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_pmmh_propose", no.v);
  for (int32_t p = 0; p < P; ++p)
    if (!leaves_d[p]) return gmx_fail("%s: null argument (a parameter leaf)", "gmx_pmmh_propose");
  const uint32_t j = it_d[0];
  gmx_key k; k.k0 = key[0]; k.k1 = key[1];
  const gmx_pmmh_keys K = gmx_pmmh_iter_keys(k, j);
  for (int64_t r = 0; r < R; ++r)
    for (int32_t p = 0; p < P; ++p) {
      const float v = gmx_pmmh_proposal(K.prop, j, (uint32_t)r, (uint32_t)p, theta_d[p * R + r], scale_d[p]);
      theta_prop_d[p * R + r] = v;
      for (int64_t i = 0; i < n; ++i) leaves_d[p][r * n + i] = v;
    }
  for (int32_t t = 0; t < T; ++t)
    for (int64_t r = 0; r < R; ++r) {
      gmx_key kp, kr;
      gmx_pmmh_step_keys(K.bank, (uint32_t)r, (uint32_t)t, &kp, &kr);
      const int64_t at = 2 * ((int64_t)t * R + r);
      keys_prop_d[at] = kp.k0; keys_prop_d[at + 1] = kp.k1;
      keys_res_d[at] = kr.k0; keys_res_d[at + 1] = kr.k1;
    }
  it_d[1] = j + 1u;
  return 0;
}

extern "C" __attribute__((used)) inline int gmx_pmmh_accept(const uint32_t key[2], uint32_t* it_d, const float* maxs_d, const uint64_t* totals_d,
                                      const int32_t* flags_d, int32_t T, int64_t R, int32_t P, int shift, double shift_ln2,
                                      double log_n, const float* lp_prop_d, float* theta_d, double* ll_d, float* lp_d,
                                      const float* theta_prop_d, float* rec_theta_d, double* rec_ll_d, uint8_t* rec_acc_d,
                                      const int64_t* rec_base_d, int64_t cap, int64_t* status_d, gmx_stream stream) {
  (void)stream;
  const gmx_refusal no = gmx_pmmh_accept_refusal_(
      !key || !it_d || !maxs_d || !totals_d || !lp_prop_d || !theta_d || !ll_d || !lp_d || !theta_prop_d || !rec_theta_d ||
          !rec_ll_d || !rec_acc_d || !rec_base_d || !status_d, P, R, T, shift, cap);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_pmmh_accept", no.v);
  const gmx_pmmh_chains C = gmx_pmmh_chains_of_(maxs_d, totals_d, flags_d, T, R, P, shift_ln2, log_n, lp_prop_d, theta_d, ll_d, lp_d,
                                               theta_prop_d, rec_theta_d, rec_ll_d, rec_acc_d);
  const uint32_t next = it_d[1];
  const uint32_t j = next - 1u;
  const int64_t row = (int64_t)j - rec_base_d[0];
  it_d[0] = next;
  if (row < 0 || row >= cap) { status_d[0] += 1; return 0; }
  gmx_key k; k.k0 = key[0]; k.k1 = key[1];
  const gmx_key k_acc = gmx_pmmh_iter_keys(k, j).acc;
  for (int64_t r = 0; r < R; ++r) gmx_pmmh_accept_chain(C, k_acc, row, (int32_t)r);
  return 0;
}
#endif
