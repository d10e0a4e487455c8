// Particle Gibbs over a bank of conditional filters (include/genmi.h "Particle Gibbs"; Andrieu, Doucet & Holenstein 2010,
// section 2.4.3): R independent chains, chain r holding (theta[:, r], the retained path of chain r of a ConditionalBank).
// One iteration j is  gmx_pg_open | the bank's conditional sweep, a draw, retain | gmx_pg_propose | the prior's log-density
// program and the T trajectory-score programs over a batch of 2R (theta on columns 0 .. R - 1, theta' on R .. 2R - 1) |
// gmx_pg_accept.  The draw synchronises, so the iteration is host-driven: j is an argument, there are no iteration words.
//   k_pg_open      k_pmmh_propose's grid and LDS scheme (gmx_pmmh.h: gmx_pmmh_span_of, gmx_pmmh_put_keys,
//                  gmx_pmmh_broadcast): one workgroup per 1024 consecutive particles, the CURRENT values of the chains its
//                  span touches parked in LDS, the bank's two or three key tables by a grid-stride loop, ONE barrier, the
//                  parameter leaves stored four entries at a time (rows_store4).
//   k_pg_propose   one thread per (parameter, chain): the pair [theta | theta'].
//   k_pg_accept    one thread per chain: the two float64 sums over the T score rows, the Metropolis-Hastings decision, the
//                  chain's state and record row, and the pinned weights ref_lw[:, r] of the parameters the next sweep runs
//                  under — column r or R + r of the observation scores, whatever the decision.  A read of row t of the
//                  [T, 2R] tables is consecutive across the chains of a wave.
// The arithmetic — the key schedule, the proposal, the sums, the decision — is stated ONCE, in the shared part below, as
// GMX_HD functions, as gmx_pmmh.h is laid out: the kernels (hipcc; included by gmx_kernels.hip only) and the ENTRY POINTS a
// plain host compiler gets (sequential loops; gmx_vm.h includes this file there) call the same ones.
#pragma once
#include "gmx_pmmh.h"                  /* the random-walk step, the step keys, the span helpers; gmx_sizes.h: the refusals */

// The keys of iteration j under the run key: k_it = fold_in(key, j); (sweep, draw, prop, acc) = split(k_it, 4)
struct gmx_pg_keys { gmx_key sweep, draw, prop, acc; };
GMX_HD gmx_pg_keys gmx_pg_iter_keys(gmx_key key, uint32_t j) {
  const gmx_key k_it = gmx_fold_in(key, j);
  gmx_pg_keys K;
  K.sweep = gmx_split_child(k_it, 0);
  K.draw = gmx_split_child(k_it, 1);
  K.prop = gmx_split_child(k_it, 2);
  K.acc = gmx_split_child(k_it, 3);
  return K;
}
// theta_pair[p, 0:R] = theta[p], theta_pair[p, R + r] = the random-walk step (at every j: the sweep ran under theta)
GMX_HD void gmx_pg_propose_one(gmx_key k_prop, const float* theta, const float* scale, int64_t R, int64_t r, int32_t p,
                               float* theta_pair) {
  const float th = theta[p * R + r];
  theta_pair[2 * p * R + r] = th;
  theta_pair[2 * p * R + R + r] = gmx_pmmh_walk(k_prop, (uint32_t)r, (uint32_t)p, th, scale[p]);
}

// What gmx_pg_accept works on (the entry point's arguments, sizes as the kernels index them)
struct gmx_pg_chains {
  const float* joint; const float* obs; const float* lp; const float* theta_pair;      // [T, 2R], [T, 2R], [2R], [P, 2R]
  int32_t T, R, P;
  float* theta; double* log_joint; float* ref_lw;                                      // [P, R], [R], [T, R]
  float* rec_theta; double* rec_lj; uint8_t* rec_acc;                                  // [cap, P, R], [cap, R], [cap, R]
};
static inline gmx_pg_chains gmx_pg_chains_of_(const float* joint_d, const float* obs_d, const float* lp_d, const float* theta_pair_d,
                                              int32_t T, int64_t R, int32_t P, float* theta_d, double* log_joint_d, float* ref_lw_d,
                                              float* rec_theta_d, double* rec_lj_d, uint8_t* rec_acc_d) {
  gmx_pg_chains C;
  C.joint = joint_d; C.obs = obs_d; C.lp = lp_d; C.theta_pair = theta_pair_d; C.T = T; C.R = (int32_t)R; C.P = P;
  C.theta = theta_d; C.log_joint = log_joint_d; C.ref_lw = ref_lw_d;
  C.rec_theta = rec_theta_d; C.rec_lj = rec_lj_d; C.rec_acc = rec_acc_d;
  return C;
}
// column c of the [T, 2R] scores summed in ascending t, in float64
GMX_HD double gmx_pg_sum(const gmx_pg_chains& C, int64_t c) {
  double acc = 0.0;
  for (int32_t t = 0; t < C.T; ++t) acc = acc + (double)C.joint[(int64_t)t * 2 * C.R + c];
  return acc;
}
// Chain r of iteration j: the decision (gmx_mh_accept's rule on the float32 log_alpha; NaN rejects), the state, row `row`
// of the record, and the pinned weights of the parameters the chain now holds
GMX_HD void gmx_pg_accept_chain(const gmx_pg_chains& C, gmx_key k_acc, int64_t row, int32_t r) {
  const int64_t R = C.R;
  const double S = gmx_pg_sum(C, r), S1 = gmx_pg_sum(C, R + r);
  const float lp = C.lp[r], lp1 = C.lp[R + r];
  const float log_alpha = (float)((S1 - S) + ((double)lp1 - (double)lp));
  const float u = gmx_uniform_sample(gmx_split_child(k_acc, (uint64_t)r), 0, 0.0f, 1.0f);
  const int take = gmx_logf(u) < log_alpha ? 1 : 0;
  const int64_t c = take ? R + r : r;
  const double lj = (take ? S1 : S) + (double)(take ? lp1 : lp);
  C.log_joint[r] = lj;
  C.rec_lj[row * R + r] = lj;
  C.rec_acc[row * R + r] = (uint8_t)take;
  for (int32_t p = 0; p < C.P; ++p) {
    const float th = C.theta_pair[2 * p * R + c];
    C.theta[p * R + r] = th;
    C.rec_theta[(row * C.P + p) * R + r] = th;
  }
  for (int32_t t = 0; t < C.T; ++t) C.ref_lw[(int64_t)t * R + r] = C.obs[(int64_t)t * 2 * R + c];
}

#if defined(__HIPCC__)

// s_val: [P, nch] floats, nch the chains the span touches (dynamic LDS, gmx_pmmh_lds_bytes_)
__global__ void __launch_bounds__(GMX_PMMH_BLOCK)
k_pg_open(uint32_t k0, uint32_t k1, uint32_t j, const float* __restrict__ theta, uint32_t P, uint32_t R, uint32_t n, uint32_t T,
          uint32_t* __restrict__ keys_prop, uint32_t* __restrict__ keys_res, uint32_t* __restrict__ keys_as,
          float* const* __restrict__ leaves) {
  extern __shared__ float s_val[];
  gmx_key key; key.k0 = k0; key.k1 = k1;
  const gmx_pg_keys K = gmx_pg_iter_keys(key, j);
  const gmx_pmmh_span S = gmx_pmmh_span_of(R, n);
  for (uint32_t q = threadIdx.x; q < S.nch * P; q += GMX_PMMH_BLOCK) {
    const uint32_t p = q / S.nch, c = q - p * S.nch;
    s_val[q] = theta[(size_t)p * R + S.r0 + c];
  }
  gmx_pmmh_put_keys(K.sweep, T, R, keys_prop, keys_res, keys_as);
  __syncthreads();
  gmx_pmmh_broadcast(s_val, S, P, n, leaves);
}

// one thread per (p, r); P * R < 2^34: 64-bit indices
__global__ void __launch_bounds__(GMX_PMMH_BLOCK)
k_pg_propose(uint32_t k0, uint32_t k1, uint32_t j, const float* __restrict__ theta, const float* __restrict__ scale, int32_t P,
             int64_t R, float* __restrict__ theta_pair) {
  const int64_t i = (int64_t)blockIdx.x * GMX_PMMH_BLOCK + threadIdx.x;
  if (i >= (int64_t)P * R) return;
  const int32_t p = (int32_t)(i / R);
  gmx_key key; key.k0 = k0; key.k1 = k1;
  gmx_pg_propose_one(gmx_pg_iter_keys(key, j).prop, theta, scale, R, i - p * R, p, theta_pair);
}

// one thread per chain
__global__ void __launch_bounds__(GMX_PMMH_BLOCK)
k_pg_accept(uint32_t k0, uint32_t k1, uint32_t j, gmx_pg_chains C, int64_t row) {
  const uint32_t r = blockIdx.x * GMX_PMMH_BLOCK + threadIdx.x;
  if (r >= (uint32_t)C.R) return;
  gmx_key key; key.k0 = k0; key.k1 = k1;
  gmx_pg_accept_chain(C, gmx_pg_iter_keys(key, j).acc, row, (int32_t)r);
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)
#include "genmi.h"

extern "C" __attribute__((used)) inline int gmx_pg_open(const uint32_t key[2], uint32_t j, const float* theta_d, int32_t P, int64_t R,
                                  int64_t n, int32_t T, uint32_t* keys_prop_d, uint32_t* keys_res_d, uint32_t* keys_as_d,
                                  float* const* leaves_d, gmx_stream stream) {
  (void)stream;
  const gmx_refusal no = gmx_pg_open_refusal_(!key || !theta_d || !keys_prop_d || !keys_res_d || !leaves_d, P, R, n, T);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_pg_open", no.v);
  for (int32_t p = 0; p < P; ++p)
    if (!leaves_d[p]) return gmx_fail("%s: null argument (a parameter leaf)", "gmx_pg_open");
  gmx_key k; k.k0 = key[0]; k.k1 = key[1];
  const gmx_pg_keys K = gmx_pg_iter_keys(k, j);
  for (int32_t p = 0; p < P; ++p)
    for (int64_t r = 0; r < R; ++r)
      for (int64_t i = 0; i < n; ++i) leaves_d[p][r * n + i] = theta_d[p * R + r];
  for (int32_t t = 0; t < T; ++t)
    for (int64_t r = 0; r < R; ++r) {
      gmx_key kp, kr, ka;
      gmx_pmmh_step_keys(K.sweep, (uint32_t)r, (uint32_t)t, &kp, &kr, &ka);
      const int64_t at = 2 * ((int64_t)t * R + r);
      keys_prop_d[at] = kp.k0; keys_prop_d[at + 1] = kp.k1;
      keys_res_d[at] = kr.k0; keys_res_d[at + 1] = kr.k1;
      if (keys_as_d) { keys_as_d[at] = ka.k0; keys_as_d[at + 1] = ka.k1; }
    }
  return 0;
}

extern "C" __attribute__((used)) inline int gmx_pg_propose(const uint32_t key[2], uint32_t j, const float* theta_d, const float* scale_d,
                                     int32_t P, int64_t R, float* theta_pair_d, gmx_stream stream) {
  (void)stream;
  const gmx_refusal no = gmx_pg_propose_refusal_(!key || !theta_d || !scale_d || !theta_pair_d, P, R);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_pg_propose", no.v);
  gmx_key k; k.k0 = key[0]; k.k1 = key[1];
  const gmx_key k_prop = gmx_pg_iter_keys(k, j).prop;
  for (int32_t p = 0; p < P; ++p)
    for (int64_t r = 0; r < R; ++r) gmx_pg_propose_one(k_prop, theta_d, scale_d, R, r, p, theta_pair_d);
  return 0;
}

extern "C" __attribute__((used)) inline int gmx_pg_accept(const uint32_t key[2], uint32_t j, const float* joint_d, const float* obs_d,
                                    const float* lp_d, const float* theta_pair_d, int32_t T, int64_t R, int32_t P, float* theta_d,
                                    double* log_joint_d, float* ref_lw_d, float* rec_theta_d, double* rec_lj_d,
                                    uint8_t* rec_acc_d, int64_t row, int64_t cap, gmx_stream stream) {
  (void)stream;
  const gmx_refusal no = gmx_pg_accept_refusal_(
      !key || !joint_d || !obs_d || !lp_d || !theta_pair_d || !theta_d || !log_joint_d || !ref_lw_d || !rec_theta_d || !rec_lj_d ||
          !rec_acc_d, P, R, T, row, cap);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_pg_accept", no.v);
  const gmx_pg_chains C = gmx_pg_chains_of_(joint_d, obs_d, lp_d, theta_pair_d, T, R, P, theta_d, log_joint_d, ref_lw_d, rec_theta_d,
                                           rec_lj_d, rec_acc_d);
  gmx_key k; k.k0 = key[0]; k.k1 = key[1];
  const gmx_key k_acc = gmx_pg_iter_keys(k, j).acc;
  for (int64_t r = 0; r < R; ++r) gmx_pg_accept_chain(C, k_acc, row, (int32_t)r);
  return 0;
}
#endif
