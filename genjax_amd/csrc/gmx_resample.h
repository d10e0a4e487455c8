// gmx_resample.h — device code of the ordered (systematic / stratified) resamplers, shared by the AOT kernels
// (gmx_kernels.hip: k_offspring, k_offspring_tile, k_shard_*).  Device only.
//
// ancestor(j) = first i with cdf_i * D > P_j (128-bit integers), D = n_out * 2^23, P_j = (j * 2^23 + u_j) * total;
// P_j increases with j, so source i owns the slot range [f(cdf_{i-1}), f(cdf_i)), f(c) = #{ j : P_j < c * D }.
#pragma once
#include "gmx_block.h"
#include "gmx_rng.h"
#include "genmi.h"

struct u128 { uint64_t hi, lo; };
__device__ __forceinline__ u128 mul64(uint64_t a, uint64_t b) {
  u128 r; r.lo = a * b; r.hi = __umul64hi(a, b); return r;
}
__device__ __forceinline__ bool gt128(u128 a, u128 b) {
  return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo);
}

// P_j for the ordered kinds
__device__ __forceinline__ u128 slot_threshold(int kind, gmx_key key, uint64_t u0, int64_t j, uint64_t total) {
  uint64_t u = (kind == GMX_RESAMPLE_SYSTEMATIC) ? u0 : (uint64_t)(gmx_bits32(key, (uint64_t)j) >> 9);
  return mul64(((uint64_t)j << 23) + u, total);
}

// The exact predicate (runs for a handful of sources per launch).  Kept inline — a real call gives the kernel a
// stack (scratch), which costs more at wave launch than the code size does — so callers on the hot path take
// `kind` as a template constant: the systematic instantiation then carries no Threefry at all.
__device__ __forceinline__ int64_t slots_below_exact(int kind, gmx_key key, uint64_t u0, uint64_t c, uint64_t D,
                                                  uint64_t total, int64_t j, int64_t n_out) {
  u128 X = mul64(c, D);
  while (j > 0 && !gt128(X, slot_threshold(kind, key, u0, j - 1, total))) --j;
  while (j < n_out && gt128(X, slot_threshold(kind, key, u0, j, total))) ++j;
  return j;
}

// ---- slot ranges, fast path without branches ----
// slots_below() above decides one CDF value with nested branches and carries the exact 128-bit predicate inline;
// k_offspring_tile evaluates it five times per thread, so here the f64 estimate is straight-line code for every
// evaluation and the (rare: ~1e-7 per evaluation) "within eps of a boundary" cases are collected in a flag and
// settled afterwards by ONE rolled loop over the exact predicate.  Same answer as slots_below() in every case.
struct sb_est { int32_t j; bool near; };
template <int kind>
// uslot (stratified only, optional): slot t's 23-bit uniform read from memory (gmx_slot_uniforms wrote
// bits32(key, t) >> 9 there — on a background stream, ahead of the chain) instead of one Threefry block per evaluation.
__device__ __forceinline__ sb_est slots_below_est(gmx_key key, uint32_t u0, uint64_t c, uint64_t total,
                                                  double n_over_total, double eps, int32_t n_out,
                                                  const uint32_t* __restrict__ uslot = nullptr) {
  const double cd = __builtin_fma((double)(uint32_t)(c >> 32), 4294967296.0, (double)(uint32_t)c);   // exact product, one rounding
  sb_est r;
  if (kind == GMX_RESAMPLE_SYSTEMATIC) {
    // slot j is below iff j + du < v  <=>  j < v - du: the count is floor(v - du) + 1 (v - du not an integer;
    // within eps of one, the exact predicate decides).  y = v - du + 1 > 0 comes out of ONE fma.
    const double y = __builtin_fma(cd, n_over_total, 1.0 - (double)u0 * (1.0 / 8388608.0));
    const int32_t t = (int32_t)y;                // floor (y > 0), saturating
    const double frac = y - (double)t;
    r.j = t < n_out ? t : n_out;
    r.near = (frac < eps) || (frac > 1.0 - eps);
    return r;
  }
  const double v = cd * n_over_total;
  int32_t t = (int32_t)v;                        // floor (v >= 0), saturating
  t = t < n_out - 1 ? t : n_out - 1;
  const double frac = v - (double)t;
  const uint32_t u = uslot ? uslot[t] : (gmx_bits32(key, (uint64_t)(uint32_t)t) >> 9);
  const double diff = frac - (double)u * (1.0 / 8388608.0);
  r.j = t + (diff > 0.0 ? 1 : 0);
  r.near = (frac < eps) || (frac > 1.0 - eps) || !(__builtin_fabs(diff) > eps);
  if (c == 0ull) { r.j = 0; r.near = false; }
  if (c >= total) { r.j = n_out; r.near = false; }
  return r;
}

// The edge settle.  R[c]: the estimate for the CDF value cv[c] — cv[0] at the lower edge of the thread's first source,
// cv[c] at the upper edge of its source c - 1.  e[0 .. 4], settled: e[1 .. 4] are the thread's own; its lower edge e[0] is
// the upper edge of the lane below (the same CDF value), so only lane 0 uses R[0] — what R[0] holds in the other lanes does
// not matter.  The (rare) flagged evaluations go through exact(c_value, j0) in ONE rolled loop, its operands picked by
// selects, and a corrected upper edge is handed to the next lane a second time.  (gmx_offspring.h writes the same out.)
template <class Exact>
__device__ __forceinline__ void gmx_edge_settle(const sb_est R[CDF_VEC + 1], const uint64_t cv[CDF_VEC + 1], int lane,
                                                Exact exact, int32_t e[CDF_VEC + 1]) {
  uint32_t near_bits = 0;
#pragma unroll
  for (int c = 1; c <= CDF_VEC; ++c) {
    e[c] = R[c].j;
    near_bits |= R[c].near ? (1u << c) : 0u;
  }
  {
    const sb_est r = R[0];
    near_bits |= (lane == 0 && r.near) ? 1u : 0u;
    e[0] = (int32_t)wave_shr1_u32((uint32_t)e[CDF_VEC], (uint32_t)r.j);
    if (lane == 0) e[0] = r.j;
  }
  if (__any(near_bits != 0u)) {          // cold
    int32_t fixed0 = e[0];
#pragma unroll 1
    for (int c = 0; c <= CDF_VEC; ++c) {
      if (near_bits & (1u << c)) {
        const uint64_t cc = c == 0 ? cv[0] : c == 1 ? cv[1] : c == 2 ? cv[2] : c == 3 ? cv[3] : cv[4];
        const int32_t j0 = c == 0 ? e[0] : c == 1 ? e[1] : c == 2 ? e[2] : c == 3 ? e[3] : e[4];
        const int32_t j = exact(cc, j0);
        if (c == 0) fixed0 = j; else if (c == 1) e[1] = j; else if (c == 2) e[2] = j; else if (c == 3) e[3] = j; else e[4] = j;
      }
    }
    const uint32_t up = wave_shr1_u32((uint32_t)e[CDF_VEC], (uint32_t)fixed0);
    e[0] = (lane == 0) ? fixed0 : (int32_t)up;
  }
}

// inclusive max-scan of u32 over the wave (the fill below)
__device__ __forceinline__ uint32_t gmx_wave_umax_scan(uint32_t v) {
#define GMX_OP(CTRL) "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 " CTRL "\n\t"
  asm(GMX_DPP_ASM_ENTER GMX_DPP_ASM_STEPS(GMX_OP) : "+v"(v));
#undef GMX_OP
  return v;
}

// ---- the fill through LDS ----
// Sources own consecutive, ascending ranges of entries (slots of a tile; guide entries of the sorted table).  Every source
// with an entry writes its mark at its first one, a max-scan fills the rest (marks increase with the entry; an empty one is
// 0), and the workgroup gets 8 consecutive entries per thread: the same cost whatever the ranges (a thread writing its own
// sources' entries in a loop diverges over their lengths: measured 2688 -> 34 us for N(0, 4) log-weights).  A pass covers
// RS_FILL_SLOTS entries; a tile owning more takes more passes (workgroup-uniform).
#define RS_FILL_SLOTS 2048             /* entries filled per pass (8 per thread): a tile owns ~1024 */
__device__ __forceinline__ void gmx_fill_zero(uint32_t* s_mark) {
  reinterpret_cast<uint4*>(s_mark)[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
  reinterpret_cast<uint4*>(s_mark)[threadIdx.x + GMX_BLOCK] = make_uint4(0u, 0u, 0u, 0u);
}
// One pass, called by every thread of the workgroup: the thread's source c marks its entries [lo[c], hi[c]) with mark0 + c;
// a / b: the filled entries base + 8 tid .. + 3 / + 4 .. + 7.  LDS: s_mark[RS_FILL_SLOTS] (16-byte aligned), s_carry[4].
// Barriers: the FIRST pass finds s_mark zeroed behind a barrier of the caller's (gmx_fill_zero; the callers share that
// barrier with something else they publish); a later one (`again`) zeroes it itself, and needs no barrier in front of
// that: every read of s_mark in a pass precedes that pass's carry barrier, which every thread has left by then.  s_carry
// is read behind the carry barrier and written next behind the two barriers of the following pass.
__device__ __forceinline__ void gmx_fill_pass(int32_t base, bool again, const int32_t lo[CDF_VEC], const int32_t hi[CDF_VEC],
                                              uint32_t mark0, uint32_t* s_mark, uint32_t* s_carry, uint4& a, uint4& b) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);      // in a scalar register: the carry selects are scalar
  if (again) {
    gmx_fill_zero(s_mark);
    __syncthreads();
  }
  // a source's first entry inside this pass (clipped at `base`: a range that began in an earlier pass continues at 0)
#pragma unroll
  for (int c = 0; c < CDF_VEC; ++c) {
    const int32_t l = lo[c] > base ? lo[c] : base;
    if (hi[c] > l && l - base < RS_FILL_SLOTS) s_mark[l - base] = mark0 + (uint32_t)c;
  }
  __syncthreads();
  a = reinterpret_cast<const uint4*>(s_mark)[2 * threadIdx.x];
  b = reinterpret_cast<const uint4*>(s_mark)[2 * threadIdx.x + 1];
  a.y = a.y > a.x ? a.y : a.x; a.z = a.z > a.y ? a.z : a.y; a.w = a.w > a.z ? a.w : a.z;
  b.x = b.x > a.w ? b.x : a.w; b.y = b.y > b.x ? b.y : b.x; b.z = b.z > b.y ? b.z : b.y; b.w = b.w > b.z ? b.w : b.z;
  const uint32_t incl = gmx_wave_umax_scan(b.w);
  uint32_t carry = wave_shr1_u32(incl, 0u);
  if (lane == 63) s_carry[wave] = incl;
  __syncthreads();                       // the carry barrier
#pragma unroll
  for (int w = 0; w < GMX_BLOCK / GMX_WAVE - 1; ++w) { const uint32_t v = s_carry[w]; carry = (w < wave_s && v > carry) ? v : carry; }
  a.x = a.x > carry ? a.x : carry; a.y = a.y > carry ? a.y : carry; a.z = a.z > carry ? a.z : carry; a.w = a.w > carry ? a.w : carry;
  b.x = b.x > carry ? b.x : carry; b.y = b.y > carry ? b.y : carry; b.z = b.z > carry ? b.z : carry; b.w = b.w > carry ? b.w : carry;
}
