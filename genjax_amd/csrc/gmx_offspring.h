// gmx_offspring.h — the body of the fused ordered resampler (k_offspring_tile, gmx_kernels.hip), as a device function:
// the AOT kernel is a wrapper around it, and a specialised site program that gathers can run it FIRST, in its own launch
// (gmx_run_args.rs; TAGGED = true): a bootstrap SMC step is then ONE launch [resample step t-1 ; extend to step t].
// Device only.
#pragma once
#include "gmx_block.h"
#include "gmx_resample.h"
#include "gmx_sorted.h"

#define RS_TILE (GMX_BLOCK * CDF_VEC)   /* 1024 log-weights per tile = one definition tile of the CDF */
#define RS_MAX_TILES GMX_MAX_TILES     /* n <= 2^21                                */
static_assert(RS_TILE == GMX_TILE, "resampling tiles are the CDF's definition tiles");
static_assert(RS_MAX_TILES % GMX_BLOCK == 0, "tile table shape");

// TAGGED (a site program's prologue): every ancestor is stored as {tag: bits 24..31 | index: bits 0..23} with a
// write-through (sc1) store — the workgroups of the SAME launch that gather through these slots poll them until the tag
// is the step's (4-byte stores are single-copy atomic: the data is its own flag; no fence, no counter).
#define GMX_ANC_TAG_SHIFT 24           /* {tag: bits 24..31 | index: bits 0..23}: 16.7 M particles per launch, tags 1 .. 255 */
#define GMX_ANC_INDEX_MASK 0xffffffu
#define GMX_ANC_TAG_MAX 255u           /* (every slot is rewritten at every step: a stale word is at most one use old) */
__device__ __forceinline__ void gmx_store_u32x4_sc1(uint32_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  typedef uint32_t v4 __attribute__((ext_vector_type(4)));
  v4 v; v.x = a; v.y = b; v.z = c; v.w = d;
  asm volatile("s_nop 1\n\tglobal_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
}
// eight consecutive words at [uniform base + 32-bit byte offset]: the scalar-base form, the second half in the offset field
__device__ __forceinline__ void gmx_store_u32x8_sc1(uint32_t* base_uniform, uint32_t off, uint4 a, uint4 b) {
  typedef uint32_t v4 __attribute__((ext_vector_type(4)));
  v4 va, vb; va.x = a.x; va.y = a.y; va.z = a.z; va.w = a.w; vb.x = b.x; vb.y = b.y; vb.z = b.z; vb.w = b.w;
  asm volatile("s_nop 1\n\tglobal_store_dwordx4 %0, %1, %3 sc1\n\tglobal_store_dwordx4 %0, %2, %3 offset:16 sc1\n\ts_nop 1"
               :: "v"(off), "v"(va), "v"(vb), "s"(base_uniform) : "memory");
}
__device__ __forceinline__ void gmx_store_u32_sc1(uint32_t* p, uint32_t a) {
  __hip_atomic_store(p, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- GMX_RESAMPLE_MULTINOMIAL_SORTED: "slots below a CDF value" from the order-statistics table (csrc/gmx_sorted.h) ----
typedef uint32_t rs_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));    // 16-byte load / store at a 4-byte-aligned address
typedef uint32_t sorted_u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));   // 8-byte load at a 4-byte-aligned address
struct sorted_ctx {
  const uint32_t* slow; const uint32_t* guide; const uint64_t* toff;
  uint64_t stot, gmax; uint32_t sh, mask; double ratio;     // ratio = S_total / total; gmax = the last bucket
};
__device__ __forceinline__ sorted_ctx sorted_ctx_of(const uint32_t* table, int64_t n, uint64_t total, uint64_t stot, uint32_t sh) {
  const gmx_sorted_layout L = gmx_sorted_layout_of(n);
  sorted_ctx X;
  X.slow = table; X.guide = table + L.off_guide;
  X.toff = reinterpret_cast<const uint64_t*>(table + L.off_toff);
  X.stot = stot;              // = toff[tiles], table[off_sh]: loaded by the caller, early
  X.sh = sh;
  X.mask = (1u << X.sh) - 1u;
  X.gmax = X.stot >> X.sh;
  X.ratio = (double)X.stot / (double)(total ? total : 1ull);
  return X;
}
__device__ __forceinline__ int64_t sorted_below_exact(const sorted_ctx& X, uint64_t c, uint64_t total, int64_t j, int64_t n) {
  const u128 R = mul64(c, X.stot);
  j = j < 0 ? 0 : (j > n ? n : j);
  auto below = [&](int64_t k) {
    const uint64_t off = X.toff[k >> 10];
    const uint64_t S = off + (uint64_t)(uint32_t)(X.slow[k] - (uint32_t)off);     // S_k - off < 2^31
    return gt128(R, mul64(S, total));
  };
  while (j > 0 && !below(j - 1)) --j;
  while (j < n && below(j)) ++j;
  return j;
}

// One thread owns 4 consecutive sources (one float4 of log-weights); a workgroup of 256 threads is ONE tile.  Every
// workgroup has to turn ALL tile statistics into its prefix and the total; four consecutive tiles to a workgroup of 1024
// threads would share that pass — measured on MI355X (config 2): the kernel itself 7.8 -> 7.3 us per launch, but the
// site program that follows went 13.1 -> 14.9 us: with one tile per 256-thread block, tile j of BOTH kernels runs as
// block j, i.e. on XCD j mod 8 (blocks are dealt round-robin), so the log-weights, ancestors and states one kernel
// leaves are found in that XCD's L2 by the other; four consecutive tiles per block put three of them on another XCD.
// Every load is issued before anything waits (unconditional, clamped addresses), wave-level reductions and scans are
// DPP (gmx_block.h), the slot ranges are straight-line f64 code with one cold exact path.
// The tile's local CDF, the edge settle and the fill through LDS are written out here, in the words of gmx_tile_load4 /
// gmx_tile_fixed4 / gmx_tile_local_pos (gmx_block.h) and gmx_edge_settle / gmx_fill_pass (gmx_resample.h), which every other
// tile resampler calls: hipcc optimises a forceinline function on its own before it inlines it (sums reassociated, selects
// hoisted), and this body's schedule — the headline's — is kept instruction for instruction.  A change to one is a change
// to the other.

// a 32-bit byte offset widened in the basic block of its access, so that the access takes the [scalar base + offset] form
// (gmx_jit.h, gmx_jit_ctx::zext_here, says why the copy is needed; it emits nothing)
__device__ __forceinline__ uint64_t rs_zext_here(uint32_t o) { asm volatile("" : "+v"(o)); return (uint64_t)o; }
#define RS_WAVES (GMX_BLOCK / GMX_WAVE)
// PER: rows of the tile table a thread holds (PER * 256 >= n_tiles; 1, 2, 4 or 8 — the launch picks the smallest):
// the statistics pass is unrolled over exactly the rows that exist.
// A tile's slots [T0, T1) get their ancestors through LDS (the fill gmx_resample.h describes): the block stores 8
// consecutive slots per thread (two 16-byte stores).
template <int kind, int PER, bool TAGGED>
__device__ __forceinline__ void
gmx_offspring_tile_body(uint32_t k0, uint32_t k1, uint32_t u0_host, const float* __restrict__ lw,
                        const float* __restrict__ tmax, const uint64_t* __restrict__ agg, int64_t n, int n_tiles, float scale,
                        float* __restrict__ max_out, uint64_t* __restrict__ total_out, int32_t* __restrict__ anc,
                        const uint32_t* __restrict__ uslot, uint32_t tag,
                        int tile0 = -1, uint64_t a_prefix = 0ull, uint64_t a_total = 0ull, uint64_t a_mk = 0ull) {
  // tile0 >= 0: the tile this call works on, when it is not the workgroup's number — a LOOPED launch (gmx_jit.h,
  // GMX_JIT_RS_LOOP: more tiles than the device holds workgroups; each workgroup handles tiles blockIdx + c * gridDim).
  // PER == 0 with agg == nullptr: the tile's prefix, the total and (M, K) arrive as arguments (gmx_tile_table_pass below).
  const int blk = tile0 >= 0 ? tile0 : (int)blockIdx.x;
  const uint32_t tagw = TAGGED ? (tag << GMX_ANC_TAG_SHIFT) : 0u;
  __shared__ uint64_t s_below[RS_WAVES], s_all[RS_WAVES], s_scan[RS_WAVES];
  __shared__ float s_max[RS_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);      // the same number in a scalar register: selects on it are scalar
  // (tile_ok and full_tile are WORKGROUP-uniform: on the scalar unit)
  const bool tile_ok = blk < n_tiles;
  const int tile_c = tile_ok ? blk : n_tiles - 1;
  // (the mask tells a kernel compiled without launch bounds — a specialised site program — that 4 tid stays inside the tile)
  const int64_t i0 = (int64_t)tile_c * RS_TILE + (int64_t)(threadIdx.x & (GMX_BLOCK - 1)) * CDF_VEC;
  // ---- issue every load first ----
  float x[CDF_VEC];
  const bool full_tile = (int64_t)(tile_c + 1) * RS_TILE <= n;
  if (full_tile) {
    float4 v = *reinterpret_cast<const float4*>(lw + i0);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
#pragma unroll
    for (int c = 0; c < CDF_VEC; ++c) {
      const int64_t ic = i0 + c < n ? i0 + c : n - 1;
      const float xv = lw[ic];
      x[c] = (i0 + c < n) ? xv : -gmx_inf();
    }
  }
  // PER == 0: the tile PREFIXES are there already (`agg` = the block gmx_tile_prefix wrote): this workgroup reads its
  // own prefix, the total and (M, K) — three loads instead of a pass over the whole table.
  constexpr bool PREF = (PER == 0);
  constexpr int PERN = PREF ? 1 : PER;
  static_assert(PER >= 0 && PER * GMX_BLOCK <= RS_MAX_TILES, "rows of the tile table per thread");
  uint64_t ta[PERN];
  float tm[PERN];
  const uint32_t tid4 = threadIdx.x * 4u;
  uint64_t pf_prefix = 0, pf_total = 0, pf_mk = 0;
  if (PREF) {
    if (agg) { pf_prefix = agg[tile_c]; pf_total = agg[n_tiles]; pf_mk = agg[n_tiles + 1]; }
    else { pf_prefix = a_prefix; pf_total = a_total; pf_mk = a_mk; }
  } else {
#pragma unroll
    for (int r = 0; r < PERN; ++r) {              // loads only (clamped rows): nothing here waits
      ta[r] = 0ull; tm[r] = -gmx_inf();
      if (r * GMX_BLOCK < n_tiles) {                // uniform: rows of the table that exist
        if ((r + 1) * GMX_BLOCK <= n_tiles) {       // uniform: a whole row — [scalar base of the row] + 8 tid / 4 tid, no
          GMX_KEEP_BRANCH;                         // 64-bit vector add, compare or select per row (gmx_jit.h, gmx_jit_ctx)
          uint32_t r0 = (uint32_t)(r * GMX_BLOCK);     // (opaque, in a scalar register: the row's base is a scalar add — left
          asm volatile("" : "+s"(r0));                //  to itself hipcc adds an offset past the immediate field per lane)
          ta[r] = *reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(agg + r0) + rs_zext_here(tid4 * 2u));
          tm[r] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(tmax + r0) + rs_zext_here(tid4));
        } else {                                   // the table's last row: clamped
          const int t = r * GMX_BLOCK + (int)threadIdx.x;
          const int tc = t < n_tiles ? t : n_tiles - 1;
          ta[r] = agg[tc];
          tm[r] = tmax[tc];
        }
      }
    }
  }
  const float tmax_mine = tmax[tile_c];
  uint64_t sx_stot = 0; uint32_t sx_sh = 0;             // the sorted kind's table header (uniform), with the other early loads
  if constexpr (kind == GMX_RESAMPLE_MULTINOMIAL_SORTED) {
    const gmx_sorted_layout L = gmx_sorted_layout_of(n);
    sx_stot = reinterpret_cast<const uint64_t*>(uslot + L.off_toff)[L.tiles];
    sx_sh = uslot[L.off_sh];
  }
  __builtin_amdgcn_sched_barrier(0);
  if (!PREF) {
#pragma unroll
    for (int r = 0; r < PERN; ++r) {
      // only the table's last row can run past n_tiles (uniform): the others keep what they loaded (a row that does
      // not exist holds 0 / -inf from above)
      if (r * GMX_BLOCK < n_tiles && (r + 1) * GMX_BLOCK > n_tiles) {
        GMX_KEEP_BRANCH;
        const int t = r * GMX_BLOCK + (int)threadIdx.x;
        ta[r] = (t < n_tiles) ? ta[r] : 0ull;
        tm[r] = (t < n_tiles) ? tm[r] : -gmx_inf();
      }
    }
  }
  const int32_t k_b = gmx_tile_exp(tmax_mine);
  const float ref_b = gmx_tile_ref(k_b);
  // phase 1: the global max, and the wave totals of each tile's local weights
  float M = -gmx_inf();
  if (PREF) {
    M = gmx_u2f((uint32_t)pf_mk);
  } else {
#pragma unroll
    for (int r = 0; r < PERN; ++r)
      if (r * GMX_BLOCK < n_tiles) M = gmx_rmax(M, tm[r]);
    M = wave_max(M);
  }
  uint64_t q[CDF_VEC];
  uint64_t run = 0;
#pragma unroll
  for (int c = 0; c < CDF_VEC; ++c) q[c] = weight_fixed(x[c], ref_b, scale);
  if (!(tile_ok && full_tile)) {          // wave-uniform: a full tile has no lane to mask, so no compares and selects
    GMX_KEEP_BRANCH;
#pragma unroll
    for (int c = 0; c < CDF_VEC; ++c) q[c] = (tile_ok && i0 + c < n) ? q[c] : 0ull;
  }
#pragma unroll
  for (int c = 0; c < CDF_VEC; ++c) {
    run += q[c];
    q[c] = run;
  }
  const uint64_t inc = wave_scan_u64(run);
  if (!PREF && lane == 0) s_max[wave] = M;
  if (lane == 63) s_scan[wave] = inc;
  __syncthreads();
  if (!PREF) {
    M = s_max[0];
#pragma unroll
    for (int w = 1; w < RS_WAVES; ++w) M = gmx_rmax(M, s_max[w]);
  }
  uint64_t wave_off = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) wave_off += (w < (wave_s & 3)) ? s_scan[w] : 0ull;   // the tile's own four waves
  const uint64_t loc = wave_off + (inc - run);          // tile-local mass before this thread's sources
  // phase 2: G_t = A_t * 2^(k_t - K) for every tile -> the mass before this block's tile, and the total
  const int32_t K = PREF ? (int32_t)(uint32_t)(pf_mk >> 32) : gmx_tile_exp(M);
  uint64_t prefix = 0, total = 0;
  if (PREF) {
    prefix = pf_prefix; total = pf_total;
  } else {
    uint64_t below = 0, all = 0;
#pragma unroll
    for (int r = 0; r < PERN; ++r) {
      if (r * GMX_BLOCK < n_tiles) {
        const int t = r * GMX_BLOCK + (int)threadIdx.x;
        const uint64_t G = gmx_tile_scale(ta[r], gmx_tile_exp(tm[r]), K);
        all += G;
        // workgroup-uniform: a row wholly in front of this block's tile counts whole, a row wholly at or behind it not
        // at all — only the row `blk` lies in compares per lane (sums of u64: any order, same integers)
        if ((r + 1) * GMX_BLOCK <= blk) { GMX_KEEP_BRANCH; below += G; }
        else if (r * GMX_BLOCK < blk) { GMX_KEEP_BRANCH; below += (t < blk) ? G : 0ull; }
      }
    }
    wave_sum2_u64(below, all);
    if (lane == 0) { s_below[wave] = below; s_all[wave] = all; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) { prefix += s_below[w]; total += s_all[w]; }
  }
  if (blk == 0 && threadIdx.x == 0) { *total_out = total; *max_out = M; }
  if (!tile_ok) return;                                  // a tile past the end (workgroup-uniform)
  gmx_key key; key.k0 = k0; key.k1 = k1;
  if (total == 0) {       // no mass at all (all weights -inf / NaN): every slot maps to the last particle
#pragma unroll
    for (int c = 0; c < CDF_VEC; ++c)
      if (i0 + c < n) {
        if (TAGGED) gmx_store_u32_sc1(reinterpret_cast<uint32_t*>(anc) + (i0 + c), (uint32_t)(n - 1) | tagw);
        else anc[i0 + c] = (int32_t)(n - 1);
      }
    return;
  }
  const double n_over_total = (double)n / (double)total;
  const double eps = (double)n * 0x1p-44 + 0x1p-40;
  const int32_t n32 = (int32_t)n;
  // CDF values at the lower edge of the thread's first source and at the upper edge of each source
  uint64_t cv[CDF_VEC + 1];
  cv[0] = prefix + gmx_tile_scale(loc, k_b, K);
#pragma unroll
  for (int c = 0; c < CDF_VEC; ++c) cv[c + 1] = prefix + gmx_tile_scale(loc + q[c], k_b, K);
  if (!full_tile) {                       // (wave-uniform, as above)
    GMX_KEEP_BRANCH;
#pragma unroll
    for (int c = 0; c < CDF_VEC; ++c) cv[c + 1] = (i0 + c < n) ? cv[c + 1] : total;
  }
  int32_t e[CDF_VEC + 1];
  constexpr bool SORTED = (kind == GMX_RESAMPLE_MULTINOMIAL_SORTED);      // `uslot` is the order-statistics table
  sorted_ctx SX;
  if constexpr (SORTED) SX = sorted_ctx_of(uslot, n, total, sx_stot, sx_sh);
  auto below_est = [&](uint64_t c) -> sb_est {
    return slots_below_est<kind == GMX_RESAMPLE_MULTINOMIAL_SORTED ? GMX_RESAMPLE_SYSTEMATIC : kind>(
        key, u0_host, c, total, n_over_total, eps, n32, uslot);              // (never called for the sorted kind)
  };
  sb_est R[CDF_VEC + 1];
  if constexpr (SORTED) {
    // the evaluations side by side: every guide read issued before any is used, then every slot probe — written one
    // evaluation after the other, the (rare) walk past the probed slots orders the loads: ten dependent round trips.
    // (cv[0]: only wave 0 evaluates its own — see below)
    uint32_t mv[CDF_VEC + 1], gv[CDF_VEC + 1], lov[CDF_VEC + 1], hiv[CDF_VEC + 1], kv[CDF_VEC + 1];
    auto eval = [&](const int c0, const int c1) {
#pragma unroll
      for (int c = c0; c <= c1; ++c) {
        const double cd = __builtin_fma((double)(uint32_t)(cv[c] >> 32), 4294967296.0, (double)(uint32_t)cv[c]);
        const double t = cd * SX.ratio;
        const uint64_t tq = (uint64_t)t;
        const double frac = t - (double)tq;
        const double teps = __builtin_fma(t, 0x1p-49, 0x1p-40);
        R[c].near = (frac < teps) || (frac > 1.0 - teps);
        const uint64_t gq = tq >> SX.sh;
        gv[c] = (uint32_t)(gq < SX.gmax ? gq : SX.gmax);      // (t within rounding of S_total: entries past gmax + 1 are not defined)
        mv[c] = (uint32_t)tq & SX.mask;
      }
#pragma unroll
      for (int c = c0; c <= c1; ++c) {
        const sorted_u32x2_a4 gh = *reinterpret_cast<const sorted_u32x2_a4*>(SX.guide + gv[c]);
        lov[c] = gh.x; hiv[c] = gh.y;
      }
#pragma unroll
      for (int c = c0; c <= c1; ++c) {
        hiv[c] = hiv[c] < (uint32_t)n32 ? hiv[c] : (uint32_t)n32;
        lov[c] = lov[c] < hiv[c] ? lov[c] : hiv[c];
      }
      rs_u32x4_a4 pa[CDF_VEC + 1], pb[CDF_VEC + 1];
#pragma unroll
      for (int c = c0; c <= c1; ++c) {        // eight slots per evaluation (past slot n - 1: still inside the table, not counted)
        pa[c] = *reinterpret_cast<const rs_u32x4_a4*>(SX.slow + lov[c]);
        pb[c] = *reinterpret_cast<const rs_u32x4_a4*>(SX.slow + lov[c] + 4u);
      }
      bool more = false;
#pragma unroll
      for (int c = c0; c <= c1; ++c) {        // the slots of a bucket ascend: the count of "<= m" is the count of leading ones
        const uint32_t pv[8] = {pa[c].x, pa[c].y, pa[c].z, pa[c].w, pb[c].x, pb[c].y, pb[c].z, pb[c].w};
        uint32_t k = lov[c];
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) k += (lov[c] + i < hiv[c] && (pv[i] & SX.mask) <= mv[c]) ? 1u : 0u;
        kv[c] = k;
        more |= (k == lov[c] + 8u && k < hiv[c]);
      }
      if (more) {                              // a bucket with more than eight slots below t: once in ~1e5 evaluations
#pragma unroll 1
        for (int c = c0; c <= c1; ++c) {
          uint32_t k = kv[c];
          if (k == lov[c] + 8u)
            while (k < hiv[c] && (SX.slow[k] & SX.mask) <= mv[c]) ++k;
          kv[c] = k;
        }
      }
#pragma unroll
      for (int c = c0; c <= c1; ++c) {
        R[c].j = (int32_t)kv[c];
        if (cv[c] == 0ull) { R[c].j = 0; R[c].near = false; }
        if (cv[c] >= total) { R[c].j = n32; R[c].near = false; }
      }
    };
    R[0].j = 0; R[0].near = false;
    eval(1, CDF_VEC);
    if (wave == 0) eval(0, 0);
  } else {
#pragma unroll
    for (int c = 1; c <= CDF_VEC; ++c) R[c] = below_est(cv[c]);
    R[0].j = 0; R[0].near = false;
    if (__builtin_amdgcn_readfirstlane(wave) == 0) R[0] = below_est(cv[0]);        // wave-uniform: a scalar branch
  }
  // lower bound of the thread's first source (cv[0]) = upper bound of the previous thread's last one (its cv[4]): lanes take
  // it from their neighbour below (gmx_edge_settle), lane 0 of waves 1 .. 3 from the wave before through LDS (s_edge:
  // published after the cold path, so a corrected value travels; read behind the barrier that precedes the slot fill), and
  // only lane 0 of wave 0 uses an evaluation of its own (the tile's first edge)
  bool near = false;
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
  near = near_bits != 0u;
  if (__any(near)) {
    // cold: the exact integer predicate for the flagged evaluations (rolled; operands picked by selects)
    const uint64_t D = (uint64_t)n << 23;
    int32_t fixed0 = e[0];
#pragma unroll 1
    for (int c = 0; c <= CDF_VEC; ++c) {
      if (near_bits & (1u << c)) {
        const uint64_t cc = c == 0 ? cv[0] : c == 1 ? cv[1] : c == 2 ? cv[2] : c == 3 ? cv[3] : cv[4];
        const int32_t j0 = c == 0 ? e[0] : c == 1 ? e[1] : c == 2 ? e[2] : c == 3 ? e[3] : e[4];
        int32_t j;
        if constexpr (SORTED) j = (int32_t)sorted_below_exact(SX, cc, total, (int64_t)j0, n);
        else j = (int32_t)slots_below_exact(kind, key, (uint64_t)u0_host, cc, D, total, (int64_t)j0, n);
        if (c == 0) fixed0 = j; else if (c == 1) e[1] = j; else if (c == 2) e[2] = j; else if (c == 3) e[3] = j; else e[4] = j;
      }
    }
    // a corrected upper bound is the next lane's lower bound
    const uint32_t up = wave_shr1_u32((uint32_t)e[CDF_VEC], (uint32_t)fixed0);
    e[0] = (lane == 0) ? fixed0 : (int32_t)up;
  }
  __shared__ int32_t s_edge[RS_WAVES];
  if (lane == 63) s_edge[wave] = e[CDF_VEC];      // the (settled) upper edge of this wave, for lane 0 of the next
  // Sources past n have e[c] = n = e of the last real source, so they own no slot.
  const int32_t e4 = e[4];
  // the marks carry the step's tag already: (src0 + c) | tagw == src0t + c (the index field cannot carry into bit 24), every
  // compared mark has the same tag and an empty one is 0, so the max-scan gives the tagged maxima and no store ORs anything
  const uint32_t src0t = (uint32_t)(int32_t)i0 | tagw;
  __shared__ __attribute__((aligned(16))) uint32_t s_mark[RS_FILL_SLOTS];
  __shared__ int32_t s_rng[2];
  __shared__ uint32_t s_carry[RS_WAVES];
  if (threadIdx.x == 0) s_rng[0] = e[0];
  if (threadIdx.x == GMX_BLOCK - 1) s_rng[1] = e4;
  gmx_fill_zero(s_mark);
  __syncthreads();                       // the first pass's zeroes, T0 and T1, s_edge
  if (lane == 0 && wave > 0) e[0] = s_edge[wave - 1];
  const int32_t T0 = __builtin_amdgcn_readfirstlane(s_rng[0]), T1 = __builtin_amdgcn_readfirstlane(s_rng[1]);
  for (int32_t base = T0; base < T1; base += RS_FILL_SLOTS) {      // block-uniform trip count (1 unless the tile owns > 2048 slots)
    if (base != T0) {
      gmx_fill_zero(s_mark);
      __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < CDF_VEC; ++c) {
      const int32_t lo = e[c] > base ? e[c] : base;
      if (e[c + 1] > lo && lo - base < RS_FILL_SLOTS) s_mark[lo - base] = src0t + (uint32_t)c;
    }
    __syncthreads();
    uint4 a = reinterpret_cast<const uint4*>(s_mark)[2 * threadIdx.x];
    uint4 b = reinterpret_cast<const uint4*>(s_mark)[2 * threadIdx.x + 1];
    a.y = a.y > a.x ? a.y : a.x; a.z = a.z > a.y ? a.z : a.y; a.w = a.w > a.z ? a.w : a.z;
    b.x = b.x > a.w ? b.x : a.w; b.y = b.y > b.x ? b.y : b.x; b.z = b.z > b.y ? b.z : b.y; b.w = b.w > b.z ? b.w : b.z;
    const uint32_t incl = gmx_wave_umax_scan(b.w);
    uint32_t carry = wave_shr1_u32(incl, 0u);
    if (lane == 63) s_carry[wave] = incl;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < RS_WAVES - 1; ++w) { const uint32_t v = s_carry[w]; carry = (w < wave_s && v > carry) ? v : carry; }
    a.x = a.x > carry ? a.x : carry; a.y = a.y > carry ? a.y : carry; a.z = a.z > carry ? a.z : carry; a.w = a.w > carry ? a.w : carry;
    b.x = b.x > carry ? b.x : carry; b.y = b.y > carry ? b.y : carry; b.z = b.z > carry ? b.z : carry; b.w = b.w > carry ? b.w : carry;
    const int32_t j = base + 8 * (int32_t)threadIdx.x;
    if (j + 8 <= T1) {
      rs_u32x4_a4 va, vb;
      va.x = a.x; va.y = a.y; va.z = a.z; va.w = a.w; vb.x = b.x; vb.y = b.y; vb.z = b.z; vb.w = b.w;
      if (TAGGED) {
        gmx_store_u32x8_sc1(reinterpret_cast<uint32_t*>(anc) + base, 32u * threadIdx.x, a, b);      // (`base`: block-uniform)
      } else {
        *reinterpret_cast<rs_u32x4_a4*>(anc + j) = va;
        *reinterpret_cast<rs_u32x4_a4*>(anc + j + 4) = vb;
      }
    } else {
      if (j + 0 < T1) { if (TAGGED) gmx_store_u32_sc1(reinterpret_cast<uint32_t*>(anc) + j + 0, a.x); else anc[j + 0] = (int32_t)a.x; }
      if (j + 1 < T1) { if (TAGGED) gmx_store_u32_sc1(reinterpret_cast<uint32_t*>(anc) + j + 1, a.y); else anc[j + 1] = (int32_t)a.y; }
      if (j + 2 < T1) { if (TAGGED) gmx_store_u32_sc1(reinterpret_cast<uint32_t*>(anc) + j + 2, a.z); else anc[j + 2] = (int32_t)a.z; }
      if (j + 3 < T1) { if (TAGGED) gmx_store_u32_sc1(reinterpret_cast<uint32_t*>(anc) + j + 3, a.w); else anc[j + 3] = (int32_t)a.w; }
      if (j + 4 < T1) { if (TAGGED) gmx_store_u32_sc1(reinterpret_cast<uint32_t*>(anc) + j + 4, b.x); else anc[j + 4] = (int32_t)b.x; }
      if (j + 5 < T1) { if (TAGGED) gmx_store_u32_sc1(reinterpret_cast<uint32_t*>(anc) + j + 5, b.y); else anc[j + 5] = (int32_t)b.y; }
      if (j + 6 < T1) { if (TAGGED) gmx_store_u32_sc1(reinterpret_cast<uint32_t*>(anc) + j + 6, b.z); else anc[j + 6] = (int32_t)b.z; }
      if (j + 7 < T1) { if (TAGGED) gmx_store_u32_sc1(reinterpret_cast<uint32_t*>(anc) + j + 7, b.w); else anc[j + 7] = (int32_t)b.w; }
    }
  }
}



// The statistics pass of a LOOPED launch (GMX_JIT_RS_LOOP): the workgroup handles the C tiles blk, blk + G, blk + 2 G, ...
// and walks the whole table of n_tiles entries TWICE: the global max first (the exponent every G_t is scaled to), then, chunk
// by chunk of G entries, the chunk's sum and the sum of its entries in front of this workgroup's tile — prefix[c] = (all
// chunks before c) + (entries cG .. cG + blk - 1): the same integers gmx_tile_prefix_block / k_tile_prefix_big produce (sums
// of u64 are exact in any order; a max does not care about order).  One pass per WORKGROUP, not per tile: at 8e6 particles
// (7813 tiles, 12 bytes each) every workgroup reads 2 x 94 KB from L2.  Two accumulators per thread whatever C.
__device__ __forceinline__ void
gmx_tile_table_pass(const float* __restrict__ tmax, const uint64_t* __restrict__ agg, int n_tiles, int blk, int G, int C,
                    uint64_t* __restrict__ s_pf /* LDS, C entries */, uint64_t& total, uint64_t& mk) {
  __shared__ float s_tm[RS_WAVES];
  __shared__ uint64_t s_acc[RS_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float M = -gmx_inf();
  for (int t = (int)threadIdx.x; t < n_tiles; t += GMX_BLOCK) M = gmx_rmax(M, tmax[t]);
  M = wave_max(M);
  if (lane == 0) s_tm[wave] = M;
  __syncthreads();
  M = s_tm[0];
#pragma unroll
  for (int w = 1; w < RS_WAVES; ++w) M = gmx_rmax(M, s_tm[w]);
  const int32_t K = gmx_tile_exp(M);
  uint64_t running = 0;
#pragma clang loop unroll(disable)
  for (int c = 0; c < C; ++c) {
    const int lo = c * G, hi = (lo + G < n_tiles) ? lo + G : n_tiles, mine = lo + blk;
    uint64_t tot = 0, part = 0;
    for (int tb = lo; tb < hi; tb += GMX_BLOCK) {      // a row of 256 entries: wholly in front of `mine` / straddling it / behind
      const int t = tb + (int)threadIdx.x;
      if (t < hi) {
        const uint64_t g_ = gmx_tile_scale(agg[t], gmx_tile_exp(tmax[t]), K);
        tot += g_;
        if (tb + GMX_BLOCK <= mine) { GMX_KEEP_BRANCH; part += g_; }          // (workgroup-uniform)
        else if (tb < mine) { GMX_KEEP_BRANCH; part += (t < mine) ? g_ : 0ull; }
      }
    }
    wave_sum2_u64(tot, part);
    if (lane == 0) { s_acc[wave][0] = tot; s_acc[wave][1] = part; }
    __syncthreads();
    uint64_t T_ = 0, P_ = 0;
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) { T_ += s_acc[w][0]; P_ += s_acc[w][1]; }
    if (threadIdx.x == 0) s_pf[c] = running + P_;
    running += T_;
    __syncthreads();
  }
  total = running;
  mk = (uint64_t)gmx_f2u(M) | ((uint64_t)(uint32_t)K << 32);
}
