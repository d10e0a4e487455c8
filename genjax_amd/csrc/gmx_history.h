// BootstrapSweep history (include/genmi.h "Sweep history"): the per-step record and the lineage walk.
//   k_history_record   a streaming copy of one step's [D + 2] rows (D state rows, the log-weights, the ancestors) into
//                      the history slabs; the ancestor row may hold the fused prologue's tagged words
//   k_lineage          m pointer walks back through T levels of ancestors, one (or GMX_LINEAGE_CHAINS) per lane
// Under hipcc: the two kernels, included by gmx_kernels.hip only (no specialised kernel needs them: this header is not
// among those embedded for hiprtc).  Under a plain host compiler: the two ENTRY POINTS as sequential loops — the
// statement of what the kernels compute that a CPU build of the C-ABI from these headers (gmx_vm.h includes this file
// there) exports, so host logic that records and walks a history can run without a device.  Those loops validate their
// arguments as the HIP entry points do and leave their message (gmx_sizes.h: the checks, gmx_fail).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GMX_HIST_BLOCK 256
#define GMX_HIST_TAG_SHIFT 24u                       // = RS_ANC_TAG_SHIFT (gmx_offspring.h): {tag | 24-bit index}
#define GMX_HIST_INDEX_MASK 0x00ffffffu

// independent chains per thread of k_lineage (1, 2 or 4).  Measured on MI355X at n = m = 1e6, T = 100
// (tools/time_history.py, DESIGN.md section 4 "Sweep history"): the default is the variant kept.
#ifndef GMX_LINEAGE_CHAINS
#define GMX_LINEAGE_CHAINS 1
#endif

// one ancestor word on its way into the record: the index, and 1 if its tag is not the expected one
__device__ __forceinline__ uint32_t hist_strip(uint32_t w, uint32_t expect_tag, uint32_t& bad) {
  bad += (w >> GMX_HIST_TAG_SHIFT) != expect_tag ? 1u : 0u;
  return w & GMX_HIST_INDEX_MASK;
}

// Row r of the step (blockIdx.y): r < D: x row r; r = D: the log-weights; r = D + 1: the ancestors.  A thread moves four
// consecutive words with ONE 16-byte store: the destination row starts anywhere in its slab (slab + t * D * n, n odd),
// so the row is cut into a head of (-dst / 4) & 3 words up to the first 16-byte boundary of the DESTINATION, a body of
// whole quads and a tail of < 4 words; head and tail are scalar.  The source of a quad is loaded with one 16-byte load
// when it is aligned too, with four coalesced 4-byte loads otherwise.
__global__ void __launch_bounds__(GMX_HIST_BLOCK)
k_history_record(const uint32_t* __restrict__ x, int32_t D, const uint32_t* __restrict__ lw,
                 const uint32_t* __restrict__ anc, int64_t n, uint32_t expect_tag, uint32_t* __restrict__ x_out,
                 uint32_t* __restrict__ lw_out, uint32_t* __restrict__ anc_out, unsigned long long* __restrict__ status) {
  const int32_t r = (int32_t)blockIdx.y;
  const uint32_t* src;
  uint32_t* dst;
  if (r < D) { src = x + (int64_t)r * n; dst = x_out + (int64_t)r * n; }
  else if (r == D) { src = lw; dst = lw_out; }
  else { src = anc; dst = anc_out; }
  const bool strip = (r == D + 1) && expect_tag != 0u;
  int64_t head = (int64_t)(((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  const int64_t quads = (n - head) >> 2;
  const int64_t q = (int64_t)blockIdx.x * GMX_HIST_BLOCK + threadIdx.x;
  uint32_t bad = 0u;
  if (q < quads) {
    const int64_t i = head + 4 * q;
    uint4 v;
    if ((((uintptr_t)(src + i)) & 15u) == 0u) {
      v = *reinterpret_cast<const uint4*>(src + i);
    } else {
      v.x = src[i]; v.y = src[i + 1]; v.z = src[i + 2]; v.w = src[i + 3];
    }
    if (strip) {
      v.x = hist_strip(v.x, expect_tag, bad); v.y = hist_strip(v.y, expect_tag, bad);
      v.z = hist_strip(v.z, expect_tag, bad); v.w = hist_strip(v.w, expect_tag, bad);
    }
    *reinterpret_cast<uint4*>(dst + i) = v;
  }
  if (q == 0) {          // the row's head and tail: at most 3 words each
    for (int64_t i = 0; i < head; ++i) {
      uint32_t w = src[i];
      if (strip) w = hist_strip(w, expect_tag, bad);
      dst[i] = w;
    }
    for (int64_t i = head + 4 * quads; i < n; ++i) {
      uint32_t w = src[i];
      if (strip) w = hist_strip(w, expect_tag, bad);
      dst[i] = w;
    }
  }
  if (bad) atomicAdd(status, (unsigned long long)bad);      // (a stale word is the rare case: no reduction needed)
}

// an index on its way into a read: inside [0, n), and counted when it was not
__device__ __forceinline__ int64_t lineage_clamp(int32_t p, int64_t n, uint32_t& bad) {
  int64_t q = (int64_t)p;
  if (q < 0) { q = 0; ++bad; }
  if (q >= n) { q = n - 1; ++bad; }
  return q;
}

// Trajectory j: p = start[j]; for t = T-1 .. 0: paths[t][j] = p; traj[t][d][j] = xs[t][d][p]; p = anc[t-1][p].
// A walk is T dependent loads: the hop to level t - 1 is issued FIRST, the D state loads of level t behind it (they do
// not depend on it), and C independent chains per thread keep C hops in flight per lane.  DK > 0: D known at compile
// time (the state loads unroll); DK = 0: any D.  j is the fastest index of both outputs: a wave's stores coalesce.
// Every element offset is 64-bit: t * D * n + d * n + p passes 2^31 at sizes that fit the device.
template <int DK, int C>
__global__ void __launch_bounds__(GMX_HIST_BLOCK)
k_lineage(const int32_t* __restrict__ anc, const float* __restrict__ xs, int32_t T, int32_t D_, int64_t n,
          const int32_t* __restrict__ start, int64_t m, int32_t* __restrict__ paths, float* __restrict__ traj,
          unsigned long long* __restrict__ status) {
  const int32_t D = DK > 0 ? DK : D_;
  const int64_t j0 = ((int64_t)blockIdx.x * C) * GMX_HIST_BLOCK + threadIdx.x;      // chain c: j0 + c * GMX_HIST_BLOCK
  int64_t p[C];
  uint32_t bad = 0u;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int64_t j = j0 + (int64_t)c * GMX_HIST_BLOCK;
    p[c] = j < m ? lineage_clamp(start[j], n, bad) : 0;
  }
  for (int32_t t = T - 1; t >= 0; --t) {
    int32_t nxt[C];
#pragma unroll
    for (int c = 0; c < C; ++c) nxt[c] = t > 0 ? anc[(int64_t)(t - 1) * n + p[c]] : 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int64_t j = j0 + (int64_t)c * GMX_HIST_BLOCK;
      if (j >= m) continue;
      if (paths) paths[(int64_t)t * m + j] = (int32_t)p[c];
      if (traj) {
        const float* row = xs + (int64_t)t * D * n + p[c];
        float* out = traj + (int64_t)t * D * m + j;
        if (DK > 0) {
          float v[DK > 0 ? DK : 1];
#pragma unroll
          for (int d = 0; d < DK; ++d) v[d] = row[(int64_t)d * n];
#pragma unroll
          for (int d = 0; d < DK; ++d) out[(int64_t)d * m] = v[d];
        } else {
          for (int32_t d = 0; d < D; ++d) out[(int64_t)d * m] = row[(int64_t)d * n];
        }
      }
    }
    if (t > 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int64_t j = j0 + (int64_t)c * GMX_HIST_BLOCK;
        uint32_t b = 0u;
        p[c] = lineage_clamp(nxt[c], n, b);
        if (j < m) bad += b;
      }
    }
  }
  if (bad) atomicAdd(status, (unsigned long long)bad);
}

#elif defined(__cplusplus) && !defined(__HIPCC_RTC__)
#include <string.h>
#include "genmi.h"
#include "gmx_sizes.h"
// (`used`: emitted, and so exported by a shared library, although nothing in the translation unit calls them)

extern "C" __attribute__((used)) inline int gmx_history_record(const float* x_d, int32_t D, const float* lw_d, const uint32_t* anc_d, int64_t n,
                                         uint32_t expect_tag, float* x_out_d, float* lw_out_d, int32_t* anc_out_d,
                                         int64_t* status_d, gmx_stream) {
  const gmx_refusal no = gmx_history_record_refusal_(D, n, expect_tag, !x_d || !lw_d || !anc_d || !x_out_d || !lw_out_d || !anc_out_d,
                                                     status_d != nullptr);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_history_record", no.v);
  memcpy(x_out_d, x_d, (size_t)D * (size_t)n * 4);
  memcpy(lw_out_d, lw_d, (size_t)n * 4);
  for (int64_t i = 0; i < n; ++i) {
    uint32_t w = anc_d[i];
    if (expect_tag != 0u) {
      if ((w >> 24) != expect_tag) *status_d += 1;
      w &= 0x00ffffffu;
    }
    anc_out_d[i] = (int32_t)w;
  }
  return 0;
}

extern "C" __attribute__((used)) inline int gmx_lineage(const int32_t* anc_d, const float* xs_d, int32_t T, int32_t D, int64_t n,
                                  const int32_t* start_d, int64_t m, int32_t* paths_d, float* traj_d, int64_t* status_d,
                                  gmx_stream) {
  const gmx_refusal no = gmx_lineage_refusal_(anc_d, xs_d, T, D, n, start_d, m, paths_d, traj_d, status_d);
  if (no.fmt) return gmx_fail(no.fmt, "gmx_lineage", no.v);
  for (int64_t j = 0; j < m; ++j) {
    int64_t p = start_d[j];
    for (int32_t t = T - 1; t >= 0; --t) {
      if (p < 0) { p = 0; *status_d += 1; }           // clamped before any read, and counted
      if (p >= n) { p = n - 1; *status_d += 1; }
      if (paths_d) paths_d[(int64_t)t * m + j] = (int32_t)p;
      if (traj_d) for (int32_t d = 0; d < D; ++d) traj_d[((int64_t)t * D + d) * m + j] = xs_d[((int64_t)t * D + d) * n + p];
      if (t) p = anc_d[(int64_t)(t - 1) * n + p];
    }
  }
  return 0;
}
#endif
