// gmx_sizes.h — how big a workspace is, what an entry point refuses, and what gmx_resample dispatches to: stated ONCE,
// for every build of the C-ABI of include/genmi.h (gmx_kernels.hip; the CPU mirror in tests/hostsim).
//   the tile constants        the definition tile of the two-level integer CDF and the tile tables built on it
//   gmx_*_bytes_ / _words_    the bodies of the gmx_*_workspace / _bytes / _words exports: each export is a one-line call
//   gmx_*_refusal_            argument checks as functions that return the message (a format taking the entry point's
//                             name, then one integer) or nothing, for gmx_fail, which writes the build's error string:
//                             the tile-form resamplers, the row-wise draws, the particle-MH pair, the particle-Gibbs three, the
//                             sharded / peer family, the sweep history
//   gmx_resample_dispatch_    the body of gmx_resample: argument checks, the workspace layout and the dispatch over kind
//                             and size.  It calls exported entry points only, so every build dispatches alike.
// Plain host C++ (static inline): no HIP, no kernel, no algorithm.  hiprtc never sees this file (it is not among the
// embedded headers): a specialised kernel gets GMX_TILE and GMX_MAX_TILES as two #defines ahead of its source.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "genmi.h"
#include "gmx_peer.h"                  /* gmx_peer_stats_words, gmx_peer_state_words */
#include "gmx_sorted.h"                /* gmx_sorted_layout_of */

#define GMX_TILE 1024                  /* one definition tile of the CDF (include/genmi.h "Resampling") */
#define GMX_MAX_TILES 2048             /* tiles of one table-per-workgroup resampling: n <= 2^21 */
#define GMX_LSE_TILE 4096              /* columns per workgroup of the two-stage row reductions */
#define GMX_LSE_ROWS_PATH_MAX_COLS 4096
#define GMX_SCAN_TILE 4096             /* items per workgroup of gmx_weight_cdf's chained scan */
#define GMX_ROWS_MAX_N (GMX_MAX_TILES * GMX_TILE)        /* what the per-row fused path takes */
#define GMX_ROWS_PIN_MAX_D 65533       /* D + 1 is a grid's y extent */

static inline int64_t gmx_tiles_(int64_t n) { return (n + GMX_TILE - 1) / GMX_TILE; }
static inline int gmx_ceil_log2_(int64_t n) {
  int need = 0;
  while (((int64_t)1 << need) < n) ++need;
  return need;
}

// ---- row reductions: gmx_logsumexp (one wave per row for many short rows: no workspace), gmx_sum_rows ----
static inline bool gmx_lse_rows_path_(int64_t rows, int64_t cols) { return rows >= 32 && cols <= GMX_LSE_ROWS_PATH_MAX_COLS; }
static inline size_t gmx_logsumexp_bytes_(int64_t rows, int64_t cols) {
  if (rows <= 0 || cols <= 0 || gmx_lse_rows_path_(rows, cols)) return 16;
  return (size_t)(rows * ((cols + GMX_LSE_TILE - 1) / GMX_LSE_TILE) * 2 * sizeof(float)) + 16;
}
static inline size_t gmx_sum_rows_bytes_(int64_t rows, int64_t cols) {
  if (rows <= 0 || cols <= 0) return 16;
  return (size_t)(rows * ((cols + GMX_LSE_TILE - 1) / GMX_LSE_TILE) * sizeof(float)) + 16;
}

// ---- the CDF array forms ----
// gmx_weight_cdf: ticket, error flag, done count, pad; then one u64 descriptor per scan tile
static inline size_t gmx_weight_cdf_bytes_(int64_t n) {
  int64_t tiles = (n + GMX_SCAN_TILE - 1) / GMX_SCAN_TILE;
  if (tiles < 1) tiles = 1;
  return 16 + (size_t)tiles * 8;
}
static inline size_t gmx_multinomial_bytes_(int64_t n_in) { return (size_t)(n_in + 4) * 4; }     // the guide table
// gmx_multinomial_tiled: two count buffers of (tiles + 16) words each
static inline size_t gmx_multinomial_tiled_bytes_(int64_t n) { return (size_t)(gmx_tiles_(n) + 16) * 8; }
// gmx_tile_prefix's block (u64 words): [0, tiles) prefixes | [tiles] total | [tiles + 1] M, K | pad to a multiple of 16
static inline size_t gmx_tile_prefix_words_(int64_t n) { return (size_t)((gmx_tiles_(n) + 2 + 15) / 16) * 16; }
static inline size_t gmx_sorted_uniforms_words_(int64_t n) { return n > 0 ? gmx_sorted_layout_of(n).words : 0; }

// ---- sharded resampling ----
// a rank's tile statistics: the block gmx_peer.h lays out (gmx_stats_block_at reads it)
static inline size_t gmx_shard_stats_bytes_(int64_t n_per_rank) { return gmx_stats_block_bytes(gmx_tiles_(n_per_rank)); }
static inline size_t gmx_shard_plan_words_(int world) { return (size_t)(GMX_PLAN_BOUNDS + world + 1); }
static inline size_t gmx_peer_landing_bytes_(int world, int64_t n_per_rank, int64_t capacity, int leaves) {
  if (world < 1 || n_per_rank < 1 || capacity < 1 || leaves < 1) return 0;
  return (gmx_peer_stats_words(world, (int)gmx_tiles_(n_per_rank)) + gmx_peer_state_words(world, capacity, leaves)) *
         sizeof(uint64_t);
}

// ---- refusals ----
// fmt == nullptr: nothing to refuse.  Otherwise a printf format taking the entry point's name (%s), then v (%lld) where
// the message quotes a value.
struct gmx_refusal { const char* fmt; long long v; };
// The error string of a build of the C-ABI (what its gmx_last_error returns) and the one way to leave a message in it:
// `fmt` takes a string, then an integer.  Returns 1, an entry point's refusal.
static thread_local char gmx_err_[512] = "";
static inline int gmx_fail(const char* fmt, const char* a = "", long long b = 0) {
  snprintf(gmx_err_, sizeof(gmx_err_), fmt, a, b);
  return 1;
}

// the sizes every tile-form resampler takes; any_n: the forms that read ONE prefix per workgroup, not the table
static inline const char* gmx_resample_shape_refusal_(int64_t n, int shift, bool any_n) {
  if (n <= 0) return "%s: n must be positive";
  if (!any_n && gmx_tiles_(n) > GMX_MAX_TILES)
    return "%s: n too large for the fused path (gmx_tile_stats + gmx_tile_prefix + gmx_resample_tiles_p, or gmx_weight_cdf + gmx_ancestors)";
  if (n > 0x7fffffffLL) return "%s: n out of range";
  if (shift < 1 || shift > 62) return "%s: shift out of range";
  if (shift + gmx_ceil_log2_(n) > 62) return "%s: shift too large for n (overflow)";      // n terms <= 2^shift stay below 2^62
  return nullptr;
}
// the tile-form resamplers: shape, null arguments, the kinds (or phase) the form takes, 16-byte alignment — in that order.
// has_null: one of the form's required pointers is null.  also16: the form's second 16-byte pointer (the order-statistics
// table of the sorted forms, gmx_multinomial_tiled's workspace), or nullptr.
enum gmx_tile_form { GMX_FORM_STATS, GMX_FORM_TILES, GMX_FORM_TILES_U, GMX_FORM_TILES_P, GMX_FORM_SORTED, GMX_FORM_SORTED_P,
                     GMX_FORM_MN_TILED };
static inline const char* gmx_tile_form_refusal_(gmx_tile_form form, int kind, int64_t n, int shift, bool has_null,
                                                 const void* lw_d, const void* also16 = nullptr, int phase = 0) {
  const bool any_n = form == GMX_FORM_STATS || form == GMX_FORM_TILES_P || form == GMX_FORM_SORTED_P;
  if (const char* m = gmx_resample_shape_refusal_(n, shift, any_n)) return m;
  if (has_null) return "%s: null argument";
  const bool ordered = kind == GMX_RESAMPLE_SYSTEMATIC || kind == GMX_RESAMPLE_STRATIFIED;
  if (form == GMX_FORM_TILES && !ordered) return "%s: kind must be systematic or stratified (use gmx_weight_cdf + gmx_ancestors)";
  if (form == GMX_FORM_TILES_P && !ordered) return "%s: kind must be systematic or stratified";
  if (form == GMX_FORM_TILES_U && kind != GMX_RESAMPLE_STRATIFIED) return "%s: stratified only (systematic draws one uniform)";
  if (form == GMX_FORM_MN_TILED && (phase < -1 || phase > 1)) return "%s: phase is -1, 0 or 1";
  if (((uintptr_t)lw_d & 15) || ((uintptr_t)also16 & 15)) {
    if (form == GMX_FORM_MN_TILED) return "%s: lw_d and workspace_d must be 16-byte aligned";
    if (form == GMX_FORM_SORTED || form == GMX_FORM_SORTED_P) return "%s: lw_d and table_d must be 16-byte aligned";
    return "%s: lw_d must be 16-byte aligned";
  }
  return nullptr;
}

// ---- row-wise draws: gmx_pick_rows, gmx_resample_rows, gmx_resample_rows_pinned, gmx_rows_pin, gmx_resample_rows_as,
// gmx_resample_rows_ess, gmx_pick_rows_take ----
// Every refusal below is the entry point's whole argument check but alignment (the HIP build's own): has_null — one of its
// always-required pointers is null — first, then the shapes, then the pointers a shape makes required (no_*: that pointer
// is null).
// The family's workspace: agg u64 [rows * tiles] | cdf u64 [cdf_words] | tmax f32 [rows * tiles], rounded up to 16 bytes.
// A size and the pointers into it are written from the same two terms.
struct gmx_rows_ws { uint64_t* agg; uint64_t* cdf; float* tmax; };
static inline uint64_t gmx_rows_cells_(int64_t rows, int64_t n) { return (uint64_t)rows * (uint64_t)gmx_tiles_(n); }
static inline uint64_t gmx_rows_cdf_words_(int kind, int64_t rows, int64_t n) {      // the iid multinomial's [rows, n] CDF
  return kind == GMX_RESAMPLE_MULTINOMIAL ? (uint64_t)rows * (uint64_t)n : 0u;
}
static inline size_t gmx_rows_ws_bytes_(uint64_t cells, uint64_t cdf_words) {
  return (size_t)((cells * 12u + cdf_words * 8u + 15u) & ~(uint64_t)15u);
}
static inline gmx_rows_ws gmx_rows_ws_carve_(void* workspace, uint64_t cells, uint64_t cdf_words) {
  gmx_rows_ws w;
  w.agg = (uint64_t*)workspace;
  w.cdf = w.agg + cells;
  w.tmax = (float*)(w.cdf + cdf_words);
  return w;
}
// gmx_pick_rows' workspace: no cdf
static inline size_t gmx_pick_rows_bytes_(int64_t rows, int64_t n) {
  if (rows < 1 || n < 1) return 16;
  return gmx_rows_ws_bytes_(gmx_rows_cells_(rows, n), 0);
}
static inline gmx_rows_ws gmx_pick_rows_carve_(void* workspace, int64_t rows, int64_t n) {
  return gmx_rows_ws_carve_(workspace, gmx_rows_cells_(rows, n), 0);
}
// shift = 62 - ceil(log2 n): a sum of n terms <= 2^shift stays below 2^62 (smc.cdf_shift)
static inline int gmx_pick_rows_shift_(int64_t n) { return 62 - gmx_ceil_log2_(n); }
static inline gmx_refusal gmx_pick_rows_refusal_(bool has_null, int64_t rows, int64_t n, int64_t ld) {
  if (has_null) return {"%s: null argument", 0};
  if (rows < 1 || rows > 0x7fffffffLL) return {"%s: rows = %lld is outside [1, 2^31)", (long long)rows};
  if (n < 1 || n > 0x7fffffffLL) return {"%s: n = %lld is outside [1, 2^31)", (long long)n};
  if (ld < n) return {"%s: ld = %lld is smaller than n", (long long)ld};
  return {nullptr, 0};
}
// row r's indices are offset by r * index_stride and stay int32: rows >= 1, n >= 1
static inline gmx_refusal gmx_index_stride_refusal_(int64_t rows, int64_t n, int64_t index_stride) {
  if (index_stride < 0 || (index_stride > 0 && (index_stride >= (1LL << 31) || rows * index_stride >= (1LL << 31) ||
                                                (rows - 1) * index_stride + n - 1 >= (1LL << 31))))
    return {"%s: index_stride = %lld does not keep rows * index_stride below 2^31", (long long)index_stride};
  return {nullptr, 0};
}
// gmx_resample_rows' workspace: the cdf for the iid multinomial only; nothing for n <= 1024
static inline size_t gmx_resample_rows_bytes_(int kind, int64_t rows, int64_t n) {
  if (rows < 1 || n <= GMX_TILE || n > GMX_ROWS_MAX_N) return 16;
  return gmx_rows_ws_bytes_(gmx_rows_cells_(rows, n), gmx_rows_cdf_words_(kind, rows, n));
}
static inline gmx_rows_ws gmx_resample_rows_carve_(void* workspace, int kind, int64_t rows, int64_t n) {
  return gmx_rows_ws_carve_(workspace, gmx_rows_cells_(rows, n), gmx_rows_cdf_words_(kind, rows, n));
}
static inline gmx_refusal gmx_resample_rows_refusal_(bool has_null, int kind, int64_t rows, int64_t n, int64_t ld,
                                                     int64_t index_stride) {
  if (has_null) return {"%s: null argument", 0};
  if (kind == GMX_RESAMPLE_MULTINOMIAL_TILED || kind == GMX_RESAMPLE_MULTINOMIAL_SORTED)
    return {"%s: GMX_RESAMPLE_MULTINOMIAL_TILED and GMX_RESAMPLE_MULTINOMIAL_SORTED have no row form (systematic, stratified "
            "or multinomial)", 0};
  if (kind < 0 || kind > 2) return {"%s: unknown kind %lld", (long long)kind};
  if (rows < 1 || rows > 0x7fffffffLL) return {"%s: rows = %lld is outside [1, 2^31)", (long long)rows};
  if (ld < n) return {"%s: ld = %lld is smaller than n", (long long)ld};
  if (n < 1 || n > GMX_ROWS_MAX_N) return {"%s: n = %lld is outside [1, 2^21]", (long long)n};
  return gmx_index_stride_refusal_(rows, n, index_stride);
}
// a pin's own arguments: D, and x_ld / x_row_stride keeping column n - 1 of every row inside a [D, x_ld] store
static inline gmx_refusal gmx_resample_rows_pin_refusal_(int64_t rows, int64_t n, int32_t D, int64_t x_ld, int64_t x_row_stride) {
  if (D < 0 || D > GMX_ROWS_PIN_MAX_D) return {"%s: D = %lld is outside [0, 65533]", (long long)D};
  if (D == 0) return {nullptr, 0};
  if (x_row_stride < 0) return {"%s: x_row_stride = %lld is negative", (long long)x_row_stride};
  if (x_ld < n || x_ld >= (1LL << 46) ||                                      // (D * x_ld stays below 2^62)
      (rows > 1 && x_row_stride > (x_ld - n) / (rows - 1)))                   // x_ld >= (rows - 1) * x_row_stride + n
    return {"%s: x_ld = %lld does not hold (rows - 1) * x_row_stride + n columns (or is 2^46 or more)", (long long)x_ld};
  return {nullptr, 0};
}
// gmx_resample_rows_pinned: gmx_resample_rows' arguments (the iid multinomial), the pin's, and the pin's two stores with D > 0
static inline gmx_refusal gmx_resample_rows_pinned_refusal_(bool has_null, int64_t rows, int64_t n, int64_t ld, int64_t index_stride,
                                                            int32_t D, int64_t x_ld, int64_t x_row_stride, bool no_pin_x,
                                                            bool no_x) {
  gmx_refusal no = gmx_resample_rows_refusal_(has_null, GMX_RESAMPLE_MULTINOMIAL, rows, n, ld, index_stride);
  if (!no.fmt) no = gmx_resample_rows_pin_refusal_(rows, n, D, x_ld, x_row_stride);
  if (no.fmt) return no;
  if (D > 0 && no_pin_x) return {"%s: null argument (pin_x_d with D > 0)", 0};
  if (D > 0 && no_x) return {"%s: null argument (x_d with D > 0)", 0};
  return {nullptr, 0};
}
// gmx_rows_pin: the above without an index_stride, and — with a broadcast — next_ld holding the rows * n particles of a row
// of the [D, next_ld] leaf
static inline gmx_refusal gmx_rows_pin_refusal_(bool has_null, int64_t rows, int64_t n, int64_t ld, int32_t D, int64_t x_ld,
                                                int64_t x_row_stride, bool has_next, int64_t next_ld, bool no_pin_x, bool no_x,
                                                bool no_next) {
  gmx_refusal no = gmx_resample_rows_refusal_(has_null, GMX_RESAMPLE_MULTINOMIAL, rows, n, ld, 0);
  if (!no.fmt) no = gmx_resample_rows_pin_refusal_(rows, n, D, x_ld, x_row_stride);
  if (no.fmt) return no;
  if (has_next && D > 0 && (next_ld < rows * n || next_ld >= (1LL << 46)))
    return {"%s: next_ld = %lld does not hold rows * n columns (or is 2^46 or more)", (long long)next_ld};
  if (D > 0 && no_pin_x) return {"%s: null argument (pin_x_d with D > 0)", 0};
  if (D > 0 && no_x) return {"%s: null argument (x_d with D > 0)", 0};
  if (D > 0 && has_next && no_next) return {"%s: null argument (next_d with next_x_d)", 0};
  return {nullptr, 0};
}
// gmx_resample_rows_as: gmx_resample_rows' arguments (the iid multinomial) and the ancestor logits' row stride
static inline gmx_refusal gmx_resample_rows_as_refusal_(bool has_null, int64_t rows, int64_t n, int64_t ld, int64_t index_stride,
                                                        int64_t as_ld) {
  const gmx_refusal no = gmx_resample_rows_refusal_(has_null, GMX_RESAMPLE_MULTINOMIAL, rows, n, ld, index_stride);
  if (no.fmt) return no;
  if (as_ld < n) return {"%s: as_ld = %lld is smaller than n", (long long)as_ld};
  return {nullptr, 0};
}
// gmx_resample_rows_as' workspace: gmx_resample_rows' (a multiple of 16 bytes), then gmx_pick_rows'; nothing for n <= 1024
static inline size_t gmx_resample_rows_as_bytes_(int64_t rows, int64_t n) {
  if (rows < 1 || n <= GMX_TILE || n > GMX_ROWS_MAX_N) return 16;
  return gmx_resample_rows_bytes_(GMX_RESAMPLE_MULTINOMIAL, rows, n) + gmx_pick_rows_bytes_(rows, n);
}
// (its second part: the first is gmx_resample_rows_carve_'s)
static inline gmx_rows_ws gmx_resample_rows_as_carve_(void* workspace, int64_t rows, int64_t n) {
  return gmx_pick_rows_carve_((uint8_t*)workspace + gmx_resample_rows_bytes_(GMX_RESAMPLE_MULTINOMIAL, rows, n), rows, n);
}
// gmx_pick_rows_take: gmx_pick_rows' matrix, the weights' row stride, the store gmx_rows_pin writes into (here: read), the
// index_stride rule of gmx_resample_rows, — with a broadcast — gmx_rows_pin's next_ld, and the two stores with D > 0
static inline gmx_refusal gmx_pick_rows_take_refusal_(bool has_null, int64_t rows, int64_t n, int64_t ld, int64_t lw_ld, int32_t D,
                                                      int64_t x_ld, int64_t x_row_stride, int64_t index_stride, bool has_next,
                                                      int64_t next_ld, bool no_x, bool no_x_out) {
  gmx_refusal no = gmx_pick_rows_refusal_(has_null, rows, n, ld);
  if (no.fmt) return no;
  if (lw_ld < n) return {"%s: lw_ld = %lld is smaller than n", (long long)lw_ld};
  no = gmx_resample_rows_pin_refusal_(rows, n, D, x_ld, x_row_stride);
  if (!no.fmt) no = gmx_index_stride_refusal_(rows, n, index_stride);
  if (no.fmt) return no;
  if (has_next && D > 0 && (next_ld / rows < n || next_ld >= (1LL << 46)))             // (rows * n may pass 2^63)
    return {"%s: next_ld = %lld does not hold rows * n columns (or is 2^46 or more)", (long long)next_ld};
  if (D > 0 && no_x) return {"%s: null argument (x_d with D > 0)", 0};
  if (D > 0 && no_x_out) return {"%s: null argument (x_out_d with D > 0)", 0};
  return {nullptr, 0};
}
// gmx_pick_rows_take's workspace: nothing for n <= 1024 (one launch); past it gmx_pick_rows' (the gathering launch reads the
// index k_pick_row wrote: nothing of its own)
static inline size_t gmx_pick_rows_take_bytes_(int64_t rows, int64_t n) {
  if (rows < 1 || n <= GMX_TILE) return 16;
  return gmx_pick_rows_bytes_(rows, n);
}
static inline gmx_rows_ws gmx_pick_rows_take_carve_(void* workspace, int64_t rows, int64_t n) {
  return gmx_pick_rows_carve_(workspace, rows, n);
}
// gmx_resample_rows_ess: gmx_resample_rows' arguments, for rows of ONE tile — the decision is taken on the row's per-element
// fixed-point weights, which past one tile are not the same integers (each tile has its own exponent), and it would have
// to be known before any tile's ancestors are written: a launch boundary
static inline gmx_refusal gmx_resample_rows_ess_refusal_(bool has_null, int kind, int64_t rows, int64_t n, int64_t ld,
                                                         int64_t index_stride) {
  if (has_null || (n >= 1 && n <= GMX_TILE)) return gmx_resample_rows_refusal_(has_null, kind, rows, n, ld, index_stride);
  const gmx_refusal no = gmx_resample_rows_refusal_(false, kind, 1, 1, 1, 0);               // the kinds, in its words
  if (no.fmt) return no;
  return {"%s: n = %lld is outside [1, 1024]: the ESS decision is taken on the fixed-point weights of a row of one tile "
          "(past one tile they are not the same integers, and the decision would need a launch of its own)", (long long)n};
}
// gmx_resample_rows_ess' workspace: nothing (one launch, a row is one tile)
static inline size_t gmx_resample_rows_ess_bytes_(int kind, int64_t rows, int64_t n) {
  (void)kind; (void)rows; (void)n;
  return 16;
}
// an ess_q8 above this resamples every row with mass (the ESS of n weights is at most n)
static inline uint32_t gmx_ess_always_(int64_t n) { return (uint32_t)(256 * n); }

// ---- particle marginal Metropolis-Hastings over a bank of filters: gmx_pmmh_propose, gmx_pmmh_accept (gmx_pmmh.h) ----
#define GMX_PMMH_BLOCK 256             /* threads per workgroup of both kernels */
#define GMX_PMMH_SPAN 1024             /* consecutive particles of the flat [R * n] axis a workgroup of the proposal broadcasts to */
#define GMX_PMMH_MAX_P 8               /* parameters: the proposal parks P draws per chain of its span in LDS (<= 32 KB) */
// chains a span of 1024 consecutive particles can touch: floor(1022 / n) + 2 (n = 1: 1024; n >= 1023: 2)
static inline int32_t gmx_pmmh_span_chains_(int64_t n) { return (int32_t)((GMX_PMMH_SPAN - 2) / n + 2); }
static inline size_t gmx_pmmh_lds_bytes_(int32_t P, int64_t n) { return (size_t)P * (size_t)gmx_pmmh_span_chains_(n) * sizeof(float); }
// what both entry points say about P, R and T
static inline gmx_refusal gmx_pmmh_shape_refusal_(int32_t P, int64_t R, int32_t T) {
  if (P < 1 || P > GMX_PMMH_MAX_P) return {"%s: P = %lld is outside [1, 8] (the proposals of a workgroup's chains are held in LDS)", (long long)P};
  if (R < 1 || R > 0x7fffffffLL) return {"%s: R = %lld is outside [1, 2^31)", (long long)R};
  if (T < 1) return {"%s: T = %lld is not positive", (long long)T};
  if ((int64_t)T * R > 0x7fffffffLL) return {"%s: T * R = %lld does not stay below 2^31", (long long)((int64_t)T * R)};
  return {nullptr, 0};
}
static inline gmx_refusal gmx_pmmh_propose_refusal_(bool has_null, int32_t P, int64_t R, int64_t n, int32_t T) {
  if (has_null) return {"%s: null argument", 0};
  const gmx_refusal no = gmx_pmmh_shape_refusal_(P, R, T);
  if (no.fmt) return no;
  if (n < 1 || n > 0x7fffffffLL) return {"%s: n = %lld is outside [1, 2^31)", (long long)n};
  if (R * n > 0x7fffffffLL) return {"%s: R * n = %lld does not stay below 2^31 (the bank's flat particle axis)", (long long)(R * n)};
  return {nullptr, 0};
}
// flags_d may be null (every step counts); the iteration recorded in row cap - 1 has to fit fold_in's 32 bits
static inline gmx_refusal gmx_pmmh_accept_refusal_(bool has_null, int32_t P, int64_t R, int32_t T, int shift, int64_t cap) {
  if (has_null) return {"%s: null argument", 0};
  const gmx_refusal no = gmx_pmmh_shape_refusal_(P, R, T);
  if (no.fmt) return no;
  if (shift < 1 || shift > 62) return {"%s: shift = %lld is outside [1, 62]", (long long)shift};
  if (cap < 1 || cap > (1LL << 32)) return {"%s: cap = %lld is outside [1, 2^32] (an iteration is fold_in's 32-bit word)", (long long)cap};
  return {nullptr, 0};
}

// ---- particle Gibbs over a bank of conditional filters: gmx_pg_open, gmx_pg_propose, gmx_pg_accept (gmx_pgibbs.h) ----
// gmx_pg_open runs on gmx_pmmh_propose's grid, span and LDS layout and refuses what it refuses (keys_as_d may be null)
static inline gmx_refusal gmx_pg_open_refusal_(bool has_null, int32_t P, int64_t R, int64_t n, int32_t T) {
  return gmx_pmmh_propose_refusal_(has_null, P, R, n, T);
}
static inline gmx_refusal gmx_pg_propose_refusal_(bool has_null, int32_t P, int64_t R) {
  if (has_null) return {"%s: null argument", 0};
  return gmx_pmmh_shape_refusal_(P, R, 1);
}
// the record row is the caller's: the iteration is an argument
static inline gmx_refusal gmx_pg_accept_refusal_(bool has_null, int32_t P, int64_t R, int32_t T, int64_t row, int64_t cap) {
  if (has_null) return {"%s: null argument", 0};
  const gmx_refusal no = gmx_pmmh_shape_refusal_(P, R, T);
  if (no.fmt) return no;
  if (cap < 1 || cap > (1LL << 32)) return {"%s: cap = %lld is outside [1, 2^32] (an iteration is fold_in's 32-bit word)", (long long)cap};
  if (row < 0 || row >= cap) return {"%s: row = %lld is outside the record [0, cap)", (long long)row};
  return {nullptr, 0};
}

// ---- sharded resampling and the fused peer exchange: gmx_shard_plan, _route, _step, _step_sorted, _totals, _step_tiles,
// _step_fused, gmx_peer_put_stats, gmx_shard_step_peer, gmx_peer_bump, gmx_sweep_verdict ----
// Each refusal is the entry point's whole argument check, in its order; none quotes a value, so it returns the format
// alone.  has_null: one of the entry point's required pointers other than the key is null.
#define GMX_SHARD_MAX_WORLD 64         /* ranks of the one-launch forms: a wave's lanes hold one total each (SHARD_MAX_WORLD) */
static inline const char* gmx_shard_check_(bool no_key, int kind, int rank, int world, int64_t n) {
  if (no_key) return "%s: null key";
  if (kind != GMX_RESAMPLE_SYSTEMATIC && kind != GMX_RESAMPLE_STRATIFIED) return "%s: systematic / stratified only (ordered slot thresholds)";
  if (world < 1 || world > 1024 || rank < 0 || rank >= world) return "%s: rank / world out of range";
  if (n <= 0 || n > 0x7fffffffLL || n * world >= (1LL << 40)) return "%s: n_per_rank out of range";
  return nullptr;
}
// capacity, then the extended index: a slot's ancestor indexes [ n_per_rank local | world * capacity received ]
static inline const char* gmx_shard_capacity_refusal_(int64_t n_per_rank, int64_t capacity) {
  return capacity < 1 || capacity > n_per_rank ? "%s: capacity must be in [1, n_per_rank]" : nullptr;
}
static inline const char* gmx_shard_extended_refusal_(int64_t n_per_rank, int world, int64_t capacity) {
  return n_per_rank + (int64_t)world * capacity > 0x7fffffffLL ? "%s: extended state index exceeds int32" : nullptr;
}
static inline const char* gmx_shard_shift_refusal_(int shift) { return shift < 1 || shift > 62 ? "%s: shift out of range" : nullptr; }
// array_form: the form has a CDF-array counterpart, which takes any world
static inline const char* gmx_shard_world_refusal_(int world, bool array_form) {
  if (world <= GMX_SHARD_MAX_WORLD) return nullptr;
  return array_form ? "%s: world <= 64 (use gmx_weight_cdf + gmx_shard_step)" : "%s: world <= 64";
}
// the keyed forms: gmx_shard_check_, null arguments, then what the form adds — capacity and the extended index (all but
// the plan); world <= 64 and the shift (the forms on tile statistics); n_per_rank <= 2^21 (the fused form holds the table:
// the step on this rank's own block strides over its earlier tiles and takes any size); alignment last.  a16: the form's
// 16-byte pointer (lw_d; cdf_d, which only the one-launch step, world <= 64, reads 16 bytes at a time); a8: its statistics
enum gmx_shard_form { GMX_SHARD_PLAN, GMX_SHARD_ROUTE, GMX_SHARD_STEP, GMX_SHARD_STEP_TILES, GMX_SHARD_STEP_FUSED };
static inline const char* gmx_shard_form_refusal_(gmx_shard_form form, bool no_key, int kind, int rank, int world,
                                                  int64_t n_per_rank, bool has_null, int64_t capacity = 1, int shift = 1,
                                                  const void* a16 = nullptr, const void* a8 = nullptr) {
  const char* m = gmx_shard_check_(no_key, kind, rank, world, n_per_rank);
  if (!m && has_null) m = "%s: null argument";
  if (m || form == GMX_SHARD_PLAN) return m;
  if (!m) m = gmx_shard_capacity_refusal_(n_per_rank, capacity);
  if (!m) m = gmx_shard_extended_refusal_(n_per_rank, world, capacity);
  if (m || form == GMX_SHARD_ROUTE) return m;
  if (form == GMX_SHARD_STEP) return world <= GMX_SHARD_MAX_WORLD && ((uintptr_t)a16 & 15) ? "%s: cdf_d must be 16-byte aligned" : nullptr;
  if (!m) m = gmx_shard_world_refusal_(world, form == GMX_SHARD_STEP_TILES);
  if (!m) m = gmx_shard_shift_refusal_(shift);
  if (!m && form == GMX_SHARD_STEP_FUSED && gmx_tiles_(n_per_rank) > GMX_MAX_TILES) m = "%s: n_per_rank too large (<= 2^21)";
  if (!m && (((uintptr_t)a16 & 15) || ((uintptr_t)a8 & 7)))
    m = form == GMX_SHARD_STEP_TILES ? "%s: lw_d must be 16-byte and stats_own_d 8-byte aligned"
                                     : "%s: lw_d must be 16-byte and stats_all_d 8-byte aligned";
  return m;
}
// the unkeyed sorted-multinomial step: the n_per_rank * world global slots index ONE order-statistics table
static inline const char* gmx_shard_step_sorted_refusal_(bool has_null, int rank, int world, int64_t n_per_rank, int64_t capacity,
                                                         const void* table_d) {
  if (has_null) return "%s: null argument";
  if (world < 1 || world > 1024 || rank < 0 || rank >= world) return "%s: rank / world out of range";
  if (n_per_rank <= 0 || n_per_rank * world > 0x7fffffffLL) return "%s: n_per_rank * world out of range (< 2^31)";
  const char* m = gmx_shard_capacity_refusal_(n_per_rank, capacity);
  if (!m) m = gmx_shard_extended_refusal_(n_per_rank, world, capacity);
  return m || !((uintptr_t)table_d & 15) ? m : "%s: table_d must be 16-byte aligned";
}
// (one workgroup strides over the whole gathered table: any number of tiles)
static inline const char* gmx_shard_totals_refusal_(bool has_null, int world, int64_t n_per_rank, const void* stats_all_d) {
  if (has_null) return "%s: null argument";
  if (world < 1 || world > 1024) return "%s: world out of range";
  if (n_per_rank <= 0 || n_per_rank > 0x7fffffffLL) return "%s: n_per_rank out of range (< 2^31)";
  return (uintptr_t)stats_all_d & 7 ? "%s: stats_all_d must be 8-byte aligned" : nullptr;
}
static inline const char* gmx_peer_check_(const gmx_peer& P, int64_t n_per_rank) {
  if (!P.land_d || !P.tag_base_d || !P.status_d) return "%s: peer has a null pointer";
  if (P.world < 1 || P.world > GMX_SHARD_MAX_WORLD || P.rank < 0 || P.rank >= P.world) return "%s: peer rank / world out of range (world <= 64)";
  if (P.step < 0) return "%s: peer.step is negative";
  const int64_t tiles = gmx_tiles_(n_per_rank);
  if (n_per_rank <= 0 || tiles > GMX_MAX_TILES || P.tiles != (int32_t)tiles) return "%s: peer.tiles must be ceil(n_per_rank / 1024) <= 2048";
  if (P.capacity < 1 || P.capacity > n_per_rank) return "%s: peer.capacity must be in [1, n_per_rank]";
  if (P.leaves < 1 || P.leaves > GMX_PEER_MAX_LEAVES) return "%s: peer.leaves must be in [1, GMX_PEER_MAX_LEAVES = 32]";
  return nullptr;
}
static inline const char* gmx_peer_put_stats_refusal_(bool has_null, const gmx_peer& P, int64_t n_per_rank) {
  return has_null ? "%s: null argument" : gmx_peer_check_(P, n_per_rank);
}
// rank, world and capacity are the peer's; the leaves' HOST arrays are read last, once they are known to be there
static inline const char* gmx_shard_step_peer_refusal_(bool no_key, int kind, const gmx_peer& P, int64_t n_per_rank, bool has_null,
                                                       int shift, const void* lw_d, const void* stats_own_d,
                                                       const void* const* state_rows_h, void* const* tail_rows_h) {
  const char* m = gmx_shard_check_(no_key, kind, P.rank, P.world, n_per_rank);
  if (!m) m = gmx_peer_check_(P, n_per_rank);
  if (!m && has_null) m = "%s: null argument";
  if (!m) m = gmx_shard_extended_refusal_(n_per_rank, P.world, P.capacity);
  if (!m) m = gmx_shard_shift_refusal_(shift);
  if (!m && (((uintptr_t)lw_d & 15) || ((uintptr_t)stats_own_d & 7))) m = "%s: lw_d must be 16-byte and stats_own_d 8-byte aligned";
  for (int l = 0; !m && l < P.leaves; ++l)
    if (!state_rows_h[l] || !tail_rows_h[l]) m = "%s: a leaf pointer is null";
  return m;
}
static inline const char* gmx_peer_bump_refusal_(const void* tag_base_d, int32_t T) { return !tag_base_d || T < 1 ? "%s: bad argument" : nullptr; }
static inline const char* gmx_sweep_verdict_refusal_(const void* overflow_d, const void* status_h, int32_t n_status, const void* verdict_d) {
  return !overflow_d || !verdict_d || n_status < 0 || n_status > 4 || (n_status && !status_h) ? "%s: bad argument (at most 4 status words)" : nullptr;
}

// ---- sweep history ----
static inline gmx_refusal gmx_history_record_refusal_(int32_t D, int64_t n, uint32_t expect_tag, bool has_null, bool has_status) {
  if (has_null) return {"%s: null argument", 0};
  if (D <= 0 || D > 65533) return {"%s: D = %lld is outside [1, 65533]", (long long)D};
  if (n <= 0 || n > 0x7fffffffLL) return {"%s: n = %lld is outside [1, 2^31)", (long long)n};
  if (expect_tag > 255u) return {"%s: expect_tag = %lld is outside [0, 255]", (long long)expect_tag};
  if (expect_tag != 0u && !has_status) return {"%s: a tag check needs status_d", 0};
  if (expect_tag != 0u && n > (1LL << 24)) return {"%s: tagged ancestors hold 24-bit indices (n = %lld)", (long long)n};
  return {nullptr, 0};
}
static inline gmx_refusal gmx_lineage_refusal_(const void* anc_d, const void* xs_d, int32_t T, int32_t D, int64_t n,
                                               const void* start_d, int64_t m, const void* paths_d, const void* traj_d,
                                               const void* status_d) {
  if (!start_d || !status_d) return {"%s: null argument", 0};
  if (!paths_d && !traj_d) return {"%s: null argument (paths_d and traj_d)", 0};
  if (traj_d && !xs_d) return {"%s: null argument (xs_d with traj_d)", 0};
  if (T <= 0 || D <= 0 || n <= 0 || m <= 0) return {"%s: T, D, n and m must be positive", 0};
  if (T > 1 && !anc_d) return {"%s: null argument (anc_d)", 0};
  if (n > 0x7fffffffLL) return {"%s: n = %lld does not fit the int32 indices", (long long)n};
  return {nullptr, 0};
}

// ---- gmx_resample: THE resampling entry point (include/genmi.h): log-weights -> ancestors for every kind and every
// n < 2^31, dispatching to the staged forms a caller that already holds tile statistics uses directly ----
struct gmx_resample_ws_layout {
  size_t agg, tmax, pref, table, mnt, cdf, cdfws, mnws, total;
};
static inline size_t gmx_ws_up_(size_t x) { return (x + 255) & ~(size_t)255; }
static inline gmx_resample_ws_layout gmx_resample_ws_of_(int64_t n) {
  gmx_resample_ws_layout L;
  const size_t tiles = (size_t)gmx_tiles_(n);
  size_t o = 0;
  L.agg = o; o = gmx_ws_up_(o + tiles * 8);
  L.tmax = o; o = gmx_ws_up_(o + tiles * 4);
  L.pref = o; o = gmx_ws_up_(o + gmx_tile_prefix_words_(n) * 8);
  L.table = o; o = gmx_ws_up_(o + gmx_sorted_uniforms_words_(n) * 4);
  L.mnt = o; o = gmx_ws_up_(o + (n <= (int64_t)GMX_ROWS_MAX_N ? gmx_multinomial_tiled_bytes_(n) : 0));
  L.cdf = o; o = gmx_ws_up_(o + (size_t)n * 8);
  L.cdfws = o; o = gmx_ws_up_(o + gmx_weight_cdf_bytes_(n));
  L.mnws = o; o = gmx_ws_up_(o + gmx_multinomial_bytes_(n));
  L.total = o;
  return L;
}
static inline size_t gmx_resample_bytes_(int64_t n) { return n > 0 ? gmx_resample_ws_of_(n).total : 0; }

// (max_partials_d / n_partials of the entry point are accepted for compatibility and unused: the tile maxima are recomputed)
static inline int gmx_resample_dispatch_(int kind, const uint32_t key[2], const float* lw_d, int64_t n,
                                         int shift, float* max_d, uint64_t* total_d, int32_t* ancestors_d,
                                         void* workspace_d, gmx_stream stream) {
  const char* who = "gmx_resample";
  if (!workspace_d || !key || !lw_d || !max_d || !total_d || !ancestors_d) return gmx_fail("%s: null argument", who);
  if ((uintptr_t)workspace_d & 15) return gmx_fail("%s: workspace_d must be 16-byte aligned", who);
  if (n <= 0 || n > 0x7fffffffLL) return gmx_fail("%s: n out of range", who);
  const gmx_resample_ws_layout L = gmx_resample_ws_of_(n);
  uint8_t* w = (uint8_t*)workspace_d;
  uint64_t* agg = (uint64_t*)(w + L.agg);
  float* tmax = (float*)(w + L.tmax);
  const bool small = gmx_tiles_(n) <= GMX_MAX_TILES;
  if (kind == GMX_RESAMPLE_MULTINOMIAL) {          // iid slot order: the CDF array + the guide-table search
    uint64_t* cdf = (uint64_t*)(w + L.cdf);
    if (gmx_tile_stats(lw_d, n, shift, tmax, agg, stream)) return 1;        // (the tile maxima: gmx_weight_cdf reduces them to the max)
    if (gmx_weight_cdf(lw_d, n, shift, tmax, gmx_tiles_(n), max_d, cdf, total_d, w + L.cdfws, stream)) return 1;
    return gmx_multinomial(key, cdf, n, total_d, n, ancestors_d, w + L.mnws, stream);
  }
  if (kind != GMX_RESAMPLE_SYSTEMATIC && kind != GMX_RESAMPLE_STRATIFIED && kind != GMX_RESAMPLE_MULTINOMIAL_TILED &&
      kind != GMX_RESAMPLE_MULTINOMIAL_SORTED)
    return gmx_fail("%s: unknown kind", who);
  if (gmx_tile_stats(lw_d, n, shift, tmax, agg, stream)) return 1;
  if (kind == GMX_RESAMPLE_MULTINOMIAL_TILED) {
    if (!small) return gmx_fail("%s: GMX_RESAMPLE_MULTINOMIAL_TILED takes n <= 2^21 (use GMX_RESAMPLE_MULTINOMIAL_SORTED)", who);
    return gmx_multinomial_tiled(key, lw_d, n, shift, tmax, agg, nullptr, max_d, total_d, ancestors_d, w + L.mnt, -1, stream);
  }
  if (small) {
    if (kind == GMX_RESAMPLE_MULTINOMIAL_SORTED)
      return gmx_resample_sorted(key, lw_d, n, shift, tmax, agg, (uint32_t*)(w + L.table), 0, max_d, total_d, ancestors_d, stream);
    return gmx_resample_tiles(kind, key, lw_d, n, shift, tmax, agg, max_d, total_d, ancestors_d, stream);
  }
  uint64_t* pref = (uint64_t*)(w + L.pref);           // past 2048 tiles: one prefix pass, then the prefix-reading forms
  if (gmx_tile_prefix(tmax, agg, n, pref, stream)) return 1;
  if (kind == GMX_RESAMPLE_MULTINOMIAL_SORTED)
    return gmx_resample_sorted_p(key, lw_d, n, shift, tmax, pref, (uint32_t*)(w + L.table), 0, max_d, total_d, ancestors_d, stream);
  return gmx_resample_tiles_p(kind, key, lw_d, n, shift, tmax, pref, max_d, total_d, ancestors_d, stream);
}
