// lhpc_plan.cpp — plan-time CSR validation and re-encodings of CSR into the
// XSLICE and XTILE layouts (see lhpc_plan.hpp).  Host only, OpenMP; every
// output is identical for any thread count.
#include "lhpc_plan.hpp"

#include <omp.h>

#include <algorithm>
#include <cstring>
#include <iterator>
#include <vector>

#include "../../include/lhpc.h"

namespace lhpc {
namespace {
inline int64_t rp_at(const void *rp, int bits, int64_t i) {
  return bits == 64 ? static_cast<const int64_t *>(rp)[i]
                    : static_cast<const int32_t *>(rp)[i];
}
}  // namespace

int validate_csr(const void *rp, int bits, const int32_t *col, int64_t n_rows, int64_t n_cols, int64_t nnz) {
  if (n_rows < 0 || nnz < 0 || rp_at(rp, bits, 0) != 0 || rp_at(rp, bits, n_rows) != nnz) return LHPC_ERR_BAD_CSR;
  int bad = 0;
#pragma omp parallel for schedule(static) reduction(| : bad)
  for (int64_t i = 0; i < n_rows; ++i) bad |= rp_at(rp, bits, i + 1) < rp_at(rp, bits, i) ? 1 : 0;
  if (bad) return LHPC_ERR_BAD_CSR;
  const uint32_t lim = static_cast<uint32_t>(n_cols);  // n_cols ≤ INT32_MAX; a negative col wraps above it
#pragma omp parallel for schedule(static) reduction(| : bad)
  for (int64_t k = 0; k < nnz; ++k) bad |= static_cast<uint32_t>(col[k]) >= lim ? 1 : 0;
  return bad ? LHPC_ERR_BAD_CSR : LHPC_OK;
}

void csr_column_block(const void *rp, int bits, const int32_t *col, const void *val, size_t tsz, int64_t r0,
                      int64_t r1, int64_t c0, int64_t c1, std::vector<int64_t> &orp, std::vector<int32_t> &ocol,
                      std::vector<unsigned char> &oval) {
  const int64_t nr = r1 - r0;
  orp.assign(static_cast<size_t>(nr) + 1, 0);
#pragma omp parallel for schedule(static)
  for (int64_t r = 0; r < nr; ++r) {
    int64_t c = 0;
    for (int64_t k = rp_at(rp, bits, r0 + r); k < rp_at(rp, bits, r0 + r + 1); ++k) c += col[k] >= c0 && col[k] < c1;
    orp[static_cast<size_t>(r) + 1] = c;
  }
  for (int64_t r = 0; r < nr; ++r) orp[static_cast<size_t>(r) + 1] += orp[static_cast<size_t>(r)];
  const int64_t m = orp[static_cast<size_t>(nr)];
  ocol.resize(static_cast<size_t>(m));
  oval.resize(static_cast<size_t>(m) * tsz);
  const auto *vb = static_cast<const unsigned char *>(val);
#pragma omp parallel for schedule(static)
  for (int64_t r = 0; r < nr; ++r) {
    int64_t o = orp[static_cast<size_t>(r)];
    for (int64_t k = rp_at(rp, bits, r0 + r); k < rp_at(rp, bits, r0 + r + 1); ++k)
      if (col[k] >= c0 && col[k] < c1) {
        ocol[static_cast<size_t>(o)] = static_cast<int32_t>(col[k] - c0);
        std::memcpy(oval.data() + static_cast<size_t>(o) * tsz, vb + static_cast<size_t>(k) * tsz, tsz);
        ++o;
      }
  }
}

int build_xslice(const void *rp, int bits, const int32_t *col, const void *val, size_t tsz,
                 int64_t n_rows, int64_t n_cols, int S, XsliceHost &o) {
  if (S < 1 || S > 256) return LHPC_ERR_INVALID_ARG;
  o.S = S;
  o.n_rows = n_rows;
  o.n_chunks = (n_rows + 63) / 64;
  o.n_rows_pad = o.n_chunks * 64;
  o.width = ((n_cols + S - 1) / S + 63) / 64 * 64;
  if (o.width == 0) o.width = 64;
  const int64_t nnz = rp_at(rp, bits, n_rows) - rp_at(rp, bits, 0);
  o.nnz = nnz;
  o.cbase.reset(new int64_t[static_cast<size_t>(S) * o.n_chunks + 1]);
  o.col.reset(new int32_t[nnz > 0 ? nnz : 1]);
  o.val.reset(new unsigned char[(nnz > 0 ? nnz : 1) * tsz]);
  const int64_t W = o.width;
  const size_t nl = static_cast<size_t>(S) * o.n_rows_pad;
  std::unique_ptr<uint16_t[]> l16(new uint16_t[nl]);
  int bad = 0, maxc = 0;
  // pass 1: in-slice lengths
#pragma omp parallel for schedule(static) reduction(| : bad) reduction(max : maxc)
  for (int64_t r = 0; r < o.n_rows_pad; ++r) {
    int cnt[256];
    std::memset(cnt, 0, sizeof(int) * static_cast<size_t>(S));
    if (r < n_rows) {
      for (int64_t k = rp_at(rp, bits, r); k < rp_at(rp, bits, r + 1); ++k) ++cnt[col[k] / W];
    }
    for (int s = 0; s < S; ++s) {
      if (cnt[s] > 65535) bad = 1;
      maxc = std::max(maxc, cnt[s]);
      l16[static_cast<size_t>(s) * o.n_rows_pad + r] = static_cast<uint16_t>(std::min(cnt[s], 65535));
    }
  }
  if (bad) return LHPC_ERR_UNSUPPORTED;
  o.lens_bytes = maxc > 255 ? 2 : 1;
  o.lens.reset(new uint8_t[nl * o.lens_bytes]);
  if (o.lens_bytes == 2) {
    std::memcpy(o.lens.get(), l16.get(), nl * 2);
  } else {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < static_cast<int64_t>(nl); ++i) o.lens[i] = static_cast<uint8_t>(l16[i]);
  }
  // chunk sizes → offsets, slice-major
  std::vector<int64_t> csz(static_cast<size_t>(S) * o.n_chunks);
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < S * o.n_chunks; ++i) {
    const uint16_t *l = l16.get() + (i / o.n_chunks) * o.n_rows_pad + (i % o.n_chunks) * 64;
    int64_t t = 0;
    for (int r = 0; r < 64; ++r) t += l[r];
    csz[static_cast<size_t>(i)] = t;
  }
  int64_t acc = 0;
  o.max_chunk = 0;
  for (int64_t i = 0; i < S * o.n_chunks; ++i) {
    o.cbase[i] = acc;
    acc += csz[static_cast<size_t>(i)];
    o.max_chunk = std::max(o.max_chunk, csz[static_cast<size_t>(i)]);
  }
  o.cbase[S * o.n_chunks] = acc;
  if (acc != nnz) return LHPC_ERR_INTERNAL;
  // pass 2: fill, one 64-row chunk per iteration (all slices)
#pragma omp parallel
  {
    std::vector<int64_t> order;   // element ids of the chunk, bucketed by (row, slice)
    std::vector<int64_t> start;   // [64][S+1] start of (row, slice) bucket in `order`
#pragma omp for schedule(dynamic, 64)
    for (int64_t c = 0; c < o.n_chunks; ++c) {
      const int64_t r0 = c * 64;
      const int64_t e0 = rp_at(rp, bits, std::min(r0, n_rows));
      const int64_t e1 = rp_at(rp, bits, std::min(r0 + 64, n_rows));
      order.assign(static_cast<size_t>(e1 - e0), 0);
      start.assign(static_cast<size_t>(64) * (S + 1), 0);
      for (int r = 0; r < 64 && r0 + r < n_rows; ++r) {
        const int64_t s0 = rp_at(rp, bits, r0 + r), s1 = rp_at(rp, bits, r0 + r + 1);
        int64_t *st = start.data() + static_cast<size_t>(r) * (S + 1);
        st[0] = s0 - e0;
        for (int s = 0; s < S; ++s) st[s + 1] = st[s] + l16[static_cast<size_t>(s) * o.n_rows_pad + r0 + r];
        int64_t fill[256];  // stable counting sort by slice
        for (int s = 0; s < S; ++s) fill[s] = st[s];
        for (int64_t k = s0; k < s1; ++k) order[static_cast<size_t>(fill[col[k] / W]++)] = k;
      }
      for (int s = 0; s < S; ++s) {
        int64_t pos = o.cbase[s * o.n_chunks + c];
        const uint16_t *l = l16.get() + static_cast<size_t>(s) * o.n_rows_pad + r0;
        auto emit = [&](int64_t e) {
          o.col[pos] = col[e];
          std::memcpy(o.val.get() + pos * tsz, static_cast<const unsigned char *>(val) + e * tsz, tsz);
          ++pos;
        };
        for (int r = 0; r < 64; ++r)
          for (int j = 0; j < l[r]; ++j)
            emit(order[static_cast<size_t>(start[static_cast<size_t>(r) * (S + 1) + s] + j)]);
      }
    }
  }
  return LHPC_OK;
}

// XTILE column blocks (lhpc_options.xtile_col_blocks).  A reduce chunk holds
// M nonzeros and meets every one of the S tiles, so its segment per tile is
// M/S nonzeros: 32 for C2 (S = 256), 4 at n = 80M (S = 2048), and the
// reduce's cost per nonzero grows with S (DESIGN.md §4 "large n": 632 GFLOP/s
// at S = 256, 533 at 768, 408 at 1024, 244 at 2048).  Cutting the columns into
// B blocks gives each block's plan S/B tiles; the blocks run in turn on x's
// column ranges, every block after the first adding into y.  A chunk also
// holds ≤ M/8 rows, so as a block's rows get shorter its chunks shrink with
// the blocks.  Same box, fp32 15 per row, forced B (profiles/r04/col_blocks):
// n = 10M (256 tiles) B = 1 / 2: 601 / 534 GFLOP/s; 40M (1024) B = 2 / 3 /
// 4: 498 / 446 / 426; 80M (2048) B = 2 / 3 / 4 / 6: 378 / 417 / 365 / 314;
// 150M (3840, two row parts) B = 2 / 3 / 4: 316 / 371 / 342.  fp64 10M (489)
// B = 1 / 2: 318 / 304; 40M (1954) B = 2 / 3 / 4 / 6: 264 / 261 / 230 / 180.
// Hence B = ⌈S / 768⌉, at most mean row length / 5.
constexpr int64_t kColBlockTiles = 768;
static int xtile_col_blocks_for(int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t S, const lhpc_options &o) {
  const int64_t most = std::max<int64_t>(1, n_cols / 64);  // ≥ 64 columns per block
  if (o.xtile_col_blocks > 0) return static_cast<int>(std::min<int64_t>(o.xtile_col_blocks, most));
  if (S <= kColBlockTiles || n_rows <= 0) return 1;
  const double mean = static_cast<double>(nnz) / static_cast<double>(n_rows);
  const int64_t bmax = std::max<int64_t>(1, static_cast<int64_t>(mean / 5.0));
  return static_cast<int>(std::min({(S + kColBlockTiles - 1) / kColBlockTiles, bmax, most}));
}

XtilePartition xtile_partition_policy(int64_t n_rows, int64_t n_cols, int64_t nnz, size_t elem_bytes, int n_splits,
                                      const lhpc_options &o) {
  XtilePartition r;
  const int64_t W = xtile_capacity(elem_bytes);
  r.tiles = (n_cols + W - 1) / W;
  // row parts when the tile stream outgrows its int32 offsets (or a lower
  // cap is asked for); user row splits keep a single plan
  // and column blocks when x spans many tiles (xtile_col_blocks_for)
  r.cap = INT32_MAX - 8 * (r.tiles + 256) - (int64_t{1} << 16);
  if (o.xtile_part_nnz > 0) r.cap = std::min<int64_t>(r.cap, o.xtile_part_nnz);
  r.col_blocks = n_splits == 0 ? xtile_col_blocks_for(n_rows, n_cols, nnz, r.tiles, o) : 1;
  r.parts = (nnz > r.cap || r.col_blocks > 1) && n_splits == 0 &&
            (r.tiles + r.col_blocks - 1) / r.col_blocks <= kXtMaxTiles;
  return r;
}

constexpr unsigned kForceFamily = LHPC_PLAN_FORCE_ROWGROUP | LHPC_PLAN_FORCE_ADAPTIVE | LHPC_PLAN_FORCE_XSLICE |
                                  LHPC_PLAN_FORCE_XTILE | LHPC_PLAN_FORCE_SELL;

bool spmv_wants_locality(int64_t n_cols, size_t elem_bytes, unsigned flags) {
  return !(flags & kForceFamily) && static_cast<double>(n_cols) * static_cast<double>(elem_bytes) > 8.0e6;
}

SpmvFamilyPolicy spmv_family_policy(const SpmvShape &s, unsigned flags, const lhpc_options &o) {
  SpmvFamilyPolicy r;
  const bool auto_ok = !(flags & kForceFamily);
  // XTILE / XSLICE when x outgrows one XCD's 4 MB L2, and only when the
  // gathers have no locality of their own: a banded or structured matrix
  // (stencil operators, the CG Laplacian) re-reads each x line from
  // neighbouring rows, which the row-local kernels already serve from L2,
  // while XSLICE would add S partials per row.  Measured: distinct 128-B x
  // lines per nonzero over sampled 8192-row chunks (≈0.8 for C2's uniform
  // columns, ≈0.03 for a 2-D Laplacian); ≤ 0.25 counts as local.
  const double locality_thr = o.spmv_locality > 0 ? o.spmv_locality : 0.25;
  const bool nolocal = spmv_wants_locality(s.n_cols, s.elem_bytes, flags) && s.lines_per_nnz > locality_thr;
  // XTILE (x tiles in LDS) is the default for gathers without locality;
  // options.spmv_no_xtile selects XSLICE instead.  A layout that does not fit
  // its index types, or a row too long for one slice, falls through.
  r.try_xtile = ((flags & LHPC_PLAN_FORCE_XTILE) || (nolocal && !o.spmv_no_xtile)) && s.n_rows > 0;
  r.part = xtile_partition_policy(s.n_rows, s.n_cols, s.nnz, s.elem_bytes, s.n_splits, o);
  r.try_xslice = ((flags & LHPC_PLAN_FORCE_XSLICE) || nolocal) && s.nnz > 0;
  // Off those paths ADAPTIVE (nnz-balanced blocks, coalesced col/val stream,
  // LDS row sums) is the default: measured equal or faster than ROWGROUP on
  // uniform rows of 3-40 nnz (within 4% at 8 and 24), and 1.26-1.5× faster on
  // C1 and the 2-D Laplacians (tools/explore_rowlen.py).
  // ROWGROUP stays selectable (FORCE_ROWGROUP).
  const bool adaptive = !(flags & LHPC_PLAN_FORCE_ROWGROUP) || (flags & LHPC_PLAN_FORCE_ADAPTIVE);
  if (!adaptive) {
    r.csr_kernel = LHPC_KERNEL_ROWGROUP;
    const double mean = s.n_rows ? static_cast<double>(s.nnz) / static_cast<double>(s.n_rows) : 0;
    int L = 4;
    while (L < 64 && L < mean) L <<= 1;
    r.L = L;
    r.R = L == 4 ? 1 : L <= 16 ? 4 : L == 32 ? 2 : 1;
    if (o.rowgroup_lanes > 0 || o.rowgroup_rows > 0) {
      // the (L, R) shapes lhpc_spmv_csr.hip instantiates
      static const int kShapes[] = {101, 201, 202, 401, 402, 404, 802, 804, 1601, 1602, 1604, 1608, 3201, 3202, 6401};
      const int want = o.rowgroup_lanes * 100 + o.rowgroup_rows;
      if (std::find(std::begin(kShapes), std::end(kShapes), want) == std::end(kShapes))
        r.csr_status = LHPC_ERR_INVALID_ARG;
      r.L = o.rowgroup_lanes;
      r.R = o.rowgroup_rows;
    }
  }
  // SELL for short rows (≤ kSellMaxW nonzeros) whose padded slices stream no
  // more bytes than CSR + row_ptr (the builder's rule): bit-identical to
  // ADAPTIVE, no row_ptr stream, LDS or barrier (the CG Laplacian: DESIGN.md §4)
  r.force_sell = (flags & LHPC_PLAN_FORCE_SELL) != 0;
  r.try_sell = adaptive && (r.force_sell || (auto_ok && !o.spmv_no_sell)) && s.max_row_len <= kSellMaxW && s.n_rows > 0;
  return r;
}

int64_t xtile_tile_width(int64_t n_cols, size_t elem_bytes, int cus, int narrow_override) {
  // tile width: the LDS capacity XtTile<T>::W, narrowed for fp32 so that the
  // tile count is a whole multiple of the CUs when that adds ≤ 10% tiles
  // (C2: 245 → 256 tiles of 39063 columns): a cache-sized range's gather
  // round of one piece per tile then fills every CU.  fp64 (single range,
  // ≈ 2 pieces per CU) lost 3% with it (C3 489 → 512 tiles: 0.913 → 0.941 ms)
  const int64_t W = xtile_capacity(elem_bytes);
  const int64_t s0 = (n_cols + W - 1) / W, s1 = (s0 + cus - 1) / cus * cus;
  // (never past build_xtile's 4096-tile cap: on a CU count that does not
  // divide 4096 the rounding could otherwise cost a plan its XTILE layout)
  bool narrow = elem_bytes == 4 && s1 * 10 <= s0 * 11 && s1 <= kXtMaxTiles;
  if (narrow_override >= 0) narrow = narrow_override != 0;
  return narrow && s1 > s0 ? (n_cols + s1 - 1) / s1 : W;
}

XtilePolicy xtile_policy(const XtileShape &s, const lhpc_options &o) {
  XtilePolicy r;
  const int64_t tsz = s.elem_bytes, W = s.W, cus = s.cus;
  const int M = s.M;
  const bool user_splits = s.n_user_splits > 0;
  r.W = W;
  r.tiles = (s.n_cols + W - 1) / W;
  r.nnz = s.nnz;
  r.cus = s.cus;
  // ≈ 2 gather workgroups per CU (one resident per CU: 160 KB of LDS each)
  // and ≥ 4 tiles' worth of stream per piece, so the tile load (W·T bytes)
  // stays ≤ 1/4 of a piece's col16 + xg traffic on small (per-rank) matrices
  r.min_piece = 4 * W * tsz / (2 + tsz);
  r.piece = std::max<int64_t>(r.min_piece, s.nnz / (2 * cus) + 1);
  if (o.xtile_piece > 0) r.piece = std::max<int64_t>(8, o.xtile_piece);
  // reduce index stream: iperm (gather each CSR position's x from the flat
  // segment concatenation in LDS), else perm (scatter into CSR slots).  Round
  // 1 kept perm below 32 full chunks per CU (per-rank matrices at N ≥ 4);
  // with the reduce as it is now iperm is as fast or faster there too — same
  // box, local work of rank 0 (tools/explore_rank_reduce.py,
  // profiles/r04/rank_reduce.jsonl): fp32 W = 4 0.132 → 0.118 ms, W = 8
  // 0.0656 → 0.0653; fp64 W = 4 0.263 → 0.245, W = 8 0.125 → 0.118
  bool ip = true;
  if (o.xtile_reduce != LHPC_XTILE_REDUCE_AUTO) ip = o.xtile_reduce == LHPC_XTILE_REDUCE_IPERM;
  // the iperm reduce addresses xg with 32-bit buffer offsets: stream + tile
  // padding (≤ 8 per tile) + one piece of slack must stay below 2 GiB
  const int64_t stream_max = s.nnz + 8 * r.tiles + 2 * M;
  if (stream_max * tsz >= (int64_t{1} << 31)) ip = false;
  r.iperm = ip;
  // aligned segments (iperm only): each (tile, chunk) segment padded to 16 B
  // (≤ VW − 1 entries per segment, ≤ 3 per 4 nonzeros in the worst case)
  const int64_t VW = 16 / tsz;
  bool al = false;
  if (o.xtile_align == LHPC_XTILE_ALIGN_UNITS) al = true;
  if (al && (!ip || (stream_max + (VW - 1) * std::min<int64_t>(s.nnz, r.tiles * (s.nnz / (M / 2) + 2))) * tsz >=
                        (int64_t{1} << 31)))
    al = false;
  // the fp32 aligned reduce with 8 segment-table entries per thread (S > 2048
  // tiles, n_cols > 84M) would spill a VGPR: packed segments there
  if (al && s.G > 4) al = false;
  r.aligned = al;
  r.supported = !(s.dev_build && al);  // aligned segments: host build only
  // chunk cuts: at the last row start in the back M/32 of the window, else
  // mid-row (the row's pieces meet in k_xtile_fixup).  Per-chunk costs are
  // fixed, so full chunks matter on skewed rows: C4 has 19803 chunks when any
  // row start in the back half is taken, 18454 with the back M/32 (C2: 18316
  // either way); options.xtile_cut overrides (entries, 1..M)
  r.cut = M / 32;
  if (o.xtile_cut > 0) r.cut = std::min(M, o.xtile_cut);
  // the xg ring (options.xtile_ring): the plan's own cache
  // ranges by default; user row ranges only when asked for (xtile_ring = 2:
  // the library's per-rank plans, which gather and reduce range by range in
  // order — lhpc_spmv_stage would gather every range into the one ring: a
  // ring plan refuses it)
  r.ring_ok = ip && !al && (user_splits ? o.xtile_ring == 2 : o.xtile_ring != 1);
  // cache-sized ranges: K nnz-balanced row ranges, gathered and reduced in
  // turn, so that each range's xg (≈ 200 MB) is still in the 256 MB Infinity
  // Cache when its reduce reads it back.  fp32 only: each extra range re-reads
  // x (n_cols·T) in its gather.  Same box: C2 reduce 352 → 295
  // µs, gather 163 → 179 µs, call 523.5 → 483.8 µs at K = 3 (K = 4: 506.7);
  // C3 (fp64, K = 6: 200 MB ranges) 928 → 944 µs, so not for fp64 — until
  // the xg ring (round 6, same box, xtile_ranges = 1 / 3 / 4 / 6 / 8: C3
  // 0.908 / 0.943 / 0.995 / 0.868 / 0.902 ms): fp64 takes the ranges when its
  // plan can hold the ring (no user row splits, iperm reduce).
  // Only while each range still streams ≥ min_piece nonzeros per tile (fp64:
  // min_piece / 2 — its ring saves the 8-B xg write-back) and K ≤ 8: every
  // range re-loads all S tiles of x, so a wide x (n = 80M: 1954 tiles; n =
  // 150M: 3662) would spend more on tile loads than the cache saves — such
  // plans keep one range (the n = 150M plan took 23.6 ms with 8 ranges per part)
  const int64_t xg_bytes = s.nnz * tsz;
  r.past_cache = xg_bytes > (int64_t{256} << 20);
  {
    const int64_t k = (xg_bytes + (int64_t{200} << 20) - 1) / (int64_t{200} << 20);
    const int64_t need = tsz == 4 ? r.min_piece : r.min_piece / 2;
    if ((tsz == 4 || r.ring_ok) && r.past_cache && k <= 8 && s.nnz / k / std::max<int64_t>(1, r.tiles) >= need)
      r.ranges = static_cast<int>(k);
  }
  if (o.xtile_ranges > 0) r.ranges = o.xtile_ranges;
  // without user splits the ranges are the plan's own nnz-balanced row cuts
  r.own_cuts = !user_splits && r.ranges > 1 && s.n_rows >= 2LL * r.ranges;
  // phase-A tables (options.xtile_pretable): iperm
  // plans without aligned segments, G = 1.  Default for fp64 only — same box,
  // two runs each: C3 reduce 89.9 → 85.3 µs per range (its 16-wave scan was
  // 2.3K of 27.8K cycles per chunk), C2 88.1 → 89.4 µs (the tables' extra
  // 2 KB per chunk outweigh an 8-wave scan)
  r.pre = ip && !al && s.G == 1 && (o.xtile_pretable == 2 || (o.xtile_pretable == 0 && tsz == 8));
  // chunk records (options.xtile_chunkrec): fp32
  // iperm plans without aligned segments, G = 1, whose rows all hold a
  // nonzero and whose reduce stores y (a record has no bit for an empty row,
  // and the record reduce has no adding store).  Phase-A tables asked for by
  // option come first: the two exclude each other.  Default: the plans that
  // take cache-sized ranges by themselves (xg past the Infinity Cache, no
  // user splits, no xtile_ranges) — same box, two runs each, C2 reduce
  // 87.6 / 87.8 → 84.4 / 84.5 µs per range and 699.2 / 698.6 → 714.5 / 713.2
  // GFLOP/s, C4 88.2 / 88.1 → 87.8 / 87.6 µs and 691.6 / 690.1 → 694.6 / 693.9
  // (profiles/r11).  Per-rank ring plans and plans inside the cache are not
  // measured: they keep the scan unless asked.
  const bool rec_auto = r.past_cache && r.ranges > 1 && !user_splits && o.xtile_ranges == 0;
  r.rec = ip && !al && s.G == 1 && tsz == 4 && !r.pre && !s.empty_rows && !s.y_add &&
          (o.xtile_chunkrec == 2 || (o.xtile_chunkrec == 0 && rec_auto));
  if (o.xtile_steps > 0) {
    const int u = o.xtile_steps;
    r.steps = u <= 2 ? 2 : u < 8 ? 4 : u < 16 ? 8 : 16;
  }
  // non-temporal xg stores when the xg of a single-range plan exceeds the 256
  // MB Infinity Cache anyway (same box, two runs each: C3 918.6 → 908.8 µs
  // median); cache-sized ranges need their xg to stay there (C2 with them
  // non-temporal: 473 → 536 µs)
  r.store = o.xtile_store;
  r.range_piece_opt = o.xtile_range_piece;
  return r;
}

int64_t XtilePolicy::range_piece(int K) const {
  // one gather round per range: ≈ one piece per (tile, range) part, so each
  // range loads every tile once (only one 160-KB gather block fits a CU)
  if (range_piece_opt > 0) return std::max<int64_t>(8, range_piece_opt);
  return std::max<int64_t>(min_piece, nnz / K / static_cast<int64_t>(cus) * 5 / 4 + 1);
}

int xtile_plan_chunks(const void *rp, int bits, const int32_t *col, int64_t n_rows, int64_t n_cols, int64_t W,
                      int M, int Rmax, int slot_bytes, const int64_t *splits, int n_splits, bool iperm,
                      int cut_window, XtileHost &o, int unit) {
  const int64_t nnz = rp_at(rp, bits, n_rows) - rp_at(rp, bits, 0);
  if (W < 8 || M < 64 || M >= 65536 || M % 16 || Rmax < 1 || (slot_bytes != 4 && slot_bytes != 8) ||
      cut_window < 1 || cut_window > M || (unit != 1 && unit != 2 && unit != 4) || (unit > 1 && !iperm))
    return LHPC_ERR_INVALID_ARG;
  const int64_t S = n_cols > 0 ? (n_cols + W - 1) / W : 1;
  if (S > kXtMaxTiles || nnz + 8 * S >= INT32_MAX || n_rows >= INT32_MAX) return LHPC_ERR_UNSUPPORTED;
  o.S = static_cast<int>(S);
  o.W = W;
  o.M = M;
  o.Rmax = Rmax;
  o.unit = unit;
  const int64_t U = unit;
  auto RP = [&](int64_t i) { return rp_at(rp, bits, i); };
  // aligned segments: the longest window [e, e + len) whose padded length
  // Σ_s ⌈count_s / U⌉·U stays ≤ M (monotone in len, so any shorter cut fits)
  std::vector<int32_t> wcnt(unit > 1 ? static_cast<size_t>(S) : 0, 0);
  std::vector<int32_t> touched;
  auto window = [&](int64_t e) -> int64_t {
    if (U == 1) return M;
    int64_t k = e, padded = 0;
    for (; k < nnz; ++k) {
      const int64_t s = col[k] / W;
      const int64_t add = wcnt[static_cast<size_t>(s)] % U == 0 ? U : 0;
      if (padded + add > M) break;
      if (wcnt[static_cast<size_t>(s)] == 0) touched.push_back(static_cast<int32_t>(s));
      ++wcnt[static_cast<size_t>(s)];
      padded += add;
    }
    for (const int32_t s : touched) wcnt[static_cast<size_t>(s)] = 0;
    touched.clear();
    return k - e;
  };
  // first row r in [lo, n_rows] with rp[r] >= e
  auto lower_row = [&](int64_t lo, int64_t e) {
    int64_t hi = n_rows;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (RP(mid) < e) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  // ---- chunks: (ce, cr) pairs; invariant: cr[c] = first row with rp >= ce[c]
  //      (or a row whose predecessors starting at ce[c] are empty)
  o.ce.assign(1, 0);
  o.cr.assign(1, 0);
  for (int i = 0; i < n_splits; ++i)
    if (splits[i] <= 0 || splits[i] >= n_rows || (i > 0 && splits[i] <= splits[i - 1]))
      return LHPC_ERR_INVALID_ARG;
  {
    int64_t e = 0, r = 0;
    int si = 0;  // next split row after r
    while (!(e == nnz && r == n_rows)) {
      int64_t en, rb;
      const int64_t Mc = window(e);
      // a cut inside the window: row starts in its back cut_window entries
      // (scaled to the window when padding shortens it)
      const int64_t cw = U == 1 ? cut_window : std::max<int64_t>(1, cut_window * Mc / M);
      // a split row is done once a chunk starts at it (e == its start, r == it)
      while (si < n_splits && (RP(splits[si]) < e || (RP(splits[si]) == e && splits[si] <= r))) ++si;
      if (si < n_splits && RP(splits[si]) <= e + Mc) {
        en = RP(splits[si]);  // a range starts at this row: cut there
        rb = splits[si];
      } else if (e + Mc >= nnz) {
        en = nnz;
        rb = n_rows;
      } else {
        const int64_t target = e + Mc;
        // last row q with rp[q] <= target
        const int64_t q = lower_row(r, target + 1) - 1;
        if (q >= r && RP(q) > e + Mc - cw) {
          en = RP(q);  // cut at a row start
        } else {
          en = target;  // cut mid-row
        }
        rb = lower_row(r, en);
      }
      if (rb - r > Rmax) {
        rb = r + Rmax;
        en = RP(rb);
      }
      o.ce.push_back(static_cast<int32_t>(en));
      o.cr.push_back(static_cast<int32_t>(rb));
      e = en;
      r = rb;
    }
  }
  const int64_t C = static_cast<int64_t>(o.ce.size()) - 1;
  o.n_chunks = C;
  // range k = chunks [rchunk[k], rchunk[k+1]): the chunk owning split row k−1 first
  o.rchunk.assign(1, 0);
  for (int i = 0; i < n_splits; ++i) {
    // chunks inside a long row just before the split also have cr == split
    // (they own no row); the range starts at the one beginning at the split row
    int64_t c = std::lower_bound(o.cr.begin(), o.cr.end(), static_cast<int32_t>(splits[i])) - o.cr.begin();
    while (c < C && !(o.cr[c] == splits[i] && o.ce[c] == RP(splits[i]))) ++c;
    if (c >= C) return LHPC_ERR_INTERNAL;
    o.rchunk.push_back(c);
  }
  o.rchunk.push_back(C);
  if (M > 65535 / (kXtSegHi - 1)) return LHPC_ERR_UNSUPPORTED;  // seg lo fits 16 bits
  o.cont.clear();
  for (int64_t c = 0; c < C; ++c) {
    const int64_t r0 = o.cr[c], r1 = o.cr[c + 1];
    if (r1 > r0 && RP(r1) > o.ce[c + 1]) o.cont.push_back(static_cast<int32_t>(c));
  }
  o.iperm_mode = iperm;
  o.slot_bytes = slot_bytes;
  o.segoff.assign(static_cast<size_t>((C + 1) * S), 0);
  return LHPC_OK;
}

int xtile_plan_offsets(XtileHost &o, std::vector<int64_t> &tbase) {
  const int64_t S = o.S, C = o.n_chunks, U = o.unit;
  auto pad = [U](int64_t len) { return (len + U - 1) / U * U; };
  int32_t *cnt = o.segoff.data() + S;  // row c+1 holds count[c] on entry
  if (U > 1)  // aligned segments: padding at each segment's end
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < C; ++c)
      for (int64_t s = 0; s < S; ++s) cnt[c * S + s] = static_cast<int32_t>(pad(cnt[c * S + s]));
  tbase.assign(static_cast<size_t>(S) + 1, 0);
  {
    std::vector<int64_t> tot(static_cast<size_t>(S), 0);
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < S; ++s) {
      int64_t t = 0;
      for (int64_t c = 0; c < C; ++c) t += cnt[c * S + s];
      tot[static_cast<size_t>(s)] = t;
    }
    for (int64_t s = 0; s < S; ++s) tbase[s + 1] = tbase[s] + (tot[s] + 7) / 8 * 8;
  }
  if (tbase[S] >= INT32_MAX) return LHPC_ERR_UNSUPPORTED;  // segment padding pushed the stream past int32
  o.total = tbase[S];
  // exclusive prefix down each tile column: segoff[c][s] = tbase[s] + Σ_{c'<c} count[c'][s]
#pragma omp parallel for schedule(static)
  for (int64_t s = 0; s < S; ++s) {
    int64_t acc = tbase[s];
    for (int64_t c = 0; c <= C; ++c) {
      const int64_t n = c < C ? o.segoff[(c + 1) * S + s] : 0;
      o.segoff[c * S + s] = static_cast<int32_t>(acc);
      acc += n;
    }
  }
  return LHPC_OK;
}

void xtile_plan_scatter_host(const int32_t *col, int64_t nnz, XtileHost &o) {
  const int64_t S = o.S, C = o.n_chunks, W = o.W;
  const bool iperm = o.iperm_mode;
  const int slot_bytes = o.slot_bytes;
  // ---- scatter (stable: CSR order inside each segment)
  o.col16.reset(new uint16_t[o.total > 0 ? o.total : 1]());
  if (iperm)
    o.iperm.reset(new uint16_t[nnz > 0 ? nnz : 1]());
  else
    o.perm.reset(new uint16_t[o.total > 0 ? o.total : 1]());
#pragma omp parallel
  {
    std::vector<int32_t> cur(static_cast<size_t>(S)), flat(iperm ? static_cast<size_t>(S) : 0);
#pragma omp for schedule(dynamic, 64)
    for (int64_t c = 0; c < C; ++c) {
      std::memcpy(cur.data(), o.segoff.data() + c * S, sizeof(int32_t) * static_cast<size_t>(S));
      if (iperm) {  // flat offset of each tile's segment in the chunk's concatenation
        int32_t f = 0;
        for (int64_t s = 0; s < S; ++s) {
          flat[static_cast<size_t>(s)] = f;
          f += o.segoff[(c + 1) * S + s] - o.segoff[c * S + s];
        }
      }
      const int64_t e0 = o.ce[c];
      for (int64_t k = e0; k < o.ce[c + 1]; ++k) {
        const int64_t s = col[k] / W;
        const int32_t g = cur[static_cast<size_t>(s)]++;
        o.col16[g] = static_cast<uint16_t>(col[k] - s * W);
        if (iperm)
          o.iperm[k] = static_cast<uint16_t>(flat[static_cast<size_t>(s)] + (g - o.segoff[c * S + s]));
        else
          o.perm[g] = static_cast<uint16_t>(xtile_slot(static_cast<int>(k - e0), slot_bytes));
      }
    }
  }
}

void xtile_plan_pieces(XtileHost &o, const std::vector<int64_t> &tbase, int64_t piece_nnz) {
  const int64_t S = o.S;
  // ---- gather workgroups: each non-empty tile split into pieces of ≈ piece_nnz.
  //      Order: tiles in runs of 8, and inside a run piece k of the 8 tiles
  //      before piece k + 1, so the pieces of one tile are 8 workgroups
  //      apart — the same XCD under round-robin dispatch — and the x tile
  //      the second one loads is an L2 hit.  (Placement only; any order is
  //      correct.)
  o.pieces.clear();
  const int64_t pn = std::max<int64_t>(8, (piece_nnz + 7) / 8 * 8);
  for (int64_t s0 = 0; s0 < S; s0 += 8) {
    std::vector<int64_t> step(8, 0), np(8, 0);
    int64_t kmax = 0;
    for (int64_t s = s0; s < std::min<int64_t>(S, s0 + 8); ++s) {
      const int64_t len = tbase[s + 1] - tbase[s];
      if (len == 0) continue;
      const int64_t P = (len + pn - 1) / pn;
      step[s - s0] = ((len + P - 1) / P + 7) / 8 * 8;
      np[s - s0] = (len + step[s - s0] - 1) / step[s - s0];
      kmax = std::max(kmax, np[s - s0]);
    }
    for (int64_t k = 0; k < kmax; ++k)
      for (int64_t s = s0; s < std::min<int64_t>(S, s0 + 8); ++s) {
        if (k >= np[s - s0]) continue;
        const int64_t g = tbase[s] + k * step[s - s0];
        o.pieces.push_back(static_cast<int32_t>(g));
        o.pieces.push_back(static_cast<int32_t>(std::min(g + step[s - s0], tbase[s + 1])));
        o.pieces.push_back(static_cast<int32_t>(s));
      }
  }
}

int build_xtile(const void *rp, int bits, const int32_t *col, int64_t n_rows, int64_t n_cols,
                int64_t W, int M, int Rmax, int64_t piece_nnz, int slot_bytes,
                const int64_t *splits, int n_splits, bool iperm, int cut_window, XtileHost &o, int unit) {
  int st = xtile_plan_chunks(rp, bits, col, n_rows, n_cols, W, M, Rmax, slot_bytes, splits, n_splits, iperm,
                             cut_window, o, unit);
  if (st != LHPC_OK) return st;
  const int64_t S = o.S, C = o.n_chunks;
  // ---- per (chunk, tile) counts → segment offsets in (tile, chunk) order
  int32_t *cnt = o.segoff.data() + S;  // row c+1 temporarily holds count[c]
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t c = 0; c < C; ++c) {
    int32_t *cc = cnt + c * S;
    for (int64_t k = o.ce[c]; k < o.ce[c + 1]; ++k) ++cc[col[k] / W];
  }
  std::vector<int64_t> tbase;
  if ((st = xtile_plan_offsets(o, tbase)) != LHPC_OK) return st;
  xtile_plan_scatter_host(col, rp_at(rp, bits, n_rows) - rp_at(rp, bits, 0), o);
  xtile_plan_pieces(o, tbase, piece_nnz);
  return LHPC_OK;
}

int xtile_run_bases(const XtileHost &o, int run, int64_t tail, std::vector<int32_t> &vbase) {
  const int64_t C = o.n_chunks, reg = 64 * static_cast<int64_t>(run);
  std::vector<int64_t> vb(static_cast<size_t>(C) + 1, 0);
  for (int64_t c = 0; c < C; ++c) vb[c + 1] = vb[c] + (o.ce[c + 1] - o.ce[c] + reg - 1) / reg * reg;
  if (vb[C] + tail >= INT32_MAX) return LHPC_ERR_UNSUPPORTED;
  vbase.assign(vb.begin(), vb.end());
  return LHPC_OK;
}

int xtile_transpose_runs(const XtileHost &o, const void *val, size_t tsz, int run, int64_t tail,
                         std::vector<int32_t> &vbase, std::unique_ptr<unsigned char[]> &valt,
                         std::unique_ptr<uint16_t[]> &ipt) {
  const int64_t C = o.n_chunks;
  if (const int st = xtile_run_bases(o, run, tail, vbase)) return st;
  const std::vector<int32_t> &vb = vbase;
  const size_t total = static_cast<size_t>(vb[C] + tail);
  valt.reset(new unsigned char[total * tsz]());
  if (o.iperm) {  // padding points at the reduce's zero slot M (x = 0 there)
    ipt.reset(new uint16_t[total]);
    std::fill(ipt.get(), ipt.get() + total, static_cast<uint16_t>(o.M));
  }
  const int vw = static_cast<int>(16 / tsz);
  const unsigned char *vs = static_cast<const unsigned char *>(val);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t c = 0; c < C; ++c) {
    const int64_t e0 = o.ce[c], m = o.ce[c + 1] - e0;
    for (int64_t i = 0; i < m; ++i) {
      std::memcpy(valt.get() + (vb[c] + xtile_wave_pos(i, run, vw)) * tsz, vs + (e0 + i) * tsz, tsz);
      if (o.iperm) ipt[static_cast<size_t>(vb[c] + xtile_wave_pos(i, run, 8))] = o.iperm[static_cast<size_t>(e0 + i)];
    }
  }
  return LHPC_OK;
}

void xtile_segment_table(const XtileHost &o, std::vector<uint32_t> &seg, std::vector<int32_t> &hi) {
  const int64_t S = o.S, C = o.n_chunks;
  if (o.rdelta.empty()) {
    const int64_t H = (C + kXtSegHi - 1) / kXtSegHi;
    seg.assign(static_cast<size_t>(std::max<int64_t>(C, 1) * S), 0u);
    hi.assign(static_cast<size_t>(std::max<int64_t>(H, 1) * S), 0);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < C; ++c) {
      const int32_t *a = o.segoff.data() + c * S, *b = a + S, *h = o.segoff.data() + (c / kXtSegHi) * kXtSegHi * S;
      if (c % kXtSegHi == 0) std::memcpy(hi.data() + (c / kXtSegHi) * S, a, sizeof(int32_t) * static_cast<size_t>(S));
      for (int64_t s = 0; s < S; ++s)
        seg[static_cast<size_t>(c * S + s)] =
            static_cast<uint32_t>(a[s] - h[s]) | (static_cast<uint32_t>(b[s] - a[s]) << 16);
    }
    return;
  }
  // ring plans: starts in ring positions (stream position + rdelta of the
  // chunk's range), hi groups of kXtSegHi chunks restarting at every range
  // (a group straddling two ranges would mix two rings' positions)
  const int64_t K = static_cast<int64_t>(o.rchunk.size()) - 1;
  std::vector<int64_t> g0;  // first chunk of each hi group, then C (group g of range k: row hrow[k] + …)
  std::vector<int32_t> gk;  // its range
  for (int64_t k = 0; k < K; ++k) {
    for (int64_t c = o.rchunk[k]; c < o.rchunk[k + 1]; c += kXtSegHi) {
      g0.push_back(c);
      gk.push_back(static_cast<int32_t>(k));
    }
  }
  g0.push_back(C);
  const int64_t H = static_cast<int64_t>(g0.size()) - 1;
  seg.assign(static_cast<size_t>(std::max<int64_t>(C, 1) * S), 0u);
  hi.assign(static_cast<size_t>(std::max<int64_t>(H, 1) * S), 0);
#pragma omp parallel for schedule(static)
  for (int64_t g = 0; g < H; ++g) {
    const int32_t *d = o.rdelta.data() + static_cast<int64_t>(gk[g]) * S;
    const int32_t *h = o.segoff.data() + g0[g] * S;
    for (int64_t s = 0; s < S; ++s) hi[static_cast<size_t>(g * S + s)] = h[s] + d[s];
    const int64_t c1 = std::min(g0[g] + kXtSegHi, o.rchunk[gk[g] + 1]);
    for (int64_t c = g0[g]; c < c1; ++c) {
      const int32_t *a = o.segoff.data() + c * S, *b = a + S;
      for (int64_t s = 0; s < S; ++s)
        seg[static_cast<size_t>(c * S + s)] =
            static_cast<uint32_t>(a[s] - h[s]) | (static_cast<uint32_t>(b[s] - a[s]) << 16);
    }
  }
}

void xtile_phase_tables(const XtileHost &o, std::vector<uint32_t> &bt, std::vector<int32_t> &base_ne) {
  const int64_t S = o.S, C = o.n_chunks, M = o.M, NBT = M / 64;
  bt.assign(static_cast<size_t>(std::max<int64_t>(C, 1) * NBT * 4), 0u);
  base_ne.assign(static_cast<size_t>(std::max<int64_t>(C, 1) * S), 0);
  const int64_t K = static_cast<int64_t>(o.rchunk.size()) - 1;
#pragma omp parallel
  {
    std::vector<uint64_t> starts(static_cast<size_t>(NBT));
#pragma omp for schedule(dynamic, 64)
    for (int64_t c = 0; c < C; ++c) {
      int64_t k = 0;  // c's range (for the ring deltas)
      if (!o.rdelta.empty())
        while (k + 1 < K && o.rchunk[k + 1] <= c) ++k;
      std::fill(starts.begin(), starts.end(), uint64_t{0});
      int32_t *bn = base_ne.data() + c * S;
      int64_t flat = 0, nne = 0;
      for (int64_t s = 0; s < S; ++s) {
        const int64_t a = o.segoff[c * S + s], len = o.segoff[(c + 1) * S + s] - a;
        if (len <= 0) continue;
        const int64_t start = a + (o.rdelta.empty() ? 0 : o.rdelta[static_cast<size_t>(k * S + s)]);
        bn[nne++] = static_cast<int32_t>(start - flat);
        starts[static_cast<size_t>(flat / 64)] |= uint64_t{1} << (flat % 64);
        flat += len;
      }
      for (int64_t r = nne; r < S; ++r) bn[r] = nne > 0 ? bn[nne - 1] : 0;
      int64_t before = 0;
      uint32_t *b4 = bt.data() + c * NBT * 4;
      for (int64_t b = 0; b < NBT; ++b) {
        const uint64_t w = starts[static_cast<size_t>(b)], w1 = w >> 1;
        b4[4 * b] = static_cast<uint32_t>(w1);
        b4[4 * b + 1] = static_cast<uint32_t>(w1 >> 32);
        b4[4 * b + 2] = static_cast<uint32_t>(before - 1 + static_cast<int64_t>(w & 1u));
        before += __builtin_popcountll(w);
      }
    }
  }
}

bool csr_has_empty_row(const void *rp, int bits, int64_t n_rows) {
  int any = 0;
#pragma omp parallel for schedule(static) reduction(| : any)
  for (int64_t i = 0; i < n_rows; ++i) any |= rp_at(rp, bits, i + 1) == rp_at(rp, bits, i) ? 1 : 0;
  return any != 0;
}

void xtile_chunk_records(const XtileHost &o, const void *rp, int bits, std::vector<uint32_t> &rec) {
  const int64_t S = o.S, C = o.n_chunks, M = o.M, BW = M / 32, RW = xtile_chunkrec_words(o.M, o.S);
  rec.assign(static_cast<size_t>(std::max<int64_t>(C, 1) * RW), 0u);
  const int64_t K = static_cast<int64_t>(o.rchunk.size()) - 1;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t c = 0; c < C; ++c) {
    int64_t k = 0;  // c's range (for the ring deltas)
    if (!o.rdelta.empty())
      while (k + 1 < K && o.rchunk[k + 1] <= c) ++k;
    uint32_t *bm = rec.data() + c * RW, *sbm = bm + BW;
    int32_t *bn = reinterpret_cast<int32_t *>(sbm + BW);
    int64_t flat = 0, nne = 0;
    for (int64_t s = 0; s < S; ++s) {
      const int64_t a = o.segoff[c * S + s], len = o.segoff[(c + 1) * S + s] - a;
      if (len <= 0) continue;
      const int64_t start = a + (o.rdelta.empty() ? 0 : o.rdelta[static_cast<size_t>(k * S + s)]);
      bn[nne++] = static_cast<int32_t>(start - flat);
      sbm[flat >> 5] |= 1u << (flat & 31);
      flat += len;
    }
    for (int64_t r = nne; r < S; ++r) bn[r] = nne > 0 ? bn[nne - 1] : 0;
    const int64_t e0 = o.ce[c], m = o.ce[c + 1] - e0, r0 = o.cr[c], r1 = o.cr[c + 1];
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t i = rp_at(rp, bits, r) - e0;
      if (i >= 0 && i < m) bm[i >> 5] |= 1u << (i & 31);
    }
    bn[S] = rp_at(rp, bits, r1) - e0 > m ? 1 : 0;
  }
}

void xtile_ring_pieces(XtileHost &o, int64_t piece_nnz, std::vector<int64_t> &rpc) {
  const int64_t S = o.S, K = static_cast<int64_t>(o.rchunk.size()) - 1;
  const int64_t pn = std::max<int64_t>(8, (piece_nnz + 7) / 8 * 8);
  auto up8 = [](int64_t v) { return (v + 7) / 8 * 8; };
  auto dn8 = [](int64_t v) { return v / 8 * 8; };
  o.pieces.clear();
  o.pext.clear();
  o.rdelta.assign(static_cast<size_t>(K * S), 0);
  o.ring_len = 0;
  o.hrow.assign(1, 0);  // hi groups of kXtSegHi chunks per range (xtile_segment_table)
  for (int64_t k = 0; k + 1 < K; ++k)
    o.hrow.push_back(o.hrow.back() + (o.rchunk[k + 1] - o.rchunk[k] + kXtSegHi - 1) / kXtSegHi);
  rpc.assign(1, 0);
  for (int64_t k = 0; k < K; ++k) {
    int64_t cur = 0;  // ring cursor (a multiple of 8)
    for (int64_t s = 0; s < S; ++s) {
      const int64_t a = o.segoff[o.rchunk[k] * S + s], b = o.segoff[o.rchunk[k + 1] * S + s];
      if (b <= a) continue;
      const int64_t d = cur - dn8(a);  // ring position of stream position g: g + d
      o.rdelta[static_cast<size_t>(k * S + s)] = static_cast<int32_t>(d);
      cur += up8(b) - dn8(a);
      // whole groups [ia, ib) in ≈ piece_nnz pieces; the partial groups at a
      // and b ride on the first / last piece as flagged extra groups
      const int64_t ia = up8(a), ib = dn8(b);
      const bool pre = a % 8 != 0, suf = b % 8 != 0 && ib >= ia;
      if (ib <= ia) {  // no whole group: one piece holding the group(s) around a (and b)
        o.pieces.insert(o.pieces.end(), {static_cast<int32_t>(ia), static_cast<int32_t>(ia), static_cast<int32_t>(s)});
        o.pext.insert(o.pext.end(), {static_cast<int32_t>(d), (pre ? 1 : 0) | (suf ? 2 : 0)});
        continue;
      }
      const int64_t P = (ib - ia + pn - 1) / pn, step = up8((ib - ia + P - 1) / P);
      for (int64_t g = ia; g < ib; g += step) {
        const int64_t e = std::min(ib, g + step);
        o.pieces.insert(o.pieces.end(), {static_cast<int32_t>(g), static_cast<int32_t>(e), static_cast<int32_t>(s)});
        o.pext.insert(o.pext.end(), {static_cast<int32_t>(d), (g == ia && pre ? 1 : 0) | (e == ib && suf ? 2 : 0)});
      }
    }
    o.ring_len = std::max(o.ring_len, cur);
    rpc.push_back(static_cast<int64_t>(o.pieces.size() / 3));
  }
}

void xtile_range_pieces(XtileHost &o, int64_t piece_nnz, std::vector<int64_t> &rpc) {
  const int64_t S = o.S, K = static_cast<int64_t>(o.rchunk.size()) - 1;
  const int64_t pn = std::max<int64_t>(8, (piece_nnz + 7) / 8 * 8);
  auto up8 = [](int64_t v) { return (v + 7) / 8 * 8; };
  o.pieces.clear();
  rpc.assign(1, 0);
  for (int64_t k = 0; k < K; ++k) {
    for (int64_t s = 0; s < S; ++s) {
      const int64_t a = up8(o.segoff[o.rchunk[k] * S + s]), b = up8(o.segoff[o.rchunk[k + 1] * S + s]);
      if (b <= a) continue;
      const int64_t P = (b - a + pn - 1) / pn, step = up8((b - a + P - 1) / P);
      for (int64_t g = a; g < b; g += step) {
        o.pieces.push_back(static_cast<int32_t>(g));
        o.pieces.push_back(static_cast<int32_t>(std::min(b, g + step)));
        o.pieces.push_back(static_cast<int32_t>(s));
      }
    }
    rpc.push_back(static_cast<int64_t>(o.pieces.size() / 3));
  }
}

void xtile_permute_gather_blocks(XtileHost &o, int vw) {
  const int64_t np = static_cast<int64_t>(o.pieces.size() / 3);
#pragma omp parallel for schedule(dynamic, 4)
  for (int64_t b = 0; b < np; ++b) {
    const int64_t g0 = o.pieces[3 * b], g1 = o.pieces[3 * b + 1];
    uint16_t tmp[512];
    for (int64_t g = g0; g + 512 <= g1; g += 512) {
      uint16_t *c = o.col16.get() + g;
      for (int l = 0; l < 64; ++l)
        for (int k = 0; k < 8; ++k) tmp[8 * l + k] = c[xtile_gather_pos(k, l, vw)];
      std::memcpy(c, tmp, sizeof(tmp));
    }
  }
}

}  // namespace lhpc
