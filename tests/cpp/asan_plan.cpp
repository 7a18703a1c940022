// asan_plan.cpp — host-only driver for the plan-time and I/O code of
// liblhpc.so (lhpc_plan.cpp, lhpc_gen.cpp, lhpc_io.cpp compiled into this
// binary with -fsanitize=address,undefined; no HIP).  Mirrors the reference's
// policy of running every Linux test under ASan
// (/root/reference/tests/CMakeLists.txt:6-9) for the code a GPU box cannot
// sanitize: the CSR validation and the XSLICE / XTILE re-encodings that index
// host arrays by caller-supplied row_ptr / col_idx, and the file readers.
// Built and run by tests/test_asan.py (`make -C tests/cpp asan`).
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lhpc.h"
#include "../../libhpc_amd/csrc/lhpc_plan.hpp"

static int failures = 0;
#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c)) {                                                              \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      ++failures;                                                            \
    }                                                                        \
  } while (0)

namespace {

struct Csr {
  int64_t n = 0, m = 0;
  std::vector<int64_t> rp;
  std::vector<int32_t> col;
  std::vector<float> val;
};

Csr uniform(int64_t n, int64_t m, int per_row, uint64_t seed) {
  Csr a;
  a.n = n;
  a.m = m;
  a.rp.resize(static_cast<size_t>(n + 1));
  CHECK(lhpc_gen_uniform_row_ptr(n, per_row, a.rp.data()) == 0);
  a.col.resize(static_cast<size_t>(a.rp[n]));
  CHECK(lhpc_gen_fill_cols(n, m, a.rp.data(), seed, a.col.data()) == 0);
  a.val.resize(a.col.size());
  CHECK(lhpc_gen_fill_values(LHPC_F32, 0, static_cast<int64_t>(a.val.size()), seed + 1, a.val.data()) == 0);
  return a;
}

Csr powerlaw(int64_t n, int64_t m, int64_t lmax, uint64_t seed) {
  Csr a;
  a.n = n;
  a.m = m;
  a.rp.resize(static_cast<size_t>(n + 1));
  int64_t nnz = 0;
  CHECK(lhpc_gen_powerlaw_row_ptr(n, m, 1.792, 1, lmax, seed, a.rp.data(), &nnz) == 0);
  a.col.resize(static_cast<size_t>(nnz));
  CHECK(lhpc_gen_fill_cols(n, m, a.rp.data(), seed, a.col.data()) == 0);
  a.val.resize(a.col.size());
  CHECK(lhpc_gen_fill_values(LHPC_F32, 0, nnz, seed + 1, a.val.data()) == 0);
  return a;
}

// XTILE invariants: every CSR nonzero appears once in its chunk's segment
// concatenation, with the column it had; chunks tile the CSR order.
// unit > 1 (aligned segments): every segment starts and ends on a multiple
// of unit, the padded concatenation stays ≤ M, iperm skips the padding.
void check_xtile(const Csr &a, bool iperm, const std::vector<int64_t> &splits, int cut = 512, int unit = 1) {
  const int64_t W = 4096;
  const int M = 1024, Rmax = 128;
  lhpc::XtileHost xt;
  const int rc = lhpc::build_xtile(a.rp.data(), 64, a.col.data(), a.n, a.m, W, M, Rmax, 3000, 4,
                                   splits.empty() ? nullptr : splits.data(), static_cast<int>(splits.size()), iperm,
                                   cut, xt, unit);
  CHECK(rc == 0);
  if (rc) return;
  const int64_t C = xt.n_chunks, S = xt.S;
  CHECK(xt.ce.front() == 0 && xt.ce[static_cast<size_t>(C)] == a.rp[a.n]);
  for (int64_t c = 0; c < C; ++c) {
    const int64_t e0 = xt.ce[c], e1 = xt.ce[c + 1];
    CHECK(e1 >= e0 && e1 - e0 <= M);
    std::vector<int> seen(static_cast<size_t>(M), 0);
    int64_t flat = 0;
    for (int64_t s = 0; s < S; ++s) {
      const int64_t g0 = xt.segoff[c * S + s], g1 = xt.segoff[(c + 1) * S + s];
      CHECK(g0 <= g1 && g1 <= xt.total);
      CHECK(g0 % unit == 0 && (g1 - g0) % unit == 0);
      for (int64_t g = g0; g < g1; ++g, ++flat) {
        if (iperm) continue;
        (void)xt.perm[g];  // perm mode: every stream entry has a slot
      }
    }
    CHECK(unit == 1 ? flat == e1 - e0 : (flat >= e1 - e0 && flat <= M));
    if (iperm) {
      for (int64_t k = e0; k < e1; ++k) {
        const int f = xt.iperm[k];
        CHECK(f >= 0 && f < flat);
        if (f >= 0 && f < flat) ++seen[static_cast<size_t>(f)];
      }
      int64_t hits = 0;
      for (int v : seen) {
        CHECK(v <= 1);
        hits += v;
      }
      CHECK(hits == e1 - e0);
    }
  }
  // cache-sized ranges: range pieces cover the stream once, and every entry
  // of range k is gathered by range k's pieces or an earlier range's
  {
    std::vector<int64_t> rpc;
    lhpc::xtile_range_pieces(xt, 700, rpc);
    const int64_t K = static_cast<int64_t>(xt.rchunk.size()) - 1;
    CHECK(static_cast<int64_t>(rpc.size()) == K + 1 && static_cast<size_t>(rpc[K]) == xt.pieces.size() / 3);
    std::vector<int> by(static_cast<size_t>(xt.total), -1);
    for (int64_t k = 0; k < K; ++k)
      for (int64_t q = rpc[k]; q < rpc[k + 1]; ++q) {
        const int64_t g0 = xt.pieces[3 * q], g1 = xt.pieces[3 * q + 1], s = xt.pieces[3 * q + 2];
        CHECK(g0 % 8 == 0 && g0 < g1 && g1 <= xt.total && s >= 0 && s < S);
        for (int64_t g = g0; g < g1 && g < xt.total; ++g) {
          CHECK(by[static_cast<size_t>(g)] < 0);
          by[static_cast<size_t>(g)] = static_cast<int>(k);
        }
      }
    for (int64_t k = 0; k < K; ++k)
      for (int64_t s = 0; s < S; ++s)
        for (int64_t g = xt.segoff[xt.rchunk[k] * S + s]; g < xt.segoff[xt.rchunk[k + 1] * S + s]; ++g)
          CHECK(by[static_cast<size_t>(g)] >= 0 && by[static_cast<size_t>(g)] <= k);
  }
  // phase-A tables (xtile_phase_tables): position f of chunk c's segment
  // concatenation lies in non-empty segment rank = term + popcount(w1 &
  // lanes below f % 64) of its 64-position batch, and its xg entry is at
  // base_ne[rank] + f — the stream (or, after xtile_ring_pieces, the ring)
  // position of that entry
  auto check_phase_tables = [&]() {
    std::vector<uint32_t> bt;
    std::vector<int32_t> bne;
    lhpc::xtile_phase_tables(xt, bt, bne);
    const int64_t NBT = xt.M / 64, K = static_cast<int64_t>(xt.rchunk.size()) - 1;
    CHECK(static_cast<int64_t>(bt.size()) == std::max<int64_t>(C, 1) * NBT * 4);
    for (int64_t c = 0; c < C; ++c) {
      int64_t k = 0;
      while (k + 1 < K && xt.rchunk[k + 1] <= c) ++k;
      int64_t flat = 0;
      for (int64_t s = 0; s < S; ++s) {
        const int64_t a = xt.segoff[c * S + s], len = xt.segoff[(c + 1) * S + s] - a;
        const int64_t d = xt.rdelta.empty() ? 0 : xt.rdelta[static_cast<size_t>(k * S + s)];
        for (int64_t j = 0; j < len; ++j, ++flat) {
          const int64_t b = flat / 64, l = flat % 64;
          const uint32_t *t4 = bt.data() + (c * NBT + b) * 4;
          const uint64_t w1 = (static_cast<uint64_t>(t4[1]) << 32) | t4[0];
          const int64_t rank = static_cast<int32_t>(t4[2]) + __builtin_popcountll(w1 & ((uint64_t{1} << l) - 1));
          CHECK(rank >= 0 && rank < S);
          if (rank >= 0 && rank < S) CHECK(bne[static_cast<size_t>(c * S + rank)] + flat == a + j + d);
        }
      }
    }
  };
  if (iperm && unit == 1) check_phase_tables();
  // the xg ring (xtile_ring_pieces): per range, emulate the gather (every
  // piece writes stream entry g at ring position g + delta, plus its flagged
  // shared groups) on a ring wiped before the range, then the reduce's reads
  // through the segment table (hi row hrow[k] + ⌊(c − rchunk[k]) / 7⌋):
  // every segment must read back exactly its own stream entries
  if (iperm && unit == 1 && xt.rchunk.size() > 2) {
    std::vector<int64_t> rpc;
    lhpc::xtile_ring_pieces(xt, 700, rpc);
    std::vector<uint32_t> seg;
    std::vector<int32_t> hi;
    lhpc::xtile_segment_table(xt, seg, hi);
    const int64_t K = static_cast<int64_t>(xt.rchunk.size()) - 1, L = xt.ring_len;
    CHECK(L > 0 && L <= xt.total + 16 * S && static_cast<int64_t>(xt.hrow.size()) == K);
    CHECK(xt.pext.size() == xt.pieces.size() / 3 * 2);
    std::vector<int64_t> ring(static_cast<size_t>(L));
    for (int64_t k = 0; k < K; ++k) {
      std::fill(ring.begin(), ring.end(), -1);
      for (int64_t q = rpc[k]; q < rpc[k + 1]; ++q) {
        const int64_t g0 = xt.pieces[3 * q], g1 = xt.pieces[3 * q + 1], d = xt.pext[2 * q], fl = xt.pext[2 * q + 1];
        CHECK(g0 % 8 == 0 && g1 % 8 == 0 && g0 <= g1 && d % 8 == 0);
        auto put = [&](int64_t g) {
          CHECK(g >= 0 && g < xt.total && g + d >= 0 && g + d < L);
          if (g + d >= 0 && g + d < L) {
            CHECK(ring[static_cast<size_t>(g + d)] < 0);  // no two writers in one range
            ring[static_cast<size_t>(g + d)] = g;
          }
        };
        for (int64_t g = g0; g < g1; ++g) put(g);
        if (fl & 1)
          for (int64_t g = g0 - 8; g < g0; ++g) put(g);
        if (fl & 2)
          for (int64_t g = g1; g < g1 + 8; ++g) put(g);
      }
      for (int64_t c = xt.rchunk[k]; c < xt.rchunk[k + 1]; ++c)
        for (int64_t s = 0; s < S; ++s) {
          const uint32_t w = seg[static_cast<size_t>(c * S + s)];
          const int64_t h = xt.hrow[k] + (c - xt.rchunk[k]) / lhpc::kXtSegHi;
          const int64_t start = hi[static_cast<size_t>(h * S + s)] + static_cast<int64_t>(w & 0xFFFFu), len = w >> 16;
          CHECK(len == xt.segoff[(c + 1) * S + s] - xt.segoff[c * S + s]);
          for (int64_t j = 0; j < len; ++j)
            CHECK(start + j >= 0 && start + j < L && ring[static_cast<size_t>(start + j)] == xt.segoff[c * S + s] + j);
        }
    }
    check_phase_tables();  // with the ring deltas
  }
  // the transposed val/iperm streams and the gather-block permutation
  std::vector<int32_t> vbase;
  std::unique_ptr<unsigned char[]> valt;
  std::unique_ptr<uint16_t[]> ipt;
  CHECK(lhpc::xtile_transpose_runs(xt, a.val.data(), 4, 16, 64 * 16, vbase, valt, ipt) == 0);
  CHECK(static_cast<int64_t>(vbase.size()) == C + 1);
  lhpc::xtile_permute_gather_blocks(xt, 4);
}

// The XTILE plan-build decisions (lhpc_plan.hpp xtile_tile_width,
// xtile_policy, xtile_partition_policy) at full-size shapes, cus = 256.
// Expected values are those of the plan build before these functions existed:
//   W, tiles, ranges of C2 / C3 / the n = 80M column block are what info()
//   reported for plans built on the GPU then (slice_width, slices, launches =
//   2 per range and part: C2 39063 / 256 / 6, C3 20480 / 489 / 12, n = 80M
//   three column blocks of 40960 / 652 / 2 each);
//   everything else (iperm, aligned, ring, pre, nt, pieces, and every row
//   without such a plan) is HAND-DERIVED from that build's code.
// G (the reduce's segment-table entries per thread, the kernel file's
// xtile_g) is an input: 1 up to 512 fp32 / 1024 fp64 tiles (fp32 ≈ 476–512:
// 2), then ⌈tiles / 512⌉ resp. ⌈tiles / 1024⌉ rounded up to a power of two.
struct PolicyCase {
  const char *name;
  int64_t n_rows, n_cols, nnz;
  int elem_bytes, n_user_splits, G;
  bool dev;
  void (*set)(lhpc_options &);
  // expected
  int64_t W, tiles, min_piece, piece;
  bool iperm, aligned, supported;
  int cut, ranges;
  bool own_cuts, pre;
  int steps;
  int K;  // the final range count the three below are asked at
  bool ring, nt;
  int64_t range_piece;
};

void check_xtile_policy() {
  constexpr int64_t C2N = 10000000, C2Z = 150000000, MB256 = int64_t{256} << 20;
  const PolicyCase cases[] = {
      // full sizes, default options
      {"C2", C2N, C2N, C2Z, 4, 0, 1, true, nullptr,
       39063, 256, 104168, 292969, true, false, true, 256, 3, true, false, 8, 3, true, false, 244141},
      {"C3", C2N, C2N, C2Z, 8, 0, 1, true, nullptr,
       20480, 489, 65536, 292969, true, false, true, 256, 6, true, true, 8, 6, true, false, 122071},
      {"n80m whole", 80000000, 80000000, 1200000000, 4, 0, 4, true, nullptr,
       39063, 2048, 104168, 2343751, false, false, true, 256, 0, false, false, 8, 0, false, true, 0},
      {"n80m column block", 80000000, 26666624, 400000000, 4, 0, 2, true, nullptr,
       40960, 652, 109226, 781251, true, false, true, 256, 0, false, false, 8, 0, false, true, 0},
      {"n150m whole", 150000000, 150000000, 2250000000, 4, 0, 8, true, nullptr,
       39063, 3840, 104168, 4394532, false, false, true, 256, 0, false, false, 8, 0, false, true, 0},
      // a rank's rows of C2 at two ranks, user splits: ranges only on request of the ring (fp64)
      {"rank f32", 5000000, C2N, 75000000, 4, 3, 1, false, nullptr,
       39063, 256, 104168, 146485, true, false, true, 256, 2, false, false, 8, 4, false, false, 104168},
      {"rank f32 ring 2", 5000000, C2N, 75000000, 4, 3, 1, false, [](lhpc_options &o) { o.xtile_ring = 2; },
       39063, 256, 104168, 146485, true, false, true, 256, 2, false, false, 8, 4, true, false, 104168},
      {"rank f64", 5000000, C2N, 75000000, 8, 3, 1, false, nullptr,
       20480, 489, 65536, 146485, true, false, true, 256, 0, false, true, 8, 0, false, true, 0},
      {"rank f64 ring 2", 5000000, C2N, 75000000, 8, 3, 1, false, [](lhpc_options &o) { o.xtile_ring = 2; },
       20480, 489, 65536, 146485, true, false, true, 256, 3, false, true, 8, 4, true, false, 91553},
      // one option each, on C2 (C3 where the default differs there)
      {"reduce perm", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_reduce = LHPC_XTILE_REDUCE_PERM; },
       39063, 256, 104168, 292969, false, false, true, 256, 3, true, false, 8, 3, false, false, 244141},
      {"align units", C2N, C2N, C2Z, 4, 0, 1, false, [](lhpc_options &o) { o.xtile_align = LHPC_XTILE_ALIGN_UNITS; },
       39063, 256, 104168, 292969, true, true, true, 256, 3, true, false, 8, 3, false, false, 244141},
      {"align units, device", C2N, C2N, C2Z, 4, 0, 1, true,
       [](lhpc_options &o) { o.xtile_align = LHPC_XTILE_ALIGN_UNITS; },
       39063, 256, 104168, 292969, true, true, false, 256, 3, true, false, 8, 3, false, false, 244141},
      {"align units, G 8", 150000000, 150000000, 400000000, 4, 0, 8, false,
       [](lhpc_options &o) { o.xtile_align = LHPC_XTILE_ALIGN_UNITS; },
       39063, 3840, 104168, 781251, true, false, true, 256, 0, false, false, 8, 0, false, true, 0},
      {"ranges 5", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_ranges = 5; },
       39063, 256, 104168, 292969, true, false, true, 256, 5, true, false, 8, 5, true, false, 146484},
      {"ring 1", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_ring = 1; },
       39063, 256, 104168, 292969, true, false, true, 256, 3, true, false, 8, 3, false, false, 244141},
      {"ring 1, C3", C2N, C2N, C2Z, 8, 0, 1, true, [](lhpc_options &o) { o.xtile_ring = 1; },
       20480, 489, 65536, 292969, true, false, true, 256, 0, false, true, 8, 0, false, true, 0},
      {"pretable 2", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_pretable = 2; },
       39063, 256, 104168, 292969, true, false, true, 256, 3, true, true, 8, 3, true, false, 244141},
      {"pretable 1, C3", C2N, C2N, C2Z, 8, 0, 1, true, [](lhpc_options &o) { o.xtile_pretable = 1; },
       20480, 489, 65536, 292969, true, false, true, 256, 6, true, false, 8, 6, true, false, 122071},
      {"pretable 2, G 2", 80000000, 26666624, 400000000, 4, 0, 2, true, [](lhpc_options &o) { o.xtile_pretable = 2; },
       40960, 652, 109226, 781251, true, false, true, 256, 0, false, false, 8, 0, false, true, 0},
      {"store nt", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_store = LHPC_STORE_NT; },
       39063, 256, 104168, 292969, true, false, true, 256, 3, true, false, 8, 3, true, true, 244141},
      {"store plain", 80000000, 26666624, 400000000, 4, 0, 2, true, [](lhpc_options &o) { o.xtile_store = LHPC_STORE_PLAIN; },
       40960, 652, 109226, 781251, true, false, true, 256, 0, false, false, 8, 0, false, false, 0},
      {"steps 3", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_steps = 3; },
       39063, 256, 104168, 292969, true, false, true, 256, 3, true, false, 4, 3, true, false, 244141},
      {"steps 16", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_steps = 16; },
       39063, 256, 104168, 292969, true, false, true, 256, 3, true, false, 16, 3, true, false, 244141},
      {"cut 64", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_cut = 64; },
       39063, 256, 104168, 292969, true, false, true, 64, 3, true, false, 8, 3, true, false, 244141},
      {"cut past M", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_cut = 100000; },
       39063, 256, 104168, 292969, true, false, true, 8192, 3, true, false, 8, 3, true, false, 244141},
      {"piece 1000", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_piece = 1000; },
       39063, 256, 104168, 1000, true, false, true, 256, 3, true, false, 8, 3, true, false, 244141},
      {"range piece 200", C2N, C2N, C2Z, 4, 0, 1, true, [](lhpc_options &o) { o.xtile_range_piece = 200; },
       39063, 256, 104168, 292969, true, false, true, 256, 3, true, false, 8, 3, true, false, 200},
      // xg at the 256 MB Infinity Cache and one entry past it (25 tiles)
      {"xg = 256 MB", 1000000, 1000000, MB256 / 4, 4, 0, 1, true, nullptr,
       40960, 25, 109226, 131073, true, false, true, 256, 0, false, false, 8, 0, false, false, 0},
      {"xg > 256 MB", 1000000, 1000000, MB256 / 4 + 1, 4, 0, 1, true, nullptr,
       40960, 25, 109226, 131073, true, false, true, 256, 2, true, false, 8, 2, true, false, 163841},
      {"xg > 256 MB, one range", 1000000, 1000000, MB256 / 4 + 1, 4, 0, 1, true,
       [](lhpc_options &o) { o.xtile_ranges = 1; },
       40960, 25, 109226, 131073, true, false, true, 256, 1, false, false, 8, 1, false, true, 0},
      // eight 200-MB ranges, and one entry more (nine: one range)
      {"k = 8", 1000000, 1000000, 419430400, 4, 0, 1, true, nullptr,
       40960, 25, 109226, 819201, true, false, true, 256, 8, true, false, 8, 8, true, false, 256001},
      {"k = 9", 1000000, 1000000, 419430401, 4, 0, 1, true, nullptr,
       40960, 25, 109226, 819201, true, false, true, 256, 0, false, false, 8, 0, false, true, 0},
      // too few nonzeros per (range, tile) for ranges: C2's nonzeros over 8 times the columns
      {"wide x", C2N, 80000000, C2Z, 4, 0, 4, true, nullptr,
       39063, 2048, 104168, 292969, true, false, true, 256, 0, false, false, 8, 0, false, true, 0},
      // the iperm reduce's 32-bit xg offsets: (nnz + 8·25 + 2·8192)·4 B just below 2 GiB, and at it
      {"iperm below 2 GiB", 1000000, 1000000, 536854327, 4, 0, 1, true, nullptr,
       40960, 25, 109226, 1048544, true, false, true, 256, 0, false, false, 8, 0, false, true, 0},
      {"iperm at 2 GiB", 1000000, 1000000, 536854328, 4, 0, 1, true, nullptr,
       40960, 25, 109226, 1048544, false, false, true, 256, 0, false, false, 8, 0, false, true, 0},
  };
  for (const PolicyCase &c : cases) {
    lhpc_options o{};  // as lhpc_options_init: every choice automatic
    o.struct_size = sizeof(o);
    if (c.set) c.set(o);
    lhpc::XtileShape s;
    s.n_rows = c.n_rows;
    s.n_cols = c.n_cols;
    s.nnz = c.nnz;
    s.elem_bytes = c.elem_bytes;
    s.M = 8192;
    s.cus = 256;
    s.n_user_splits = c.n_user_splits;
    s.dev_build = c.dev;
    s.W = lhpc::xtile_tile_width(c.n_cols, static_cast<size_t>(c.elem_bytes), 256);
    s.G = c.G;
    const lhpc::XtilePolicy p = lhpc::xtile_policy(s, o);
    const bool ok = p.W == c.W && p.tiles == c.tiles && p.min_piece == c.min_piece && p.piece == c.piece &&
                    p.iperm == c.iperm && p.aligned == c.aligned && p.supported == c.supported && p.cut == c.cut &&
                    p.ranges == c.ranges && p.own_cuts == c.own_cuts && p.pre == c.pre && p.steps == c.steps &&
                    p.ring(c.K) == c.ring && p.nt(c.K) == c.nt && (c.K <= 1 || p.range_piece(c.K) == c.range_piece);
    if (!ok)
      std::fprintf(stderr,
                   "xtile_policy %s: W %lld tiles %lld min_piece %lld piece %lld iperm %d aligned %d supported %d "
                   "cut %d ranges %d own_cuts %d pre %d steps %d ring %d nt %d range_piece %lld\n",
                   c.name, (long long)p.W, (long long)p.tiles, (long long)p.min_piece, (long long)p.piece, p.iperm,
                   p.aligned, p.supported, p.cut, p.ranges, p.own_cuts, p.pre, p.steps, p.ring(c.K), p.nt(c.K),
                   (long long)(c.K > 1 ? p.range_piece(c.K) : 0));
    CHECK(ok);
  }
  // the tile width alone: the 10% rule's last accepted and first rejected
  // tile count (233 / 232 → 256), the 4096-tile cap (4097 → 4352 tiles is
  // within 10%; on 304 CUs 4000 → 4256), fp64 never, and the override
  CHECK(lhpc::xtile_tile_width(40960 * 233, 4, 256) == 37280);
  CHECK(lhpc::xtile_tile_width(40960 * 232, 4, 256) == 40960);
  CHECK(lhpc::xtile_tile_width(40960 * 3900, 4, 256) == 39000);
  CHECK(lhpc::xtile_tile_width(int64_t{40960} * 4097, 4, 256) == 40960);
  CHECK(lhpc::xtile_tile_width(40960 * 4000, 4, 304) == 40960);
  CHECK(lhpc::xtile_tile_width(20480 * 245, 8, 256) == 20480);
  CHECK(lhpc::xtile_tile_width(C2N, 4, 256, 0) == 40960);
  CHECK(lhpc::xtile_tile_width(20480 * 245, 8, 256, 1) == 19600);

  // xtile_partition_policy: {tiles, cap, column blocks, parts}; cap = 2^31 − 1
  // − 8·(tiles + 256) − 2^16.  HAND-DERIVED but for n = 80M's three blocks.
  struct PartCase {
    const char *name;
    int64_t n_rows, n_cols, nnz;
    size_t elem_bytes;
    int n_splits;
    void (*set)(lhpc_options &);
    int64_t tiles, cap;
    int B;
    bool parts;
  };
  const PartCase parts[] = {
      {"C2", C2N, C2N, C2Z, 4, 0, nullptr, 245, 2147414103, 1, false},
      {"C3", C2N, C2N, C2Z, 8, 0, nullptr, 489, 2147412151, 1, false},
      {"n80m", 80000000, 80000000, 1200000000, 4, 0, nullptr, 1954, 2147400431, 3, true},
      {"n150m", 150000000, 150000000, 2250000000, 4, 0, nullptr, 3663, 2147386759, 3, true},
      {"n80m, user splits", 80000000, 80000000, 1200000000, 4, 3, nullptr, 1954, 2147400431, 1, false},
      {"col blocks 2", C2N, C2N, C2Z, 4, 0, [](lhpc_options &o) { o.xtile_col_blocks = 2; }, 245, 2147414103, 2, true},
      {"col blocks 2, user splits", C2N, C2N, C2Z, 4, 2, [](lhpc_options &o) { o.xtile_col_blocks = 2; }, 245,
       2147414103, 1, false},
      {"part nnz", C2N, C2N, C2Z, 4, 0, [](lhpc_options &o) { o.xtile_part_nnz = 50000000; }, 245, 50000000, 1, true},
      {"part nnz, user splits", C2N, C2N, C2Z, 4, 1, [](lhpc_options &o) { o.xtile_part_nnz = 50000000; }, 245,
       50000000, 1, false},
      // short rows bound the blocks: 8200 tiles, 10 per row → 2 blocks of 4100 tiles > 4096: no parts
      {"4100 tiles per block", 1000000, int64_t{40960} * 8200, 10000000, 4, 0, nullptr, 8200, 2147350463, 2, false},
      {"2734 tiles per block", 1000000, int64_t{40960} * 8200, 15000000, 4, 0, nullptr, 8200, 2147350463, 3, true},
  };
  for (const PartCase &c : parts) {
    lhpc_options o{};  // as lhpc_options_init: every choice automatic
    o.struct_size = sizeof(o);
    if (c.set) c.set(o);
    const lhpc::XtilePartition r = lhpc::xtile_partition_policy(c.n_rows, c.n_cols, c.nnz, c.elem_bytes, c.n_splits, o);
    const bool ok = r.tiles == c.tiles && r.cap == c.cap && r.col_blocks == c.B && r.parts == c.parts;
    if (!ok)
      std::fprintf(stderr, "xtile_partition_policy %s: tiles %lld cap %lld B %d parts %d\n", c.name,
                   (long long)r.tiles, (long long)r.cap, r.col_blocks, r.parts);
    CHECK(ok);
  }
}

// The kernel-family decision of plan creation (lhpc_plan.hpp
// spmv_wants_locality, spmv_family_policy).  Expected values are read off the
// plan creation code as it was before these functions existed (one copy for
// host arrays, one for device arrays), HAND-DERIVED.  Defaults: fp32, no
// flags, automatic options, no user splits, 100000 rows, 500000 nonzeros,
// longest row 5; stages are listed in the order they are attempted.
void check_spmv_family_policy() {
  constexpr unsigned RG = LHPC_PLAN_FORCE_ROWGROUP, AD = LHPC_PLAN_FORCE_ADAPTIVE, XS = LHPC_PLAN_FORCE_XSLICE,
                     XT = LHPC_PLAN_FORCE_XTILE, SE = LHPC_PLAN_FORCE_SELL;
  constexpr int ADAPTIVE = LHPC_KERNEL_ADAPTIVE, ROWGROUP = LHPC_KERNEL_ROWGROUP;
  struct Case {
    const char *name;
    unsigned flags;
    size_t elem_bytes;
    int64_t n_rows, n_cols, nnz, max_row_len;
    double lines_per_nnz;
    void (*set)(lhpc_options &);
    // expected
    bool wants, xtile, xslice, sell, force_sell;
    int kernel, L, R, csr_status;  // L = 0: not compared (ADAPTIVE has no shape)
  };
  const int64_t N = 100000, Z = 500000;
  const Case cases[] = {
      // the 8.0e6-byte threshold of x is strict
      {"x = 8.0e6 B", 0, 4, N, 2000000, Z, 5, 1.0, nullptr, false, false, false, true, false, ADAPTIVE, 0, 0, 0},
      {"x = 8.0e6 B + 4", 0, 4, N, 2000001, Z, 5, 0.0, nullptr, true, false, false, true, false, ADAPTIVE, 0, 0, 0},
      {"fp64 x = 8.0e6 B", 0, 8, N, 1000000, Z, 5, 1.0, nullptr, false, false, false, true, false, ADAPTIVE, 0, 0, 0},
      {"fp64 x = 8.0e6 B + 8", 0, 8, N, 1000001, Z, 5, 0.0, nullptr, true, false, false, true, false, ADAPTIVE, 0, 0, 0},
      // local at the threshold (> is strict), not local above it
      {"lines 0.25", 0, 4, N, 3000000, Z, 5, 0.25, nullptr, true, false, false, true, false, ADAPTIVE, 0, 0, 0},
      {"lines 0.26", 0, 4, N, 3000000, Z, 5, 0.26, nullptr, true, true, true, true, false, ADAPTIVE, 0, 0, 0},
      {"locality 0.5, lines 0.4", 0, 4, N, 3000000, Z, 5, 0.4, [](lhpc_options &o) { o.spmv_locality = 0.5; },
       true, false, false, true, false, ADAPTIVE, 0, 0, 0},
      {"locality 0.5, lines 0.6", 0, 4, N, 3000000, Z, 5, 0.6, [](lhpc_options &o) { o.spmv_locality = 0.5; },
       true, true, true, true, false, ADAPTIVE, 0, 0, 0},
      {"no xtile", 0, 4, N, 3000000, Z, 5, 1.0, [](lhpc_options &o) { o.spmv_no_xtile = 1; },
       true, false, true, true, false, ADAPTIVE, 0, 0, 0},
      {"not local, nnz 0", 0, 4, N, 3000000, 0, 0, 1.0, nullptr, true, true, false, true, false, ADAPTIVE, 0, 0, 0},
      {"no rows", 0, 4, 0, 3000000, 0, 0, 1.0, nullptr, true, false, false, false, false, ADAPTIVE, 0, 0, 0},
      // forced families: no automatic choice beside them
      {"force xtile, small x", XT, 4, N, N, Z, 5, 1.0, nullptr, false, true, false, false, false, ADAPTIVE, 0, 0, 0},
      {"force xslice", XS, 4, N, N, Z, 5, 1.0, nullptr, false, false, true, false, false, ADAPTIVE, 0, 0, 0},
      {"force sell, longest 8", SE, 4, N, N, Z, 8, 1.0, nullptr, false, false, false, true, true, ADAPTIVE, 0, 0, 0},
      {"force sell, longest 9", SE, 4, N, N, Z, 9, 1.0, nullptr, false, false, false, false, true, ADAPTIVE, 0, 0, 0},
      {"force sell, no rows", SE, 4, 0, N, 0, 0, 1.0, nullptr, false, false, false, false, true, ADAPTIVE, 0, 0, 0},
      {"auto, longest 9", 0, 4, N, N, Z, 9, 1.0, nullptr, false, false, false, false, false, ADAPTIVE, 0, 0, 0},
      {"no sell", 0, 4, N, N, Z, 5, 1.0, [](lhpc_options &o) { o.spmv_no_sell = 1; },
       false, false, false, false, false, ADAPTIVE, 0, 0, 0},
      {"force rowgroup", RG, 4, N, N, Z, 5, 1.0, nullptr, false, false, false, false, false, ROWGROUP, 8, 4, 0},
      {"force rowgroup + adaptive", RG | AD, 4, N, N, Z, 5, 1.0, nullptr, false, false, false, false, false, ADAPTIVE, 0, 0, 0},
      // ROWGROUP's shape from the mean row length
      {"rowgroup mean 4", RG, 4, N, N, 4 * N, 5, 1.0, nullptr, false, false, false, false, false, ROWGROUP, 4, 1, 0},
      {"rowgroup mean 4.5", RG, 4, N, N, 9 * N / 2, 5, 1.0, nullptr, false, false, false, false, false, ROWGROUP, 8, 4, 0},
      {"rowgroup mean 16", RG, 4, N, N, 16 * N, 20, 1.0, nullptr, false, false, false, false, false, ROWGROUP, 16, 4, 0},
      {"rowgroup mean 16.5", RG, 4, N, N, 33 * N / 2, 20, 1.0, nullptr, false, false, false, false, false, ROWGROUP, 32, 2, 0},
      {"rowgroup mean 32.5", RG, 4, N, N, 65 * N / 2, 40, 1.0, nullptr, false, false, false, false, false, ROWGROUP, 64, 1, 0},
      // ... or from the options, when lhpc_spmv_csr.hip instantiates the pair
      {"rowgroup 16 x 8", RG, 4, N, N, Z, 5, 1.0, [](lhpc_options &o) { o.rowgroup_lanes = 16, o.rowgroup_rows = 8; },
       false, false, false, false, false, ROWGROUP, 16, 8, 0},
      {"rowgroup 8 x 8", RG, 4, N, N, Z, 5, 1.0, [](lhpc_options &o) { o.rowgroup_lanes = 8, o.rowgroup_rows = 8; },
       false, false, false, false, false, ROWGROUP, 0, 0, LHPC_ERR_INVALID_ARG},
      {"rowgroup 8 x 0", RG, 4, N, N, Z, 5, 1.0, [](lhpc_options &o) { o.rowgroup_lanes = 8; },
       false, false, false, false, false, ROWGROUP, 0, 0, LHPC_ERR_INVALID_ARG},
      // the shape error waits for the CSR stage: XTILE is tried first
      {"force xtile + rowgroup 8 x 8", XT | RG, 4, N, N, Z, 5, 1.0,
       [](lhpc_options &o) { o.rowgroup_lanes = 8, o.rowgroup_rows = 8; },
       false, true, false, false, false, ROWGROUP, 0, 0, LHPC_ERR_INVALID_ARG},
  };
  for (const Case &c : cases) {
    lhpc_options o{};  // as lhpc_options_init: every choice automatic
    o.struct_size = sizeof(o);
    if (c.set) c.set(o);
    lhpc::SpmvShape s;
    s.n_rows = c.n_rows;
    s.n_cols = c.n_cols;
    s.nnz = c.nnz;
    s.elem_bytes = c.elem_bytes;
    s.max_row_len = c.max_row_len;
    s.lines_per_nnz = c.lines_per_nnz;
    const bool wants = lhpc::spmv_wants_locality(c.n_cols, c.elem_bytes, c.flags);
    const lhpc::SpmvFamilyPolicy p = lhpc::spmv_family_policy(s, c.flags, o);
    const bool ok = wants == c.wants && p.try_xtile == c.xtile && p.try_xslice == c.xslice && p.try_sell == c.sell &&
                    p.force_sell == c.force_sell && p.csr_kernel == c.kernel && p.csr_status == c.csr_status &&
                    (c.L == 0 || (p.L == c.L && p.R == c.R));
    if (!ok)
      std::fprintf(stderr, "spmv_family_policy %s: wants %d xtile %d xslice %d sell %d force_sell %d kernel %d L %d R %d status %d\n",
                   c.name, wants, p.try_xtile, p.try_xslice, p.try_sell, p.force_sell, p.csr_kernel, p.L, p.R,
                   p.csr_status);
    CHECK(ok);
  }
  // the XTILE stage builds what xtile_partition_policy says (user splits: one plan)
  lhpc_options o{};
  o.struct_size = sizeof(o);
  o.xtile_part_nnz = 200000;
  lhpc::SpmvShape s;
  s.n_rows = N, s.n_cols = 3000000, s.nnz = Z, s.max_row_len = 5;
  CHECK(lhpc::spmv_family_policy(s, 0, o).part.parts && lhpc::spmv_family_policy(s, 0, o).part.cap == 200000);
  s.n_splits = 2;
  CHECK(!lhpc::spmv_family_policy(s, 0, o).part.parts);
}

void check_bad_csr() {
  // every builder pass indexes host arrays by col / row_ptr, so validation
  // must reject these before any of them runs (lhpc_spmv_plan_create)
  const int64_t rp[] = {0, 2, 3};
  const int32_t good[] = {0, 4, 2}, big[] = {0, 5, 2}, neg[] = {0, -1, 2};
  CHECK(lhpc::validate_csr(rp, 64, good, 2, 5, 3) == 0);
  CHECK(lhpc::validate_csr(rp, 64, big, 2, 5, 3) == LHPC_ERR_BAD_CSR);
  CHECK(lhpc::validate_csr(rp, 64, neg, 2, 5, 3) == LHPC_ERR_BAD_CSR);
  const int64_t down[] = {0, 3, 2};
  CHECK(lhpc::validate_csr(down, 64, good, 2, 5, 2) == LHPC_ERR_BAD_CSR);
  const int32_t rp32[] = {1, 2, 3};
  CHECK(lhpc::validate_csr(rp32, 32, good, 2, 5, 3) == LHPC_ERR_BAD_CSR);  // row_ptr[0] != 0
  CHECK(lhpc::validate_csr(rp, 64, good, 2, 5, 4) == LHPC_ERR_BAD_CSR);     // row_ptr[n] != nnz
}

void check_io(const Csr &a) {
  char tmpl[] = "/tmp/lhpc_asan_XXXXXX";
  const int fd = mkstemp(tmpl);
  CHECK(fd >= 0);
  close(fd);
  const int64_t nnz = a.rp[a.n];
  CHECK(lhpc_csr_save(tmpl, LHPC_F32, a.n, a.m, nnz, a.rp.data(), 64, a.col.data(), a.val.data()) == 0);
  int dt = -1, bits = 0;
  int64_t n = 0, m = 0, z = 0;
  CHECK(lhpc_csr_load_header(tmpl, &dt, &n, &m, &z, &bits) == 0);
  CHECK(dt == LHPC_F32 && n == a.n && m == a.m && z == nnz && bits == 64);
  std::vector<int64_t> rp(static_cast<size_t>(n + 1));
  std::vector<int32_t> col(static_cast<size_t>(z));
  std::vector<float> val(static_cast<size_t>(z));
  CHECK(lhpc_csr_load(tmpl, rp.data(), col.data(), val.data()) == 0);
  CHECK(rp == a.rp && col == a.col && val == a.val);
  // truncated file: the loader must refuse, not read past the mapping
  CHECK(truncate(tmpl, 100) == 0);
  CHECK(lhpc_csr_load_header(tmpl, &dt, &n, &m, &z, &bits) != 0 || lhpc_csr_load(tmpl, rp.data(), col.data(), val.data()) != 0);
  std::remove(tmpl);
  // Matrix Market: symmetric expansion, comments, a bad entry
  const std::string mtx = std::string(tmpl) + ".mtx";
  FILE *f = std::fopen(mtx.c_str(), "w");
  std::fprintf(f, "%%%%MatrixMarket matrix coordinate real symmetric\n%% c\n3 3 3\n1 1 2.0\n2 1 -1.5\n3 3 4e0\n");
  std::fclose(f);
  int64_t zmax = 0, cnt = 0;
  int sym = -1, fld = -1;
  CHECK(lhpc_mm_read_header(mtx.c_str(), &n, &m, &zmax, &sym, &fld) == 0 && zmax == 6);
  std::vector<int32_t> r(static_cast<size_t>(zmax)), c(static_cast<size_t>(zmax));
  std::vector<double> v(static_cast<size_t>(zmax));
  CHECK(lhpc_mm_read_coo(mtx.c_str(), r.data(), c.data(), v.data(), &cnt) == 0 && cnt == 4);
  f = std::fopen(mtx.c_str(), "w");
  std::fprintf(f, "%%%%MatrixMarket matrix coordinate real general\n3 3 2\n1 1 1.0\n4 1 1.0\n");
  std::fclose(f);
  CHECK(lhpc_mm_read_header(mtx.c_str(), &n, &m, &zmax, &sym, &fld) == 0);
  CHECK(lhpc_mm_read_coo(mtx.c_str(), r.data(), c.data(), v.data(), &cnt) != 0);  // row 4 of 3
  std::remove(mtx.c_str());
}

}  // namespace

int main() {
  check_bad_csr();
  check_xtile_policy();
  check_spmv_family_policy();
  const Csr u = uniform(20000, 30000, 15, 0x5EED0001);
  const Csr p = powerlaw(20000, 20000, 3000, 0x5EED0004);
  const Csr e = uniform(777, 100, 0, 7);  // all rows empty
  for (bool ip : {false, true}) {
    check_xtile(u, ip, {});
    check_xtile(p, ip, {});
    check_xtile(p, ip, {1, 5000, 19999});
    check_xtile(u, ip, {5000, 10000, 15000});
    check_xtile(p, ip, {}, 32);
    check_xtile(p, ip, {77}, 1024);
    check_xtile(e, ip, {});
  }
  for (int unit : {2, 4}) {  // aligned segments (iperm only)
    check_xtile(u, true, {}, 512, unit);
    check_xtile(p, true, {1, 5000, 19999}, 512, unit);
    check_xtile(p, true, {}, 32, unit);
    check_xtile(e, true, {}, 512, unit);
  }
  for (int S : {1, 8, 64}) {
    lhpc::XsliceHost xs;
    const int rc = lhpc::build_xslice(p.rp.data(), 64, p.col.data(), p.val.data(), 4, p.n, p.m, S, xs);
    CHECK(rc == 0 || rc == LHPC_ERR_UNSUPPORTED);
    if (rc == 0) CHECK(xs.nnz == p.rp[p.n]);
  }
  int64_t cuts[9];
  CHECK(lhpc_csr_partition_rows(p.rp.data(), 64, p.n, 8, cuts) == 0);
  for (int k = 0; k < 8; ++k) CHECK(cuts[k] <= cuts[k + 1]);
  check_io(u);
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ALL OK (asan plan/io)\n");
  return 0;
}
