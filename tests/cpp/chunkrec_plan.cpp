// chunkrec_plan.cpp — host-only driver for the XTILE chunk records
// (lhpc_plan.cpp xtile_chunk_records, options.xtile_chunkrec), built with
// -fsanitize=address,undefined by tests/cpp/chunkrec.mk and run by
// tests/test_chunkrec_plan.py (no HIP, no GPU).
//   - the record builder against a brute-force construction that walks the
//     reduce kernel's own steps in plain loops: the segment scan over the
//     device segment table (lo | len << 16 words plus hi rows, per range in
//     ring plans) with its bit per non-empty segment, the row decode from
//     row_ptr with its bit per owned row start below m, and the row-runs-on
//     test of the last owned row;
//   - xtile_policy's gating of the records at the full-size C2 / C4 shapes
//     and at the shapes of the pinned small plans.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/lhpc.h"
#include "../../libhpc_amd/csrc/lhpc_plan.hpp"

static int failures = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

namespace {

struct Csr {
  int64_t n = 0, m = 0;
  std::vector<int64_t> rp;
  std::vector<int32_t> col;
};

Csr from_lengths(const std::vector<int64_t> &len, int64_t n_cols, uint64_t seed) {
  Csr a;
  a.n = static_cast<int64_t>(len.size());
  a.m = n_cols;
  a.rp.assign(1, 0);
  for (int64_t l : len) a.rp.push_back(a.rp.back() + l);
  std::mt19937_64 g(seed);
  a.col.resize(static_cast<size_t>(a.rp.back()));
  for (int64_t r = 0; r < a.n; ++r) {
    for (int64_t k = a.rp[r]; k < a.rp[r + 1]; ++k) a.col[static_cast<size_t>(k)] = static_cast<int32_t>(g() % n_cols);
    std::sort(a.col.begin() + a.rp[r], a.col.begin() + a.rp[r + 1]);
  }
  return a;
}

struct Want {  // what a case must contain, so that the shapes asked for are really there
  bool full_chunk = false, last_chunk_1 = false, row_past_M = false;
};

// The record of every chunk against the kernel's steps.  ring: the plan's
// ranges (its splits + 1) share an xg ring (xtile_ring_pieces).
void check_records(const char *name, const Csr &a, int64_t W, int M, int S_want, const std::vector<int64_t> &splits,
                   bool ring, const Want &want) {
  lhpc::XtileHost xt;
  const int rc = lhpc::build_xtile(a.rp.data(), 64, a.col.data(), a.n, a.m, W, M, M / 8, 3000, 4,
                                   splits.empty() ? nullptr : splits.data(), static_cast<int>(splits.size()), true,
                                   M / 32, xt, 1);
  CHECK(rc == 0);
  if (rc) return;
  if (ring) {
    std::vector<int64_t> rpc;
    lhpc::xtile_ring_pieces(xt, 700, rpc);
    CHECK(!xt.rdelta.empty() && xt.hrow.size() == splits.size() + 1);
  }
  const int64_t C = xt.n_chunks, S = xt.S, BW = M / 32, RW = lhpc::xtile_chunkrec_words(M, xt.S);
  CHECK(S == S_want && RW % 4 == 0 && RW >= 2 * BW + S + 1);
  std::vector<uint32_t> seg, rec;
  std::vector<int32_t> hi;
  lhpc::xtile_segment_table(xt, seg, hi);
  lhpc::xtile_chunk_records(xt, a.rp.data(), 64, rec);
  CHECK(static_cast<int64_t>(rec.size()) == std::max<int64_t>(C, 1) * RW);
  const int64_t K = static_cast<int64_t>(xt.rchunk.size()) - 1;
  bool full = false, last1 = false;
  int64_t bad = 0;
  for (int64_t c = 0; c < C; ++c) {
    int64_t k = 0;
    while (k + 1 < K && xt.rchunk[k + 1] <= c) ++k;
    // the launch's hi-row arguments: per range in ring plans, else the whole stream's
    const int64_t hc0 = ring ? xt.rchunk[k] : 0, hrow0 = ring ? xt.hrow[static_cast<size_t>(k)] : 0;
    const int64_t e0 = xt.ce[c], m = xt.ce[c + 1] - e0, r0 = xt.cr[c], R = xt.cr[c + 1] - r0;
    full |= m == M;
    last1 |= c == C - 1 && m == 1;
    std::vector<uint32_t> w(static_cast<size_t>(RW), 0u);
    uint32_t *bm = w.data(), *sbm = bm + BW;  // the record's order: bm, sbm, base_ne, flags
    int32_t *bne = reinterpret_cast<int32_t *>(sbm + BW);
    // scan: thread sI holds segment sI's start and end, the prefix over the
    // threads gives its flat offset and its rank among the non-empty ones
    int64_t off = 0, rank = 0;
    for (int64_t sI = 0; sI < S; ++sI) {
      const uint32_t sw = seg[static_cast<size_t>(c * S + sI)];
      const int64_t sa = hi[static_cast<size_t>((hrow0 + (c - hc0) / lhpc::kXtSegHi) * S + sI)] + (sw & 0xFFFFu);
      const int64_t len = sw >> 16;
      if (len > 0) {
        bne[rank++] = static_cast<int32_t>(sa - off);
        sbm[off >> 5] |= 1u << (off & 31);  // atomicOr
      }
      off += len;
    }
    CHECK(off == m);
    for (int64_t r = rank; r < S; ++r) bne[r] = rank > 0 ? bne[rank - 1] : 0;  // the builder's padding rule
    // row decode: thread j loads row_ptr[r0 + min(j, R)]
    for (int64_t j = 0; j < R; ++j) {
      const int64_t rv = a.rp[static_cast<size_t>(r0 + j)] - e0;
      CHECK(rv >= 0);
      if (rv < m) bm[rv >> 5] |= 1u << (rv & 31);  // atomicOr
    }
    const int64_t rvR = a.rp[static_cast<size_t>(r0 + R)] - e0;
    bne[S] = (rvR <= m ? rvR : m + 1) > m ? 1 : 0;  // rpl[R] > m
    for (int64_t i = 0; i < RW; ++i) bad += rec[static_cast<size_t>(c * RW + i)] != w[static_cast<size_t>(i)];
    // a plan without empty rows: as many row-start bits as owned rows
    if (!lhpc::csr_has_empty_row(a.rp.data(), 64, a.n)) {
      int64_t bits = 0;
      for (int64_t i = 0; i < BW; ++i) bits += __builtin_popcount(bm[i]);
      CHECK(bits == R);
    }
  }
  if (bad) std::fprintf(stderr, "%s: %lld record words differ\n", name, static_cast<long long>(bad));
  CHECK(bad == 0);
  if (want.full_chunk) CHECK(full);
  if (want.last_chunk_1) CHECK(last1);
  if (want.row_past_M) {
    bool seen = false;
    for (int64_t c = 0; c + 2 < C && !seen; ++c) seen = xt.cr[c + 1] == xt.cr[c + 2] && xt.cr[c] < xt.cr[c + 1];
    CHECK(seen);  // a chunk that owns no row start: it lies inside one row
  }
  std::printf("records %-28s S %4lld chunks %5lld ranges %lld%s ok\n", name, static_cast<long long>(S),
              static_cast<long long>(C), static_cast<long long>(K), ring ? " (ring)" : "");
}

std::vector<int64_t> rep(int64_t n, int64_t l) { return std::vector<int64_t>(static_cast<size_t>(n), l); }
std::vector<int64_t> cat(std::initializer_list<std::vector<int64_t>> parts) {
  std::vector<int64_t> o;
  for (const auto &p : parts) o.insert(o.end(), p.begin(), p.end());
  return o;
}

void check_all_records() {
  const int M = 1024;
  const int64_t W = 4096;
  for (const int S : {3, 256}) {
    const int64_t n_cols = W * S - 7;
    // m = M with a row end on the chunk end (no row start in the window's
    // back M/32), a row crossing two chunk ends, rows of 15, 3 and 1
    const auto len = cat({{900, M - 900}, rep(300, 15), {2 * M + 5}, rep(200, 3), {M - 1, 1}, rep(500, 15), {M, 1}});
    const Csr a = from_lengths(len, n_cols, 0xA0 + S);
    Want w;
    w.full_chunk = w.row_past_M = true;
    check_records("one range", a, W, M, S, {}, false, w);
    // a full chunk whose row ends on its end, then a last chunk of one nonzero
    w.row_past_M = false;
    w.last_chunk_1 = true;
    check_records("full chunk, then 1", from_lengths({M, 1}, n_cols, 0xB0 + S), W, M, S, {}, false, w);
    const int64_t n = a.n;
    check_records("3 ranges", a, W, M, S, {n / 3, 2 * n / 3}, false, Want{});
    check_records("3 ring ranges", a, W, M, S, {n / 3, 2 * n / 3}, true, Want{});
    // an empty row: the records still hold what the kernel would compute,
    // and the policy answers "off" (check_policy)
    const Csr e = from_lengths(cat({rep(100, 15), {0}, rep(100, 15), {0, 0, 3000, 0}}), n_cols, 0xE0 + S);
    CHECK(lhpc::csr_has_empty_row(e.rp.data(), 64, e.n));
    CHECK(!lhpc::csr_has_empty_row(a.rp.data(), 64, a.n));
    check_records("empty rows", e, W, M, S, {}, false, Want{});
  }
  // the fp32 reduce's own sizes: M = 8192, 40960-column tiles
  {
    const Csr a = from_lengths(cat({{7000, 1192}, rep(3000, 15), {20000}, {8192, 1}}), 40960 * 3 - 7, 0xA9);
    Want w;
    w.full_chunk = w.row_past_M = true;
    check_records("M 8192", a, 40960, 8192, 3, {}, false, w);
    w.row_past_M = false;
    w.last_chunk_1 = true;
    check_records("M 8192: full chunk, then 1", from_lengths({8192, 1}, 40960 * 3 - 7, 0xAB), 40960, 8192, 3, {}, false, w);
  }
  // a single nonzero
  check_records("nnz 1", from_lengths({1}, 4096 * 3 - 7, 0xAA), 4096, M, 3, {}, false, Want{});
}

// xtile_policy: where the records are chosen.  Option 0 chooses them for
// fp32 G = 1 iperm plans that take cache-sized ranges by themselves (C2, C4).

lhpc::XtilePolicy policy(int64_t n_rows, int64_t n_cols, int64_t nnz, int tsz, int G, int n_user_splits,
                         bool empty_rows, bool y_add, const lhpc_options &o) {
  lhpc::XtileShape s;
  s.n_rows = n_rows;
  s.n_cols = n_cols;
  s.nnz = nnz;
  s.elem_bytes = tsz;
  s.M = 8192;  // both types: 64-B runs, 512 / 1024 threads
  s.cus = 256;
  s.n_user_splits = n_user_splits;
  s.dev_build = true;
  s.W = lhpc::xtile_tile_width(n_cols, static_cast<size_t>(tsz), 256);
  s.G = G;
  s.empty_rows = empty_rows;
  s.y_add = y_add;
  return lhpc::xtile_policy(s, o);
}

void check_policy() {
  constexpr int64_t N = 10000000, C2Z = 150000000, C4Z = 150335590;
  auto opts = [](int rec) {
    lhpc_options o{};
    o.struct_size = sizeof(o);
    o.xtile_chunkrec = rec;
    return o;
  };
  for (const int64_t nnz : {C2Z, C4Z}) {
    CHECK(policy(N, N, nnz, 4, 1, 0, false, false, opts(0)).rec);
    CHECK(policy(N, N, nnz, 4, 1, 0, false, false, opts(0)).own_cuts);
    CHECK(!policy(N, N, nnz, 4, 1, 0, true, false, opts(0)).rec);   // an empty row
    CHECK(!policy(N, N, nnz, 4, 1, 3, false, false, opts(0)).rec);  // user row splits (the per-rank plans)
    CHECK(policy(N, N, nnz, 4, 1, 3, false, false, opts(2)).rec);
    {
      lhpc_options o = opts(0);
      o.xtile_ranges = 3;  // ranges by option, not by themselves
      CHECK(!policy(N, N, nnz, 4, 1, 0, false, false, o).rec);
      o.xtile_ranges = 1;
      CHECK(!policy(N, N, nnz, 4, 1, 0, false, false, o).rec);
    }
    // xg inside the Infinity Cache: no ranges, no records
    CHECK(!policy(1000000, 1000000, (int64_t{256} << 20) / 4, 4, 1, 0, false, false, opts(0)).rec);
    CHECK(policy(1000000, 1000000, (int64_t{256} << 20) / 4 + 1, 4, 1, 0, false, false, opts(0)).rec);
    CHECK(policy(N, N, nnz, 4, 1, 0, false, false, opts(2)).rec);
    CHECK(!policy(N, N, nnz, 4, 1, 0, false, false, opts(1)).rec);
    CHECK(!policy(N, N, nnz, 4, 1, 0, true, false, opts(2)).rec);   // an empty row
    CHECK(!policy(N, N, nnz, 4, 1, 0, false, true, opts(2)).rec);   // a column block that adds into y
    CHECK(!policy(N, N, nnz, 8, 1, 0, false, false, opts(2)).rec);  // fp64 (C3) keeps its phase-A tables
    CHECK(policy(N, N, nnz, 8, 1, 0, false, false, opts(2)).pre);
    CHECK(!policy(N, N, nnz, 4, 2, 0, false, false, opts(2)).rec);  // G = 2
    lhpc_options o = opts(2);
    o.xtile_pretable = 2;  // the two exclude each other: the tables asked for by option win
    CHECK(policy(N, N, nnz, 4, 1, 0, false, false, o).pre && !policy(N, N, nnz, 4, 1, 0, false, false, o).rec);
    o = opts(2);
    o.xtile_reduce = LHPC_XTILE_REDUCE_PERM;
    CHECK(!policy(N, N, nnz, 4, 1, 0, false, false, o).rec);
    o = opts(2);
    o.xtile_align = LHPC_XTILE_ALIGN_UNITS;
    CHECK(!policy(N, N, nnz, 4, 1, 0, false, false, o).rec);
    // the records change no other decision
    const lhpc::XtilePolicy p0 = policy(N, N, nnz, 4, 1, 0, false, false, opts(1));
    const lhpc::XtilePolicy p2 = policy(N, N, nnz, 4, 1, 0, false, false, opts(2));
    CHECK(p0.W == p2.W && p0.piece == p2.piece && p0.iperm == p2.iperm && p0.aligned == p2.aligned &&
          p0.cut == p2.cut && p0.ranges == p2.ranges && p0.own_cuts == p2.own_cuts && p0.pre == p2.pre &&
          p0.steps == p2.steps && p0.ring(3) == p2.ring(3) && p0.nt(3) == p2.nt(3));
  }
  // the pinned small plans (tests/golden/xtile_layout_pinned.json): 30060
  // rows, 0.52M nonzeros, fp32 3 / 256 / 500 / 600 tiles and fp64 3 / 256 /
  // 1100 — automatic options leave every one of them without records, with
  // and without empty rows, whatever else the case sets
  struct Pin {
    int tsz, tiles, G;
  };
  const Pin pins[] = {{4, 3, 1}, {4, 256, 1}, {4, 500, 2}, {4, 600, 2}, {8, 3, 1}, {8, 256, 1}, {8, 1100, 2}};
  void (*const sets[])(lhpc_options &) = {
      [](lhpc_options &) {},
      [](lhpc_options &o) { o.xtile_reduce = 2; o.xtile_ranges = 1; },
      [](lhpc_options &o) { o.xtile_ranges = 3; },
      [](lhpc_options &o) { o.xtile_ranges = 3; o.xtile_ring = 1; },
      [](lhpc_options &o) { o.xtile_ranges = 2; o.xtile_ring = 2; },
      [](lhpc_options &o) { o.xtile_store = LHPC_STORE_NT; },
      [](lhpc_options &o) { o.xtile_steps = 4; },
      [](lhpc_options &o) { o.xtile_cut = 64; },
      [](lhpc_options &o) { o.xtile_piece = 1000; },
      [](lhpc_options &o) { o.xtile_pretable = 2; },
  };
  for (const Pin &pn : pins)
    for (const auto set : sets)
      for (const int splits : {0, 5})
        for (const bool empty : {true, false}) {
          lhpc_options o = opts(0);
          set(o);
          const int64_t n_cols = static_cast<int64_t>(pn.tsz == 4 ? 40960 : 20480) * pn.tiles - 7;
          CHECK(!policy(30060, n_cols, 522247, pn.tsz, pn.G, splits, empty, false, o).rec);
        }
}

}  // namespace

int main() {
  check_all_records();
  check_policy();
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("ALL OK (chunk records)\n");
  return 0;
}
