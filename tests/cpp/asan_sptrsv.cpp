// asan_sptrsv.cpp — the host analysis of the triangular solve
// (libhpc_amd/csrc/lhpc_sptrsv_host.cpp: validation, levels, sliced layout,
// schedule) compiled with -fsanitize=address,undefined into this stand-alone
// CPU program (tests/cpp/sptrsv.mk `asan`, run by tests/test_sptrsv_asan.py).
// It walks the test matrices of tests/test_sptrsv_api.py — natural and
// red–black grids, a dense triangle, grid/chain/grid blocks (both), diagonal only,
// unsorted rows with a duplicate and both triangles, n = 1, n = 0 — lower and
// (transposed) upper, unit and non-unit, 32- and 64-bit row_ptr, several
// chain_rows, checks the layout against the CSR it came from, and feeds the
// invalid inputs that must come back as LHPC_ERR_BAD_CSR before any array is
// indexed by them.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../libhpc_amd/csrc/lhpc_sptrsv.hpp"

namespace {

struct Csr {
  int64_t n = 0;
  std::vector<int64_t> rp{0};
  std::vector<int32_t> col;
};

using Coo = std::vector<std::pair<int32_t, int32_t>>;

// rows in the order given (stable), so a shuffled list gives unsorted rows
Csr from_coo(int64_t n, const Coo &e, bool transpose) {
  Csr a;
  a.n = n;
  a.rp.assign(static_cast<size_t>(n) + 1, 0);
  for (auto [r, c] : e) ++a.rp[static_cast<size_t>(transpose ? c : r) + 1];
  std::partial_sum(a.rp.begin(), a.rp.end(), a.rp.begin());
  std::vector<int64_t> at(a.rp.begin(), a.rp.end() - 1);
  a.col.resize(e.size());
  for (auto [r, c] : e) a.col[static_cast<size_t>(at[static_cast<size_t>(transpose ? c : r)]++)] = transpose ? r : c;
  return a;
}

Coo grid(int nx, int ny, bool red_black) {
  std::vector<int32_t> index(static_cast<size_t>(nx) * ny);
  if (red_black) {
    int32_t k = 0;
    for (int parity = 0; parity < 2; ++parity)
      for (int i = 0; i < nx * ny; ++i)
        if ((i % nx + i / nx) % 2 == parity) index[static_cast<size_t>(i)] = k++;
  } else {
    std::iota(index.begin(), index.end(), 0);
  }
  Coo e;
  for (int iy = 0; iy < ny; ++iy)
    for (int ix = 0; ix < nx; ++ix) {
      const int i = iy * nx + ix;
      auto put = [&](bool in, int j) {
        if (in) e.emplace_back(index[static_cast<size_t>(i)], index[static_cast<size_t>(j)]);
      };
      put(iy > 0, i - nx);
      put(ix > 0, i - 1);
      put(true, i);
      put(ix < nx - 1, i + 1);
      put(iy < ny - 1, i + nx);
    }
  return e;
}

int failures = 0;
void expect(bool ok, const std::string &what) {
  if (!ok) {
    std::fprintf(stderr, "FAIL: %s\n", what.c_str());
    ++failures;
  }
}

// the analysis of one matrix, checked against the CSR
void check(const std::string &name, const Csr &a, unsigned trsv, int chain_rows, int bits) {
  const bool upper = trsv & LHPC_TRSV_UPPER, unit = trsv & LHPC_TRSV_UNIT_DIAG;
  const std::string tag = name + " trsv " + std::to_string(trsv) + " chain " + std::to_string(chain_rows) + " bits " +
                          std::to_string(bits);
  const std::vector<int32_t> rp32(a.rp.begin(), a.rp.end());
  const void *rp = bits == 64 ? static_cast<const void *>(a.rp.data()) : static_cast<const void *>(rp32.data());
  const int64_t nnz = static_cast<int64_t>(a.col.size());
  std::vector<int32_t> level(static_cast<size_t>(a.n));
  int64_t n_levels = -1;
  int st = lhpc_sptrsv_levels(a.n, nnz, rp, bits, a.col.data(), trsv, level.data(), &n_levels);
  expect(st == LHPC_OK, tag + ": levels status " + std::to_string(st));
  if (st != LHPC_OK) return;
  // the rule itself
  int64_t top = 0;
  for (int64_t k = 0; k < a.n; ++k) {
    const int64_t i = upper ? a.n - 1 - k : k;
    int32_t lv = 0;
    for (int64_t p = a.rp[i]; p < a.rp[i + 1]; ++p)
      if (upper ? a.col[p] > i : a.col[p] < i) lv = std::max(lv, level[a.col[p]] + 1);
    expect(level[i] == lv, tag + ": level of row " + std::to_string(i));
    top = std::max<int64_t>(top, lv + 1);
  }
  expect(n_levels == top, tag + ": n_levels");

  lhpc::TrsvLayout o;
  st = lhpc::sptrsv_layout_host(o, a.n, nnz, rp, bits, a.col.data(), trsv, chain_rows);
  expect(st == LHPC_OK, tag + ": layout status " + std::to_string(st));
  if (st != LHPC_OK) return;
  expect(o.n_levels == n_levels && static_cast<int64_t>(o.level_slice.size()) == n_levels + 1, tag + ": level table");
  expect(static_cast<int64_t>(o.slice_off.size()) == o.n_slices + 1 && o.slice_off[o.n_slices] == o.padded &&
             static_cast<int64_t>(o.col.size()) == o.padded &&
             static_cast<int64_t>(o.slice_row.size()) == o.n_slices * 64 &&
             static_cast<int64_t>(o.src.size()) == o.padded + (unit ? 0 : o.n_slices * 64),
         tag + ": array sizes");
  std::vector<int> seen(static_cast<size_t>(a.n), 0);
  int64_t kept = 0, max_rows = 0;
  for (int64_t l = 0; l < o.n_levels; ++l) {
    int64_t rows = 0, prev = -1;
    for (int64_t s = o.level_slice[l]; s < o.level_slice[l + 1]; ++s) {
      const int64_t off = o.slice_off[s], w = (o.slice_off[s + 1] - off) / 64;
      int64_t longest = 0;
      for (int lane = 0; lane < 64; ++lane) {
        const int32_t row = o.slice_row[s * 64 + lane];
        if (row < 0) {
          for (int64_t e = 0; e < w; ++e) expect(o.col[off + e * 64 + lane] == -1, tag + ": idle lane holds an entry");
          if (!unit) expect(o.src[o.padded + s * 64 + lane] == lhpc::kTrsvNoSource, tag + ": idle lane has a diagonal");
          continue;
        }
        expect(row < a.n && level[row] == l && row > prev, tag + ": row order inside a level");
        prev = row;
        ++rows;
        ++seen[row];
        // the row's kept entries in CSR order, then padding
        int64_t e = 0;
        for (int64_t p = a.rp[row]; p < a.rp[row + 1]; ++p) {
          if (a.col[p] == row) {
            if (!unit) expect(o.src[o.padded + s * 64 + lane] == static_cast<uint32_t>(p), tag + ": diagonal source");
          } else if (upper ? a.col[p] > row : a.col[p] < row) {
            const int64_t q = off + e * 64 + lane;
            expect(e < w && o.col[q] == a.col[p] && o.src[q] == static_cast<uint32_t>(p), tag + ": entry order");
            ++e;
          }
        }
        kept += e;
        longest = std::max(longest, e);
        for (; e < w; ++e)
          expect(o.col[off + e * 64 + lane] == -1 && o.src[off + e * 64 + lane] == lhpc::kTrsvNoSource,
                 tag + ": padding");
      }
      expect(longest == w, tag + ": slice wider than its longest row");
    }
    max_rows = std::max(max_rows, rows);
  }
  expect(std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }), tag + ": every row exactly once");
  expect(kept == o.kept && max_rows == o.max_level_rows, tag + ": kept / max_level_rows");
  // the schedule covers the levels in order; chain steps are maximal runs
  int64_t l = 0;
  for (const lhpc::TrsvStep &s : o.steps) {
    expect(s.level_begin == l && s.level_end > l && s.slice_begin == o.level_slice[s.level_begin] &&
               s.slice_end == o.level_slice[s.level_end] && (s.chain || s.level_end == l + 1),
           tag + ": step bounds");
    l = s.level_end;
  }
  expect(l == o.n_levels, tag + ": steps do not end at the last level");
  if (chain_rows < 0) expect(static_cast<int64_t>(o.steps.size()) == o.n_levels, tag + ": never chain");
  if (chain_rows > 0 && o.max_level_rows <= chain_rows && o.n_levels > 0)
    expect(o.steps.size() == 1 && o.steps[0].chain, tag + ": one chain step");
  expect(o.chain_rows == (chain_rows == 0 ? lhpc::kTrsvChainRowsAuto : chain_rows < 0 ? -1 : chain_rows),
         tag + ": threshold in force");
}

int levels_status(std::vector<int64_t> rp, std::vector<int32_t> col, unsigned trsv, int bits) {
  const std::vector<int32_t> rp32(rp.begin(), rp.end());
  const int64_t n = static_cast<int64_t>(rp.size()) - 1;
  std::vector<int32_t> level(static_cast<size_t>(std::max<int64_t>(n, 1)));
  int64_t nl = 0;
  lhpc::TrsvLayout o;
  const void *p = bits == 64 ? static_cast<const void *>(rp.data()) : static_cast<const void *>(rp32.data());
  const int a = lhpc_sptrsv_levels(n, static_cast<int64_t>(col.size()), p, bits, col.data(), trsv, level.data(), &nl);
  const int b = lhpc::sptrsv_layout_host(o, n, static_cast<int64_t>(col.size()), p, bits, col.data(), trsv, 0);
  expect(a == b, "levels and layout disagree on a status");
  return a;
}

}  // namespace

int main() {
  std::vector<std::pair<std::string, std::pair<int64_t, Coo>>> mats;
  mats.push_back({"grid_nat", {37 * 29, grid(37, 29, false)}});
  mats.push_back({"grid_rb", {64 * 33, grid(64, 33, true)}});
  {
    Coo e;
    for (int32_t r = 0; r < 130; ++r)
      for (int32_t c = 0; c <= r; ++c) e.emplace_back(r, c);
    mats.push_back({"dense130", {130, e}});
  }
  // mixed: the five middle rows depend on the block before (row i − 5: one
  // level, 3 in all); mixed_chain: on the row just before (7 levels)
  for (int back : {5, 1}) {
    std::mt19937 rng(0x7A5);
    Coo e;
    for (int32_t i = 0; i < 3005; ++i) {
      e.emplace_back(i, i);
      if (i >= 1500 && i < 1505) e.emplace_back(i, i - back);
      if (i >= 1505) {
        for (int k = 0; k < 3; ++k) e.emplace_back(i, static_cast<int32_t>(rng() % 1500));  // duplicates may occur
        e.emplace_back(i, 1504);
      }
    }
    mats.push_back({back == 5 ? "mixed" : "mixed_chain", {3005, e}});
  }
  {
    Coo e;
    for (int32_t i = 0; i < 200; ++i) e.emplace_back(i, i);
    mats.push_back({"diag", {200, e}});
  }
  {
    Coo e = grid(37, 29, false);
    e.emplace_back(500, 499);
    std::shuffle(e.begin(), e.end(), std::mt19937(0x51));
    mats.push_back({"unsorted", {37 * 29, e}});
  }
  mats.push_back({"one", {1, Coo{{0, 0}}}});
  mats.push_back({"empty", {0, Coo{}}});

  for (const auto &m : mats)
    for (int transpose = 0; transpose < 2; ++transpose) {
      const Csr a = from_coo(m.second.first, m.second.second, transpose != 0);
      for (unsigned unit : {0u, 2u})
        for (int chain : {-1, 0, 1, 64, 2048})
          for (int bits : {32, 64}) check(m.first, a, (transpose ? 1u : 0u) | unit, chain, bits);
      // a matrix with both triangles serves the other solve too
      if (m.first.rfind("grid", 0) == 0 || m.first == "unsorted") check(m.first, a, transpose ? 0u : 1u, 64, 32);
    }
  for (int m : {3, 4}) {
    // the counts tests/test_gpu_sptrsv.py asks the plan for: mixed 3 / 3 / 1, mixed_chain 3 / 7 / 1
    const Csr a = from_coo(mats[m].second.first, mats[m].second.second, false);
    const std::vector<int32_t> rp32(a.rp.begin(), a.rp.end());
    const size_t levels = m == 3 ? 3 : 7;
    for (auto [chain, want] : {std::pair<int, size_t>{64, 3}, {-1, levels}, {2048, 1}}) {
      lhpc::TrsvLayout o;
      const int st = lhpc::sptrsv_layout_host(o, a.n, static_cast<int64_t>(a.col.size()), rp32.data(), 32,
                                              a.col.data(), 0, chain);
      expect(st == LHPC_OK && static_cast<size_t>(o.n_levels) == levels && o.steps.size() == want,
             mats[m].first + ": " + std::to_string(o.steps.size()) + " steps at chain_rows " + std::to_string(chain));
    }
  }

  for (int bits : {32, 64}) {
    expect(levels_status({0, 1, 3}, {0, 0, 1}, 0, bits) == LHPC_OK, "a valid 2 × 2");
    expect(levels_status({0, 1, 3}, {0, 0, 0}, 0, bits) == LHPC_ERR_BAD_CSR, "missing diagonal");
    expect(levels_status({0, 1, 3}, {0, 0, 0}, 2, bits) == LHPC_OK, "missing diagonal, unit");
    expect(levels_status({0, 1, 3}, {0, 1, 1}, 0, bits) == LHPC_ERR_BAD_CSR, "doubled diagonal");
    expect(levels_status({0, 1, 3}, {0, 0, 2}, 0, bits) == LHPC_ERR_BAD_CSR, "column = n");
    expect(levels_status({0, 1, 3}, {0, -1, 1}, 0, bits) == LHPC_ERR_BAD_CSR, "negative column");
    expect(levels_status({0, 1, 3}, {0, 0, INT32_MAX}, 3, bits) == LHPC_ERR_BAD_CSR, "huge column in the ignored triangle");
    expect(levels_status({0, 1, 3}, {INT32_MIN, 0, 1}, 2, bits) == LHPC_ERR_BAD_CSR, "INT32_MIN column");
    expect(levels_status({0, 3, 1, 3}, {0, 1, 2}, 0, bits) == LHPC_ERR_BAD_CSR, "decreasing row_ptr");
    expect(levels_status({1, 1, 3}, {0, 0, 1}, 0, bits) == LHPC_ERR_BAD_CSR, "row_ptr[0] != 0");
    expect(levels_status({0, 1, 2}, {0, 0, 1}, 0, bits) == LHPC_ERR_BAD_CSR, "row_ptr[n] != nnz");
    expect(levels_status({0, 1, 7}, {0, 0, 1}, 0, bits) == LHPC_ERR_BAD_CSR, "row_ptr[n] past the arrays");
    expect(levels_status({0, -1, 3}, {0, 0, 1}, 0, bits) == LHPC_ERR_BAD_CSR, "negative row_ptr");
  }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("ALL OK (asan sptrsv)\n");
  return 0;
}
