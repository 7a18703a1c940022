// lhpc_sptrsv_host.cpp — host analysis of the level-scheduled triangular
// solve: validation, levels, the sliced layout and the launch schedule
// (lhpc_sptrsv.hpp).  One sequential O(nnz) pass each; no HIP dependency, so
// tests/cpp/asan_sptrsv.cpp builds this file alone under ASan/UBSan.
#include "lhpc_sptrsv.hpp"

#include <algorithm>

#include "lhpc_abi.hpp"

namespace lhpc {
namespace {

inline int64_t rp_at(const void *rp, int bits, int64_t i) {
  return bits == 64 ? static_cast<const int64_t *>(rp)[i] : static_cast<const int32_t *>(rp)[i];
}

// kept off-diagonal entry of row i?
inline bool kept(bool upper, int64_t i, int32_t c) { return upper ? c > i : c < i; }

}  // namespace

int sptrsv_levels_host(int64_t n, int64_t nnz, const void *row_ptr, int bits, const int32_t *col, unsigned trsv,
                       int32_t *level, int64_t *n_levels) {
  const bool upper = (trsv & LHPC_TRSV_UPPER) != 0, unit = (trsv & LHPC_TRSV_UNIT_DIAG) != 0;
  // row_ptr first: every position read below then lies inside [0, nnz)
  if (rp_at(row_ptr, bits, 0) != 0 || rp_at(row_ptr, bits, n) != nnz) return LHPC_ERR_BAD_CSR;
  for (int64_t i = 0; i < n; ++i)
    if (rp_at(row_ptr, bits, i) > rp_at(row_ptr, bits, i + 1)) return LHPC_ERR_BAD_CSR;
  for (int64_t p = 0; p < nnz; ++p)
    if (col[p] < 0 || col[p] >= n) return LHPC_ERR_BAD_CSR;
  int64_t top = 0;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t i = upper ? n - 1 - k : k;  // the rows this one may depend on come first
    const int64_t p0 = rp_at(row_ptr, bits, i), p1 = rp_at(row_ptr, bits, i + 1);
    int32_t lv = 0;
    int diag = 0;
    for (int64_t p = p0; p < p1; ++p) {
      const int32_t c = col[p];
      if (c == i) ++diag;
      else if (kept(upper, i, c)) lv = std::max(lv, level[c] + 1);
    }
    if (!unit && diag != 1) return LHPC_ERR_BAD_CSR;
    level[i] = lv;
    top = std::max<int64_t>(top, lv + 1);
  }
  *n_levels = top;
  return LHPC_OK;
}

int sptrsv_layout_host(TrsvLayout &o, int64_t n, int64_t nnz, const void *row_ptr, int bits, const int32_t *col,
                       unsigned trsv, int chain_rows) {
  const bool upper = (trsv & LHPC_TRSV_UPPER) != 0, unit = (trsv & LHPC_TRSV_UNIT_DIAG) != 0;
  o = TrsvLayout();
  o.n = n;
  o.chain_rows = chain_rows == 0 ? kTrsvChainRowsAuto : chain_rows < 0 ? -1 : chain_rows;
  std::vector<int32_t> level(static_cast<size_t>(n));
  const int st = sptrsv_levels_host(n, nnz, row_ptr, bits, col, trsv, level.data(), &o.n_levels);
  if (st != LHPC_OK) return st;
  const size_t nl = static_cast<size_t>(o.n_levels);
  // rows by level, ascending row index inside a level (a counting sort)
  std::vector<int64_t> first(nl + 1, 0);
  for (int64_t i = 0; i < n; ++i) ++first[static_cast<size_t>(level[i]) + 1];
  o.level_slice.assign(nl + 1, 0);
  std::vector<int64_t> rows(nl);  // rows of every level
  for (size_t l = 0; l < nl; ++l) {
    rows[l] = first[l + 1];
    o.max_level_rows = std::max(o.max_level_rows, first[l + 1]);
    o.level_slice[l + 1] = o.level_slice[l] + (first[l + 1] + kTrsvSlice - 1) / kTrsvSlice;
    first[l + 1] = 0;  // from here on: rows of level l placed so far
  }
  o.n_slices = o.level_slice[nl];
  const size_t slots = static_cast<size_t>(o.n_slices) * kTrsvSlice;
  o.slice_row.assign(slots, -1);
  std::vector<int32_t> width(static_cast<size_t>(o.n_slices), 0);  // the slice's longest row
  std::vector<int64_t> slot_of(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    const size_t l = static_cast<size_t>(level[i]);
    const int64_t slot = o.level_slice[l] * kTrsvSlice + first[l + 1]++;
    slot_of[i] = slot;
    o.slice_row[slot] = static_cast<int32_t>(i);
    int64_t len = 0;
    for (int64_t p = rp_at(row_ptr, bits, i); p < rp_at(row_ptr, bits, i + 1); ++p) len += kept(upper, i, col[p]);
    // a row longer than INT32_MAX entries cannot be walked by the kernels' int loop
    if (len > INT32_MAX) return LHPC_ERR_UNSUPPORTED;
    int32_t &w = width[slot / kTrsvSlice];
    w = std::max(w, static_cast<int32_t>(len));
    o.kept += len;
  }
  o.slice_off.assign(static_cast<size_t>(o.n_slices) + 1, 0);
  for (int64_t s = 0; s < o.n_slices; ++s) o.slice_off[s + 1] = o.slice_off[s] + int64_t{width[s]} * kTrsvSlice;
  o.padded = o.slice_off[o.n_slices];
  o.col.assign(static_cast<size_t>(o.padded), -1);
  o.src.assign(static_cast<size_t>(o.padded) + (unit ? 0 : slots), kTrsvNoSource);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t slot = slot_of[i], lane = slot % kTrsvSlice;
    int64_t q = o.slice_off[slot / kTrsvSlice] + lane;  // entry e at off + e·64 + lane
    for (int64_t p = rp_at(row_ptr, bits, i); p < rp_at(row_ptr, bits, i + 1); ++p) {
      const int32_t c = col[p];
      if (c == i) {
        if (!unit) o.src[static_cast<size_t>(o.padded + slot)] = static_cast<uint32_t>(p);
      } else if (kept(upper, i, c)) {
        o.col[q] = c;
        o.src[q] = static_cast<uint32_t>(p);
        q += kTrsvSlice;
      }
    }
  }
  // the schedule: a level above the threshold is a grid step of its own, a
  // maximal run of levels at or below it one chain step
  for (int64_t l = 0; l < o.n_levels;) {
    TrsvStep st;
    st.level_begin = l;
    st.chain = o.chain_rows > 0 && rows[l] <= o.chain_rows;
    ++l;
    if (st.chain)
      while (l < o.n_levels && rows[l] <= o.chain_rows) ++l;
    st.level_end = l;
    st.slice_begin = o.level_slice[st.level_begin];
    st.slice_end = o.level_slice[st.level_end];
    o.steps.push_back(st);
  }
  return LHPC_OK;
}

}  // namespace lhpc

using namespace lhpc;

extern "C" int lhpc_sptrsv_levels(int64_t n, int64_t nnz, const void *row_ptr, int row_ptr_bits,
                                  const int32_t *col_idx, unsigned trsv, int32_t *level, int64_t *n_levels) {
  try {
    if (n < 0 || nnz < 0 || n > INT32_MAX || !row_ptr || (row_ptr_bits != 32 && row_ptr_bits != 64) ||
        (nnz > 0 && !col_idx) || (n > 0 && !level) || !n_levels ||
        (trsv & ~static_cast<unsigned>(LHPC_TRSV_UPPER | LHPC_TRSV_UNIT_DIAG)) ||
        (row_ptr_bits == 32 && nnz > INT32_MAX))
      return LHPC_ERR_INVALID_ARG;
    return sptrsv_levels_host(n, nnz, row_ptr, row_ptr_bits, col_idx, trsv, level, n_levels);
  } LHPC_ABI_CATCH
}
