// lhpc_sptrsv.hpp — the host analysis of the level-scheduled triangular solve
// (lhpc_sptrsv_host.cpp, no HIP dependency) and the layout it hands to the
// device side (lhpc_sptrsv.hip).  include/lhpc.h "CSR triangular solve" states
// the operator; DESIGN.md §4.6 the layout and the schedule.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/lhpc.h"

namespace lhpc {

constexpr int kTrsvSlice = 64;                 // rows per slice: one wave, a lane per row
constexpr int kTrsvChainThreads = 1024;        // the chain step's one workgroup (16 waves)
constexpr int kTrsvChainRowsAuto = 256;        // chain_rows = 0: measured, DESIGN.md §4.6
constexpr uint32_t kTrsvNoSource = 0xFFFFFFFFu;  // a layout slot without a CSR entry (padding, idle lane)

// One kernel launch of lhpc_sptrsv: levels [level_begin, level_end), whose
// slices are [slice_begin, slice_end).  A grid step covers one level.
struct TrsvStep {
  int64_t slice_begin = 0, slice_end = 0;
  int64_t level_begin = 0, level_end = 0;
  int chain = 0;
};

struct TrsvLayout {
  int64_t n = 0, kept = 0, n_levels = 0, max_level_rows = 0, n_slices = 0, padded = 0;
  int chain_rows = 0;  // the threshold in force (< 0: never chain)
  std::vector<int64_t> level_slice;  // n_levels + 1: the first slice of every level
  std::vector<int64_t> slice_off;    // n_slices + 1: the slice's first entry (a multiple of 64 apart)
  std::vector<int32_t> slice_row;    // n_slices · 64: the lane's row, −1 for an idle lane
  std::vector<int32_t> col;          // padded: column, −1 for padding
  // padded + n_slices · 64 (without a unit diagonal; else padded): the CSR
  // position of every layout entry, then of every lane's diagonal
  std::vector<uint32_t> src;
  std::vector<TrsvStep> steps;
};

// level[0..n) and *n_levels by the rule of include/lhpc.h; LHPC_ERR_BAD_CSR
// for an invalid A or (non-unit) a row without exactly one diagonal entry.
// Nothing indexes an array by a column before that column has been checked.
int sptrsv_levels_host(int64_t n, int64_t nnz, const void *row_ptr, int bits, const int32_t *col, unsigned trsv,
                       int32_t *level, int64_t *n_levels);
// The whole analysis: levels, slices, padded columns, source positions and
// the launch schedule for chain_rows (0: automatic).
int sptrsv_layout_host(TrsvLayout &o, int64_t n, int64_t nnz, const void *row_ptr, int bits, const int32_t *col,
                       unsigned trsv, int chain_rows);

}  // namespace lhpc
