// lhpc_spmm_plan.hpp — the SpMM plan (lhpc_spmm.hip) and what its callers in
// other translation units share with it: lhpc_solver_multi.hip keeps its work
// with the plan, as lhpc_cg_solve does with the SpMV plan.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

#include "lhpc_common.hpp"

struct lhpc_spmm_plan {
  int dtype = LHPC_F32;
  int device = 0;
  int rp64 = 0;  // device row_ptr is int64 (the caller's width is kept)
  int64_t n_rows = 0, n_cols = 0, nnz = 0;
  void *d_row_ptr = nullptr;
  int32_t *d_col = nullptr;
  void *d_val = nullptr;
  int64_t *d_blocks = nullptr;  // {first row, its row_ptr} per block boundary
  int64_t n_blocks = 0, n_long = 0;
  int64_t bytes = 0;
  // host-buffer calls: packed (ld = k) copies of X and Y, grown on demand
  void *d_xstage = nullptr, *d_ystage = nullptr;
  size_t xstage_bytes = 0, ystage_bytes = 0;
  // lhpc_spmm_dot: per-block, per-column partials (n_blocks × k fp64), grown on demand
  void *d_dpart = nullptr;
  size_t dpart_bytes = 0;
  // lhpc_cg_solve_multi (lhpc_solver_multi.hip), one solve at a time: R, P, Q
  // packed at ld = k; per-column fp64 scalars, modes and row-tile partials;
  // the pinned buffer the host reads the scalars through.  Grown with k.
  std::atomic<int> cg_busy{0};
  void *cg_vecs = nullptr, *cg_scal = nullptr;
  size_t cg_vecs_bytes = 0, cg_scal_bytes = 0;
  void *cg_host = nullptr;
  size_t cg_host_bytes = 0;
  // LHPC_PLAN_TRANSPOSE (the plan is Aᵀ's): entry q of Aᵀ is entry d_tperm[q]
  // of the caller's A; lhpc_spmm_plan_set_values gathers the caller's values
  // into d_tval (nnz values, allocated by the first update)
  uint32_t *d_tperm = nullptr;
  void *d_tval = nullptr;
};

namespace lhpc {

constexpr int kSpmmPanelMax = 32;  // widest column panel of one launch
// Per-column dots over row-major n × k blocks (lhpc_spmm_dot, the multi-RHS
// solver): the rows of a unit (a block of the SpMM table, a row tile of the
// solver) are summed in kDotStreams interleaved streams, stream s holding the
// unit's local rows r ≡ s (mod 64) in ascending r; the 64 stream sums are
// added in ascending s; the units' partials are added per column by
// coldot_finish_launch in an order that depends on their number only.
constexpr int kDotStreams = 64;
constexpr int kPanelThreads = 256;  // workgroup of the panel kernels (= kBlock)

// One column's stream sums → LDS, and their sum in ascending s.  Group g of
// the G = 256 / P lane groups holds streams g, g + G, … in d[0 .. NS); lane j
// of a group owns column j of the panel.  `part` is 64·P doubles of LDS that
// no lane still reads for anything else.  Valid in the lanes of group 0.
template <int P, int NS>
__device__ __forceinline__ double dot_streams_sum(const double (&d)[NS], double *part, int g, int j) {
  constexpr int G = kPanelThreads / P;
  static_assert(NS * G == kDotStreams, "every stream has one group");
#pragma unroll
  for (int u = 0; u < NS; ++u) part[(g + u * G) * P + j] = d[u];
  __syncthreads();
  double t = 0.0;
  if (g == 0) {
    t = part[j];
    for (int s = 1; s < kDotStreams; ++s) t += part[s * P + j];
  }
  return t;
}

// d[u] += v for the one u == sel (sel is uniform over the lanes of a wave)
template <int NS>
__device__ __forceinline__ void dot_stream_add(double (&d)[NS], int sel, double v) {
#pragma unroll
  for (int u = 0; u < NS; ++u)
    if (u == sel) d[u] += v;
}

// ---- lhpc_spmm.hip
// free + allocate when `want` exceeds what the buffer has (accounted in acct)
int spmm_grow(void **buf, size_t &have, size_t want, int64_t &acct);
// the partials buffer of lhpc_spmm_dot for k columns, so that later calls allocate nothing
int spmm_dot_reserve(lhpc_spmm_plan *p, int k);
// out[j] = Σ_u part[u·k + j], u < n_units, one workgroup per column: thread t
// adds units t, t + 256, … ascending, then the fixed tree of one workgroup —
// an order that depends on n_units only.  n_units = 0 writes 0.  A column
// with mode[j] == 0 is skipped (out[j] keeps its value); mode = null: none is.
int coldot_finish_launch(const double *part, int64_t n_units, int k, const int *mode, double *out, hipStream_t s);

}  // namespace lhpc
