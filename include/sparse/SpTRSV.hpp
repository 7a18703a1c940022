// sparse/SpTRSV.hpp — x = L⁻¹·b / x = U⁻¹·b for a sparse triangle on MI355X
// behind the reference's host types: the level-scheduled solve under
// Gauss–Seidel / SSOR sweeps and ILU(0) / IC(0) applications.
//
//   sparse::SpTRSVPlan<T>  RAII owner of the analysed triangle in HBM; A is
//                          square and may hold both triangles (trsv picks one:
//                          LHPC_TRSV_LOWER / LHPC_TRSV_UPPER, | LHPC_TRSV_UNIT_DIAG)
//   sparse::sptrsv(plan, b, x)  with b, x hpc::HPCHighDimensionFlatArray<1,T,...>
//                               (host, synchronous); x may be b
//   sparse::sptrsv(plan, d_b, d_x, stream)  raw HBM pointers (async, capturable)
//   sparse::sptrsv_levels(A, trsv)  the level of every row (host only)
// For Lᵀ: sparse::transpose (sparse/Transpose.hpp), then LHPC_TRSV_UPPER.
// Forwards to the C ABI (include/lhpc.h "CSR triangular solve", which fixes
// every x_i bit for bit); non-zero status → std::system_error
// (include/lhpc_error.hpp).  The reference has no triangular solve (and no
// SpMV); the operator and its numerics are defined in DESIGN.md.
#pragma once
#ifndef LHPC_SPARSE_SPTRSV_HPP_
#define LHPC_SPARSE_SPTRSV_HPP_

#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "../hpc/HPCHighDimensionFlatArray.hpp"
#include "../lhpc.h"
#include "../lhpc_error.hpp"
#include "CSRMatrix.hpp"
#include "SpMV.hpp"

namespace sparse {

template <typename T>
class SpTRSVPlan {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "SpTRSV is fp32 or fp64");

 public:
  // chain_rows: 0 automatic, < 0 never chain, > 0 the largest level a chain step takes
  template <typename OffsetT>
  explicit SpTRSVPlan(const CSRMatrix<T, std::int32_t, OffsetT> &A, unsigned trsv = LHPC_TRSV_LOWER,
                      int chain_rows = 0, int device = -1, unsigned flags = LHPC_PLAN_DEFAULT)
      : n_(A.n_rows) {
    if (A.n_rows != A.n_cols) lhpc::throwLhpcError(LHPC_ERR_INVALID_ARG, __FILE__, __LINE__);
    lhpc::checkLhpc(lhpc_sptrsv_plan_create(&plan_, std::is_same_v<T, float> ? LHPC_F32 : LHPC_F64, A.n_rows, A.nnz(),
                                            A.row_ptr.data(), sizeof(OffsetT) * 8, A.col_idx.data(), A.val.data(),
                                            trsv, chain_rows, device, flags));
  }
  // A already in HBM (sparse/DeviceCSR.hpp): its arrays come to the host for the analysis
  explicit SpTRSVPlan(const DeviceCSRView<T> &A, unsigned trsv = LHPC_TRSV_LOWER, int chain_rows = 0,
                      unsigned flags = LHPC_PLAN_DEFAULT)
      : n_(A.n_rows) {
    if (A.n_rows != A.n_cols) lhpc::throwLhpcError(LHPC_ERR_INVALID_ARG, __FILE__, __LINE__);
    lhpc::checkLhpc(lhpc_sptrsv_plan_create(&plan_, std::is_same_v<T, float> ? LHPC_F32 : LHPC_F64, A.n_rows, A.nnz,
                                            A.row_ptr, A.row_ptr_bits, A.col_idx, A.val, trsv, chain_rows, A.device,
                                            flags | LHPC_PLAN_DEVICE_INPUT));
  }
  SpTRSVPlan(const SpTRSVPlan &) = delete;
  SpTRSVPlan &operator=(const SpTRSVPlan &) = delete;
  SpTRSVPlan(SpTRSVPlan &&o) noexcept : plan_(std::exchange(o.plan_, nullptr)), n_(o.n_) {}
  SpTRSVPlan &operator=(SpTRSVPlan &&o) noexcept {
    if (this != &o) {
      reset();
      plan_ = std::exchange(o.plan_, nullptr);
      n_ = o.n_;
    }
    return *this;
  }
  ~SpTRSVPlan() { reset(); }

  lhpc_sptrsv_plan_info info() const {
    lhpc_sptrsv_plan_info i{};
    lhpc::checkLhpc(lhpc_sptrsv_plan_info_get(plan_, &i));
    return i;
  }
  // Same structure, new values (lhpc_sptrsv_plan_set_values): A's nnz values
  // in the CSR order the plan was made from, ignored entries in their places.
  void set_values(const T *val, std::int64_t nnz, bool on_device = false, void *stream = nullptr) {
    lhpc::checkLhpc(lhpc_sptrsv_plan_set_values(plan_, val, nnz, on_device ? 1 : 0, stream));
  }
  template <typename OffsetT>
  void set_values(const CSRMatrix<T, std::int32_t, OffsetT> &A) {
    if (A.n_rows != n_ || A.n_cols != n_) lhpc::throwLhpcError(LHPC_ERR_INVALID_ARG, __FILE__, __LINE__);
    set_values(A.val.data(), static_cast<std::int64_t>(A.nnz()));
  }
  std::int64_t rows() const noexcept { return n_; }
  lhpc_sptrsv_plan *native() noexcept { return plan_; }

 private:
  void reset() noexcept {
    if (plan_) lhpc_sptrsv_plan_destroy(plan_);
    plan_ = nullptr;
  }
  lhpc_sptrsv_plan *plan_ = nullptr;
  std::int64_t n_ = 0;
};

// Host vectors: the logical cells [0, n) of 1-D flat arrays, ghost cells
// skipped and untouched.  x may be b itself.  Synchronous.
template <typename T, std::size_t LB, std::size_t HB, std::size_t AB, class AlB, std::size_t LX, std::size_t HX,
          std::size_t AX, class AlX>
void sptrsv(SpTRSVPlan<T> &plan, const hpc::HPCHighDimensionFlatArray<1, T, LB, HB, AB, AlB> &b,
            hpc::HPCHighDimensionFlatArray<1, T, LX, HX, AX, AlX> &x) {
  if (static_cast<std::int64_t>(b.dims()[0]) < plan.rows() || static_cast<std::int64_t>(x.dims()[0]) < plan.rows())
    lhpc::throwLhpcError(LHPC_ERR_INVALID_ARG, __FILE__, __LINE__);
  lhpc::checkLhpc(lhpc_sptrsv(plan.native(), b.data() + LB, x.data() + LX, 0, nullptr));
}

// Device vectors (HBM pointers), asynchronous on `stream` (a hipStream_t):
// kernel launches only, so the call can be captured into a graph.
template <typename T>
void sptrsv(SpTRSVPlan<T> &plan, const T *d_b, T *d_x, void *stream = nullptr) {
  lhpc::checkLhpc(lhpc_sptrsv(plan.native(), d_b, d_x, 1, stream));
}

// level[i] of every row of the triangle trsv picks (lhpc_sptrsv_levels): host
// only.  Throws LHPC_ERR_BAD_CSR for an invalid A or, without
// LHPC_TRSV_UNIT_DIAG, a row without exactly one diagonal entry.
template <typename T, typename OffsetT>
std::vector<std::int32_t> sptrsv_levels(const CSRMatrix<T, std::int32_t, OffsetT> &A, unsigned trsv = LHPC_TRSV_LOWER) {
  if (A.n_rows != A.n_cols) lhpc::throwLhpcError(LHPC_ERR_INVALID_ARG, __FILE__, __LINE__);
  std::vector<std::int32_t> level(static_cast<std::size_t>(A.n_rows));
  std::int64_t n_levels = 0;
  lhpc::checkLhpc(lhpc_sptrsv_levels(A.n_rows, A.nnz(), A.row_ptr.data(), sizeof(OffsetT) * 8, A.col_idx.data(), trsv,
                                     level.data(), &n_levels));
  return level;
}

}  // namespace sparse
#endif  // LHPC_SPARSE_SPTRSV_HPP_
