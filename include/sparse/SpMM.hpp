// sparse/SpMM.hpp — Y = A·X on MI355X behind the reference's host types: one
// CSR matrix applied to a row-major block of k vectors at once.
//
//   sparse::SpMMPlan<T>  RAII owner of the HBM copy of A (CSR, one per GPU)
//   sparse::spmm(plan, X, Y)  with X, Y hpc::HPCHighDimensionFlatArray<2,T,...>
//                             (host, synchronous): X is n_cols × k, Y n_rows × k;
//                             the arrays' padded row lengths are the leading
//                             dimensions, ghost cells are skipped and untouched
//   sparse::spmm(plan, k, d_X, ldx, d_Y, ldy, stream)  raw HBM pointers (async)
//   sparse::spmm_dot(plan, k, d_X, ldx, d_Y, ldy, d_W, ldw, d_dots, stream)
//                             the same with d_dots[j] = Σ_i W[i,j]·Y[i,j] (async)
//   sparse::cg(plan, k, d_B, ldb, d_X, ldx, tol, max_iter, check_every, stream)
//                             k CG solves in step on one SpMM per iteration
//                             (synchronous) → CGMultiResult
// Forwards to the C ABI (include/lhpc.h "CSR SpMM"); non-zero status →
// std::system_error (include/lhpc_error.hpp).  The reference has no SpMM (and
// no SpMV); the operator and its numerics are defined in DESIGN.md.
#pragma once
#ifndef LHPC_SPARSE_SPMM_HPP_
#define LHPC_SPARSE_SPMM_HPP_

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
class SpMMPlan {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "SpMM is fp32 or fp64");

 public:
  template <typename OffsetT>
  explicit SpMMPlan(const CSRMatrix<T, std::int32_t, OffsetT> &A, int device = -1, unsigned flags = LHPC_PLAN_DEFAULT)
      : n_rows_(A.n_rows), n_cols_(A.n_cols) {
    transposed(flags);
    lhpc::checkLhpc(lhpc_spmm_plan_create(&plan_, std::is_same_v<T, float> ? LHPC_F32 : LHPC_F64, A.n_rows, A.n_cols,
                                          A.nnz(), A.row_ptr.data(), sizeof(OffsetT) * 8, A.col_idx.data(),
                                          A.val.data(), device, flags));
  }
  // A already in HBM (sparse/DeviceCSR.hpp): validated and copied on the device
  explicit SpMMPlan(const DeviceCSRView<T> &A, unsigned flags = LHPC_PLAN_DEFAULT)
      : n_rows_(A.n_rows), n_cols_(A.n_cols) {
    transposed(flags);
    lhpc::checkLhpc(lhpc_spmm_plan_create(&plan_, std::is_same_v<T, float> ? LHPC_F32 : LHPC_F64, A.n_rows, A.n_cols,
                                          A.nnz, A.row_ptr, A.row_ptr_bits, A.col_idx, A.val, A.device,
                                          flags | LHPC_PLAN_DEVICE_INPUT));
  }
  SpMMPlan(const SpMMPlan &) = delete;
  SpMMPlan &operator=(const SpMMPlan &) = delete;
  SpMMPlan(SpMMPlan &&o) noexcept
      : plan_(std::exchange(o.plan_, nullptr)), n_rows_(o.n_rows_), n_cols_(o.n_cols_), transposed_(o.transposed_) {}
  SpMMPlan &operator=(SpMMPlan &&o) noexcept {
    if (this != &o) {
      reset();
      plan_ = std::exchange(o.plan_, nullptr);
      n_rows_ = o.n_rows_;
      n_cols_ = o.n_cols_;
      transposed_ = o.transposed_;
    }
    return *this;
  }
  ~SpMMPlan() { reset(); }

  lhpc_spmm_plan_info info() const {
    lhpc_spmm_plan_info i{};
    lhpc::checkLhpc(lhpc_spmm_plan_info_get(plan_, &i));
    return i;
  }
  // Same structure, new values (lhpc_spmm_plan_set_values), as
  // SpMVPlan<T>::set_values: one copy into the plan's CSR val.
  void set_values(const T *val, std::int64_t nnz, bool on_device = false, void *stream = nullptr) {
    lhpc::checkLhpc(lhpc_spmm_plan_set_values(plan_, val, nnz, on_device ? 1 : 0, stream));
  }
  template <typename OffsetT>
  void set_values(const CSRMatrix<T, std::int32_t, OffsetT> &A) {
    // a LHPC_PLAN_TRANSPOSE plan: A's shape (and CSR order), not the operator's
    if (A.n_rows != (transposed_ ? n_cols_ : n_rows_) || A.n_cols != (transposed_ ? n_rows_ : n_cols_))
      lhpc::throwLhpcError(LHPC_ERR_INVALID_ARG, __FILE__, __LINE__);
    set_values(A.val.data(), static_cast<std::int64_t>(A.nnz()));
  }
  std::int64_t rows() const noexcept { return n_rows_; }
  std::int64_t cols() const noexcept { return n_cols_; }
  bool is_transposed() const noexcept { return transposed_; }
  lhpc_spmm_plan *native() noexcept { return plan_; }

 private:
  void reset() noexcept {
    if (plan_) lhpc_spmm_plan_destroy(plan_);
    plan_ = nullptr;
  }
  // LHPC_PLAN_TRANSPOSE: the plan is Aᵀ's, rows() and cols() the operator's
  void transposed(unsigned flags) noexcept {
    transposed_ = (flags & LHPC_PLAN_TRANSPOSE) != 0;
    if (transposed_) std::swap(n_rows_, n_cols_);
  }
  lhpc_spmm_plan *plan_ = nullptr;
  std::int64_t n_rows_ = 0, n_cols_ = 0;
  bool transposed_ = false;
};

// Host blocks: the logical cells [0, n) × [0, k) of 2-D flat arrays.  The
// padded physical row length is the leading dimension and the data pointer is
// offset past the ghost rows and columns, which are left untouched.
// Synchronous.
template <typename T, std::size_t LX, std::size_t HX, std::size_t AX, class AlX, std::size_t LY,
          std::size_t HY, std::size_t AY, class AlY>
void spmm(SpMMPlan<T> &plan, const hpc::HPCHighDimensionFlatArray<2, T, LX, HX, AX, AlX> &X,
          hpc::HPCHighDimensionFlatArray<2, T, LY, HY, AY, AlY> &Y) {
  const std::size_t k = X.dims()[1];
  if (static_cast<std::int64_t>(X.dims()[0]) < plan.cols() || static_cast<std::int64_t>(Y.dims()[0]) < plan.rows() ||
      Y.dims()[1] != k || k < 1 || k > static_cast<std::size_t>(INT32_MAX))
    lhpc::throwLhpcError(LHPC_ERR_INVALID_ARG, __FILE__, __LINE__);
  const std::int64_t ldx = static_cast<std::int64_t>(X.strides()[0]), ldy = static_cast<std::int64_t>(Y.strides()[0]);
  lhpc::checkLhpc(lhpc_spmm(plan.native(), static_cast<int>(k), X.data() + LX * ldx + LX, ldx,
                            Y.data() + LY * ldy + LY, ldy, 0, nullptr));
}

// Device blocks (HBM pointers, leading dimensions in elements), asynchronous
// on `stream` (a hipStream_t).
template <typename T>
void spmm(SpMMPlan<T> &plan, int k, const T *d_X, std::int64_t ldx, T *d_Y, std::int64_t ldy,
          void *stream = nullptr) {
  lhpc::checkLhpc(lhpc_spmm(plan.native(), k, d_X, ldx, d_Y, ldy, 1, stream));
}

// Y = A·X as spmm stores it and d_dots[j] = Σ_i W[i, j]·Y[i, j] (fp64, k
// doubles in HBM) in one pass over A; W is n_rows × k and may be X when A is
// square.  Asynchronous on `stream`.
template <typename T>
void spmm_dot(SpMMPlan<T> &plan, int k, const T *d_X, std::int64_t ldx, T *d_Y, std::int64_t ldy, const T *d_W,
              std::int64_t ldw, double *d_dots, void *stream = nullptr) {
  lhpc::checkLhpc(lhpc_spmm_dot(plan.native(), k, d_X, ldx, d_Y, ldy, d_W, ldw, d_dots, stream));
}

// per column: the iteration at which it stopped and its ‖r‖/‖b‖
struct CGMultiResult {
  std::vector<int> iterations;
  std::vector<double> residual;
};

// Conjugate gradient for the k columns of d_B (row-major n × k in HBM) on one
// SpMM per iteration; d_X holds the initial guesses and receives the
// solutions (lhpc_cg_solve_multi).  Synchronous.  A column that broke down
// (the matrix is not SPD) makes the call throw, like every non-zero status.
template <typename T>
CGMultiResult cg(SpMMPlan<T> &plan, int k, const T *d_B, std::int64_t ldb, T *d_X, std::int64_t ldx,
                 double tol = 1e-8, int max_iter = 1000, int check_every = 1, void *stream = nullptr) {
  if (k < 1) lhpc::throwLhpcError(LHPC_ERR_INVALID_ARG, __FILE__, __LINE__);
  CGMultiResult r{std::vector<int>(static_cast<std::size_t>(k)), std::vector<double>(static_cast<std::size_t>(k))};
  lhpc::checkLhpc(lhpc_cg_solve_multi(plan.native(), k, d_B, ldb, d_X, ldx, tol, max_iter, check_every,
                                      r.iterations.data(), r.residual.data(), stream));
  return r;
}

}  // namespace sparse
#endif  // LHPC_SPARSE_SPMM_HPP_
