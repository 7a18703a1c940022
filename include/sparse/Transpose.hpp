// sparse/Transpose.hpp — Aᵀ of a host sparse::CSRMatrix, computed on the GPU.
//
//   auto At = sparse::transpose(A);                 // CSRMatrix, A.n_cols × A.n_rows
//   std::vector<std::uint32_t> perm;
//   auto At = sparse::transpose(A, perm);           // … and the entry permutation
//
// Forwards to lhpc_csr_transpose (include/lhpc.h "CSR transpose"): entry q of
// Aᵀ is entry perm[q] of A, the order of a stable sort of A's entry positions
// by column, so rows of Aᵀ come out with ascending columns, duplicates are
// kept in input order, and transposing twice gives a sorted-row CSR back.
// The reference has no counterpart.  For a plan of Aᵀ there is no need to
// transpose first: pass LHPC_PLAN_TRANSPOSE to sparse::SpMVPlan / SpMMPlan.
// device ≥ 0 selects the GPU (needs the HIP runtime); −1 is the current one.
#pragma once
#ifndef LHPC_SPARSE_TRANSPOSE_HPP_
#define LHPC_SPARSE_TRANSPOSE_HPP_

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <type_traits>
#include <vector>

#include "../lhpc.h"
#include "../lhpc_error.hpp"
#include "CSRMatrix.hpp"

namespace sparse {

namespace detail {
template <typename T, typename OffsetT>
CSRMatrix<T, std::int32_t, OffsetT> transpose_impl(const CSRMatrix<T, std::int32_t, OffsetT> &A, std::uint32_t *perm,
                                                   int device) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "transpose is fp32 or fp64");
  if (static_cast<std::int64_t>(A.row_ptr.size()) != A.n_rows + 1 || A.val.size() != A.col_idx.size())
    lhpc::throwLhpcError(LHPC_ERR_INVALID_ARG, __FILE__, __LINE__);
  int prev = -1;
  if (device >= 0) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) lhpc::throwLhpcError(static_cast<int>(e), __FILE__, __LINE__);
  }
  CSRMatrix<T, std::int32_t, OffsetT> At(A.n_cols, A.n_rows);
  At.col_idx.resize(A.col_idx.size());
  At.val.resize(A.val.size());
  const bool pattern = A.val.empty();  // nnz = 0: nothing to read
  const int st = lhpc_csr_transpose(std::is_same_v<T, float> ? LHPC_F32 : LHPC_F64, A.n_rows, A.n_cols, A.nnz(),
                                    A.row_ptr.data(), sizeof(OffsetT) * 8, A.col_idx.data(),
                                    pattern ? nullptr : A.val.data(), At.row_ptr.data(), At.col_idx.data(),
                                    pattern ? nullptr : At.val.data(), perm, /*on_device=*/0, nullptr);
  if (device >= 0 && prev >= 0) (void)hipSetDevice(prev);
  lhpc::checkLhpc(st);
  return At;
}
}  // namespace detail

template <typename T, typename OffsetT>
CSRMatrix<T, std::int32_t, OffsetT> transpose(const CSRMatrix<T, std::int32_t, OffsetT> &A, int device = -1) {
  return detail::transpose_impl(A, nullptr, device);
}

// … also returning perm (nnz entries): At.val[q] == A.val[perm[q]]
template <typename T, typename OffsetT>
CSRMatrix<T, std::int32_t, OffsetT> transpose(const CSRMatrix<T, std::int32_t, OffsetT> &A,
                                              std::vector<std::uint32_t> &perm, int device = -1) {
  perm.assign(static_cast<std::size_t>(A.nnz()), 0u);
  return detail::transpose_impl(A, perm.data(), device);
}

}  // namespace sparse
#endif  // LHPC_SPARSE_TRANSPOSE_HPP_
