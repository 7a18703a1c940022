// test_transpose_api.cpp — sparse::transpose (include/sparse/Transpose.hpp) and
// LHPC_PLAN_TRANSPOSE plans of sparse::SpMVPlan / sparse::SpMMPlan as a
// reference user would call them.  A rectangular CSRMatrix with unsorted rows
// and a duplicate coordinate is transposed on the GPU and compared, array by
// array, with a host counting transposition (stable by construction); the
// transposed plan is compared bit for bit with a plan built from the
// transposed matrix, before and after set_values in A's CSR order; dyadic
// values, so a host double-precision loop gives the same bits too.  Built by
// tests/cpp/transpose.mk (tests/test_transpose_api.py) and run on the GPU by
// tests/test_gpu_transpose.py; exit status 0 = pass.
#include <HPCHighDimensionFlatArray.hpp>
#include <sparse/SpMM.hpp>
#include <sparse/SpMV.hpp>
#include <sparse/Transpose.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <system_error>
#include <vector>

namespace {

int fail(const char *what) {
  std::fprintf(stderr, "FAIL: %s\n", what);
  return 1;
}

double dyadic(unsigned i) { return static_cast<double>(static_cast<int>((i * 2654435761u) >> 28) % 17 - 8) * 0.125; }

template <typename V>
bool same_bits(const V &a, const V &b) {
  return a.size() == b.size() &&
         (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(typename V::value_type)) == 0);
}

template <typename T>
std::vector<T> apply_plan(sparse::SpMVPlan<T> &plan, const std::vector<T> &x) {
  hpc::HPCHighDimensionFlatArray<1, T> X(x.size()), Y(static_cast<std::size_t>(plan.rows()));
  for (std::size_t i = 0; i < x.size(); ++i) X(i) = x[i];
  sparse::spmv(plan, X, Y);
  std::vector<T> y(static_cast<std::size_t>(plan.rows()));
  for (std::size_t i = 0; i < y.size(); ++i) y[i] = Y(i);
  return y;
}

// host transposition: count per column, scan, place in position order (stable)
template <typename T, typename OffsetT>
sparse::CSRMatrix<T, std::int32_t, OffsetT> host_transpose(const sparse::CSRMatrix<T, std::int32_t, OffsetT> &A,
                                                           std::vector<std::uint32_t> &perm) {
  sparse::CSRMatrix<T, std::int32_t, OffsetT> At(A.n_cols, A.n_rows);
  const std::size_t nnz = A.col_idx.size();
  At.col_idx.resize(nnz);
  At.val.resize(nnz);
  perm.assign(nnz, 0u);
  for (std::size_t p = 0; p < nnz; ++p) ++At.row_ptr[static_cast<std::size_t>(A.col_idx[p]) + 1];
  for (std::int64_t c = 0; c < A.n_cols; ++c)
    At.row_ptr[static_cast<std::size_t>(c) + 1] += At.row_ptr[static_cast<std::size_t>(c)];
  std::vector<OffsetT> next(At.row_ptr.begin(), At.row_ptr.end() - 1);
  for (std::int64_t r = 0; r < A.n_rows; ++r)
    for (auto p = A.row_ptr[static_cast<std::size_t>(r)]; p < A.row_ptr[static_cast<std::size_t>(r) + 1]; ++p) {
      const auto q = static_cast<std::size_t>(next[static_cast<std::size_t>(A.col_idx[static_cast<std::size_t>(p)])]++);
      At.col_idx[q] = static_cast<std::int32_t>(r);
      At.val[q] = A.val[static_cast<std::size_t>(p)];
      perm[q] = static_cast<std::uint32_t>(p);
    }
  return At;
}

template <typename T, typename OffsetT>
int run(std::int64_t n, std::int64_t m, unsigned flags) {
  sparse::CSRMatrix<T, std::int32_t, OffsetT> A(n, m);
  for (std::int64_t i = 0; i < n; ++i) {
    const int len = static_cast<int>(i % 9);  // 0 … 8 per row, columns in no order
    for (int j = 0; j < len; ++j) {
      A.col_idx.push_back(static_cast<std::int32_t>((i * 37 + (len - j) * 151) % m));
      A.val.push_back(static_cast<T>(dyadic(static_cast<unsigned>(i * 31 + j))));
    }
    if (len >= 2) A.col_idx.back() = A.col_idx[A.col_idx.size() - 2];  // a duplicate coordinate, other value
    A.row_ptr[static_cast<std::size_t>(i + 1)] = static_cast<OffsetT>(A.col_idx.size());
  }
  std::vector<std::uint32_t> perm, want_perm;
  const auto want = host_transpose(A, want_perm);
  const auto At = sparse::transpose(A, perm);
  if (At.n_rows != m || At.n_cols != n) return fail("transpose: shape");
  if (!same_bits(At.row_ptr, want.row_ptr)) return fail("transpose: row_ptr");
  if (!same_bits(At.col_idx, want.col_idx)) return fail("transpose: col_idx");
  if (!same_bits(At.val, want.val)) return fail("transpose: val");
  if (!same_bits(perm, want_perm)) return fail("transpose: perm");
  const auto At2 = sparse::transpose(A);  // without perm
  if (!same_bits(At2.col_idx, want.col_idx) || !same_bits(At2.val, want.val)) return fail("transpose without perm");
  // (Aᵀ)ᵀ has A's entries with every row sorted by column, ties in input order: again Aᵀ when transposed
  const auto Att = sparse::transpose(At);
  if (Att.n_rows != n || !same_bits(Att.row_ptr, A.row_ptr)) return fail("transpose twice: row_ptr");
  const auto Attt = sparse::transpose(Att);
  if (!same_bits(Attt.col_idx, At.col_idx) || !same_bits(Attt.val, At.val)) return fail("transpose three times");

  std::vector<T> x(static_cast<std::size_t>(n));  // Aᵀ·x reads n values
  for (std::int64_t r = 0; r < n; ++r) x[static_cast<std::size_t>(r)] = static_cast<T>(dyadic(static_cast<unsigned>(r * 13 + 5)));
  sparse::SpMVPlan<T> tp(A, -1, flags | LHPC_PLAN_TRANSPOSE), fresh(At, -1, flags);
  if (tp.rows() != m || tp.cols() != n || !tp.is_transposed()) return fail("transposed plan: rows() / cols()");
  const lhpc_spmv_plan_info ti = tp.info(), fi = fresh.info();
  if (ti.n_rows != m || ti.n_cols != n || ti.kernel != fi.kernel || ti.nnz != fi.nnz) return fail("transposed plan: info");
  const std::vector<T> y = apply_plan(tp, x);
  if (!same_bits(y, apply_plan(fresh, x))) return fail("transposed plan against the plan of the transposed matrix");
  std::vector<T> host(static_cast<std::size_t>(m));
  {
    std::vector<double> acc(static_cast<std::size_t>(m), 0.0);  // dyadic: any order is exact
    for (std::int64_t r = 0; r < n; ++r)
      for (auto p = A.row_ptr[static_cast<std::size_t>(r)]; p < A.row_ptr[static_cast<std::size_t>(r) + 1]; ++p)
        acc[static_cast<std::size_t>(A.col_idx[static_cast<std::size_t>(p)])] +=
            static_cast<double>(A.val[static_cast<std::size_t>(p)]) * static_cast<double>(x[static_cast<std::size_t>(r)]);
    for (std::size_t c = 0; c < host.size(); ++c) host[c] = static_cast<T>(acc[c]);
  }
  for (std::size_t c = 0; c < host.size(); ++c)
    if (y[c] != host[c]) return fail("transposed plan against the host loop");

  // set_values in A's order: the CSRMatrix overload checks A's shape
  auto B = A;
  for (std::size_t k = 0; k < B.val.size(); ++k) B.val[k] = static_cast<T>(dyadic(static_cast<unsigned>(7 * k + 3)));
  std::vector<std::uint32_t> unused;
  const auto Bt = host_transpose(B, unused);
  sparse::SpMVPlan<T> fresh_b(Bt, -1, flags);
  const std::vector<T> want_b = apply_plan(fresh_b, x);
  if (same_bits(want_b, y)) return fail("the two value sets give the same y: the test shows nothing");
  tp.set_values(B);
  if (!same_bits(apply_plan(tp, x), want_b)) return fail("set_values(CSRMatrix) on a transposed plan");
  tp.set_values(A.val.data(), A.nnz());
  if (!same_bits(apply_plan(tp, x), y)) return fail("set_values(host pointer) on a transposed plan");
  bool threw = false;
  try {
    tp.set_values(Bt);  // the operator's shape is not A's (n ≠ m)
  } catch (const std::system_error &) {
    threw = true;
  }
  if (!threw) return fail("set_values(matrix of the operator's shape) did not throw");

  // the SpMM plan: k = 3 columns that all hold x
  constexpr int k = 3;
  sparse::SpMMPlan<T> mm(A, -1, LHPC_PLAN_TRANSPOSE);
  if (mm.rows() != m || mm.cols() != n) return fail("transposed SpMM plan: rows() / cols()");
  hpc::HPCHighDimensionFlatArray<2, T> X(static_cast<std::size_t>(n), k), Y(static_cast<std::size_t>(m), k);
  for (std::int64_t r = 0; r < n; ++r)
    for (int j = 0; j < k; ++j) X(r, j) = x[static_cast<std::size_t>(r)];
  sparse::spmm(mm, X, Y);
  for (std::int64_t c = 0; c < m; ++c)
    for (int j = 0; j < k; ++j)
      if (Y(c, j) != host[static_cast<std::size_t>(c)]) return fail("transposed SpMM plan");
  mm.set_values(B);
  sparse::spmm(mm, X, Y);
  for (std::int64_t c = 0; c < m; ++c)
    for (int j = 0; j < k; ++j)
      if (std::memcmp(&Y(c, j), &want_b[static_cast<std::size_t>(c)], sizeof(T)) != 0)
        return fail("transposed SpMM plan after set_values(CSRMatrix)");
  return 0;
}

}  // namespace

int main() {
  try {
    if (int st = run<float, std::int32_t>(3000, 2570, LHPC_PLAN_FORCE_XTILE)) return st;
    if (int st = run<double, std::int64_t>(1290, 2000, LHPC_PLAN_FORCE_XTILE)) return st;
    if (int st = run<double, std::int32_t>(1290, 2000, LHPC_PLAN_FORCE_ADAPTIVE)) return st;
    if (int st = run<float, std::int64_t>(300, 257, LHPC_PLAN_DEFAULT)) return st;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "FAIL: exception: %s\n", e.what());
    return 1;
  }
  std::printf("transpose cpp api: ok\n");
  return 0;
}
