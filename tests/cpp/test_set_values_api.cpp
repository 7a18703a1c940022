// test_set_values_api.cpp — sparse::SpMVPlan<T>::set_values and
// sparse::SpMMPlan<T>::set_values as a reference user would call them: a plan
// built from a sparse::CSRMatrix follows the matrix when its values change
// (same row_ptr / col_idx).  Every result is compared bit for bit with a
// fresh plan built from the new values; dyadic values, so a host
// double-precision loop gives the same bits too.  Host values (the CSRMatrix
// overload and the pointer overload) and HBM values (on_device).  A wrong nnz
// must throw through lhpc::checkLhpc.  Built by tests/cpp/set_values.mk
// (tests/test_set_values_api.py) and run on the GPU by
// tests/test_gpu_set_values.py; exit status 0 = pass.
#include <HPCHighDimensionFlatArray.hpp>
#include <sparse/SpMM.hpp>
#include <sparse/SpMV.hpp>

#include <hip/hip_runtime.h>

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

template <typename T>
bool same_bits(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

template <typename T>
std::vector<T> apply(sparse::SpMVPlan<T> &plan, const std::vector<T> &x, std::int64_t n) {
  hpc::HPCHighDimensionFlatArray<1, T> X(x.size()), Y(static_cast<std::size_t>(n));
  for (std::size_t i = 0; i < x.size(); ++i) X(i) = x[i];
  sparse::spmv(plan, X, Y);
  std::vector<T> y(static_cast<std::size_t>(n));
  for (std::int64_t i = 0; i < n; ++i) y[static_cast<std::size_t>(i)] = Y(static_cast<std::size_t>(i));
  return y;
}

template <typename T, typename OffsetT>
int run(std::int64_t n, std::int64_t m, unsigned flags) {
  sparse::CSRMatrix<T, std::int32_t, OffsetT> A(n, m);
  for (std::int64_t i = 0; i < n; ++i) {
    const int len = static_cast<int>(i % 9);  // 0 … 8 per row: every kernel family takes it
    for (int j = 0; j < len; ++j) {
      A.col_idx.push_back(static_cast<std::int32_t>((i * 37 + j * 151) % m));
      A.val.push_back(static_cast<T>(dyadic(static_cast<unsigned>(i * 31 + j))));
    }
    A.row_ptr[static_cast<std::size_t>(i + 1)] = static_cast<OffsetT>(A.col_idx.size());
  }
  auto B = A;  // the same structure, other values
  for (std::size_t k = 0; k < B.val.size(); ++k) B.val[k] = static_cast<T>(dyadic(static_cast<unsigned>(7 * k + 3)));
  std::vector<T> x(static_cast<std::size_t>(m));
  for (std::int64_t c = 0; c < m; ++c) x[static_cast<std::size_t>(c)] = static_cast<T>(dyadic(static_cast<unsigned>(c * 13 + 5)));

  sparse::SpMVPlan<T> plan(A, -1, flags), fresh(B, -1, flags);
  const std::vector<T> ya = apply(plan, x, n), want = apply(fresh, x, n);
  std::vector<T> host(static_cast<std::size_t>(n));
  for (std::int64_t i = 0; i < n; ++i) {
    double s = 0.0;
    for (auto e = B.row_ptr[static_cast<std::size_t>(i)]; e < B.row_ptr[static_cast<std::size_t>(i + 1)]; ++e)
      s += static_cast<double>(B.val[static_cast<std::size_t>(e)]) *
           static_cast<double>(x[static_cast<std::size_t>(B.col_idx[static_cast<std::size_t>(e)])]);
    host[static_cast<std::size_t>(i)] = static_cast<T>(s);
  }
  if (!same_bits(want, host)) return fail("fresh plan against the host loop");
  if (same_bits(ya, want)) return fail("the two value sets give the same y: the test shows nothing");

  plan.set_values(B);  // host values, CSRMatrix overload
  if (!same_bits(apply(plan, x, n), want)) return fail("set_values(CSRMatrix)");
  plan.set_values(A.val.data(), A.nnz());  // back, pointer overload
  if (!same_bits(apply(plan, x, n), ya)) return fail("set_values(host pointer)");
  T *dv = nullptr;  // HBM values, asynchronous on the null stream
  if (hipMalloc(&dv, B.val.size() * sizeof(T)) != hipSuccess ||
      hipMemcpy(dv, B.val.data(), B.val.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
    return fail("hipMalloc / hipMemcpy");
  plan.set_values(dv, B.nnz(), true);
  if (!same_bits(apply(plan, x, n), want)) return fail("set_values(device pointer)");

  bool threw = false;
  try {
    plan.set_values(B.val.data(), B.nnz() - 1);
  } catch (const std::system_error &) {
    threw = true;
  }
  if (!threw) return fail("wrong nnz did not throw");
  if (!same_bits(apply(plan, x, n), want)) return fail("a refused call changed the plan");

  // the SpMM plan: k = 3 columns that all hold x
  constexpr int k = 3;
  sparse::SpMMPlan<T> mm(A);
  hpc::HPCHighDimensionFlatArray<2, T> X(static_cast<std::size_t>(m), k), Y(static_cast<std::size_t>(n), k);
  for (std::int64_t c = 0; c < m; ++c)
    for (int j = 0; j < k; ++j) X(c, j) = x[static_cast<std::size_t>(c)];
  mm.set_values(dv, B.nnz(), true);
  if (hipDeviceSynchronize() != hipSuccess) return fail("spmm set_values(device pointer)");
  sparse::spmm(mm, X, Y);
  for (std::int64_t i = 0; i < n; ++i)
    for (int j = 0; j < k; ++j)
      if (Y(i, j) != host[static_cast<std::size_t>(i)]) return fail("spmm after set_values(device pointer)");
  mm.set_values(A);
  sparse::spmm(mm, X, Y);
  for (std::int64_t i = 0; i < n; ++i)
    for (int j = 0; j < k; ++j)
      if (std::memcmp(&Y(i, j), &ya[static_cast<std::size_t>(i)], sizeof(T)) != 0)
        return fail("spmm after set_values(CSRMatrix)");
  (void)hipFree(dv);
  return 0;
}

}  // namespace

int main() {
  try {
    if (int st = run<float, std::int32_t>(3000, 2570, LHPC_PLAN_FORCE_XTILE)) return st;
    if (int st = run<double, std::int64_t>(1290, 2000, LHPC_PLAN_FORCE_XTILE)) return st;
    if (int st = run<double, std::int32_t>(1290, 2000, LHPC_PLAN_FORCE_SELL)) return st;
    if (int st = run<float, std::int64_t>(300, 257, LHPC_PLAN_DEFAULT)) return st;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "FAIL: exception: %s\n", e.what());
    return 1;
  }
  std::printf("set_values cpp api: ok\n");
  return 0;
}
