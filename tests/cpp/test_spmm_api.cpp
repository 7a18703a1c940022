// test_spmm_api.cpp — sparse::SpMMPlan / sparse::spmm as a reference user
// would call them: A a sparse::CSRMatrix, X and Y 2-D
// hpc::HPCHighDimensionFlatArray blocks with non-zero ghost widths (the
// padded row length is the leading dimension), compared with a host
// double-precision loop.  Dyadic values, so every summation order is exact:
// the comparison is bit for bit, and every ghost cell must keep its canary.
// Also the raw-pointer overload on HBM buffers with its own leading
// dimensions.  Built and run by tests/test_gpu_spmm.py; exit status 0 = pass.
#include <HPCHighDimensionFlatArray.hpp>
#include <sparse/SpMM.hpp>

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <system_error>
#include <vector>

namespace {

int fail(const char *what) {
  std::fprintf(stderr, "FAIL: %s\n", what);
  return 1;
}

double dyadic(unsigned i) { return static_cast<double>(static_cast<int>((i * 2654435761u) >> 28) % 17 - 8) * 0.125; }

template <typename T, typename OffsetT>
int run(std::int64_t n, std::int64_t m, int k) {
  sparse::CSRMatrix<T, std::int32_t, OffsetT> A(n, m);
  for (std::int64_t i = 0; i < n; ++i) {
    const int len = i == 7 ? 2500 : static_cast<int>(i % 23);  // one long row, empty rows
    for (int j = 0; j < len; ++j) {
      A.col_idx.push_back(static_cast<std::int32_t>((i * 37 + j * 151) % m));
      A.val.push_back(static_cast<T>(dyadic(static_cast<unsigned>(i * 31 + j))));
    }
    A.row_ptr[static_cast<std::size_t>(i + 1)] = static_cast<OffsetT>(A.col_idx.size());
  }
  constexpr std::size_t GX = 2, GY = 3;
  constexpr T kCanary = T(-77.5);
  hpc::HPCHighDimensionFlatArray<2, T, GX> X(m, k);
  hpc::HPCHighDimensionFlatArray<2, T, GY, 1> Y(n, k);
  for (std::size_t i = 0; i < X.size(); ++i) X.data()[i] = kCanary;
  for (std::size_t i = 0; i < Y.size(); ++i) Y.data()[i] = kCanary;
  for (std::int64_t c = 0; c < m; ++c)
    for (int j = 0; j < k; ++j) X(c, j) = static_cast<T>(dyadic(static_cast<unsigned>(c * 13 + j * 7 + 5)));

  sparse::SpMMPlan<T> plan(A);
  const lhpc_spmm_plan_info inf = plan.info();
  if (inf.n_rows != n || inf.n_cols != m || inf.nnz != A.nnz() || inf.n_long_rows != 1 || inf.panel_max != 32)
    return fail("plan info");
  sparse::spmm(plan, X, Y);

  std::vector<double> want(static_cast<std::size_t>(n) * k, 0.0);
  for (std::int64_t i = 0; i < n; ++i)
    for (auto e = A.row_ptr[static_cast<std::size_t>(i)]; e < A.row_ptr[static_cast<std::size_t>(i + 1)]; ++e)
      for (int j = 0; j < k; ++j)
        want[static_cast<std::size_t>(i) * k + j] +=
            static_cast<double>(A.val[static_cast<std::size_t>(e)]) *
            static_cast<double>(X(A.col_idx[static_cast<std::size_t>(e)], j));
  for (std::int64_t i = 0; i < n; ++i)
    for (int j = 0; j < k; ++j)
      if (Y(i, j) != static_cast<T>(want[static_cast<std::size_t>(i) * k + j])) return fail("spmm on flat arrays");
  // ghost cells of Y (3 low, 1 high in both dimensions) keep the canary
  const std::int64_t ldy = static_cast<std::int64_t>(Y.strides()[0]);
  if (ldy != k + static_cast<std::int64_t>(GY) + 1) return fail("padded row length");
  std::size_t logical = 0;
  for (std::int64_t r = 0; r < n + static_cast<std::int64_t>(GY) + 1; ++r)
    for (std::int64_t c = 0; c < ldy; ++c) {
      const bool in = r >= static_cast<std::int64_t>(GY) && r < static_cast<std::int64_t>(GY) + n &&
                      c >= static_cast<std::int64_t>(GY) && c < static_cast<std::int64_t>(GY) + k;
      logical += in;
      if (!in && Y.data()[r * ldy + c] != kCanary) return fail("ghost cell of Y written");
    }
  if (logical != static_cast<std::size_t>(n) * k) return fail("cell count");

  // raw-pointer overload: HBM buffers, ldx = k + 1, ldy = k + 2, asynchronous
  const std::int64_t ldx = k + 1, ldyd = k + 2;
  std::vector<T> hx(static_cast<std::size_t>(m * ldx), kCanary), hy(static_cast<std::size_t>(n * ldyd), kCanary);
  for (std::int64_t c = 0; c < m; ++c)
    for (int j = 0; j < k; ++j) hx[static_cast<std::size_t>(c * ldx + j)] = X(c, j);
  T *dx = nullptr, *dy = nullptr;
  if (hipMalloc(&dx, hx.size() * sizeof(T)) != hipSuccess || hipMalloc(&dy, hy.size() * sizeof(T)) != hipSuccess)
    return fail("hipMalloc");
  if (hipMemcpy(dx, hx.data(), hx.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dy, hy.data(), hy.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
    return fail("hipMemcpy");
  sparse::SpMMPlan<T> moved(std::move(plan));
  sparse::spmm(moved, k, dx, ldx, dy, ldyd);
  if (hipDeviceSynchronize() != hipSuccess) return fail("spmm on device pointers");
  if (hipMemcpy(hy.data(), dy, hy.size() * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return fail("hipMemcpy");
  (void)hipFree(dx);
  (void)hipFree(dy);
  for (std::int64_t i = 0; i < n; ++i)
    for (std::int64_t j = 0; j < ldyd; ++j)
      if (hy[static_cast<std::size_t>(i * ldyd + j)] != (j < k ? Y(i, j) : kCanary)) return fail("device block");

  // errors go through lhpc::checkLhpc
  bool threw = false;
  try {
    sparse::spmm(moved, k, dx, static_cast<std::int64_t>(k - 1), dy, ldyd);
  } catch (const std::system_error &) {
    threw = true;
  }
  return threw ? 0 : fail("ldx < k did not throw");
}

}  // namespace

int main() {
  try {
    if (int st = run<float, std::int32_t>(300, 257, 5)) return st;
    if (int st = run<double, std::int64_t>(129, 200, 33)) return st;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "FAIL: exception: %s\n", e.what());
    return 1;
  }
  std::printf("spmm cpp api: ok\n");
  return 0;
}
