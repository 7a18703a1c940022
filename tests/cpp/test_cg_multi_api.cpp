// test_cg_multi_api.cpp — sparse::cg (k conjugate-gradient solves in step on
// one SpMM plan) and sparse::spmm_dot as a user of include/sparse/SpMM.hpp
// would call them: a small 2-D Laplacian, k = 3 right-hand sides in HBM with
// their own leading dimensions, the residuals recomputed on the host in
// double precision.  Built and run by tests/test_gpu_cg_multi.py; exit
// status 0 = pass.
#include <sparse/SpMM.hpp>

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <system_error>
#include <vector>

namespace {

int fail(const char *what) {
  std::fprintf(stderr, "FAIL: %s\n", what);
  return 1;
}

int run() {
  const int nx = 24, ny = 17, k = 3;
  const std::int64_t n = nx * ny, ldb = k + 2, ldx = k + 1;
  sparse::CSRMatrix<double, std::int32_t, std::int32_t> A(n, n);
  for (int y = 0; y < ny; ++y)
    for (int x = 0; x < nx; ++x) {
      const std::int64_t i = static_cast<std::int64_t>(y) * nx + x;
      auto put = [&](std::int64_t c, double v) {
        A.col_idx.push_back(static_cast<std::int32_t>(c));
        A.val.push_back(v);
      };
      if (y > 0) put(i - nx, -1.0);
      if (x > 0) put(i - 1, -1.0);
      put(i, 4.0);
      if (x < nx - 1) put(i + 1, -1.0);
      if (y < ny - 1) put(i + nx, -1.0);
      A.row_ptr[static_cast<std::size_t>(i + 1)] = static_cast<std::int32_t>(A.col_idx.size());
    }
  const double kCanary = -77.5;
  std::vector<double> hb(static_cast<std::size_t>(n * ldb), kCanary), hx(static_cast<std::size_t>(n * ldx), kCanary);
  for (std::int64_t i = 0; i < n; ++i)
    for (int j = 0; j < k; ++j) {
      hb[static_cast<std::size_t>(i * ldb + j)] = std::sin(0.37 * static_cast<double>(i + 1) * (j + 1)) + 0.25 * j;
      hx[static_cast<std::size_t>(i * ldx + j)] = 0.0;
    }
  double *db = nullptr, *dx = nullptr, *dy = nullptr, *dd = nullptr;
  if (hipMalloc(&db, hb.size() * 8) != hipSuccess || hipMalloc(&dx, hx.size() * 8) != hipSuccess ||
      hipMalloc(&dy, static_cast<std::size_t>(n * k) * 8) != hipSuccess || hipMalloc(&dd, k * 8) != hipSuccess)
    return fail("hipMalloc");
  if (hipMemcpy(db, hb.data(), hb.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dx, hx.data(), hx.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return fail("hipMemcpy");

  sparse::SpMMPlan<double> plan(A);
  const double tol = 1e-10;
  const sparse::CGMultiResult res = sparse::cg(plan, k, db, ldb, dx, ldx, tol, 2000, 2);
  if (res.iterations.size() != static_cast<std::size_t>(k) || res.residual.size() != static_cast<std::size_t>(k))
    return fail("result sizes");
  if (hipMemcpy(hx.data(), dx, hx.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail("hipMemcpy");
  for (int j = 0; j < k; ++j) {
    if (res.iterations[static_cast<std::size_t>(j)] < 2 || res.iterations[static_cast<std::size_t>(j)] % 2 != 0 ||
        !(res.residual[static_cast<std::size_t>(j)] <= tol))
      return fail("iterations / reported residual");
    double rr = 0.0, bb = 0.0;  // the true residual b − A·x on the host
    for (std::int64_t i = 0; i < n; ++i) {
      double ax = 0.0;
      for (auto e = A.row_ptr[static_cast<std::size_t>(i)]; e < A.row_ptr[static_cast<std::size_t>(i + 1)]; ++e)
        ax += A.val[static_cast<std::size_t>(e)] * hx[static_cast<std::size_t>(A.col_idx[static_cast<std::size_t>(e)] * ldx + j)];
      const double b = hb[static_cast<std::size_t>(i * ldb + j)];
      rr += (b - ax) * (b - ax);
      bb += b * b;
    }
    if (!(std::sqrt(rr) <= 1e-8 * std::sqrt(bb))) return fail("true residual");
  }
  for (std::int64_t i = 0; i < n; ++i)
    if (hx[static_cast<std::size_t>(i * ldx + k)] != kCanary) return fail("a column >= k of X was written");

  // spmm_dot: Y = A·X and dots[j] = X_j·Y_j, here b·x up to the solve's residual
  sparse::spmm_dot(plan, k, dx, ldx, dy, static_cast<std::int64_t>(k), dx, ldx, dd);
  if (hipDeviceSynchronize() != hipSuccess) return fail("spmm_dot");
  std::vector<double> hd(k), hy(static_cast<std::size_t>(n * k));
  if (hipMemcpy(hd.data(), dd, k * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(hy.data(), dy, hy.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("hipMemcpy");
  for (int j = 0; j < k; ++j) {
    double want = 0.0, mag = 0.0;
    for (std::int64_t i = 0; i < n; ++i) {
      const double t = hx[static_cast<std::size_t>(i * ldx + j)] * hy[static_cast<std::size_t>(i * k + j)];
      want += t;
      mag += std::fabs(t);
    }
    if (!(std::fabs(hd[static_cast<std::size_t>(j)] - want) <= 1e-12 * mag)) return fail("spmm_dot value");
  }

  bool threw = false;  // errors go through lhpc::checkLhpc
  try {
    sparse::cg(plan, k, db, static_cast<std::int64_t>(k - 1), dx, ldx);
  } catch (const std::system_error &) {
    threw = true;
  }
  (void)hipFree(db);
  (void)hipFree(dx);
  (void)hipFree(dy);
  (void)hipFree(dd);
  return threw ? 0 : fail("ldb < k did not throw");
}

}  // namespace

int main() {
  try {
    if (int st = run()) return st;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "FAIL: exception: %s\n", e.what());
    return 1;
  }
  std::printf("cg multi cpp api: ok\n");
  return 0;
}
