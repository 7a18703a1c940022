// test_bicgstab_api.cpp — sparse::bicgstab (include/sparse/SpMV.hpp) as a
// drop-in user would call it.  The 64 × 48 upwind convection–diffusion
// operator (not symmetric) is solved in fp64 at tol 1e-10 and held to the
// bounds of tests/test_gpu_bicgstab.py: reported residual ≤ tol, true residual
// (host fp64) ≤ 2·tol, ‖x − x*‖ ≤ 1e-8·‖x*‖ against a banded LU (the matrix is
// strictly diagonally dominant: no pivoting), iterations ≤ 2 × those of a host
// restatement of the recurrence.  fp32: 32 × 32 at tol 1e-5.  Then the
// breakdown: [[0, 1], [−1, 0]], b = (1, 1), x0 = (0.25, −0.5) has r̂·v = 0
// exactly — the C call returns LHPC_ERR_INTERNAL at 0 iterations with a finite
// residual and x0 untouched, and the wrapper throws.  Built by
// tests/cpp/bicgstab.mk (tests/test_bicgstab_api.py) and run on the GPU by
// tests/test_gpu_bicgstab.py; exit status 0 = pass.
#include <hip/hip_runtime_api.h>
#include <sparse/SpMV.hpp>

#include <cmath>
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

template <typename T>
sparse::CSRMatrix<T> convdiff(int nx, int ny, double shift) {
  sparse::CSRMatrix<T> A(static_cast<std::int64_t>(nx) * ny, static_cast<std::int64_t>(nx) * ny);
  for (int iy = 0; iy < ny; ++iy)
    for (int ix = 0; ix < nx; ++ix) {
      const std::int32_t i = iy * nx + ix;
      auto put = [&](bool in, std::int32_t c, double v) {
        if (!in) return;
        A.col_idx.push_back(c);
        A.val.push_back(static_cast<T>(v));
      };
      put(iy > 0, i - nx, -1.25);
      put(ix > 0, i - 1, -1.5);
      put(true, i, 4.0 + shift);
      put(ix < nx - 1, i + 1, -0.5);
      put(iy < ny - 1, i + nx, -0.75);
      A.row_ptr[static_cast<std::size_t>(i) + 1] = static_cast<std::int32_t>(A.col_idx.size());
    }
  return A;
}

template <typename T>
std::vector<double> matvec(const sparse::CSRMatrix<T> &A, const std::vector<double> &x) {
  std::vector<double> y(static_cast<std::size_t>(A.n_rows), 0.0);
  for (std::int64_t r = 0; r < A.n_rows; ++r)
    for (auto k = A.row_ptr[static_cast<std::size_t>(r)]; k < A.row_ptr[static_cast<std::size_t>(r) + 1]; ++k)
      y[static_cast<std::size_t>(r)] += static_cast<double>(A.val[static_cast<std::size_t>(k)]) *
                                        x[static_cast<std::size_t>(A.col_idx[static_cast<std::size_t>(k)])];
  return y;
}

double dot(const std::vector<double> &a, const std::vector<double> &b) {
  double s = 0.0;
  for (std::size_t i = 0; i < a.size(); ++i) s += a[i] * b[i];
  return s;
}

// banded LU without pivoting, half bandwidth bw
std::vector<double> direct_solve(const sparse::CSRMatrix<double> &A, int bw, std::vector<double> b) {
  const std::int64_t n = A.n_rows, w = 2 * bw + 1;
  std::vector<double> band(static_cast<std::size_t>(n * w), 0.0);  // band[r·w + (c − r + bw)]
  for (std::int64_t r = 0; r < n; ++r)
    for (auto k = A.row_ptr[static_cast<std::size_t>(r)]; k < A.row_ptr[static_cast<std::size_t>(r) + 1]; ++k)
      band[static_cast<std::size_t>(r * w + A.col_idx[static_cast<std::size_t>(k)] - r + bw)] =
          A.val[static_cast<std::size_t>(k)];
  auto at = [&](std::int64_t r, std::int64_t c) -> double & { return band[static_cast<std::size_t>(r * w + c - r + bw)]; };
  for (std::int64_t k = 0; k < n; ++k)
    for (std::int64_t r = k + 1; r < n && r <= k + bw; ++r) {
      const double m = at(r, k) / at(k, k);
      if (m == 0.0) continue;
      for (std::int64_t c = k + 1; c < n && c <= k + bw; ++c) at(r, c) -= m * at(k, c);
      b[static_cast<std::size_t>(r)] -= m * b[static_cast<std::size_t>(k)];
    }
  for (std::int64_t r = n - 1; r >= 0; --r) {
    double s = b[static_cast<std::size_t>(r)];
    for (std::int64_t c = r + 1; c < n && c <= r + bw; ++c) s -= at(r, c) * b[static_cast<std::size_t>(c)];
    b[static_cast<std::size_t>(r)] = s / at(r, r);
  }
  return b;
}

// the recurrence of include/lhpc.h on the host in fp64, from x = 0: its iteration count
int host_iterations(const sparse::CSRMatrix<double> &A, const std::vector<double> &b, double tol, int max_iter) {
  const std::size_t n = b.size();
  std::vector<double> x(n, 0.0), r = b, rh = b, p = b, s(n);
  const double bb = dot(b, b), stop = tol * tol * (bb > 0 ? bb : 1.0);
  double rho = dot(r, r);
  if (rho <= stop) return 0;
  for (int it = 1; it <= max_iter; ++it) {
    const std::vector<double> v = matvec(A, p);
    const double alpha = rho / dot(rh, v);
    for (std::size_t i = 0; i < n; ++i) s[i] = r[i] - alpha * v[i];
    const std::vector<double> t = matvec(A, s);
    const bool final_step = dot(s, s) <= stop;
    const double omega = final_step ? 0.0 : dot(t, s) / dot(t, t);
    for (std::size_t i = 0; i < n; ++i) {
      x[i] += alpha * p[i] + omega * s[i];
      r[i] = s[i] - omega * t[i];
    }
    const double rho1 = dot(rh, r);
    if (dot(r, r) <= stop || final_step) return it;
    const double beta = (rho1 / rho) * (alpha / omega);
    for (std::size_t i = 0; i < n; ++i) p[i] = r[i] + beta * (p[i] - omega * v[i]);
    rho = rho1;
  }
  return max_iter;
}

template <typename T>
struct DeviceVec {
  T *p = nullptr;
  explicit DeviceVec(const std::vector<T> &h) {
    if (hipMalloc(reinterpret_cast<void **>(&p), h.size() * sizeof(T)) != hipSuccess ||
        hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("hipMalloc / hipMemcpy");
  }
  DeviceVec(const DeviceVec &) = delete;
  DeviceVec &operator=(const DeviceVec &) = delete;
  ~DeviceVec() { (void)hipFree(p); }
  std::vector<T> host(std::size_t n) const {
    std::vector<T> h(n);
    if (hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy");
    return h;
  }
};

std::vector<double> rhs(std::size_t n) {  // uniform in (−1, 1), a fixed sequence
  std::vector<double> b(n);
  std::uint64_t z = 0x9E3779B97F4A7C15ull;
  for (auto &v : b) {
    z = z * 6364136223846793005ull + 1442695040888963407ull;
    v = static_cast<double>(z >> 11) / 4503599627370496.0 - 1.0;
  }
  return b;
}

int run_f64() {
  constexpr int nx = 64, ny = 48;
  constexpr double tol = 1e-10;
  const auto A = convdiff<double>(nx, ny, 0.5);
  const std::size_t n = static_cast<std::size_t>(A.n_rows);
  const std::vector<double> b = rhs(n), want = direct_solve(A, nx, b);
  const int it_host = host_iterations(A, b, tol, 5000);
  if (it_host < 1 || it_host >= 5000) return fail("fp64: the host restatement did not converge");
  sparse::SpMVPlan<double> plan(A);
  DeviceVec<double> db(b), dx(std::vector<double>(n, 0.0));
  const auto [it, res] = sparse::bicgstab(plan, db.p, dx.p, tol, 5000, 7, nullptr);
  const std::vector<double> x = dx.host(n), ax = matvec(A, x);
  double rr = 0.0, ee = 0.0;
  for (std::size_t i = 0; i < n; ++i) {
    rr += (b[i] - ax[i]) * (b[i] - ax[i]);
    ee += (x[i] - want[i]) * (x[i] - want[i]);
  }
  const double true_res = std::sqrt(rr / dot(b, b)), err = std::sqrt(ee / dot(want, want));
  std::printf("bicgstab fp64 %dx%d: iters %d (host %d) resid %.3e true %.3e error %.3e\n", nx, ny, it, it_host, res,
              true_res, err);
  if (!(res <= tol)) return fail("fp64: reported residual above tol");
  if (!(true_res <= 2 * tol)) return fail("fp64: true residual above 2·tol");
  if (!(err <= 1e-8)) return fail("fp64: error against the direct solve above 1e-8");
  if (it < 1 || it > 2 * it_host) return fail("fp64: iterations above twice the host restatement's");
  return 0;
}

int run_f32() {
  const auto A = convdiff<float>(32, 32, 0.5);
  const std::size_t n = static_cast<std::size_t>(A.n_rows);
  const std::vector<double> bd = rhs(n);
  const std::vector<float> b(bd.begin(), bd.end());
  sparse::SpMVPlan<float> plan(A);
  DeviceVec<float> db(b), dx(std::vector<float>(n, 0.0f));
  const auto [it, res] = sparse::bicgstab(plan, db.p, dx.p, 1e-5, 5000, 5);
  std::printf("bicgstab fp32 32x32: iters %d resid %.3e\n", it, res);
  if (!(res <= 1e-5) || it < 1) return fail("fp32: not converged to 1e-5");
  return 0;
}

int run_breakdown() {
  sparse::CSRMatrix<double> A(2, 2);
  A.col_idx = {1, 0};
  A.val = {1.0, -1.0};
  A.row_ptr = {0, 1, 2};
  const std::vector<double> b = {1.0, 1.0}, x0 = {0.25, -0.5};
  sparse::SpMVPlan<double> plan(A);
  DeviceVec<double> db(b), dx(x0);
  int it = -1;
  double res = -1.0;
  const int st = lhpc_bicgstab_solve(plan.native(), db.p, dx.p, 1e-10, 100, 10, &it, &res, nullptr);
  std::printf("bicgstab breakdown: status %d iters %d resid %.3e\n", st, it, res);
  if (st != LHPC_ERR_INTERNAL) return fail("breakdown: status is not LHPC_ERR_INTERNAL");
  if (it != 0) return fail("breakdown: iters != 0");
  if (!std::isfinite(res) || !(res > 0.0)) return fail("breakdown: residual not finite");
  const std::vector<double> x = dx.host(2);
  if (std::memcmp(x.data(), x0.data(), 2 * sizeof(double)) != 0) return fail("breakdown: x is not x0 bit for bit");
  bool threw = false;
  try {
    (void)sparse::bicgstab(plan, db.p, dx.p);
  } catch (const std::system_error &e) {
    threw = e.code().value() == LHPC_ERR_INTERNAL;
  }
  if (!threw) return fail("breakdown: sparse::bicgstab did not throw LHPC_ERR_INTERNAL");
  return 0;
}

}  // namespace

int main() {
  try {
    if (int st = run_f64()) return st;
    if (int st = run_f32()) return st;
    if (int st = run_breakdown()) return st;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "FAIL: exception: %s\n", e.what());
    return 1;
  }
  std::printf("bicgstab cpp api: ok\n");
  return 0;
}
