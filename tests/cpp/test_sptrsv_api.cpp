// test_sptrsv_api.cpp — sparse::SpTRSVPlan / sparse::sptrsv / sparse::sptrsv_levels
// (include/sparse/SpTRSV.hpp) as a drop-in user would call them.  The whole
// 5-point operator on 37 × 29 (both triangles in every row, random
// off-diagonals, diagonal 6) is solved for its lower and its upper triangle,
// with and without a unit diagonal, in fp32 and fp64, through host flat arrays
// (in place too) and through device pointers, from a host matrix and from a
// DeviceCSRView, and after set_values; every result is compared bit for bit
// with a C++ restatement of the arithmetic include/lhpc.h states (this file is
// built with -ffp-contract=off).  Built by tests/cpp/sptrsv.mk
// (tests/test_sptrsv_api.py) and run on the GPU by tests/test_gpu_sptrsv.py;
// exit status 0 = pass.
#include <hip/hip_runtime_api.h>
#include <sparse/SpTRSV.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <system_error>
#include <vector>

namespace {

int fail(const char *what) {
  std::fprintf(stderr, "FAIL: %s\n", what);
  return 1;
}

double uniform(std::uint64_t &z) {  // (−1, 1), a fixed sequence
  z = z * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<double>(z >> 11) / 4503599627370496.0 - 1.0;
}

template <typename T>
sparse::CSRMatrix<T> grid(int nx, int ny, std::uint64_t seed) {
  sparse::CSRMatrix<T> A(static_cast<std::int64_t>(nx) * ny, static_cast<std::int64_t>(nx) * ny);
  for (int iy = 0; iy < ny; ++iy)
    for (int ix = 0; ix < nx; ++ix) {
      const std::int32_t i = iy * nx + ix;
      auto put = [&](bool in, std::int32_t c, double v) {
        if (!in) return;
        A.col_idx.push_back(c);
        A.val.push_back(static_cast<T>(v));
      };
      put(iy > 0, i - nx, uniform(seed));
      put(ix > 0, i - 1, uniform(seed));
      put(true, i, 6.0);
      put(ix < nx - 1, i + 1, uniform(seed));
      put(iy < ny - 1, i + nx, uniform(seed));
      A.row_ptr[static_cast<std::size_t>(i) + 1] = static_cast<std::int32_t>(A.col_idx.size());
    }
  return A;
}

// include/lhpc.h "CSR triangular solve" on the host
template <typename T>
std::vector<T> host_solve(const sparse::CSRMatrix<T> &A, const std::vector<T> &b, unsigned trsv) {
  const bool upper = trsv & LHPC_TRSV_UPPER, unit = trsv & LHPC_TRSV_UNIT_DIAG;
  const std::int64_t n = A.n_rows;
  std::vector<T> x(static_cast<std::size_t>(n));
  for (std::int64_t k = 0; k < n; ++k) {
    const std::int64_t i = upper ? n - 1 - k : k;
    double s = 0.0, d = 1.0;
    for (auto p = A.row_ptr[static_cast<std::size_t>(i)]; p < A.row_ptr[static_cast<std::size_t>(i) + 1]; ++p) {
      const std::int32_t c = A.col_idx[static_cast<std::size_t>(p)];
      const double v = static_cast<double>(A.val[static_cast<std::size_t>(p)]);
      if (c == i) {
        if (!unit) d = v;
      } else if (upper ? c > i : c < i) {
        const double prod = v * static_cast<double>(x[static_cast<std::size_t>(c)]);
        s += prod;
      }
    }
    const double r = static_cast<double>(b[static_cast<std::size_t>(i)]) - s;
    x[static_cast<std::size_t>(i)] = static_cast<T>(unit ? r : r / d);
  }
  return x;
}

template <typename T>
struct DeviceVec {
  T *p = nullptr;
  explicit DeviceVec(const T *h, std::size_t n) {
    if (hipMalloc(reinterpret_cast<void **>(&p), std::max<std::size_t>(n, 1) * sizeof(T)) != hipSuccess ||
        hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
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

template <typename T>
bool same_bits(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

template <typename T>
int run(const char *name) {
  constexpr int nx = 37, ny = 29;
  const auto A = grid<T>(nx, ny, 0x9E3779B97F4A7C15ull);
  const std::size_t n = static_cast<std::size_t>(A.n_rows);
  std::uint64_t z = 0x1234567ull;
  std::vector<T> b(n);
  for (auto &v : b) v = static_cast<T>(uniform(z));
  auto A2 = A;  // the same structure, other values
  for (std::size_t r = 0; r < n; ++r)
    for (auto p = static_cast<std::size_t>(A2.row_ptr[r]); p < static_cast<std::size_t>(A2.row_ptr[r + 1]); ++p)
      A2.val[p] = A2.col_idx[p] == static_cast<std::int32_t>(r) ? static_cast<T>(5.0) : static_cast<T>(uniform(z));

  const std::vector<std::int32_t> lv = sparse::sptrsv_levels(A, LHPC_TRSV_LOWER);
  for (int iy = 0; iy < ny; ++iy)
    for (int ix = 0; ix < nx; ++ix)
      if (lv[static_cast<std::size_t>(iy * nx + ix)] != ix + iy) return fail("levels: not ix + iy on the natural grid");

  for (unsigned trsv : {0u, 1u, 2u, 3u}) {
    const std::vector<T> want = host_solve(A, b, trsv);
    sparse::SpTRSVPlan<T> plan(A, trsv, /*chain_rows=*/trsv == 1u ? -1 : 0);
    const lhpc_sptrsv_plan_info inf = plan.info();
    if (inf.n != A.n_rows || inf.n_levels != nx + ny - 1 || inf.max_level_rows != ny || inf.upper != int(trsv & 1u) ||
        inf.unit_diag != int((trsv >> 1) & 1u) || inf.launches != (trsv == 1u ? nx + ny - 1 : 1))
      return fail("info does not describe the plan");
    // host flat arrays, then in place
    hpc::HPCHighDimensionFlatArray<1, T> B(n), X(n);
    for (std::size_t i = 0; i < n; ++i) B(i) = b[i];
    sparse::sptrsv(plan, B, X);
    for (std::size_t i = 0; i < n; ++i)
      if (std::memcmp(&X(i), &want[i], sizeof(T)) != 0) return fail("host arrays: bits differ from the restatement");
    sparse::sptrsv(plan, B, B);
    for (std::size_t i = 0; i < n; ++i)
      if (std::memcmp(&B(i), &want[i], sizeof(T)) != 0) return fail("host arrays in place: bits differ");
    // device pointers
    DeviceVec<T> db(b.data(), n), dx(b.data(), n);
    sparse::sptrsv(plan, static_cast<const T *>(db.p), dx.p);
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    if (!same_bits(dx.host(n), want)) return fail("device pointers: bits differ from the restatement");
    // a plan from device arrays
    DeviceVec<std::int32_t> drp(A.row_ptr.data(), n + 1), dcol(A.col_idx.data(), A.col_idx.size());
    DeviceVec<T> dval(A.val.data(), A.val.size());
    sparse::DeviceCSRView<T> view;
    view.n_rows = view.n_cols = A.n_rows;
    view.nnz = A.nnz();
    view.row_ptr = drp.p;
    view.col_idx = dcol.p;
    view.val = dval.p;
    if (hipGetDevice(&view.device) != hipSuccess) return fail("hipGetDevice");
    sparse::SpTRSVPlan<T> dplan(view, trsv);
    sparse::sptrsv(dplan, static_cast<const T *>(db.p), dx.p);
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    if (!same_bits(dx.host(n), want)) return fail("DeviceCSRView plan: bits differ from the restatement");
    // new values, host then device
    const std::vector<T> want2 = host_solve(A2, b, trsv);
    plan.set_values(A2);
    sparse::sptrsv(plan, static_cast<const T *>(db.p), dx.p);
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    if (!same_bits(dx.host(n), want2)) return fail("set_values (host): bits differ from the restatement");
    DeviceVec<T> dval2(A2.val.data(), A2.val.size());
    dplan.set_values(dval2.p, A2.nnz(), /*on_device=*/true);
    sparse::sptrsv(dplan, static_cast<const T *>(db.p), dx.p);
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    if (!same_bits(dx.host(n), want2)) return fail("set_values (device): bits differ from the restatement");
    bool threw = false;
    try {
      plan.set_values(A2.val.data(), A2.nnz() - 1);
    } catch (const std::system_error &e) {
      threw = e.code().value() == LHPC_ERR_INVALID_ARG;
    }
    if (!threw) return fail("set_values with a wrong nnz did not throw LHPC_ERR_INVALID_ARG");
  }
  // a row without a diagonal entry is refused unless the diagonal is unit
  auto bad = A;
  bad.col_idx[0] = 1;  // row 0: (0, 0) becomes a second (0, 1)
  bool threw = false;
  try {
    sparse::SpTRSVPlan<T> p(bad, LHPC_TRSV_LOWER);
  } catch (const std::system_error &e) {
    threw = e.code().value() == LHPC_ERR_BAD_CSR;
  }
  if (!threw) return fail("a missing diagonal did not throw LHPC_ERR_BAD_CSR");
  std::printf("sptrsv %s %dx%d: lower/upper, unit/non-unit, host/device, set_values: bit-equal\n", name, nx, ny);
  return 0;
}

}  // namespace

int main() {
  try {
    if (int st = run<double>("fp64")) return st;
    if (int st = run<float>("fp32")) return st;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "FAIL: exception: %s\n", e.what());
    return 1;
  }
  std::printf("sptrsv cpp api: ok\n");
  return 0;
}
