// lhpc_solver_multi.hip — k conjugate-gradient recurrences in step on one SpMM
// plan (lhpc_cg_solve_multi): k right-hand sides share one stream of A per
// iteration instead of k.  This is not block CG (no k × k solves): column j
// goes through exactly the operations of a one-column solve of B_j.  No
// reference counterpart.
//
// B, X and the work R, P, Q are row-major n × k blocks (R, P, Q packed at
// ld = k, kept with the plan).  Per iteration:
//   Q = A·P, pq_j = P_j·Q_j                  lhpc_spmm_dot (dot in the SpMM epilogue)
//   α_j = rr_j/pq_j; R_j −= α_j·Q_j;         k_cgm_r (reads R Q, writes R, tile partials)
//   rr'_j = R_j·R_j                          + the per-column finish
//   β_j = rr'_j/rr_j; X_j += α_j·P_j;        k_cgm_xp (reads X P R, writes X P)
//   P_j = R_j + β_j·P_j
// α and β are fp64 quotients of per-column device scalars, cast to T; element
// arithmetic is in T without contraction — the arithmetic of lhpc_cg_solve.
// Every column has a mode on the device — 0 frozen (nothing of X_j, R_j, P_j
// is written), 1 x only (X_j += α_j·P_j, the converged column's last step),
// 2 full update — which the host changes only at a convergence check, the
// only host synchronisations and host → device copies of the loop.
//
// Kernels k_cgm_*<T, P>: one 256-thread workgroup per tile of kCgTileRows
// rows and per panel of P columns, G = 256/P lane groups, lane j of a group
// owning column panel0 + blockIdx.y·P + j (the mapping of k_spmm_csr): a lane
// group touches P·sizeof(T) contiguous bytes of a row, a wave 64/P rows.
// Dots: fp64, per tile in 64 interleaved streams (stream s = the tile's local
// rows r ≡ s mod 64, ascending), the stream sums added in ascending s, the
// tiles added per column by coldot_finish_launch — an order that depends on n
// only, never on k, the leading dimensions, the panel or the column's
// position.  With lhpc_spmm's contract that makes X_j, iters_out[j] and
// resid_out[j] bit-identical for every k, ldb, ldx and j, and run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "lhpc_spmm_plan.hpp"

namespace lhpc {
namespace {

constexpr int kCgTileRows = 256;  // rows of one dot tile: fixes the summation order, never tuned per call
constexpr int kModeFrozen = 0, kModeXOnly = 1, kModeFull = 2;

template <int P>
struct PanelGeom {
  static_assert(P == 4 || P == 8 || P == 16 || P == 32, "panel widths");
  static constexpr int G = kPanelThreads / P;   // lane groups
  static constexpr int NS = kDotStreams / G;    // streams (and rows in flight) per group
  static constexpr int STEPS = kCgTileRows / (G * NS);  // row batches of a tile
  static_assert(STEPS * G * NS == kCgTileRows && kCgTileRows % kDotStreams == 0, "whole batches, whole streams");
};

// R = B − Q, P = R; tile partials of B_j·B_j (part_bb) and R_j·R_j (part_rr)
template <typename T, int P>
__global__ __launch_bounds__(kPanelThreads) void k_cgm_init(const T *__restrict__ B, int64_t ldb,
                                                            const T *__restrict__ Q, T *__restrict__ R,
                                                            T *__restrict__ Pv, int64_t n, int k, int panel0,
                                                            double *__restrict__ part_bb,
                                                            double *__restrict__ part_rr) {
  using Gm = PanelGeom<P>;
  constexpr int G = Gm::G, NS = Gm::NS;
  __shared__ double lpart[kDotStreams * P];
  const int tid = threadIdx.x, j = tid & (P - 1), g = tid / P;
  const int cj = panel0 + static_cast<int>(blockIdx.y) * P + j;
  const bool act = cj < k;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kCgTileRows;
  const int nrows = static_cast<int>(n - row0 < kCgTileRows ? n - row0 : kCgTileRows);
  double dbb[NS], drr[NS];
#pragma unroll
  for (int u = 0; u < NS; ++u) dbb[u] = drr[u] = 0.0;
  if (act) {
    for (int st = 0; st < Gm::STEPS; ++st) {
      T bv[NS], qv[NS];
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        const int lr = g + (st * NS + u) * G;
        bv[u] = qv[u] = T(0);
        if (lr < nrows) {
          LHPC_DEVICE_CHECK(row0 + lr < n);
          bv[u] = B[(row0 + lr) * ldb + cj];
          qv[u] = Q[(row0 + lr) * k + cj];
        }
      }
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        const int lr = g + (st * NS + u) * G;
        if (lr < nrows) {
          const T ri = bv[u] - qv[u];
          R[(row0 + lr) * k + cj] = ri;
          Pv[(row0 + lr) * k + cj] = ri;
          dbb[u] += static_cast<double>(bv[u]) * static_cast<double>(bv[u]);
          drr[u] += static_cast<double>(ri) * static_cast<double>(ri);
        }
      }
    }
  }
  const double tbb = dot_streams_sum<P, NS>(dbb, lpart, g, j);
  __syncthreads();  // group 0 has read the first set of stream sums
  const double trr = dot_streams_sum<P, NS>(drr, lpart, g, j);
  if (g == 0 && act) {
    part_bb[static_cast<int64_t>(blockIdx.x) * k + cj] = tbb;
    part_rr[static_cast<int64_t>(blockIdx.x) * k + cj] = trr;
  }
}

// columns that are not frozen: α = num/den; R −= α·Q; tile partials of R·R
template <typename T, int P>
__global__ __launch_bounds__(kPanelThreads) void k_cgm_r(T *__restrict__ R, const T *__restrict__ Q, int64_t n, int k,
                                                         int panel0, const double *__restrict__ num,
                                                         const double *__restrict__ den,
                                                         const int *__restrict__ mode, double *__restrict__ part) {
  using Gm = PanelGeom<P>;
  constexpr int G = Gm::G, NS = Gm::NS;
  __shared__ double lpart[kDotStreams * P];
  const int tid = threadIdx.x, j = tid & (P - 1), g = tid / P;
  const int cj = panel0 + static_cast<int>(blockIdx.y) * P + j;
  const bool on = cj < k && mode[cj] != kModeFrozen;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kCgTileRows;
  const int nrows = static_cast<int>(n - row0 < kCgTileRows ? n - row0 : kCgTileRows);
  double d[NS];
#pragma unroll
  for (int u = 0; u < NS; ++u) d[u] = 0.0;
  if (on) {
    const T a = static_cast<T>(num[cj] / den[cj]);
    for (int st = 0; st < Gm::STEPS; ++st) {
      T rv[NS], qv[NS];
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        const int lr = g + (st * NS + u) * G;
        rv[u] = qv[u] = T(0);
        if (lr < nrows) {
          LHPC_DEVICE_CHECK(row0 + lr < n);
          rv[u] = R[(row0 + lr) * k + cj];
          qv[u] = Q[(row0 + lr) * k + cj];
        }
      }
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        const int lr = g + (st * NS + u) * G;
        if (lr < nrows) {
          const T ri = rv[u] - a * qv[u];
          R[(row0 + lr) * k + cj] = ri;
          d[u] += static_cast<double>(ri) * static_cast<double>(ri);
        }
      }
    }
  }
  const double t = dot_streams_sum<P, NS>(d, lpart, g, j);
  if (g == 0 && on) part[static_cast<int64_t>(blockIdx.x) * k + cj] = t;
}

// mode 2: α = anum/aden, β = bnum/anum; X += α·P, P = R + β·P.  mode 1: X += α·P.
template <typename T, int P>
__global__ __launch_bounds__(kPanelThreads) void k_cgm_xp(T *__restrict__ X, int64_t ldx, T *__restrict__ Pv,
                                                          const T *__restrict__ R, int64_t n, int k, int panel0,
                                                          const double *__restrict__ anum,
                                                          const double *__restrict__ aden,
                                                          const double *__restrict__ bnum,
                                                          const int *__restrict__ mode) {
  using Gm = PanelGeom<P>;
  constexpr int G = Gm::G, NS = Gm::NS;
  const int tid = threadIdx.x, j = tid & (P - 1), g = tid / P;
  const int cj = panel0 + static_cast<int>(blockIdx.y) * P + j;
  const int m = cj < k ? mode[cj] : kModeFrozen;
  if (m == kModeFrozen) return;  // no barrier below
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kCgTileRows;
  const int nrows = static_cast<int>(n - row0 < kCgTileRows ? n - row0 : kCgTileRows);
  const bool full = m == kModeFull;
  const T a = static_cast<T>(anum[cj] / aden[cj]);
  const T beta = full ? static_cast<T>(bnum[cj] / anum[cj]) : T(0);
  for (int st = 0; st < Gm::STEPS; ++st) {
    T xv[NS], pv[NS], rv[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int lr = g + (st * NS + u) * G;
      xv[u] = pv[u] = rv[u] = T(0);
      if (lr < nrows) {
        LHPC_DEVICE_CHECK(row0 + lr < n);
        xv[u] = X[(row0 + lr) * ldx + cj];
        pv[u] = Pv[(row0 + lr) * k + cj];
        if (full) rv[u] = R[(row0 + lr) * k + cj];
      }
    }
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int lr = g + (st * NS + u) * G;
      if (lr < nrows) {
        X[(row0 + lr) * ldx + cj] = xv[u] + a * pv[u];
        if (full) Pv[(row0 + lr) * k + cj] = rv[u] + beta * pv[u];
      }
    }
  }
}

// full panels of kSpmmPanelMax columns in one launch (blockIdx.y = panel), the
// remaining columns in a launch of the narrowest panel that holds them — the
// panels of lhpc_spmm.  `go(width tag, panel0, n_panels)` launches one of them.
template <typename F>
int for_panels(int k, F &&go) {
  const int full = k / kSpmmPanelMax, rest = k % kSpmmPanelMax;
  if (full > 65535) return LHPC_ERR_UNSUPPORTED;  // gridDim.y
  if (full > 0) go(std::integral_constant<int, kSpmmPanelMax>{}, 0, full);
  const int p0 = full * kSpmmPanelMax;
  if (rest == 0) return LHPC_OK;
  if (rest <= 4) go(std::integral_constant<int, 4>{}, p0, 1);
  else if (rest <= 8) go(std::integral_constant<int, 8>{}, p0, 1);
  else if (rest <= 16) go(std::integral_constant<int, 16>{}, p0, 1);
  else go(std::integral_constant<int, 32>{}, p0, 1);
  return LHPC_OK;
}

struct Work {
  int64_t n = 0, n_tiles = 0;
  int k = 0;
  void *R = nullptr, *P = nullptr, *Q = nullptr;
  double *bb = nullptr, *rr[2] = {nullptr, nullptr}, *pq = nullptr, *part = nullptr;
  int *mode = nullptr;
};

template <typename T>
int init_launch(const Work &w, const void *B, int64_t ldb, hipStream_t s) {
  if (w.n_tiles == 0) return LHPC_OK;
  LHPC_TRY(for_panels(w.k, [&](auto pw, int p0, int np) {
    hipLaunchKernelGGL((k_cgm_init<T, decltype(pw)::value>), dim3(static_cast<unsigned>(w.n_tiles), np),
                       dim3(kPanelThreads), 0, s, static_cast<const T *>(B), ldb, static_cast<const T *>(w.Q),
                       static_cast<T *>(w.R), static_cast<T *>(w.P), w.n, w.k, p0, w.part,
                       w.part + w.n_tiles * w.k);
  }));
  return check_launch(s);
}

template <typename T>
int r_launch(const Work &w, int c, hipStream_t s) {
  if (w.n_tiles > 0) {
    LHPC_TRY(for_panels(w.k, [&](auto pw, int p0, int np) {
      hipLaunchKernelGGL((k_cgm_r<T, decltype(pw)::value>), dim3(static_cast<unsigned>(w.n_tiles), np),
                         dim3(kPanelThreads), 0, s, static_cast<T *>(w.R), static_cast<const T *>(w.Q), w.n, w.k, p0,
                         w.rr[c], w.pq, w.mode, w.part);
    }));
    LHPC_TRY(check_launch(s));
  }
  return coldot_finish_launch(w.part, w.n_tiles, w.k, w.mode, w.rr[c ^ 1], s);
}

template <typename T>
int xp_launch(const Work &w, int c, void *X, int64_t ldx, hipStream_t s) {
  if (w.n_tiles == 0) return LHPC_OK;
  LHPC_TRY(for_panels(w.k, [&](auto pw, int p0, int np) {
    hipLaunchKernelGGL((k_cgm_xp<T, decltype(pw)::value>), dim3(static_cast<unsigned>(w.n_tiles), np),
                       dim3(kPanelThreads), 0, s, static_cast<T *>(X), ldx, static_cast<T *>(w.P),
                       static_cast<const T *>(w.R), w.n, w.k, p0, w.rr[c], w.pq, w.rr[c ^ 1], w.mode);
  }));
  return check_launch(s);
}

int cg_multi_owned(lhpc_spmm_plan *p, int k, const void *B, int64_t ldb, void *X, int64_t ldx, double tol,
                   int max_iter, int check_every, int *iters_out, double *resid_out, hipStream_t s) {
  RocTxRange rx("lhpc_cg_solve_multi");
  const bool f32 = p->dtype == LHPC_F32;
  const size_t ts = f32 ? 4 : 8;
  if (check_every < 1) check_every = 1;
  LHPC_HIP_TRY(hipSetDevice(p->device));
  Work w;
  w.n = p->n_rows;
  w.k = k;
  w.n_tiles = (w.n + kCgTileRows - 1) / kCgTileRows;
  if (w.n_tiles > INT32_MAX) return LHPC_ERR_UNSUPPORTED;  // gridDim.x
  const size_t ku = static_cast<size_t>(k), blk = static_cast<size_t>(w.n) * ku * ts;
  // plan-owned work, grown with k (the previous solve has drained its stream):
  // R P Q | bb rr0 rr1 pq, modes, 2 sets of tile partials | pinned rr bb modeA modeB
  LHPC_TRY(spmm_grow(&p->cg_vecs, p->cg_vecs_bytes, 3 * blk, p->bytes));
  LHPC_TRY(spmm_grow(&p->cg_scal, p->cg_scal_bytes,
                     (5 * ku + 2 * static_cast<size_t>(w.n_tiles) * ku) * sizeof(double), p->bytes));
  LHPC_TRY(spmm_dot_reserve(p, k));
  if (p->cg_host_bytes < 4 * ku * sizeof(double)) {
    if (p->cg_host) LHPC_HIP_TRY(hipHostFree(p->cg_host));
    p->cg_host = nullptr;
    p->cg_host_bytes = 0;
    LHPC_HIP_TRY(hipHostMalloc(&p->cg_host, 4 * ku * sizeof(double), hipHostMallocDefault));
    p->cg_host_bytes = 4 * ku * sizeof(double);
  }
  char *vb = static_cast<char *>(p->cg_vecs);
  w.R = vb;
  w.P = vb + blk;
  w.Q = vb + 2 * blk;
  double *sc = static_cast<double *>(p->cg_scal);
  w.bb = sc;
  w.rr[0] = sc + ku;
  w.rr[1] = sc + 2 * ku;
  w.pq = sc + 3 * ku;
  w.mode = reinterpret_cast<int *>(sc + 4 * ku);
  w.part = sc + 5 * ku;
  double *h_rr = static_cast<double *>(p->cg_host), *h_bb = h_rr + ku;
  int *h_mode_a = reinterpret_cast<int *>(h_rr + 2 * ku), *h_mode_b = reinterpret_cast<int *>(h_rr + 3 * ku);

  // bb = B·B; Q = A·X; R = B − Q; P = R; rr = R·R
  LHPC_TRY(lhpc_spmm(p, k, X, ldx, w.Q, k, 1, s));
  LHPC_TRY(f32 ? init_launch<float>(w, B, ldb, s) : init_launch<double>(w, B, ldb, s));
  LHPC_TRY(coldot_finish_launch(w.part, w.n_tiles, k, nullptr, w.bb, s));
  LHPC_TRY(coldot_finish_launch(w.part + w.n_tiles * k, w.n_tiles, k, nullptr, w.rr[0], s));
  LHPC_HIP_TRY(hipMemcpyAsync(h_bb, w.bb, ku * sizeof(double), hipMemcpyDeviceToHost, s));  // pinned
  LHPC_HIP_TRY(hipMemcpyAsync(h_rr, w.rr[0], ku * sizeof(double), hipMemcpyDeviceToHost, s));
  LHPC_HIP_TRY(hipStreamSynchronize(s));

  std::vector<double> stop(ku), rr_end(ku);
  std::vector<int> iters(ku, 0), mode(ku, kModeFull);
  int status = LHPC_OK, n_active = 0;
  for (int j = 0; j < k; ++j) {
    stop[j] = tol * tol * (h_bb[j] > 0.0 ? h_bb[j] : 1.0);
    rr_end[j] = h_rr[j];
    if (!std::isfinite(h_rr[j])) {
      status = LHPC_ERR_INTERNAL;  // a non-finite B or X: nothing to iterate on
      mode[j] = kModeFrozen;
    } else if (h_rr[j] <= stop[j]) {
      mode[j] = kModeFrozen;  // done at 0 iterations
    }
    n_active += mode[j] != kModeFrozen;
  }
  // both pinned mode arrays are written before the copies that read them are
  // enqueued, and not again before the next check's synchronisation
  auto upload = [&](int *h) -> int {
    LHPC_HIP_TRY(hipMemcpyAsync(w.mode, h, ku * sizeof(int), hipMemcpyHostToDevice, s));
    return LHPC_OK;
  };
  std::copy(mode.begin(), mode.end(), h_mode_a);
  LHPC_TRY(upload(h_mode_a));

  int cur = 0;
  for (int it = 1; it <= max_iter && n_active > 0; ++it, cur ^= 1) {
    LHPC_TRY(lhpc_spmm_dot(p, k, w.P, k, w.Q, k, w.P, k, w.pq, s));
    LHPC_TRY(f32 ? r_launch<float>(w, cur, s) : r_launch<double>(w, cur, s));
    bool x_only = false;
    if (it % check_every == 0 || it == max_iter) {
      LHPC_HIP_TRY(hipMemcpyAsync(h_rr, w.rr[cur ^ 1], ku * sizeof(double), hipMemcpyDeviceToHost, s));
      LHPC_HIP_TRY(hipStreamSynchronize(s));
      bool changed = false;
      for (int j = 0; j < k; ++j) {
        if (mode[j] == kModeFrozen) continue;
        rr_end[j] = h_rr[j];
        iters[j] = it;
        if (!std::isfinite(h_rr[j])) {
          status = LHPC_ERR_INTERNAL;  // breakdown (p·Ap = 0 or overflow): matrix not SPD?
          mode[j] = kModeFrozen;       // X_j is not updated
        } else if (h_rr[j] <= stop[j]) {
          mode[j] = kModeXOnly;  // X_j += α_j·P_j below, then frozen
          x_only = true;
        } else {
          continue;
        }
        changed = true;
        --n_active;
      }
      if (changed) {
        for (int j = 0; j < k; ++j) {
          h_mode_a[j] = mode[j];
          if (mode[j] == kModeXOnly) mode[j] = kModeFrozen;
          h_mode_b[j] = mode[j];
        }
        LHPC_TRY(upload(h_mode_a));
      }
    }
    LHPC_TRY(f32 ? xp_launch<float>(w, cur, X, ldx, s) : xp_launch<double>(w, cur, X, ldx, s));
    if (x_only) LHPC_TRY(upload(h_mode_b));
  }
  LHPC_HIP_TRY(hipStreamSynchronize(s));
  for (int j = 0; j < k; ++j) {
    if (iters_out) iters_out[j] = iters[j];
    if (resid_out)
      resid_out[j] = std::isfinite(rr_end[j])
                         ? std::sqrt(std::max(rr_end[j], 0.0)) / std::sqrt(h_bb[j] > 0.0 ? h_bb[j] : 1.0)
                         : rr_end[j];
  }
  return status;
}

}  // namespace
}  // namespace lhpc

using namespace lhpc;

// One solve per plan at a time, as lhpc_cg_solve: the work belongs to the
// plan, and the flag is released only once the solve's stream has drained (an
// error return after the first enqueue leaves kernels in flight that use it).
extern "C" int lhpc_cg_solve_multi(lhpc_spmm_plan *plan, int k, const void *B, int64_t ldb, void *X, int64_t ldx,
                                   double tol, int max_iter, int check_every, int *iters_out, double *resid_out,
                                   void *stream) {
  try {
    // sizes first, the plan is read after them
    if (!plan || k < 1 || ldb < k || ldx < k || max_iter < 0 || !(tol >= 0.0)) return LHPC_ERR_INVALID_ARG;
    if (!B || !X) return LHPC_ERR_INVALID_ARG;
    if (plan->n_rows != plan->n_cols) return LHPC_ERR_INVALID_ARG;  // CG needs a square (SPD) matrix
    int idle = 0;
    if (!plan->cg_busy.compare_exchange_strong(idle, 1)) return LHPC_ERR_BUSY;
    struct Release {  // on every exit, the exception path included
      lhpc_spmm_plan *p;
      hipStream_t s;
      ~Release() {
        (void)hipStreamSynchronize(s);  // a no-op wait on the success path (already drained)
        p->cg_busy.store(0);
      }
    } release{plan, static_cast<hipStream_t>(stream)};
    return cg_multi_owned(plan, k, B, ldb, X, ldx, tol, max_iter, check_every, iters_out, resid_out,
                          static_cast<hipStream_t>(stream));
  } LHPC_ABI_CATCH
}
