// lhpc_bicgstab.hip — BiCGStab on the SpMV plan, for matrices that are not
// symmetric positive definite (convection–diffusion, Jacobians, A + σI of a
// non-normal A), where lhpc_cg_solve reports a breakdown.  It needs A·x only,
// so every kernel family, row parts and LHPC_PLAN_TRANSPOSE plans serve it.
// No reference counterpart.
//
// Per iteration (HBM-bound vector work around two SpMVs; n elements of the
// plan's dtype per vector pass):
//   v = A·p, σ = r̂·v            lhpc_spmv_dot (ADAPTIVE / SELL: the dot is the
//                               SpMV's epilogue and reads r̂; else SpMV +
//                               k_bi_dot: reads r̂ v)
//   α = ρ/σ                     k_bi_alpha (one block)
//   s = r − α·v, ss = s·s       k_bi_s (reads r v, writes s, block partials)
//   t = A·s, ts = t·s           lhpc_spmv_dot as above (w = s, the SpMV's own
//   tt = t·t                    input), then k_bi_dot (reads t); else SpMV +
//                               k_bi_ts_tt (reads t s, both dots in one pass)
//   ω = ts/tt                   k_bi_omega (one block: sums ss, tt, ts)
//   x += α·p + ω·s, r = s − ω·t k_bi_xr (reads x p s t r̂, writes x r, block
//   ρ' = r̂·r, rr = r·r          partials of both dots)
//   β = (ρ'/ρ)·(α/ω)            k_bi_rho (one block: sums ρ' and rr, tests)
//   p = r + β·(p − ω·v)         k_bi_p (reads r p v, writes p)
// ADAPTIVE / SELL: 2 SpMVs (r̂ rides the first one's epilogue: 1 pass) and
// 3 + 1 + 7 + 4 = 15 vector passes; other families: 2 SpMVs and
// 2 + 3 + 2 + 7 + 4 = 18 vector passes.  lhpc_cg_solve: 1 SpMV and 8 passes.
//
// The latch.  The three one-block kernels test for convergence and breakdown
// where σ, ω and ρ' / rr come into being and keep a state word in HBM
// (active, done, broke down) beside the iteration count and rr; every vector
// kernel reads the state first and writes nothing once it is not active, and
// the one-block kernels then leave the scalars alone.  So the iterations the
// host issues between two reads of the latch (check_every of them) change
// nothing after the solve has ended: x, the iteration count and the residual
// do not depend on check_every.  The SpMVs of those iterations still run, on
// the frozen vectors, and nothing reads what they write.
// Dots accumulate in fp64 in a fixed two-stage order (per-block strided sums,
// then one block in index order; the fused dot in the SpMV's block order):
// deterministic run to run.  No atomics; scalars are plain stores of thread 0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "lhpc_common.hpp"
#include "lhpc_spmv_impl.hpp"

namespace lhpc {
namespace {

constexpr int kVecThreads = 256;
constexpr int kDotBlocks = 1024;

// the solve's scalars (fp64 words of plan->bi_scal); the first three are the
// latch the host reads: bb, rr and the word pair {state, iterations completed}
enum : int {
  kBB = 0, kRR, kStateIt, kRho, kSigma, kTs, kAlpha, kOmega, kBeta, kStop, kFinal,
  kScalars = 16,
  kPartA = kScalars,             // ss, then ρ'
  kPartB = kPartA + kDotBlocks,  // tt, then rr
  kPartC = kPartB + kDotBlocks,  // σ / ts where the SpMV's dot is not fused; bb
  kScalWords = kPartC + kDotBlocks,
};
enum : int { kActive = 0, kDone = 1, kBroke = 2 };

__device__ __forceinline__ const int *state_of(const double *sc) { return reinterpret_cast<const int *>(sc + kStateIt); }
__device__ __forceinline__ int *state_of(double *sc) { return reinterpret_cast<int *>(sc + kStateIt); }
// finite: neither infinity nor NaN (x − x is 0 exactly then, NaN otherwise)
__device__ __forceinline__ bool is_fin(double x) { return x - x == 0.0; }

__device__ __forceinline__ double block_sum(double v, double *sh) {
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  const int w = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  __syncthreads();  // sh may still be read from the previous sum
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < kVecThreads / kWave; ++i) s += sh[i];
  return s;  // valid in thread 0
}

// Σ part[0..nb) in a fixed order by one block; valid in thread 0
__device__ __forceinline__ double part_sum(const double *__restrict__ part, int nb, double *sh) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += kVecThreads) s += part[i];
  return block_sum(s, sh);
}

// ---- vector passes: 256 threads, grid-stride, block partials in fp64

// part[b] = Σ a[i]·b[i]; FROZEN: only while the state is active
template <typename T, bool FROZEN>
__global__ __launch_bounds__(kVecThreads) void k_bi_dot(const T *__restrict__ a, const T *__restrict__ b, int64_t n,
                                                        const double *__restrict__ sc, double *__restrict__ part) {
  __shared__ double sh[kVecThreads / kWave];
  if (FROZEN && *state_of(sc) != kActive) return;
  double s = 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kVecThreads + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kVecThreads)
    s += static_cast<double>(a[i]) * static_cast<double>(b[i]);
  const double t = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// r = b − q, r̂ = r, p = r; partials of r·r
template <typename T>
__global__ __launch_bounds__(kVecThreads) void k_bi_init(const T *__restrict__ b, const T *__restrict__ q,
                                                         T *__restrict__ r, T *__restrict__ rh, T *__restrict__ p,
                                                         int64_t n, double *__restrict__ part) {
  __shared__ double sh[kVecThreads / kWave];
  double s = 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kVecThreads + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kVecThreads) {
    const T ri = b[i] - q[i];
    r[i] = ri;
    rh[i] = ri;
    p[i] = ri;
    s += static_cast<double>(ri) * static_cast<double>(ri);
  }
  const double t = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// s = r − α·v; partials of s·s
template <typename T>
__global__ __launch_bounds__(kVecThreads) void k_bi_s(const T *__restrict__ r, const T *__restrict__ v,
                                                      T *__restrict__ sv, int64_t n, const double *__restrict__ sc,
                                                      double *__restrict__ part) {
  __shared__ double sh[kVecThreads / kWave];
  if (*state_of(sc) != kActive) return;
  const T a = static_cast<T>(sc[kAlpha]);
  double s = 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kVecThreads + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kVecThreads) {
    const T si = r[i] - a * v[i];
    sv[i] = si;
    s += static_cast<double>(si) * static_cast<double>(si);
  }
  const double t = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// partials of t·s and t·t in one pass over t and s
template <typename T>
__global__ __launch_bounds__(kVecThreads) void k_bi_ts_tt(const T *__restrict__ t, const T *__restrict__ sv,
                                                          int64_t n, const double *__restrict__ sc,
                                                          double *__restrict__ part_ts, double *__restrict__ part_tt) {
  __shared__ double sh[kVecThreads / kWave];
  if (*state_of(sc) != kActive) return;
  double a = 0.0, b = 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kVecThreads + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kVecThreads) {
    const double ti = static_cast<double>(t[i]);
    a += ti * static_cast<double>(sv[i]);
    b += ti * ti;
  }
  const double ta = block_sum(a, sh);
  const double tb = block_sum(b, sh);
  if (threadIdx.x == 0) {
    part_ts[blockIdx.x] = ta;
    part_tt[blockIdx.x] = tb;
  }
}

// x += α·p + ω·s, r = s − ω·t; partials of r̂·r and r·r
template <typename T>
__global__ __launch_bounds__(kVecThreads) void k_bi_xr(T *__restrict__ x, const T *__restrict__ p,
                                                       const T *__restrict__ sv, const T *__restrict__ t,
                                                       const T *__restrict__ rh, T *__restrict__ r, int64_t n,
                                                       const double *__restrict__ sc, double *__restrict__ part_rho,
                                                       double *__restrict__ part_rr) {
  __shared__ double sh[kVecThreads / kWave];
  if (*state_of(sc) != kActive) return;
  const T a = static_cast<T>(sc[kAlpha]), w = static_cast<T>(sc[kOmega]);
  double d0 = 0.0, d1 = 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kVecThreads + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kVecThreads) {
    const T si = sv[i];
    x[i] = x[i] + (a * p[i] + w * si);
    const T ri = si - w * t[i];
    r[i] = ri;
    d0 += static_cast<double>(rh[i]) * static_cast<double>(ri);
    d1 += static_cast<double>(ri) * static_cast<double>(ri);
  }
  const double t0 = block_sum(d0, sh);
  const double t1 = block_sum(d1, sh);
  if (threadIdx.x == 0) {
    part_rho[blockIdx.x] = t0;
    part_rr[blockIdx.x] = t1;
  }
}

// p = r + β·(p − ω·v)
template <typename T>
__global__ __launch_bounds__(kVecThreads) void k_bi_p(const T *__restrict__ r, T *__restrict__ p,
                                                      const T *__restrict__ v, int64_t n,
                                                      const double *__restrict__ sc) {
  if (*state_of(sc) != kActive) return;
  const T beta = static_cast<T>(sc[kBeta]), w = static_cast<T>(sc[kOmega]);
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kVecThreads + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kVecThreads)
    p[i] = r[i] + beta * (p[i] - w * v[i]);
}

// ---- the one-block kernels: each finishes the dots of the pass before it,
// tests them and derives the next scalar.  A breakdown found here comes
// before x is written for the iteration, so the latch keeps the count and rr
// of the last completed one: only the state word changes.

// bb, rr = ρ (nb partials each, bb in kPartC, rr in kPartA), stop, the state
__global__ __launch_bounds__(kVecThreads) void k_bi_start(double *__restrict__ sc, int nb, double tol) {
  __shared__ double sh[kVecThreads / kWave];
  const double bb = part_sum(sc + kPartC, nb, sh);
  const double rr = part_sum(sc + kPartA, nb, sh);
  if (threadIdx.x != 0) return;
  const double stop = tol * tol * (bb > 0.0 ? bb : 1.0);
  sc[kBB] = bb;
  sc[kRR] = rr;
  sc[kRho] = rr;
  sc[kStop] = stop;
  int *st = state_of(sc);
  st[1] = 0;
  st[0] = !is_fin(rr) ? kBroke : rr <= stop ? kDone : kActive;
}

// σ (nb > 0: its partials in kPartC; else lhpc_spmv_dot wrote sc[kSigma]); α = ρ/σ
__global__ __launch_bounds__(kVecThreads) void k_bi_alpha(double *__restrict__ sc, int nb) {
  __shared__ double sh[kVecThreads / kWave];
  if (*state_of(sc) != kActive) return;
  const double sum = part_sum(sc + kPartC, nb, sh);
  if (threadIdx.x != 0) return;
  const double sigma = nb > 0 ? sum : sc[kSigma];
  const double alpha = sc[kRho] / sigma;
  if (!is_fin(sigma) || !is_fin(alpha) || sigma == 0.0) {
    state_of(sc)[0] = kBroke;
    return;
  }
  sc[kAlpha] = alpha;
}

// ss (kPartA), tt (kPartB), ts (nb_ts > 0: kPartC; else sc[kTs]); ω = ts/tt,
// or ω = 0 and the final step when ss ≤ stop
__global__ __launch_bounds__(kVecThreads) void k_bi_omega(double *__restrict__ sc, int nb, int nb_ts) {
  __shared__ double sh[kVecThreads / kWave];
  if (*state_of(sc) != kActive) return;
  const double ss = part_sum(sc + kPartA, nb, sh);
  const double tt = part_sum(sc + kPartB, nb, sh);
  const double sum = part_sum(sc + kPartC, nb_ts, sh);
  if (threadIdx.x != 0) return;
  if (ss <= sc[kStop]) {
    sc[kOmega] = 0.0;
    sc[kFinal] = 1.0;
    return;
  }
  const double ts = nb_ts > 0 ? sum : sc[kTs];
  const double omega = ts / tt;
  if (!is_fin(tt) || !is_fin(omega) || omega == 0.0) {
    state_of(sc)[0] = kBroke;
    return;
  }
  sc[kOmega] = omega;
  sc[kFinal] = 0.0;
}

// ρ' (kPartA), rr (kPartB): the iteration is complete — count it, latch rr,
// test it; else β = (ρ'/ρ)·(α/ω), ρ = ρ'
__global__ __launch_bounds__(kVecThreads) void k_bi_rho(double *__restrict__ sc, int nb) {
  __shared__ double sh[kVecThreads / kWave];
  if (*state_of(sc) != kActive) return;
  const double rho1 = part_sum(sc + kPartA, nb, sh);
  const double rr = part_sum(sc + kPartB, nb, sh);
  if (threadIdx.x != 0) return;
  int *st = state_of(sc);
  st[1] += 1;
  sc[kRR] = rr;
  if (!is_fin(rr)) {
    st[0] = kBroke;  // overflow: this iteration's x is written
  } else if (rr <= sc[kStop] || sc[kFinal] != 0.0) {
    st[0] = kDone;
  } else if (rho1 == 0.0) {
    st[0] = kBroke;  // the next iteration cannot be formed; this one stands
  } else {
    sc[kBeta] = (rho1 / sc[kRho]) * (sc[kAlpha] / sc[kOmega]);
    sc[kRho] = rho1;
  }
}

int vec_grid(int64_t n) {
  return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(kDotBlocks, (n + kVecThreads - 1) / kVecThreads)));
}

// everything of one solve that does not depend on the dtype
struct Solve {
  lhpc_spmv_plan *plan;
  int64_t n;
  int g;            // vector grid
  bool fused_dot;   // lhpc_spmv_dot is one pass and allocates nothing after its first call
  double *sc;
  void *r, *rh, *p, *v, *sv, *t, *x;
  hipStream_t s;
};

template <typename T>
int iteration(const Solve &w) {
  const dim3 grid(w.g), block(kVecThreads), one(1);
  double *sc = w.sc;
  T *r = static_cast<T *>(w.r), *rh = static_cast<T *>(w.rh), *p = static_cast<T *>(w.p), *v = static_cast<T *>(w.v),
    *sv = static_cast<T *>(w.sv), *t = static_cast<T *>(w.t), *x = static_cast<T *>(w.x);
  if (w.fused_dot) {
    LHPC_TRY(lhpc_spmv_dot(w.plan, p, v, rh, sc + kSigma, w.s));
  } else {
    LHPC_TRY(lhpc_spmv(w.plan, p, v, 1, w.s));
    hipLaunchKernelGGL((k_bi_dot<T, true>), grid, block, 0, w.s, rh, v, w.n, sc, sc + kPartC);
  }
  hipLaunchKernelGGL(k_bi_alpha, one, block, 0, w.s, sc, w.fused_dot ? 0 : w.g);
  hipLaunchKernelGGL((k_bi_s<T>), grid, block, 0, w.s, r, v, sv, w.n, sc, sc + kPartA);
  LHPC_TRY(check_launch(w.s));
  if (w.fused_dot) {
    LHPC_TRY(lhpc_spmv_dot(w.plan, sv, t, sv, sc + kTs, w.s));
    hipLaunchKernelGGL((k_bi_dot<T, true>), grid, block, 0, w.s, t, t, w.n, sc, sc + kPartB);
  } else {
    LHPC_TRY(lhpc_spmv(w.plan, sv, t, 1, w.s));
    hipLaunchKernelGGL((k_bi_ts_tt<T>), grid, block, 0, w.s, t, sv, w.n, sc, sc + kPartC, sc + kPartB);
  }
  hipLaunchKernelGGL(k_bi_omega, one, block, 0, w.s, sc, w.g, w.fused_dot ? 0 : w.g);
  hipLaunchKernelGGL((k_bi_xr<T>), grid, block, 0, w.s, x, p, sv, t, rh, r, w.n, sc, sc + kPartA, sc + kPartB);
  hipLaunchKernelGGL(k_bi_rho, one, block, 0, w.s, sc, w.g);
  hipLaunchKernelGGL((k_bi_p<T>), grid, block, 0, w.s, r, p, v, w.n, sc);
  return check_launch(w.s);
}

// bb, r = b − A·x, r̂ = p = r, ρ = rr, stop, the state
template <typename T>
int start(const Solve &w, const void *b, double tol) {
  const dim3 grid(w.g), block(kVecThreads), one(1);
  const T *bt = static_cast<const T *>(b);
  LHPC_TRY(lhpc_spmv(w.plan, w.x, w.v, 1, w.s));  // first: it also makes the plan's device current
  hipLaunchKernelGGL((k_bi_dot<T, false>), grid, block, 0, w.s, bt, bt, w.n, w.sc, w.sc + kPartC);
  hipLaunchKernelGGL((k_bi_init<T>), grid, block, 0, w.s, bt, static_cast<const T *>(w.v), static_cast<T *>(w.r),
                     static_cast<T *>(w.rh), static_cast<T *>(w.p), w.n, w.sc + kPartA);
  hipLaunchKernelGGL(k_bi_start, one, block, 0, w.s, w.sc, w.g, tol);
  return check_launch(w.s);
}

int solve_owned(lhpc_spmv_plan *plan, const void *b, void *x_user, double tol, int max_iter, int check_every,
                int *iters_out, double *resid_out, hipStream_t s) {
  lhpc_spmv_plan_info info{};
  LHPC_TRY(lhpc_spmv_plan_info_get(plan, &info));
  if (info.n_rows != info.n_cols) return LHPC_ERR_INVALID_ARG;
  RocTxRange rx("lhpc_bicgstab_solve");
  const int64_t n = info.n_rows;
  const bool f32 = info.dtype == LHPC_F32;
  const size_t vb = static_cast<size_t>(n) * (f32 ? 4 : 8);
  if (check_every < 1) check_every = 1;
  // the work, kept with the plan (a captured block holds its addresses):
  // r r̂ p v s t and a working x, the scalars and partials, the pinned latch
  if (!plan->bi_vecs) {  // on the plan's device, whatever the caller's current device
    int cur = 0;
    LHPC_HIP_TRY(hipGetDevice(&cur));
    LHPC_HIP_TRY(hipSetDevice(plan->device));
    hipError_t e = hipMalloc(&plan->bi_vecs, std::max<size_t>(vb, 8) * 7);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&plan->bi_scal), kScalWords * sizeof(double));
    if (e == hipSuccess)
      e = hipHostMalloc(reinterpret_cast<void **>(&plan->bi_host), 3 * sizeof(double), hipHostMallocDefault);
    (void)hipSetDevice(cur);
    LHPC_HIP_TRY(e);
  }
  char *base = static_cast<char *>(plan->bi_vecs);
  Solve w{};
  w.plan = plan;
  w.n = n;
  w.g = vec_grid(n);
  w.fused_dot = (plan->kernel == LHPC_KERNEL_ADAPTIVE || plan->kernel == LHPC_KERNEL_SELL) && !plan->multi &&
                plan->parts.empty() && plan->n_blocks > 0 && plan->n_blocks <= int64_t{2048} * 2048;
  w.sc = plan->bi_scal;
  w.r = base, w.rh = base + vb, w.p = base + 2 * vb, w.v = base + 3 * vb, w.sv = base + 4 * vb, w.t = base + 5 * vb;
  w.x = base + 6 * vb;
  w.s = s;
  // the latch as the host sees it: {bb, rr, {state, iterations}} in pinned memory
  double *h = plan->bi_host;
  const int *h_state = reinterpret_cast<const int *>(h + kStateIt);
  auto read_latch = [&]() -> int {
    LHPC_HIP_TRY(hipMemcpyAsync(h, w.sc, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    LHPC_HIP_TRY(hipStreamSynchronize(s));
    return LHPC_OK;
  };
  auto body = [&]() -> int { return f32 ? iteration<float>(w) : iteration<double>(w); };

  LHPC_HIP_TRY(hipMemcpyAsync(w.x, x_user, vb, hipMemcpyDeviceToDevice, s));
  LHPC_TRY(f32 ? start<float>(w, b, tol) : start<double>(w, b, tol));
  LHPC_TRY(read_latch());  // iteration 0: b = 0, a warm start that already solves, a non-finite residual

  // Graph blocks: the check_every iterations between two reads of the latch,
  // captured once and replayed.  Every iteration has the same form, so one
  // graph per check_every serves every block of every later solve.  Same
  // conditions as lhpc_cg_solve's.
#ifdef LHPC_DEBUG_SYNC
  bool graphs = false;
#else
  bool graphs = s != nullptr && check_every >= 4 && w.fused_dot;
#endif
  if (plan->bi_graph && plan->bi_graph_iters != check_every) {
    (void)hipGraphExecDestroy(plan->bi_graph);
    plan->bi_graph = nullptr;
  }
  auto capture = [&]() -> bool {
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
    int st = LHPC_OK;
    for (int i = 0; i < check_every && st == LHPC_OK; ++i) st = body();
    const hipError_t e = hipStreamEndCapture(s, &g);
    (void)hipGetLastError();
    const bool ok = st == LHPC_OK && e == hipSuccess && g &&
                    hipGraphInstantiate(&plan->bi_graph, g, nullptr, nullptr, 0) == hipSuccess;
    if (g) (void)hipGraphDestroy(g);
    if (!ok && plan->bi_graph) {
      (void)hipGraphExecDestroy(plan->bi_graph);
      plan->bi_graph = nullptr;
    }
    plan->bi_graph_iters = ok ? check_every : 0;
    return ok;
  };
  int it = 0;
  if (h_state[0] == kActive && max_iter > 0) {
    if (graphs && !plan->d_dpart)  // the fused dot's partials exist before any capture (state active: σ is rewritten)
      LHPC_TRY(lhpc_spmv_dot(plan, w.p, w.v, w.rh, w.sc + kSigma, s));
    while (it < max_iter) {
      if (graphs && it % check_every == 0 && it + check_every <= max_iter) {
        if (!plan->bi_graph && !capture()) {
          graphs = false;  // capture refused: the plain loop below
          continue;
        }
        LHPC_HIP_TRY(hipGraphLaunch(plan->bi_graph, s));
        it += check_every;
      } else {
        LHPC_TRY(body());
        ++it;
        if (it % check_every != 0 && it != max_iter) continue;
      }
      LHPC_TRY(read_latch());
      if (h_state[0] != kActive) break;
    }
  }
  LHPC_HIP_TRY(hipMemcpyAsync(x_user, w.x, vb, hipMemcpyDeviceToDevice, s));
  LHPC_HIP_TRY(hipStreamSynchronize(s));
  const double bb = h[kBB], rr = h[kRR];
  if (iters_out) *iters_out = h_state[1];
  if (resid_out) *resid_out = std::sqrt(std::max(rr, 0.0)) / std::sqrt(bb > 0.0 ? bb : 1.0);
  return h_state[0] == kBroke ? LHPC_ERR_INTERNAL : LHPC_OK;
}

}  // namespace
}  // namespace lhpc

using namespace lhpc;

// One solve per plan at a time, of either kind: the flag is lhpc_cg_solve's,
// released only once the solve's stream has drained (see there).
extern "C" int lhpc_bicgstab_solve(lhpc_spmv_plan *plan, const void *b, void *x, double tol, int max_iter,
                                   int check_every, int *iters_out, double *resid_out, void *stream) {
  try {
    if (!plan || !b || !x || max_iter < 0 || !(tol >= 0.0)) return LHPC_ERR_INVALID_ARG;
    int idle = 0;
    if (!plan->cg_busy.compare_exchange_strong(idle, 1)) return LHPC_ERR_BUSY;
    struct Release {  // on every exit, the exception path included
      lhpc_spmv_plan *p;
      hipStream_t s;
      ~Release() {
        (void)hipStreamSynchronize(s);
        p->cg_busy.store(0);
      }
    } release{plan, static_cast<hipStream_t>(stream)};
    return solve_owned(plan, b, x, tol, max_iter, check_every, iters_out, resid_out,
                       static_cast<hipStream_t>(stream));
  } LHPC_ABI_CATCH
}
