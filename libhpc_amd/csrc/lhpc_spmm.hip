// lhpc_spmm.hip — Y = A·X for gfx950 (MI355X): A an n_rows × n_cols CSR
// matrix kept as CSR in HBM, X a row-major n_cols × k block of vectors
// (element (c, j) at X[c·ldx + j]), Y row-major n_rows × k (include/lhpc.h
// "CSR SpMM").  The reference has no SpMV and no SpMM; the
// operator is Y[i, j] = Σ_{m=row_ptr[i]}^{row_ptr[i+1]-1} val[m]·X[col_idx[m], j].
//
// k_spmm_csr<T, I, P>: one 256-thread workgroup per block of the ADAPTIVE
// block table (csr_build_blocks: ≤ 2048 nonzeros and ≤ 256 rows, or one long
// row) and per panel of P columns.  The workgroup streams its block's
// col/val (and row bounds) once into LDS, coalesced and non-temporal; then
// G = 256/P lane groups walk the rows, lane j of a group owning column
// col0 + j: every lane of a group reads the same LDS entry (a broadcast) and
// one gather instruction of a group touches P·sizeof(T) contiguous bytes of
// row col_idx[m] of X — a whole 128-B line at P = 32 in fp32.
// Numerics: fp64 accumulation in registers, one rounding at the store
// (SURVEY §8c), and a summation order per element that depends on row i's
// structure only — never on k, ldx, ldy, the panel or the lane:
//   rows of ≤ 2048 nonzeros  ascending m;
//   longer rows              kLongStreams = 64 interleaved streams (stream s
//                            holds m ≡ s mod 64, each summed ascending), the
//                            64 partials then added in ascending s.
// No atomics, fixed order: results are identical run to run.
//
// k_spmm_dot<T, I, P>: the same phases, in a kernel of its own (sharing one
// body moved k_spmm_csr's fp64 instantiations past their 64 VGPRs), with
// dots[j] = Σ_i W[i, j]·Y[i, j] in the epilogue (lhpc_spmm_dot; the p·Ap of the
// multi-RHS CG), from the stored (rounded) Y in fp64; the stored Y is
// bit-identical to k_spmm_csr's.  Order
// per column, a function of A's block table and n_rows only (never of k, the
// leading dimensions, the panel or the column's position):
//   per block    64 interleaved streams, stream s = the block's local rows
//                r ≡ s (mod 64) added in ascending r (group g owns streams
//                g, g + G, …: row g + t·G goes to accumulator t mod 64/G);
//                the 64 stream sums added in ascending s.  A long-row block
//                contributes its one product.
//   per column   the block partials (plan-owned n_blocks × k fp64) added by
//                k_coldot_finish, one workgroup per column: thread t adds
//                blocks t, t + 256, … ascending, then the fixed tree of
//                block_sum — a function of n_blocks only.
// Lanes past k skip the product phase but stay until the barrier that
// precedes the reuse of LDS for the stream sums.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "lhpc_plan.hpp"
#include "lhpc_spmm_plan.hpp"
#include "lhpc_spmv_impl.hpp"

namespace lhpc {
namespace {

static_assert(kPanelThreads == kBlock, "the panel kernels are kBlock wide");
constexpr int kSpmmBlockNnz = 2048;  // csr_build_blocks' nonzeros per block
constexpr int kLongStreams = 64;     // long rows: interleaved partial sums (= 256 / the narrowest panel)
// gathers in flight per lane before the dependent adds (8: DESIGN.md §4.2;
// -DLHPC_SPMM_UNROLL=n builds the A/B variants, results are identical)
#ifndef LHPC_SPMM_UNROLL
#define LHPC_SPMM_UNROLL 8
#endif
constexpr int kSpmmUnroll = LHPC_SPMM_UNROLL;

// one row of the block in LDS times column xj of X: the nonzeros in ascending
// order, kSpmmUnroll gathers issued before the dependent adds; rounded once
template <typename T>
__device__ __forceinline__ T spmm_row(const T *lval, const int32_t *lcol, int rs, int re, const T *__restrict__ xj,
                                      int64_t ldx, int64_t n_cols) {
  double a = 0.0;
  for (int m0 = rs; m0 < re; m0 += kSpmmUnroll) {
    T v[kSpmmUnroll], x[kSpmmUnroll];
#pragma unroll
    for (int u = 0; u < kSpmmUnroll; ++u) {
      v[u] = T(0);
      x[u] = T(0);
      if (m0 + u < re) {
        const int32_t c = lcol[m0 + u];
        v[u] = lval[m0 + u];
        LHPC_DEVICE_CHECK(c >= 0 && c < n_cols);
        x[u] = xj[static_cast<int64_t>(c) * ldx];
      }
    }
#pragma unroll
    for (int u = 0; u < kSpmmUnroll; ++u)
      if (m0 + u < re) a += static_cast<double>(v[u]) * static_cast<double>(x[u]);
  }
  return static_cast<T>(a);
}

template <typename T, typename I, int P>
__global__ __launch_bounds__(kBlock) void k_spmm_csr(
    const I *__restrict__ row_ptr, const int32_t *__restrict__ col, const T *__restrict__ val,
    const T *__restrict__ X, int64_t ldx, T *__restrict__ Y, int64_t ldy, const int64_t *__restrict__ blocks,
    int64_t n_rows, int64_t n_cols, int k, int panel0) {
  static_assert(P == 4 || P == 8 || P == 16 || P == 32, "panel widths");
  constexpr int G = kBlock / P;        // lane groups per workgroup
  constexpr int NS = kLongStreams / G;  // long rows: streams per group
  static_assert(NS >= 1 && NS * G == kLongStreams, "every stream has one group");
  // the block's stream (normal blocks) or the long row's partials: never both
  constexpr size_t kStreamBytes = kSpmmBlockNnz * (sizeof(int32_t) + sizeof(T));
  constexpr size_t kPartBytes = sizeof(double) * kLongStreams * P;
  __shared__ __attribute__((aligned(16))) unsigned char smem[kStreamBytes > kPartBytes ? kStreamBytes : kPartBytes];
  __shared__ int32_t lrp[kBlock + 1];  // row bounds relative to the block's first nonzero
  T *lval = reinterpret_cast<T *>(smem);
  int32_t *lcol = reinterpret_cast<int32_t *>(smem + kSpmmBlockNnz * sizeof(T));
  double *part = reinterpret_cast<double *>(smem);

  const int tid = threadIdx.x;
  const int j = tid & (P - 1), g = tid / P;
  const int64_t r0 = blocks[2 * blockIdx.x], base = blocks[2 * blockIdx.x + 1];
  const int64_t r1 = blocks[2 * blockIdx.x + 2];
  const int64_t cnt = blocks[2 * blockIdx.x + 3] - base;
  const int nrows = static_cast<int>(r1 - r0);
  const int cj = panel0 + static_cast<int>(blockIdx.y) * P + j;  // this lane's column of X and Y
  const bool act = cj < k;
  const T *__restrict__ xj = X + cj;
  T *__restrict__ yj = Y + cj;

  if (cnt > kSpmmBlockNnz) {
    // one long row: the group of stream s adds nonzeros s, s + 64, … ascending
    double a[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) a[u] = 0.0;
    if (act) {
      for (int64_t m0 = 0; m0 < cnt; m0 += kLongStreams) {
        int32_t c[NS];
        T v[NS], x[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) {
          const int64_t m = m0 + g + u * G;
          c[u] = -1;
          v[u] = T(0);
          if (m < cnt) {
            c[u] = ld_stream(col + base + m);
            v[u] = ld_stream(val + base + m);
          }
        }
#pragma unroll
        for (int u = 0; u < NS; ++u) {
          x[u] = T(0);
          if (c[u] >= 0) {
            LHPC_DEVICE_CHECK(c[u] < n_cols);
            x[u] = xj[static_cast<int64_t>(c[u]) * ldx];
          }
        }
#pragma unroll
        for (int u = 0; u < NS; ++u)
          if (c[u] >= 0) a[u] += static_cast<double>(v[u]) * static_cast<double>(x[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < NS; ++u) part[(g + u * G) * P + j] = a[u];
    __syncthreads();
    if (g == 0 && act) {
      double t = part[j];
      for (int s = 1; s < kLongStreams; ++s) t += part[s * P + j];
      LHPC_DEVICE_CHECK(r0 < n_rows);
      yj[r0 * ldy] = static_cast<T>(t);
    }
    return;
  }

  // stream phase: the block's col/val once, coalesced; row bounds with them
  constexpr int PER = kSpmmBlockNnz / kBlock;
  {
    int32_t c[PER];
    T v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int64_t m = i * kBlock + tid;
      c[i] = 0;
      v[i] = T(0);
      if (m < cnt) {
        c[i] = ld_stream(col + base + m);
        v[i] = ld_stream(val + base + m);
      }
    }
    if (tid <= nrows) lrp[tid] = static_cast<int32_t>(static_cast<int64_t>(row_ptr[r0 + tid]) - base);
    if (tid == 0 && nrows == kBlock) lrp[kBlock] = static_cast<int32_t>(cnt);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int m = i * kBlock + tid;
      if (m < cnt) {
        lcol[m] = c[i];
        lval[m] = v[i];
      }
    }
  }
  __syncthreads();
  if (!act) return;

  // product phase: group g takes rows g, g + G, …; per row the nonzeros in
  // ascending order, kSpmmUnroll gathers issued before the dependent adds
  for (int r = g; r < nrows; r += G) {
    const int rs = lrp[r], re = lrp[r + 1];
    double a = 0.0;
    for (int m0 = rs; m0 < re; m0 += kSpmmUnroll) {
      T v[kSpmmUnroll], x[kSpmmUnroll];
#pragma unroll
      for (int u = 0; u < kSpmmUnroll; ++u) {
        v[u] = T(0);
        x[u] = T(0);
        if (m0 + u < re) {
          const int32_t c = lcol[m0 + u];
          v[u] = lval[m0 + u];
          LHPC_DEVICE_CHECK(c >= 0 && c < n_cols);
          x[u] = xj[static_cast<int64_t>(c) * ldx];
        }
      }
#pragma unroll
      for (int u = 0; u < kSpmmUnroll; ++u)
        if (m0 + u < re) a += static_cast<double>(v[u]) * static_cast<double>(x[u]);
    }
    LHPC_DEVICE_CHECK(r0 + r < n_rows);
    yj[(r0 + r) * ldy] = static_cast<T>(a);
  }
}

// k_spmm_csr with the per-column dot in its epilogue (header comment): the
// same stream and product phases — Y is stored bit-identical — as a kernel of
// its own, so that k_spmm_csr's code and register budget stay what they were.
template <typename T, typename I, int P>
__global__ __launch_bounds__(kBlock) void k_spmm_dot(
    const I *__restrict__ row_ptr, const int32_t *__restrict__ col, const T *__restrict__ val,
    const T *__restrict__ X, int64_t ldx, T *__restrict__ Y, int64_t ldy, const int64_t *__restrict__ blocks,
    int64_t n_rows, int64_t n_cols, int k, int panel0, const T *W, int64_t ldw, double *__restrict__ dpart) {
  static_assert(P == 4 || P == 8 || P == 16 || P == 32, "panel widths");
  constexpr int G = kBlock / P;        // lane groups per workgroup
  constexpr int NS = kLongStreams / G;  // long rows: streams per group
  static_assert(NS >= 1 && NS * G == kLongStreams, "every stream has one group");
  // the block's stream (normal blocks) or the long row's partials: never both
  constexpr size_t kStreamBytes = kSpmmBlockNnz * (sizeof(int32_t) + sizeof(T));
  constexpr size_t kPartBytes = sizeof(double) * kLongStreams * P;
  __shared__ __attribute__((aligned(16))) unsigned char smem[kStreamBytes > kPartBytes ? kStreamBytes : kPartBytes];
  __shared__ int32_t lrp[kBlock + 1];  // row bounds relative to the block's first nonzero
  T *lval = reinterpret_cast<T *>(smem);
  int32_t *lcol = reinterpret_cast<int32_t *>(smem + kSpmmBlockNnz * sizeof(T));
  double *part = reinterpret_cast<double *>(smem);

  const int tid = threadIdx.x;
  const int j = tid & (P - 1), g = tid / P;
  const int64_t r0 = blocks[2 * blockIdx.x], base = blocks[2 * blockIdx.x + 1];
  const int64_t r1 = blocks[2 * blockIdx.x + 2];
  const int64_t cnt = blocks[2 * blockIdx.x + 3] - base;
  const int nrows = static_cast<int>(r1 - r0);
  const int cj = panel0 + static_cast<int>(blockIdx.y) * P + j;  // this lane's column of X and Y
  const bool act = cj < k;
  const T *__restrict__ xj = X + cj;
  T *__restrict__ yj = Y + cj;

  if (cnt > kSpmmBlockNnz) {
    // one long row: the group of stream s adds nonzeros s, s + 64, … ascending
    double a[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) a[u] = 0.0;
    if (act) {
      for (int64_t m0 = 0; m0 < cnt; m0 += kLongStreams) {
        int32_t c[NS];
        T v[NS], x[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) {
          const int64_t m = m0 + g + u * G;
          c[u] = -1;
          v[u] = T(0);
          if (m < cnt) {
            c[u] = ld_stream(col + base + m);
            v[u] = ld_stream(val + base + m);
          }
        }
#pragma unroll
        for (int u = 0; u < NS; ++u) {
          x[u] = T(0);
          if (c[u] >= 0) {
            LHPC_DEVICE_CHECK(c[u] < n_cols);
            x[u] = xj[static_cast<int64_t>(c[u]) * ldx];
          }
        }
#pragma unroll
        for (int u = 0; u < NS; ++u)
          if (c[u] >= 0) a[u] += static_cast<double>(v[u]) * static_cast<double>(x[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < NS; ++u) part[(g + u * G) * P + j] = a[u];
    __syncthreads();
    if (g == 0 && act) {
      double t = part[j];
      for (int s = 1; s < kLongStreams; ++s) t += part[s * P + j];
      LHPC_DEVICE_CHECK(r0 < n_rows);
      const T y = static_cast<T>(t);
      yj[r0 * ldy] = y;
      dpart[static_cast<int64_t>(blockIdx.x) * k + cj] = static_cast<double>(W[r0 * ldw + cj]) * static_cast<double>(y);
    }
    return;
  }

  // stream phase: the block's col/val once, coalesced; row bounds with them
  constexpr int PER = kSpmmBlockNnz / kBlock;
  {
    int32_t c[PER];
    T v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int64_t m = i * kBlock + tid;
      c[i] = 0;
      v[i] = T(0);
      if (m < cnt) {
        c[i] = ld_stream(col + base + m);
        v[i] = ld_stream(val + base + m);
      }
    }
    if (tid <= nrows) lrp[tid] = static_cast<int32_t>(static_cast<int64_t>(row_ptr[r0 + tid]) - base);
    if (tid == 0 && nrows == kBlock) lrp[kBlock] = static_cast<int32_t>(cnt);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int m = i * kBlock + tid;
      if (m < cnt) {
        lcol[m] = c[i];
        lval[m] = v[i];
      }
    }
  }
  __syncthreads();
  // lanes past k stay for the barrier below; row g + t·G is of stream
  // g + (t mod NS)·G, whose sum is d[t mod NS]
  double d[NS];
#pragma unroll
  for (int u = 0; u < NS; ++u) d[u] = 0.0;
  if (act) {
    const T *__restrict__ wj = W + cj;
    int t = 0;
    for (int r = g; r < nrows; r += G, ++t) {
      const T y = spmm_row<T>(lval, lcol, lrp[r], lrp[r + 1], xj, ldx, n_cols);
      LHPC_DEVICE_CHECK(r0 + r < n_rows);
      const T w = wj[(r0 + r) * ldw];
      yj[(r0 + r) * ldy] = y;
      dot_stream_add<NS>(d, t & (NS - 1), static_cast<double>(w) * static_cast<double>(y));
    }
  }
  __syncthreads();  // every group has left lval / lcol: part takes their place
  const double bs = dot_streams_sum<P, NS>(d, part, g, j);
  if (g == 0 && act) dpart[static_cast<int64_t>(blockIdx.x) * k + cj] = bs;
}

// out[j] = Σ_b part[b·k + j] in a fixed order (one workgroup per column)
__global__ __launch_bounds__(kBlock) void k_coldot_finish(const double *__restrict__ part, int64_t nb, int k,
                                                          const int *__restrict__ mode, double *__restrict__ out) {
  __shared__ double sh[kBlock / kWave];
  const int j = blockIdx.x;
  if (mode && mode[j] == 0) return;  // the whole workgroup
  double v = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += kBlock) v += part[b * k + j];
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < kBlock / kWave; ++i) t += sh[i];
    out[j] = t;
  }
}

// W = null: k_spmm_csr; else k_spmm_dot with the plan's partials buffer
template <typename T, typename I, int P>
int launch_panel(const lhpc_spmm_plan *p, int k, const void *X, int64_t ldx, void *Y, int64_t ldy, int panel0,
                 int n_panels, const void *W, int64_t ldw, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(p->n_blocks), static_cast<unsigned>(n_panels));
  if (W)
    hipLaunchKernelGGL((k_spmm_dot<T, I, P>), grid, dim3(kBlock), 0, s, static_cast<const I *>(p->d_row_ptr), p->d_col,
                       static_cast<const T *>(p->d_val), static_cast<const T *>(X), ldx, static_cast<T *>(Y), ldy,
                       p->d_blocks, p->n_rows, p->n_cols, k, panel0, static_cast<const T *>(W), ldw,
                       static_cast<double *>(p->d_dpart));
  else
    hipLaunchKernelGGL((k_spmm_csr<T, I, P>), grid, dim3(kBlock), 0, s, static_cast<const I *>(p->d_row_ptr), p->d_col,
                       static_cast<const T *>(p->d_val), static_cast<const T *>(X), ldx, static_cast<T *>(Y), ldy,
                       p->d_blocks, p->n_rows, p->n_cols, k, panel0);
  return check_launch(s);
}

// full panels of kSpmmPanelMax columns in one launch (blockIdx.y = panel), then
// the remaining columns in a launch of the narrowest panel that holds them
template <typename T, typename I>
int launch_spmm(const lhpc_spmm_plan *p, int k, const void *X, int64_t ldx, void *Y, int64_t ldy, const void *W,
                int64_t ldw, hipStream_t s) {
  const int full = k / kSpmmPanelMax, rest = k % kSpmmPanelMax;
  if (full > 65535) return LHPC_ERR_UNSUPPORTED;  // gridDim.y
  if (full > 0) LHPC_TRY((launch_panel<T, I, kSpmmPanelMax>(p, k, X, ldx, Y, ldy, 0, full, W, ldw, s)));
  const int p0 = full * kSpmmPanelMax;
  if (rest == 0) return LHPC_OK;
  if (rest <= 4) return launch_panel<T, I, 4>(p, k, X, ldx, Y, ldy, p0, 1, W, ldw, s);
  if (rest <= 8) return launch_panel<T, I, 8>(p, k, X, ldx, Y, ldy, p0, 1, W, ldw, s);
  if (rest <= 16) return launch_panel<T, I, 16>(p, k, X, ldx, Y, ldy, p0, 1, W, ldw, s);
  return launch_panel<T, I, 32>(p, k, X, ldx, Y, ldy, p0, 1, W, ldw, s);
}

int launch(const lhpc_spmm_plan *p, int k, const void *X, int64_t ldx, void *Y, int64_t ldy, hipStream_t s,
           const void *W = nullptr, int64_t ldw = 0) {
  if (p->n_blocks == 0) return LHPC_OK;
  if (p->dtype == LHPC_F32)
    return p->rp64 ? launch_spmm<float, int64_t>(p, k, X, ldx, Y, ldy, W, ldw, s)
                   : launch_spmm<float, int32_t>(p, k, X, ldx, Y, ldy, W, ldw, s);
  return p->rp64 ? launch_spmm<double, int64_t>(p, k, X, ldx, Y, ldy, W, ldw, s)
                 : launch_spmm<double, int32_t>(p, k, X, ldx, Y, ldy, W, ldw, s);
}

// host ↔ device copy of an `rows` × k block with leading dimensions (elements)
int copy_block(void *dst, int64_t ldd, const void *src, int64_t lds, int64_t rows, int k, size_t tsz,
               hipMemcpyKind kind) {
  if (rows == 0) return LHPC_OK;
  if (ldd == k && lds == k) {
    LHPC_HIP_TRY(hipMemcpy(dst, src, static_cast<size_t>(rows) * k * tsz, kind));
  } else {
    LHPC_HIP_TRY(hipMemcpy2D(dst, static_cast<size_t>(ldd) * tsz, src, static_cast<size_t>(lds) * tsz,
                             static_cast<size_t>(k) * tsz, static_cast<size_t>(rows), kind));
  }
  return LHPC_OK;
}

}  // namespace

int spmm_grow(void **buf, size_t &have, size_t want, int64_t &acct) {
  if (want <= have && *buf) return LHPC_OK;
  if (*buf) {
    LHPC_HIP_TRY(hipFree(*buf));
    *buf = nullptr;
    acct -= static_cast<int64_t>(have);
    have = 0;
  }
  LHPC_TRY(dmalloc(buf, want, acct));
  have = std::max<size_t>(want, 16);
  return LHPC_OK;
}

int spmm_dot_reserve(lhpc_spmm_plan *p, int k) {
  return spmm_grow(&p->d_dpart, p->dpart_bytes, static_cast<size_t>(p->n_blocks) * k * sizeof(double), p->bytes);
}

int coldot_finish_launch(const double *part, int64_t n_units, int k, const int *mode, double *out, hipStream_t s) {
  hipLaunchKernelGGL(k_coldot_finish, dim3(static_cast<unsigned>(k)), dim3(kBlock), 0, s, part, n_units, k, mode, out);
  return check_launch(s);
}

namespace {

int plan_build(lhpc_spmm_plan *p, const void *row_ptr, int bits, const int32_t *col_idx, const void *val,
               bool device_input) {
  const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
  const size_t rpb = static_cast<size_t>(p->n_rows + 1) * (bits / 8);
  const size_t nnz = static_cast<size_t>(p->nnz);
  const hipMemcpyKind kind = device_input ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // row_ptr on the host, for the block table
  std::vector<unsigned char> hrp;
  const void *rp_host = row_ptr;
  if (device_input) {
    // the arrays may still be in flight on any stream of the caller
    LHPC_HIP_TRY(hipDeviceSynchronize());
    LHPC_TRY(validate_csr_device(row_ptr, bits, col_idx, p->n_rows, p->n_cols, p->nnz));
    hrp.resize(rpb);
    LHPC_HIP_TRY(hipMemcpy(hrp.data(), row_ptr, rpb, hipMemcpyDeviceToHost));
    rp_host = hrp.data();
  }
  LHPC_TRY(dmalloc(&p->d_row_ptr, rpb, p->bytes));
  LHPC_TRY(dmalloc(reinterpret_cast<void **>(&p->d_col), nnz * 4, p->bytes));
  LHPC_TRY(dmalloc(&p->d_val, nnz * tsz, p->bytes));
  LHPC_HIP_TRY(hipMemcpy(p->d_row_ptr, row_ptr, rpb, kind));
  if (nnz) {
    LHPC_HIP_TRY(hipMemcpy(p->d_col, col_idx, nnz * 4, kind));
    LHPC_HIP_TRY(hipMemcpy(p->d_val, val, nnz * tsz, kind));
  }
  const std::vector<int64_t> bp = csr_block_table(RowPtrView{rp_host, bits}, p->n_rows, p->n_blocks, p->n_long);
  if (p->n_blocks > INT32_MAX) return LHPC_ERR_UNSUPPORTED;  // gridDim.x
  LHPC_TRY(dmalloc(reinterpret_cast<void **>(&p->d_blocks), bp.size() * 8, p->bytes));
  LHPC_HIP_TRY(hipMemcpy(p->d_blocks, bp.data(), bp.size() * 8, hipMemcpyHostToDevice));
  return LHPC_OK;
}

}  // namespace
}  // namespace lhpc

using namespace lhpc;

extern "C" int lhpc_spmm_plan_create(lhpc_spmm_plan **out, int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                     const void *row_ptr, int row_ptr_bits, const int32_t *col_idx, const void *val,
                                     int device, unsigned flags) {
  try {
    if (!out) return LHPC_ERR_INVALID_ARG;
    *out = nullptr;
    if ((dtype != LHPC_F32 && dtype != LHPC_F64) || n_rows < 0 || n_cols < 0 || nnz < 0 || !row_ptr ||
        (row_ptr_bits != 32 && row_ptr_bits != 64) || n_cols > INT32_MAX || (nnz > 0 && (!col_idx || !val)) ||
        (row_ptr_bits == 32 && nnz > INT32_MAX) || device < -1)
      return LHPC_ERR_INVALID_ARG;
    // there is one kernel family and no partial sums to choose
    if (flags & ~static_cast<unsigned>(LHPC_PLAN_VALIDATE | LHPC_PLAN_DEVICE_INPUT | LHPC_PLAN_TRANSPOSE))
      return LHPC_ERR_INVALID_ARG;
    const bool transpose = (flags & LHPC_PLAN_TRANSPOSE) != 0;
    if (transpose && n_rows > INT32_MAX) return LHPC_ERR_INVALID_ARG;  // A's rows are the operator's columns
    RocTxRange rx("lhpc_spmm_plan_create");
    const bool device_input = (flags & LHPC_PLAN_DEVICE_INPUT) != 0;
    // always (LHPC_PLAN_VALIDATE is implied): the kernel indexes X by col_idx
    // (a transposed plan's A is checked on the device, lhpc_transpose.hip)
    if (!device_input && !transpose) LHPC_TRY(validate_csr(row_ptr, row_ptr_bits, col_idx, n_rows, n_cols, nnz));
    int dev = device;
    if (dev < 0 ? hipGetDevice(&dev) != hipSuccess : hipSetDevice(dev) != hipSuccess) {
      (void)hipGetLastError();
      return LHPC_ERR_NO_DEVICE;
    }
    if (!is_gfx950(dev)) return LHPC_ERR_NO_DEVICE;
    auto *p = new (std::nothrow) lhpc_spmm_plan();
    if (!p) return LHPC_ERR_ALLOC;
    p->dtype = dtype;
    p->device = dev;
    p->rp64 = row_ptr_bits == 64;
    p->n_rows = transpose ? n_cols : n_rows;
    p->n_cols = transpose ? n_rows : n_cols;
    p->nnz = nnz;
    int st;
    if (transpose) {
      // Aᵀ's arrays from the device transposition, then the device-input
      // build; the plan keeps the permutation for set_values
      TransposedCsr t;
      st = dmalloc(reinterpret_cast<void **>(&p->d_tperm), static_cast<size_t>(nnz) * 4, p->bytes);
      if (st == LHPC_OK)
        st = transpose_for_plan(t, dtype == LHPC_F32 ? 4 : 8, n_rows, n_cols, nnz, row_ptr, row_ptr_bits, col_idx, val,
                                device_input, p->d_tperm);
      if (st == LHPC_OK)
        st = plan_build(p, t.t_rp, row_ptr_bits, static_cast<const int32_t *>(t.t_col), t.t_val, true);
    } else {
      st = plan_build(p, row_ptr, row_ptr_bits, col_idx, val, device_input);
    }
    if (st != LHPC_OK) {
      lhpc_spmm_plan_destroy(p);
      return st;
    }
    *out = p;
    return LHPC_OK;
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmm(lhpc_spmm_plan *p, int k, const void *X, int64_t ldx, void *Y, int64_t ldy, int on_device,
                         void *stream) {
  try {
    // sizes first, the plan is read after them
    if (!p || k < 1 || ldx < k || ldy < k) return LHPC_ERR_INVALID_ARG;
    if ((p->n_cols > 0 && !X) || (p->n_rows > 0 && !Y)) return LHPC_ERR_INVALID_ARG;
    RocTxRange rx("lhpc_spmm");
    hipStream_t s = static_cast<hipStream_t>(stream);
    LHPC_HIP_TRY(hipSetDevice(p->device));
    if (on_device) return launch(p, k, X, ldx, Y, ldy, s);
    // host buffers: synchronous strided copies through packed plan-owned
    // buffers, which only host-buffer calls touch (they end synchronised)
    const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
    LHPC_TRY(spmm_grow(&p->d_xstage, p->xstage_bytes, static_cast<size_t>(p->n_cols) * k * tsz, p->bytes));
    LHPC_TRY(spmm_grow(&p->d_ystage, p->ystage_bytes, static_cast<size_t>(p->n_rows) * k * tsz, p->bytes));
    LHPC_TRY(copy_block(p->d_xstage, k, X, ldx, p->n_cols, k, tsz, hipMemcpyHostToDevice));
    LHPC_TRY(launch(p, k, p->d_xstage, k, p->d_ystage, k, s));
    LHPC_HIP_TRY(hipStreamSynchronize(s));
    return copy_block(Y, ldy, p->d_ystage, k, p->n_rows, k, tsz, hipMemcpyDeviceToHost);
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmm_dot(lhpc_spmm_plan *p, int k, const void *X, int64_t ldx, void *Y, int64_t ldy,
                             const void *W, int64_t ldw, double *dots, void *stream) {
  try {
    // sizes first, the plan is read after them
    if (!p || k < 1 || ldx < k || ldy < k || ldw < k) return LHPC_ERR_INVALID_ARG;
    if (!X || !Y || !W || !dots) return LHPC_ERR_INVALID_ARG;
    RocTxRange rx("lhpc_spmm_dot");
    hipStream_t s = static_cast<hipStream_t>(stream);
    LHPC_HIP_TRY(hipSetDevice(p->device));
    LHPC_TRY(spmm_dot_reserve(p, k));  // allocates only when k outgrows the buffer
    LHPC_TRY(launch(p, k, X, ldx, Y, ldy, s, W, ldw));
    return coldot_finish_launch(static_cast<const double *>(p->d_dpart), p->n_blocks, k, nullptr, dots, s);
  } LHPC_ABI_CATCH
}

// the plan's val is the caller's in CSR order: one copy, nothing re-encoded
extern "C" int lhpc_spmm_plan_set_values(lhpc_spmm_plan *p, const void *val, int64_t nnz, int values_on_device,
                                         void *stream) {
  try {
    if (!p || (nnz > 0 && !val) || nnz != p->nnz) return LHPC_ERR_INVALID_ARG;
    if (p->cg_busy.load()) return LHPC_ERR_BUSY;
    if (nnz == 0 || p->n_rows == 0) return LHPC_OK;
    RocTxRange rx("lhpc_spmm_plan_set_values");
    hipStream_t s = static_cast<hipStream_t>(stream);
    LHPC_HIP_TRY(hipSetDevice(p->device));
    const size_t bytes = static_cast<size_t>(nnz) * (p->dtype == LHPC_F32 ? 4 : 8);
    if (p->d_tperm) {
      // LHPC_PLAN_TRANSPOSE: val is in A's CSR order; through the plan's
      // permutation into the staging buffer (allocated by the first update),
      // then the one copy of every SpMM plan
      if (!p->d_tval) {
        LHPC_TRY(dmalloc(&p->d_tval, bytes, p->bytes));
        LHPC_HIP_TRY(hipStreamSynchronize(s));
      }
      const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
      if (values_on_device) {
        LHPC_TRY(gather_values(p->d_tval, val, p->d_tperm, nnz, tsz, s));
        LHPC_HIP_TRY(hipMemcpyAsync(p->d_val, p->d_tval, bytes, hipMemcpyDeviceToDevice, s));
        return LHPC_OK;
      }
      void *tmp = nullptr;  // stream-ordered library scratch, freed before return
      LHPC_HIP_TRY(scratch_alloc(&tmp, bytes, s));
      hipError_t e = hipMemcpyAsync(tmp, val, bytes, hipMemcpyHostToDevice, s);
      int st = e == hipSuccess ? gather_values(p->d_tval, tmp, p->d_tperm, nnz, tsz, s) : static_cast<int>(e);
      if (st == LHPC_OK) st = static_cast<int>(hipMemcpyAsync(p->d_val, p->d_tval, bytes, hipMemcpyDeviceToDevice, s));
      (void)hipFreeAsync(tmp, s);
      e = hipStreamSynchronize(s);
      return st != LHPC_OK ? st : static_cast<int>(e);
    }
    LHPC_HIP_TRY(hipMemcpyAsync(p->d_val, val, bytes,
                                values_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    if (!values_on_device) LHPC_HIP_TRY(hipStreamSynchronize(s));
    return LHPC_OK;
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmm_plan_info_get(const lhpc_spmm_plan *p, lhpc_spmm_plan_info *info) {
  try {
    if (!p || !info) return LHPC_ERR_INVALID_ARG;
    info->dtype = p->dtype;
    info->device = p->device;
    info->n_rows = p->n_rows;
    info->n_cols = p->n_cols;
    info->nnz = p->nnz;
    info->n_blocks = p->n_blocks;
    info->n_long_rows = p->n_long;
    info->device_bytes = p->bytes;
    info->panel_max = kSpmmPanelMax;
    return LHPC_OK;
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmm_plan_destroy(lhpc_spmm_plan *p) {
  try {
    if (!p) return LHPC_OK;
    (void)hipSetDevice(p->device);
    for (void *q : {p->d_row_ptr, static_cast<void *>(p->d_col), p->d_val, static_cast<void *>(p->d_blocks),
                    p->d_xstage, p->d_ystage, p->d_dpart, p->cg_vecs, p->cg_scal, static_cast<void *>(p->d_tperm),
                    p->d_tval})
      if (q) (void)hipFree(q);
    if (p->cg_host) (void)hipHostFree(p->cg_host);
    delete p;
    return LHPC_OK;
  } LHPC_ABI_CATCH
}
