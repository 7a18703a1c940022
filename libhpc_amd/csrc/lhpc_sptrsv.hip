// lhpc_sptrsv.hip — level-scheduled sparse triangular solve (lhpc_sptrsv_*).
//
// The reference has no counterpart (it has no SpMV).  Operator and
// arithmetic: include/lhpc.h "CSR triangular solve"; row i's sum runs over
// its kept entries in CSR order in fp64, product rounded before the add
// (-ffp-contract=off), so every x_i is fixed bit for bit.
//
// Layout (lhpc_sptrsv_host.cpp): rows sorted by level, each level cut into
// slices of 64 rows stored column-major like k_spmv_sell's — entry e of lane l
// at off + e·64 + l, col = −1 for padding, which is skipped, never multiplied.
// Two kernels, issued in the order the plan fixed at creation:
//   k_trsv_grid   one level: a wave per slice, a lane per row.  Earlier
//                 levels' x is visible through the kernel boundary.
//   k_trsv_chain  a run of small levels in ONE 1024-thread workgroup with
//                 __syncthreads() between levels.  Its 16 waves share one CU
//                 and its L1, so the barrier's workgroup-scope release /
//                 acquire is what makes a level's x visible to the next; x
//                 has no const __restrict__ view there, so no load of it is
//                 hoisted over the barrier.
// No flag, spin or cross-workgroup wait anywhere: the only ordering between
// workgroups is the kernel boundary, which is what a solve with many large
// levels is bound by (4.5 µs per launch issued eagerly).
// x may be b: a lane reads b[row] before it writes x[row] and no other lane
// touches that row, so neither pointer is __restrict__.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include "lhpc_common.hpp"
#include "lhpc_spmv_impl.hpp"
#include "lhpc_sptrsv.hpp"

struct lhpc_sptrsv_plan {
  int dtype = LHPC_F32, device = 0, upper = 0, unit = 0;
  int64_t n = 0, nnz = 0;  // nnz: of the caller's A (set_values)
  int64_t kept = 0, n_levels = 0, max_level_rows = 0, n_slices = 0, padded = 0;
  int chain_rows = 0;
  std::vector<lhpc::TrsvStep> steps;
  int64_t *d_level_slice = nullptr;  // n_levels + 1
  int64_t *d_slice_off = nullptr;    // n_slices + 1
  int32_t *d_slice_row = nullptr;    // n_slices · 64
  int32_t *d_col = nullptr;          // padded
  // padded values, then (non-unit) n_slices · 64 diagonals in slot order; d_src
  // holds the CSR position each of them came from (kTrsvNoSource: padding 0,
  // idle lane's diagonal 1)
  void *d_val = nullptr;
  uint32_t *d_src = nullptr;
  int64_t n_val = 0;  // entries of d_val and d_src
  void *d_bstage = nullptr, *d_xstage = nullptr;  // host-buffer calls (first such call)
  int64_t bytes = 0;
};

namespace lhpc {
namespace {

constexpr int kTrsvGridThreads = 256;

// One slice: lane l solves row slice_row[s·64 + l].
template <typename T, bool UNIT>
__device__ __forceinline__ void trsv_slice(int64_t s, int lane, int64_t n, int64_t padded,
                                           const int64_t *__restrict__ slice_off,
                                           const int32_t *__restrict__ slice_row, const int32_t *__restrict__ col,
                                           const T *__restrict__ val, const T *b, T *x) {
  const int64_t off = slice_off[s];
  const int width = static_cast<int>((slice_off[s + 1] - off) / kTrsvSlice);
  const int64_t slot = s * kTrsvSlice + lane;
  const int32_t row = slice_row[slot];
  LHPC_DEVICE_CHECK(row >= -1 && row < n && off + int64_t{width} * kTrsvSlice <= padded);
  double sum = 0.0;
  const int32_t *cp = col + off + lane;
  const T *vp = val + off + lane;
  for (int e = 0; e < width; ++e) {
    const int32_t c = cp[int64_t{e} * kTrsvSlice];
    if (c >= 0) {  // padding is skipped: it never meets a non-finite x
      LHPC_DEVICE_CHECK(c < n);
      sum += static_cast<double>(vp[int64_t{e} * kTrsvSlice]) * static_cast<double>(x[c]);
    }
  }
  if (row >= 0) {
    const double r = static_cast<double>(b[row]) - sum;
    if constexpr (UNIT) x[row] = static_cast<T>(r);
    else x[row] = static_cast<T>(r / static_cast<double>(val[padded + slot]));
  }
}

// Grid step: slices [s0, s1) of one level, a wave per slice.
template <typename T, bool UNIT>
__global__ __launch_bounds__(kTrsvGridThreads) void k_trsv_grid(int64_t s0, int64_t s1, int64_t n, int64_t padded,
                                                                const int64_t *__restrict__ slice_off,
                                                                const int32_t *__restrict__ slice_row,
                                                                const int32_t *__restrict__ col,
                                                                const T *__restrict__ val, const T *b, T *x) {
  const int64_t s = s0 + static_cast<int64_t>(blockIdx.x) * (kTrsvGridThreads / kWave) + threadIdx.x / kWave;
  if (s >= s1) return;
  trsv_slice<T, UNIT>(s, static_cast<int>(threadIdx.x) & (kWave - 1), n, padded, slice_off, slice_row, col, val, b, x);
}

// Chain step: levels [l0, l1) in one workgroup; wave w takes slices w, w + 16, …
// of the level.  Every wave runs the same number of barriers (the level count).
template <typename T, bool UNIT>
__global__ __launch_bounds__(kTrsvChainThreads) void k_trsv_chain(int64_t l0, int64_t l1, int64_t n, int64_t padded,
                                                                  const int64_t *__restrict__ level_slice,
                                                                  const int64_t *__restrict__ slice_off,
                                                                  const int32_t *__restrict__ slice_row,
                                                                  const int32_t *__restrict__ col,
                                                                  const T *__restrict__ val, const T *b, T *x) {
  const int wave = static_cast<int>(threadIdx.x) / kWave, lane = static_cast<int>(threadIdx.x) & (kWave - 1);
  int64_t s_next = level_slice[l0];
  for (int64_t l = l0; l < l1; ++l) {
    const int64_t s0 = s_next;
    s_next = level_slice[l + 1];
    for (int64_t s = s0 + wave; s < s_next; s += kTrsvChainThreads / kWave)
      trsv_slice<T, UNIT>(s, lane, n, padded, slice_off, slice_row, col, val, b, x);
    __syncthreads();  // this level's x, stored by any wave, is read by the next level
  }
}

// dst[q] = val[src[q]]; a slot without a source is padding (0) below `padded`
// and an idle lane's diagonal (1) above it
template <typename T>
__global__ __launch_bounds__(kTrsvGridThreads) void k_trsv_values(const T *__restrict__ val,
                                                                  const uint32_t *__restrict__ src, int64_t n_val,
                                                                  int64_t padded, int64_t nnz, T *__restrict__ dst) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kTrsvGridThreads;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kTrsvGridThreads + threadIdx.x; q < n_val; q += stride) {
    const uint32_t p = src[q];
    LHPC_DEVICE_CHECK(p == kTrsvNoSource || static_cast<int64_t>(p) < nnz);
    dst[q] = p == kTrsvNoSource ? static_cast<T>(q < padded ? 0 : 1) : val[p];
  }
}

template <typename T, bool UNIT>
int launch_steps(const lhpc_sptrsv_plan *p, const void *b, void *x, hipStream_t s) {
  const T *val = static_cast<const T *>(p->d_val);
  for (const TrsvStep &st : p->steps) {
    if (st.chain) {
      hipLaunchKernelGGL((k_trsv_chain<T, UNIT>), dim3(1), dim3(kTrsvChainThreads), 0, s, st.level_begin, st.level_end,
                         p->n, p->padded, p->d_level_slice, p->d_slice_off, p->d_slice_row, p->d_col, val,
                         static_cast<const T *>(b), static_cast<T *>(x));
    } else {
      constexpr int per_block = kTrsvGridThreads / kWave;
      const unsigned grid = static_cast<unsigned>((st.slice_end - st.slice_begin + per_block - 1) / per_block);
      hipLaunchKernelGGL((k_trsv_grid<T, UNIT>), dim3(grid), dim3(kTrsvGridThreads), 0, s, st.slice_begin,
                         st.slice_end, p->n, p->padded, p->d_slice_off, p->d_slice_row, p->d_col, val,
                         static_cast<const T *>(b), static_cast<T *>(x));
    }
    LHPC_TRY(check_launch(s));
  }
  return LHPC_OK;
}

int launch(const lhpc_sptrsv_plan *p, const void *b, void *x, hipStream_t s) {
  if (p->dtype == LHPC_F32)
    return p->unit ? launch_steps<float, true>(p, b, x, s) : launch_steps<float, false>(p, b, x, s);
  return p->unit ? launch_steps<double, true>(p, b, x, s) : launch_steps<double, false>(p, b, x, s);
}

// the plan's values from A's (HBM, CSR order): one launch on s
int gather(const lhpc_sptrsv_plan *p, const void *val, hipStream_t s) {
  if (p->n_val == 0) return LHPC_OK;
  const unsigned grid =
      static_cast<unsigned>(std::min<int64_t>((p->n_val + kTrsvGridThreads - 1) / kTrsvGridThreads, 16384));
  if (p->dtype == LHPC_F32)
    hipLaunchKernelGGL(k_trsv_values<float>, dim3(grid), dim3(kTrsvGridThreads), 0, s,
                       static_cast<const float *>(val), p->d_src, p->n_val, p->padded, p->nnz,
                       static_cast<float *>(p->d_val));
  else
    hipLaunchKernelGGL(k_trsv_values<double>, dim3(grid), dim3(kTrsvGridThreads), 0, s,
                       static_cast<const double *>(val), p->d_src, p->n_val, p->padded, p->nnz,
                       static_cast<double *>(p->d_val));
  return check_launch(s);
}

// host values through library scratch; s has drained on return
int gather_host(const lhpc_sptrsv_plan *p, const void *val, hipStream_t s) {
  const size_t bytes = static_cast<size_t>(p->nnz) * (p->dtype == LHPC_F32 ? 4 : 8);
  void *tmp = nullptr;
  if (bytes) {
    LHPC_HIP_TRY(scratch_alloc(&tmp, bytes, s));
    const hipError_t e = hipMemcpyAsync(tmp, val, bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
      (void)hipFreeAsync(tmp, s);
      return static_cast<int>(e);
    }
  }
  const int st = gather(p, tmp, s);
  if (tmp) (void)hipFreeAsync(tmp, s);
  const hipError_t e = hipStreamSynchronize(s);
  return st != LHPC_OK ? st : static_cast<int>(e);
}

template <typename V>
int upload(V **dst, const std::vector<V> &v, int64_t &acct) {
  LHPC_TRY(dmalloc(reinterpret_cast<void **>(dst), v.size() * sizeof(V), acct));
  if (!v.empty()) LHPC_HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice));
  return LHPC_OK;
}

int plan_upload(lhpc_sptrsv_plan *p, const TrsvLayout &lay, const void *val, bool device_input) {
  p->kept = lay.kept;
  p->n_levels = lay.n_levels;
  p->max_level_rows = lay.max_level_rows;
  p->n_slices = lay.n_slices;
  p->padded = lay.padded;
  p->chain_rows = lay.chain_rows;
  p->steps = lay.steps;
  p->n_val = static_cast<int64_t>(lay.src.size());
  LHPC_TRY(upload(&p->d_level_slice, lay.level_slice, p->bytes));
  LHPC_TRY(upload(&p->d_slice_off, lay.slice_off, p->bytes));
  LHPC_TRY(upload(&p->d_slice_row, lay.slice_row, p->bytes));
  LHPC_TRY(upload(&p->d_col, lay.col, p->bytes));
  LHPC_TRY(upload(&p->d_src, lay.src, p->bytes));
  LHPC_TRY(dmalloc(&p->d_val, lay.src.size() * (p->dtype == LHPC_F32 ? 4 : 8), p->bytes));
  // the values take the route every later lhpc_sptrsv_plan_set_values takes
  if (device_input) {
    LHPC_TRY(gather(p, val, nullptr));
    LHPC_HIP_TRY(hipStreamSynchronize(nullptr));
    return LHPC_OK;
  }
  return gather_host(p, val, nullptr);
}

}  // namespace
}  // namespace lhpc

using namespace lhpc;

extern "C" int lhpc_sptrsv_plan_create(lhpc_sptrsv_plan **out, int dtype, int64_t n, int64_t nnz, const void *row_ptr,
                                       int row_ptr_bits, const int32_t *col_idx, const void *val, unsigned trsv,
                                       int chain_rows, int device, unsigned flags) {
  try {
    if (!out) return LHPC_ERR_INVALID_ARG;
    *out = nullptr;
    if ((dtype != LHPC_F32 && dtype != LHPC_F64) || n < 0 || nnz < 0 || n > INT32_MAX || !row_ptr ||
        (row_ptr_bits != 32 && row_ptr_bits != 64) || (nnz > 0 && (!col_idx || !val)) ||
        (row_ptr_bits == 32 && nnz > INT32_MAX) || device < -1 ||
        (trsv & ~static_cast<unsigned>(LHPC_TRSV_UPPER | LHPC_TRSV_UNIT_DIAG)) ||
        (flags & ~static_cast<unsigned>(LHPC_PLAN_VALIDATE | LHPC_PLAN_DEVICE_INPUT | LHPC_PLAN_TRANSPOSE)))
      return LHPC_ERR_INVALID_ARG;
    // Lᵀ: lhpc_csr_transpose, then LHPC_TRSV_UPPER; source positions are 32-bit
    if ((flags & LHPC_PLAN_TRANSPOSE) || nnz >= (int64_t{1} << 32)) return LHPC_ERR_UNSUPPORTED;
    RocTxRange rx("lhpc_sptrsv_plan_create");
    const bool device_input = (flags & LHPC_PLAN_DEVICE_INPUT) != 0;
    TrsvLayout lay;
    // host input: the analysis (and LHPC_ERR_BAD_CSR) before any device is touched
    if (!device_input) LHPC_TRY(sptrsv_layout_host(lay, n, nnz, row_ptr, row_ptr_bits, col_idx, trsv, chain_rows));
    int dev = device;
    if (dev < 0 ? hipGetDevice(&dev) != hipSuccess : hipSetDevice(dev) != hipSuccess) {
      (void)hipGetLastError();
      return LHPC_ERR_NO_DEVICE;
    }
    if (!is_gfx950(dev)) return LHPC_ERR_NO_DEVICE;
    if (device_input) {
      // the arrays may still be in flight on any stream of the caller; they
      // come to the host for the analysis
      LHPC_HIP_TRY(hipDeviceSynchronize());
      std::vector<unsigned char> hrp(static_cast<size_t>(n + 1) * (row_ptr_bits / 8));
      std::vector<int32_t> hcol(static_cast<size_t>(nnz));
      LHPC_HIP_TRY(hipMemcpy(hrp.data(), row_ptr, hrp.size(), hipMemcpyDeviceToHost));
      if (nnz) LHPC_HIP_TRY(hipMemcpy(hcol.data(), col_idx, hcol.size() * 4, hipMemcpyDeviceToHost));
      LHPC_TRY(sptrsv_layout_host(lay, n, nnz, hrp.data(), row_ptr_bits, hcol.data(), trsv, chain_rows));
    }
    auto *p = new (std::nothrow) lhpc_sptrsv_plan();
    if (!p) return LHPC_ERR_ALLOC;
    p->dtype = dtype;
    p->device = dev;
    p->upper = (trsv & LHPC_TRSV_UPPER) != 0;
    p->unit = (trsv & LHPC_TRSV_UNIT_DIAG) != 0;
    p->n = n;
    p->nnz = nnz;
    const int st = plan_upload(p, lay, val, device_input);
    if (st != LHPC_OK) {
      lhpc_sptrsv_plan_destroy(p);
      return st;
    }
    *out = p;
    return LHPC_OK;
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_sptrsv(lhpc_sptrsv_plan *p, const void *b, void *x, int buffers_on_device, void *stream) {
  try {
    if (!p || (p->n > 0 && (!b || !x))) return LHPC_ERR_INVALID_ARG;
    if (p->n == 0) return LHPC_OK;
    RocTxRange rx("lhpc_sptrsv");
    hipStream_t s = static_cast<hipStream_t>(stream);
    LHPC_HIP_TRY(hipSetDevice(p->device));
    if (buffers_on_device) return launch(p, b, x, s);
    // host buffers through plan-owned staging, which only such calls touch
    // (they end synchronised)
    const size_t bytes = static_cast<size_t>(p->n) * (p->dtype == LHPC_F32 ? 4 : 8);
    if (!p->d_bstage) LHPC_TRY(dmalloc(&p->d_bstage, bytes, p->bytes));
    if (!p->d_xstage) LHPC_TRY(dmalloc(&p->d_xstage, bytes, p->bytes));
    LHPC_HIP_TRY(hipMemcpyAsync(p->d_bstage, b, bytes, hipMemcpyHostToDevice, s));
    LHPC_TRY(launch(p, p->d_bstage, p->d_xstage, s));
    LHPC_HIP_TRY(hipStreamSynchronize(s));
    LHPC_HIP_TRY(hipMemcpy(x, p->d_xstage, bytes, hipMemcpyDeviceToHost));
    return LHPC_OK;
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_sptrsv_plan_set_values(lhpc_sptrsv_plan *p, const void *val, int64_t nnz, int values_on_device,
                                           void *stream) {
  try {
    if (!p || (nnz > 0 && !val) || nnz != p->nnz) return LHPC_ERR_INVALID_ARG;
    if (nnz == 0 || p->n == 0) return LHPC_OK;
    RocTxRange rx("lhpc_sptrsv_plan_set_values");
    hipStream_t s = static_cast<hipStream_t>(stream);
    LHPC_HIP_TRY(hipSetDevice(p->device));
    return values_on_device ? gather(p, val, s) : gather_host(p, val, s);
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_sptrsv_plan_info_get(const lhpc_sptrsv_plan *p, lhpc_sptrsv_plan_info *info) {
  try {
    if (!p || !info) return LHPC_ERR_INVALID_ARG;
    info->dtype = p->dtype;
    info->device = p->device;
    info->upper = p->upper;
    info->unit_diag = p->unit;
    info->n = p->n;
    info->nnz = p->kept;
    info->n_levels = p->n_levels;
    info->max_level_rows = p->max_level_rows;
    info->n_slices = p->n_slices;
    info->padded_entries = p->padded;
    info->chain_rows = p->chain_rows;
    info->launches = static_cast<int>(p->steps.size());
    info->device_bytes = p->bytes;
    return LHPC_OK;
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_sptrsv_plan_destroy(lhpc_sptrsv_plan *p) {
  try {
    if (!p) return LHPC_OK;
    (void)hipSetDevice(p->device);
    for (void *q : {static_cast<void *>(p->d_level_slice), static_cast<void *>(p->d_slice_off),
                    static_cast<void *>(p->d_slice_row), static_cast<void *>(p->d_col), p->d_val,
                    static_cast<void *>(p->d_src), p->d_bstage, p->d_xstage})
      if (q) (void)hipFree(q);
    delete p;
    return LHPC_OK;
  } LHPC_ABI_CATCH
}
