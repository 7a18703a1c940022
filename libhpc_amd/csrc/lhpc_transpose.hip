// lhpc_transpose.hip — CSR transposition on the GPU (lhpc_csr_transpose) and
// the value gather of transposed plans (LHPC_PLAN_TRANSPOSE).
//
// The reference has no counterpart (it has no SpMV).  Aᵀ is
// defined by a stable sort of A's entry positions by column index:
//   perm       = argsort(col_idx, stable)
//   t_col[q]   = row of entry perm[q]        t_val[q] = val[perm[q]]
//   t_row_ptr[c] = #{p : col_idx[p] < c}
// so every output is fixed bit for bit (include/lhpc.h).
//
// Three steps on the caller's stream, N = nnz (DESIGN.md §4 "Transposed plans"):
//  1. k_tr_keys      col_idx → sort keys, positions 0 … N−1 → sort payload, and
//                    the row of every entry → rowidx (reads 4N, writes 12N)
//  2. the project's stable 32-bit pair sort over the bits_for(n_cols) low bits
//     (lhpc_sort.hpp: 20N bytes per 8-bit pass)
//  3. k_tr_finish    one pass over the sorted (key, position) stream: gathers
//                    rowidx and val through the position, and writes
//                    t_row_ptr at the key boundaries (reads 8N + two gathers,
//                    writes 4N + N values)
// Row of an entry: rowidx is expanded once in position order in step 1, where
// a block's 1024 consecutive positions lie in a short window of row_ptr that
// two searches bound and the L1 holds, and gathered through perm in step 3
// beside val (one 4-byte gather per entry, the access val needs anyway).
// Searching row_ptr per sorted entry instead would save rowidx's 4N written
// and the gather, and pay log2(n_rows) dependent loads per entry at random
// places of an (n_rows + 1)-word array: for 10M rows the ~8 last levels miss
// the L2, 8 sectors per entry against one.
// No float atomics, no spin-waits, no inter-workgroup hand-off.
// Measured (one MI355X, C2 fp32, 150M entries, profiles/r12): 11.6 ms, of
// which k_tr_finish 6.25 ms (its two gathers through perm, not its streams),
// k_tr_keys 1.43 ms, the three sort passes 2.33 ms; DESIGN.md §4.5 has the
// comparison with the COO → CSR route and what would move it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "lhpc_common.hpp"
#include "lhpc_sort.hpp"
#include "lhpc_spmv_impl.hpp"

namespace lhpc {
namespace {

constexpr int kTrThreads = 256;
constexpr int kTrE = 4;  // consecutive entries per thread (one 16-B vector of 4-B words)
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int64_t rp_at(const void *rp, int bits, int64_t i) {
  return bits == 64 ? static_cast<const int64_t *>(rp)[i] : static_cast<const int32_t *>(rp)[i];
}

// the last row r in [lo, hi] with row_ptr[r] ≤ p (row_ptr[lo] ≤ p is given):
// the row that holds position p, whatever empty rows precede it
__device__ __forceinline__ int64_t row_of(const void *rp, int bits, int64_t lo, int64_t hi, int64_t p) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (rp_at(rp, bits, mid) <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Step 1.  Thread t of the grid takes positions [4t, 4t + 4).  The block's
// positions lie in rows [r_lo, r_hi], found by two searches of the whole
// row_ptr; every entry then searches that window only (indices stay inside
// [0, n_rows − 1] whatever row_ptr holds).
// VEC (col_idx and pos 16-B aligned; keys and rowidx are library scratch):
// 16-B loads and stores, as k_coo_keys (lhpc_sort.hip).
template <bool VEC>
__global__ __launch_bounds__(kTrThreads) void k_tr_keys(const void *__restrict__ rp, int bits, int64_t n_rows,
                                                        const int32_t *__restrict__ col, int64_t nnz,
                                                        uint32_t *__restrict__ keys, uint32_t *__restrict__ pos,
                                                        int32_t *__restrict__ rowidx) {
  __shared__ int64_t win[2];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * (kTrThreads * kTrE);
  const int64_t b1 = std::min<int64_t>(nnz, b0 + kTrThreads * kTrE) - 1;  // the block's last position (b0 < nnz)
  if (threadIdx.x < 2) win[threadIdx.x] = row_of(rp, bits, 0, n_rows - 1, threadIdx.x == 0 ? b0 : b1);
  __syncthreads();
  const int64_t r_hi = win[1];
  const int64_t i = b0 + static_cast<int64_t>(threadIdx.x) * kTrE;
  if (i >= nnz) return;
  int64_t r = win[0];
  if (VEC && i + kTrE <= nnz) {
    const i32x4 c = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(col + i));
    i32x4 rr;
#pragma unroll
    for (int e = 0; e < kTrE; ++e) {
      r = row_of(rp, bits, r, r_hi, i + e);
      rr[e] = static_cast<int32_t>(r);
    }
    *reinterpret_cast<i32x4 *>(keys + i) = c;
    *reinterpret_cast<u32x4 *>(pos + i) = u32x4{static_cast<uint32_t>(i), static_cast<uint32_t>(i + 1),
                                                static_cast<uint32_t>(i + 2), static_cast<uint32_t>(i + 3)};
    *reinterpret_cast<i32x4 *>(rowidx + i) = rr;
  } else {
    for (int64_t j = i; j < std::min<int64_t>(nnz, i + kTrE); ++j) {
      r = row_of(rp, bits, r, r_hi, j);
      keys[j] = static_cast<uint32_t>(col[j]);
      pos[j] = static_cast<uint32_t>(j);
      rowidx[j] = static_cast<int32_t>(r);
    }
  }
}

// Step 3.  Thread t takes sorted positions q ∈ [4t, 4t + 4) of the N + 1
// positions 0 … N, where position N stands for a closing entry of key n_cols.
// A position whose key differs from its predecessor's (key −1 in front of
// position 0) starts its column: t_row_ptr[key] = q, and the empty columns
// between the two keys start there too — those are filled by the whole wave,
// one gap at a time, so a long run of empty columns costs gap / 64 steps.
// Every key is < n_cols (A was validated), so the stores stay inside
// t_row_ptr's n_cols + 1 words; perm is a permutation of 0 … N−1 (the sort
// moves what step 1 wrote), so the gathers stay inside rowidx and val.
// VEC: perm, t_col and t_val 16-B aligned (keys is library scratch).
template <typename V, typename O, bool VEC>
__global__ __launch_bounds__(kTrThreads) void k_tr_finish(const uint32_t *__restrict__ keys,
                                                          const uint32_t *__restrict__ perm,
                                                          const int32_t *__restrict__ rowidx,
                                                          const V *__restrict__ val, int64_t nnz, int64_t n_cols,
                                                          int32_t *__restrict__ t_col, V *__restrict__ t_val,
                                                          O *__restrict__ t_rp) {
  const int lane = static_cast<int>(threadIdx.x) & (kWave - 1);
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * kTrThreads + threadIdx.x) * kTrE;
  int64_t key[kTrE];
  int64_t prev = -1;  // the key in front of position i
  if (i > 0 && i <= nnz) prev = keys[i - 1];
  if (VEC && i + kTrE <= nnz) {
    const u32x4 k = *reinterpret_cast<const u32x4 *>(keys + i);
    const u32x4 p = *reinterpret_cast<const u32x4 *>(perm + i);
    i32x4 rr;
    V vv[kTrE];
#pragma unroll
    for (int e = 0; e < kTrE; ++e) {
      key[e] = k[e];
      rr[e] = rowidx[p[e]];
      if (val) vv[e] = val[p[e]];
    }
    *reinterpret_cast<i32x4 *>(t_col + i) = rr;
    if (val) {
      if constexpr (sizeof(V) == 4) {
        *reinterpret_cast<f32x4 *>(t_val + i) = f32x4{vv[0], vv[1], vv[2], vv[3]};
      } else {
        *reinterpret_cast<f64x2 *>(t_val + i) = f64x2{vv[0], vv[1]};
        *reinterpret_cast<f64x2 *>(t_val + i + 2) = f64x2{vv[2], vv[3]};
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < kTrE; ++e) {
      const int64_t q = i + e;
      key[e] = n_cols;  // position N closes the last column; positions past it repeat it (no boundary)
      if (q < nnz) {
        key[e] = keys[q];
        const uint32_t p = perm[q];
        t_col[q] = rowidx[p];
        if (val) t_val[q] = val[p];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < kTrE; ++e) {
    const int64_t q = i + e;
    const bool head = q <= nnz && key[e] != prev;
    if (head) t_rp[key[e]] = static_cast<O>(q);
    // the empty columns (prev, key) in front of it
    uint64_t m = __ballot(head && key[e] - prev > 1);
    while (m) {
      const int l = __ffsll(static_cast<unsigned long long>(m)) - 1;
      m &= m - 1;
      const int64_t c0 = __shfl(prev, l, kWave), c1 = __shfl(key[e], l, kWave);
      const O start = static_cast<O>(__shfl(q, l, kWave));
      for (int64_t c = c0 + 1 + lane; c < c1; c += kWave) t_rp[c] = start;
    }
    prev = key[e];
  }
}

// dst[q] = src[perm[q]]: a transposed plan's new values, given in A's CSR
// order, into the order of Aᵀ's entries
template <typename V>
__global__ __launch_bounds__(kTrThreads) void k_tr_gather(const V *__restrict__ src, const uint32_t *__restrict__ perm,
                                                          int64_t n, V *__restrict__ dst) {
  const int64_t T = static_cast<int64_t>(gridDim.x) * kTrThreads;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kTrThreads + threadIdx.x; q < n; q += T) dst[q] = src[perm[q]];
}

bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15u) == 0;
}

template <typename V, typename O>
void launch_finish(const uint32_t *keys, const uint32_t *perm, const int32_t *rowidx, const void *val, int64_t nnz,
                   int64_t n_cols, int32_t *t_col, void *t_val, void *t_rp, hipStream_t s) {
  // positions 0 … nnz, four per thread
  const unsigned grid = static_cast<unsigned>((nnz + 1 + kTrThreads * kTrE - 1) / (kTrThreads * kTrE));
  if (aligned16(perm, t_col, t_val))
    hipLaunchKernelGGL((k_tr_finish<V, O, true>), dim3(grid), dim3(kTrThreads), 0, s, keys, perm, rowidx,
                       static_cast<const V *>(val), nnz, n_cols, t_col, static_cast<V *>(t_val), static_cast<O *>(t_rp));
  else
    hipLaunchKernelGGL((k_tr_finish<V, O, false>), dim3(grid), dim3(kTrThreads), 0, s, keys, perm, rowidx,
                       static_cast<const V *>(val), nnz, n_cols, t_col, static_cast<V *>(t_val), static_cast<O *>(t_rp));
}

}  // namespace

int gather_values(void *dst, const void *src, const uint32_t *perm, int64_t n, size_t tsz, hipStream_t s) {
  if (n <= 0) return LHPC_OK;
  const unsigned grid = static_cast<unsigned>(std::min<int64_t>((n + kTrThreads - 1) / kTrThreads, 16384));
  if (tsz == 4)
    hipLaunchKernelGGL(k_tr_gather<float>, dim3(grid), dim3(kTrThreads), 0, s, static_cast<const float *>(src), perm, n,
                       static_cast<float *>(dst));
  else
    hipLaunchKernelGGL(k_tr_gather<double>, dim3(grid), dim3(kTrThreads), 0, s, static_cast<const double *>(src), perm,
                       n, static_cast<double *>(dst));
  return check_launch(s);
}

int csr_transpose_dev(size_t tsz, int64_t n_rows, int64_t n_cols, int64_t nnz, const void *row_ptr, int bits,
                      const int32_t *col_idx, const void *val, void *t_row_ptr, int32_t *t_col_idx, void *t_val,
                      uint32_t *perm, hipStream_t s) {
  // the arrays may still be in flight on s; the check runs on the null stream
  LHPC_HIP_TRY(hipStreamSynchronize(s));
  LHPC_TRY(validate_csr_device(row_ptr, bits, col_idx, n_rows, n_cols, nnz));
  if (nnz == 0) {
    LHPC_HIP_TRY(hipMemsetAsync(t_row_ptr, 0, static_cast<size_t>(n_cols + 1) * (bits / 8), s));
    LHPC_HIP_TRY(hipStreamSynchronize(s));
    return LHPC_OK;
  }
  {
    DevBuf keys, rowidx, pos;  // released on s before the closing synchronisation
    LHPC_HIP_TRY(keys.alloc(static_cast<size_t>(nnz) * 4, s));
    LHPC_HIP_TRY(rowidx.alloc(static_cast<size_t>(nnz) * 4, s));
    if (!perm) {
      LHPC_HIP_TRY(pos.alloc(static_cast<size_t>(nnz) * 4, s));
      perm = static_cast<uint32_t *>(pos.p);
    }
    uint32_t *kp = static_cast<uint32_t *>(keys.p);
    int32_t *rip = static_cast<int32_t *>(rowidx.p);
    const unsigned grid = static_cast<unsigned>((nnz + kTrThreads * kTrE - 1) / (kTrThreads * kTrE));
    if (aligned16(col_idx, perm))
      hipLaunchKernelGGL(k_tr_keys<true>, dim3(grid), dim3(kTrThreads), 0, s, row_ptr, bits, n_rows, col_idx, nnz, kp,
                         perm, rip);
    else
      hipLaunchKernelGGL(k_tr_keys<false>, dim3(grid), dim3(kTrThreads), 0, s, row_ptr, bits, n_rows, col_idx, nnz, kp,
                         perm, rip);
    LHPC_TRY(check_launch(s));
    // the position order inside a column comes from the sort's stability
    LHPC_TRY(sort_pairs_u32_dev(kp, perm, nnz, 0, bits_for(n_cols), s));
    if (!val) tsz = 4;  // pattern only: the value type is not read
    if (tsz == 4) {
      if (bits == 64) launch_finish<float, int64_t>(kp, perm, rip, val, nnz, n_cols, t_col_idx, t_val, t_row_ptr, s);
      else launch_finish<float, int32_t>(kp, perm, rip, val, nnz, n_cols, t_col_idx, t_val, t_row_ptr, s);
    } else {
      if (bits == 64) launch_finish<double, int64_t>(kp, perm, rip, val, nnz, n_cols, t_col_idx, t_val, t_row_ptr, s);
      else launch_finish<double, int32_t>(kp, perm, rip, val, nnz, n_cols, t_col_idx, t_val, t_row_ptr, s);
    }
    LHPC_TRY(check_launch(s));
  }
  LHPC_HIP_TRY(hipStreamSynchronize(s));
  return LHPC_OK;
}

int transpose_for_plan(TransposedCsr &t, size_t tsz, int64_t n_rows, int64_t n_cols, int64_t nnz, const void *row_ptr,
                       int bits, const int32_t *col_idx, const void *val, bool device_input, uint32_t *perm) {
  RocTxRange rx("plan create: transpose");
  const size_t n = static_cast<size_t>(nnz), rpb = static_cast<size_t>(n_rows + 1) * (bits / 8);
  auto dalloc = [](void **p, size_t bytes) -> int {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e == hipErrorOutOfMemory) return LHPC_ERR_ALLOC;
    return static_cast<int>(e);
  };
  if (device_input) {
    // the arrays may still be in flight on any stream of the caller
    LHPC_HIP_TRY(hipDeviceSynchronize());
  } else {
    LHPC_TRY(dalloc(&t.up_rp, rpb));
    LHPC_TRY(dalloc(&t.up_col, n * 4));
    LHPC_TRY(dalloc(&t.up_val, n * tsz));
    LHPC_HIP_TRY(hipMemcpy(t.up_rp, row_ptr, rpb, hipMemcpyHostToDevice));
    if (n) {
      LHPC_HIP_TRY(hipMemcpy(t.up_col, col_idx, n * 4, hipMemcpyHostToDevice));
      LHPC_HIP_TRY(hipMemcpy(t.up_val, val, n * tsz, hipMemcpyHostToDevice));
    }
    row_ptr = t.up_rp;
    col_idx = static_cast<const int32_t *>(t.up_col);
    val = t.up_val;
  }
  LHPC_TRY(dalloc(&t.t_rp, static_cast<size_t>(n_cols + 1) * (bits / 8)));
  LHPC_TRY(dalloc(&t.t_col, n * 4));
  LHPC_TRY(dalloc(&t.t_val, n * tsz));
  LHPC_TRY(csr_transpose_dev(tsz, n_rows, n_cols, nnz, row_ptr, bits, col_idx, val, t.t_rp,
                             static_cast<int32_t *>(t.t_col), t.t_val, perm, nullptr));
  t.free_input();  // the layout build needs the room more than A's copy
  return LHPC_OK;
}

}  // namespace lhpc

using namespace lhpc;

extern "C" int lhpc_csr_transpose(int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void *row_ptr,
                                  int row_ptr_bits, const int32_t *col_idx, const void *val, void *t_row_ptr,
                                  int32_t *t_col_idx, void *t_val, uint32_t *perm, int on_device, void *stream) {
  try {
    if ((dtype != LHPC_F32 && dtype != LHPC_F64) || (row_ptr_bits != 32 && row_ptr_bits != 64) || n_rows < 0 ||
        n_cols < 0 || nnz < 0 || n_rows > INT32_MAX || n_cols > INT32_MAX || !row_ptr || !t_row_ptr ||
        (nnz > 0 && (!col_idx || !t_col_idx)) || (val == nullptr) != (t_val == nullptr) ||
        (row_ptr_bits == 32 && nnz > INT32_MAX))
      return LHPC_ERR_INVALID_ARG;
    if (nnz >= (int64_t{1} << 32)) return LHPC_ERR_UNSUPPORTED;  // the sort's 32-bit ranks and positions
    RocTxRange rx("lhpc_csr_transpose");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t tsz = dtype == LHPC_F32 ? 4 : 8;
    if (on_device)
      return csr_transpose_dev(tsz, n_rows, n_cols, nnz, row_ptr, row_ptr_bits, col_idx, val, t_row_ptr, t_col_idx,
                               t_val, perm, s);
    const size_t ob = row_ptr_bits / 8, n = static_cast<size_t>(nnz);
    const size_t rpb = static_cast<size_t>(n_rows + 1) * ob, trpb = static_cast<size_t>(n_cols + 1) * ob;
    HostStage drp, dc, dv, dtrp, dtc, dtv, dpm;
    LHPC_HIP_TRY(drp.alloc(rpb));
    LHPC_HIP_TRY(dc.alloc(n * 4));
    LHPC_HIP_TRY(dtrp.alloc(trpb));
    LHPC_HIP_TRY(dtc.alloc(n * 4));
    LHPC_HIP_TRY(dpm.alloc(n * 4));
    if (val) {
      LHPC_HIP_TRY(dv.alloc(n * tsz));
      LHPC_HIP_TRY(dtv.alloc(n * tsz));
    }
    LHPC_HIP_TRY(hipMemcpy(drp.p, row_ptr, rpb, hipMemcpyHostToDevice));
    if (n) {
      LHPC_HIP_TRY(hipMemcpy(dc.p, col_idx, n * 4, hipMemcpyHostToDevice));
      if (val) LHPC_HIP_TRY(hipMemcpy(dv.p, val, n * tsz, hipMemcpyHostToDevice));
    }
    LHPC_TRY(csr_transpose_dev(tsz, n_rows, n_cols, nnz, drp.p, row_ptr_bits, static_cast<const int32_t *>(dc.p),
                               val ? dv.p : nullptr, dtrp.p, static_cast<int32_t *>(dtc.p), val ? dtv.p : nullptr,
                               static_cast<uint32_t *>(dpm.p), s));  // ends with a stream synchronize
    LHPC_HIP_TRY(hipMemcpy(t_row_ptr, dtrp.p, trpb, hipMemcpyDeviceToHost));
    if (n) {
      LHPC_HIP_TRY(hipMemcpy(t_col_idx, dtc.p, n * 4, hipMemcpyDeviceToHost));
      if (val) LHPC_HIP_TRY(hipMemcpy(t_val, dtv.p, n * tsz, hipMemcpyDeviceToHost));
      if (perm) LHPC_HIP_TRY(hipMemcpy(perm, dpm.p, n * 4, hipMemcpyDeviceToHost));
    }
    return LHPC_OK;
  } LHPC_ABI_CATCH
}
