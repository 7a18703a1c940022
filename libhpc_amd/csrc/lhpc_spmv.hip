// lhpc_spmv.hip — CSR SpMV y = A·x for gfx950 (MI355X), behind include/lhpc.h:
// plan creation and the C ABI.  Creation is one flow for host and device
// input (plan_create_impl): checks, source set-up (validation), row
// statistics and the locality sample, then the family stages XTILE → XSLICE
// → SELL → CSR that lhpc_plan.hpp spmv_family_policy selects (build_single).
// The kernels and the family builders live in lhpc_spmv_{csr,xslice,xtile}.hip
// (lhpc_spmv_impl.hpp).
//
// The reference has no SpMV; the operator is defined
// here as y[i] = Σ_{k=row_ptr[i]}^{row_ptr[i+1]-1} val[k]·x[col_idx[k]].
// Numerics: every dtype accumulates in fp64 registers and rounds once at the
// store (SURVEY §8c "binding recommendation"), so fp32 results are within
// 2^-24·|y| + ~1e-16·Σ|a·x| of the exact sum for any row length.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "lhpc_plan.hpp"
#include "lhpc_spmv_impl.hpp"

namespace lhpc {
namespace {

// Distinct 128-B x lines touched per nonzero, over up to 32 evenly spaced
// chunks of 8192 consecutive rows (1.0 = no reuse within a chunk).  The
// columns of a device source are copied to the host chunk by chunk.
double gather_lines_per_nnz(const CsrSource &src, int64_t n_rows, int64_t n_cols, size_t tsz) {
  constexpr int64_t kChunk = 8192, kSamples = 32;
  const int shift = tsz == 8 ? 4 : 5;  // 16 doubles / 32 floats per line
  const int64_t chunks = (n_rows + kChunk - 1) / kChunk;
  const int64_t step = std::max<int64_t>(1, chunks / kSamples);
  int64_t lines = 0, nz = 0;
  std::vector<int32_t> copy;
  // distinct lines per sample with a bitmap over x's lines (set, count, then
  // clear what was set): O(nonzeros) where a sort + unique cost ≈ 0.2 s for C2
  std::vector<uint64_t> seen(static_cast<size_t>(((n_cols >> shift) + 64) / 64), 0);
  for (int64_t c = 0; c < chunks; c += step) {
    const int64_t r0 = c * kChunk, r1 = std::min(n_rows, r0 + kChunk);
    const int64_t k0 = src.rp[r0], k1 = src.rp[r1];
    const int32_t *col = src.col + k0;
    if (src.d_rp && k1 > k0) {
      copy.resize(static_cast<size_t>(k1 - k0));
      if (hipMemcpy(copy.data(), col, copy.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1.0;
      col = copy.data();
    }
    for (int64_t k = 0; k < k1 - k0; ++k) {
      const uint64_t l = static_cast<uint64_t>(col[k]) >> shift, bit = uint64_t{1} << (l & 63);
      uint64_t &w = seen[static_cast<size_t>(l >> 6)];
      lines += (w & bit) ? 0 : 1;
      w |= bit;
    }
    for (int64_t k = 0; k < k1 - k0; ++k) seen[static_cast<size_t>((static_cast<uint64_t>(col[k]) >> shift) >> 6)] = 0;
    nz += k1 - k0;
  }
  return nz ? static_cast<double>(lines) / static_cast<double>(nz) : 1.0;
}

// device CSR checks for LHPC_PLAN_DEVICE_INPUT (validate_csr on the GPU):
// bit 0: row_ptr[0] != 0, decreasing, or row_ptr[n_rows] != nnz; bit 1: a
// column outside [0, n_cols)
__global__ void k_validate_device_csr(const void *rp, int bits, const int32_t *col, int64_t n_rows, int64_t n_cols,
                                      int64_t nnz, unsigned *flag) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x, T = static_cast<int64_t>(gridDim.x) * blockDim.x;
  auto at = [&](int64_t i) -> int64_t {
    return bits == 64 ? static_cast<const int64_t *>(rp)[i] : static_cast<const int32_t *>(rp)[i];
  };
  unsigned bad = 0;
  for (int64_t i = t; i < n_rows; i += T)
    if (at(i + 1) < at(i)) bad |= 1u;
  if (t == 0 && (at(0) != 0 || at(n_rows) != nnz)) bad |= 1u;
  for (int64_t k = t; k < nnz; k += T)
    if (col[k] < 0 || col[k] >= n_cols) bad |= 2u;
  if (bad) atomicOr(flag, bad);
}

// XTILE column blocks from device-resident CSR (build_parts, device source):
// rows [r0, r0 + nr) restricted to columns [c0, c1), rebased — the device
// twin of lhpc_plan.cpp csr_column_block (count per row, host scan, scatter)
__device__ __forceinline__ int64_t rp_dev(const void *rp, int bits, int64_t i) {
  return bits == 64 ? static_cast<const int64_t *>(rp)[i] : static_cast<const int32_t *>(rp)[i];
}
__global__ void k_colblock_count(const void *rp, int bits, const int32_t *col, int64_t r0, int64_t nr, int32_t c0,
                                 int32_t c1, int32_t *cnt) {
  const int64_t T = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < nr; r += T) {
    int32_t c = 0;
    for (int64_t k = rp_dev(rp, bits, r0 + r), e = rp_dev(rp, bits, r0 + r + 1); k < e; ++k)
      c += col[k] >= c0 && col[k] < c1;
    cnt[r] = c;
  }
}
template <typename T>
__global__ void k_colblock_scatter(const void *rp, int bits, const int32_t *col, const T *val, int64_t r0, int64_t nr,
                                   int32_t c0, int32_t c1, const int64_t *orp, int32_t *ocol, T *oval) {
  const int64_t G = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < nr; r += G) {
    int64_t o = orp[r];
    for (int64_t k = rp_dev(rp, bits, r0 + r), e = rp_dev(rp, bits, r0 + r + 1); k < e; ++k)
      if (col[k] >= c0 && col[k] < c1) {
        ocol[o] = col[k] - c0;
        oval[o] = val[k];
        ++o;
      }
  }
}

// one column block on the device: host row offsets in orp, device col/val in
// the returned buffers (freed by the caller)
int colblock_device(const void *d_rp, int bits, const int32_t *d_col, const void *d_val, size_t tsz, int64_t r0,
                    int64_t r1, int64_t c0, int64_t c1, std::vector<int64_t> &orp, void **d_ocol, void **d_oval) {
  const int64_t nr = r1 - r0;
  *d_ocol = *d_oval = nullptr;
  orp.assign(static_cast<size_t>(nr) + 1, 0);
  std::vector<int32_t> cnt(static_cast<size_t>(nr));
  int32_t *d_cnt = nullptr;
  int64_t *d_orp = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_cnt), static_cast<size_t>(std::max<int64_t>(nr, 1)) * 4);
  const unsigned grid = static_cast<unsigned>(std::min<int64_t>((nr + 255) / 256 + 1, 8192));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_colblock_count, dim3(grid), dim3(256), 0, nullptr, d_rp, bits, d_col, r0, nr,
                       static_cast<int32_t>(c0), static_cast<int32_t>(c1), d_cnt);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(cnt.data(), d_cnt, static_cast<size_t>(nr) * 4, hipMemcpyDeviceToHost);
  (void)hipFree(d_cnt);
  if (e != hipSuccess) return static_cast<int>(e);
  for (int64_t r = 0; r < nr; ++r) orp[static_cast<size_t>(r) + 1] = orp[static_cast<size_t>(r)] + cnt[static_cast<size_t>(r)];
  const int64_t m = orp[static_cast<size_t>(nr)];
  if (m == 0) return LHPC_OK;
  e = hipMalloc(&d_orp, static_cast<size_t>(nr + 1) * 8);
  if (e == hipSuccess) e = hipMemcpy(d_orp, orp.data(), static_cast<size_t>(nr + 1) * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(d_ocol, static_cast<size_t>(m) * 4);
  if (e == hipSuccess) e = hipMalloc(d_oval, static_cast<size_t>(m) * tsz);
  if (e == hipSuccess) {
    if (tsz == 4)
      hipLaunchKernelGGL(k_colblock_scatter<float>, dim3(grid), dim3(256), 0, nullptr, d_rp, bits, d_col,
                         static_cast<const float *>(d_val), r0, nr, static_cast<int32_t>(c0), static_cast<int32_t>(c1),
                         d_orp, static_cast<int32_t *>(*d_ocol), static_cast<float *>(*d_oval));
    else
      hipLaunchKernelGGL(k_colblock_scatter<double>, dim3(grid), dim3(256), 0, nullptr, d_rp, bits, d_col,
                         static_cast<const double *>(d_val), r0, nr, static_cast<int32_t>(c0), static_cast<int32_t>(c1),
                         d_orp, static_cast<int32_t *>(*d_ocol), static_cast<double *>(*d_oval));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  (void)hipFree(d_orp);
  return static_cast<int>(e);
}

int launch(const lhpc_spmv_plan *p, const void *x, void *y, hipStream_t s) {
  if (!p->parts.empty()) {
    const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
    for (size_t i = 0; i < p->parts.size(); ++i)
      LHPC_TRY(xtile_launch(p->parts[i], static_cast<const unsigned char *>(x) + p->part_col[i] * tsz,
                            static_cast<unsigned char *>(y) + p->part_row[i] * tsz, s));
    return LHPC_OK;
  }
  if (p->kernel == LHPC_KERNEL_XTILE) return xtile_launch(p, x, y, s);
  if (p->kernel == LHPC_KERNEL_XSLICE) return xslice_launch(p, x, y, s);
  return csr_launch(p, x, y, s);
}

// ------------------------------------------------------------ plan creation
// A plan under construction is destroyed with whatever it owns unless
// creation succeeds and releases it into *out.
struct PlanDeleter {
  void operator()(lhpc_spmv_plan *p) const { lhpc_spmv_plan_destroy(p); }
};
using PlanPtr = std::unique_ptr<lhpc_spmv_plan, PlanDeleter>;

// nullptr: no memory
lhpc_spmv_plan *new_plan(const lhpc_options &o, int dtype, int device, int64_t n_rows, int64_t n_cols, int64_t nnz) {
  auto *p = new (std::nothrow) lhpc_spmv_plan();
  if (!p) return nullptr;
  p->opt = o;
  p->dtype = dtype;
  p->device = device;
  p->n_rows = n_rows;
  p->n_cols = n_cols;
  p->nnz = nnz;
  return p;
}

// a refused XTILE build leaves no parts behind
void reset_parts(lhpc_spmv_plan *p) {
  for (auto *q : p->parts) lhpc_spmv_plan_destroy(q);
  p->parts.clear();
  p->part_row.clear();
  p->part_col.clear();
  p->bytes = 0;
}

// Host copies of device-resident input: row_ptr from the start (every
// decision reads it), col / val once a stage without a GPU builder needs them.
struct HostCopy {
  std::vector<unsigned char> rp, val;
  std::vector<int32_t> col;
};

// LHPC_PLAN_DEVICE_INPUT: row_ptr / col_idx / val in HBM of the plan's device
// (e.g. straight from lhpc_coo_to_csr on the device), validated on the GPU;
// row_ptr (n_rows + 1 words) comes back to the host
int device_source(CsrSource &src, HostCopy &host, int64_t n_rows, int64_t n_cols, int64_t nnz) {
  RocTxRange rx("lhpc_spmv_plan_create: device input");
  // the arrays may still be in flight on any stream of the caller (plan
  // creation is synchronous anyway)
  LHPC_HIP_TRY(hipDeviceSynchronize());
  LHPC_TRY(validate_csr_device(src.rp.p, src.rp.bits, src.col, n_rows, n_cols, nnz));
  host.rp.resize(static_cast<size_t>(n_rows + 1) * (src.rp.bits / 8));
  LHPC_HIP_TRY(hipMemcpy(host.rp.data(), src.rp.p, host.rp.size(), hipMemcpyDeviceToHost));
  src.d_rp = src.rp.p;
  src.rp.p = host.rp.data();
  return LHPC_OK;
}

// a stage without a GPU builder: a device source becomes a host source, once
int to_host(CsrSource &src, HostCopy &host, int64_t nnz, size_t tsz) {
  if (!src.d_rp) return LHPC_OK;
  host.col.resize(static_cast<size_t>(nnz));
  host.val.resize(static_cast<size_t>(nnz) * tsz);
  if (nnz) {
    LHPC_HIP_TRY(hipMemcpy(host.col.data(), src.col, host.col.size() * 4, hipMemcpyDeviceToHost));
    LHPC_HIP_TRY(hipMemcpy(host.val.data(), src.val, host.val.size(), hipMemcpyDeviceToHost));
  }
  src = CsrSource{src.rp, host.col.data(), host.val.data(), nullptr};
  return LHPC_OK;
}

// XTILE row parts: the tile stream of one plan is addressed with int32
// offsets (nnz + 8 padding entries per tile < 2^31, lhpc_plan.cpp
// build_xtile).  A larger matrix (n ≳ 143M rows at 15 nonzeros per row) is
// cut into nnz-balanced row parts of ≤ cap nonzeros, each an ordinary XTILE
// plan over its rows (row_ptr rebased, the caller's col/val at the part's
// offset) run in turn on the same x, instead of dropping to XSLICE.  With
// B > 1 column blocks every row part is further cut by column (lhpc_plan.cpp
// xtile_partition_policy).
// LHPC_ERR_UNSUPPORTED when some single row exceeds the cap.
// A device source has every part's column block cut and layout built on the GPU.
int build_parts(lhpc_spmv_plan *p, const CsrSource &src, int64_t cap, int B) {
  const RowPtrView rp = src.rp;
  const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
  const int64_t n_rows = p->n_rows;
  int64_t n_parts = std::max<int64_t>(1, (p->nnz + cap - 1) / cap);
  std::vector<int64_t> cuts;
  for (;; ++n_parts) {  // nnz-balanced cuts; one more part until every part fits
    cuts.assign(static_cast<size_t>(n_parts) + 1, 0);
    LHPC_TRY(lhpc_csr_partition_rows(rp.p, rp.bits, n_rows, static_cast<int>(n_parts), cuts.data()));
    bool fit = true;
    for (int64_t i = 0; i < n_parts && fit; ++i) {
      const int64_t r0 = cuts[i], r1 = cuts[i + 1];
      if (r1 - r0 == 1 && rp[r1] - rp[r0] > cap) return LHPC_ERR_UNSUPPORTED;  // one row past the cap
      fit = rp[r1] - rp[r0] <= cap;
    }
    if (fit) break;
    if (n_parts > n_rows) return LHPC_ERR_UNSUPPORTED;
  }
  // column block bounds, 64-column aligned (x + bound stays 256-B aligned)
  std::vector<int64_t> cb(static_cast<size_t>(B) + 1, p->n_cols);
  for (int b = 0; b < B; ++b) cb[b] = p->n_cols * b / B / 64 * 64;
  std::vector<int64_t> lrp;  // the part's row offsets, rebased
  // the part's col / val live where the source's do (xtile_build reads only
  // whether d_rp is set)
  auto add = [&](int64_t r0, int64_t r1, int64_t c0, int64_t c1, const int32_t *lc, const void *lv, int64_t lnnz,
                 int acc) -> int {
    auto *q = new_plan(p->opt, p->dtype, p->device, r1 - r0, c1 - c0, lnnz);
    if (!q) return LHPC_ERR_ALLOC;
    p->parts.push_back(q);
    p->part_row.push_back(r0);
    p->part_col.push_back(c0);
    q->xt_acc = acc;
    if (B > 1) q->opt.xtile_chunkrec = 1;  // column blocks: every block keeps the row_ptr reduce (rows empty in a block)
    LHPC_TRY(xtile_build(q, CsrSource{RowPtrView{lrp.data(), 64}, lc, lv, src.d_rp}));
    p->bytes += q->bytes;
    return LHPC_OK;
  };
  std::vector<int32_t> lcol;
  std::vector<unsigned char> lval;
  for (int64_t i = 0; i < n_parts; ++i) {
    const int64_t r0 = cuts[i], r1 = cuts[i + 1];
    if (r1 == r0) continue;
    const int64_t e0 = rp[r0];
    if (B == 1 || rp[r1] == e0) {
      lrp.resize(static_cast<size_t>(r1 - r0 + 1));
      for (int64_t r = r0; r <= r1; ++r) lrp[static_cast<size_t>(r - r0)] = rp[r] - e0;
      LHPC_TRY(add(r0, r1, 0, p->n_cols, src.col + e0,
                   static_cast<const unsigned char *>(src.val) + e0 * static_cast<int64_t>(tsz), rp[r1] - e0, 0));
      continue;
    }
    bool first = true;  // the first non-empty block stores every row of the part
    for (int b = 0; b < B; ++b) {
      if (src.d_rp) {
        struct Tmp {
          void *c = nullptr, *v = nullptr;
          ~Tmp() {
            if (c) (void)hipFree(c);
            if (v) (void)hipFree(v);
          }
        } t;
        LHPC_TRY(colblock_device(src.d_rp, rp.bits, src.col, src.val, tsz, r0, r1, cb[b], cb[b + 1], lrp, &t.c, &t.v));
        const int64_t m = lrp.back();
        if (m == 0) continue;  // adds nothing
        LHPC_TRY(add(r0, r1, cb[b], cb[b + 1], static_cast<const int32_t *>(t.c), t.v, m, first ? 0 : 1));
      } else {
        csr_column_block(rp.p, rp.bits, src.col, src.val, tsz, r0, r1, cb[b], cb[b + 1], lrp, lcol, lval);
        if (lcol.empty()) continue;  // adds nothing
        LHPC_TRY(add(r0, r1, cb[b], cb[b + 1], lcol.data(), lval.data(), static_cast<int64_t>(lcol.size()),
                     first ? 0 : 1));
      }
      first = false;
    }
  }
  p->part_row.push_back(n_rows);
  p->kernel = LHPC_KERNEL_XTILE;
  p->S = p->parts.empty() ? 0 : p->parts[0]->S;
  p->xs_width = p->parts.empty() ? 0 : p->parts[0]->xs_width;
  return LHPC_OK;
}

// one plan, or row parts × column blocks (lhpc_plan.hpp xtile_partition_policy)
int xtile_build_whole(lhpc_spmv_plan *p, const CsrSource &src, const XtilePartition &pp) {
  return pp.parts ? build_parts(p, src, pp.cap, pp.col_blocks) : xtile_build(p, src);
}

// host A → HBM copies → the device layout build; LHPC_ERR_UNSUPPORTED when
// the device build does not apply (aligned segments) or the copies do not fit
// in HBM
int xtile_build_uploaded(lhpc_spmv_plan *p, const CsrSource &src, const XtilePartition &pp) {
  if (p->opt.xtile_host_build == 1 || p->opt.xtile_align == LHPC_XTILE_ALIGN_UNITS || p->nnz == 0)
    return LHPC_ERR_UNSUPPORTED;
  struct Tmp {
    void *a = nullptr;
    ~Tmp() {
      if (a) (void)hipFree(a);
    }
  } d_rp, d_col, d_val;
  const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
  const size_t rpb = static_cast<size_t>(p->n_rows + 1) * (src.rp.bits / 8);
  const size_t nnz = static_cast<size_t>(p->nnz);
  if (hipMalloc(&d_rp.a, rpb) != hipSuccess || hipMalloc(&d_col.a, nnz * 4) != hipSuccess ||
      hipMalloc(&d_val.a, nnz * tsz) != hipSuccess) {
    (void)hipGetLastError();
    return LHPC_ERR_UNSUPPORTED;
  }
  LHPC_HIP_TRY(hipMemcpy(d_rp.a, src.rp.p, rpb, hipMemcpyHostToDevice));
  LHPC_HIP_TRY(hipMemcpy(d_col.a, src.col, nnz * 4, hipMemcpyHostToDevice));
  LHPC_HIP_TRY(hipMemcpy(d_val.a, src.val, nnz * tsz, hipMemcpyHostToDevice));
  return xtile_build_whole(p, CsrSource{src.rp, static_cast<const int32_t *>(d_col.a), d_val.a, d_rp.a}, pp);
}

// The XTILE stage.  The layout is built on the GPU: from a device source as
// it is, from host arrays through uploaded copies (byte-identical to the host
// build, DESIGN.md §4 device input; C2 0.57 → ≈ 0.15 s).  The host build takes
// over when the GPU build refuses (aligned segments, no memory).  The GPU
// build makes the host build's own refusals (xtile_plan_chunks: tiles, int32
// stream offsets), so a device source needs no guard in front of it: what
// neither can hold ends as LHPC_ERR_UNSUPPORTED, for XSLICE or a CSR kernel.
int xtile_stage(lhpc_spmv_plan *p, CsrSource &src, HostCopy &host, const XtilePartition &pp) {
  const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
  const std::vector<int64_t> splits_in = p->split_rows;  // a build may add cache-range cuts
  int st = src.d_rp ? xtile_build_whole(p, src, pp) : xtile_build_uploaded(p, src, pp);
  if (st == LHPC_ERR_UNSUPPORTED) {
    reset_parts(p);
    p->split_rows = splits_in;
    LHPC_TRY(to_host(src, host, p->nnz, tsz));
    st = xtile_build_whole(p, src, pp);
  }
  if (st == LHPC_ERR_UNSUPPORTED) reset_parts(p);
  return st;
}

// The CSR stage: ROWGROUP / ADAPTIVE keep the caller's CSR — row_ptr (int32
// offsets whenever they fit: 4 B/row less HBM traffic), col, val — and
// ADAPTIVE its block table
int csr_upload(lhpc_spmv_plan *p, const CsrSource &src, size_t tsz) {
  const size_t nnz = static_cast<size_t>(p->nnz);
  p->rp64 = p->nnz > INT32_MAX ? 1 : 0;
  const size_t rp_bytes = static_cast<size_t>(p->n_rows + 1) * (p->rp64 ? 8 : 4);
  LHPC_TRY(dmalloc(&p->d_row_ptr, rp_bytes, p->bytes));
  LHPC_TRY(dmalloc(reinterpret_cast<void **>(&p->d_col), nnz * 4, p->bytes));
  LHPC_TRY(dmalloc(&p->d_val, nnz * tsz, p->bytes));
  if (p->rp64 == (src.rp.bits == 64 ? 1 : 0)) {
    LHPC_HIP_TRY(hipMemcpy(p->d_row_ptr, src.rp.p, rp_bytes, hipMemcpyHostToDevice));
  } else {  // row_ptr in the device width
    std::vector<int32_t> tmp(static_cast<size_t>(p->n_rows + 1));
    for (int64_t i = 0; i <= p->n_rows; ++i) tmp[static_cast<size_t>(i)] = static_cast<int32_t>(src.rp[i]);
    LHPC_HIP_TRY(hipMemcpy(p->d_row_ptr, tmp.data(), rp_bytes, hipMemcpyHostToDevice));
  }
  if (nnz) {
    LHPC_HIP_TRY(hipMemcpy(p->d_col, src.col, nnz * 4, hipMemcpyHostToDevice));
    LHPC_HIP_TRY(hipMemcpy(p->d_val, src.val, nnz * tsz, hipMemcpyHostToDevice));
  }
  if (p->kernel != LHPC_KERNEL_ADAPTIVE) return LHPC_OK;
  const std::vector<int64_t> bp = csr_block_table(src.rp, p->n_rows, p->n_blocks, p->n_long);
  LHPC_TRY(dmalloc(reinterpret_cast<void **>(&p->d_blocks), bp.size() * 8, p->bytes));
  LHPC_HIP_TRY(hipMemcpy(p->d_blocks, bp.data(), bp.size() * 8, hipMemcpyHostToDevice));
  return LHPC_OK;
}

// A single-device plan: row statistics, the locality sample if the policy
// wants it, then the family stages in spmv_family_policy's order.  A stage
// that answers LHPC_ERR_UNSUPPORTED leaves the plan to the next one.  A device
// source stays on the device for the stages with a GPU builder (XTILE, SELL);
// the first stage without one copies it to the host (to_host).
int build_single(lhpc_spmv_plan *p, CsrSource &src, HostCopy &host, unsigned flags, int n_splits) {
  const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
  SpmvShape sh;
  sh.n_rows = p->n_rows;
  sh.n_cols = p->n_cols;
  sh.nnz = p->nnz;
  sh.elem_bytes = tsz;
  sh.n_splits = n_splits;
  for (int64_t i = 0; i < p->n_rows; ++i) sh.max_row_len = std::max(sh.max_row_len, src.rp[i + 1] - src.rp[i]);
  if (spmv_wants_locality(p->n_cols, tsz, flags)) sh.lines_per_nnz = gather_lines_per_nnz(src, p->n_rows, p->n_cols, tsz);
  const SpmvFamilyPolicy pol = spmv_family_policy(sh, flags, p->opt);

  int st = LHPC_ERR_UNSUPPORTED;
  if (pol.try_xtile) st = xtile_stage(p, src, host, pol.part);
  if (st == LHPC_ERR_UNSUPPORTED && pol.try_xslice) {
    LHPC_TRY(to_host(src, host, p->nnz, tsz));
    st = xslice_build(p, src.rp, src.col, src.val, tsz, flags);
  }
  if (st == LHPC_ERR_UNSUPPORTED && pol.try_sell) st = sell_build(p, src, tsz, pol.force_sell);
  if (st != LHPC_ERR_UNSUPPORTED) return st;
  LHPC_TRY(pol.csr_status);
  if (pol.force_sell) return LHPC_ERR_UNSUPPORTED;  // a row longer than kSellMaxW (or no rows)
  p->kernel = pol.csr_kernel;
  p->L = pol.L;
  p->R = pol.R;
  LHPC_TRY(to_host(src, host, p->nnz, tsz));
  return csr_upload(p, src, tsz);
}

// the plan's device: device_ids[0] or the current one, and a gfx950
int pick_device(const int *device_ids, int n_devices, int &dev) {
  if (device_ids && n_devices >= 1) {
    dev = device_ids[0];
    LHPC_HIP_TRY(hipSetDevice(dev));
  } else {
    LHPC_HIP_TRY(hipGetDevice(&dev));
  }
  return is_gfx950(dev) ? LHPC_OK : LHPC_ERR_NO_DEVICE;
}

int plan_create_impl(lhpc_spmv_plan **out, int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz,
                     const void *row_ptr, int row_ptr_bits, const int32_t *col_idx, const void *val,
                     const int *device_ids, int n_devices, unsigned flags, int n_splits,
                     const int64_t *split_rows, const lhpc_options *opts) {
  if (!out) return LHPC_ERR_INVALID_ARG;
  const lhpc_options o = resolve_options(opts);
  *out = nullptr;
  if ((dtype != LHPC_F32 && dtype != LHPC_F64) || n_rows < 0 || n_cols < 0 || nnz < 0 ||
      !row_ptr || (row_ptr_bits != 32 && row_ptr_bits != 64) || n_cols > INT32_MAX ||
      (nnz > 0 && (!col_idx || !val)))
    return LHPC_ERR_INVALID_ARG;
  if (n_devices < 0 || (n_devices > 1 && !device_ids)) return LHPC_ERR_INVALID_ARG;
  if (row_ptr_bits == 32 && nnz > INT32_MAX) return LHPC_ERR_INVALID_ARG;
  // several devices driven by this one host thread: one local
  // plan, stream, comm stream (and RCCL comm) per device (lhpc_multi.hip)
  const bool multi = n_devices > 1 || (o.multi_force && n_devices == 1 && device_ids);
  const bool device_input = (flags & LHPC_PLAN_DEVICE_INPUT) != 0;
  const bool transpose = (flags & LHPC_PLAN_TRANSPOSE) != 0;
  flags &= ~static_cast<unsigned>(LHPC_PLAN_DEVICE_INPUT | LHPC_PLAN_TRANSPOSE);  // from here on src says where A lives
  if (transpose) {
    if (n_rows > INT32_MAX) return LHPC_ERR_INVALID_ARG;  // A's rows are the operator's columns
    // row ranges and the row-block split are those of A·x
    if (n_splits > 0 || multi) return LHPC_ERR_UNSUPPORTED;
  }

  CsrSource src{RowPtrView{row_ptr, row_ptr_bits}, col_idx, val, nullptr};
  HostCopy host;
  int dev = 0;
  if (transpose) {
    // LHPC_PLAN_TRANSPOSE: A is transposed on the plan's device
    // (lhpc_transpose.hip, which validates it there) and the plan is built
    // from Aᵀ's arrays as from any device input; it keeps the permutation
    LHPC_TRY(pick_device(device_ids, n_devices, dev));
    PlanPtr p(new_plan(o, dtype, dev, n_cols, n_rows, nnz));
    if (!p) return LHPC_ERR_ALLOC;
    int64_t perm_bytes = 0;  // booked once the family stands (a refused XTILE build resets the count)
    LHPC_TRY(dmalloc(reinterpret_cast<void **>(&p->d_tperm), static_cast<size_t>(nnz) * 4, perm_bytes));
    TransposedCsr t;
    LHPC_TRY(transpose_for_plan(t, dtype == LHPC_F32 ? 4 : 8, n_rows, n_cols, nnz, row_ptr, row_ptr_bits, col_idx, val,
                                device_input, p->d_tperm));
    src = CsrSource{RowPtrView{t.t_rp, row_ptr_bits}, static_cast<const int32_t *>(t.t_col), t.t_val, nullptr};
    LHPC_TRY(device_source(src, host, n_cols, n_rows, nnz));
    LHPC_TRY(build_single(p.get(), src, host, flags, 0));
    p->bytes += perm_bytes;
    *out = p.release();
    return LHPC_OK;  // t: Aᵀ's arrays are freed now that the layout stands
  }
  if (device_input) {
    LHPC_TRY(pick_device(device_ids, n_devices, dev));  // where the arrays are
    LHPC_TRY(device_source(src, host, n_rows, n_cols, nnz));
  } else {
    // always: every layout pass indexes host arrays by row_ptr / col_idx, and
    // every kernel indexes x by col_idx (LHPC_PLAN_VALIDATE is implied)
    LHPC_TRY(validate_csr(row_ptr, row_ptr_bits, col_idx, n_rows, n_cols, nnz));
  }
  if (multi) {  // built from host arrays; picks its devices itself
    if (n_splits > 0) return LHPC_ERR_UNSUPPORTED;
    LHPC_TRY(to_host(src, host, nnz, dtype == LHPC_F32 ? 4 : 8));
    PlanPtr p(new_plan(o, dtype, 0, n_rows, n_cols, nnz));
    if (!p) return LHPC_ERR_ALLOC;
    LHPC_TRY(multi_create(p.get(), src.rp, src.col, src.val, device_ids, n_devices, flags));
    *out = p.release();
    return LHPC_OK;
  }
  if (!device_input) LHPC_TRY(pick_device(device_ids, n_devices, dev));

  PlanPtr p(new_plan(o, dtype, dev, n_rows, n_cols, nnz));
  if (!p) return LHPC_ERR_ALLOC;
  if (n_splits > 0) p->split_rows.assign(split_rows, split_rows + n_splits);
  LHPC_TRY(build_single(p.get(), src, host, flags, n_splits));
  // row ranges exist only in the XTILE tile-stream layout
  if (n_splits > 0 && (p->kernel != LHPC_KERNEL_XTILE || p->xt_srow.size() != static_cast<size_t>(n_splits) + 2))
    return LHPC_ERR_UNSUPPORTED;
  *out = p.release();
  return LHPC_OK;
}

}  // namespace

bool is_gfx950(int dev) {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return false;
  return std::strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

int validate_csr_device(const void *row_ptr, int row_ptr_bits, const int32_t *col_idx, int64_t n_rows,
                        int64_t n_cols, int64_t nnz) {
  unsigned *flag = nullptr;
  LHPC_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&flag), 4));
  hipError_t e = hipMemset(flag, 0, 4);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_validate_device_csr, dim3(1024), dim3(256), 0, nullptr, row_ptr, row_ptr_bits, col_idx,
                       n_rows, n_cols, nnz, flag);
    e = hipGetLastError();
  }
  unsigned bad = 0;
  if (e == hipSuccess) e = hipMemcpy(&bad, flag, 4, hipMemcpyDeviceToHost);
  (void)hipFree(flag);
  if (e != hipSuccess) return static_cast<int>(e);
  return bad ? LHPC_ERR_BAD_CSR : LHPC_OK;
}

}  // namespace lhpc

using namespace lhpc;

extern "C" int lhpc_spmv_plan_create(lhpc_spmv_plan **out, int dtype, int64_t n_rows,
                                     int64_t n_cols, int64_t nnz, const void *row_ptr,
                                     int row_ptr_bits, const int32_t *col_idx,
                                     const void *val, const int *device_ids,
                                     int n_devices, unsigned flags) {
  try {
    RocTxRange rx("lhpc_spmv_plan_create");
    return plan_create_impl(out, dtype, n_rows, n_cols, nnz, row_ptr, row_ptr_bits, col_idx, val,
                            device_ids, n_devices, flags, 0, nullptr, nullptr);
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmv_plan_create_opts(lhpc_spmv_plan **out, int dtype, int64_t n_rows,
                                          int64_t n_cols, int64_t nnz, const void *row_ptr,
                                          int row_ptr_bits, const int32_t *col_idx,
                                          const void *val, const int *device_ids, int n_devices,
                                          unsigned flags, int n_splits, const int64_t *split_rows,
                                          const lhpc_options *opts) {
  try {
    if (!out || n_splits < 0 || (n_splits > 0 && !split_rows)) return LHPC_ERR_INVALID_ARG;
    for (int i = 0; i < n_splits; ++i)
      if (split_rows[i] <= 0 || split_rows[i] >= n_rows || (i > 0 && split_rows[i] <= split_rows[i - 1]))
        return LHPC_ERR_INVALID_ARG;
    RocTxRange rx("lhpc_spmv_plan_create");
    return plan_create_impl(out, dtype, n_rows, n_cols, nnz, row_ptr, row_ptr_bits, col_idx, val, device_ids,
                            n_devices, flags, n_splits, split_rows, opts);
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmv_plan_create_split(lhpc_spmv_plan **out, int dtype, int64_t n_rows,
                                           int64_t n_cols, int64_t nnz, const void *row_ptr,
                                           int row_ptr_bits, const int32_t *col_idx,
                                           const void *val, const int *device_ids, int n_devices,
                                           unsigned flags, int n_splits, const int64_t *split_rows) {
  try {
    if (n_splits < 1) return LHPC_ERR_INVALID_ARG;
    return lhpc_spmv_plan_create_opts(out, dtype, n_rows, n_cols, nnz, row_ptr, row_ptr_bits, col_idx, val,
                                      device_ids, n_devices, flags, n_splits, split_rows, nullptr);
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmv_stage(const lhpc_spmv_plan *p, const void *x, void *stream) {
  try {
    if (!p || (p->n_cols > 0 && !x)) return LHPC_ERR_INVALID_ARG;
    if (p->xt_srow.empty() || p->xt_ring) return LHPC_ERR_UNSUPPORTED;  // a ring holds one range's xg
    RocTxRange rx("lhpc_spmv_stage");
    LHPC_HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return xtile_stage(p, x, s);
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmv_range(const lhpc_spmv_plan *p, int k, void *y_range, void *stream) {
  try {
    if (!p || p->xt_srow.empty() || k < 0 || k + 2 > static_cast<int>(p->xt_srow.size()))
      return LHPC_ERR_INVALID_ARG;
    if (p->xt_ring) return LHPC_ERR_UNSUPPORTED;
    if (p->xt_srow[k + 1] > p->xt_srow[k] && !y_range) return LHPC_ERR_INVALID_ARG;
    RocTxRange rx("lhpc_spmv_range");
    LHPC_HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return xtile_range(p, k, y_range, s);
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmv(lhpc_spmv_plan *p, const void *x, void *y, int on_device,
                         void *stream) {
  try {
    if (!p || (p->n_cols > 0 && !x) || (p->n_rows > 0 && !y)) return LHPC_ERR_INVALID_ARG;
    RocTxRange rx("lhpc_spmv");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p->multi) return multi_home(p, x, y, on_device, s);
    LHPC_HIP_TRY(hipSetDevice(p->device));
    const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
    const void *dx = x;
    void *dy = y;
    if (!on_device) {
      if (!p->d_xstage) {
        LHPC_TRY(dmalloc(&p->d_xstage, static_cast<size_t>(p->n_cols) * tsz, p->bytes));
        LHPC_TRY(dmalloc(&p->d_ystage, static_cast<size_t>(p->n_rows) * tsz, p->bytes));
      }
      // host buffers: synchronous copies (see lhpc_sort.hip HostStage); the
      // staging buffers are only touched by host-buffer calls, which end synced
      LHPC_HIP_TRY(hipMemcpy(p->d_xstage, x, static_cast<size_t>(p->n_cols) * tsz, hipMemcpyHostToDevice));
      dx = p->d_xstage;
      dy = p->d_ystage;
    }
    const int st = launch(p, dx, dy, s);
    if (st != LHPC_OK) return st;
    if (!on_device) {
      LHPC_HIP_TRY(hipStreamSynchronize(s));
      LHPC_HIP_TRY(hipMemcpy(y, p->d_ystage, static_cast<size_t>(p->n_rows) * tsz, hipMemcpyDeviceToHost));
    }
    return LHPC_OK;
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_vec_dot(int dtype, int64_t n, const void *a, const void *b, double *out, void *stream);

extern "C" int lhpc_spmv_dot(lhpc_spmv_plan *p, const void *x, void *y, const void *w, double *dot_out,
                             void *stream) {
  try {
    if (!p || !dot_out || (p->n_cols > 0 && !x) || (p->n_rows > 0 && (!y || !w))) return LHPC_ERR_INVALID_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    LHPC_HIP_TRY(hipSetDevice(p->device));
    if ((p->kernel == LHPC_KERNEL_ADAPTIVE || p->kernel == LHPC_KERNEL_SELL) && p->n_blocks > 0) {
      const int st = csr_launch_dot(p, x, y, w, dot_out, s);
      if (st != LHPC_ERR_UNSUPPORTED) return st;
    }
    // other kernel families: SpMV, then a separate dot pass
    LHPC_TRY(lhpc_spmv(p, x, y, 1, stream));
    return lhpc_vec_dot(p->dtype, p->n_rows, w, y, dot_out, stream);
  } LHPC_ABI_CATCH
}

namespace lhpc {
namespace {
// Which plans can take new values in place: those whose layout positions are
// a function of row_ptr alone.  XSLICE and XTILE column blocks place a value
// by its column, which the plan does not keep; a multi-device plan spans
// devices.  (Every part of a plan of parts has a part_col entry: a row part
// starts at column 0 and covers every column.)
int set_values_supported(const lhpc_spmv_plan *p) {
  if (p->multi) return LHPC_ERR_UNSUPPORTED;
  if (!p->parts.empty()) {
    int64_t sum = 0;
    for (size_t i = 0; i < p->parts.size(); ++i) {
      const lhpc_spmv_plan *q = p->parts[i];
      if (p->part_col[i] != 0 || q->n_cols != p->n_cols || q->xt_acc) return LHPC_ERR_UNSUPPORTED;
      sum += q->nnz;
    }
    return sum == p->nnz ? LHPC_OK : LHPC_ERR_UNSUPPORTED;
  }
  return p->kernel == LHPC_KERNEL_XSLICE ? LHPC_ERR_UNSUPPORTED : LHPC_OK;
}

// val in HBM of the plan's device; launches and asynchronous copies on s only
// (but for a SELL plan's first update, lhpc_spmv_csr.hip sell_set_values)
int set_values_device(lhpc_spmv_plan *p, const void *val, hipStream_t s) {
  const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
  if (!p->parts.empty()) {  // row parts: part i takes the values after the earlier parts'
    int64_t off = 0;
    for (const lhpc_spmv_plan *q : p->parts) {
      LHPC_TRY(xtile_set_values(q, static_cast<const unsigned char *>(val) + off * static_cast<int64_t>(tsz), s));
      off += q->nnz;
    }
    return LHPC_OK;
  }
  if (p->kernel == LHPC_KERNEL_XTILE) return xtile_set_values(p, val, s);
  if (p->kernel == LHPC_KERNEL_SELL) return sell_set_values(p, val, s);
  // ADAPTIVE / ROWGROUP: d_val is val in CSR order
  LHPC_HIP_TRY(hipMemcpyAsync(p->d_val, val, static_cast<size_t>(p->nnz) * tsz, hipMemcpyDeviceToDevice, s));
  return LHPC_OK;
}
}  // namespace
}  // namespace lhpc

extern "C" int lhpc_spmv_plan_set_values(lhpc_spmv_plan *p, const void *val, int64_t nnz, int values_on_device,
                                         void *stream) {
  try {
    if (!p || (nnz > 0 && !val) || nnz != p->nnz) return LHPC_ERR_INVALID_ARG;
    if (p->cg_busy.load()) return LHPC_ERR_BUSY;
    LHPC_TRY(set_values_supported(p));
    if (nnz == 0 || p->n_rows == 0) return LHPC_OK;
    RocTxRange rx("lhpc_spmv_plan_set_values");
    hipStream_t s = static_cast<hipStream_t>(stream);
    LHPC_HIP_TRY(hipSetDevice(p->device));
    const size_t bytes = static_cast<size_t>(nnz) * (p->dtype == LHPC_F32 ? 4 : 8);
    if (p->d_tperm) {
      // LHPC_PLAN_TRANSPOSE: val is in A's CSR order; gathered through the
      // plan's permutation into Aᵀ's order, then the family's update runs
      // from that buffer.  The buffer comes with the first update.
      if (!p->d_tval) {
        LHPC_TRY(dmalloc(&p->d_tval, bytes, p->bytes));
        LHPC_HIP_TRY(hipStreamSynchronize(s));
      }
      const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
      if (values_on_device) {
        LHPC_TRY(gather_values(p->d_tval, val, p->d_tperm, nnz, tsz, s));
        return set_values_device(p, p->d_tval, s);
      }
      void *tmp = nullptr;  // stream-ordered library scratch, freed before return
      LHPC_HIP_TRY(scratch_alloc(&tmp, bytes, s));
      hipError_t e = hipMemcpyAsync(tmp, val, bytes, hipMemcpyHostToDevice, s);
      int st = e == hipSuccess ? gather_values(p->d_tval, tmp, p->d_tperm, nnz, tsz, s) : static_cast<int>(e);
      if (st == LHPC_OK) st = set_values_device(p, p->d_tval, s);
      (void)hipFreeAsync(tmp, s);
      e = hipStreamSynchronize(s);
      return st != LHPC_OK ? st : static_cast<int>(e);
    }
    if (values_on_device) return set_values_device(p, val, s);
    if (p->parts.empty() && p->kernel != LHPC_KERNEL_XTILE && p->kernel != LHPC_KERNEL_SELL) {
      // CSR order in the plan too: straight into place
      LHPC_HIP_TRY(hipMemcpyAsync(p->d_val, val, bytes, hipMemcpyHostToDevice, s));
      LHPC_HIP_TRY(hipStreamSynchronize(s));
      return LHPC_OK;
    }
    void *tmp = nullptr;  // stream-ordered library scratch, freed before return
    LHPC_HIP_TRY(scratch_alloc(&tmp, bytes, s));
    hipError_t e = hipMemcpyAsync(tmp, val, bytes, hipMemcpyHostToDevice, s);
    const int st = e == hipSuccess ? set_values_device(p, tmp, s) : static_cast<int>(e);
    (void)hipFreeAsync(tmp, s);
    e = hipStreamSynchronize(s);
    return st != LHPC_OK ? st : static_cast<int>(e);
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmv_plan_info_get(const lhpc_spmv_plan *p, lhpc_spmv_plan_info *info) {
  try {
    if (!p || !info) return LHPC_ERR_INVALID_ARG;
    info->dtype = p->dtype;
    info->kernel = p->kernel;
    info->lanes_per_row = p->kernel == LHPC_KERNEL_ROWGROUP ? p->L : 0;
    info->rows_per_group = p->kernel == LHPC_KERNEL_ROWGROUP ? p->R : 0;
    info->n_rows = p->n_rows;
    info->n_cols = p->n_cols;
    info->nnz = p->nnz;
    info->n_blocks = p->n_blocks;
    info->n_long_rows = p->n_long;
    info->device_bytes = p->bytes;
    info->device = p->device;
    info->launches = p->kernel == LHPC_KERNEL_XSLICE ? 2 : 1;
    if (p->kernel == LHPC_KERNEL_XTILE) {
      info->launches = p->xt_mall > 1 ? 2 * p->xt_mall + (p->xt_cont > 0 ? 1 : 0)
                                      : (p->xt_pieces > 0 ? 1 : 0) + 1 + (p->xt_cont > 0 ? 1 : 0);
      info->n_blocks = p->xt_C;
      info->n_long_rows = p->xt_cont;
    }
    info->slices = p->S;
    info->slice_width = p->xs_width;
    if (p->kernel == LHPC_KERNEL_SELL) {  // 64-row slices, widest slice in nonzeros
      info->slices = static_cast<int>((p->n_rows + kWave - 1) / kWave);
      info->slice_width = p->sell_w;
    }
    if (!p->parts.empty()) {  // XTILE row parts: totals over the parts
      info->launches = 0;
      info->n_blocks = 0;
      info->n_long_rows = 0;
      for (const auto *q : p->parts) {
        lhpc_spmv_plan_info qi{};
        LHPC_TRY(lhpc_spmv_plan_info_get(q, &qi));
        info->launches += qi.launches;
        info->n_blocks += qi.n_blocks;
        info->n_long_rows += qi.n_long_rows;
      }
    }
    return LHPC_OK;
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmv_plan_destroy(lhpc_spmv_plan *p) {
  try {
    if (!p) return LHPC_OK;
    if (p->multi) multi_free(p);
    for (auto *q : p->parts) lhpc_spmv_plan_destroy(q);
    (void)hipSetDevice(p->device);
    for (void *q : {p->d_row_ptr, static_cast<void *>(p->d_col), p->d_val, static_cast<void *>(p->d_blocks),
                    p->d_xstage, p->d_ystage, p->d_lens, static_cast<void *>(p->d_cbase), p->d_partial,
                    static_cast<void *>(p->d_dpart), static_cast<void *>(p->d_cdesc), static_cast<void *>(p->d_cr),
                    static_cast<void *>(p->d_seghi), static_cast<void *>(p->d_seg), static_cast<void *>(p->d_pieces), static_cast<void *>(p->d_cont),
                    static_cast<void *>(p->d_col16), static_cast<void *>(p->d_perm), p->d_xg,
                    static_cast<void *>(p->d_pieces_cp), static_cast<void *>(p->d_pext),
                    static_cast<void *>(p->d_carry), static_cast<void *>(p->d_sell_rp),
                    static_cast<void *>(p->d_rec), static_cast<void *>(p->d_tperm), p->d_tval})
      if (q) (void)hipFree(q);
    if (p->h_scalars) (void)hipHostFree(p->h_scalars);
    for (hipGraphExec_t g : p->cg_graph)
      if (g) (void)hipGraphExecDestroy(g);
    if (p->cg_vecs) (void)hipFree(p->cg_vecs);
    if (p->cg_scal) (void)hipFree(p->cg_scal);
    if (p->bi_graph) (void)hipGraphExecDestroy(p->bi_graph);
    if (p->bi_host) (void)hipHostFree(p->bi_host);
    if (p->bi_vecs) (void)hipFree(p->bi_vecs);
    if (p->bi_scal) (void)hipFree(p->bi_scal);
    delete p;
    return LHPC_OK;
  } LHPC_ABI_CATCH
}

// Test support: FNV-1a digests of an XTILE plan's device layout, in the
// order row_ptr, col16, perm/iperm, val runs, chunk descriptors, cr, segment
// table (lo/len, hi), gather pieces, cont — so a test can byte-compare the
// layout built on the GPU from device input with the host build's.
extern "C" int lhpc_spmv_plan_layout_digest(const lhpc_spmv_plan *p, uint64_t *out, int cap, int *n_out) {
  try {
    if (!p || !out || !n_out || cap < 10) return LHPC_ERR_INVALID_ARG;
    if (p->kernel != LHPC_KERNEL_XTILE || p->multi) return LHPC_ERR_UNSUPPORTED;
    if (!p->parts.empty()) {  // row parts / column blocks: the parts' digests folded in order
      for (int i = 0; i < 10; ++i) out[i] = 0xcbf29ce484222325ull;
      for (size_t j = 0; j < p->parts.size(); ++j) {
        uint64_t d[10];
        int n = 0;
        LHPC_TRY(lhpc_spmv_plan_layout_digest(p->parts[j], d, 10, &n));
        const uint64_t where = static_cast<uint64_t>(p->part_row[j]) * 0x9E3779B97F4A7C15ull ^
                               static_cast<uint64_t>(p->part_col[j]) ^ static_cast<uint64_t>(p->parts[j]->xt_acc) << 63;
        for (int i = 0; i < 10; ++i) out[i] = (out[i] ^ d[i] ^ where) * 0x100000001b3ull;
      }
      *n_out = 10;
      return LHPC_OK;
    }
    LHPC_HIP_TRY(hipSetDevice(p->device));
    const size_t tsz = p->dtype == LHPC_F32 ? 4 : 8;
    const int64_t C = p->xt_C;
    const std::pair<const void *, size_t> arr[10] = {
        {p->d_row_ptr, static_cast<size_t>(p->n_rows + 1) * 4},
        {p->d_col16, static_cast<size_t>(p->xt_total) * 2},
        {p->d_perm, static_cast<size_t>(p->xt_p == 3 ? p->xt_nrun : p->xt_total + 2) * 2},
        {p->d_val, static_cast<size_t>(p->xt_nrun) * tsz},
        {p->d_cdesc, static_cast<size_t>(8 * C + 8) * 4},
        {p->d_cr, static_cast<size_t>(C + 1) * 4},
        {p->d_seg, static_cast<size_t>(p->xt_seg_n) * 4},  // segment table (or PRE: batch rank terms)
        {p->d_seghi, static_cast<size_t>(p->xt_seghi_n) * 4},
        {p->d_pieces, static_cast<size_t>(p->xt_pieces) * 12},
        {p->d_cont, static_cast<size_t>(p->xt_cont) * 4}};
    std::vector<unsigned char> h;
    for (int i = 0; i < 10; ++i) {
      h.resize(arr[i].second);
      if (arr[i].second) LHPC_HIP_TRY(hipMemcpy(h.data(), arr[i].first, arr[i].second, hipMemcpyDeviceToHost));
      uint64_t x = 0xcbf29ce484222325ull;
      for (unsigned char b : h) x = (x ^ b) * 0x100000001b3ull;
      out[i] = x ^ static_cast<uint64_t>(arr[i].second);
    }
    *n_out = 10;
    return LHPC_OK;
  } LHPC_ABI_CATCH
}

extern "C" int lhpc_spmv_plan_chunkrec(const lhpc_spmv_plan *p, int *on, uint64_t *digest) {
  try {
    if (!p || !on) return LHPC_ERR_INVALID_ARG;
    uint64_t x = 0xcbf29ce484222325ull;
    *on = 0;
    if (!p->parts.empty()) {
      for (const auto *q : p->parts) {
        int qon = 0;
        uint64_t qd = 0;
        LHPC_TRY(lhpc_spmv_plan_chunkrec(q, &qon, digest ? &qd : nullptr));
        *on |= qon;
        x = (x ^ qd) * 0x100000001b3ull;
      }
    } else if (p->kernel == LHPC_KERNEL_XTILE && p->xt_rec) {
      *on = 1;
      if (digest) {
        LHPC_HIP_TRY(hipSetDevice(p->device));
        std::vector<unsigned char> h(static_cast<size_t>(p->xt_rec_n) * 4);
        if (!h.empty()) LHPC_HIP_TRY(hipMemcpy(h.data(), p->d_rec, h.size(), hipMemcpyDeviceToHost));
        for (unsigned char b : h) x = (x ^ b) * 0x100000001b3ull;
        x ^= static_cast<uint64_t>(h.size());
      }
    }
    if (digest) *digest = x;
    return LHPC_OK;
  } LHPC_ABI_CATCH
}
