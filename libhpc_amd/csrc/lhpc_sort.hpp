// lhpc_sort.hpp — what lhpc_sort.hip lends to the other translation units
// (lhpc_transpose.hip): the 32-bit pair sort on device arrays, the key width
// of an index range, and the scratch / staging owners of the sort entry points.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lhpc_common.hpp"

namespace lhpc {

// stream-ordered library scratch (lhpc_common.hpp scratch_alloc), freed on
// the stream it was taken on
struct DevBuf {
  void *p = nullptr;
  hipStream_t s = nullptr;
  ~DevBuf() {
    if (p) (void)hipFreeAsync(p, s);
  }
  hipError_t alloc(size_t bytes, hipStream_t st) {
    s = st;
    return scratch_alloc(&p, bytes, st);  // library pool (lhpc_common.hpp)
  }
};

// Staging buffers of the host-buffer entry points: plain hipMalloc (not the
// stream-ordered pool) and synchronous copies.  Asynchronous pageable copies
// into pool memory on the null stream were seen to land after the kernel
// that read them (rows read as 0 in 4 of 25 runs of tests/cpp
// test_sparse_grid gpu, the 4-entry Matrix Market case).  Every step of that
// path was ordered on the one caller stream; DESIGN.md §9 traces it and
// records what was ruled out.
struct HostStage {
  void *p = nullptr;
  ~HostStage() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
};

// keys of the 32-bit pair sort's sub-tile (lhpc_radix_sort_pairs_u32: 1024
// threads × 16 pairs); a run of equal keys longer than this spans sub-tiles
constexpr int kSortPairsTile = 16384;

int bits_for(int64_t v);  // bits to hold values in [0, v)

// lhpc_radix_sort_pairs_u32 on device arrays: stable, in place, bits
// [begin_bit, end_bit) of the keys, asynchronous on s (n < 2^32; n ≤ 1 or an
// empty bit range leaves the arrays as they are)
int sort_pairs_u32_dev(uint32_t *keys, uint32_t *vals, int64_t n, int begin_bit, int end_bit, hipStream_t s);

}  // namespace lhpc
