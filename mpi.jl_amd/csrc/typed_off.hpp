// typed_off.hpp — the one map from a packed stream to a derived datatype's
// memory layout, shared by the byte movers of copy.hip (seg_pack_kernel,
// typed_xfer_kernel) and the typed accumulate of kernels.hpp
// (acc_typed_kernel).
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace mpigx {

// Packed byte p of a stream of instances of one type -> byte offset from the
// typed buffer's pointer (pack_kernel's map: instance, run by binary search
// over the per-instance prefix, block, byte).  nruns = 0: contiguous.
__device__ __forceinline__ long long typed_off(const TypeRun* runs, const long long* pfx, int nruns, long long size,
                                               long long extent, long long p) {
  if (nruns == 0) return p;
  const long long k = p / size, r = p - k * size;
  int lo = 0;
  if (nruns > 1) {
    int hi = nruns - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pfx[mid] <= r) lo = mid;
      else hi = mid - 1;
    }
  }
  const TypeRun R = runs[lo];
  const long long q = r - pfx[lo], i = q / R.len, b = q - i * R.len;
  return k * extent + R.off + i * R.stride + b;
}

}  // namespace mpigx
