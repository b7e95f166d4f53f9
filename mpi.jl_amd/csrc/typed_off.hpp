// typed_off.hpp — the one map from a packed stream to a derived datatype's
// memory layout, shared by the byte movers of copy.hip (seg_pack_kernel,
// typed_xfer_kernel), the typed accumulate and the typed fold of kernels.hpp
// (acc_typed_kernel, fold_typed_kernel).
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace mpigx {

// Where packed byte p of a stream of instances of one type lies: instance k,
// run `run` (binary search over the per-instance prefix), block i of that
// run, byte b of that block.  nruns >= 1.
struct TypedPos {
  long long k, i, b;
  int run;
};
__device__ __forceinline__ TypedPos typed_pos(const TypeRun* runs, const long long* pfx, int nruns, long long size,
                                              long long p) {
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
  const long long len = runs[lo].len;
  const long long q = r - pfx[lo], i = q / len, b = q - i * len;
  return TypedPos{k, i, b, lo};
}

// Packed byte p of a stream of instances of one type -> byte offset from the
// typed buffer's pointer (pack_kernel's map: instance, run by binary search
// over the per-instance prefix, block, byte).  nruns = 0: contiguous.
__device__ __forceinline__ long long typed_off(const TypeRun* runs, const long long* pfx, int nruns, long long size,
                                               long long extent, long long p) {
  if (nruns == 0) return p;
  const TypedPos t = typed_pos(runs, pfx, nruns, size, p);
  const TypeRun R = runs[t.run];
  return t.k * extent + R.off + t.i * R.stride + t.b;
}

}  // namespace mpigx
