// rs_launch.hpp — host-side entry points into the reduce-scatter kernels
// (redscat.hpp rs_kernel, instantiated per representation by rs_rep.hip).
// A header of its own beside launch.hpp: the 75 kernel objects of kern_rep.hip
// do not depend on it.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace mpigx {

// FoldArgs.mode of rs_kernel (the FoldMode values of fold_kernel end at 10).
//   M_RS_ZC  : entry barrier (view check), fold slice b of my block straight
//              from every rank's mapped sendbuf, exit barrier
//   M_RS_PUSH: block p of my sendbuf -> rank p's arena slot [me], barrier,
//              fold my block from my own slots, barrier
constexpr int M_RS_ZC = 11, M_RS_PUSH = 12;

// MPICH 3.3.2 MPIR_Reduce_scatter(_block)_intra_auto: recursive halving below
// this many bytes of all blocks together, pairwise exchange from it up
// (commutative ops).
constexpr long long kRsPairwiseMin = 524288;

// rs_kernel instantiation for n <= 8 ranks: NMAX = n rounded up to a power of
// two; the tree takes SH_FULL when every leaf is present without a pre-step,
// else SH_PRE; the left fold SH_FULL or SH_POW2 (no pre-step partners).
inline bool rs_shape(int n, int sched, int ntree, int rem, int* nmax, int* shape) {
  if (n < 2 || n > 8) return false;
  *nmax = n <= 2 ? 2 : n <= 4 ? 4 : 8;
  if (sched == S_TREE) *shape = (rem == 0 && ntree == *nmax) ? SH_FULL : SH_PRE;
  else *shape = ntree == *nmax ? SH_FULL : SH_POW2;
  return true;
}

// Elements per block slice of a block of `len` elements cut for `grid` blocks:
// ONE rule for the sender of a block (M_RS_PUSH phase 1) and its owner (the
// fold), so block b of the owner reads what block b of every sender stored.
__host__ __device__ inline long long rs_slice(long long len, long long grid, int w) {
  const long long s = (len + grid - 1) / grid;
  return (s + w - 1) / w * w;
}

using RsLauncher = hipError_t (*)(int op, int nmax, int sched, int shape, dim3 grid, hipStream_t s, const FoldArgs& a);
// resident blocks per CU of the rs_kernel instantiation (it spins on its peers)
using RsOccQuery = int (*)(int op, int nmax, int sched, int shape);

#define MPIGX_DECL_RS(NAME)                                                                                        \
  hipError_t launch_rs_##NAME(int op, int nmax, int sched, int shape, dim3 grid, hipStream_t s, const FoldArgs& a); \
  int occupancy_rs_##NAME(int op, int nmax, int sched, int shape);
MPIGX_DECL_RS(i8) MPIGX_DECL_RS(u8) MPIGX_DECL_RS(i16) MPIGX_DECL_RS(u16)
MPIGX_DECL_RS(i32) MPIGX_DECL_RS(u32) MPIGX_DECL_RS(i64) MPIGX_DECL_RS(u64)
MPIGX_DECL_RS(f32) MPIGX_DECL_RS(f64) MPIGX_DECL_RS(c64) MPIGX_DECL_RS(c128)
MPIGX_DECL_RS(bf16)
#undef MPIGX_DECL_RS

}  // namespace mpigx
