// rs_rep.hip — instantiates rs_kernel (redscat.hpp) for ONE element
// representation and exposes its launcher and occupancy query (rs_launch.hpp).
// Compiled once per Rep (see Makefile):
//   -DMPIGX_REP=<Rep> -DMPIGX_REP_NAME=<name> [-DMPIGX_RS_MINMAX_ONLY]
// Only what the dispatch can reach is built: NMAX 2 / 4 / 8, per schedule the
// full shape and the guarded one (5 kernels each), for the (op, type) pairs
// MPICH accepts.  A signed integer rep builds MIN / MAX only
// (-DMPIGX_RS_MINMAX_ONLY): the other ops give the same bits through the
// unsigned twin's kernels (device.hpp add_ / mul_), where the host sends them
// (mpigx.cpp rs_rep_for).
#include "redscat.hpp"

#ifndef MPIGX_REP
#error "compile with -DMPIGX_REP=<Rep> -DMPIGX_REP_NAME=<name>"
#endif
#define MPIGX_CAT2(a, b) a##b
#define MPIGX_CAT(a, b) MPIGX_CAT2(a, b)

namespace mpigx {
namespace {
using T = RepType<MPIGX_REP>::T;
[[maybe_unused]] constexpr bool kInt = is_int<T>::v;
[[maybe_unused]] constexpr bool kCplx = is_cplx<T>::v;

constexpr bool valid_op(int op) {
#ifdef MPIGX_RS_MINMAX_ONLY
  return op == O_MIN || op == O_MAX;
#else
  return op == O_SUM || op == O_PROD || (!kCplx && op >= O_MIN && op <= O_LXOR) ||
         (kInt && op >= O_BAND && op <= O_BXOR);
#endif
}

template <int K> struct OpOf;
template <> struct OpOf<O_SUM> { using type = OpSum; };
template <> struct OpOf<O_PROD> { using type = OpProd; };
template <> struct OpOf<O_MIN> { using type = OpMin; };
template <> struct OpOf<O_MAX> { using type = OpMax; };
template <> struct OpOf<O_LAND> { using type = OpLand; };
template <> struct OpOf<O_LOR> { using type = OpLor; };
template <> struct OpOf<O_LXOR> { using type = OpLxor; };
template <> struct OpOf<O_BAND> { using type = OpBand; };
template <> struct OpOf<O_BOR> { using type = OpBor; };
template <> struct OpOf<O_BXOR> { using type = OpBxor; };

// F(kernel) for the instantiation (nmax, shape) of schedule SCHED; the guarded
// shape is SH_PRE for the tree and SH_POW2 for the left fold (rs_shape)
#define MPIGX_RS_PICK(F)                                                              \
  constexpr int G = SCHED == S_TREE ? SH_PRE : SH_POW2;                               \
  if (nmax == 2) return F((rs_kernel<OP, T, 2, SCHED, SH_FULL, zc_u<T>(8)>));         \
  if (nmax == 4 && shape == SH_FULL) return F((rs_kernel<OP, T, 4, SCHED, SH_FULL, zc_u<T>(4)>)); \
  if (nmax == 4) return F((rs_kernel<OP, T, 4, SCHED, G, zc_u<T>(4)>));               \
  if (shape == SH_FULL) return F((rs_kernel<OP, T, 8, SCHED, SH_FULL, zc_u<T>(2)>));  \
  return F((rs_kernel<OP, T, 8, SCHED, G, zc_u<T>(2)>));

template <class OP, int SCHED>
hipError_t rs_sched(int nmax, int shape, dim3 grid, hipStream_t s, const FoldArgs& a) {
  auto go = [&](auto k) {
    hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, s, a);
    return hipGetLastError();
  };
  MPIGX_RS_PICK(go)
}
template <class OP, int SCHED>
int rs_occ_sched(int nmax, int shape) {
  auto occ = [&](auto k) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, kThreads, 0) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    return nb;
  };
  MPIGX_RS_PICK(occ)
}
#undef MPIGX_RS_PICK

template <int K>
hipError_t rs_op(int nmax, int sched, int shape, dim3 grid, hipStream_t s, const FoldArgs& a) {
  if constexpr (valid_op(K)) {
    using OP = typename OpOf<K>::type;
    return sched == S_LINEAR ? rs_sched<OP, S_LINEAR>(nmax, shape, grid, s, a)
                             : rs_sched<OP, S_TREE>(nmax, shape, grid, s, a);
  }
  return hipErrorInvalidValue;  // a missing kernel is an error, never a fall-back
}
template <int K>
int rs_occ_op(int nmax, int sched, int shape) {
  if constexpr (valid_op(K)) {
    using OP = typename OpOf<K>::type;
    return sched == S_LINEAR ? rs_occ_sched<OP, S_LINEAR>(nmax, shape) : rs_occ_sched<OP, S_TREE>(nmax, shape);
  }
  return 0;
}
}  // namespace

hipError_t MPIGX_CAT(launch_rs_, MPIGX_REP_NAME)(int op, int nmax, int sched, int shape, dim3 grid, hipStream_t s,
                                                const FoldArgs& a) {
  switch (op) {
    case O_SUM: return rs_op<O_SUM>(nmax, sched, shape, grid, s, a);
    case O_PROD: return rs_op<O_PROD>(nmax, sched, shape, grid, s, a);
    case O_MIN: return rs_op<O_MIN>(nmax, sched, shape, grid, s, a);
    case O_MAX: return rs_op<O_MAX>(nmax, sched, shape, grid, s, a);
    case O_LAND: return rs_op<O_LAND>(nmax, sched, shape, grid, s, a);
    case O_LOR: return rs_op<O_LOR>(nmax, sched, shape, grid, s, a);
    case O_LXOR: return rs_op<O_LXOR>(nmax, sched, shape, grid, s, a);
    case O_BAND: return rs_op<O_BAND>(nmax, sched, shape, grid, s, a);
    case O_BOR: return rs_op<O_BOR>(nmax, sched, shape, grid, s, a);
    case O_BXOR: return rs_op<O_BXOR>(nmax, sched, shape, grid, s, a);
    default: return hipErrorInvalidValue;
  }
}

int MPIGX_CAT(occupancy_rs_, MPIGX_REP_NAME)(int op, int nmax, int sched, int shape) {
  switch (op) {
    case O_SUM: return rs_occ_op<O_SUM>(nmax, sched, shape);
    case O_PROD: return rs_occ_op<O_PROD>(nmax, sched, shape);
    case O_MIN: return rs_occ_op<O_MIN>(nmax, sched, shape);
    case O_MAX: return rs_occ_op<O_MAX>(nmax, sched, shape);
    case O_LAND: return rs_occ_op<O_LAND>(nmax, sched, shape);
    case O_LOR: return rs_occ_op<O_LOR>(nmax, sched, shape);
    case O_LXOR: return rs_occ_op<O_LXOR>(nmax, sched, shape);
    case O_BAND: return rs_occ_op<O_BAND>(nmax, sched, shape);
    case O_BOR: return rs_occ_op<O_BOR>(nmax, sched, shape);
    case O_BXOR: return rs_occ_op<O_BXOR>(nmax, sched, shape);
    default: return 0;
  }
}

}  // namespace mpigx
