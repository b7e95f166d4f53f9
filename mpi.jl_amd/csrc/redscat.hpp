// redscat.hpp — Reduce_scatter_block / Reduce_scatter in a kernel of their own.
//
// Rank r receives the reduction of block r of every rank's sendbuf and nothing
// else: the first half of the two-shot Allreduce without its mid barrier and
// allgather.  The host resolves everything per rank (mpigx.cpp
// reduce_scatter_common): src[s] / src2[j] are the fold's leaves already
// offset to the start of MY block (this round of it), so element e of the
// block is src[s][e] in every source and out[e] in the output.
//
//   M_RS_ZC   entry barrier (zc_enter, the view check) -> fold slice b of my
//             block straight from every rank's IPC-mapped sendbuf -> exit
//             barrier (nobody reads my sendbuf any more).  Two epochs.
//   M_RS_PUSH below MPIGX_ZC_MIN: slice b of block p of my sendbuf -> rank p's
//             arena slot [me] (remote stores; my own block into my own slot)
//             -> barrier -> fold my block from my slots (local HBM) -> barrier
//             (nobody writes my slots before I have read them).  No entry
//             barrier, like the push two-shot: the peers' previous launch
//             ended with a barrier of every block.
//   In place (A.own, both modes): the result goes to the start of the buffer
//             that is also the input.  What my block b would store there is
//             read by other ranks through the mapping (zero-copy) and by other
//             blocks of my own rank (my own leaf; phase 1 of the staged path),
//             in whichever block THEIR partition puts it — with unequal counts
//             not block b, so the per-block barriers order nothing.  The fold
//             therefore goes into a private temporary (A.recv), a whole-launch
//             barrier (rank_barrier_grid: every block of every rank) replaces
//             the exit barrier, and then slice b is copied to the user's
//             buffer (A.send).  Two epochs; only the in-place form pays for
//             the extra local copy.
//
// Two schedules (MPICH 3.3.2, restated in tests/redscat_model.py):
//   S_TREE    recursive halving: a balanced tree per destination over a
//             permutation of the leaves (leaf i = new rank d ^ bitrev(i)), the
//             lower leaf inout; pre-step partner j (src2[j], the even rank)
//             folds as `in` into leaf leaf2_rank[j] (the odd rank) — the
//             partners are not the first `rem` leaves as in the Allreduce's
//             tree, hence a fold of its own here.
//   S_LINEAR  left fold over src[0..ntree): pairwise exchange (leaves rotated
//             and reversed from r) and MPIGX_ORDER_LINEAR (rank order).
//
// NMAX (2, 4, 8) is a compile-time constant and U = 16 / NMAX vectors per
// thread keep ~16 loads in flight (the rule of ar_zc_kernel).
#pragma once
#include "kernels.hpp"
#include "rs_launch.hpp"

namespace mpigx {

template <class OP, class T, int NMAX, int SCHED, int SHAPE, int W>
__device__ __forceinline__ void rs_fold_leaves(const FoldArgs& A, Leaves<T, NMAX, SHAPE, W>& L, Vec<T, W>& res) {
  auto& v = L.v;
  const int nt = ntree_of<NMAX, SHAPE>(A);
  if constexpr (SCHED == S_LINEAR) {
#pragma unroll
    for (int s = 1; s < NMAX; ++s)
      if (s < nt) vapply<OP, T, W>(v[0], v[0], v[s]);
  } else {
    if constexpr (SHAPE == SH_PRE) {
      // the partner's leaf is a runtime value: compared against every leaf
      // (wave-uniform branches), never used as an index into the registers
#pragma unroll
      for (int j = 0; j < NMAX / 2; ++j)
        if (j < A.rem) {
          const int t = A.leaf2_rank[j];
#pragma unroll
          for (int s = 0; s < NMAX; ++s)
            if (s == t) vapply<OP, T, W>(v[s], v[s], L.u[j]);  // inout = odd rank 2q+1, in = even rank 2q
        }
    }
    fold_tree<OP, T, NMAX, W, 0>(nt, v);
  }
  res = v[0];
}

// Fold [lo, hi) of my block into out, the block cooperating; `vec`: every
// pointer involved is 16-B aligned (lo is a multiple of the vector width).
template <class OP, class T, int NMAX, int SCHED, int SHAPE, int U>
__device__ __forceinline__ void rs_span(const FoldArgs& A, const T* const* src, const T* const* src2, long long lo,
                                        long long hi, T* out, bool vec) {
  constexpr int W = VecW<T>::v;
  const long long tid = threadIdx.x, nt = blockDim.x;
  long long e0 = lo;
  if (vec) {
    const long long nv = (hi - lo) / W;
    long long v0 = tid;
    for (; v0 + (long long)(U - 1) * nt < nv; v0 += U * nt) {
      Leaves<T, NMAX, SHAPE, W> L[U];
#pragma unroll
      for (int u = 0; u < U; ++u) load_leaves<T, NMAX, SCHED, SHAPE, W>(A, src, src2, lo + (v0 + u * nt) * W, L[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        Vec<T, W> r;
        rs_fold_leaves<OP, T, NMAX, SCHED, SHAPE, W>(A, L[u], r);
        stv<T, W>(out + lo + (v0 + u * nt) * W, r);
      }
    }
    for (; v0 < nv; v0 += nt) {
      Leaves<T, NMAX, SHAPE, W> L;
      load_leaves<T, NMAX, SCHED, SHAPE, W>(A, src, src2, lo + v0 * W, L);
      Vec<T, W> r;
      rs_fold_leaves<OP, T, NMAX, SCHED, SHAPE, W>(A, L, r);
      stv<T, W>(out + lo + v0 * W, r);
    }
    e0 = lo + nv * W;
  }
  // unaligned operands (a block at an odd displacement) and the ragged tail
#pragma unroll 1
  for (long long e = e0 + tid; e < hi; e += nt) {
    Leaves<T, NMAX, SHAPE, 1> L;
    load_leaves<T, NMAX, SCHED, SHAPE, 1>(A, src, src2, e, L);
    Vec<T, 1> r;
    rs_fold_leaves<OP, T, NMAX, SCHED, SHAPE, 1>(A, L, r);
    out[e] = r.x[0];
  }
}

template <class OP, class T, int NMAX, int SCHED, int SHAPE, int U>
__global__ __launch_bounds__(kThreads) void rs_kernel(FoldArgs A0) {
  __shared__ FoldArgs A;  // indexed by runtime ranks below (see fold_kernel)
  {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&A0);
    uint32_t* d = reinterpret_cast<uint32_t*>(&A);
    for (unsigned i = threadIdx.x; i < sizeof(FoldArgs) / 4; i += blockDim.x) d[i] = w[i];
    __syncthreads();
  }
  constexpr int W = VecW<T>::v;
  const PeerView& pv = A.pv;
  const T* const* src = reinterpret_cast<const T* const*>(A.src);
  const T* const* src2 = reinterpret_cast<const T* const*>(A.src2);
  T* out = (T*)A.recv;
  const int n = pv.n, r = pv.rank, b = blockIdx.x, es = A.esize;
  uint64_t ep = pv.epoch;
  int ab = 0;
  kernel_started(pv);
  stamp(pv, 0);
  if (A.mode == M_RS_PUSH) {
    // phase 1 stores into the peers' arenas before any barrier (zc_enter's checks)
    if (args_fault(pv)) {
      if (threadIdx.x == 0) __hip_atomic_store(pv.err, kErrProtocol, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      signal_done(pv, 0);
      return;
    }
    stamp(pv, 1);
    // zc_recv[p]: block p of my sendbuf (this round), zc_avail[p]: its bytes
    char* dsts[NMAX];
    const char* srcs[NMAX];
    long long lens[NMAX];
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
      dsts[j] = nullptr;
      srcs[j] = nullptr;
      lens[j] = 0;
      if (j < n) {
        const int p = (r + j) % n;
        const long long ce = A.zc_avail[p] / es;
        const long long psl = rs_slice(ce, gridDim.x, W);
        const long long l2 = lmin((long long)b * psl, ce), h2 = lmin(l2 + psl, ce);
        dsts[j] = pv.stage[p] + (long long)r * A.slot_bytes + l2 * es;
        srcs[j] = A.zc_recv[p] + l2 * es;
        lens[j] = (h2 - l2) * es;
      }
    }
    block_gather<NMAX>(dsts, srcs, lens, n);
    stamp(pv, 2);
    if (!rank_barrier(pv, ep++)) {  // every rank's slice b of my block is in my slots
      signal_done(pv, 0);
      return;
    }
    stamp(pv, 3);
  } else {
    if (!zc_enter(pv, ep++, &ab)) {  // every rank's sendbuf is ready, one view
      signal_done(pv, 0);
      return;
    }
    stamp(pv, 1);
  }
  const long long lo = lmin((long long)b * A.slice, A.count), hi = lmin(lo + A.slice, A.count);
  if (!ab) {
    bool vec = ((uintptr_t)out & 15) == 0;
#pragma unroll
    for (int s = 0; s < NMAX; ++s)
      if (s < A.ntree) vec &= ((uintptr_t)A.src[s] & 15) == 0;
    if constexpr (SHAPE == SH_PRE && SCHED == S_TREE) {
#pragma unroll
      for (int s = 0; s < NMAX / 2; ++s)
        if (s < A.rem) vec &= ((uintptr_t)A.src2[s] & 15) == 0;
    }
    rs_span<OP, T, NMAX, SCHED, SHAPE, U>(A, src, src2, lo, hi, out, vec);
  }
  if (A.own) {
    // in place (either mode): `out` is my temporary.  The user's buffer
    // (A.send) is written only once EVERY block of EVERY rank has finished
    // reading: the region my block b stores is read by whichever block of its
    // owner (or of my own rank, phase 1 / my own leaf) the owner's partition
    // puts there, so a barrier among the blocks b would not do.
    stamp(pv, 2);
    if (!rank_barrier_grid(pv, ep++, &ab)) {
      signal_done(pv, 0);
      return;
    }
    stamp(pv, 3);
    if (!ab) block_copy((char*)A.send + lo * es, (const char*)(out + lo), (hi - lo) * es);
    stamp(pv, 4);
    stamp(pv, 5);
    // no exit barrier: after the whole-launch one nobody reads my buffer or my slots
    signal_done(pv, ab);
    return;
  }
  if (A.mode == M_RS_ZC) {
    stamp(pv, 2);
    stamp(pv, 3);
  }
  stamp(pv, 4);
  if (rank_barrier_exit(pv, ep++, &ab)) stamp(pv, 5);  // nobody reads my sendbuf / writes my slots any more
  signal_done(pv, ab);
}

}  // namespace mpigx
