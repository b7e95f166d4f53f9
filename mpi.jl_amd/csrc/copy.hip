// copy.hip — Bcast! / Allgather! / Alltoall! / Barrier (src/collective.jl:15-42,
// 295-335, 489-532) and the xGMI probe: byte movement through the staging
// arenas, block b of every rank owning the same byte slice, peers pulled over
// xGMI with all peers interleaved per thread (block_gather).
#include "kernels.hpp"
#include "launch.hpp"
#include "typed.hpp"
#include "typed_off.hpp"

namespace mpigx {

// NMAX = n rounded up to a power of two (2, 4, 8, 16) and U = 16 / NMAX
// 16-B vectors per peer per thread in flight (block_gather_u): ~16 loads
// outstanding per thread at every rank count (one per peer held the n = 2
// same-device Allgather at a third of HBM, VERDICT r02 / DESIGN §5).
template <int NMAX, int U>
__device__ __forceinline__ int copy_body(const CopyArgs& A);

template <int NMAX, int U>
__global__ __launch_bounds__(kThreads) void copy_kernel(CopyArgs A) {
  // per-rank arrays are indexed at run time: staged in LDS (kernels.hpp)
  __shared__ CopyArgs sA;
  static_assert(sizeof(CopyArgs) % 4 == 0, "CopyArgs word copy");
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&A);
  uint32_t* d = reinterpret_cast<uint32_t*>(&sA);
  for (unsigned i = threadIdx.x; i < sizeof(CopyArgs) / 4; i += blockDim.x) d[i] = w[i];
  __syncthreads();
  kernel_started(sA.pv);
  stamp(sA.pv, 0);
  const int ab = copy_body<NMAX, U>(sA);
  signal_done(sA.pv, ab);
}

// Slice b of chunk k of a chunked byte range: [k*chunk, (k+1)*chunk) ∩ [0,bytes).
__device__ __forceinline__ void chunk_slice(const CopyArgs& A, int k, int b, long long* lo, long long* hi) {
  const long long c0 = lmin((long long)k * A.chunk, A.bytes), c1 = lmin(c0 + A.chunk, A.bytes);
  *lo = lmin(c0 + (long long)b * A.slice, c1);
  *hi = lmin(*lo + A.slice, c1);
}

// one source -> one destination with U * 16 B per thread in flight
template <int U>
__device__ __forceinline__ void block_copy_u(char* dst, const char* src, long long len) {
  char* d[1] = {dst};
  const char* s[1] = {src};
  const long long l[1] = {len};
  block_gather_u<1, U>(d, s, l, 1);
}

// one source -> up to NMAX destinations (null = none): every 16-B vector is
// loaded once (U per thread in flight, unguarded: a lane past the end
// re-reads the last vector) and stored to each destination; unaligned
// operands go byte by byte
// (the pointers come from LDS: made wave-uniform, device.hpp wave_uniform)
template <int NMAX, int U>
__device__ __forceinline__ void block_relay_u(char* const (&outs)[NMAX], const char* src, long long len) {
  if (len <= 0) return;
  const long long tid = threadIdx.x, nt = blockDim.x;
  src = wave_uniform(src);
  char* o[NMAX];
  bool vec = ((uintptr_t)src & 15) == 0;
#pragma unroll
  for (int j = 0; j < NMAX; ++j) {
    o[j] = wave_uniform(outs[j]);
    if (o[j]) vec &= ((uintptr_t)o[j] & 15) == 0;
  }
  long long done = 0;
  if (vec) {
    const long long nv = len / 16;
    for (long long i = tid; i < nv; i += U * nt) {
      u32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long k = i + u * nt;
        v[u] = ld16(src + 16 * (k < nv ? k : nv - 1));
      }
#pragma unroll
      for (int j = 0; j < NMAX; ++j)
        if (o[j])
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (i + u * nt < nv) st16(o[j] + 16 * (i + u * nt), v[u]);
    }
    done = nv * 16;
  }
  for (long long k = done + tid; k < len; k += nt) {
    const char c = src[k];
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
      if (o[j]) o[j][k] = c;
  }
}

template <int NMAX, int U>
__device__ __forceinline__ int copy_body(const CopyArgs& A) {  // returns the zero-copy abort verdict
  const PeerView& pv = A.pv;
  const int b = blockIdx.x, r = pv.rank, n = pv.n;
  uint64_t ep = pv.epoch;
  if (A.mode == C_BARRIER) {
    rank_barrier(pv, ep);
    return 0;
  }
  const long long lo = lmin((long long)b * A.slice, A.bytes), hi = lmin(lo + A.slice, A.bytes);
  const long long len = hi - lo;
  char* mine = pv.stage[r];
  const char* send = (const char*)A.send;
  char* recv = (char*)A.recv;

  if (A.mode == C_PROBE_ALL || A.mode == C_PROBE_ONE) {
    // xGMI probe: pull A.bytes from every peer's staging, all peers
    // interleaved (PROBE_ALL: aggregate ingress), or from rank r+1 only
    // (PROBE_ONE: one link); loads folded into a register to stay live.
    if (!rank_barrier(pv, ep++)) return 0;
    const int m = A.mode == C_PROBE_ONE ? 1 : n - 1;
    const long long nv = len / 16;
    u32x4 acc = {0, 0, 0, 0};
    for (long long i = threadIdx.x; i < nv; i += blockDim.x) {
#pragma unroll
      for (int j = 0; j < NMAX; ++j)
        if (j < m) acc ^= ld16(pv.stage[(r + 1 + j) % n] + lo + 16 * i);
    }
    if (acc.x == 0x9e3779b9u && acc.y == 0x7f4a7c15u) reinterpret_cast<u32x4*>(mine)[threadIdx.x] = acc;
    rank_barrier_exit(pv, ep++);
    return 0;
  }
  if (A.mode == C_BCAST_LL || A.mode == C_ALLGATHER_LL || A.mode == C_ALLTOALL_LL) {
    // block b: lines of byte slice [lo, hi) of every rank's block; no barrier
    const long long tid = threadIdx.x, nt = blockDim.x;
    const unsigned flag = A.ll_flag;
    const long long l0 = lo / 8, l1 = hi > lo ? (hi + 7) / 8 : l0;
    const bool bc = A.mode == C_BCAST_LL, a2a = A.mode == C_ALLTOALL_LL;
    if (!bc || r == A.root) {
      for (long long i = l0 + tid; i < l1; i += nt)
        for (int p = 0; p < n; ++p)
          if (p != r) ll_put(A.ll_push[p], i, ll_pack8(a2a ? send + (long long)p * A.total : send, i, A.bytes), flag);
    } else if (b == 0 && tid == 0) {
      for (int p = 0; p < n; ++p)
        if (p != r) ll_put(A.ll_push[p], 0, 0, flag);  // token: "I am in this launch"
    }
    flush_remote_stores();
    if (!bc) {  // my own block (skipped in place)
      const char* own = a2a ? send + (long long)r * A.total : send;
      char* dst = recv + (long long)r * A.total;
      if (own != dst) block_copy(dst + lo, own + lo, len);
    }
    __syncthreads();  // IN_PLACE Alltoall: this slice of my blocks is read before peers' bytes land on it
    bool ok = true;
    const uint64_t t0 = wall_clock64();
    uint64_t next = kCancelPoll;  // one cancel-word read per kCancelPoll of waiting
    for (int p = 0; p < n && ok; ++p) {
      if (p == r) continue;
      const char* in = ll_from(pv, A.ll_in, p, A.ll_stride);
      uint64_t d;
      if (!bc || p == A.root) {
        char* dst = bc ? recv : recv + (long long)p * A.total;
        for (long long i = l0 + tid; i < l1 && ok; i += nt) {
          ok = ll_get(pv, in, i, flag, t0, next, &d);
          if (ok) ll_store8(dst, i, A.bytes, d);
        }
      } else if (b == 0 && tid == 0) {
        ok = ll_get(pv, in, 0, flag, t0, next, &d);
      }
    }
    if (!ok) __hip_atomic_store(pv.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return 0;
  }
  if (A.mode == C_BCAST) {
    // every non-root pulls from the root: the root's egress spreads over
    // its links by itself (one reader per link)
    if (r == A.root) block_copy(mine + lo, send + lo, len);
    if (!rank_barrier(pv, ep++)) return 0;
    if (r != A.root) block_copy_u<2 * U>(recv + lo, pv.stage[A.root] + lo, len);
    rank_barrier_exit(pv, ep++);
    return 0;
  }
  char* dsts[NMAX];
  const char* srcs[NMAX];
  long long lens[NMAX];
  if (A.mode == C_BCAST_SAG) {
    // scatter + allgather (block b owns slice b of every chunk): the root
    // stages everything; rank q pulls chunk q from the root into its own
    // staging; then every non-root pulls chunk p from rank p (the root's
    // chunk from the root, its own chunk locally).  Each root link carries
    // 2S/n, every other link S/n, instead of S on each root link.
    long long l, h;
    if (r == A.root)
      for (int k = 0; k < n; ++k) {
        chunk_slice(A, k, b, &l, &h);
        block_copy(mine + l, send + l, h - l);
      }
    if (!rank_barrier(pv, ep++)) return 0;
    if (r != A.root) {
      chunk_slice(A, r, b, &l, &h);
      block_copy(mine + l, pv.stage[A.root] + l, h - l);
    }
    if (!rank_barrier(pv, ep++)) return 0;
    if (r != A.root) {
      int m = 0;
#pragma unroll
      for (int j = 0; j < NMAX; ++j) {
        dsts[j] = nullptr;
        srcs[j] = nullptr;
        lens[j] = 0;
        if (j < n) {
          const int p = (r + j) % n;
          chunk_slice(A, p, b, &l, &h);
          dsts[j] = recv + l;
          srcs[j] = (p == r ? mine : pv.stage[p]) + l;
          lens[j] = h - l;
          m = j + 1;
        }
      }
      block_gather_u<NMAX, U>(dsts, srcs, lens, m);
    }
    rank_barrier_exit(pv, ep++);
    return 0;
  }
  if (A.mode == C_ALLGATHER) {
    block_copy(mine + lo, send + lo, len);
    if (!rank_barrier(pv, ep++)) return 0;
    // my own block (unless in place) + every peer's, interleaved
    int m = 0;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
      dsts[j] = nullptr;
      srcs[j] = nullptr;
      lens[j] = 0;
      if (j < n) {
        const int p = (r + j) % n;
        dsts[j] = recv + (long long)p * A.total + lo;
        srcs[j] = p == r ? mine + lo : pv.stage[p] + lo;
        lens[j] = (p == r && send + lo == dsts[j]) ? 0 : len;
        m = j + 1;
      }
    }
    block_gather_u<NMAX, U>(dsts, srcs, lens, m);
    rank_barrier_exit(pv, ep++);
    return 0;
  }
  if (A.mode == C_ALLGATHER_ZC) {
    // no staging: block p of my recvbuf <- rank p's block (its sendbuf, or
    // with IN_PLACE block p of its recvbuf: zsrc[p] points there); every
    // rank writes only blocks of its own recvbuf other than its own
    int ab;
    if (!zc_enter(pv, ep++, &ab)) return 0;
    if (!ab) {
      int m = 0;
#pragma unroll
      for (int j = 0; j < NMAX; ++j) {
        dsts[j] = nullptr;
        srcs[j] = nullptr;
        lens[j] = 0;
        if (j < n) {
          const int p = (r + j) % n;
          dsts[j] = recv + (long long)p * A.total + lo;
          srcs[j] = A.zsrc[p] + lo;
          lens[j] = srcs[j] == dsts[j] ? 0 : len;
          m = j + 1;
        }
      }
      block_gather_u<NMAX, U>(dsts, srcs, lens, m);
    }
    rank_barrier_exit(pv, ep++, &ab);
    return ab;
  }
  if (A.mode == C_BCAST_ZC) {
    // every non-root pulls the root's buffer (its IPC mapping) into its own
    int ab;
    if (!zc_enter(pv, ep++, &ab)) return 0;
    if (!ab && r != A.root) block_copy_u<2 * U>(recv + lo, A.zsrc[A.root] + lo, len);
    rank_barrier_exit(pv, ep++, &ab);
    return ab;
  }
  if (A.mode == C_BCAST_RELAY_ZC) {
    // relay: the n - 1 non-roots own the n - 1 chunks (owner i = root + 1 + i);
    // the owner pulls slice b of its chunk from the root's buffer and stores
    // it into its own buffer and every other non-root's (their mappings) in
    // the same pass.  Root links carry S/(n-1) out, every link between
    // non-roots S/(n-1) each way: one pass and one barrier fewer than the
    // scatter + allgather, whose root links carry 2S/n in two phases.  The
    // exit barrier is the fenced one: it publishes the stores into peers.
    long long l, h;
    int ab;
    if (!zc_enter(pv, ep++, &ab)) return 0;
    if (!ab && r != A.root) {
      chunk_slice(A, (r - A.root - 1 + n) % n, b, &l, &h);
      char* outs[NMAX];
#pragma unroll
      for (int j = 0; j < NMAX; ++j) {
        const int p = (r + j) % n;
        outs[j] = (j < n && p != A.root) ? (j == 0 ? recv : (char*)A.zsrc[p]) + l : nullptr;
      }
      block_relay_u<NMAX, NMAX <= 4 ? 8 : 4>(outs, A.zsrc[A.root] + l, h - l);
    }
    rank_barrier(pv, ep++, &ab);
    return ab;
  }
  if (A.mode == C_BCAST_SAG_ZC) {
    // scatter + allgather between the user buffers: rank q pulls chunk q from
    // the root into its own buffer, then chunk p from rank p's buffer.  Rank
    // q writes only chunks != q of its buffer after the scatter, and peers
    // read only its chunk q.
    long long l, h;
    int ab;
    if (!zc_enter(pv, ep++, &ab)) return 0;
    if (!ab && r != A.root) {
      chunk_slice(A, r, b, &l, &h);
      block_copy(recv + l, A.zsrc[A.root] + l, h - l);
    }
    if (!rank_barrier(pv, ep++, &ab)) return 0;
    if (!ab && r != A.root) {
      int m = 0;
#pragma unroll
      for (int j = 0; j < NMAX; ++j) {
        dsts[j] = nullptr;
        srcs[j] = nullptr;
        lens[j] = 0;
        if (j + 1 < n) {
          const int p = (r + 1 + j) % n;
          chunk_slice(A, p, b, &l, &h);
          dsts[j] = recv + l;
          srcs[j] = A.zsrc[p] + l;
          lens[j] = h - l;
          m = j + 1;
        }
      }
      block_gather_u<NMAX, U>(dsts, srcs, lens, m);
    }
    rank_barrier_exit(pv, ep++, &ab);
    return ab;
  }
  if (A.mode == C_ALLTOALL_ZC) {
    // no staging: block r of rank p's sendbuf -> block p of my recvbuf
    int ab;
    if (!zc_enter(pv, ep++, &ab)) return 0;  // every rank's sendbuf is ready
    if (!ab) {
    int m = 0;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
      dsts[j] = nullptr;
      srcs[j] = nullptr;
      lens[j] = 0;
      if (j < n) {
        const int p = (r + j) % n;
        dsts[j] = recv + (long long)p * A.total + lo;
        srcs[j] = A.zsrc[p] + (long long)r * A.total + lo;
        lens[j] = len;
        m = j + 1;
      }
    }
    block_gather_u<NMAX, U>(dsts, srcs, lens, m);
    }
    rank_barrier_exit(pv, ep++, &ab);  // nobody reads my sendbuf any more
    return ab;
  }
  // C_ALLTOALL: block p of my send goes to rank p; block j of my recv comes
  // from rank j's block r.  Staging blocks are A.sstride (16-B multiple) apart.
  for (int p = 0; p < n; ++p) block_copy(mine + (long long)p * A.sstride + lo, send + (long long)p * A.total + lo, len);
  if (!rank_barrier(pv, ep++)) return 0;
  int m = 0;
#pragma unroll
  for (int j = 0; j < NMAX; ++j) {
    dsts[j] = nullptr;
    srcs[j] = nullptr;
    lens[j] = 0;
    if (j < n) {
      const int p = (r + j) % n;
      dsts[j] = recv + (long long)p * A.total + lo;
      srcs[j] = pv.stage[p] + (long long)r * A.sstride + lo;
      lens[j] = len;
      m = j + 1;
    }
  }
  block_gather_u<NMAX, U>(dsts, srcs, lens, m);
  rank_barrier_exit(pv, ep++);
  return 0;
}

// ---------------------------------------------------------------------------
// v-collectives (collective.jl:90-578: Scatter!/Scatterv!/Gather!/Gatherv!/
// Allgatherv!/Alltoallv!) — SURVEY §8f next #1.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void round_slice(long long L, long long off, long long R, int G, int b, long long* lo,
                                            long long* hi) {
  long long len = L - off;
  if (len < 0) len = 0;
  if (len > R) len = R;
  const long long sl = ((len + G - 1) / G + 15) / 16 * 16;
  *lo = lmin((long long)b * sl, len);
  *hi = lmin(*lo + sl, len);
}

template <int NMAX, int U>
__device__ __forceinline__ void vx_body(const VArgs& A) {
  const PeerView& pv = A.pv;
  const int b = blockIdx.x, r = pv.rank, n = pv.n;
  uint64_t ep = pv.epoch;
  char* mine = pv.stage[r];
  for (int j = 0; j < A.ncopy; ++j) {
    long long lo, hi;
    round_slice(A.c_len[j], A.round_off, A.R, A.G, b, &lo, &hi);
    block_copy(mine + kSlotBase + (long long)A.c_slot[j] * A.R + lo, A.send + A.c_src[j] + A.round_off + lo, hi - lo);
  }
  if (!rank_barrier(pv, ep++)) return;
  char* dsts[NMAX];
  const char* srcs[NMAX];
  long long lens[NMAX];
  int m = 0;
#pragma unroll
  for (int j = 0; j < NMAX; ++j) {
    dsts[j] = nullptr;
    srcs[j] = nullptr;
    lens[j] = 0;
    if (j < n) {
      const int p = (r + j) % n;
      long long lo, hi;
      round_slice(A.p_len[p], A.round_off, A.R, A.G, b, &lo, &hi);
      dsts[j] = A.recv + A.p_dst[p] + A.round_off + lo;
      srcs[j] = pv.stage[p] + kSlotBase + (long long)A.p_slot[p] * A.R + lo;
      lens[j] = hi - lo;
      m = j + 1;
    }
  }
  block_gather_u<NMAX, U>(dsts, srcs, lens, m);
  rank_barrier_exit(pv, ep++);
}

template <int NMAX, int U>
__global__ __launch_bounds__(kThreads) void vx_kernel(VArgs A) {
  kernel_started(A.pv);
  vx_body<NMAX, U>(A);
  signal_done(A.pv);
}

hipError_t launch_vx(dim3 grid, hipStream_t s, const VArgs& a) {
  const int n = a.pv.n;
  if (n <= 2) hipLaunchKernelGGL((vx_kernel<2, 8>), grid, dim3(kThreads), 0, s, a);
  else if (n <= 4) hipLaunchKernelGGL((vx_kernel<4, 4>), grid, dim3(kThreads), 0, s, a);
  else if (n <= 8) hipLaunchKernelGGL((vx_kernel<8, 2>), grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((vx_kernel<16, 1>), grid, dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

// Point-to-point transfers (src/pointtopoint.jl): one launch moves every
// message matched in one progress pass; segment j owns blocks
// [blk0[j], blk0[j+1]) and is cut into equal 16-B-multiple slices.  The
// receiver pulls from the sender's (IPC-mapped) buffer, so writes stay local.
__global__ __launch_bounds__(kThreads) void xfer_kernel(XferArgs A) {
  pull_acquire(A.coherent);
  const int b = blockIdx.x;
  int j = 0;
  while (j + 1 < A.nseg && b >= A.blk0[j + 1]) ++j;
  const long long g = A.blk0[j + 1] - A.blk0[j], k = b - A.blk0[j];
  const long long slice = ((A.bytes[j] + g - 1) / g + 15) & ~15ll;
  const long long lo = lmin(k * slice, A.bytes[j]), hi = lmin(lo + slice, A.bytes[j]);
  block_copy(A.dst[j] + lo, A.src[j] + lo, hi - lo);
  pull_release(A.coherent);
}

hipError_t launch_xfer(hipStream_t s, const XferArgs& a) {
  hipLaunchKernelGGL(xfer_kernel, dim3(a.blk0[a.nseg]), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

// Derived-datatype pack / unpack (types.cpp): unit u = packed bytes
// [u*W, u*W+W) of the stream -> instance, run (binary search over the
// per-instance prefix), block, byte -> typed address.  Gather/scatter
// bound by HBM (or xGMI when `contig` is a peer's buffer).
template <int W>
__global__ __launch_bounds__(kThreads) void pack_kernel(PackArgs A) {
  pull_acquire(A.coherent);
  using V = typename std::conditional<W == 16, u32x4,
            typename std::conditional<W == 8, uint64_t,
            typename std::conditional<W == 4, uint32_t,
            typename std::conditional<W == 2, uint16_t, uint8_t>::type>::type>::type>::type;
  const long long nt = (long long)gridDim.x * blockDim.x;
  for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < A.units; u += nt) {
    const long long p = u * W;
    const long long k = p / A.size, r = p - k * A.size;
    int lo = 0;
    if (A.nruns > 1) {
      int hi = A.nruns - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (A.pfx[mid] <= r) lo = mid;
        else hi = mid - 1;
      }
    }
    const TypeRun R = A.runs[lo];
    const long long q = r - A.pfx[lo], i = q / R.len, b = q - i * R.len;
    const long long t = k * A.extent + R.off + i * R.stride + b;
    if (A.unpack) *reinterpret_cast<V*>(A.typed + t) = *reinterpret_cast<const V*>(A.contig + p);
    else *reinterpret_cast<V*>(A.contig + p) = *reinterpret_cast<const V*>(A.typed + t);
  }
  pull_release(A.coherent);
}

hipError_t launch_pack(hipStream_t s, const PackArgs& a) {
  long long g = (a.units + kThreads - 1) / kThreads;
  g = g < 1 ? 1 : (g > 4096 ? 4096 : g);
  switch (a.w) {
    case 16: hipLaunchKernelGGL(pack_kernel<16>, dim3((unsigned)g), dim3(kThreads), 0, s, a); break;
    case 8: hipLaunchKernelGGL(pack_kernel<8>, dim3((unsigned)g), dim3(kThreads), 0, s, a); break;
    case 4: hipLaunchKernelGGL(pack_kernel<4>, dim3((unsigned)g), dim3(kThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL(pack_kernel<2>, dim3((unsigned)g), dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL(pack_kernel<1>, dim3((unsigned)g), dim3(kThreads), 0, s, a); break;
  }
  return hipGetLastError();
}

// (typed_off, the packed-byte -> typed-offset map of the kernels below, lives
// in typed_off.hpp: the typed accumulate of kernels.hpp uses it too)

template <int W>
struct UnitOf {
  using type = typename std::conditional<W == 16, u32x4,
               typename std::conditional<W == 8, uint64_t,
               typename std::conditional<W == 4, uint32_t,
               typename std::conditional<W == 2, uint16_t, uint8_t>::type>::type>::type>::type;
};

// Segmented pack / unpack (typed.hpp SegPackArgs): every range of a
// v-collective's typed side in one launch.  Block b serves segment j with
// blk0[j] <= b < blk0[j+1] and, of that segment's units, the share
// [k*share, (k+1)*share) of its k-th block.
template <int W>
__global__ __launch_bounds__(kThreads) void seg_pack_kernel(SegPackArgs A) {
  pull_acquire(A.coherent);
  using V = typename UnitOf<W>::type;
  const int b = blockIdx.x;
  int j = 0;
  while (j + 1 < A.nseg && b >= A.blk0[j + 1]) ++j;
  const long long g = A.blk0[j + 1] - A.blk0[j], k = b - A.blk0[j];
  const long long share = (A.units[j] + g - 1) / g;
  const long long u0 = lmin(k * share, A.units[j]), u1 = lmin(u0 + share, A.units[j]);
  char* typed = A.typed + A.t_off[j];
  char* contig = A.contig + A.c_off[j];
  for (long long u = u0 + threadIdx.x; u < u1; u += blockDim.x) {
    const long long p = u * W;
    const long long t = typed_off(A.runs, A.pfx, A.nruns, A.size, A.extent, p);
    if (A.unpack) *reinterpret_cast<V*>(typed + t) = *reinterpret_cast<const V*>(contig + p);
    else *reinterpret_cast<V*>(contig + p) = *reinterpret_cast<const V*>(typed + t);
  }
  pull_release(A.coherent);
}

// Deals kSegGrid blocks to the non-empty segments in proportion to their
// units (at least one each; an empty segment gets none) and launches; nothing
// is launched when every segment is empty.
hipError_t launch_seg_pack(hipStream_t s, const SegPackArgs& in) {
  SegPackArgs a = in;
  long long total = 0;
  for (int j = 0; j < a.nseg; ++j) total += a.units[j];
  if (total <= 0) return hipSuccess;
  long long G = (total + kThreads - 1) / kThreads;
  G = G > kSegGrid ? kSegGrid : G;
  a.blk0[0] = 0;
  for (int j = 0; j < a.nseg; ++j) {
    long long g = 0;
    if (a.units[j] > 0) {
      g = (long long)((double)G * (double)a.units[j] / (double)total);
      const long long need = (a.units[j] + kThreads - 1) / kThreads;
      g = g > need ? need : g;
      g = g < 1 ? 1 : g;
    }
    a.blk0[j + 1] = a.blk0[j] + (int)g;
  }
  for (int j = a.nseg; j < kMaxRanks; ++j) a.blk0[j + 1] = a.blk0[a.nseg];
  const dim3 grid((unsigned)a.blk0[a.nseg]);
  switch (a.w) {
    case 16: hipLaunchKernelGGL(seg_pack_kernel<16>, grid, dim3(kThreads), 0, s, a); break;
    case 8: hipLaunchKernelGGL(seg_pack_kernel<8>, grid, dim3(kThreads), 0, s, a); break;
    case 4: hipLaunchKernelGGL(seg_pack_kernel<4>, grid, dim3(kThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL(seg_pack_kernel<2>, grid, dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL(seg_pack_kernel<1>, grid, dim3(kThreads), 0, s, a); break;
  }
  return hipGetLastError();
}

// Segmented pack / unpack with a type map per segment (typed.hpp SegWArgs):
// every block of an Alltoallw side in one launch.  Block b serves segment j
// with blk0[j] <= b < blk0[j+1] and the share [k*share, (k+1)*share) of that
// segment's units; the segment's fields are block-uniform, so the switch on
// its unit width does not diverge.
template <int W>
__device__ __forceinline__ void segw_move(char* typed, char* contig, const SegW& S, long long u0, long long u1,
                                          int unpack) {
  using V = typename UnitOf<W>::type;
  for (long long u = u0 + threadIdx.x; u < u1; u += blockDim.x) {
    const long long p = u * W;
    const long long t = typed_off(S.runs, S.pfx, S.nruns, S.size, S.extent, p);
    if (unpack) *reinterpret_cast<V*>(typed + t) = *reinterpret_cast<const V*>(contig + p);
    else *reinterpret_cast<V*>(contig + p) = *reinterpret_cast<const V*>(typed + t);
  }
}

__global__ __launch_bounds__(kThreads) void segw_pack_kernel(SegWArgs A) {
  pull_acquire(A.coherent);
  const int b = blockIdx.x;
  int j = 0;
  while (j + 1 < A.nseg && b >= A.blk0[j + 1]) ++j;
  const SegW S = A.seg[j];
  const long long g = A.blk0[j + 1] - A.blk0[j], k = b - A.blk0[j];
  const long long share = (S.units + g - 1) / g;
  const long long u0 = lmin(k * share, S.units), u1 = lmin(u0 + share, S.units);
  char* typed = A.typed + S.t_off;
  char* contig = A.contig + S.c_off;
  switch (S.w) {
    case 16: segw_move<16>(typed, contig, S, u0, u1, A.unpack); break;
    case 8: segw_move<8>(typed, contig, S, u0, u1, A.unpack); break;
    case 4: segw_move<4>(typed, contig, S, u0, u1, A.unpack); break;
    case 2: segw_move<2>(typed, contig, S, u0, u1, A.unpack); break;
    default: segw_move<1>(typed, contig, S, u0, u1, A.unpack); break;
  }
  pull_release(A.coherent);
}

// Deals kSegGrid blocks to the non-empty segments in proportion to their
// BYTES (their units are of different widths): at least one block each, never
// more than a segment's units fill, none for an empty segment.  Nothing is
// launched when every segment is empty.
hipError_t launch_segw_pack(hipStream_t s, const SegWArgs& in) {
  SegWArgs a = in;
  if (a.nseg < 0 || a.nseg > kMaxRanks) return hipErrorInvalidValue;
  long long total = 0, want = 0;
  for (int j = 0; j < a.nseg; ++j) {
    if (a.seg[j].units <= 0) continue;
    total += a.seg[j].units * a.seg[j].w;
    want += (a.seg[j].units + kThreads - 1) / kThreads;
  }
  if (total <= 0) return hipSuccess;
  const long long G = want > kSegGrid ? kSegGrid : want;
  a.blk0[0] = 0;
  for (int j = 0; j < a.nseg; ++j) {
    long long g = 0;
    if (a.seg[j].units > 0) {
      g = (long long)((double)G * (double)(a.seg[j].units * a.seg[j].w) / (double)total);
      const long long need = (a.seg[j].units + kThreads - 1) / kThreads;
      g = g > need ? need : g;
      g = g < 1 ? 1 : g;
    }
    a.blk0[j + 1] = a.blk0[j] + (int)g;
  }
  for (int j = a.nseg; j < kMaxRanks; ++j) a.blk0[j + 1] = a.blk0[a.nseg];
  hipLaunchKernelGGL(segw_pack_kernel, dim3((unsigned)a.blk0[a.nseg]), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

// Typed -> typed transfer (typed.hpp TypedXferArgs): unit u of the packed
// stream is read at src through the source map and written at dst through the
// destination map, one pass.  The destination is always local memory; the
// source may be a peer's (IPC-mapped) buffer, hence xfer_kernel's bracket.
template <int W>
__global__ __launch_bounds__(kThreads) void typed_xfer_kernel(TypedXferArgs A) {
  // run lists that arrived as arguments are searched with per-lane indices:
  // staged in LDS (kernel arguments indexed at run time would go to scratch)
  __shared__ TypeRun sruns[kInlineRuns];
  __shared__ long long spfx[kInlineRuns + 1];
  if (A.s.inl | A.d.inl) {
    for (int i = threadIdx.x; i < kInlineRuns; i += blockDim.x) sruns[i] = A.iruns[i];
    for (int i = threadIdx.x; i <= kInlineRuns; i += blockDim.x) spfx[i] = A.ipfx[i];
    __syncthreads();
  }
  pull_acquire(A.coherent);
  using V = typename UnitOf<W>::type;
  const TypeRun* sr = A.s.inl ? sruns : A.s.runs;
  const long long* sp = A.s.inl ? spfx : A.s.pfx;
  const TypeRun* dr = A.d.inl ? sruns : A.d.runs;
  const long long* dp = A.d.inl ? spfx : A.d.pfx;
  const long long nt = (long long)gridDim.x * blockDim.x;
  for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < A.units; u += nt) {
    const long long p = u * W;
    const long long so = typed_off(sr, sp, A.s.nruns, A.s.size, A.s.extent, p);
    const long long dO = typed_off(dr, dp, A.d.nruns, A.d.size, A.d.extent, p);
    *reinterpret_cast<V*>(A.dst + dO) = *reinterpret_cast<const V*>(A.src + so);
  }
  pull_release(A.coherent);
}

hipError_t launch_typed_xfer(hipStream_t s, const TypedXferArgs& a) {
  if (a.units <= 0) return hipSuccess;
  if (a.s.inl && a.d.inl) return hipErrorInvalidValue;  // one inline run list per launch
  long long g = (a.units + kThreads - 1) / kThreads;
  g = g > kSegGrid ? kSegGrid : g;
  const dim3 grid((unsigned)g);
  switch (a.w) {
    case 16: hipLaunchKernelGGL(typed_xfer_kernel<16>, grid, dim3(kThreads), 0, s, a); break;
    case 8: hipLaunchKernelGGL(typed_xfer_kernel<8>, grid, dim3(kThreads), 0, s, a); break;
    case 4: hipLaunchKernelGGL(typed_xfer_kernel<4>, grid, dim3(kThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL(typed_xfer_kernel<2>, grid, dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL(typed_xfer_kernel<1>, grid, dim3(kThreads), 0, s, a); break;
  }
  return hipGetLastError();
}

hipError_t launch_copy(dim3 grid, hipStream_t s, const CopyArgs& a) {
  const int n = a.pv.n;
  if (n <= 2) hipLaunchKernelGGL((copy_kernel<2, 8>), grid, dim3(kThreads), 0, s, a);
  else if (n <= 4) hipLaunchKernelGGL((copy_kernel<4, 4>), grid, dim3(kThreads), 0, s, a);
  else if (n <= 8) hipLaunchKernelGGL((copy_kernel<8, 2>), grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((copy_kernel<16, 1>), grid, dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Read-only stream of nin HBM buffers (mpigx_diag.h mpigx_read_probe): the
// ceiling of config 2's fold on the box it runs on.  Same access layout as
// fold_local_kernel<SH_FULL, U = 4> (thread t of block b reads the four
// 16-B vectors (4b+u)*256 + t of every input, all nin x 4 non-temporal loads
// in flight before any use) with the fold and the store removed: the loads
// are XOR-ed into a register that is stored only if it equals a value it
// never takes, so the compiler keeps every load and the kernel writes nothing.
// ---------------------------------------------------------------------------
struct ReadProbeArgs {
  const char* in[kMaxRanks];
  int nin;
  long long nvec;  // 16-B vectors per input
  u32x4* sink;
};
template <int NIN>
__global__ __launch_bounds__(kThreads) void read_probe_kernel(ReadProbeArgs A) {
  constexpr int U = 4;
  u32x4 acc = {0, 0, 0, 0};
  const long long step = (long long)gridDim.x * (U * kThreads);
  for (long long v0 = (long long)blockIdx.x * (U * kThreads) + threadIdx.x; v0 < A.nvec; v0 += step) {
    u32x4 x[U][NIN];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int s = 0; s < NIN; ++s) {
        const long long k = v0 + (long long)u * kThreads;
        x[u][s] = ld16(A.in[s] + 16 * (k < A.nvec ? k : A.nvec - 1));
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int s = 0; s < NIN; ++s) acc ^= x[u][s];
  }
  if (acc.x == 0x9e3779b9u && acc.y == 0x7f4a7c15u && acc.z == 0x85ebca6bu) A.sink[threadIdx.x] = acc;
}

hipError_t launch_read_probe(const void* const* in, int nin, long long bytes, void* sink, hipStream_t s) {
  ReadProbeArgs a;
  for (int k = 0; k < kMaxRanks; ++k) a.in[k] = k < nin ? (const char*)in[k] : nullptr;
  a.nin = nin;
  a.nvec = bytes / 16;
  a.sink = (u32x4*)sink;
  const long long g = (a.nvec + 4 * kThreads - 1) / (4 * kThreads);
  const dim3 grid((unsigned)(g < 1 ? 1 : g > (1ll << 30) ? (1ll << 30) : g));
  switch (nin) {
    case 1: hipLaunchKernelGGL(read_probe_kernel<1>, grid, dim3(kThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL(read_probe_kernel<2>, grid, dim3(kThreads), 0, s, a); break;
    case 4: hipLaunchKernelGGL(read_probe_kernel<4>, grid, dim3(kThreads), 0, s, a); break;
    case 8: hipLaunchKernelGGL(read_probe_kernel<8>, grid, dim3(kThreads), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 8-read : 1-write stream (mpigx_diag.h mpigx_mix_probe): config 2's own
// ceiling on the box it runs on.  The read probe above
// measures the inputs alone; the fold also writes 256 MiB, and the box's rate
// for that mix is what bounds it.  Same layout, loads and stores as
// fold_local_kernel<SH_FULL, U = 4>: thread t of block b loads the four 16-B
// vectors (4b+u)*256 + t of every input (all nin x 4 loads in flight first),
// then stores, per vector, the XOR of its nin loads with the fold's
// write-through buffer store (stv_wt).  XOR is one VALU op per dword, so what
// is left of the fold is its memory traffic and its load -> store dependence.
// ---------------------------------------------------------------------------
struct MixProbeArgs {
  const char* in[kMaxRanks];
  long long nvec;  // 16-B vectors per input (and of the output)
  char* out;
};
template <int NIN>
__global__ __launch_bounds__(kThreads) void mix_probe_kernel(MixProbeArgs A) {
  constexpr int U = 4;
  const long long tid = threadIdx.x;
  const long long step = (long long)gridDim.x * (U * kThreads);
  for (long long v0 = (long long)blockIdx.x * (U * kThreads) + tid; v0 < A.nvec; v0 += step) {
    if (v0 + (long long)(U - 1) * kThreads < A.nvec) {
      u32x4 x[U][NIN];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int s = 0; s < NIN; ++s) x[u][s] = ld16(A.in[s] + 16 * (v0 + (long long)u * kThreads));
      const __amdgpu_buffer_rsrc_t span = span_rsrc(A.out + 16 * (v0 - tid), U * kThreads * 16);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        Vec<unsigned, 4> r;
        u32x4 a = x[u][0];
#pragma unroll
        for (int s = 1; s < NIN; ++s) a ^= x[u][s];
        *reinterpret_cast<u32x4*>(r.x) = a;
        stv_wt<unsigned, 4>(span, (int)(tid + u * kThreads) * 16, r);
      }
    } else {
      for (int u = 0; u < U; ++u) {
        const long long k = v0 + (long long)u * kThreads;
        if (k >= A.nvec) break;
        u32x4 a = ld16(A.in[0] + 16 * k);
        for (int s = 1; s < NIN; ++s) a ^= ld16(A.in[s] + 16 * k);
        st16(A.out + 16 * k, a);
      }
    }
  }
}

hipError_t launch_mix_probe(const void* const* in, int nin, long long bytes, void* out, hipStream_t s) {
  MixProbeArgs a;
  for (int k = 0; k < kMaxRanks; ++k) a.in[k] = k < nin ? (const char*)in[k] : nullptr;
  a.nvec = bytes / 16;
  a.out = (char*)out;
  const long long g = (a.nvec + 4 * kThreads - 1) / (4 * kThreads);
  const dim3 grid((unsigned)(g < 1 ? 1 : g > (1ll << 30) ? (1ll << 30) : g));
  switch (nin) {
    case 1: hipLaunchKernelGGL(mix_probe_kernel<1>, grid, dim3(kThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL(mix_probe_kernel<2>, grid, dim3(kThreads), 0, s, a); break;
    case 4: hipLaunchKernelGGL(mix_probe_kernel<4>, grid, dim3(kThreads), 0, s, a); break;
    case 8: hipLaunchKernelGGL(mix_probe_kernel<8>, grid, dim3(kThreads), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// Resident 256-thread blocks per CU of the byte movers that spin on their
// peers (copy_kernel, vx_kernel) of an n-rank communicator; 0 if unknown.
template <class K>
int occ_k(K k) {
  int v = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k, kThreads, 0) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return v;
}
int occupancy_copy(int n) {
  if (n <= 2) return occ_k(copy_kernel<2, 8>);
  if (n <= 4) return occ_k(copy_kernel<4, 4>);
  if (n <= 8) return occ_k(copy_kernel<8, 2>);
  return occ_k(copy_kernel<16, 1>);
}
int occupancy_vx(int n) {
  if (n <= 2) return occ_k(vx_kernel<2, 8>);
  if (n <= 4) return occ_k(vx_kernel<4, 4>);
  if (n <= 8) return occ_k(vx_kernel<8, 2>);
  return occ_k(vx_kernel<16, 1>);
}

}  // namespace mpigx
