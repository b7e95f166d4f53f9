// typed.hpp — arguments and launchers of the derived-datatype kernels of the
// v-collectives and of one-sided Get / Put (copy.hip).  Kept apart from
// common.hpp so that only copy.hip and the host runtime depend on it, not the
// per-representation kernel objects.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace mpigx {

// Segmented pack (typed -> packed) / unpack of up to kMaxRanks ranges of ONE
// typed buffer in one launch (Gatherv / Scatterv / Allgatherv / Alltoallv:
// range p = the block of rank p).  Segment j = `units[j]` W-byte units whose
// first instance lies at typed + t_off[j] and whose packed bytes start at
// contig + c_off[j]; it owns blocks [blk0[j], blk0[j+1]) (dealt in proportion
// to its bytes, as xfer_kernel's), each of which takes an equal share of the
// segment's units.  Inside a segment the map is pack_kernel's.
constexpr int kSegGrid = 4096;  // blocks dealt per launch (+ at most one per segment)
struct SegPackArgs {
  char* typed;
  char* contig;
  const TypeRun* runs;   // device copy, typemap order
  const long long* pfx;  // packed bytes before run r within one instance (nruns + 1)
  int nruns;
  int w;
  int unpack;
  int coherent;
  int nseg;
  int blk0[kMaxRanks + 1];
  long long size, extent;
  long long t_off[kMaxRanks];
  long long c_off[kMaxRanks];
  long long units[kMaxRanks];
};

// Segmented pack / unpack in which every segment has a type map, a unit width
// and byte offsets of its own (Alltoallw: segment q = the block of peer q, in
// the datatype of that peer).  Segment j = `units` units of `w` bytes whose
// first instance lies at typed + t_off (bytes) and whose packed bytes start at
// contig + c_off; `nruns` = 0 is a contiguous block (predefined or contiguous
// type), otherwise the map is typed_off's over runs / pfx (the per-type device
// copies).  Segment j owns blocks [blk0[j], blk0[j+1]), dealt in proportion to
// its bytes; all threads of a block serve one segment, so the width is
// block-uniform.  64 B per segment: 1.1 KiB of kernel arguments at 16.
struct SegW {
  const TypeRun* runs;
  const long long* pfx;
  long long size, extent;
  long long t_off, c_off;
  long long units;
  int nruns;
  int w;
};
struct SegWArgs {
  char* typed;
  char* contig;
  int unpack;
  int coherent;
  int nseg;
  int blk0[kMaxRanks + 1];
  SegW seg[kMaxRanks];
};

// One side of a typed transfer: `nruns` = 0 is a contiguous stream (packed
// byte p lives at p), otherwise instances `extent` apart of `size` packed
// bytes each, mapped through runs / pfx as in PackArgs.
struct TypeMap {
  const TypeRun* runs;
  const long long* pfx;
  int nruns;
  int inl;  // runs / pfx are the inline arrays of TypedXferArgs (staged in LDS)
  long long size, extent;
};
// Typed -> typed transfer (Get: the origin pulls the target's window through
// the target type into its buffer through the origin type; Put: the target
// pulls the origin's packed bytes into its window through the target type,
// whose runs arrive with the envelope and travel as kernel arguments).
constexpr int kInlineRuns = 64;
struct TypedXferArgs {
  const char* src;
  char* dst;
  TypeMap s, d;
  int w;
  int coherent;  // system-scope acquire at start / release at end (pull_fences())
  long long units;
  TypeRun iruns[kInlineRuns];
  long long ipfx[kInlineRuns + 1];
};

hipError_t launch_seg_pack(hipStream_t s, const SegPackArgs& a);
hipError_t launch_segw_pack(hipStream_t s, const SegWArgs& a);
hipError_t launch_typed_xfer(hipStream_t s, const TypedXferArgs& a);

}  // namespace mpigx
