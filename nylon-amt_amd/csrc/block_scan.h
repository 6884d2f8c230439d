// Workgroup-wide scans for the 256-thread kernels of notes.hip and labels.hip: the order of every list those kernels write comes from these
// prefix sums, never from atomics.
#pragma once
#include <limits.h>
#include "hftt_common.h"

struct OpMax { static __device__ int id() { return INT_MIN; } static __device__ int f(int a, int b) { return a > b ? a : b; } };
struct OpMin { static __device__ int id() { return INT_MAX; } static __device__ int f(int a, int b) { return a < b ? a : b; } };
struct OpAdd { static __device__ int id() { return 0; } static __device__ int f(int a, int b) { return a + b; } };

// Inclusive scan of x over the workgroup's 256 threads (REV: suffix, over tid .. 255); `excl` receives the exclusive one.  Shuffles inside a
// wave, four wave totals through `slot` (4 ints of LDS that belong to this call site) and ONE barrier: every thread of the workgroup calls it.
// A call site's slot is written again only in the next loop iteration, behind the barrier of another call site or of the caller's broadcast.
template <class Op, bool REV>
__device__ int block_scan(int x, int* slot, int& excl) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = REV ? __shfl_down(x, d) : __shfl_up(x, d);
    if (REV ? lane + d < 64 : lane >= d) x = Op::f(x, y);
  }
  int nb = REV ? __shfl_down(x, 1) : __shfl_up(x, 1);
  if (lane == (REV ? 63 : 0)) nb = Op::id();
  if (lane == (REV ? 0 : 63)) slot[w] = x;
  __syncthreads();
  int acc = Op::id();
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (REV ? i > w : i < w) acc = Op::f(acc, slot[i]);
  excl = Op::f(nb, acc);
  return Op::f(x, acc);
}
