// The polyphase FIR of the resampler (gfx950), written once for resample_kernel (logmel.hip: a whole file) and resample_stream_kernel
// (resample_stream.hip: S streams with their state carried forward): the input window of a workgroup's outputs staged in LDS, and the tap loop
// of one output -- four interleaved fmaf accumulators over t mod 4, a0 takes the tail taps, (a0 + a1) + (a2 + a3).  The kernels differ only in
// where an input sample comes from (the `load` of resample_stage) and where an output goes.  See include/hftt_hip.h for the contract.
#pragma once
#include "hftt_common.h"

// the input window of outputs o0 .. olast (at most 256 consecutive ones): frames f0 .. f1, input samples sbase .. sbase + wlen
struct resample_win {
  long f0, sbase;
  int wlen;
};

__device__ __forceinline__ resample_win resample_window(long o0, long olast, int up, int down, int width, int taps) {
  const long f0 = o0 / up, f1 = olast / up;
  return {f0, f0 * down - width, (int)(f1 - f0) * down + taps};
}

// win[i] = load(sbase + i) for the whole window, then the barrier: load(s) is the input sample at index s, zero where the signal has none
template <typename LOAD>
__device__ __forceinline__ void resample_stage(float* win, const resample_win& w, int tid, LOAD load) {
  for (int i = tid; i < w.wlen; i += 256) win[i] = load(w.sbase + i);
  __syncthreads();
}

// output o of the staged window: the dot product of its taps input samples with kernel row o % up
__device__ __forceinline__ float resample_taps(const float* win, const resample_win& wn, const float* kernel, long o, int up, int down, int taps) {
  const long f = o / up;
  const int ph = (int)(o - f * up);
  const float* k = kernel + (long)ph * taps;
  const float* w = win + (int)(f - wn.f0) * down;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int t = 0;
#pragma unroll 4
  for (; t + 4 <= taps; t += 4) {
    a0 = fmaf(w[t], k[t], a0);
    a1 = fmaf(w[t + 1], k[t + 1], a1);
    a2 = fmaf(w[t + 2], k[t + 2], a2);
    a3 = fmaf(w[t + 3], k[t + 3], a3);
  }
  for (; t < taps; t++) a0 = fmaf(w[t], k[t], a0);
  return (a0 + a1) + (a2 + a3);
}
