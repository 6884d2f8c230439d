// The dry sample of a clip window (gfx950): what clip_logmel_kernel stages in front of the noise term -- the primary through warp_sample or read
// directly, fmul by the gain, then fadd(s, fmul(partner, mix_gain)).  ONE device function, clip_dry, called term by term by the staging loops of
// clip_logmel_kernel (clip_logmel.hip) and of clip_room_kernel (clip_room.hip): the signal the room convolves is the signal the log-mel stages.
// See include/hftt_hip.h for the contract (clip log-mel, warp, clip mixing).
#pragma once
#include "hftt_common.h"
#include "wave_warp.h"
#include "../../include/hftt_hip.h"

// one source (primary or partner) of window b: its file inside the corpus and its warp; n < 0: no such source, np = the samples the frames see
struct clip_source {
  long samp0, n, np;
  warp_win w;
};

// file < 0, file >= n_files, a table entry that leaves the corpus, or (WARP) a warp outside the contract's ranges: n = np = -1
template <bool WARP>
__device__ __forceinline__ clip_source clip_source_load(const long* file_samp0, int n_files, long total_samples, int file, const hftt_warp_args& wa, int b) {
  clip_source s = {};
  s.n = -1;
  if (file >= 0 && file < n_files) {
    s.samp0 = file_samp0[file];
    s.n = file_samp0[file + 1] - s.samp0;
    if (s.samp0 < 0 || s.n < 0 || s.samp0 + s.n > total_samples) s.n = -1;         // a table that leaves the corpus: nothing is read there
  }
  s.np = s.n;
  if constexpr (WARP) {
    s.w = warp_load(wa, b);
    if (!s.w.ok) s.n = -1;
    s.np = s.n >= 0 ? warp_len(s.n, s.w) : -1;
  }
  return s;
}

// One term of the dry sample at position i of the source's (warped) file; x = the source's sample there, zero outside [0, np).
//   PARTNER = false  the primary's term: x, fmul by `gain` when has_gain                 (prev is not read)
//   PARTNER = true   the partner's term on top of prev: fadd(prev, fmul(x, gain))          (gain = mix_gain; has_gain is not read)
// One rounding per operation: __fmul_rn / __fadd_rn are plain operators in this toolchain, which the compiler may contract into an fma -- not
// in this function.  proto: the warp's prototype table (WARP only).
template <bool WARP, bool PARTNER>
__device__ __forceinline__ float clip_dry(float prev, const void* wave, bool i16, const clip_source& src, const float* proto, long i, bool has_gain, float gain) {
#pragma clang fp contract(off)
  float x = 0.f;                                      // outside [0, np): zeros, never a neighbouring file's samples
  if (i >= 0 && i < src.np) {
    if constexpr (WARP) x = warp_sample(wave, i16, src.samp0, src.n, src.np, proto, src.w, i);
    else x = warp_source(wave, i16, src.samp0 + i);
  }
  if constexpr (PARTNER) {
    const float p = x * gain;
    return prev + p;
  } else {
    return has_gain ? x * gain : x;
  }
}
