// The warped sample (gfx950): one window's warp and the Hann-windowed sinc that reads a resident waveform at pos = j * step - delay (Q24).
// ONE device function, called by the dry sample of the clip kernels (clip_dry.h: for the primary and, under clip mixing, the partner, in the
// staging loops of clip_logmel_kernel and clip_room_kernel) and by wave_warp_kernel (wave_warp.hip): what the log-mel sees is what
// hftt_wave_warp writes.  See include/hftt_hip.h for the contract; every operation and its order is stated there.
#pragma once
#include "hftt_common.h"
#include "../../include/hftt_hip.h"

// window b's warp; ok = false: a step, delay or cutoff outside the contract's ranges (the window is treated as one without a file)
struct warp_win {
  long delay;
  int step, H;
  float cut;
  bool ok, identity;
};

__device__ __forceinline__ warp_win warp_load(const hftt_warp_args& w, int b) {
  warp_win v;
  v.step = w.step_q24[b];
  v.delay = w.delay_q24[b];
  v.cut = w.cut[b];
  v.ok = v.step >= HFTT_WARP_STEP_MIN && v.step <= HFTT_WARP_STEP_MAX && v.delay >= 0 && v.delay <= HFTT_WARP_DELAY_MAX && v.cut >= 0.25f && v.cut <= 1.f;
  v.H = v.ok ? (int)((float)HFTT_WARP_ZEROS / v.cut) + 2 : 0;          // <= 26
  v.identity = v.step == (1 << 24) && (v.delay & ((1l << 24) - 1)) == 0;
  return v;
}

// samples of the warped file (n: of the source file, < 2^39)
__device__ __forceinline__ long warp_len(long n, const warp_win& w) {
  return n <= 0 ? 0 : (((n - 1) << 24) + w.delay) / w.step + 1;
}

__device__ __forceinline__ float warp_source(const void* wave, bool i16, long at) {
  return i16 ? (float)((const short*)wave)[at] * (1.f / 32768.f) : ((const float*)wave)[at];
}

// Warped sample j of the file at samp0 (n source samples, np = warp_len(n, w) warped ones), before gain and noise; w.ok holds.
__device__ __forceinline__ float warp_sample(const void* wave, bool i16, long samp0, long n, long np, const float* T, const warp_win& w, long j) {
#pragma clang fp contract(off)
  if (j < 0 || j >= np) return 0.f;
  if (w.identity) {
    const long i = j - (w.delay >> 24);
    return i >= 0 && i < n ? warp_source(wave, i16, samp0 + i) : 0.f;
  }
  const long pos = j * (long)w.step - w.delay;       // <= ((n - 1) << 24) + delay: no overflow
  const long ic = pos >> 24;
  long lo = ic - w.H, hi = ic + w.H + 1;
  lo = lo < 0 ? 0 : lo;                               // outside [0, n): zeros, never a neighbouring file's samples
  hi = hi > n - 1 ? n - 1 : hi;
  float acc = 0.f;
  for (long i = lo; i <= hi; i++) {
    long d = pos - (i << 24);
    d = d < 0 ? -d : d;
    const float q = (float)d * w.cut;
    if (!(q <= (float)HFTT_WARP_ZEROS * 16777216.f)) continue;
    const float x = q * ((float)HFTT_WARP_TABLE_L / 16777216.f);
    const int e = (int)x;
    const float f = x - (float)e;
    const float t0 = T[e], t1 = T[e + 1];
    const float wgt = t0 + f * (t1 - t0);
    acc = acc + (wgt * w.cut) * warp_source(wave, i16, samp0 + i);
  }
  return acc;
}
