// The frame transform of the log-mel front end (gfx950), written once: packed, windowed frame in LDS -> |X|^2 of its 2048-point real transform
// -> one mel row's log, in pieces: frame_stage (one radix-4 Stockham stage), frame_split (split pass and power), frame_mel (mel sum and log).
// Called by logmel_kernel (logmel.hip: one workgroup per frame) and by clip_logmel_kernel (clip_logmel.hip: a run of
// frames per workgroup), so the two compute a frame with the same operations in the same order.  The callers own the LDS arrays, the packing
// and where a result goes; tests/frontend_emul.py restates these functions in fp32 and counts their roundings by name.
#pragma once
#include "hftt_common.h"

namespace {

// twiddle: e^(-2 pi i m / NFFT), 0 <= m < NFFT, from the host's table (tc / ts: cos / sin of 2 pi k / NFFT, k < NFFT / 2; the second half
// turn is a sign)
template <int NFFT>
__device__ __forceinline__ float2 frame_tw(const float* tc, const float* ts, int m) {
  const int mm = m & (NFFT / 2 - 1);
  const float c = tc[mm], sn = ts[mm];
  return (m & (NFFT / 2)) ? make_float2(-c, sn) : make_float2(c, -sn);
}

// complex multiply
__device__ __forceinline__ float2 frame_cmul(float2 a, float2 w) {
  return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

// The frame is REAL, so its 2048-point transform is one 1024-point COMPLEX transform of z[n] = x[2n] + i x[2n+1] plus a pass that separates
// the spectra of the even and odd samples (X[k] = E[k] + W^k O[k], E / O from Z[k] and conj(Z[N/2 - k])): half the butterflies.  The
// 1024-point transform is radix-4 Stockham (autosort: natural order in, natural order out, no bit-reversal pass): 5 stages of ONE butterfly
// per thread and one barrier each.  Points live in LDS as interleaved (re, im) pairs: a stage READS x[j + q N/4] -- consecutive lanes,
// consecutive 8-byte words: conflict-free -- and writes its four results Ns apart (stride-4 Ns writes: 4-way conflicts in the first three
// stages, none in the last two).
// The loop over Ns = 1, 4 .. 256 that swaps the two buffers stays in the kernels: with it inside a function here, the same source compiled to
// another packing of the butterflies into v_pk_* lanes and another choice of which product of a complex multiply is fused, i.e. other roundings
// (DESIGN.md section 10).
// One stage: the caller's barrier behind the writes of src; a barrier behind the writes of dst.  Called by all 256 threads of the workgroup.
template <int NFFT>
__device__ __forceinline__ void frame_stage(const float2* src, float2* dst, int Ns, const float* tc, const float* ts, int tid) {
  static_assert(NFFT == 2048, "one butterfly per thread: 1024 complex points, 256 threads");
  constexpr int N = NFFT / 2, Q = N / 4;              // complex points, butterflies per stage (= threads)
  const int j = tid, k = j & (Ns - 1);
  const int step = NFFT / (4 * Ns);                   // twiddle index of exp(-2 pi i k / (4 Ns)) per unit k
  float2 v0 = src[j], v1 = src[j + Q], v2 = src[j + 2 * Q], v3 = src[j + 3 * Q];
  if (Ns > 1) {
    v1 = frame_cmul(v1, frame_tw<NFFT>(tc, ts, k * step));
    v2 = frame_cmul(v2, frame_tw<NFFT>(tc, ts, 2 * k * step));
    v3 = frame_cmul(v3, frame_tw<NFFT>(tc, ts, 3 * k * step));
  }
  const float2 a02 = make_float2(v0.x + v2.x, v0.y + v2.y), s02 = make_float2(v0.x - v2.x, v0.y - v2.y);
  const float2 a13 = make_float2(v1.x + v3.x, v1.y + v3.y), s13 = make_float2(v1.x - v3.x, v1.y - v3.y);
  const int j0 = ((j - k) << 2) + k;                  // (j / Ns) * 4 Ns + k
  dst[j0] = make_float2(a02.x + a13.x, a02.y + a13.y);
  dst[j0 + Ns] = make_float2(s02.x + s13.y, s02.y - s13.x);            // v0 - i v1 - v2 + i v3
  dst[j0 + 2 * Ns] = make_float2(a02.x - a13.x, a02.y - a13.y);
  dst[j0 + 3 * Ns] = make_float2(s02.x - s13.y, s02.y + s13.x);        // v0 + i v1 - v2 - i v3
  __syncthreads();
}

// In: Z = the transform's result in src[N], behind a barrier.  Out: pw[0 .. N] = |X|^2, behind a barrier.
template <int NFFT>
__device__ __forceinline__ void frame_split(const float2* src, float* pw, const float* tc, const float* ts, int tid) {
  constexpr int N = NFFT / 2;
  // split pass: E = (Z[k] + conj Z[N-k]) / 2, O = (Z[k] - conj Z[N-k]) / (2i), X[k] = E + W^k O, k = 0 .. N (Z[N] = Z[0]); power: |X|^2
  for (int k = tid; k <= N; k += 256) {
    const float2 zk = src[k & (N - 1)], zn = src[(N - k) & (N - 1)];
    const float2 e = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
    const float2 o = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
    const float2 wo = frame_cmul(o, frame_tw<NFFT>(tc, ts, k));
    const float xr = e.x + wo.x, xi = e.y + wo.y;
    pw[k] = xr * xr + xi * xi;
  }
  __syncthreads();
}

// mel sum: one row of the sparse slaney/htk filterbank (CSR by mel: len weights from fb_w[off] on bins st ..), summed in sequence, and its log
__device__ __forceinline__ float frame_mel(const float* fb_w, const float* pw, int st, int len, int off, float log_offset) {
  float acc = 0.f;
  for (int j = 0; j < len; j++) acc += fb_w[off + j] * pw[st + j];
  return logf(acc + log_offset);
}

}  // namespace
