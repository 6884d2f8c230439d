// Warped waveform windows (gfx950): the samples that hftt_clip_logmel_warp stages, written to memory before gain and noise.
//   hftt_wave_warp  B windows [len warped samples] of the files' concatenated samples (fp32 or int16) -> fp32 [B, len]
// One thread per output sample, each calling wave_warp.h's warp_sample -- the function the clip log-mel's staging loop calls -- so the
// interpolation is observable, and an augmented copy of a file is one launch.  See include/hftt_hip.h for the contract.
#include "hftt_common.h"
#include "hftt_launch.h"
#include "wave_warp.h"
#include "../../include/hftt_hip.h"

namespace {

constexpr int TPB = 256;

__global__ __launch_bounds__(TPB) void wave_warp_kernel(const hftt_wave_warp_desc g, int nchunks) {
  const int b = (int)(blockIdx.x / (unsigned)nchunks);
  const int c = (int)(blockIdx.x % (unsigned)nchunks) * TPB + threadIdx.x;
  if (c >= g.len) return;
  const int file = g.win_file[b];
  float s = 0.f;                                      // no such file, an invalid warp, outside [0, n'): zeros
  if (file >= 0 && file < g.n_files) {
    const long samp0 = g.file_samp0[file];
    const long n = g.file_samp0[file + 1] - samp0;
    const warp_win w = warp_load(g.warp, b);
    if (w.ok && samp0 >= 0 && n >= 0 && samp0 + n <= g.total_samples) {
      const long start = g.win_start[b];
      const long np = warp_len(n, w);
      // (start + c cannot wrap: a start within 2^62 of either end of int64 is outside every file)
      if (start > -(1l << 62) && start < (1l << 62)) s = warp_sample(g.wave, g.wave_i16 != 0, samp0, n, np, g.warp.proto, w, start + c);
    }
  }
  ((float*)g.out)[(long)b * g.len + c] = s;
}

}  // namespace

extern "C" int hftt_wave_warp(const hftt_wave_warp_desc* d, void* stream) {
  HFTT_REQUIRE(d, "wave_warp: null descriptor");
  HFTT_REQUIRE(d->wave, "wave_warp: wave is null");
  HFTT_REQUIRE(d->file_samp0, "wave_warp: file_samp0 is null");
  HFTT_REQUIRE(d->win_file && d->win_start, "wave_warp: null window table (win_file / win_start)");
  HFTT_REQUIRE(d->warp.step_q24 && d->warp.delay_q24 && d->warp.cut && d->warp.proto, "wave_warp: null warp table (step_q24 / delay_q24 / cut / proto)");
  HFTT_REQUIRE(d->out, "wave_warp: out is null");
  HFTT_REQUIRE(d->wave_i16 == 0 || d->wave_i16 == 1, "wave_warp: wave_i16=%d (0 = fp32, 1 = int16)", d->wave_i16);
  HFTT_REQUIRE(d->B >= 1, "wave_warp: B=%d must be positive", d->B);
  HFTT_REQUIRE(d->len >= 1, "wave_warp: len=%d must be positive", d->len);
  HFTT_REQUIRE(d->n_files >= 1, "wave_warp: n_files=%d must be positive", d->n_files);
  HFTT_REQUIRE(d->total_samples >= 0 && d->total_samples <= (1l << 38), "wave_warp: total_samples=%ld outside 0 .. 2^38 (Q24 positions)", (long)d->total_samples);
  const int nchunks = hftt_ceil_div(d->len, TPB);
  HFTT_REQUIRE((long)d->B * nchunks < (1l << 31), "wave_warp: B=%d windows of len=%d exceed 2^31 workgroups", d->B, d->len);
  return hftt_launch<wave_warp_kernel>("wave_warp", dim3((unsigned)((long)d->B * nchunks)), dim3(TPB), 0, (hipStream_t)stream, *d, nchunks);
}
