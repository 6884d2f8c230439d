// Clip log-mel (gfx950): the spectrogram windows of a training batch straight from a resident WAVEFORM corpus, one launch.
//   hftt_clip_logmel       B windows [width frames] of the files' concatenated samples (fp32 or int16) -> spec [B, n_mels, width] fp32
//   hftt_clip_logmel_warp  the same of the files played back at a per-window rate and delay: the staged sample is wave_warp.h's warp_sample
// A workgroup owns one window and a run of RUN consecutive frames.  It stages the (RUN - 1) * hop + n_fft samples those frames cover once in
// LDS -- converted, gained, noised, zeros outside the file: consecutive frames share 7/8 of them at hop = n_fft / 8 -- transforms frame after
// frame with the arithmetic of logmel_kernel (logmel.hip: packed 1024-point radix-4 Stockham transform, split pass, |X|^2, sequential CSR mel
// sum, logf), gathers the columns in an LDS tile [n_mels][RUN] and stores it along the frame axis: RUN * 4 = 64 contiguous bytes per
// (window, mel) row.  One writer per element, no atomics, no workspace.  See include/hftt_hip.h for the contract.
// The frame transform is written a second time (clip_logmel_kernel.h) on purpose: tests/frontend_emul.py cites logmel.hip by line (DESIGN.md
// section 9).  The kernel lives in clip_logmel_kernel.h, which clip_mix.hip instantiates with a second source.
#include "hftt_common.h"
#include "hftt_launch.h"
#include "clip_logmel_kernel.h"

// the refusals of both entry points (clip_logmel_kernel.h) and the launch; wa == nullptr: the unwarped instantiation
static int clip_logmel_launch(const hftt_clip_logmel_desc* d, const hftt_warp_args* wa, void* stream) {
  long lds;
  int nruns;
  if (clip_logmel_refuse(d, wa, &lds, &nruns)) return 1;
  const dim3 grid((unsigned)((long)d->B * nruns));
  if (wa) return hftt_launch<clip_logmel_kernel<2048, true>>("clip_logmel_warp", grid, dim3(256), (int)lds, (hipStream_t)stream, *d, *wa, nruns);
  return hftt_launch<clip_logmel_kernel<2048, false>>("clip_logmel", grid, dim3(256), (int)lds, (hipStream_t)stream, *d, hftt_warp_args{}, nruns);
}

extern "C" int hftt_clip_logmel(const hftt_clip_logmel_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_logmel: null descriptor");
  return clip_logmel_launch(d, nullptr, stream);
}

extern "C" int hftt_clip_logmel_warp(const hftt_clip_logmel_warp_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_logmel: null descriptor");
  return clip_logmel_launch(&d->base, &d->warp, stream);
}
