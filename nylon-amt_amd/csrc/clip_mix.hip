// Clip mixing, the audio half (gfx950): the clip log-mel of two clips summed while their samples are staged, one launch.
//   hftt_clip_logmel_mix       hftt_clip_logmel with a per-window partner (file, start frame, gain) added onto the primary's extent
//   hftt_clip_logmel_mix_warp  the same with each source played back under its own warp: both go through wave_warp.h's warp_sample
// The kernel is clip_logmel_kernel.h's, instantiated with a partner table: the partner's sample is added into the same stage[j] slot, so the LDS
// layout, the frame transform and the tile store are hftt_clip_logmel's.  A translation unit of its own because tests pin clip_logmel.hip to
// its two kernels.  See include/hftt_hip.h for the contract.
#include "hftt_common.h"
#include "hftt_launch.h"
#include "clip_logmel_kernel.h"

// the refusals of both entry points and the launch; wa == nullptr: neither source is warped (wb is not read)
static int clip_mix_launch(const hftt_clip_logmel_desc* d, const hftt_warp_args* wa, const hftt_clip_mix_args* m, const hftt_warp_args* wb, void* stream) {
  long lds;
  int nruns;
  if (clip_logmel_refuse(d, wa, &lds, &nruns)) return 1;
  HFTT_REQUIRE(m->mix_file && m->mix_start && m->mix_gain, "clip_logmel: null partner table (mix_file / mix_start / mix_gain)");
  if (wa) HFTT_REQUIRE(wb->step_q24 && wb->delay_q24 && wb->cut && wb->proto, "clip_logmel: null partner warp table (step_q24 / delay_q24 / cut / proto)");
  const dim3 grid((unsigned)((long)d->B * nruns));
  if (wa) return hftt_launch<clip_logmel_kernel<2048, true, clip_mix>>("clip_logmel_mix_warp", grid, dim3(256), (int)lds, (hipStream_t)stream, *d, *wa, nruns, clip_mix{*m, *wb});
  return hftt_launch<clip_logmel_kernel<2048, false, clip_mix>>("clip_logmel_mix", grid, dim3(256), (int)lds, (hipStream_t)stream, *d, hftt_warp_args{}, nruns, clip_mix{*m, hftt_warp_args{}});
}

extern "C" int hftt_clip_logmel_mix(const hftt_clip_logmel_mix_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_logmel: null descriptor");
  return clip_mix_launch(&d->base, nullptr, &d->mix, nullptr, stream);
}

extern "C" int hftt_clip_logmel_mix_warp(const hftt_clip_logmel_mix_warp_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_logmel: null descriptor");
  return clip_mix_launch(&d->base, &d->warp, &d->mix, &d->mix_warp, stream);
}
