// Clip mixing, the label half (gfx950): the labels of two clips summed, one launch.
//   hftt_labels_render_mix  hftt_labels_render[_warp] with a per-window partner whose group is walked BEHIND the primary's with the same carried
//                           state (o, off, mpe, vel) -- the reference's velocity rule reads the combined onset track, so two renders combined
//                           afterwards are not it
// The kernel is labels_walk.h's, instantiated with a partner table.  A translation unit of its own because tests pin labels.hip to its two
// kernels.  See include/hftt_hip.h for the contract.
#include "hftt_common.h"
#include "hftt_launch.h"
#include "labels_walk.h"

extern "C" int hftt_labels_render_mix(const hftt_labels_mix_desc* m, void* stream) {
  HFTT_REQUIRE(m, "labels_render: null descriptor");
  const hftt_labels_desc* d = &m->base;
  const bool warp_a = m->shift || m->t_delay || m->t_scale, warp_b = m->mix_shift || m->mix_t_delay || m->mix_t_scale;
  if (labels_refuse(d, !warp_a || !warp_b)) return 1;
  HFTT_REQUIRE(m->mix_file && m->mix_start, "labels_render: null partner table (mix_file / mix_start)");
  HFTT_REQUIRE(m->a_frames, "labels_render: a_frames is null");
  HFTT_REQUIRE(!warp_a || (m->shift && m->t_delay && m->t_scale), "labels_render: null warp table (shift / t_delay / t_scale: all or none)");
  HFTT_REQUIRE(!warp_b || (m->mix_shift && m->mix_t_delay && m->mix_t_scale), "labels_render: null partner warp table (mix_shift / mix_t_delay / mix_t_scale: all or none)");
  HFTT_REQUIRE(!(warp_a || warp_b) || m->file_end_sec, "labels_render: null warp table (file_end_sec)");
  const int nchunks = hftt_ceil_div(d->len, CH);
  const dim3 grid((unsigned)((long)d->B * nchunks * d->N));      // < 2^31: at most one workgroup per element
  const label_warp lw = {m->shift, m->t_delay, m->t_scale, m->file_end_sec};
  const label_mix mx = {m->mix_file, m->mix_start, {m->mix_shift, m->mix_t_delay, m->mix_t_scale, m->file_end_sec}, m->a_frames};
  if (d->form == HFTT_LABELS_TRAIN) return hftt_launch<labels_render_kernel<true, label_mix>>("labels_render_mix", grid, dim3(CH), 0, (hipStream_t)stream, *d, lw, nchunks, mx);
  return hftt_launch<labels_render_kernel<false, label_mix>>("labels_render_mix", grid, dim3(CH), 0, (hipStream_t)stream, *d, lw, nchunks, mx);
}
