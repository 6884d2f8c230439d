// Label rendering on the device (gfx950): note lists -> the frame labels that training consumes, the reference's corpus/conv_note2label.py:8-111
// (note2label) restated per output element.  The reference walks the notes and paints frames; every rule it applies to a frame reads only that
// frame's own state, so one thread can own frame f of one pitch and walk that pitch's notes in list order instead:
//   hftt_labels_render       B windows [len frames] of a corpus-wide note table -> onset / offset / mpe / velocity [B, len, N], one launch
//   hftt_labels_render_warp  the same under a per-window pitch shift and time map t' = (t + t_delay) * t_scale (the labels of a warped clip)
// See include/hftt_hip.h for the contract.  One writer per element, no atomics; the survivors of the note filter keep their list order through a
// prefix sum, so a result is bit-identical from launch to launch.  The kernel lives in labels_walk.h, which labels_mix.hip instantiates with a
// second source.
#include "hftt_common.h"
#include "hftt_launch.h"
#include "labels_walk.h"

// the refusals of both entry points (labels_walk.h) and the launch; w == nullptr: no warp
static int labels_launch(const hftt_labels_desc* d, const hftt_labels_warp_desc* w, void* stream) {
  if (labels_refuse(d, w == nullptr)) return 1;
  const int nchunks = hftt_ceil_div(d->len, CH);
  const dim3 grid((unsigned)((long)d->B * nchunks * d->N));      // < 2^31: at most one workgroup per element
  label_warp lw = {};
  if (w) {
    HFTT_REQUIRE(w->shift && w->t_delay && w->t_scale && w->file_end_sec, "labels_render: null warp table (shift / t_delay / t_scale / file_end_sec)");
    lw = {w->shift, w->t_delay, w->t_scale, w->file_end_sec};
  }
  const char* what = w ? "labels_render_warp" : "labels_render";
  if (d->form == HFTT_LABELS_TRAIN) return hftt_launch<labels_render_kernel<true>>(what, grid, dim3(CH), 0, (hipStream_t)stream, *d, lw, nchunks);
  return hftt_launch<labels_render_kernel<false>>(what, grid, dim3(CH), 0, (hipStream_t)stream, *d, lw, nchunks);
}

extern "C" int hftt_labels_render(const hftt_labels_desc* d, void* stream) {
  HFTT_REQUIRE(d, "labels_render: null descriptor");
  return labels_launch(d, nullptr, stream);
}

extern "C" int hftt_labels_render_warp(const hftt_labels_warp_desc* d, void* stream) {
  HFTT_REQUIRE(d, "labels_render: null descriptor");
  return labels_launch(&d->base, d, stream);
}
