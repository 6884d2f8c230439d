// Label rendering on the device (gfx950): note lists -> the frame labels that training consumes, the reference's corpus/conv_note2label.py:8-111
// (note2label) restated per output element.  The reference walks the notes and paints frames; every rule it applies to a frame reads only that
// frame's own state, so one thread can own frame f of one pitch and walk that pitch's notes in list order instead:
//   hftt_labels_render       B windows [len frames] of a corpus-wide note table -> onset / offset / mpe / velocity [B, len, N], one launch
//   hftt_labels_render_warp  the same under a per-window pitch shift and time map t' = (t + t_delay) * t_scale (the labels of a warped clip)
//   hftt_labels_render_mix   either with a per-window partner whose group is walked BEHIND the primary's with the same carried state (o, off,
//                            mpe, vel) -- the reference's velocity rule reads the combined onset track, so two renders combined afterwards
//                            are not it
// See include/hftt_hip.h for the contract.  One writer per element, no atomics; the survivors of the note filter keep their list order through a
// prefix sum, so a result is bit-identical from launch to launch.
#include <math.h>
#include "hftt_common.h"
#include "hftt_host.h"
#include "hftt_launch.h"
#include "block_scan.h"
#include "../../include/hftt_hip.h"

// The value arithmetic below is the reference's, one fp64 operation for one: nothing in this file may be contracted into an fma.
#pragma clang fp contract(off)

namespace {

constexpr int CH = HFTT_LABELS_CHUNK;          // frames per workgroup = notes per filter pass = threads per workgroup
static_assert(CH == 256, "block_scan (block_scan.h) is written for four waves");

// (int)(sec * fps + 0.5) and the triangle value in the reference's doubles, with IEEE division
__device__ inline int frame_of(double sec, double fps) {
  return (int)(sec * fps + 0.5);
}
// den = sharpness * hop_ms
__device__ inline float triangle(int f, double hop_ms, double t_ms, double den) {
  const double v = 1.0 - __ddiv_rn(fabs((double)f * hop_ms - t_ms), den);
  return (float)(v > 0.0 ? v : 0.0);
}

// The survivors of one filter pass, in list order.  Every frame thread reads the same entry at the same time: LDS broadcasts.
struct survivors {
  double on_ms[CH], off_ms[CH], off_den[CH];
  int on_f[CH], off_f[CH], sharp[CH], vel[CH];   // sharp < 0: no offset target
};

// the per-window map of hftt_labels_render_warp (null pointers for hftt_labels_render, which never reads them)
struct label_warp {
  const int32_t* shift;
  const double* t_delay;
  const double* t_scale;
  const double* file_end_sec;
};

// the partner of hftt_labels_render_mix: its window table, its map (lw.shift == nullptr: none) and the primaries' audio frame counts
struct label_mix {
  const int32_t* mix_file;
  const int32_t* mix_start;
  label_warp lw;
  const int64_t* a_frames;
};
__device__ __forceinline__ const label_mix& label_mix_of(const label_mix& mx) { return mx; }

// One source of a cell: what the walk needs to know about (file, first frame of the window) under an optional map.
struct label_source {
  bool warp;
  double t_delay, t_scale;
  long nframe;                                 // frames of the (warped) file; 0: no such file
  long f0, f1, f;                              // the workgroup renders file frames [f0, f1); this thread frame f
  int beg, end;                                // the group's records (empty when nothing can reach [f0, f1): the same for every thread)
};

// Under a warp (lw.shift != nullptr: the same for every thread of the launch, so the branches below do not diverge and the unwarped launch
// executes the operations it always did) output pitch j walks source pitch j - shift[b], every note time t is (t + t_delay[b]) * t_scale[b]
// (two roundings: this file is compiled without contraction), and the file's frame count follows from its last offset under the same map.
__device__ __forceinline__ label_source label_source_of(const hftt_labels_desc& g, const label_warp& lw, int file, long start, int b, int j, int k, int tid) {
  label_source a;
  const int N = g.N;
  const bool known = file >= 0 && file < g.n_files;
  int jsrc = j;                                // the pitch whose notes this column shows
  a.t_delay = 0.0;
  a.t_scale = 1.0;
  a.nframe = 0;
  a.warp = lw.shift != nullptr;
  if (a.warp) {
    jsrc = j - lw.shift[b];
    a.t_delay = lw.t_delay[b];
    a.t_scale = lw.t_scale[b];
    if (known) {
      const bool empty = g.row_ptr[(long)file * N] == g.row_ptr[(long)file * N + N];
      a.nframe = empty ? 1 : (long)frame_of((lw.file_end_sec[file] + a.t_delay) * a.t_scale, g.fps) + 1;
    }
  } else {
    a.nframe = known ? g.file_nframe[file] : 0;
  }
  a.f0 = start + (long)k * CH;                 // file frame of thread 0
  a.f1 = a.f0 + (g.len - k * CH < CH ? g.len - k * CH : CH);
  a.f = a.f0 + tid;
  a.beg = a.end = 0;
  if (known && a.f1 > 0 && a.f0 < a.nframe && jsrc >= 0 && jsrc < N) {  // (the same for every thread: the barriers of the walk are met by all or by none)
    a.beg = g.row_ptr[(long)file * N + jsrc];
    a.end = g.row_ptr[(long)file * N + jsrc + 1];
    a.beg = a.beg < 0 ? 0 : a.beg;
    a.end = a.end > g.n_notes ? g.n_notes : a.end;
  }
  return a;
}

// The walk of one source's group: filter passes of CH notes into LDS in list order, then every frame thread with `inside` walks the
// survivors, carrying o, off, mpe, vel.  Every thread of the workgroup calls it with the same beg / end.
__device__ __forceinline__ void label_walk(const hftt_labels_desc& g, const label_source& a, bool inside, survivors& s, int* slot, int& total, int tid,
                                           float& o, float& off, int& mpe, int& vel) {
  const double hop_ms = g.hop_ms, fps = g.fps;
  const int tol = g.tol;
  const double on_den = (double)tol * hop_ms;
  const long f0 = a.f0, f1 = a.f1, f = a.f;
  for (long c0 = a.beg; c0 < a.end; c0 += CH) {
    // filter: note c0 + tid survives when one of its three frame ranges can reach [f0, f1)
    bool keep = false;
    double on_ms = 0.0, off_ms = 0.0, off_den = 0.0;
    int on_f = 0, off_f = 0, sharp = -1, v = 0;
    if (c0 + tid < a.end) {
      const hftt_label_note n = g.notes[c0 + tid];
      double on_sec = n.onset_sec, off_sec = n.offset_sec;
      if (a.warp) {
        on_sec = (on_sec + a.t_delay) * a.t_scale;
        off_sec = (off_sec + a.t_delay) * a.t_scale;
      }
      on_f = frame_of(on_sec, fps);
      off_f = frame_of(off_sec, fps);
      on_ms = on_sec * 1000.0;
      off_ms = off_sec * 1000.0;
      v = n.velocity;
      long lo = (long)on_f - tol, hi = (long)on_f + tol;
      if (off_f > hi) hi = off_f;              // mpe: on_f .. off_f
      if (!(n.flags & 1)) {
        sharp = tol;
        if (g.duration_tolerance) {
          const int dur = (int)(__ddiv_rn((off_ms - on_ms) * 0.2, hop_ms) + 0.5);
          if (dur > sharp) sharp = dur;
        }
        off_den = (double)sharp * hop_ms;
        if ((long)off_f - sharp < lo) lo = (long)off_f - sharp;
        if ((long)off_f + sharp > hi) hi = (long)off_f + sharp;
      }
      keep = lo < f1 && hi >= f0;
    }
    int at;
    const int inc = block_scan<OpAdd, false>(keep ? 1 : 0, slot, at);
    if (keep) {
      s.on_ms[at] = on_ms; s.off_ms[at] = off_ms; s.off_den[at] = off_den;
      s.on_f[at] = on_f; s.off_f[at] = off_f; s.sharp[at] = sharp; s.vel[at] = v;
    }
    if (tid == CH - 1) total = inc;
    __syncthreads();
    const int n = total;
    if (inside) {
      for (int i = 0; i < n; i++) {
        const long d_on = f - s.on_f[i], d_off = f - s.off_f[i];
        if (d_on >= -tol && d_on <= tol) {
          o = fmaxf(o, triangle((int)f, hop_ms, s.on_ms[i], on_den));
          if (o >= 0.5f && (d_on >= 0 || vel == 0)) vel = s.vel[i];
        }
        if (d_on >= 0 && d_off <= 0) mpe = 1;
        const int sharp = s.sharp[i];
        if (d_off >= -(long)sharp && d_off <= sharp) off = fmaxf(off, triangle((int)f, hop_ms, s.off_ms[i], s.off_den[i]));
      }
    }
    __syncthreads();                           // the next pass writes the list and `total` again
  }
}

// One workgroup per (pitch, chunk of CH frames, window), pitch fastest so that workgroups in flight together fill whole output rows.
// The map is a launch argument, not a template parameter: the forms without a partner stay the two kernels whose registers and occupancy
// tests/test_labels_capi.py pins.  The partner is a trailing parameter pack -- empty or one label_mix -- so that the forms without one keep
// the kernel arguments they always had: behind the primary's walk the same walk runs over the partner's group at the
// partner's frame, carrying the cell's state on.
template <bool TRAIN, typename... MX>
__global__ __launch_bounds__(CH) void labels_render_kernel(const hftt_labels_desc g, const label_warp lw, int nchunks, const MX... mx_pack) {
  constexpr bool MIX = sizeof...(MX) == 1;
  static_assert(sizeof...(MX) <= 1, "at most one partner");
  __shared__ survivors s;
  __shared__ int slot[4];
  __shared__ int total;
  const int tid = threadIdx.x, N = g.N;
  const int j = (int)(blockIdx.x % (unsigned)N);
  const unsigned rest = blockIdx.x / (unsigned)N;
  const int k = (int)(rest % (unsigned)nchunks), b = (int)(rest / (unsigned)nchunks);
  const int t = k * CH + tid;                  // frame inside the window
  const label_source a = label_source_of(g, lw, g.win_file[b], (long)g.win_start[b], b, j, k, tid);
  float o = 0.f, off = 0.f;
  int mpe = 0, vel = 0;
  label_walk(g, a, t < g.len && a.f >= 0 && a.f < a.nframe, s, slot, total, tid, o, off, mpe, vel);
  if constexpr (MIX) {
    const label_mix& mx = label_mix_of(mx_pack...);
    label_source p = label_source_of(g, mx.lw, mx.mix_file[b], (long)mx.mix_start[b], b, j, k, tid);
    const long af = mx.a_frames[b];
    if (!(a.f1 > 0 && a.f0 < af)) p.beg = p.end = 0;           // (uniform) no frame of the workgroup has audio of the primary under it
    label_walk(g, p, t < g.len && p.f >= 0 && p.f < p.nframe && a.f >= 0 && a.f < af, s, slot, total, tid, o, off, mpe, vel);
  }
  if (t >= g.len) return;
  const long e = ((long)b * g.len + t) * N + j;
  ((float*)g.onset)[e] = o;
  ((float*)g.offset)[e] = off;
  if constexpr (TRAIN) {
    ((float*)g.mpe)[e] = (float)mpe;
    ((long*)g.velocity)[e] = vel;
  } else {
    ((unsigned char*)g.mpe)[e] = (unsigned char)mpe;
    ((signed char*)g.velocity)[e] = (signed char)vel;
  }
}

}  // namespace

// The refusals of hftt_labels_desc for every entry point, in front of the launch; need_nframe: a source without a map reads file_nframe.
static int labels_refuse(const hftt_labels_desc* d, bool need_nframe) {
  HFTT_REQUIRE(d->n_files >= 1, "labels_render: n_files=%d must be positive", d->n_files);
  HFTT_REQUIRE(d->n_notes >= 0, "labels_render: n_notes=%d is negative", d->n_notes);
  HFTT_REQUIRE(d->B >= 1, "labels_render: B=%d must be positive", d->B);
  HFTT_REQUIRE(d->len >= 1, "labels_render: len=%d must be positive", d->len);
  HFTT_REQUIRE(d->N >= 1 && d->N <= 128, "labels_render: N=%d outside 1..128", d->N);
  HFTT_REQUIRE(d->tol >= 1, "labels_render: tol=%d must be at least 1 (the triangle's half-width in frames: int(50 / hop_ms + 0.5))", d->tol);
  HFTT_REQUIRE(d->hop_ms > 0.0 && d->fps > 0.0, "labels_render: hop_ms=%g / fps=%g must be positive", d->hop_ms, d->fps);
  HFTT_REQUIRE(d->duration_tolerance == 0 || d->duration_tolerance == 1, "labels_render: duration_tolerance=%d (0 / 1)", d->duration_tolerance);
  HFTT_REQUIRE(d->form == HFTT_LABELS_TRAIN || d->form == HFTT_LABELS_STORE, "labels_render: form=%d (0 = train, 1 = store)", d->form);
  HFTT_REQUIRE(d->notes || d->n_notes == 0, "labels_render: notes is null at n_notes=%d", d->n_notes);
  HFTT_REQUIRE(d->row_ptr, "labels_render: row_ptr is null");
  HFTT_REQUIRE(!need_nframe || d->file_nframe, "labels_render: file_nframe is null");
  HFTT_REQUIRE(d->win_file, "labels_render: win_file is null");
  HFTT_REQUIRE(d->win_start, "labels_render: win_start is null");
  HFTT_REQUIRE(d->onset && d->offset && d->mpe && d->velocity, "labels_render: null output (onset / offset / mpe / velocity)");
  HFTT_REQUIRE((long)d->B * d->len * d->N < (1l << 31), "labels_render: B=%d windows of len=%d frames and N=%d exceed 2^31 elements", d->B, d->len, d->N);
  return 0;
}

// the grid, the output form and the launch of every entry point, behind its refusals; mx == nullptr: no partner
static int labels_launch(const char* what, const hftt_labels_desc* d, const label_warp& lw, const label_mix* mx, void* stream) {
  const int nchunks = hftt_ceil_div(d->len, CH);
  const dim3 grid((unsigned)((long)d->B * nchunks * d->N));      // < 2^31: at most one workgroup per element
  const bool train = d->form == HFTT_LABELS_TRAIN;
  if (mx && train) return hftt_launch<labels_render_kernel<true, label_mix>>(what, grid, dim3(CH), 0, (hipStream_t)stream, *d, lw, nchunks, *mx);
  if (mx) return hftt_launch<labels_render_kernel<false, label_mix>>(what, grid, dim3(CH), 0, (hipStream_t)stream, *d, lw, nchunks, *mx);
  if (train) return hftt_launch<labels_render_kernel<true>>(what, grid, dim3(CH), 0, (hipStream_t)stream, *d, lw, nchunks);
  return hftt_launch<labels_render_kernel<false>>(what, grid, dim3(CH), 0, (hipStream_t)stream, *d, lw, nchunks);
}

extern "C" int hftt_labels_render(const hftt_labels_desc* d, void* stream) {
  HFTT_REQUIRE(d, "labels_render: null descriptor");
  if (labels_refuse(d, true)) return 1;
  return labels_launch("labels_render", d, label_warp{}, nullptr, stream);
}

extern "C" int hftt_labels_render_warp(const hftt_labels_warp_desc* w, void* stream) {
  HFTT_REQUIRE(w, "labels_render: null descriptor");
  if (labels_refuse(&w->base, false)) return 1;
  HFTT_REQUIRE(w->shift && w->t_delay && w->t_scale && w->file_end_sec, "labels_render: null warp table (shift / t_delay / t_scale / file_end_sec)");
  return labels_launch("labels_render_warp", &w->base, label_warp{w->shift, w->t_delay, w->t_scale, w->file_end_sec}, nullptr, stream);
}

extern "C" int hftt_labels_render_mix(const hftt_labels_mix_desc* m, void* stream) {
  HFTT_REQUIRE(m, "labels_render: null descriptor");
  const bool warp_a = m->shift || m->t_delay || m->t_scale, warp_b = m->mix_shift || m->mix_t_delay || m->mix_t_scale;
  if (labels_refuse(&m->base, !warp_a || !warp_b)) return 1;
  HFTT_REQUIRE(m->mix_file && m->mix_start, "labels_render: null partner table (mix_file / mix_start)");
  HFTT_REQUIRE(m->a_frames, "labels_render: a_frames is null");
  HFTT_REQUIRE(!warp_a || (m->shift && m->t_delay && m->t_scale), "labels_render: null warp table (shift / t_delay / t_scale: all or none)");
  HFTT_REQUIRE(!warp_b || (m->mix_shift && m->mix_t_delay && m->mix_t_scale), "labels_render: null partner warp table (mix_shift / mix_t_delay / mix_t_scale: all or none)");
  HFTT_REQUIRE(!(warp_a || warp_b) || m->file_end_sec, "labels_render: null warp table (file_end_sec)");
  const label_mix mx = {m->mix_file, m->mix_start, {m->mix_shift, m->mix_t_delay, m->mix_t_scale, m->file_end_sec}, m->a_frames};
  return labels_launch("labels_render_mix", &m->base, label_warp{m->shift, m->t_delay, m->t_scale, m->file_end_sec}, &mx, stream);
}
