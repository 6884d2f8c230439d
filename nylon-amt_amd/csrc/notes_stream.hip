// Streaming note decoding on the device (gfx950): AMT.mpe2note (model/amt.py:179-341, mode_offset 'shorter') with its state carried forward.
//   hftt_notes_stream_step  S streams, each with its four rolls as a ring of H rows -> the notes that no later row can change
// See include/hftt_hip.h for the contract and the finality rules; tests/notes_stream_emul.py is the same walk in numpy, statement for
// statement.  One lane per (stream, pitch) walks the rows c .. row_end of its pitch sequentially: N is the contiguous axis of the rings, so the
// lanes of a wave read neighbouring words of one row while they are in step.  No atomics: a count pass, a prefix sum over (stream, pitch), and
// an emit pass that alone commits the state, so a call without room leaves the state as it was.
#include <limits.h>
#include <math.h>
#include "hftt_common.h"
#include "block_scan.h"
#include "hftt_launch.h"
#include "../../include/hftt_hip.h"

namespace {

constexpr int WG = 128;                       // lanes per workgroup = the largest N: one workgroup per stream
constexpr int SCAN = 256;                     // block_scan (block_scan.h) is written for four waves

// the record of one (stream, pitch): all zero = a fresh stream
struct rec {
  long c;                                     // commit frame: every onset peak in front of it has been returned, or is the head
  long w;                                     // row_end at the last committed call
  long head;                                  // frame + 1 of the one pending onset in front of c; 0 = none
  double head_time;
  int head_vel;
  int flags;                                  // 1: closed and decoded; 2: overflow
  float on_m1, on_pv, off_m1, off_pv;         // on / off[c - 1] and the value of the run in front of the run that holds c - 1
  long pad;
};
static_assert(sizeof(rec) == 64, "hftt_notes_stream_state_bytes counts 64 bytes per record");
enum { F_DONE = 1, F_OVERFLOW = 2 };
enum { FOUND = 0, UNDEC, END, PASSED };
enum { NO = 0, PEAK, OPEN };

// one pitch track inside the ring: rows c .. W lie at ring rows (cb + i - c) mod H with W - c <= H; row c - 1 is the record's
struct track {
  const float* a;                             // the ring of this (stream, pitch), row stride N
  long c;
  int cb, H, N;
  float m1;
};

__device__ __forceinline__ long ring_at(long c, int cb, int H, int N, long i) {
  int k = cb + (int)(i - c);
  if (k >= H) k -= H;
  k = k < 0 ? 0 : (k >= H ? H - 1 : k);       // c <= i < c + H by construction (the overflow check in front of the walk); never outside the ring
  return (long)k * N;
}

__device__ __forceinline__ float tget(const track& t, long i) { return i == t.c - 1 ? t.m1 : t.a[ring_at(t.c, t.cb, t.H, t.N, i)]; }

// the run of a track that holds a frame, moved forward run by run; rows below W only
struct cursor {
  long s, e;
  float v, pv, nv;
  bool open, valid;
};

__device__ __forceinline__ void cur_extend(cursor& q, const track& t, long W) {
  long i = q.s + 1;
  while (i < W && tget(t, i) == q.v) i++;
  q.e = i - 1;
  q.open = i == W;
  q.nv = q.open ? -INFINITY : tget(t, i);
}

__device__ __forceinline__ void cur_init(cursor& q, const track& t, long W, float pv) {
  q.valid = t.c < W;
  q.s = q.e = t.c; q.v = q.pv = q.nv = 0.f; q.open = true;
  if (!q.valid) return;
  q.v = tget(t, t.c);
  q.pv = t.c == 0 ? -INFINITY : (q.v != t.m1 ? t.m1 : pv);
  cur_extend(q, t, W);
}

__device__ __forceinline__ void cur_next(cursor& q, const track& t, long W) {
  q.s = q.e + 1; q.pv = q.v; q.v = q.nv;
  cur_extend(q, t, W);
}

__device__ __forceinline__ int cur_status(const cursor& q, float thr, bool closed) {
  if (!(q.v >= thr && q.v > q.pv)) return NO;
  if (q.open) return closed ? PEAK : OPEN;
  return q.v > q.nv ? PEAK : NO;
}

// the first peak frame >= from: FOUND (*at) | UNDEC (*at: the first frame >= from that is undecided) | PASSED: no peak up to L, all decided |
// END: no peak below W, all decided.  The cursor stays on the run of the answer.
__device__ __forceinline__ int cur_find(cursor& q, const track& t, long W, float thr, bool closed, long from, long L, long* at) {
  *at = -1;
  for (;;) {
    if (!q.valid) return END;
    if (from > q.e) {
      if (q.open) return END;
      cur_next(q, t, W);
      continue;
    }
    const long start = from > q.s ? from : q.s;
    if (start > L) return PASSED;
    const int st = cur_status(q, thr, closed);
    if (st != NO) { *at = start; return st == OPEN ? UNDEC : FOUND; }
    if (q.open) return END;
    cur_next(q, t, W);
  }
}

// time of the peak at frame i (model/amt.py _pick_peaks): i * hop in double at frame 0, at the file's last frame and between equal neighbours,
// else the fp32 refinement of notes.hip's peak_time, never contracted.  A peak decided before the close is never the last row.
__device__ __forceinline__ double ptime(const track& t, long i, long W, bool closed, double hop, float h2) {
#pragma clang fp contract(off)
  const double tm = (double)i * hop;
  if (i == 0 || (closed && i == W - 1)) return tm;
  const float l = tget(t, i - 1), c = tget(t, i), r = tget(t, i + 1);
  if (l > r) return (double)__fsub_rn((float)tm, __fdiv_rn(__fmul_rn(h2, __fsub_rn(l, r)), __fsub_rn(c, r)));
  if (l < r) return (double)__fadd_rn((float)tm, __fdiv_rn(__fmul_rn(h2, __fsub_rn(r, l)), __fsub_rn(c, l)));
  return tm;
}

__device__ __forceinline__ double dmin(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ long lmin(long a, long b) { return b < a ? b : a; }

// (cur, pv) of a track carried from frame c to frame c_new
__device__ __forceinline__ void carry(const track& t, long c_new, float* m1, float* pv) {
  float cur = *m1, p = *pv;
  for (long i = t.c; i < c_new; i++) {
    const float v = tget(t, i);
    if (i == 0) { cur = v; p = -INFINITY; }
    else if (v != cur) { p = cur; cur = v; }
  }
  *m1 = cur; *pv = p;
}

struct stream_args {
  hftt_notes_stream_desc d;
  int* counts;                                // [S * N] behind the records, zero between calls
};

// One pitch of one stream, one step.  Returns the number of notes that are final; EMIT: writes them from record `base` on and commits the
// record.  r: the record as loaded.
template <bool EMIT>
__device__ int walk(const stream_args& g, int s, int j, long W, bool closed, const rec& r, rec* out, long base, float h2) {
#pragma clang fp contract(off)
  const hftt_notes_stream_desc& d = g.d;
  const int H = d.H, N = d.N;
  const long c = r.c;
  const int cb = (int)(c % H);
  const long ring = ((long)s * H) * N + j;
  const track on = {(const float*)d.onset + ring, c, cb, H, N, r.on_m1};
  const track off = {(const float*)d.offset + ring, c, cb, H, N, r.off_m1};
  const float* mp = (const float*)d.mpe + ring;
  const signed char* vl = (const signed char*)d.velocity + ring;
  const double hop = d.hop_sec;
  const bool keep_zero = d.mode_velocity != 0;
  cursor oc, fc;
  cur_init(oc, on, W, r.on_pv);
  cur_init(fc, off, W, r.off_pv);
  auto vel = [&](long i) { return (int)vl[ring_at(c, cb, H, N, i)]; };
  auto below = [&](long a, long b) {           // the first frame of [a, min(b, W)) below thred_mpe; -1: none
    const long e = lmin(b, W);
    for (long i = a; i < e; i++)
      if (mp[ring_at(c, cb, H, N, i)] < d.thred_mpe) return i;
    return -1l;
  };
  int n = 0;
  const long head = r.head - 1;
  long new_head = -1, c_new = W;
  double ft = r.head_time;
  int fv = r.head_vel;
  long f = head;
  bool have = head >= 0;
  if (!have) {
    const int kind = cur_find(oc, on, W, d.thred_onset, closed, c, W, &f);
    have = kind == FOUND;
    if (kind == UNDEC) c_new = f;
  }
  while (have) {
    bool kept = true;
    if (f != head) {
      fv = vel(f);
      kept = keep_zero || fv > 0;
      if (kept) ft = ptime(on, f, W, closed, hop, h2);
    }
    const long x = f + 1 > c ? f + 1 : c;
    long ln;
    const int kind = cur_find(oc, on, W, d.thred_onset, closed, x, W, &ln);
    if (!kept) {                              // a dropped onset: it only ended the note in front of it
      if (kind == FOUND) { f = ln; continue; }
      c_new = kind == UNDEC ? ln : W;
      break;
    }
    bool final = false;
    double val = 0.0;
    long d_on = W;
    if (kind == FOUND) {                      // case A: the next onset peak is known
      const double tn = ptime(on, ln, W, closed, hop, h2);
      const long m = below(x, ln);
      long p;
      const int k2 = cur_find(fc, off, W, d.thred_offset, closed, x, ln, &p);
      if (k2 == UNDEC) {
        c_new = lmin(lmin(ln, p), m >= 0 ? m : ln);
      } else {
        const long loff = k2 == FOUND ? p : ln;
        const double toff = k2 == FOUND ? ptime(off, p, W, closed, hop, h2) : tn;
        val = m < 0 || loff <= m ? toff : (double)m * hop;
        if (keep_zero || vel(ln) > 0) val = dmin(val, tn);
        else if (ln + 1 <= oc.e && (keep_zero || vel(ln + 1) > 0)) val = dmin(val, ptime(on, ln + 1, W, closed, hop, h2));
        final = true;
      }
    } else if (closed) {                      // the file's last onset
      long p;
      const int k2 = cur_find(fc, off, W, d.thred_offset, closed, x, W, &p);
      const long m = below(x, W);
      if (k2 == FOUND) val = m < 0 || p <= m ? ptime(off, p, W, closed, hop, h2) : (double)m * hop;
      else val = m >= 0 ? (double)m * hop : (double)(W - 1) * hop;
      final = true;
    } else {                                  // case B: no onset peak decided behind f
      d_on = kind == UNDEC ? ln : W;
      long p;
      const int k2 = cur_find(fc, off, W, d.thred_offset, closed, x, W, &p);
      const long lim = k2 == END ? W : p;
      const long m = below(x, lim);
      long ev = -1;
      if (m >= 0) { ev = m; val = (double)m * hop; }
      else if (k2 == FOUND) { ev = p; val = ptime(off, p, W, closed, hop, h2); }
      if (ev >= 0 && d_on > ev + 1) final = true;
      else c_new = lmin(lmin(d_on, lim), m >= 0 ? m : W);
    }
    if (!final) { new_head = f; break; }      // f waits as the head
    if constexpr (EMIT) {
      const long idx = base + n;
      if (idx >= 0 && idx < d.cap) {
        ((int*)d.out_pitch)[idx] = j + d.note_min;
        ((int*)d.out_velocity)[idx] = fv;
        ((double*)d.out_onset)[idx] = ft;
        ((double*)d.out_offset)[idx] = val;
      }
    }
    n++;
    if (kind != FOUND) { c_new = closed ? W : d_on; break; }
    f = ln;
  }
  if constexpr (EMIT) {
    rec o = r;
    o.c = c_new; o.w = W; o.head = new_head + 1;
    o.head_time = new_head >= 0 ? ft : 0.0;
    o.head_vel = new_head >= 0 ? fv : 0;
    o.flags = closed ? F_DONE : 0;
    carry(on, c_new, &o.on_m1, &o.on_pv);
    carry(off, c_new, &o.off_m1, &o.off_pv);
    *out = o;
  }
  return n;
}

// what both passes decide first, the same way: the lane's record, the stream's horizon, and whether the stream's rows are still in the ring
struct lane_in {
  rec r;
  long W;
  bool active, closed, done, overflow;        // overflow: of the whole stream (any pitch)
};

__device__ __forceinline__ lane_in lane_load(const stream_args& g, int s, int j) {
  const hftt_notes_stream_desc& d = g.d;
  lane_in in;
  in.active = j < d.N;
  in.W = ((const long*)d.row_end)[s];
  in.closed = ((const int*)d.closed)[s] != 0;
  in.r = rec{};
  if (in.active) in.r = ((const rec*)d.state)[(long)s * d.N + j];
  in.done = (in.r.flags & F_DONE) != 0;
  const bool lost = in.active && ((in.r.flags & F_OVERFLOW) || (!in.done && (in.W < in.r.w || in.W - in.r.c > d.H || in.W - in.r.w > d.H)));
  in.overflow = __syncthreads_or(lost) != 0;
  return in;
}

__global__ __launch_bounds__(WG) void notes_stream_count_kernel(const stream_args g, float h2) {
  const int s = blockIdx.x, j = threadIdx.x;
  const lane_in in = lane_load(g, s, j);
  if (!in.active) return;
  int n = 0;
  if (!in.overflow && !in.done) n = walk<false>(g, s, j, in.W, in.closed, in.r, nullptr, 0, h2);
  g.counts[(long)s * g.d.N + j] = n;
}

// counts [n] -> their exclusive prefix sums in place; *total = the number of notes of this call
__global__ __launch_bounds__(SCAN) void notes_stream_offsets_kernel(int* cnt, int n, int* total) {
  __shared__ int slot[4];
  __shared__ int bc;
  const int tid = threadIdx.x;
  int carry = 0;
  for (int i0 = 0; i0 < n; i0 += SCAN) {
    const int i = i0 + tid;
    int ex;
    const int inc = block_scan<OpAdd, false>(i < n ? cnt[i] : 0, slot, ex);
    if (i < n) cnt[i] = carry + ex;
    if (tid == SCAN - 1) bc = carry + inc;
    __syncthreads();
    carry = bc;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

__global__ __launch_bounds__(WG) void notes_stream_emit_kernel(const stream_args g, float h2) {
  const hftt_notes_stream_desc& d = g.d;
  const int s = blockIdx.x, j = threadIdx.x;
  const lane_in in = lane_load(g, s, j);
  if (!in.active) return;
  const long e = (long)s * d.N + j;
  const int base = g.counts[e];
  const int total = *(const int*)d.n_notes;
  g.counts[e] = 0;                            // the scratch is zero between calls: the state of an untouched stream stays bit-identical
  if (j == 0) {
    ((int*)d.stream_notes)[s] = base;
    if (s == d.S - 1) ((int*)d.stream_notes)[d.S] = total;
    ((int*)d.overflow)[s] = in.overflow ? 1 : 0;
  }
  if (total > d.cap) return;                  // no room: nothing is written, nothing committed
  rec* out = (rec*)d.state + e;
  if (in.overflow) {
    if (!(in.r.flags & F_OVERFLOW)) out->flags = in.r.flags | F_OVERFLOW;
    return;
  }
  if (in.done) return;
  walk<true>(g, s, j, in.W, in.closed, in.r, out, base, h2);
}

}  // namespace

extern "C" int64_t hftt_notes_stream_state_bytes(int32_t S, int32_t N) {
  if (S < 1 || N < 1 || N > 128 || (long)S * N >= (1l << 24)) return 0;
  return (int64_t)(sizeof(rec) + sizeof(int)) * S * N;
}

extern "C" int hftt_notes_stream_step(const hftt_notes_stream_desc* d, void* stream) {
  const char* what = "notes_stream_step";
  HFTT_REQUIRE(d, "notes_stream_step: null descriptor");
  HFTT_REQUIRE(d->S >= 1, "notes_stream_step: S=%d must be positive", d->S);
  HFTT_REQUIRE(d->N >= 1 && d->N <= 128, "notes_stream_step: N=%d outside 1..128", d->N);
  HFTT_REQUIRE((long)d->S * d->N < (1l << 24), "notes_stream_step: S=%d streams of N=%d exceed 2^24 records", d->S, d->N);
  HFTT_REQUIRE(d->H >= 4, "notes_stream_step: H=%d ring rows, at least 4", d->H);
  HFTT_REQUIRE((long)d->S * d->H * d->N < (1l << 40), "notes_stream_step: S=%d rings of H=%d x N=%d exceed 2^40 elements", d->S, d->H, d->N);
  HFTT_REQUIRE(d->max_new >= 0 && d->max_new <= d->H, "notes_stream_step: max_new=%d new rows outside 0..H=%d (the ring cannot take them)", d->max_new, d->H);
  HFTT_REQUIRE(d->mode_velocity == 0 || d->mode_velocity == 1, "notes_stream_step: mode_velocity=%d (0 = ignore_zero, 1 = org)", d->mode_velocity);
  HFTT_REQUIRE(d->mode_offset == 0, "notes_stream_step: mode_offset=%d: a stream decodes mode_offset 'shorter' (0) only -- under 'longer' / 'offset' a note "
               "may wait for an offset peak anywhere later in the file", d->mode_offset);
  HFTT_REQUIRE(d->cap >= 0, "notes_stream_step: cap=%d is negative", d->cap);
  HFTT_REQUIRE(d->onset && d->offset && d->mpe && d->velocity, "notes_stream_step: null ring (onset / offset / mpe / velocity)");
  HFTT_REQUIRE(d->row_end && d->closed, "notes_stream_step: null table (row_end / closed)");
  HFTT_REQUIRE(d->stream_notes && d->n_notes && d->overflow, "notes_stream_step: null count (stream_notes / n_notes / overflow)");
  HFTT_REQUIRE(d->cap == 0 || (d->out_pitch && d->out_velocity && d->out_onset && d->out_offset),
               "notes_stream_step: null output (out_pitch / out_velocity / out_onset / out_offset) at cap=%d", d->cap);
  HFTT_REQUIRE(d->state, "notes_stream_step: state is null");
  const int64_t need = hftt_notes_stream_state_bytes(d->S, d->N);
  HFTT_REQUIRE(d->state_bytes >= need, "notes_stream_step: state_bytes=%ld below hftt_notes_stream_state_bytes(S, N)=%ld", (long)d->state_bytes, (long)need);
  stream_args a;
  a.d = *d;
  a.counts = (int*)((char*)d->state + sizeof(rec) * (size_t)d->S * d->N);
  const float h2 = (float)(d->hop_sec * 0.5);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = hftt_launch<notes_stream_count_kernel>(what, dim3((unsigned)d->S), dim3(WG), 0, st, a, h2)) return rc;
  if (int rc = hftt_launch<notes_stream_offsets_kernel>(what, dim3(1), dim3(SCAN), 0, st, a.counts, d->S * d->N, (int*)d->n_notes)) return rc;
  return hftt_launch<notes_stream_emit_kernel>(what, dim3((unsigned)d->S), dim3(WG), 0, st, a, h2);
}
