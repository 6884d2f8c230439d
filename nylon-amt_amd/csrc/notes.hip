// Note decoding on the device (gfx950): the host half of AMT.transcript / transcript_stride / mpe2note (model/amt.py) as kernels.
//   hftt_stitch        a batch of model outputs -> rows of the file-long rolls, velocity logits -> int8 argmax (model/amt.py transcript)
//   hftt_notes_decode  the four rolls of one file -> the note list of AMT.mpe2note before its final sort, pitch-major, ascending onset frame
// See include/hftt_hip.h for the contract.  No atomics anywhere: every output element has one writer, and the note order comes from prefix sums.
#include <limits.h>
#include <math.h>
#include "hftt_common.h"
#include "block_scan.h"
#include "hftt_launch.h"
#include "../../include/hftt_hip.h"

namespace {

constexpr int CH = HFTT_NOTES_CHUNK;          // frames per chunk = threads per workgroup: one frame per thread
static_assert(CH == 256, "block_scan (block_scan.h) is written for four waves");

// ---------------------------------------------------------------------------------------------------------------------------------------
// stitch
// ---------------------------------------------------------------------------------------------------------------------------------------
struct stitch_args {
  hftt_stitch_desc d;
  int dst[HFTT_STITCH_MAX_CLIPS];             // the host array of the descriptor, by value
};

__device__ inline bool arg_gt(float a, float b) { return a > b || (a != a && b == b); }      // NaN counts as the maximum (torch / numpy argmax)

// L = 1 << lshift lanes share one (clip, row, note) element: lane `sub` reads classes sub * VEC + i * L * VEC .. (VEC = 4: one 16-byte load, so a
// half wave reads the 512 contiguous bytes of V = 128), keeps its first maximum, and a butterfly over the L lanes picks the larger value, the
// lower index among equals.  Lane 0 of the group copies the element's three posteriors and writes the class.
template <int VEC>
__global__ __launch_bounds__(256) void stitch_kernel(const stitch_args g, int lshift) {
  const hftt_stitch_desc& d = g.d;
  const int L = 1 << lshift;
  const long gt = (long)blockIdx.x * 256 + threadIdx.x;
  const long e = gt >> lshift;
  const int sub = (int)(gt & (L - 1));
  const long E = (long)d.b * d.len * d.N;
  const bool valid = e < E;
  long src = 0, dst = 0;
  if (valid) {
    const int n = (int)(e % d.N);
    const long cr = e / d.N;
    const int r = (int)(cr % d.len), c = (int)(cr / d.len);
    src = ((long)c * d.T + d.src0 + r) * d.N + n;
    dst = ((long)g.dst[c] + r) * d.N + n;
  }
  float best = 0.f;
  int bi = -1;
  if (valid) {
    const float* v = (const float*)d.velocity + src * d.V;
    for (int i = sub * VEC; i < d.V; i += L * VEC) {
      if constexpr (VEC == 4) {
        const float4 q = *(const float4*)(v + i);
        const float x[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int u = 0; u < 4; u++)
          if (bi < 0 || arg_gt(x[u], best)) { best = x[u]; bi = i + u; }
      } else {
        const float x = v[i];
        if (bi < 0 || arg_gt(x, best)) { best = x; bi = i; }
      }
    }
  }
  for (int s = L >> 1; s > 0; s >>= 1) {
    const float ov = __shfl_xor(best, s);
    const int oi = __shfl_xor(bi, s);
    if (oi >= 0 && (bi < 0 || arg_gt(ov, best) || (!arg_gt(best, ov) && oi < bi))) { best = ov; bi = oi; }
  }
  if (valid && sub == 0) {
    ((float*)d.roll_onset)[dst] = ((const float*)d.onset)[src];
    ((float*)d.roll_offset)[dst] = ((const float*)d.offset)[src];
    ((float*)d.roll_mpe)[dst] = ((const float*)d.mpe)[src];
    ((signed char*)d.roll_velocity)[dst] = (signed char)bi;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// notes: per (pitch, chunk) state in the workspace, 8 ints each, then one count per (pitch, chunk)
// ---------------------------------------------------------------------------------------------------------------------------------------
enum { ST_RS_ON = 0, ST_RS_OFF, ST_RE_ON, ST_RE_OFF, ST_NX_ON, ST_NX_OFF, ST_NX_BELOW, ST_NX_KEPT, ST_INTS };

// _pick_peaks (model/amt.py) for frame f of one pitch track `a` (stride N): frame f is a peak when a[f] >= thr and the value of the run before
// its run and of the run after it are smaller (or there is none).  Run start s and run end e come from a prefix max / suffix min over the
// chunk's run boundaries; a run that reaches over the chunk's border takes them from the carries rs_first / re_last.  Returns e through e_out.
template <int S0>
__device__ bool peak_of(const float* a, int N, int F, int f, bool valid, float thr, int rs_first, int re_last, int (*slots)[4], int* e_out) {
  float v = 0.f;
  bool st = false, en = false;
  if (valid) {
    v = a[(long)f * N];
    st = f == 0 || a[(long)(f - 1) * N] != v;
    en = f == F - 1 || a[(long)(f + 1) * N] != v;
  }
  int ex;
  int s = block_scan<OpMax, false>(st ? f : -1, slots[S0], ex);
  int e = block_scan<OpMin, true>(en ? f : INT_MAX, slots[S0 + 1], ex);
  if (s < 0) s = rs_first;
  if (e == INT_MAX) e = re_last;
  *e_out = e;
  if (!valid) return false;
  const float prev = s > 0 ? a[(long)(s - 1) * N] : -INFINITY;
  const float next = e < F - 1 ? a[(long)(e + 1) * N] : -INFINITY;
  return v >= thr && v > prev && v > next;
}

// time of the peak at frame i (model/amt.py _pick_peaks): i * hop in double at the edges and between equal neighbours, else the fp32 refinement
// float32(i * hop) -/+ (h2 * (l - r)) / (c - r): fp32 subtract, multiply, correctly rounded divide, subtract, never contracted
__device__ double peak_time(const float* a, int N, int F, int i, double hop, float h2) {
#pragma clang fp contract(off)
  const double t = (double)i * hop;
  if (i == 0 || i == F - 1) return t;
  const float l = a[(long)(i - 1) * N], c = a[(long)i * N], r = a[(long)(i + 1) * N];
  if (l > r) return (double)__fsub_rn((float)t, __fdiv_rn(__fmul_rn(h2, __fsub_rn(l, r)), __fsub_rn(c, r)));
  if (l < r) return (double)__fadd_rn((float)t, __fdiv_rn(__fmul_rn(h2, __fsub_rn(r, l)), __fsub_rn(c, l)));
  return t;
}

// One workgroup per pitch.  Forward over the chunks: the run start at every chunk's first frame (both tracks).  Backward over the chunks: the
// run end at every chunk's last frame, the next onset peak / offset peak / frame below thred_mpe / kept onset behind every chunk, and the
// number of kept notes in it.  Two carried ints per track and direction; a run is decided in the chunk that holds the frame.
__global__ __launch_bounds__(CH) void notes_scan_kernel(const hftt_notes_desc g, int nchunks) {
  __shared__ int slots[16][4];
  __shared__ int bc[8];
  const int tid = threadIdx.x, j = blockIdx.x, N = g.N, F = (int)g.F;
  const float* on = (const float*)g.onset + j;
  const float* off = (const float*)g.offset + j;
  const float* mp = (const float*)g.mpe + j;
  const signed char* vel = (const signed char*)g.velocity + j;
  int* st = (int*)g.ws + (long)j * nchunks * ST_INTS;
  int* cnt = (int*)g.ws + (long)N * nchunks * ST_INTS + (long)j * nchunks;
  int rs_on = 0, rs_off = 0;
  for (int k = 0; k < nchunks; k++) {
    const int f = k * CH + tid;
    if (tid == 0) { st[k * ST_INTS + ST_RS_ON] = rs_on; st[k * ST_INTS + ST_RS_OFF] = rs_off; }
    bool s1 = false, s2 = false;
    if (f < F) {
      s1 = f == 0 || on[(long)(f - 1) * N] != on[(long)f * N];
      s2 = f == 0 || off[(long)(f - 1) * N] != off[(long)f * N];
    }
    int ex;
    const int a = block_scan<OpMax, false>(s1 ? f : -1, slots[0], ex);
    const int b = block_scan<OpMax, false>(s2 ? f : -1, slots[1], ex);
    if (tid == CH - 1) { bc[0] = a < 0 ? rs_on : a; bc[1] = b < 0 ? rs_off : b; }
    __syncthreads();
    rs_on = bc[0]; rs_off = bc[1];
  }
  int re_on = F - 1, re_off = F - 1, nx_on = F, nx_off = F, nx_bl = F, nx_kp = F;
  for (int k = nchunks - 1; k >= 0; k--) {
    const int f = k * CH + tid;
    const bool valid = f < F;
    int e_on, e_off, ex;
    const bool p_on = peak_of<2>(on, N, F, f, valid, g.thred_onset, st[k * ST_INTS + ST_RS_ON], re_on, slots, &e_on);
    const bool p_off = peak_of<4>(off, N, F, f, valid, g.thred_offset, st[k * ST_INTS + ST_RS_OFF], re_off, slots, &e_off);
    const bool below = valid && mp[(long)f * N] < g.thred_mpe;
    const bool kept = p_on && (g.mode_velocity != 0 || vel[(long)f * N] > 0);
    const int m_on = block_scan<OpMin, true>(p_on ? f : INT_MAX, slots[6], ex);
    const int m_off = block_scan<OpMin, true>(p_off ? f : INT_MAX, slots[7], ex);
    const int m_bl = block_scan<OpMin, true>(below ? f : INT_MAX, slots[8], ex);
    const int m_kp = block_scan<OpMin, true>(kept ? f : INT_MAX, slots[9], ex);
    const int c = block_scan<OpAdd, true>(kept ? 1 : 0, slots[10], ex);
    if (tid == 0) {
      int* s = st + k * ST_INTS;
      s[ST_RE_ON] = re_on; s[ST_RE_OFF] = re_off;
      s[ST_NX_ON] = nx_on; s[ST_NX_OFF] = nx_off; s[ST_NX_BELOW] = nx_bl; s[ST_NX_KEPT] = nx_kp;
      cnt[k] = c;
      bc[0] = e_on; bc[1] = e_off;
      bc[2] = OpMin::f(m_on, nx_on); bc[3] = OpMin::f(m_off, nx_off); bc[4] = OpMin::f(m_bl, nx_bl); bc[5] = OpMin::f(m_kp, nx_kp);
    }
    __syncthreads();
    re_on = bc[0]; re_off = bc[1]; nx_on = bc[2]; nx_off = bc[3]; nx_bl = bc[4]; nx_kp = bc[5];
  }
}

// counts [n] (pitch-major, chunks ascending) -> their exclusive prefix sums in place; *total = the number of notes that exist
__global__ __launch_bounds__(CH) void notes_offsets_kernel(int* cnt, int n, int* total) {
  __shared__ int slot[4];
  __shared__ int bc;
  const int tid = threadIdx.x;
  int carry = 0;
  for (int i0 = 0; i0 < n; i0 += CH) {
    const int i = i0 + tid;
    int ex;
    const int inc = block_scan<OpAdd, false>(i < n ? cnt[i] : 0, slot, ex);
    if (i < n) cnt[i] = carry + ex;
    if (tid == CH - 1) bc = carry + inc;
    __syncthreads();
    carry = bc;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// One workgroup per (chunk, pitch): the per-onset part of AMT.mpe2note (model/amt.py), one thread per frame, for the onsets that are kept.
__global__ __launch_bounds__(CH) void notes_emit_kernel(const hftt_notes_desc g, int nchunks, float h2) {
  __shared__ int slots[16][4];
  const int tid = threadIdx.x, k = blockIdx.x, j = blockIdx.y, N = g.N, F = (int)g.F;
  const float* on = (const float*)g.onset + j;
  const float* off = (const float*)g.offset + j;
  const float* mp = (const float*)g.mpe + j;
  const signed char* vel = (const signed char*)g.velocity + j;
  const int* st = (const int*)g.ws + ((long)j * nchunks + k) * ST_INTS;
  const int base = ((const int*)g.ws)[(long)N * nchunks * ST_INTS + (long)j * nchunks + k];
  const int f = k * CH + tid;
  const bool valid = f < F;
  int e, x_on, x_off, x_bl, x_kp, rank;
  const bool p_on = peak_of<0>(on, N, F, f, valid, g.thred_onset, st[ST_RS_ON], st[ST_RE_ON], slots, &e);
  const bool p_off = peak_of<2>(off, N, F, f, valid, g.thred_offset, st[ST_RS_OFF], st[ST_RE_OFF], slots, &e);
  const bool below = valid && mp[(long)f * N] < g.thred_mpe;
  const int velocity = p_on ? (int)vel[(long)f * N] : 0;
  const bool kept = p_on && (g.mode_velocity != 0 || velocity > 0);
  block_scan<OpMin, true>(p_on ? f : INT_MAX, slots[4], x_on);
  block_scan<OpMin, true>(p_off ? f : INT_MAX, slots[5], x_off);
  block_scan<OpMin, true>(below ? f : INT_MAX, slots[6], x_bl);
  block_scan<OpMin, true>(kept ? f : INT_MAX, slots[7], x_kp);
  block_scan<OpAdd, false>(kept ? 1 : 0, slots[8], rank);
  if (!kept) return;
  const long idx = (long)base + rank;
  if (idx >= g.cap) return;
  const double hop = g.hop_sec;
  const int nxt_on = OpMin::f(x_on, st[ST_NX_ON]), nxt_off = OpMin::f(x_off, st[ST_NX_OFF]);      // first onset / offset peak behind f, F = none
  const int nxt_bl = OpMin::f(x_bl, st[ST_NX_BELOW]), nxt_kp = OpMin::f(x_kp, st[ST_NX_KEPT]);    // first frame >= f + 1 below thred_mpe; next kept onset
  const double time_onset = peak_time(on, N, F, f, hop, h2);
  const int loc_next = nxt_on;
  const double time_next = nxt_on < F ? peak_time(on, N, F, nxt_on, hop, h2) : (double)(F - 1) * hop;
  const bool flag_offset = nxt_off < F;
  int loc_offset = f + 1;
  double time_offset = 0.0;
  if (flag_offset) {
    loc_offset = nxt_off;
    time_offset = peak_time(off, N, F, nxt_off, hop, h2);
    if (loc_offset > loc_next) { loc_offset = loc_next; time_offset = time_next; }
  }
  const bool flag_mpe = nxt_bl < loc_next;
  const int loc_mpe = flag_mpe ? nxt_bl : f + 1;
  const double time_mpe = (double)loc_mpe * hop;
  double offset_value;
  if (!flag_offset && !flag_mpe) offset_value = time_next;
  else if (flag_offset && !flag_mpe) offset_value = time_offset;
  else if (!flag_offset && flag_mpe) offset_value = time_mpe;
  else if (g.mode_offset == 2) offset_value = time_offset;
  else if (g.mode_offset == 1) offset_value = loc_offset >= loc_mpe ? time_offset : time_mpe;
  else offset_value = loc_offset <= loc_mpe ? time_offset : time_mpe;
  if (nxt_kp < F) {                                    // the trim between consecutive kept notes of one pitch
    const double t = nxt_kp == nxt_on ? time_next : peak_time(on, N, F, nxt_kp, hop, h2);
    if (t < offset_value) offset_value = t;
  }
  ((int*)g.out_pitch)[idx] = j + g.note_min;
  ((int*)g.out_velocity)[idx] = velocity;
  ((double*)g.out_onset)[idx] = time_onset;
  ((double*)g.out_offset)[idx] = offset_value;
}

inline long notes_chunks(long F) { return (F + CH - 1) / CH; }

}  // namespace

extern "C" int hftt_stitch(const hftt_stitch_desc* d, void* stream) {
  HFTT_REQUIRE(d, "stitch: null descriptor");
  HFTT_REQUIRE(d->onset && d->offset && d->mpe && d->velocity, "stitch: null operand (onset / offset / mpe / velocity)");
  HFTT_REQUIRE(d->roll_onset && d->roll_offset && d->roll_mpe && d->roll_velocity, "stitch: null roll (roll_onset / roll_offset / roll_mpe / roll_velocity)");
  HFTT_REQUIRE(d->dst, "stitch: dst is null (a HOST array of b first rows)");
  HFTT_REQUIRE(d->b >= 1 && d->b <= HFTT_STITCH_MAX_CLIPS, "stitch: b=%d outside 1..%d", d->b, HFTT_STITCH_MAX_CLIPS);
  HFTT_REQUIRE(d->T >= 1, "stitch: T=%d must be positive", d->T);
  HFTT_REQUIRE(d->N >= 1 && d->N <= 128, "stitch: N=%d outside 1..128", d->N);
  HFTT_REQUIRE(d->V >= 1 && d->V <= 128, "stitch: V=%d outside 1..128 (the class is stored as int8)", d->V);
  HFTT_REQUIRE(d->F >= 0, "stitch: F=%ld is negative", (long)d->F);
  HFTT_REQUIRE((long)d->F * d->N < (1l << 31), "stitch: F=%ld rows of N=%d exceed 2^31 elements", (long)d->F, d->N);
  HFTT_REQUIRE(d->len >= 1 && d->len <= d->T, "stitch: len=%d outside 1..T=%d", d->len, d->T);
  HFTT_REQUIRE(d->src0 >= 0 && d->src0 <= d->T - d->len, "stitch: src0=%d outside 0..T-len=%d", d->src0, d->T - d->len);
  stitch_args a;
  a.d = *d;
  for (int c = 0; c < HFTT_STITCH_MAX_CLIPS; c++) a.dst[c] = 0;
  for (int c = 0; c < d->b; c++) {
    HFTT_REQUIRE(d->dst[c] >= 0 && (long)d->dst[c] + d->len <= (long)d->F, "stitch: dst[%d]=%d outside 0..F-len=%ld", c, d->dst[c], (long)d->F - d->len);
    for (int p = 0; p < c; p++)
      HFTT_REQUIRE(d->dst[p] + d->len <= d->dst[c] || d->dst[c] + d->len <= d->dst[p], "stitch: dst[%d]=%d and dst[%d]=%d overlap at len=%d (one writer per row)", p, d->dst[p], c, d->dst[c], d->len);
    a.dst[c] = d->dst[c];
  }
  a.d.dst = nullptr;
  const bool vec = d->V % 4 == 0 && ((uintptr_t)d->velocity & 15) == 0;
  const int per = vec ? d->V / 4 : d->V;               // loads that cover one element's classes
  int lshift = 0;
  while ((1 << lshift) < per && lshift < 6) lshift++;
  const long threads = ((long)d->b * d->len * d->N) << lshift;
  const dim3 grid((unsigned)((threads + 255) / 256));
  if (vec) return hftt_launch<stitch_kernel<4>>("stitch", grid, dim3(256), 0, (hipStream_t)stream, a, lshift);
  return hftt_launch<stitch_kernel<1>>("stitch", grid, dim3(256), 0, (hipStream_t)stream, a, lshift);
}

extern "C" int64_t hftt_notes_ws_bytes(int64_t F, int32_t N) {
  if (F < 0 || N < 1 || N > 128) return 0;
  return 64 + 4 * (int64_t)(ST_INTS + 1) * N * notes_chunks(F);
}

extern "C" int hftt_notes_decode(const hftt_notes_desc* d, void* stream) {
  HFTT_REQUIRE(d, "notes_decode: null descriptor");
  HFTT_REQUIRE(d->F >= 0, "notes_decode: F=%ld is negative", (long)d->F);
  HFTT_REQUIRE(d->N >= 1 && d->N <= 128, "notes_decode: N=%d outside 1..128", d->N);
  HFTT_REQUIRE((long)d->F * d->N < (1l << 31), "notes_decode: F=%ld frames of N=%d exceed 2^31 elements (the note count is an int32)", (long)d->F, d->N);
  HFTT_REQUIRE(d->cap >= 0, "notes_decode: cap=%d is negative", d->cap);
  HFTT_REQUIRE(d->mode_velocity == 0 || d->mode_velocity == 1, "notes_decode: mode_velocity=%d (0 = ignore_zero, 1 = org)", d->mode_velocity);
  HFTT_REQUIRE(d->mode_offset >= 0 && d->mode_offset <= 2, "notes_decode: mode_offset=%d (0 = shorter, 1 = longer, 2 = offset)", d->mode_offset);
  HFTT_REQUIRE(d->n_notes, "notes_decode: n_notes is null");
  HFTT_REQUIRE(d->cap == 0 || (d->out_pitch && d->out_velocity && d->out_onset && d->out_offset),
               "notes_decode: null output (out_pitch / out_velocity / out_onset / out_offset) at cap=%d", d->cap);
  HFTT_REQUIRE(d->F == 0 || (d->onset && d->offset && d->mpe && d->velocity), "notes_decode: null roll (onset / offset / mpe / velocity)");
  HFTT_REQUIRE(d->ws, "notes_decode: ws is null");
  HFTT_REQUIRE(d->ws_bytes >= hftt_notes_ws_bytes(d->F, d->N), "notes_decode: ws_bytes=%ld below hftt_notes_ws_bytes(F, N)=%ld", (long)d->ws_bytes,
               (long)hftt_notes_ws_bytes(d->F, d->N));
  const int nchunks = (int)notes_chunks(d->F);
  int* cnt = (int*)d->ws + (long)d->N * nchunks * ST_INTS;
  if (d->F == 0) {                                      // no frame, no note, no launch: the total alone is written
    if (hftt_device_guard("notes_decode") != 0) return 3;
    hipError_t e = hipMemsetAsync(d->n_notes, 0, sizeof(int), (hipStream_t)stream);
    if (e != hipSuccess) { hftt_set_error("notes_decode: clearing n_notes failed: %s", hipGetErrorString(e)); return 2; }
    return 0;
  }
  if (int rc = hftt_launch<notes_scan_kernel>("notes_decode", dim3((unsigned)d->N), dim3(CH), 0, (hipStream_t)stream, *d, nchunks)) return rc;
  if (int rc = hftt_launch<notes_offsets_kernel>("notes_decode", dim3(1), dim3(CH), 0, (hipStream_t)stream, cnt, d->N * nchunks, (int*)d->n_notes)) return rc;
  return hftt_launch<notes_emit_kernel>("notes_decode", dim3((unsigned)nchunks, (unsigned)d->N), dim3(CH), 0, (hipStream_t)stream, *d, nchunks,
                                        (float)(d->hop_sec * 0.5));
}
