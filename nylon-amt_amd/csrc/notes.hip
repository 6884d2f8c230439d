// Note decoding on the device (gfx950): the host half of AMT.transcript / transcript_stride / mpe2note (model/amt.py) as kernels.
//   hftt_stitch        a batch of model outputs -> rows of the file-long rolls, velocity logits -> int8 argmax (model/amt.py transcript)
//   hftt_notes_decode  the four rolls of one file -> the note list of AMT.mpe2note before its final sort, pitch-major, ascending onset frame
//   hftt_notes_decode_seg  the same for rolls that hold many files back to back, every file decoded on its own rows alone
//   hftt_clip_windows  the clip windows of many files (a_input[i:i+width].T with the min_value padding), transposed through LDS in one launch
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

// The four tracks of one pitch over the rows that are decoded as one file: F rows from the base pointers, stride N
struct notes_track {
  const float* on; const float* off; const float* mp;
  const signed char* vel;
  int F;
};

__device__ inline notes_track track_of(const hftt_notes_desc& g, long row0, int F, int j) {
  const long o = row0 * g.N + j;
  return {(const float*)g.onset + o, (const float*)g.offset + o, (const float*)g.mpe + o, (const signed char*)g.velocity + o, F};
}

// One workgroup per pitch (and segment).  Forward over the chunks: the run start at every chunk's first frame (both tracks).  Backward over
// the chunks: the run end at every chunk's last frame, the next onset peak / offset peak / frame below thred_mpe / kept onset behind every
// chunk, and the number of kept notes in it.  Two carried ints per track and direction; a run is decided in the chunk that holds the frame.
// st: ST_INTS ints per chunk, cnt: one int per chunk, both of this pitch's nchunks chunks.
__device__ void notes_scan_body(const hftt_notes_desc& g, const notes_track& t, int nchunks, int* st, int* cnt, int (*slots)[4], int* bc) {
  const int tid = threadIdx.x, N = g.N, F = t.F;
  const float* on = t.on;
  const float* off = t.off;
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
    const bool below = valid && t.mp[(long)f * N] < g.thred_mpe;
    const bool kept = p_on && (g.mode_velocity != 0 || t.vel[(long)f * N] > 0);
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

// one file: counts and state [pitch][chunk]
__global__ __launch_bounds__(CH) void notes_scan_kernel(const hftt_notes_desc g, int nchunks) {
  __shared__ int slots[16][4];
  __shared__ int bc[8];
  const int j = blockIdx.x;
  int* st = (int*)g.ws + (long)j * nchunks * ST_INTS;
  int* cnt = (int*)g.ws + (long)g.N * nchunks * ST_INTS + (long)j * nchunks;
  notes_scan_body(g, track_of(g, 0, (int)g.F, j), nchunks, st, cnt, slots, bc);
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

// The per-onset part of AMT.mpe2note (model/amt.py) for chunk k of one pitch, one thread per frame, for the onsets that are kept.  st: the
// chunk's ST_INTS ints of state; base: the number of notes in front of the chunk's first; j: the pitch index that the records carry.
__device__ void notes_emit_body(const hftt_notes_desc& g, const notes_track& t, int j, int k, const int* st, int base, float h2, int (*slots)[4]) {
  const int tid = threadIdx.x, N = g.N, F = t.F;
  const float* on = t.on;
  const float* off = t.off;
  const int f = k * CH + tid;
  const bool valid = f < F;
  int e, x_on, x_off, x_bl, x_kp, rank;
  const bool p_on = peak_of<0>(on, N, F, f, valid, g.thred_onset, st[ST_RS_ON], st[ST_RE_ON], slots, &e);
  const bool p_off = peak_of<2>(off, N, F, f, valid, g.thred_offset, st[ST_RS_OFF], st[ST_RE_OFF], slots, &e);
  const bool below = valid && t.mp[(long)f * N] < g.thred_mpe;
  const int velocity = p_on ? (int)t.vel[(long)f * N] : 0;
  const bool kept = p_on && (g.mode_velocity != 0 || velocity > 0);
  block_scan<OpMin, true>(p_on ? f : INT_MAX, slots[4], x_on);
  block_scan<OpMin, true>(p_off ? f : INT_MAX, slots[5], x_off);
  block_scan<OpMin, true>(below ? f : INT_MAX, slots[6], x_bl);
  block_scan<OpMin, true>(kept ? f : INT_MAX, slots[7], x_kp);
  block_scan<OpAdd, false>(kept ? 1 : 0, slots[8], rank);
  if (!kept) return;
  const long idx = (long)base + rank;
  if (idx < 0 || idx >= g.cap) return;
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
    const double tk = nxt_kp == nxt_on ? time_next : peak_time(on, N, F, nxt_kp, hop, h2);
    if (tk < offset_value) offset_value = tk;
  }
  ((int*)g.out_pitch)[idx] = j + g.note_min;
  ((int*)g.out_velocity)[idx] = velocity;
  ((double*)g.out_onset)[idx] = time_onset;
  ((double*)g.out_offset)[idx] = offset_value;
}

// one file: one workgroup per (chunk, pitch)
__global__ __launch_bounds__(CH) void notes_emit_kernel(const hftt_notes_desc g, int nchunks, float h2) {
  __shared__ int slots[16][4];
  const int k = blockIdx.x, j = blockIdx.y;
  const int* st = (const int*)g.ws + ((long)j * nchunks + k) * ST_INTS;
  const int base = ((const int*)g.ws)[(long)g.N * nchunks * ST_INTS + (long)j * nchunks + k];
  notes_emit_body(g, track_of(g, 0, (int)g.F, j), j, k, st, base, h2, slots);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// segmented notes: ws = [chunk table: tbl ints | state: ST_INTS ints per (segment, pitch, chunk) | counts: one int each], the two lists laid
// out [segment][pitch][chunk]: element N * chunk0[s] + j * nchunks_s + k, with chunk0 the table's exclusive prefix of the chunk counts
// ---------------------------------------------------------------------------------------------------------------------------------------
struct seg_args {
  hftt_notes_desc d;
  const int* seg_row0;       // device [n_seg + 1]
  int* seg_notes;            // device [n_seg + 1]
  int n_seg, tbl, chunks;    // tbl: ints of the table region; chunks: the host table's chunk total (what the workspace holds)
};

// chunk0[s] = sum over s' < s of ceil(F_s' / CH), s = 0 .. n_seg, from the DEVICE row table.  A negative length counts as none.
__global__ __launch_bounds__(CH) void notes_seg_table_kernel(const seg_args a) {
  __shared__ int slot[4];
  __shared__ int bc;
  const int tid = threadIdx.x;
  int* chunk0 = (int*)a.d.ws;
  int carry = 0;
  for (int s0 = 0; s0 <= a.n_seg; s0 += CH) {
    const int s = s0 + tid;
    int c = 0;
    if (s < a.n_seg) {
      const int len = a.seg_row0[s + 1] - a.seg_row0[s];
      c = len > 0 ? (len + CH - 1) / CH : 0;
    }
    int ex;
    const int inc = block_scan<OpAdd, false>(c, slot, ex);
    if (s <= a.n_seg) chunk0[s] = carry + ex;
    if (tid == CH - 1) bc = carry + inc;
    __syncthreads();
    carry = bc;
    __syncthreads();
  }
}

// rows and chunks of segment s as the device tables give them; false when they do not lie inside the rolls and the workspace (a device table
// that differs from the host's checked one): the workgroup then does nothing
__device__ inline bool seg_of(const seg_args& a, int s, long* row0, int* F, int* c0, int* nch) {
  const int* chunk0 = (const int*)a.d.ws;
  const long r0 = a.seg_row0[s], r1 = a.seg_row0[s + 1];
  *row0 = r0; *F = (int)(r1 - r0); *c0 = chunk0[s]; *nch = chunk0[s + 1] - chunk0[s];
  return r0 >= 0 && r1 > r0 && r1 <= (long)a.d.F && *c0 >= 0 && *nch == (*F + CH - 1) / CH && *c0 + *nch <= a.chunks;
}

// one workgroup per (pitch, segment): blockIdx.x = s * N + j
__global__ __launch_bounds__(CH) void notes_seg_scan_kernel(const seg_args a) {
  __shared__ int slots[16][4];
  __shared__ int bc[8];
  const int N = a.d.N, s = blockIdx.x / N, j = blockIdx.x % N;
  long row0; int F, c0, nch;
  if (!seg_of(a, s, &row0, &F, &c0, &nch)) return;
  const long e = (long)N * c0 + (long)j * nch;
  int* st = (int*)a.d.ws + a.tbl + e * ST_INTS;
  int* cnt = (int*)a.d.ws + a.tbl + (long)N * a.chunks * ST_INTS + e;
  notes_scan_body(a.d, track_of(a.d, row0, F, j), nch, st, cnt, slots, bc);
}

// seg_notes[s] = the prefix at segment s's first count (an empty segment shares the next one's), the total behind the last
__global__ __launch_bounds__(CH) void notes_seg_heads_kernel(const seg_args a) {
  const int s = blockIdx.x * CH + threadIdx.x;
  if (s > a.n_seg) return;
  const int* chunk0 = (const int*)a.d.ws;
  const int* cnt = (const int*)a.d.ws + a.tbl + (long)a.d.N * a.chunks * ST_INTS;
  const int c = chunk0[s];
  a.seg_notes[s] = c >= 0 && c < a.chunks ? cnt[(long)a.d.N * c] : *(const int*)a.d.n_notes;
}

// one workgroup per (chunk of any segment, pitch): the segment is the last one whose first chunk is not behind blockIdx.x
__global__ __launch_bounds__(CH) void notes_seg_emit_kernel(const seg_args a, float h2) {
  __shared__ int slots[16][4];
  const int c = blockIdx.x, j = blockIdx.y, N = a.d.N;
  const int* chunk0 = (const int*)a.d.ws;
  int lo = 0, hi = a.n_seg;                            // first s in [0, n_seg] with chunk0[s + 1] > c; n_seg: none
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (chunk0[mid + 1] > c) hi = mid; else lo = mid + 1;
  }
  if (lo >= a.n_seg) return;
  long row0; int F, c0, nch;
  if (!seg_of(a, lo, &row0, &F, &c0, &nch) || c < c0) return;
  const int k = c - c0;
  const long e = (long)N * c0 + (long)j * nch + k;
  const int* st = (const int*)a.d.ws + a.tbl + e * ST_INTS;
  const int base = ((const int*)a.d.ws)[a.tbl + (long)N * a.chunks * ST_INTS + e];
  notes_emit_body(a.d, track_of(a.d, row0, F, j), j, k, st, base, h2, slots);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// clip windows: a tile of TILE frames x TILE bins through LDS, read along the bins, written along the frames
// ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int TILE = 64;

__global__ __launch_bounds__(256) void clip_windows_kernel(const hftt_clip_windows_desc d, int tiles_t, int tiles_k) {
  __shared__ float tile[TILE][TILE + 1];              // + 1 word: the column read below meets 64 different banks
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long blk = blockIdx.x;
  const int tt = (int)(blk % tiles_t);
  const int tk = (int)((blk / tiles_t) % tiles_k);
  const int b = (int)(blk / ((long)tiles_t * tiles_k));
  const int t0 = tt * TILE, k0 = tk * TILE;
  const int f = d.win_file[b];
  const long s = d.win_start[b];
  long r0 = 0, nf = 0;
  if (f >= 0 && f < d.n_files) {
    r0 = d.file_row0[f];
    nf = (long)d.file_row0[f + 1] - r0;
    if (r0 < 0 || nf < 0 || r0 + nf > d.R) nf = 0;    // rows outside the feature array: nothing of this file is read
  }
  const float* feat = (const float*)d.feature;
  for (int i = w; i < TILE; i += 4) {                  // a wave reads 64 bins of one frame: 256 contiguous bytes
    const long fr = s + t0 + i;
    const int k = k0 + lane;
    float v = d.fill;
    if (t0 + i < d.width && k < d.n_bins && fr >= 0 && fr < nf) v = feat[(r0 + fr) * d.n_bins + k];
    tile[i][lane] = v;
  }
  __syncthreads();
  float* out = (float*)d.out;
  for (int i = w; i < TILE; i += 4) {                  // a wave writes 64 frames of one bin: 256 contiguous bytes
    const int k = k0 + i, t = t0 + lane;
    if (k < d.n_bins && t < d.width) out[((long)b * d.n_bins + k) * d.width + t] = tile[lane][i];
  }
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

// the rejections that the one-file and the segmented decode share (everything but the workspace size); 0 = accepted
static int notes_check(const hftt_notes_desc* d, const char* what) {
  HFTT_REQUIRE(d->F >= 0, "%s: F=%ld is negative", what, (long)d->F);
  HFTT_REQUIRE(d->N >= 1 && d->N <= 128, "%s: N=%d outside 1..128", what, d->N);
  HFTT_REQUIRE((long)d->F * d->N < (1l << 31), "%s: F=%ld frames of N=%d exceed 2^31 elements (the note count is an int32)", what, (long)d->F, d->N);
  HFTT_REQUIRE(d->cap >= 0, "%s: cap=%d is negative", what, d->cap);
  HFTT_REQUIRE(d->mode_velocity == 0 || d->mode_velocity == 1, "%s: mode_velocity=%d (0 = ignore_zero, 1 = org)", what, d->mode_velocity);
  HFTT_REQUIRE(d->mode_offset >= 0 && d->mode_offset <= 2, "%s: mode_offset=%d (0 = shorter, 1 = longer, 2 = offset)", what, d->mode_offset);
  HFTT_REQUIRE(d->n_notes, "%s: n_notes is null", what);
  HFTT_REQUIRE(d->cap == 0 || (d->out_pitch && d->out_velocity && d->out_onset && d->out_offset),
               "%s: null output (out_pitch / out_velocity / out_onset / out_offset) at cap=%d", what, d->cap);
  HFTT_REQUIRE(d->F == 0 || (d->onset && d->offset && d->mpe && d->velocity), "%s: null roll (onset / offset / mpe / velocity)", what);
  HFTT_REQUIRE(d->ws, "%s: ws is null", what);
  return 0;
}

static int notes_clear(const char* what, void* p, size_t bytes, hipStream_t st) {
  hipError_t e = hipMemsetAsync(p, 0, bytes, st);
  if (e != hipSuccess) { hftt_set_error("%s: clearing the counts failed: %s", what, hipGetErrorString(e)); return 2; }
  return 0;
}

extern "C" int hftt_notes_decode(const hftt_notes_desc* d, void* stream) {
  HFTT_REQUIRE(d, "notes_decode: null descriptor");
  if (int rc = notes_check(d, "notes_decode")) return rc;
  HFTT_REQUIRE(d->ws_bytes >= hftt_notes_ws_bytes(d->F, d->N), "notes_decode: ws_bytes=%ld below hftt_notes_ws_bytes(F, N)=%ld", (long)d->ws_bytes,
               (long)hftt_notes_ws_bytes(d->F, d->N));
  const int nchunks = (int)notes_chunks(d->F);
  int* cnt = (int*)d->ws + (long)d->N * nchunks * ST_INTS;
  if (d->F == 0) {                                      // no frame, no note, no launch: the total alone is written
    if (hftt_device_guard("notes_decode") != 0) return 3;
    return notes_clear("notes_decode", d->n_notes, sizeof(int), (hipStream_t)stream);
  }
  if (int rc = hftt_launch<notes_scan_kernel>("notes_decode", dim3((unsigned)d->N), dim3(CH), 0, (hipStream_t)stream, *d, nchunks)) return rc;
  if (int rc = hftt_launch<notes_offsets_kernel>("notes_decode", dim3(1), dim3(CH), 0, (hipStream_t)stream, cnt, d->N * nchunks, (int*)d->n_notes)) return rc;
  return hftt_launch<notes_emit_kernel>("notes_decode", dim3((unsigned)nchunks, (unsigned)d->N), dim3(CH), 0, (hipStream_t)stream, *d, nchunks,
                                        (float)(d->hop_sec * 0.5));
}

inline long seg_table_ints(long n_seg) { return (n_seg + 1 + 15) / 16 * 16; }

// every segment ends with at most one partial chunk: at most ceil(F / CH) + n_seg chunks whatever the borders are
extern "C" int64_t hftt_notes_seg_ws_bytes(int64_t F, int32_t N, int32_t n_seg) {
  if (F < 0 || N < 1 || N > 128 || n_seg < 0) return 0;
  return 64 + 4 * seg_table_ints(n_seg) + 4 * (int64_t)(ST_INTS + 1) * N * (notes_chunks(F) + n_seg);
}

extern "C" int hftt_notes_decode_seg(const hftt_notes_seg_desc* s, void* stream) {
  const char* what = "notes_decode_seg";
  HFTT_REQUIRE(s, "notes_decode_seg: null descriptor");
  const hftt_notes_desc* d = &s->notes;
  if (int rc = notes_check(d, what)) return rc;
  HFTT_REQUIRE(s->n_seg >= 0, "notes_decode_seg: n_seg=%d is negative", s->n_seg);
  HFTT_REQUIRE(s->seg_notes, "notes_decode_seg: seg_notes is null");
  HFTT_REQUIRE(s->n_seg == 0 || (s->seg_row0_host && s->seg_row0), "notes_decode_seg: null table (seg_row0_host / seg_row0) at n_seg=%d", s->n_seg);
  HFTT_REQUIRE((long)s->n_seg * d->N < (1l << 31), "notes_decode_seg: n_seg=%d segments of N=%d exceed 2^31 workgroups", s->n_seg, d->N);
  long chunks = 0;
  if (s->n_seg == 0) {
    HFTT_REQUIRE(d->F == 0, "notes_decode_seg: seg_row0_host: n_seg=0 covers no row, F=%ld", (long)d->F);
  } else {
    const int32_t* t = s->seg_row0_host;
    HFTT_REQUIRE(t[0] == 0, "notes_decode_seg: seg_row0_host[0]=%d must be 0", t[0]);
    for (int i = 0; i < s->n_seg; i++) {
      HFTT_REQUIRE(t[i + 1] >= t[i], "notes_decode_seg: seg_row0_host[%d]=%d below seg_row0_host[%d]=%d (non-decreasing)", i + 1, t[i + 1], i, t[i]);
      chunks += notes_chunks((long)t[i + 1] - t[i]);
    }
    HFTT_REQUIRE(t[s->n_seg] == d->F, "notes_decode_seg: seg_row0_host[n_seg=%d]=%d must be F=%ld", s->n_seg, t[s->n_seg], (long)d->F);
  }
  const int64_t need = hftt_notes_seg_ws_bytes(d->F, d->N, s->n_seg);
  HFTT_REQUIRE(d->ws_bytes >= need, "notes_decode_seg: ws_bytes=%ld below hftt_notes_seg_ws_bytes(F, N, n_seg)=%ld", (long)d->ws_bytes, (long)need);
  hipStream_t st = (hipStream_t)stream;
  if (chunks == 0) {                                    // no frame, no note, no launch: the counts alone are written
    if (hftt_device_guard(what) != 0) return 3;
    if (int rc = notes_clear(what, d->n_notes, sizeof(int), st)) return rc;
    return notes_clear(what, s->seg_notes, sizeof(int) * ((size_t)s->n_seg + 1), st);
  }
  seg_args a;
  a.d = *d;
  a.seg_row0 = (const int*)s->seg_row0;
  a.seg_notes = (int*)s->seg_notes;
  a.n_seg = s->n_seg;
  a.tbl = (int)seg_table_ints(s->n_seg);
  a.chunks = (int)chunks;
  int* cnt = (int*)d->ws + a.tbl + (long)d->N * chunks * ST_INTS;
  // a segment that the device table describes otherwise is skipped by the kernels: its counts must not be read uninitialised
  if (hftt_device_guard(what) != 0) return 3;
  if (int rc = notes_clear(what, cnt, sizeof(int) * (size_t)d->N * chunks, st)) return rc;
  if (int rc = hftt_launch<notes_seg_table_kernel>(what, dim3(1), dim3(CH), 0, st, a)) return rc;
  if (int rc = hftt_launch<notes_seg_scan_kernel>(what, dim3((unsigned)((long)s->n_seg * d->N)), dim3(CH), 0, st, a)) return rc;
  if (int rc = hftt_launch<notes_offsets_kernel>(what, dim3(1), dim3(CH), 0, st, cnt, (int)(d->N * chunks), (int*)d->n_notes)) return rc;
  if (int rc = hftt_launch<notes_seg_heads_kernel>(what, dim3((unsigned)((s->n_seg + 1 + CH - 1) / CH)), dim3(CH), 0, st, a)) return rc;
  return hftt_launch<notes_seg_emit_kernel>(what, dim3((unsigned)chunks, (unsigned)d->N), dim3(CH), 0, st, a, (float)(d->hop_sec * 0.5));
}

extern "C" int hftt_clip_windows(const hftt_clip_windows_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_windows: null descriptor");
  HFTT_REQUIRE(d->feature && d->file_row0 && d->win_file && d->win_start && d->out,
               "clip_windows: null pointer (feature / file_row0 / win_file / win_start / out)");
  HFTT_REQUIRE(d->B >= 1, "clip_windows: B=%d must be positive", d->B);
  HFTT_REQUIRE(d->width >= 1, "clip_windows: width=%d must be positive", d->width);
  HFTT_REQUIRE(d->n_bins >= 1, "clip_windows: n_bins=%d must be positive", d->n_bins);
  HFTT_REQUIRE(d->n_files >= 0, "clip_windows: n_files=%d is negative", d->n_files);
  HFTT_REQUIRE(d->R >= 0, "clip_windows: R=%ld is negative", (long)d->R);
  HFTT_REQUIRE((long)d->B * d->n_bins < (1l << 31) && (long)d->B * d->n_bins * d->width < (1l << 31), "clip_windows: B=%d windows of n_bins=%d x width=%d exceed 2^31 elements", d->B, d->n_bins, d->width);
  const int tiles_t = (d->width + TILE - 1) / TILE, tiles_k = (d->n_bins + TILE - 1) / TILE;
  const long blocks = (long)d->B * tiles_t * tiles_k;  // <= B * width * n_bins < 2^31
  return hftt_launch<clip_windows_kernel>("clip_windows", dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *d, tiles_t, tiles_k);
}
