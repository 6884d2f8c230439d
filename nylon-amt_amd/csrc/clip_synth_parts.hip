// Clip synth, played (gfx950): the windows of a training batch rendered from the note table under a per-window PERFORMANCE -- transposition,
// time map, tuning -- and with a second part under its own voice summed onto the first, one launch.
//   hftt_clip_synth_parts  hftt_clip_synth's inputs + per-window (shift, t_delay, t_scale, tune_q31) for each part + a partner (file, start,
//                          voice, gain) -> the same scratch corpus and tables
// This is a deliberate SECOND copy of clip_synth.hip's walk: that file compiles to exactly one kernel whose name, resources and text
// tests/test_synth_capi.py pins, so it stays byte for byte and a template over it is ruled out.  What keeps the two from drifting is
// tests/test_synth_parts_gpu.py: under an identity performance (all groups NULL, and identity values) this kernel's four outputs are
// torch.equal to clip_synth_kernel's.  Both share clip_synth_fn.h (S and E) and block_scan.h.
// Shape: clip_synth_kernel's -- a workgroup per window and tile of TILE samples, TPB threads, SPT samples per thread in registers.  One device
// function, synth_part, filters one part's records against the tile (in that part's coordinates, cut to the part's own extent) into LDS in table
// order and walks the survivors; it is called for the primary and then, under a branch that is uniform over the workgroup, for the partner with
// the SAME accumulators, the same survivor list and the partner file's row pointers re-staged.  Per-window values and bank entries are uniform
// (readfirstlane): the tuning product inc * tune_q31 >> 31 is scalar arithmetic next to the bank load.  No global store stands in front of the
// uniform loads (tables() runs behind the walk).  One writer per element, no atomics.  See include/hftt_hip.h for the contract.
#include "hftt_common.h"
#include "hftt_host.h"
#include "hftt_launch.h"
#include "block_scan.h"
#include "clip_synth_fn.h"
#include "../../include/hftt_hip.h"

// Every product and sum below is rounded on its own (the contract counts the roundings; the time map is fp64 with two roundings, never an
// fma); the one fma is spelled out.
#pragma clang fp contract(off)

namespace {

constexpr int CH = HFTT_SYNTH_CHUNK;                 // records per filter pass = threads per workgroup
constexpr int TPB = CH;
constexpr int GROUPS = 2;                            // quads of samples per thread
constexpr int SPT = 4 * GROUPS;                      // samples per thread
constexpr int TILE = TPB * SPT;                      // samples per workgroup
static_assert(CH == 256 && TILE == 2048, "block_scan (block_scan.h) is written for four waves; the header states the tile");

// frames in front of a window that its row holds: ceil((n_fft / 2) / hop) + lead
__host__ __device__ inline long parts_front(int n_fft, int hop, int lead) { return (n_fft / 2 + hop - 1) / hop + (long)lead; }

// The survivors of one filter pass, in table order.  Every thread reads the same entry at the same time: LDS broadcasts.
struct survivors {
  long on[CH], dur[CH];                              // n_on, D under the part's time map
  int row[CH];                                       // the bank row: pitch + shift, inside 0 .. N - 1
  float vg[CH];                                      // vel_gain[v, velocity]
};

// a value that every lane holds alike, moved to the scalar registers: what is indexed with it is loaded on the scalar unit
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ float uni(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ long uni(long x) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(x >> 32));
  return (long)(((unsigned long)hi << 32) | lo);
}
__device__ __forceinline__ double uni(double x) { return __longlong_as_double(uni((long)__double_as_longlong(x))); }

// how window b plays one part: the identity where a group is absent (t + 0) * 1 and inc * 2^31 >> 31 leave the bits they are given
struct play_of {
  int shift;
  double t_delay, t_scale;
  unsigned tune;
};
__device__ __forceinline__ play_of play_at(const hftt_synth_play_args& a, int b) {
  play_of p = {0, 0.0, 1.0, 1u << 31};
  if (a.shift) {
    p.shift = uni(a.shift[b]);
    p.t_delay = uni(a.t_delay[b]);
    p.t_scale = uni(a.t_scale[b]);
  }
  if (a.tune_q31) p.tune = (unsigned)uni((int)a.tune_q31[b]);
  return p;
}

// One part onto the accumulators: the records of `file` under voice v and play pl whose sounding range meets the tile -- samples [lo, hi) in
// THIS part's coordinates -- cut to the part's own extent [0, n_part), in table order.  Every thread of the workgroup calls it with the same
// arguments (they are uniform), so the barriers are met by all or by none.  scaled: the coefficient carries `gain` (the partner's one further
// rounding, formed once per record and partial).
__device__ __forceinline__ void synth_part(const hftt_clip_synth_desc& g, const play_of& pl, int file, int v, long n_part, long lo, long hi, bool scaled, float gain,
                                           survivors& s, int* rp, int* slot, int& total, int tid, float (&acc)[SPT]) {
  const int N = g.N, H = g.H;
  const long flo = lo > 0 ? lo : 0, fhi = hi < n_part ? hi : n_part;           // what of the tile lies inside the part
  if (fhi <= flo) return;
  __syncthreads();                                    // whoever still reads the row pointers of the part in front has done so
  for (int k = tid; k <= N; k += TPB) {
    const int r = g.row_ptr[(long)file * N + k];
    rp[k] = r < 0 ? 0 : r > g.n_notes ? g.n_notes : r;
  }
  __syncthreads();
  int attack = g.attack[v], release = g.release[v];
  attack = attack < 1 ? 1 : attack;
  release = release < 0 ? 0 : release;
  const float attf = (float)attack, rel = g.rel[v];
  const float* __restrict__ vgain = g.vel_gain + (long)v * 128;
  const int row0 = v * N;                             // (V N H < 2^31, the launcher saw to it: 32-bit products stay on the scalar unit)
  const long beg = uni(rp[0]), end = uni(rp[N]);
  for (long c0 = beg; c0 < end; c0 += CH) {
    // filter: record c0 + tid survives when its sounding range meets [flo, fhi) and its bank row exists
    bool keep = false;
    long on = 0, dur = 0;
    int p = 0;
    float vg = 0.f;
    const long c = c0 + tid;
    if (c < end) {
      const hftt_label_note n = g.notes[c];
      const double on_sec = (n.onset_sec + pl.t_delay) * pl.t_scale;            // the expression of hftt_labels_render_warp: two roundings
      const double off_sec = (n.offset_sec + pl.t_delay) * pl.t_scale;
      on = (long)(on_sec * g.sr + 0.5);
      dur = (long)(off_sec * g.sr + 0.5) - on;
      dur = dur < 1 ? 1 : dur;
      keep = on < fhi && on + dur + release > flo;
      if (keep) {
        int a = 0, z = N;                             // the smallest p with rp[p + 1] > c
        while (a < z) {
          const int mid = (a + z) >> 1;
          if (rp[mid + 1] <= c) a = mid + 1; else z = mid;
        }
        p = (a < N ? a : N - 1) + pl.shift;           // the row that sounds; outside the bank: no operation
        keep = p >= 0 && p < N;
        const int vel = n.velocity < 0 ? 0 : n.velocity > 127 ? 127 : n.velocity;
        vg = vgain[vel];
      }
    }
    int at;
    const int inc = block_scan<OpAdd, false>(keep ? 1 : 0, slot, at);
    if (keep) {
      s.on[at] = on; s.dur[at] = dur; s.row[at] = p; s.vg[at] = vg;
    }
    if (tid == CH - 1) total = inc;
    __syncthreads();
    const int n = uni(total);
    for (int k = 0; k < n; k++) {
      const long dur_k = uni(s.dur[k]), on_k = uni(s.on[k]);
      const long tau0 = lo - on_k, sound = dur_k + release;
      // tau inside [t_lo, t_lo + t_n): the record sounds AND the sample lies inside the part
      const long t_lo = on_k < 0 ? -on_k : 0, t_hi = sound < n_part - on_k ? sound : n_part - on_k;
      const unsigned long t_n = t_hi > t_lo ? (unsigned long)(t_hi - t_lo) : 0ul;
      const float vg_k = uni(s.vg[k]);
      const int bank = (row0 + uni(s.row[k])) * H;
      // what depends on the sample alone
      float tf[SPT], t2[SPT], ra[SPT];
      unsigned ph[SPT];
      bool live[SPT], any = false;
#pragma unroll
      for (int j = 0; j < SPT; j++) {
        const long tau = tau0 + 4 * (tid + (j >> 2) * TPB) + (j & 3);
        live[j] = (unsigned long)(tau - t_lo) < t_n;
        any = any || live[j];
        tf[j] = (float)tau;
        t2[j] = rel * (float)(tau > dur_k ? tau - dur_k : 0);
        ra[j] = (float)(tau + 1 < attack ? tau + 1 : (long)attack) / attf;
        ph[j] = (unsigned)tau;
      }
      if (__builtin_amdgcn_ballot_w64(any) == 0) continue;                      // no sample of this wave hears the record (no barrier below)
      for (int h = 0; h < H; h++) {
        const unsigned dphi = (unsigned)(((unsigned long)g.inc[bank + h] * pl.tune) >> 31);
        float g0 = g.amp[bank + h] * vg_k;
        g0 = scaled ? g0 * gain : g0;
        const float dc = g.dec[bank + h];
#pragma unroll
        for (int j = 0; j < SPT; j++) {
          const float u = (float)(int)(dphi * ph[j]) * 0x1p-32f;
          const float x = fminf(dc * tf[j] + t2[j], 126.f);
          const float cj = (g0 * ra[j]) * synth_exp2(-x);
          const float a = __builtin_fmaf(cj, synth_sin_turns(u), acc[j]);
          acc[j] = live[j] ? a : acc[j];
        }
      }
    }
    __syncthreads();                                  // the next pass writes the list and `total` again
  }
}

__global__ __launch_bounds__(TPB) void clip_synth_parts_kernel(const hftt_clip_synth_parts_desc d, int ntiles) {
  __shared__ survivors s;
  __shared__ int rp[128 + 1];                         // the part's row pointers: records rp[p] .. rp[p + 1] have pitch p
  __shared__ int slot[4];
  __shared__ int total;
  const hftt_clip_synth_desc& g = d.base;
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)ntiles);
  const int tile = (int)(blockIdx.x % (unsigned)ntiles);
  const int hop = g.hop;
  const int file = g.win_file[b];
  const int v = g.voice_index[b];
  const long ws = g.win_start[b];
  const long front = parts_front(g.n_fft, hop, g.lead);
  const bool known = file >= 0 && file < g.n_files;
  long np = known ? d.nsamp[b] : 0;                   // samples of the window's synthetic file under its map
  np = np < 0 ? 0 : np;
  const long ob = (ws > front ? ws - front : 0) * hop;                         // first sample of the pseudo-file
  long eb = (ws + g.width - 1) * hop + g.n_fft / 2;                            // (the span the launcher accepted bounds it: no overflow)
  eb = eb < np ? eb : np;
  const bool valid = known && v >= 0 && v < g.V && ob <= np;
  const long len = valid && eb > ob ? eb - ob : 0;                             // samples of the pseudo-file, <= span
  // the window's table entries, by one thread -- behind the walk, not in front of it: no store to global memory stands in front of the loads
  // at uniform addresses (the window's entries, the bank), so they stay on the scalar unit
  const auto tables = [&]() {
    if (tile != 0 || tid != 0) return;
    g.out_samp0[2 * b] = (long)b * g.span;
    g.out_samp0[2 * b + 1] = (long)b * g.span + len;
    if (b == g.B - 1) g.out_samp0[2 * g.B] = (long)g.B * g.span;
    g.out_win_file[b] = valid ? 2 * b : -1;
    g.out_win_start[b] = (int)(ws - ob / hop);        // win_start[b] itself, or `front`
  };
  const long t0 = (long)tile * TILE;                  // of the pseudo-file
  if (t0 >= len) {                                    // (uniform) nothing of this tile is shown; behind here the window is valid
    tables();
    return;
  }
  const long left = len - t0;                         // samples of this tile that exist (may exceed TILE)
  const long lo = ob + t0, hi = lo + (left < TILE ? left : TILE);              // the tile is primary samples [lo, hi)
  float acc[SPT] = {};
  synth_part(g, play_at(d.play, b), uni(file), uni(v), np, lo, hi, false, 1.f, s, rp, slot, total, tid, acc);
  if (d.part_file) {                                  // (uniform) the partner, carried by the same accumulators
    const int pfile = uni(d.part_file[b]), pv = uni(d.part_voice[b]);
    if (pfile >= 0 && pfile < g.n_files && pv >= 0 && pv < g.V) {
      long nb = d.part_nsamp[b];
      nb = nb < 0 ? 0 : nb;
      const long delta = ((long)d.part_start[b] - ws) * hop;                   // partner position of primary sample 0
      synth_part(g, play_at(d.part_play, b), pfile, pv, uni(nb), lo + delta, hi + delta, true, uni(d.part_gain[b]), s, rp, slot, total, tid, acc);
    }
  }
  float* out = (float*)g.out + (long)b * g.span + t0;
#pragma unroll
  for (int q = 0; q < GROUPS; q++) {
    const int x = 4 * (tid + q * TPB);
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (x + e < left) out[x + e] = acc[4 * q + e];
  }
  tables();
}

bool whole(const hftt_synth_play_args& a) { return (a.shift && a.t_delay && a.t_scale) || (!a.shift && !a.t_delay && !a.t_scale); }
bool given(const hftt_synth_play_args& a) { return a.shift || a.t_delay || a.t_scale || a.tune_q31; }

}  // namespace

extern "C" int hftt_clip_synth_parts(const hftt_clip_synth_parts_desc* p, void* stream) {
  HFTT_REQUIRE(p, "clip_synth_parts: null descriptor");
  const hftt_clip_synth_desc* d = &p->base;
  HFTT_REQUIRE(d->n_notes >= 0, "clip_synth_parts: n_notes=%d is negative", d->n_notes);
  HFTT_REQUIRE(d->notes || d->n_notes == 0, "clip_synth_parts: notes is null at n_notes=%d", d->n_notes);
  HFTT_REQUIRE(d->row_ptr, "clip_synth_parts: row_ptr is null");
  HFTT_REQUIRE(p->nsamp, "clip_synth_parts: nsamp is null");
  HFTT_REQUIRE(d->win_file && d->win_start, "clip_synth_parts: null window table (win_file / win_start)");
  HFTT_REQUIRE(d->inc && d->amp && d->dec && d->vel_gain && d->rel && d->attack && d->release, "clip_synth_parts: null voice bank (inc / amp / dec / vel_gain / rel / attack / release)");
  HFTT_REQUIRE(d->voice_index, "clip_synth_parts: voice_index is null");
  HFTT_REQUIRE(d->out && d->out_samp0 && d->out_win_file && d->out_win_start, "clip_synth_parts: null output (out / out_samp0 / out_win_file / out_win_start)");
  HFTT_REQUIRE(whole(p->play), "clip_synth_parts: null play table (shift / t_delay / t_scale: all or none)");
  HFTT_REQUIRE(whole(p->part_play), "clip_synth_parts: null partner play table (part_play shift / t_delay / t_scale: all or none)");
  const bool any_part = p->part_file || p->part_start || p->part_voice || p->part_gain;
  const bool all_part = p->part_file && p->part_start && p->part_voice && p->part_gain;
  HFTT_REQUIRE(!any_part || all_part, "clip_synth_parts: null partner table (part_file / part_start / part_voice / part_gain: all or none)");
  HFTT_REQUIRE(all_part || !p->part_nsamp, "clip_synth_parts: part_nsamp given without partner tables");
  HFTT_REQUIRE(all_part || !given(p->part_play), "clip_synth_parts: part_play given without partner tables");
  HFTT_REQUIRE(!all_part || p->part_nsamp, "clip_synth_parts: part_nsamp is null with partner tables");
  HFTT_REQUIRE(d->n_fft == 2048, "clip_synth_parts: n_fft=%d unsupported (2048 only)", d->n_fft);
  HFTT_REQUIRE(d->B >= 1 && d->B < (1 << 30), "clip_synth_parts: B=%d outside 1 .. 2^30 (2 B pseudo-files)", d->B);
  HFTT_REQUIRE(d->width >= 1, "clip_synth_parts: width=%d must be positive", d->width);
  HFTT_REQUIRE(d->hop >= 1, "clip_synth_parts: hop=%d must be positive", d->hop);
  HFTT_REQUIRE(d->n_files >= 1, "clip_synth_parts: n_files=%d must be positive", d->n_files);
  HFTT_REQUIRE(d->N >= 1 && d->N <= 128, "clip_synth_parts: N=%d outside 1..128", d->N);
  HFTT_REQUIRE(d->V >= 1, "clip_synth_parts: V=%d must be positive", d->V);
  HFTT_REQUIRE(d->H >= 1 && d->H <= HFTT_SYNTH_MAX_PARTIALS, "clip_synth_parts: H=%d outside 1..%d partials", d->H, HFTT_SYNTH_MAX_PARTIALS);
  HFTT_REQUIRE((long)d->V * d->N * d->H < (1l << 31), "clip_synth_parts: a bank of V=%d voices, N=%d pitches and H=%d partials exceeds 2^31 entries", d->V, d->N, d->H);
  HFTT_REQUIRE(d->lead >= 0, "clip_synth_parts: lead=%d is negative", d->lead);
  HFTT_REQUIRE(d->sr > 0.0 && d->sr <= 1e12, "clip_synth_parts: sr=%g must be positive (and finite)", d->sr);
  const __int128 need = ((__int128)parts_front(d->n_fft, d->hop, d->lead) + d->width - 1) * d->hop + d->n_fft / 2;
  HFTT_REQUIRE(d->span >= need, "clip_synth_parts: span=%ld below the %ld samples a window of width=%d and lead=%d at hop=%d can show", (long)d->span, (long)need, d->width,
               d->lead, d->hop);
  const long ntiles = ((long)need + TILE - 1) / TILE;
  HFTT_REQUIRE((__int128)d->B * ntiles < (1l << 31), "clip_synth_parts: B=%d windows of width=%d and lead=%d exceed 2^31 workgroups", d->B, d->width, d->lead);
  const dim3 grid((unsigned)((long)d->B * ntiles));
  return hftt_launch<clip_synth_parts_kernel>("clip_synth_parts", grid, dim3(TPB), 0, (hipStream_t)stream, *p, (int)ntiles);
}
