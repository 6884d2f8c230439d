// Clip synth (gfx950): the windows of a training batch rendered from the corpus-wide note table under one voice of a resident bank each, one launch.
//   hftt_clip_synth  B windows of the note table of hftt_labels_render + a voice bank (V voices of H decaying partials per pitch)
//                    -> samples fp32 [B, span] and the tables under which a plain hftt_clip_logmel reads them as files (hftt_clip_room's convention)
// A workgroup owns one window and a tile of TILE consecutive samples.  It scans the file's records -- contiguous in the table: pitch group after
// pitch group -- CH at a time, keeps those whose sounding range [n_on, n_on + D + release) meets the tile in LDS in TABLE order (block_scan.h;
// the pitch of a record is found in the file's N + 1 row pointers, staged in LDS), and then only evaluates: a thread owns GROUPS quads of four
// consecutive samples and walks the survivors; per survivor it forms what depends on the sample alone (tau, the attack ramp, the release term)
// once and then takes the partials h = 0 .. H - 1, whose bank entries are uniform over the workgroup (the survivor's fields go through
// readfirstlane, so the bank is read on the scalar unit).  acc = fma(c, S(u), acc) in that order for every sample, wherever its tile begins:
// S and E (clip_synth_fn.h) are evaluated per sample from the exact wrapped phase, there is no recurrence.  More sounding records than CH are
// further passes.  One writer per element, no atomics.  See include/hftt_hip.h for the contract.
#include "hftt_common.h"
#include "hftt_host.h"
#include "hftt_launch.h"
#include "block_scan.h"
#include "clip_synth_fn.h"
#include "../../include/hftt_hip.h"

// Every product and sum below is rounded on its own (the contract counts the roundings); the one fma is spelled out.
#pragma clang fp contract(off)

namespace {

constexpr int CH = HFTT_SYNTH_CHUNK;                 // records per filter pass = threads per workgroup
constexpr int TPB = CH;
constexpr int GROUPS = 2;                            // quads of samples per thread
constexpr int SPT = 4 * GROUPS;                      // samples per thread
constexpr int TILE = TPB * SPT;                      // samples per workgroup
static_assert(CH == 256 && TILE == 2048, "block_scan (block_scan.h) is written for four waves; the header states the tile");

// frames in front of a window that its row holds: ceil((n_fft / 2) / hop) + lead
__host__ __device__ inline long synth_front(int n_fft, int hop, int lead) { return (n_fft / 2 + hop - 1) / hop + (long)lead; }

// The survivors of one filter pass, in table order.  Every thread reads the same entry at the same time: LDS broadcasts.
struct survivors {
  long on[CH], dur[CH];                              // n_on, D
  int pitch[CH];
  float vg[CH];                                      // vel_gain[v, velocity]
};

// a value that every lane holds alike, moved to the scalar registers: what is indexed with it is loaded on the scalar unit
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ float uni(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ long uni(long x) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(x >> 32));
  return (long)(((unsigned long)hi << 32) | lo);
}

__global__ __launch_bounds__(TPB) void clip_synth_kernel(const hftt_clip_synth_desc g, int ntiles) {
  __shared__ survivors s;
  __shared__ int rp[128 + 1];                         // the file's row pointers: records rp[p] .. rp[p + 1] have pitch p
  __shared__ int slot[4];
  __shared__ int total;
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)ntiles);
  const int tile = (int)(blockIdx.x % (unsigned)ntiles);
  const int hop = g.hop, N = g.N, H = g.H;
  const int file = g.win_file[b];
  const int v = g.voice_index[b];
  const long ws = g.win_start[b];
  const long front = synth_front(g.n_fft, hop, g.lead);
  const bool known = file >= 0 && file < g.n_files;
  long np = known ? g.file_nsamp[file] : 0;           // samples of the synthetic file
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
  for (int k = tid; k <= N; k += TPB) {
    const int r = g.row_ptr[(long)file * N + k];
    rp[k] = r < 0 ? 0 : r > g.n_notes ? g.n_notes : r;
  }
  __syncthreads();
  const long left = len - t0;                         // samples of this tile that exist (may exceed TILE)
  const long lo = ob + t0, hi = lo + (left < TILE ? left : TILE);              // the tile is file samples [lo, hi)
  int attack = g.attack[v], release = g.release[v];
  attack = attack < 1 ? 1 : attack;
  release = release < 0 ? 0 : release;
  const float attf = (float)attack, rel = g.rel[v];
  const float* __restrict__ vgain = g.vel_gain + (long)v * 128;
  const int row0 = v * N;                             // (V N H < 2^31, the launcher saw to it: 32-bit products stay on the scalar unit)
  float acc[SPT] = {};
  const long beg = uni(rp[0]), end = uni(rp[N]);
  for (long c0 = beg; c0 < end; c0 += CH) {
    // filter: record c0 + tid survives when its sounding range meets [lo, hi)
    bool keep = false;
    long on = 0, dur = 0;
    int p = 0;
    float vg = 0.f;
    const long c = c0 + tid;
    if (c < end) {
      const hftt_label_note n = g.notes[c];
      on = (long)(n.onset_sec * g.sr + 0.5);
      dur = (long)(n.offset_sec * g.sr + 0.5) - on;
      dur = dur < 1 ? 1 : dur;
      keep = on < hi && on + dur + release > lo;
      if (keep) {
        int a = 0, z = N;                             // the smallest p with rp[p + 1] > c
        while (a < z) {
          const int mid = (a + z) >> 1;
          if (rp[mid + 1] <= c) a = mid + 1; else z = mid;
        }
        p = a < N ? a : N - 1;
        const int vel = n.velocity < 0 ? 0 : n.velocity > 127 ? 127 : n.velocity;
        vg = vgain[vel];
      }
    }
    int at;
    const int inc = block_scan<OpAdd, false>(keep ? 1 : 0, slot, at);
    if (keep) {
      s.on[at] = on; s.dur[at] = dur; s.pitch[at] = p; s.vg[at] = vg;
    }
    if (tid == CH - 1) total = inc;
    __syncthreads();
    const int n = uni(total);
    for (int k = 0; k < n; k++) {
      const long dur_k = uni(s.dur[k]);
      const long tau0 = lo - uni(s.on[k]), sound = dur_k + release;
      const float vg_k = uni(s.vg[k]);
      const int bank = (row0 + uni(s.pitch[k])) * H;
      // what depends on the sample alone
      float tf[SPT], t2[SPT], ra[SPT];
      unsigned ph[SPT];
      bool live[SPT], any = false;
#pragma unroll
      for (int j = 0; j < SPT; j++) {
        const long tau = tau0 + 4 * (tid + (j >> 2) * TPB) + (j & 3);
        live[j] = (unsigned long)tau < (unsigned long)sound;
        any = any || live[j];
        tf[j] = (float)tau;
        t2[j] = rel * (float)(tau > dur_k ? tau - dur_k : 0);
        ra[j] = (float)(tau + 1 < attack ? tau + 1 : (long)attack) / attf;
        ph[j] = (unsigned)tau;
      }
      if (__builtin_amdgcn_ballot_w64(any) == 0) continue;                      // no sample of this wave hears the record (no barrier below)
      for (int h = 0; h < H; h++) {
        const unsigned dphi = g.inc[bank + h];
        const float g0 = g.amp[bank + h] * vg_k, dc = g.dec[bank + h];
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

}  // namespace

extern "C" int hftt_clip_synth(const hftt_clip_synth_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_synth: null descriptor");
  HFTT_REQUIRE(d->n_notes >= 0, "clip_synth: n_notes=%d is negative", d->n_notes);
  HFTT_REQUIRE(d->notes || d->n_notes == 0, "clip_synth: notes is null at n_notes=%d", d->n_notes);
  HFTT_REQUIRE(d->row_ptr, "clip_synth: row_ptr is null");
  HFTT_REQUIRE(d->file_nsamp, "clip_synth: file_nsamp is null");
  HFTT_REQUIRE(d->win_file && d->win_start, "clip_synth: null window table (win_file / win_start)");
  HFTT_REQUIRE(d->inc && d->amp && d->dec && d->vel_gain && d->rel && d->attack && d->release, "clip_synth: null voice bank (inc / amp / dec / vel_gain / rel / attack / release)");
  HFTT_REQUIRE(d->voice_index, "clip_synth: voice_index is null");
  HFTT_REQUIRE(d->out && d->out_samp0 && d->out_win_file && d->out_win_start, "clip_synth: null output (out / out_samp0 / out_win_file / out_win_start)");
  HFTT_REQUIRE(d->n_fft == 2048, "clip_synth: n_fft=%d unsupported (2048 only)", d->n_fft);
  HFTT_REQUIRE(d->B >= 1 && d->B < (1 << 30), "clip_synth: B=%d outside 1 .. 2^30 (2 B pseudo-files)", d->B);
  HFTT_REQUIRE(d->width >= 1, "clip_synth: width=%d must be positive", d->width);
  HFTT_REQUIRE(d->hop >= 1, "clip_synth: hop=%d must be positive", d->hop);
  HFTT_REQUIRE(d->n_files >= 1, "clip_synth: n_files=%d must be positive", d->n_files);
  HFTT_REQUIRE(d->N >= 1 && d->N <= 128, "clip_synth: N=%d outside 1..128", d->N);
  HFTT_REQUIRE(d->V >= 1, "clip_synth: V=%d must be positive", d->V);
  HFTT_REQUIRE(d->H >= 1 && d->H <= HFTT_SYNTH_MAX_PARTIALS, "clip_synth: H=%d outside 1..%d partials", d->H, HFTT_SYNTH_MAX_PARTIALS);
  HFTT_REQUIRE((long)d->V * d->N * d->H < (1l << 31), "clip_synth: a bank of V=%d voices, N=%d pitches and H=%d partials exceeds 2^31 entries", d->V, d->N, d->H);
  HFTT_REQUIRE(d->lead >= 0, "clip_synth: lead=%d is negative", d->lead);
  HFTT_REQUIRE(d->sr > 0.0 && d->sr <= 1e12, "clip_synth: sr=%g must be positive (and finite)", d->sr);
  const __int128 need = ((__int128)synth_front(d->n_fft, d->hop, d->lead) + d->width - 1) * d->hop + d->n_fft / 2;
  HFTT_REQUIRE(d->span >= need, "clip_synth: span=%ld below the %ld samples a window of width=%d and lead=%d at hop=%d can show", (long)d->span, (long)need, d->width, d->lead,
               d->hop);
  const long ntiles = ((long)need + TILE - 1) / TILE;
  HFTT_REQUIRE((__int128)d->B * ntiles < (1l << 31), "clip_synth: B=%d windows of width=%d and lead=%d exceed 2^31 workgroups", d->B, d->width, d->lead);
  const dim3 grid((unsigned)((long)d->B * ntiles));
  return hftt_launch<clip_synth_kernel>("clip_synth", grid, dim3(TPB), 0, (hipStream_t)stream, *d, (int)ntiles);
}
