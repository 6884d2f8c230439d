// Clip room (gfx950): the dry signal of every window of a training batch convolved with one impulse response of a resident bank, one launch.
//   hftt_clip_room  B windows of the files' concatenated samples (fp32 or int16), optionally warped and mixed as hftt_clip_logmel_{warp,mix,mix_warp}
//                   stage them, times gain -> wet samples fp32 [B, span] and the tables under which a plain hftt_clip_logmel reads them as files
// A workgroup owns one window and a tile of TILE consecutive wet samples.  It stages the dry span the tile needs ONCE in LDS -- PAD + TILE samples,
// PAD = the response's taps rounded up to a multiple of four, through clip_dry.h's one dry-sample function, zeros outside the (warped) file --
// and then only multiplies: a thread owns GROUPS quads of four consecutive outputs and walks the taps four at a time in increasing order.  Per
// step and quad it reads ONE aligned float4 of the signal (ds_read_b128, lanes on consecutive 16-byte words: conflict-free) -- the four
// samples in front of the quad it already holds -- and does 16 fmas out of the 8 samples in registers; the four taps are one uniform 16-byte
// load from the bank in global memory.  acc[q] = fma(h[k], dry[i - k], acc[q]) for k = 0 .. taps - 1: every output takes every tap in the same
// order wherever its tile begins.  One writer per element, no atomics.  See include/hftt_hip.h for the contract.
#include "hftt_common.h"
#include "hftt_host.h"
#include "hftt_launch.h"
#include "clip_dry.h"
#include "../../include/hftt_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int GROUPS = 2;                            // quads of outputs per thread
constexpr int TILE = TPB * 4 * GROUPS;               // wet samples per workgroup
static_assert(TILE == 2048 && (HFTT_ROOM_MAX_TAPS + 4 + TILE) * 4 <= 64 * 1024, "the staged span of the longest response fits the default 64 KB of LDS");

// frames in front of a window whose samples its first frame reads: ceil((n_fft / 2) / hop)
__host__ __device__ inline long room_lead(int n_fft, int hop) { return (n_fft / 2 + hop - 1) / hop; }

// Four taps k0 .. k0 + 3 onto the quads: output q of a quad takes dry[i_q - k0 - m] = (cur, prev) entry 4 + q - m of the eight samples held,
// prev = the four samples in front of cur.  TAIL: the response ends inside these four (nt of them are taps).
template <bool TAIL>
__device__ __forceinline__ void room_taps(float (&acc)[GROUPS][4], const float4 (&cur)[GROUPS], const float4 (&prev)[GROUPS], const float* __restrict__ h, int nt) {
#pragma unroll
  for (int m = 0; m < 4; m++) {
    if (TAIL && m >= nt) break;
    const float hm = h[m];
#pragma unroll
    for (int g = 0; g < GROUPS; g++) {
      const float w[8] = {prev[g].x, prev[g].y, prev[g].z, prev[g].w, cur[g].x, cur[g].y, cur[g].z, cur[g].w};
#pragma unroll
      for (int q = 0; q < 4; q++) acc[g][q] = __builtin_fmaf(hm, w[4 + q - m], acc[g][q]);
    }
  }
}

template <bool WARP, bool MIX>
__global__ __launch_bounds__(TPB) void clip_room_kernel(const hftt_clip_room_desc g, int ntiles) {
  extern __shared__ float4 stage4[];                  // PAD + TILE samples; stage[j] = dry[tile0 - PAD + j]
  float* stage = reinterpret_cast<float*>(stage4);
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)ntiles);
  const int tile = (int)(blockIdx.x % (unsigned)ntiles);
  const int hop = g.hop;
  const int file = g.win_file[b];
  const clip_source A = clip_source_load<WARP>(g.file_samp0, g.n_files, g.total_samples, file, g.warp, b);
  const int r = g.ir_index[b];
  const long ws = g.win_start[b];
  const long lead = room_lead(g.n_fft, hop);
  const long ob = (ws > lead ? ws - lead : 0) * hop;                           // first sample of the pseudo-file
  long eb = (ws + g.width - 1) * hop + g.n_fft / 2;                            // |.| < 2^33 * hop: no overflow
  eb = eb < A.np ? eb : A.np;
  const bool valid = A.n >= 0 && r < g.n_ir && ob <= A.np;
  const long len = valid && eb > ob ? eb - ob : 0;                             // samples of the pseudo-file, <= span
  if (tile == 0 && tid == 0) {                        // the window's table entries, by one thread
    g.out_samp0[2 * b] = (long)b * g.span;
    g.out_samp0[2 * b + 1] = (long)b * g.span + len;
    if (b == g.B - 1) g.out_samp0[2 * g.B] = (long)g.B * g.span;
    g.out_win_file[b] = valid ? 2 * b : -1;
    g.out_win_start[b] = (int)(ws - ob / hop);        // win_start[b] itself, or `lead`
  }
  const long t0 = (long)tile * TILE;                  // of the pseudo-file
  if (t0 >= len) return;                              // (uniform) nothing of this tile is shown
  const bool wet = r >= 0;
  int taps = 0, pad = 0;
  const float* __restrict__ h = nullptr;
  if (wet) {
    taps = g.ir_taps[r];
    taps = taps < 1 ? 1 : taps > g.L ? g.L : taps;
    pad = ((taps - 1) / 4 + 1) * 4;
    h = g.ir + (long)r * g.L;
  }
  const long i0 = ob + t0 - pad;                      // sample of the (warped) file that stage[0] holds
  const int slen = pad + TILE;
  const float gain = g.gain ? g.gain[b] : 1.f;
  for (int j = tid; j < slen; j += TPB) {
    const long i = i0 + j;
    float s = 0.f;
    if (i >= 0 && i < A.np) s = clip_dry<WARP, false>(0.f, g.wave, g.wave_i16 != 0, A, g.warp.proto, i, g.gain != nullptr, gain);
    stage[j] = s;
  }
  if constexpr (MIX) {
    // the partner, in a pass of its own over the slots this thread has just written (as clip_logmel_kernel does)
    const clip_source Bs = clip_source_load<WARP>(g.file_samp0, g.n_files, g.total_samples, g.mix.mix_file[b], g.mix_warp, b);
    if (Bs.n >= 0) {
      const long shiftB = ((long)g.mix.mix_start[b] - ws) * hop;
      const float gainB = g.mix.mix_gain[b];
      for (int j = tid; j < slen; j += TPB) {
        const long i = i0 + j;
        if (i < 0 || i >= A.np) continue;             // outside the primary's extent the staged zero stays
        stage[j] = clip_dry<WARP, true>(stage[j], g.wave, g.wave_i16 != 0, Bs, g.mix_warp.proto, i + shiftB, true, gainB);
      }
    }
  }
  __syncthreads();
  float* out = (float*)g.out + (long)b * g.span + t0;
  const long left = len - t0;                         // outputs of this tile that exist (may exceed TILE)
  if (!wet) {                                         // a dry window: the staged samples, bit for bit
    for (int x = tid; x < TILE && x < left; x += TPB) out[x] = stage[x];
    return;
  }
  float acc[GROUPS][4] = {};
  float4 cur[GROUPS], prev[GROUPS];
  int at[GROUPS];                                     // float4 index of the quad's own samples
#pragma unroll
  for (int q = 0; q < GROUPS; q++) {
    at[q] = pad / 4 + tid + q * TPB;
    cur[q] = stage4[at[q]];
  }
  int k0 = 0;
  for (; k0 + 4 <= taps; k0 += 4) {
#pragma unroll
    for (int q = 0; q < GROUPS; q++) prev[q] = stage4[at[q] - k0 / 4 - 1];
    room_taps<false>(acc, cur, prev, h + k0, 4);
#pragma unroll
    for (int q = 0; q < GROUPS; q++) cur[q] = prev[q];
  }
  if (k0 < taps) {
#pragma unroll
    for (int q = 0; q < GROUPS; q++) prev[q] = stage4[at[q] - k0 / 4 - 1];
    room_taps<true>(acc, cur, prev, h + k0, taps - k0);
  }
#pragma unroll
  for (int q = 0; q < GROUPS; q++) {
    const int x = 4 * (tid + q * TPB);
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (x + e < left) out[x + e] = acc[q][e];
  }
}

}  // namespace

extern "C" int hftt_clip_room(const hftt_clip_room_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_room: null descriptor");
  HFTT_REQUIRE(d->wave, "clip_room: wave is null");
  HFTT_REQUIRE(d->file_samp0, "clip_room: file_samp0 is null");
  HFTT_REQUIRE(d->win_file && d->win_start, "clip_room: null window table (win_file / win_start)");
  HFTT_REQUIRE(d->ir && d->ir_taps && d->ir_index, "clip_room: null response table (ir / ir_taps / ir_index)");
  HFTT_REQUIRE(d->out && d->out_samp0 && d->out_win_file && d->out_win_start, "clip_room: null output (out / out_samp0 / out_win_file / out_win_start)");
  HFTT_REQUIRE(d->wave_i16 == 0 || d->wave_i16 == 1, "clip_room: wave_i16=%d (0 = fp32, 1 = int16)", d->wave_i16);
  HFTT_REQUIRE(d->n_fft == 2048, "clip_room: n_fft=%d unsupported (2048 only)", d->n_fft);
  HFTT_REQUIRE(d->B >= 1 && d->B < (1 << 30), "clip_room: B=%d outside 1 .. 2^30 (2 B pseudo-files)", d->B);
  HFTT_REQUIRE(d->width >= 1, "clip_room: width=%d must be positive", d->width);
  HFTT_REQUIRE(d->hop >= 1, "clip_room: hop=%d must be positive", d->hop);
  HFTT_REQUIRE(d->n_files >= 1, "clip_room: n_files=%d must be positive", d->n_files);
  HFTT_REQUIRE(d->total_samples >= 0, "clip_room: total_samples=%ld is negative", (long)d->total_samples);
  HFTT_REQUIRE(d->n_ir >= 1, "clip_room: n_ir=%d must be positive", d->n_ir);
  HFTT_REQUIRE(d->L >= 1 && d->L <= HFTT_ROOM_MAX_TAPS, "clip_room: L=%d outside 1..%d taps", d->L, HFTT_ROOM_MAX_TAPS);
  const hftt_warp_args& wa = d->warp;
  const hftt_warp_args& wb = d->mix_warp;
  const bool warp = wa.step_q24 || wa.delay_q24 || wa.cut || wa.proto;
  const bool mix = d->mix.mix_file || d->mix.mix_start || d->mix.mix_gain;
  const bool mix_warp = wb.step_q24 || wb.delay_q24 || wb.cut || wb.proto;
  if (warp) {
    HFTT_REQUIRE(wa.step_q24 && wa.delay_q24 && wa.cut && wa.proto, "clip_room: null warp table (step_q24 / delay_q24 / cut / proto: all or none)");
    HFTT_REQUIRE(d->total_samples <= (1l << 38), "clip_room: total_samples=%ld beyond 2^38 (Q24 positions)", (long)d->total_samples);
  }
  if (mix) HFTT_REQUIRE(d->mix.mix_file && d->mix.mix_start && d->mix.mix_gain, "clip_room: null partner table (mix_file / mix_start / mix_gain: all or none)");
  if (mix && warp) HFTT_REQUIRE(wb.step_q24 && wb.delay_q24 && wb.cut && wb.proto, "clip_room: null partner warp table (step_q24 / delay_q24 / cut / proto)");
  else HFTT_REQUIRE(!mix_warp, "clip_room: a partner warp table without both a warp and a partner");
  const long need = (room_lead(d->n_fft, d->hop) + d->width - 1) * d->hop + d->n_fft / 2;
  HFTT_REQUIRE(d->span >= need, "clip_room: span=%ld below the %ld samples a window of width=%d at hop=%d can show", (long)d->span, need, d->width, d->hop);
  const int ntiles = (int)((need + TILE - 1) / TILE);
  HFTT_REQUIRE((long)d->B * ntiles < (1l << 31), "clip_room: B=%d windows of width=%d exceed 2^31 workgroups", d->B, d->width);
  const int lds = (((d->L - 1) / 4 + 1) * 4 + TILE) * 4;
  const dim3 grid((unsigned)((long)d->B * ntiles));
  if (mix && warp) return hftt_launch<clip_room_kernel<true, true>>("clip_room", grid, dim3(TPB), lds, (hipStream_t)stream, *d, ntiles);
  if (mix) return hftt_launch<clip_room_kernel<false, true>>("clip_room", grid, dim3(TPB), lds, (hipStream_t)stream, *d, ntiles);
  if (warp) return hftt_launch<clip_room_kernel<true, false>>("clip_room", grid, dim3(TPB), lds, (hipStream_t)stream, *d, ntiles);
  return hftt_launch<clip_room_kernel<false, false>>("clip_room", grid, dim3(TPB), lds, (hipStream_t)stream, *d, ntiles);
}
