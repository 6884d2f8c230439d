// Clip log-mel (gfx950): the spectrogram windows of a training batch straight from a resident WAVEFORM corpus, one launch.
//   hftt_clip_logmel           B windows [width frames] of the files' concatenated samples (fp32 or int16) -> spec [B, n_mels, width] fp32
//   hftt_clip_logmel_warp      the same of the files played back at a per-window rate and delay: the staged sample is wave_warp.h's warp_sample
//   hftt_clip_logmel_mix       hftt_clip_logmel with a per-window partner (file, start frame, gain) added onto the primary's extent
//   hftt_clip_logmel_mix_warp  the same with each source played back under its own warp: both go through warp_sample
// A workgroup owns one window and a run of RUN consecutive frames.  It stages the (RUN - 1) * hop + n_fft samples those frames cover once in
// LDS -- converted, gained, noised, zeros outside the file: consecutive frames share 7/8 of them at hop = n_fft / 8 -- transforms frame after
// frame with logmel_kernel's frame transform (logmel_frame.h: packed 1024-point radix-4 Stockham transform, split pass, |X|^2, sequential CSR
// mel sum, logf), gathers the columns in an LDS tile [n_mels][RUN] and stores it along the frame axis: RUN * 4 = 64 contiguous bytes per
// (window, mel) row.  One writer per element, no atomics, no workspace.  A partner's sample is added into the same stage[j] slot, so the LDS
// layout, the frame transform and the tile store are the same in all four forms.  The staged sample in front of the noise term is clip_dry.h's
// one device function, which clip_room_kernel (clip_room.hip) convolves.  See include/hftt_hip.h for the contract.
#include "hftt_common.h"
#include "hftt_host.h"
#include "hftt_launch.h"
#include "clip_dry.h"
#include "logmel_frame.h"
#include "../../include/hftt_hip.h"

namespace {

constexpr int RUN = HFTT_CLIP_LOGMEL_RUN;        // frames per workgroup
constexpr int MAX_MELS = HFTT_CLIP_LOGMEL_MAX_MELS;
constexpr int STATIC_LDS = 2 * 1024 * 8 + 1028 * 4 + MAX_MELS * (RUN + 1) * 4;
static_assert(RUN == 16 && MAX_MELS == 256, "one thread per mel row; 16 lanes store one row segment");

// 1 / sqrt(21845), rounded once: the sum of four uniform bytes has variance 4 (256^2 - 1) / 12 = 21845
constexpr float NOISE_C = 0x1.bb688cp-8f;

// The noise term onto a staged dry sample (clip_dry.h): one fadd of one fmul, never an fma -- __fmul_rn / __fadd_rn are plain operators in this
// toolchain, which the compiler may contract: not in this function.  The noise is keyed on (file, sample), so every frame and every clip sees
// the same noisy waveform; nstd = fmul(noise_std[b], NOISE_C).
__device__ __forceinline__ float add_noise(float s, float nstd, uint64_t seed, uint32_t file, uint64_t i) {
#pragma clang fp contract(off)
  const uint32_t h = hftt_hash(seed, file, i);
  const int sum = (int)(h & 0xFFu) + (int)((h >> 8) & 0xFFu) + (int)((h >> 16) & 0xFFu) + (int)(h >> 24) - 510;
  const float nz = (float)sum * nstd;
  return s + nz;
}

// WARP: only the staging loop differs -- the window's frames are counted in the warped file and a staged sample is interpolated from the
// source in global memory (up to 26 taps; neighbouring lanes read overlapping spans).  The LDS arrays and the frame transform are the same.
// MIX: the staging loop adds a second source, the window's PARTNER (mx; include/hftt_hip.h, clip mixing), into the same stage[j] slot: the
// partner's (warped) sample at the primary's position moved by (mix_start - win_start) * hop, times mix_gain, added behind the primary's gain
// and in front of the noise.  Which samples are staged and which columns are fill follows the primary alone.  
struct clip_mix {
  hftt_clip_mix_args t;
  hftt_warp_args w;            // the partners' warps (WARP only)
};

// The partner tables are a trailing parameter pack -- empty or one clip_mix -- so that the forms without a partner keep the kernel arguments
// they always had.
__device__ __forceinline__ const clip_mix& clip_mix_of(const clip_mix& mx) { return mx; }

template <int NFFT, bool WARP, typename... MX>
__global__ __launch_bounds__(256) void clip_logmel_kernel(const hftt_clip_logmel_desc g, const hftt_warp_args wa, int nruns, const MX... mx_pack) {
  constexpr bool MIX = sizeof...(MX) == 1;
  static_assert(sizeof...(MX) <= 1, "at most one partner");
  constexpr int N = NFFT / 2;                         // complex points
  __shared__ float2 bufA[N];
  __shared__ float2 bufB[N];
  __shared__ float pw[N + 4];                         // N + 1 used; the dynamic part behind stays 16-byte aligned
  __shared__ float tile[MAX_MELS][RUN + 1];           // [mel][frame of the run], one word of padding: the column writes meet 32 banks
  extern __shared__ float stage[];                    // (RUN - 1) * hop + NFFT samples
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)nruns);
  const int c0 = (int)(blockIdx.x % (unsigned)nruns) * RUN;      // first column of the run
  const int ncol = g.width - c0 < RUN ? g.width - c0 : RUN;
  const int hop = g.hop;
  const int file = g.win_file[b];
  const clip_source A = clip_source_load<WARP>(g.file_samp0, g.n_files, g.total_samples, file, wa, b);
  const long n = A.n, np = A.np;                      // n < 0: no such file, every column is fill; np: samples of the file as the frames see it
  const long nframe = n >= 0 ? 1 + np / hop : 0;
  const long t0 = (long)g.win_start[b] + c0;          // file frame of column c0
  const bool any = t0 < nframe && t0 + ncol > 0;      // (the same for every thread: the barriers below are met by all or by none)
  if (any) {
    const long i0 = t0 * hop - NFFT / 2;              // sample of the file that stage[0] holds
    const int slen = (ncol - 1) * hop + NFFT;
    const float gain = g.gain ? g.gain[b] : 1.f;
    const float nstd = g.noise_std ? g.noise_std[b] * NOISE_C : 0.f;          // (a lone product: nothing to contract with)
    for (int j = tid; j < slen; j += 256) {
      const long i = i0 + j;
      float s = 0.f;                                  // outside [0, n): zeros, never a neighbouring file's samples
      if (i >= 0 && i < np) {
        s = clip_dry<WARP, false>(0.f, g.wave, g.wave_i16 != 0, A, wa.proto, i, g.gain != nullptr, gain);
        // with a partner the noise waits for the second pass below: it is added behind the partner's term
        if (!MIX && g.noise_std != nullptr) s = add_noise(s, nstd, g.seed, (uint32_t)file, (uint64_t)i);
      }
      stage[j] = s;
    }
    if constexpr (MIX) {
      // The partner (the same for every thread of the workgroup): its file as the primary's above, nB < 0 = it contributes nothing.  A pass
      // of its own over the slots this thread has just written (no barrier), so that the two sources' warps are not live together.
      const clip_mix& mx = clip_mix_of(mx_pack...);
      const clip_source Bs = clip_source_load<WARP>(g.file_samp0, g.n_files, g.total_samples, mx.t.mix_file[b], mx.w, b);
      const long nB = Bs.n;
      const long shiftB = ((long)mx.t.mix_start[b] - (long)g.win_start[b]) * hop;      // |.| < 2^32 * hop: no overflow
      const float gainB = mx.t.mix_gain[b];
      if (nB >= 0 || g.noise_std != nullptr) {
        for (int j = tid; j < slen; j += 256) {
          const long i = i0 + j;
          if (i < 0 || i >= np) continue;             // outside the primary's extent the staged zero stays
          float s = stage[j];
          if (nB >= 0) s = clip_dry<WARP, true>(s, g.wave, g.wave_i16 != 0, Bs, mx.w.proto, i + shiftB, true, gainB);
          if (g.noise_std != nullptr) s = add_noise(s, nstd, g.seed, (uint32_t)file, (uint64_t)i);
          stage[j] = s;
        }
      }
    }
  }
  const float* tc = g.twiddle;
  const float* ts = g.twiddle + NFFT / 2;
  float2 win[N / 256];                                // this thread's window entries, the same for every frame
#pragma unroll
  for (int u = 0; u < N / 256; u++) win[u] = make_float2(g.window[2 * (tid + 256 * u)], g.window[2 * (tid + 256 * u) + 1]);
  const bool mel = tid < g.n_mels;                    // n_mels <= MAX_MELS = the threads: thread m owns mel row m
  const int st = mel ? g.fb_start[tid] : 0, len = mel ? g.fb_len[tid] : 0, off = mel ? g.fb_off[tid] : 0;
  __syncthreads();
  for (int c = 0; c < ncol; c++) {
    const long t = t0 + c;
    if (t < 0 || t >= nframe) {                       // (uniform) a frame outside the file
      if (mel) tile[tid][c] = g.fill;
      continue;
    }
    const float* x = stage + c * hop;
#pragma unroll
    for (int u = 0; u < N / 256; u++) {
      const int k = tid + 256 * u;
      bufA[k] = make_float2(x[2 * k] * win[u].x, x[2 * k + 1] * win[u].y);
    }
    __syncthreads();
    float2* src = bufA;
    float2* dst = bufB;
#pragma unroll
    for (int Ns = 1; Ns < N; Ns *= 4) {
      frame_stage<NFFT>(src, dst, Ns, tc, ts, tid);
      float2* sw = src; src = dst; dst = sw;
    }
    frame_split<NFFT>(src, pw, tc, ts, tid);
    if (mel) tile[tid][c] = frame_mel(g.fb_w, pw, st, len, off, g.log_offset);
    // no barrier here: the next frame writes bufA, then (behind a barrier) bufB, and pw only behind six more
  }
  __syncthreads();
  // the run's columns of every mel row, 16 lanes per row: one contiguous piece of ncol * 4 bytes each
  float* out = (float*)g.out + (long)b * g.n_mels * g.width + c0;
  const int col = tid & (RUN - 1);
  if (col < ncol)
    for (int m = tid / RUN; m < g.n_mels; m += 256 / RUN) out[(long)m * g.width + col] = tile[m][col];
}

}  // namespace

// The refusals of hftt_clip_logmel_desc for every entry point (wa == nullptr: no warp), in front of the launch; *lds = the dynamic LDS in bytes,
// *nruns = the runs of RUN frames per window.
static int clip_logmel_refuse(const hftt_clip_logmel_desc* d, const hftt_warp_args* wa, long* lds_bytes, int* runs) {
  HFTT_REQUIRE(d->wave, "clip_logmel: wave is null");
  HFTT_REQUIRE(d->file_samp0, "clip_logmel: file_samp0 is null");
  HFTT_REQUIRE(d->win_file && d->win_start, "clip_logmel: null window table (win_file / win_start)");
  HFTT_REQUIRE(d->window && d->twiddle && d->fb_start && d->fb_len && d->fb_off && d->fb_w, "clip_logmel: null table (window / twiddle / fb_start / fb_len / fb_off / fb_w)");
  HFTT_REQUIRE(d->out, "clip_logmel: out is null");
  HFTT_REQUIRE(d->wave_i16 == 0 || d->wave_i16 == 1, "clip_logmel: wave_i16=%d (0 = fp32, 1 = int16)", d->wave_i16);
  HFTT_REQUIRE(d->n_fft == 2048, "clip_logmel: n_fft=%d unsupported (2048 only)", d->n_fft);
  HFTT_REQUIRE(d->B >= 1, "clip_logmel: B=%d must be positive", d->B);
  HFTT_REQUIRE(d->width >= 1, "clip_logmel: width=%d must be positive", d->width);
  HFTT_REQUIRE(d->n_mels >= 1 && d->n_mels <= MAX_MELS, "clip_logmel: n_mels=%d outside 1..%d (a workgroup's output tile)", d->n_mels, MAX_MELS);
  HFTT_REQUIRE(d->hop >= 1, "clip_logmel: hop=%d must be positive", d->hop);
  HFTT_REQUIRE(d->n_files >= 1, "clip_logmel: n_files=%d must be positive", d->n_files);
  HFTT_REQUIRE(d->total_samples >= 0, "clip_logmel: total_samples=%ld is negative", (long)d->total_samples);
  if (wa) {
    HFTT_REQUIRE(wa->step_q24 && wa->delay_q24 && wa->cut && wa->proto, "clip_logmel: null warp table (step_q24 / delay_q24 / cut / proto)");
    HFTT_REQUIRE(d->total_samples <= (1l << 38), "clip_logmel: total_samples=%ld beyond 2^38 (Q24 positions)", (long)d->total_samples);
  }
  const long lds = ((long)(RUN - 1) * d->hop + d->n_fft) * 4;
  HFTT_REQUIRE(lds + STATIC_LDS <= 64 * 1024, "clip_logmel: hop=%d: the %d frames of a workgroup cover %ld samples, beyond 64 KB of LDS", d->hop, RUN, lds / 4);
  const int nruns = hftt_ceil_div(d->width, RUN);
  HFTT_REQUIRE((long)d->B * nruns < (1l << 31), "clip_logmel: B=%d windows of width=%d exceed 2^31 workgroups", d->B, d->width);
  *lds_bytes = lds;
  *runs = nruns;
  return 0;
}

// the refusals of all four entry points and the launch; wa == nullptr: no source is warped (wb is not read), m == nullptr: no partner
static int clip_logmel_launch(const hftt_clip_logmel_desc* d, const hftt_warp_args* wa, const hftt_clip_mix_args* m, const hftt_warp_args* wb, void* stream) {
  long lds;
  int nruns;
  if (clip_logmel_refuse(d, wa, &lds, &nruns)) return 1;
  if (m) {
    HFTT_REQUIRE(m->mix_file && m->mix_start && m->mix_gain, "clip_logmel: null partner table (mix_file / mix_start / mix_gain)");
    if (wa) HFTT_REQUIRE(wb->step_q24 && wb->delay_q24 && wb->cut && wb->proto, "clip_logmel: null partner warp table (step_q24 / delay_q24 / cut / proto)");
  }
  const dim3 grid((unsigned)((long)d->B * nruns));
  if (m && wa) return hftt_launch<clip_logmel_kernel<2048, true, clip_mix>>("clip_logmel_mix_warp", grid, dim3(256), (int)lds, (hipStream_t)stream, *d, *wa, nruns, clip_mix{*m, *wb});
  if (m) return hftt_launch<clip_logmel_kernel<2048, false, clip_mix>>("clip_logmel_mix", grid, dim3(256), (int)lds, (hipStream_t)stream, *d, hftt_warp_args{}, nruns, clip_mix{*m, hftt_warp_args{}});
  if (wa) return hftt_launch<clip_logmel_kernel<2048, true>>("clip_logmel_warp", grid, dim3(256), (int)lds, (hipStream_t)stream, *d, *wa, nruns);
  return hftt_launch<clip_logmel_kernel<2048, false>>("clip_logmel", grid, dim3(256), (int)lds, (hipStream_t)stream, *d, hftt_warp_args{}, nruns);
}

extern "C" int hftt_clip_logmel(const hftt_clip_logmel_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_logmel: null descriptor");
  return clip_logmel_launch(d, nullptr, nullptr, nullptr, stream);
}

extern "C" int hftt_clip_logmel_warp(const hftt_clip_logmel_warp_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_logmel: null descriptor");
  return clip_logmel_launch(&d->base, &d->warp, nullptr, nullptr, stream);
}

extern "C" int hftt_clip_logmel_mix(const hftt_clip_logmel_mix_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_logmel: null descriptor");
  return clip_logmel_launch(&d->base, nullptr, &d->mix, nullptr, stream);
}

extern "C" int hftt_clip_logmel_mix_warp(const hftt_clip_logmel_mix_warp_desc* d, void* stream) {
  HFTT_REQUIRE(d, "clip_logmel: null descriptor");
  return clip_logmel_launch(&d->base, &d->warp, &d->mix, &d->mix_warp, stream);
}
