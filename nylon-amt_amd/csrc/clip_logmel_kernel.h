// The clip log-mel's workgroup body (gfx950), written once for the translation units that instantiate it: clip_logmel.hip (hftt_clip_logmel,
// hftt_clip_logmel_warp) and clip_mix.hip (hftt_clip_logmel_mix, hftt_clip_logmel_mix_warp).  Each of them instantiates clip_logmel_kernel and
// keeps its entry points and launches; see clip_logmel.hip for the description of the kernel.
#pragma once
#include "hftt_common.h"
#include "hftt_host.h"
#include "wave_warp.h"
#include "../../include/hftt_hip.h"

namespace {

constexpr int RUN = HFTT_CLIP_LOGMEL_RUN;        // frames per workgroup
constexpr int MAX_MELS = HFTT_CLIP_LOGMEL_MAX_MELS;
constexpr int STATIC_LDS = 2 * 1024 * 8 + 1028 * 4 + MAX_MELS * (RUN + 1) * 4;
static_assert(RUN == 16 && MAX_MELS == 256, "one thread per mel row; 16 lanes store one row segment");

// 1 / sqrt(21845), rounded once: the sum of four uniform bytes has variance 4 (256^2 - 1) / 12 = 21845
constexpr float NOISE_C = 0x1.bb688cp-8f;

// The sample that enters the window product: fmul by the gain, fadd of the noise term, one rounding each.  __fmul_rn / __fadd_rn are plain
// operators in this toolchain, which the compiler may contract into an fma: not in this function.  The noise is keyed on (file, sample), so
// every frame and every clip sees the same noisy waveform; nstd = fmul(noise_std[b], NOISE_C).
__device__ __forceinline__ float mix(float s, bool has_gain, float gain, bool has_noise, float nstd, uint64_t seed, uint32_t file, uint64_t i) {
#pragma clang fp contract(off)
  if (has_gain) s = s * gain;
  if (has_noise) {
    const uint32_t h = hftt_hash(seed, file, i);
    const int sum = (int)(h & 0xFFu) + (int)((h >> 8) & 0xFFu) + (int)((h >> 16) & 0xFFu) + (int)(h >> 24) - 510;
    const float nz = (float)sum * nstd;
    s = s + nz;
  }
  return s;
}

// the partner's term: fadd(s, fmul(sB, gainB)), two roundings
__device__ __forceinline__ float add_scaled(float s, float sB, float gainB) {
#pragma clang fp contract(off)
  const float p = sB * gainB;
  return s + p;
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
  static_assert(NFFT == 2048, "the stage count below is for 1024 complex points");
  constexpr int N = NFFT / 2, Q = N / 4;              // complex points, butterflies per stage (= threads)
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
  long samp0 = 0, n = -1;                             // n < 0: no such file, every column is fill
  if (file >= 0 && file < g.n_files) {
    samp0 = g.file_samp0[file];
    n = g.file_samp0[file + 1] - samp0;
    if (samp0 < 0 || n < 0 || samp0 + n > g.total_samples) n = -1;       // a table that leaves the corpus: nothing is read there
  }
  warp_win w = {};
  long np = n;                                        // samples of the file as the frames see it
  if constexpr (WARP) {
    w = warp_load(wa, b);
    if (!w.ok) n = -1;
    np = n >= 0 ? warp_len(n, w) : -1;
  }
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
        if constexpr (WARP) s = warp_sample(g.wave, g.wave_i16 != 0, samp0, n, np, wa.proto, w, i);
        else s = g.wave_i16 ? (float)((const short*)g.wave)[samp0 + i] * (1.f / 32768.f) : ((const float*)g.wave)[samp0 + i];
        // with a partner the noise waits for the second pass below: it is added behind the partner's term
        s = mix(s, g.gain != nullptr, gain, !MIX && g.noise_std != nullptr, nstd, g.seed, (uint32_t)file, (uint64_t)i);
      }
      stage[j] = s;
    }
    if constexpr (MIX) {
      // The partner (the same for every thread of the workgroup): its file as the primary's above, nB < 0 = it contributes nothing.  A pass
      // of its own over the slots this thread has just written (no barrier), so that the two sources' warps are not live together.
      const clip_mix& mx = clip_mix_of(mx_pack...);
      const int fileB = mx.t.mix_file[b];
      long sampB = 0, nB = -1;
      if (fileB >= 0 && fileB < g.n_files) {
        sampB = g.file_samp0[fileB];
        nB = g.file_samp0[fileB + 1] - sampB;
        if (sampB < 0 || nB < 0 || sampB + nB > g.total_samples) nB = -1;
      }
      warp_win wB = {};
      long npB = nB;
      if constexpr (WARP) {
        wB = warp_load(mx.w, b);
        if (!wB.ok) nB = -1;
        npB = nB >= 0 ? warp_len(nB, wB) : -1;
      }
      const long shiftB = ((long)mx.t.mix_start[b] - (long)g.win_start[b]) * hop;      // |.| < 2^32 * hop: no overflow
      const float gainB = mx.t.mix_gain[b];
      if (nB >= 0 || g.noise_std != nullptr) {
        for (int j = tid; j < slen; j += 256) {
          const long i = i0 + j;
          if (i < 0 || i >= np) continue;             // outside the primary's extent the staged zero stays
          float s = stage[j];
          if (nB >= 0) {
            const long iB = i + shiftB;
            float sB = 0.f;                           // outside [0, n'_B): zeros
            if (iB >= 0 && iB < npB) {
              if constexpr (WARP) sB = warp_sample(g.wave, g.wave_i16 != 0, sampB, nB, npB, mx.w.proto, wB, iB);
              else sB = g.wave_i16 ? (float)((const short*)g.wave)[sampB + iB] * (1.f / 32768.f) : ((const float*)g.wave)[sampB + iB];
            }
            s = add_scaled(s, sB, gainB);
          }
          stage[j] = mix(s, false, 1.f, g.noise_std != nullptr, nstd, g.seed, (uint32_t)file, (uint64_t)i);
        }
      }
    }
  }
  const float* tc = g.twiddle;
  const float* ts = g.twiddle + NFFT / 2;
  auto tw = [&](int m) {                              // e^(-2 pi i m / 2048), 0 <= m < 2048
    const int mm = m & (NFFT / 2 - 1);
    const float c = tc[mm], sn = ts[mm];
    return (m & (NFFT / 2)) ? make_float2(-c, sn) : make_float2(c, -sn);
  };
  auto cmul = [](float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); };
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
      const int j = tid, k = j & (Ns - 1);
      const int step = NFFT / (4 * Ns);               // twiddle index of exp(-2 pi i k / (4 Ns)) per unit k
      float2 v0 = src[j], v1 = src[j + Q], v2 = src[j + 2 * Q], v3 = src[j + 3 * Q];
      if (Ns > 1) { v1 = cmul(v1, tw(k * step)); v2 = cmul(v2, tw(2 * k * step)); v3 = cmul(v3, tw(3 * k * step)); }
      const float2 a02 = make_float2(v0.x + v2.x, v0.y + v2.y), s02 = make_float2(v0.x - v2.x, v0.y - v2.y);
      const float2 a13 = make_float2(v1.x + v3.x, v1.y + v3.y), s13 = make_float2(v1.x - v3.x, v1.y - v3.y);
      const int j0 = ((j - k) << 2) + k;              // (j / Ns) * 4 Ns + k
      dst[j0] = make_float2(a02.x + a13.x, a02.y + a13.y);
      dst[j0 + Ns] = make_float2(s02.x + s13.y, s02.y - s13.x);          // v0 - i v1 - v2 + i v3
      dst[j0 + 2 * Ns] = make_float2(a02.x - a13.x, a02.y - a13.y);
      dst[j0 + 3 * Ns] = make_float2(s02.x - s13.y, s02.y + s13.x);      // v0 + i v1 - v2 - i v3
      __syncthreads();
      float2* sw = src; src = dst; dst = sw;
    }
    // real spectrum: E = (Z[k] + conj Z[N-k]) / 2, O = (Z[k] - conj Z[N-k]) / (2i), X[k] = E + W^k O, k = 0 .. N (Z[N] = Z[0]); |X|^2
    for (int k = tid; k <= N; k += 256) {
      const float2 zk = src[k & (N - 1)], zn = src[(N - k) & (N - 1)];
      const float2 e = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
      const float2 o = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
      const float2 wo = cmul(o, tw(k));
      const float xr = e.x + wo.x, xi = e.y + wo.y;
      pw[k] = xr * xr + xi * xi;
    }
    __syncthreads();
    if (mel) {
      float acc = 0.f;
      for (int j = 0; j < len; j++) acc += g.fb_w[off + j] * pw[st + j];
      tile[tid][c] = logf(acc + g.log_offset);
    }
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

// The refusals of every entry point that launches clip_logmel_kernel (wa == nullptr: no warp), in front of the launch; *lds = the dynamic LDS in
// bytes, *nruns = the runs of RUN frames per window.
static inline int clip_logmel_refuse(const hftt_clip_logmel_desc* d, const hftt_warp_args* wa, long* lds_bytes, int* runs) {
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
