// Log-mel front end (gfx950): one workgroup per STFT frame.
//   frame (centred, zero padded) * periodic hann -> real 2048-point FFT in LDS (1024-point complex radix-4 Stockham + split) -> |X|^2 (1025 bins)
//   -> sparse slaney/htk mel filterbank (CSR by mel: ~2k non-zeros of 1025x256) -> log(. + offset)
// Replaces torchaudio MelSpectrogram + log of AMT.wav2feature (model/amt.py:59-61); see include/hftt_hip.h.
#include "hftt_common.h"
#include "hftt_launch.h"
#include "logmel_frame.h"
#include "resample_fir.h"
#include "../../include/hftt_hip.h"

namespace {

// The frame is real: its 2048-point transform is one 1024-point complex radix-4 Stockham transform of the packed frame plus a split pass
// (logmel_frame.h: frame_stage and frame_split, written once for this kernel and clip_logmel_kernel).  Here: the frame's start, the packing
// -- global loads, each slot with its own bounds test --, the loop over the stages and the store of one mel row per thread and pass.
template <int NFFT>
__global__ __launch_bounds__(256) void logmel_kernel(const hftt_logmel_desc g) {
  constexpr int N = NFFT / 2;                         // complex points
  __shared__ float2 bufA[N];
  __shared__ float2 bufB[N];
  __shared__ float pw[N + 1];
  const int tid = threadIdx.x;
  const long frame = blockIdx.x;
  const long start = frame * g.hop - NFFT / 2;
  const float* tc = g.twiddle;
  const float* ts = g.twiddle + NFFT / 2;
#pragma unroll
  for (int u = 0; u < N / 256; u++) {
    const int n = tid + 256 * u;
    const long s0 = start + 2 * n;
    const float xe = (s0 >= 0 && s0 < g.n_samples) ? g.wave[s0] * g.window[2 * n] : 0.f;
    const float xo = (s0 + 1 >= 0 && s0 + 1 < g.n_samples) ? g.wave[s0 + 1] * g.window[2 * n + 1] : 0.f;
    bufA[n] = make_float2(xe, xo);
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
  for (int m = tid; m < g.n_mels; m += 256)
    g.feat[frame * g.n_mels + m] = frame_mel(g.fb_w, pw, g.fb_start[m], g.fb_len[m], g.fb_off[m], g.log_offset);
}

// Polyphase band-limited resampling (the convolution of torchaudio.transforms.Resample, model/amt.py:57-58): output sample f * new + p is the
// dot product of taps input samples starting at f * orig - width with kernel row p.  One thread per output sample.  Round 6: a workgroup's 256
// consecutive outputs span at most 255 / up + 1 input frames, so their input window ((f1 - f0) * down + taps samples, zero-filled outside the
// signal) is staged in LDS once -- the tap loop has no bounds test and reads the window as LDS broadcasts -- and the loop runs four
// independent accumulators, sixteen kernel-row loads in flight per lane (the row of a lane is its own 4 x taps bytes of the [up, taps] table,
// L2-resident: <= 300 KB at 44.1 -> 16 kHz; the round-5 loop carried one dependent FMA and one bounds-tested load per tap: 1.3 ms per minute
// of 44.1 kHz audio).  The window staging and the tap loop are resample_fir.h's, shared with resample_stream_kernel (resample_stream.hip).
__global__ __launch_bounds__(256) void resample_kernel(const hftt_resample_desc g) {
  extern __shared__ float win[];
  const int tid = threadIdx.x;
  const long o0 = (long)blockIdx.x * 256;
  const long olast = (o0 + 255 < g.n_out ? o0 + 255 : g.n_out - 1);
  const resample_win wn = resample_window(o0, olast, g.up, g.down, g.width, g.taps);
  resample_stage(win, wn, tid, [&](long s) { return (s >= 0 && s < g.n_in) ? g.wave[s] : 0.f; });
  const long o = o0 + tid;
  if (o >= g.n_out) return;
  g.out[o] = resample_taps(win, wn, g.kernel, o, g.up, g.down, g.taps);
}

}  // namespace

extern "C" int hftt_resample(const hftt_resample_desc* d, void* stream) {
  HFTT_REQUIRE(d && d->wave && d->kernel && d->out, "resample: null operand");
  HFTT_REQUIRE(d->up > 0 && d->down > 0 && d->taps > 0 && d->width >= 0 && d->n_in > 0 && d->n_out > 0, "resample: bad shape");
  HFTT_REQUIRE(d->taps == 2 * d->width + d->down, "resample: taps must be 2 * width + down (the kernel rows of Resample)");
  HFTT_REQUIRE(d->n_out <= (d->n_in * d->up + d->down - 1) / d->down, "resample: n_out exceeds ceil(n_in * up / down)");
  const long wlen = (long)(255 / d->up + 1) * d->down + d->taps;      // the input window of 256 consecutive outputs, staged in LDS
  HFTT_REQUIRE(wlen * 4 <= 64 * 1024, "resample: the input window of one workgroup (%ld samples at down = %d, taps = %d) exceeds 64 KB of LDS", wlen, d->down, d->taps);
  return hftt_launch<resample_kernel>("resample", dim3((unsigned)((d->n_out + 255) / 256)), dim3(256), (int)(wlen * 4), (hipStream_t)stream, *d);
}

extern "C" int hftt_logmel(const hftt_logmel_desc* d, void* stream) {
  HFTT_REQUIRE(d && d->wave && d->window && d->twiddle && d->fb_start && d->fb_len && d->fb_off && d->fb_w && d->feat, "logmel: null operand");
  HFTT_REQUIRE(d->n_fft == 2048, "logmel: n_fft=%d unsupported (2048 only)", d->n_fft);
  HFTT_REQUIRE(d->hop > 0 && d->n_mels > 0 && d->n_frames > 0 && d->n_samples > 0, "logmel: bad shape");
  HFTT_REQUIRE(d->n_frames == 1 + d->n_samples / d->hop, "logmel: n_frames must be 1 + n_samples/hop");
  return hftt_launch<logmel_kernel<2048>>("logmel", dim3((unsigned)d->n_frames), dim3(256), 0, (hipStream_t)stream, *d);
}
