// Streaming resampler (gfx950): hftt_resample's polyphase FIR with its state carried forward, S streams in one launch.
//   grid (ceil(max_count / 256), S): workgroup (x, s) produces outputs out_first[s] + 256 x .. + 256 of stream s, from the stream's packed input
//   -- the tail the host carried over from the last call followed by the new samples, fp32 or int16 -- into the stream's slot of the resampled
//   store; at a close it also zero-fills the slot behind the last output, up to the last sample the file's final log-mel frame reads.
// The window staging and the tap loop are resample_fir.h's, the ones resample_kernel (logmel.hip) runs: an output reads the same samples in the
// same order, so every push's outputs are the whole-file kernel's, bit for bit.  What differs is the source of a staged sample: absolute index i
// of the stream's own timeline lies at wave[in_off + i - in_first] for in_first <= i < in_end and is zero elsewhere -- in front of sample 0, and at
// or beyond the end of a closing stream; for a stream that is not closing the host never asks for an output whose window reaches in_end.
// Every index that comes out of the device tables is also held inside [0, wave_len) / [0, store_len): a wrong table loses samples, it never
// leaves the two buffers.  Ordinary vector stores, one writer per element, no atomics.  See include/hftt_hip.h for the contract.
#include "hftt_common.h"
#include "hftt_host.h"
#include "hftt_launch.h"
#include "resample_fir.h"
#include "../../include/hftt_hip.h"

namespace {

enum { T_IN_OFF = 0, T_IN_FIRST, T_IN_END, T_CLOSING, T_OUT_FIRST, T_COUNT, T_OUT_POS, T_FILL };
static_assert(T_FILL + 1 == HFTT_RESAMPLE_STREAM_ROWS, "the rows of the per-stream table");

template <bool I16>
__global__ __launch_bounds__(256) void resample_stream_kernel(const hftt_resample_stream_desc g) {
  extern __shared__ float win[];
  const int tid = threadIdx.x;
  const int s = blockIdx.y;
  const int64_t* tab = g.tab + s;
  const long count = tab[(long)T_COUNT * g.S];
  const long fill = tab[(long)T_CLOSING * g.S] != 0 ? tab[(long)T_FILL * g.S] : 0;
  const long b0 = (long)blockIdx.x * 256;
  if (b0 >= count && b0 >= fill) return;              // nothing to do (count 0, no close): before any sample is touched
  const long out_first = tab[(long)T_OUT_FIRST * g.S], out_pos = tab[(long)T_OUT_POS * g.S];
  // the close: zeros behind the last output, spread over the stream's workgroups
  for (long i = b0 + tid; i < fill; i += (long)gridDim.x * 256) {
    const long p = out_pos + count + i;
    if (p >= 0 && p < g.store_len) g.store[p] = 0.f;
  }
  if (b0 >= count) return;                            // (the same for every thread: the barrier below is met by all or by none)
  const long in_off = tab[(long)T_IN_OFF * g.S], in_first = tab[(long)T_IN_FIRST * g.S], in_end = tab[(long)T_IN_END * g.S];
  const long o0 = out_first + b0;
  const long olast = out_first + (b0 + 255 < count ? b0 + 255 : count - 1);
  const resample_win wn = resample_window(o0, olast, g.up, g.down, g.width, g.taps);
  resample_stage(win, wn, tid, [&](long i) {
    if (i < 0 || i < in_first || i >= in_end) return 0.f;
    const long j = in_off + (i - in_first);
    if (j < 0 || j >= g.wave_len) return 0.f;
    if constexpr (I16) return (float)((const short*)g.wave)[j] * (1.0f / 32768.0f);
    else return ((const float*)g.wave)[j];
  });
  if (b0 + tid >= count) return;
  const long p = out_pos + b0 + tid;
  const float y = resample_taps(win, wn, g.kernel, o0 + tid, g.up, g.down, g.taps);
  if (p >= 0 && p < g.store_len) g.store[p] = y;
}

}  // namespace

extern "C" int hftt_resample_stream(const hftt_resample_stream_desc* d, void* stream) {
  HFTT_REQUIRE(d, "resample_stream: null descriptor");
  HFTT_REQUIRE(d->wave, "resample_stream: wave is null");
  HFTT_REQUIRE(d->kernel, "resample_stream: kernel is null");
  HFTT_REQUIRE(d->tab, "resample_stream: tab is null");
  HFTT_REQUIRE(d->store, "resample_stream: store is null");
  HFTT_REQUIRE(d->S >= 1 && d->S <= 65535, "resample_stream: S=%d outside 1..65535 (one grid row per stream)", d->S);
  HFTT_REQUIRE(d->up > 0 && d->down > 0, "resample_stream: up=%d, down=%d must be positive", d->up, d->down);
  HFTT_REQUIRE(d->width >= 0 && d->taps == 2 * d->width + d->down, "resample_stream: taps=%d must be 2 * width + down (width=%d, down=%d: the kernel rows of Resample)", d->taps, d->width, d->down);
  HFTT_REQUIRE(d->max_count >= 0 && d->max_count < (1l << 39), "resample_stream: max_count=%ld outside 0..2^39", (long)d->max_count);
  HFTT_REQUIRE(d->wave_i16 == 0 || d->wave_i16 == 1, "resample_stream: wave_i16=%d (0 = fp32, 1 = int16)", d->wave_i16);
  HFTT_REQUIRE(d->wave_len >= 0 && d->store_len >= 0, "resample_stream: wave_len=%ld, store_len=%ld must not be negative", (long)d->wave_len, (long)d->store_len);
  const long wlen = (long)(255 / d->up + 1) * d->down + d->taps;      // the input window of 256 consecutive outputs, staged in LDS
  HFTT_REQUIRE(wlen * 4 <= 64 * 1024, "resample_stream: the input window of one workgroup (%ld samples at down = %d, taps = %d) exceeds 64 KB of LDS", wlen, d->down, d->taps);
  const long gx = d->max_count > 0 ? (d->max_count + 255) / 256 : 1;
  const dim3 grid((unsigned)gx, (unsigned)d->S);
  if (d->wave_i16) return hftt_launch<resample_stream_kernel<true>>("resample_stream", grid, dim3(256), (int)(wlen * 4), (hipStream_t)stream, *d);
  return hftt_launch<resample_stream_kernel<false>>("resample_stream", grid, dim3(256), (int)(wlen * 4), (hipStream_t)stream, *d);
}
