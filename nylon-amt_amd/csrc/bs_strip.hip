// Strip kernels of the bf16 mode for SMALL widths (round 5): every nn.Linear with K, N <= 192 and the fused position-wise feed-forward block
// d = 64 / p = 128 of the reference's default model (training/m_training.py:56-61) -- BASELINE config 2, "Tiny hFT bf16".  Until round 5 the
// bf16 mode at this size ran the round-1 block GEMMs (51 % of its step) and was slower than the x3 mode.  The kernels are small_strip.h's, the
// family the x3 mode runs at this size; this file holds what the bf16 activation stream changes (the policy BsStream) and the two entry points:
//   * the weights in LDS are the hi fragments only (<= 24 KB; 32 KB for the fused block's two): this family reads the hi fragment of each 2 KB
//     (hi, lo) pair of the compact pack (the bf16 rounding of the weight) and skips the lo one, so one pack serves both precision modes;
//   * every tensor between kernels is bf16; results leave as whole 128-byte lines through a wave-private LDS patch (strip_pipe.h: patch_put /
//     patch_flush -- a PAIR of 32-column tiles at a time; every N of this family is a multiple of 64);
//   * one MFMA pass (bf16 operands, fp32 accumulate).
#include <stdlib.h>
#include <type_traits>
#include <utility>
#include "hftt_common.h"
#include "hftt_launch.h"
#include "strip_internal.h"
#include "../../include/hftt_hip.h"

namespace {

#include "strip_pipe.h"

// The bf16 activation stream: a chunk is the 16 bytes as they lie in memory, one MFMA pass on the hi fragment of each pair, every tensor bf16
// (the h16 of the hooks is always true here), results through the pair patch.
struct BsStream {
  using Chunk = u4v;
  static constexpr int PAIR_BYTES = 1024;             // the hi fragment of each (hi, lo) pair
  static constexpr int STAGE_BYTES = PATCH_BYTES;
  static constexpr const char* LINEAR_WHAT = "bs_strip_linear";
  static constexpr const char* MLP_WHAT = "bs_strip_mlp";
  static constexpr bool STAGES_OUTSIDE = false;
  static constexpr int wgs(int) { return 2; }         // (three by LDS for most shapes, two by the launch bound)

  // hi fragments of `pairs` (hi, lo) pairs -> LDS, 1 KB each (16 bytes per thread and step)
  static __device__ __forceinline__ void copy_weights(unsigned char* lds, const unsigned short* w, int pairs, int tid) {
    const unsigned char* src = reinterpret_cast<const unsigned char*>(w);
    for (int i = tid; i < pairs * 64; i += 256) {
      const int pr = i >> 6, c = i & 63;
      *reinterpret_cast<uint4*>(lds + pr * 1024 + c * 16) = *reinterpret_cast<const uint4*>(src + (long)pr * 2048 + c * 16);
    }
  }
  // chunk ch = 2 * pt + u of the lane's row view (row + 16 * h): features 32 * pt + 8 * u + [0, 8) of the lane half
  template <int KC>
  static __device__ __forceinline__ void load_strip(u4v (&xr)[KC], const void* x, long off) {
    const unsigned short* p0 = reinterpret_cast<const unsigned short*>(x) + off;
#pragma unroll
    for (int c = 0; c < KC; c++) xr[c] = *reinterpret_cast<const u4v*>(p0 + (c >> 1) * 32 + (c & 1) * 8);
  }
  static __device__ __forceinline__ void tile_mac(const unsigned char* wl, int pair, const u4v& x, f32x16& acc) {
    acc = mfma32(*reinterpret_cast<const bf16x8*>(wl + pair * 1024), as_frag(x), acc);
  }
  static __device__ __forceinline__ void load16(const void* base, long off, bool, float* v) {
    const unsigned short* p = reinterpret_cast<const unsigned short*>(base) + off;
    const u4v a = *reinterpret_cast<const u4v*>(p), b = *reinterpret_cast<const u4v*>(p + 8);
    unpack8(a, v); unpack8(b, v + 8);
  }
  static __device__ __forceinline__ void values8(const u4v& c, float* v) { unpack8(c, v); }
  static __device__ __forceinline__ void split16(const float* v, u4v (&hf)[2]) { hf[0] = pack8u(v); hf[1] = pack8u(v + 8); }
  // whole 128-byte lines through the wave's patch (strip_pipe.h), a PAIR of tiles at a time: the odd tile flushes the pair
  static __device__ __forceinline__ void* rows(void* base, long off, bool) { return reinterpret_cast<unsigned short*>(base) + off; }
  static __device__ __forceinline__ void emit(unsigned char* patch, const float* v, int j, int hb, int lane, const void* rows, long ld, int t, bool ok, bool) {
    if (!ok) return;
    patch_put(patch, j, hb, t & 1, pack8u(v), pack8u(v + 8));
    if (t & 1) patch_flush(patch, lane, rows, (int)ld, t >> 1);
  }
  template <int K32, int NT, bool LN, bool HR>
  static int launch_linear(dim3 grid, int lds, hipStream_t st, const hftt_strip_desc& d);
  template <int MODE, bool HH>
  static int launch_mlp(dim3 grid, int lds, hipStream_t st, const hftt_ffn_desc& d);
};

#include "small_strip.h"

template <int K32, int NT, bool LN, bool HR>
__global__ __launch_bounds__(256, 2) void bs_linear_kernel(const hftt_strip_desc g) {
  static_assert(NT % 2 == 0, "tile pairs");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  small_linear<BsStream, K32, NT, LN, HR>(g, smem);
}
template <int MODE>
__global__ __launch_bounds__(256, 2) void bs_mlp_kernel(const hftt_ffn_desc g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  small_mlp<BsStream, MODE, true>(g, smem);
}
template <int K32, int NT, bool LN, bool HR>
int BsStream::launch_linear(dim3 grid, int lds, hipStream_t st, const hftt_strip_desc& d) {
  return hftt_launch<bs_linear_kernel<K32, NT, LN, HR>>(LINEAR_WHAT, grid, dim3(256), lds, st, d);
}
template <int MODE, bool HH>
int BsStream::launch_mlp(dim3 grid, int lds, hipStream_t st, const hftt_ffn_desc& d) {
  return hftt_launch<bs_mlp_kernel<MODE>>(MLP_WHAT, grid, dim3(256), lds, st, d);
}

}  // namespace

// -1: not a shape / storage of this family (the caller goes on to its own checks); otherwise the launch status.
// The shapes of the d = 64 model (K x N): forward 64x192 (q, k, v), 64x128 (cross k, v), 64x64 (cross q; fc_o + LayerNorm), backward 64x64,
// 192x64 / 128x64 (dX of the fused projections, + residual)
int hftt_bs_strip_linear_try(const hftt_strip_desc& d, hipStream_t st) {
  const uint32_t bf = HFTT_SL_X_BF16 | HFTT_SL_C_BF16;
  if ((d.flags & bf) != bf || d.N > 192 || d.K > 192 || d.N % 64 != 0 || d.K % 64 != 0) return -1;
  if (d.M <= 0 || d.M % 32 != 0 || d.x == nullptr || d.w == nullptr || d.C == nullptr || d.gate != nullptr) {
    hftt_set_error("bs_strip_linear: M=%d must be a positive multiple of 32, x / w / C non-null, no gate", d.M);
    return 1;
  }
  if (d.residual != nullptr && !(d.flags & HFTT_SL_RES_BF16)) { hftt_set_error("bs_strip_linear: the residual of the bf16 small-width family is bf16"); return 1; }
  if ((((uintptr_t)d.x | (uintptr_t)d.C | (uintptr_t)d.w | (uintptr_t)d.residual | (uintptr_t)d.pre_ln_out) & 15) != 0 || d.ldx % 8 != 0 || d.ldc % 8 != 0 ||
      (d.residual != nullptr && d.ldr % 8 != 0)) {
    hftt_set_error("bs_strip_linear: operands must be 16-byte aligned with row strides that are multiples of 8 elements");
    return 1;
  }
  if (d.drop_p < 0.f || d.drop_p >= 1.f || d.res_mod < 0 || (long)d.M * d.N >= (1L << 33)) { hftt_set_error("bs_strip_linear: drop_p / res_mod / M*N out of range"); return 1; }
  if (d.ln_gamma != nullptr && (d.N != 64 || d.ln_beta == nullptr || d.ldc != 64 || (d.flags & HFTT_SL_RELU))) { hftt_set_error("bs_strip_linear: LayerNorm needs N == ldc == 64, beta, no ReLU"); return 1; }
  return small_dispatch_linear<BsStream>(d, st);
}

int hftt_bs_strip_mlp_try(const hftt_ffn_desc& d, hipStream_t st) {
  if (d.d != 64 || d.p != 128) return -1;
  // the family computes on the bf16 stream only: the same storage requirement as check_ffn (strip_gemm.hip) -- a d = 64 descriptor without
  // the all-bf16 flags is an error here, not a reinterpretation of fp32 buffers
  const uint32_t all = HFTT_SL_X_BF16 | HFTT_SL_C_BF16 | HFTT_SL_RES_BF16;
  if ((d.flags & all) != all) { hftt_set_error("bs_strip_mlp: the fused block is all-bf16 (flags X_BF16 | C_BF16 | RES_BF16), got flags 0x%x", d.flags); return 1; }
  if ((long)d.M * d.p >= (1L << 33)) { hftt_set_error("bs_strip_mlp: M*p too large for the 32-bit dropout pair index"); return 1; }
  if (d.M <= 0 || d.M % 32 != 0 || d.x == nullptr || d.w == nullptr || d.y == nullptr) { hftt_set_error("bs_strip_mlp: M=%d must be a positive multiple of 32, x / w / y non-null", d.M); return 1; }
  if ((((uintptr_t)d.x | (uintptr_t)d.y | (uintptr_t)d.w | (uintptr_t)d.residual | (uintptr_t)d.pre_ln_out | (uintptr_t)d.h_out | (uintptr_t)d.gate) & 15) != 0 ||
      d.ldx % 8 != 0 || d.ldy % 8 != 0 || (d.h_out != nullptr && d.ldh % 8 != 0) || (d.gate != nullptr && d.ldg % 8 != 0) || (d.residual != nullptr && d.ldr % 8 != 0)) {
    hftt_set_error("bs_strip_mlp: operands must be 16-byte aligned with row strides that are multiples of 8 elements");
    return 1;
  }
  if (d.drop_p < 0.f || d.drop_p >= 1.f) { hftt_set_error("bs_strip_mlp: drop_p out of range"); return 1; }
  if (d.mode == 0) {
    if (d.ln_gamma == nullptr || d.ln_beta == nullptr || d.ldy != 64 || d.residual != nullptr) { hftt_set_error("bs_strip_mlp: the forward needs gamma, beta, ldy == 64 and takes its residual from x"); return 1; }
    return small_launch_mlp<BsStream, 0, true>(d, st);
  }
  if (d.gate == nullptr || d.h_out == nullptr) { hftt_set_error("bs_strip_mlp: the backward needs the stored hidden (gate) and the dh output"); return 1; }
  return small_launch_mlp<BsStream, 1, true>(d, st);
}
