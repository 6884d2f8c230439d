// Strip kernels for SMALL widths (the reference's default model, training/m_training.py:56-61: d = 64, ff = 128): every nn.Linear with
// K, N <= 192 and the fused position-wise feed-forward block d = 64 / p = 128, written once for both activation streams.  Included inside the
// anonymous namespace of x3_strip.hip (split-operand modes: policy X3Stream<E>) and of bs_strip.hip (bf16 stream: policy BsStream), behind
// strip_pipe.h and the helpers the unit's policy uses.
//
// What is different from the d = 256 family: the WHOLE weight matrix of a launch fits LDS (<= 48 KB as hi + lo fragment pairs, half of that
// for the bf16 stream, which keeps the hi fragments only; 64 / 32 KB for the fused block), so there is no ring, no per-slot barrier and no
// weight traffic after the first microsecond -- a workgroup copies the pack once and then walks 128-token blocks, each wave on its own
// 32-token strip (MFMA B operand).  The weights are the A operand, so accumulator register g of a lane is feature 16 h + g of the lane's token
// and bias / ReLU / dropout / residual / LayerNorm run per lane.  These launches are HBM-bound by a wide margin (arithmetic intensity
// <= 128 F/B at d = 64), so the design goal is bytes in flight: small register footprints (ONE accumulator tile) for 2-3 workgroups per CU,
// whole-line stores, nothing else.
//
// Pack: hftt_x3_strip_pack order 2 ("compact"): fragment pair (k chunk c, output tile t) at pair index slot_offset + c * NT + t
// (slot_stride = NT = N / 32), 2 KB per pair: 1 KB hi fragment, 1 KB lo fragment, lane layout as in the other orders.  One pack (bf16 halves)
// serves both precision modes of the small model: the bf16 stream reads the hi fragment (the bf16 rounding of the weight) and skips the lo one.
//
// The stream policy P supplies what differs between the two streams:
//   Chunk                                      8 features of the lane's token as the B operand of one k chunk
//   PAIR_BYTES, STAGE_BYTES, wgs(lds)          LDS bytes per fragment pair and per wave's staging patch; workgroups per CU
//   LINEAR_WHAT, MLP_WHAT                      the name a launch goes by (hftt_launch, error texts)
//   copy_weights(lds, w, pairs, tid)           packed pairs -> LDS
//   load_strip(xr, x, off)                     the lane's KC chunks of the row view at element offset off (+ conversion)
//   tile_mac(wl, pair, chunk, acc)             acc += W(pair) . chunk
//   load16(base, off, h16, v)                  16 residual / gate values at element offset off (h16: stored as bf16)
//   values8(chunk, v)                          the 8 values of a held chunk (the fused block's residual is its input)
//   split16(v, hf)                             16 hidden values -> the two chunks of the second GEMM's operand
//   rows(base, off, h16)                       the row-major tensor base at element offset off (h16: stored as bf16)
//   emit(stg, v, j, hb, lane, rows, ld, t, ok, h16)
//                                              the lane's 16 values of 32-column tile t of the wave's 32 rows (`rows`: the first of them);
//                                              tiles of a tensor arrive in order t = 0, 1, ...; ok wave-uniform
//   STAGES_OUTSIDE                             whether an OPTIONAL tensor's emits are entered for a strip outside M as well (either answer stores
//                                              the same; hipcc allocates each stream's kernels best with the test where that stream had it)
//   launch_linear<K32, NT, LN, HR>(...), launch_mlp<MODE, HH>(...)      hftt_launch of the unit's __global__ symbol
#pragma once

// the lane's place in block blk of the persistent loop
struct SmallLane {
  int hb;                                             // lane >> 5, re-formed per block
  long row0, tok, tokc;                               // the wave's first token, the lane's token, the same clamped to the last row
  bool wave_ok;                                       // the wave's strip lies inside M (M % 32 == 0: host check)
};
__device__ __forceinline__ SmallLane small_lane(long blk, int wave, int j, int h, int M) {
  SmallLane s;
  int hb = h;
  asm volatile("" : "+v"(hb));                       // (per-tile column arithmetic stays inside the iteration)
  s.hb = hb;
  s.row0 = blk * 128 + wave * 32;
  s.tok = s.row0 + j;
  s.wave_ok = s.row0 < M;
  s.tokc = s.tok < M ? s.tok : (long)M - 1;
  return s;
}
__device__ __forceinline__ void small_bias(f32x16& acc, const float* p) {
  float b[16];
  lds16f(p, b);
#pragma unroll
  for (int q = 0; q < 16; q++) acc[q] = b[q];
}

// LayerNorm over the 64 features of the lane's token (32 in acc, partner lane ^ 32 the rest); the pre-LayerNorm rows (training, `pre`: the wave's
// first, or NULL), then the output (`y`)
template <typename P>
__device__ __forceinline__ void small_ln_rows(f32x16 (&acc)[2], const float* gamma_lds, const float* beta_lds, unsigned char* stg, int j, int lane, const SmallLane& s,
                                              float* mean_out, float* rstd_out, void* pre, bool pre16, void* y, long ld) {
  float sum = 0.f;
#pragma unroll
  for (int ot = 0; ot < 2; ot++)
#pragma unroll
    for (int q = 0; q < 16; q++) sum += acc[ot][q];
  const float mean = xor32_sum(sum) * (1.0f / 64.0f);
  float qs = 0.f;
#pragma unroll
  for (int ot = 0; ot < 2; ot++)
#pragma unroll
    for (int q = 0; q < 16; q++) { const float dlt = acc[ot][q] - mean; qs += dlt * dlt; }
  const float rstd = 1.0f / sqrtf(xor32_sum(qs) * (1.0f / 64.0f) + 1e-5f);
  if (s.wave_ok && s.hb == 0) {
    if (mean_out != nullptr) mean_out[s.tok] = mean;
    if (rstd_out != nullptr) rstd_out[s.tok] = rstd;
  }
  if (pre != nullptr && (s.wave_ok || P::STAGES_OUTSIDE)) {      // (wave-uniform)
#pragma unroll
    for (int ot = 0; ot < 2; ot++) {
      float v[16];
#pragma unroll
      for (int q = 0; q < 16; q++) v[q] = acc[ot][q];
      P::emit(stg, v, j, s.hb, lane, pre, ld, ot, s.wave_ok, pre16);
    }
  }
#pragma unroll
  for (int ot = 0; ot < 2; ot++) {
    float v[16], ga[16], be[16];
    lds16f(gamma_lds + ot * 32 + 16 * s.hb, ga);
    lds16f(beta_lds + ot * 32 + 16 * s.hb, be);
#pragma unroll
    for (int q = 0; q < 16; q++) v[q] = (acc[ot][q] - mean) * rstd * ga[q] + be[q];
    P::emit(stg, v, j, s.hb, lane, y, ld, ot, s.wave_ok, false);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// C = epi(x . Wl^T + bias): K = 32 * K32, N = 32 * NT;  LN: N == 64 with dropout / residual / LayerNorm
// ---------------------------------------------------------------------------------------------------------------------
template <typename P, int K32, int NT, bool LN>
struct SmallCfg {
  static constexpr int KC = 2 * K32;
  static constexpr int WBYTES = KC * NT * P::PAIR_BYTES;
  static constexpr int PRM = NT * 32 + (LN ? 128 : 0);                 // bias | gamma | beta (floats)
  static constexpr int LDS = WBYTES + 4 * PRM + 4 * P::STAGE_BYTES;
};

template <typename P, int K32, int NT, bool LN, bool HR>
__device__ __forceinline__ void small_linear(const hftt_strip_desc& g, unsigned char* smem) {
  using Cfg = SmallCfg<P, K32, NT, LN>;
  constexpr int KC = Cfg::KC;
  static_assert(!LN || NT == 2, "LayerNorm form: N == 64");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const long nblk = ((long)g.M + 127) / 128;
  float* prm = reinterpret_cast<float*>(smem + Cfg::WBYTES);
  unsigned char* stg = smem + Cfg::WBYTES + 4 * Cfg::PRM + wave * P::STAGE_BYTES;
  const bool relu = g.flags & HFTT_SL_RELU;

  P::copy_weights(smem, g.w, KC * NT, tid);
  for (int i = tid; i < NT * 32; i += 256) prm[i] = g.bias != nullptr ? g.bias[i] : 0.f;
  if (LN && tid < 64) { prm[NT * 32 + tid] = g.ln_gamma[tid]; prm[NT * 32 + 64 + tid] = g.ln_beta[tid]; }
  __syncthreads();

  const uint32_t thr = hftt_keep_thr(g.drop_p);
  const float inv_keep = hftt_keep_scale(g.drop_p);
  const unsigned char* wl = smem + lane * 16;
  for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const SmallLane s = small_lane(blk, wave, j, h, g.M);
    const int hb = s.hb;
    typename P::Chunk xr[KC];
    P::load_strip(xr, g.x, s.tokc * g.ldx + 16 * hb);
    const long rrow = g.res_mod > 0 ? (long)((unsigned)s.tokc % (unsigned)g.res_mod) : s.tokc;
    const long roff = HR ? rrow * g.ldr + 16 * hb : 0;
    void* cwave = P::rows(g.C, s.row0 * g.ldc, false);
    const uint64_t rowq = ((uint64_t)s.tok * (uint64_t)g.N) >> 2;
    f32x16 lacc[LN ? 2 : 1];
#pragma unroll
    for (int t = 0; t < NT; t++) {
      f32x16 acc;
      small_bias(acc, prm + t * 32 + 16 * hb);
      float r[16];
      if (HR) P::load16(g.residual, roff + t * 32, false, r);
#pragma unroll
      for (int c = 0; c < KC; c++) P::tile_mac(wl, c * NT + t, xr[c], acc);
      float v[16];
#pragma unroll
      for (int q = 0; q < 16; q++) {
        float a = acc[q];
        if (!LN && relu) a = fmaxf(a, 0.f);
        v[q] = a * g.out_scale;
      }
      if (g.drop_p > 0.f) drop16(v, g.drop_seed, g.drop_site, rowq + ((t * 32 + 16 * hb) >> 2), thr, inv_keep);
      if (HR) {
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] += r[q];
      }
      if constexpr (LN) {
#pragma unroll
        for (int q = 0; q < 16; q++) lacc[t][q] = v[q];
      } else {
        P::emit(stg, v, j, hb, lane, cwave, g.ldc, t, s.wave_ok, false);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (LN) {
      const bool p16 = g.flags & HFTT_SL_PRE_BF16;
      small_ln_rows<P>(lacc, prm + NT * 32, prm + NT * 32 + 64, stg, j, lane, s, g.ln_mean, g.ln_rstd,
                       g.pre_ln_out != nullptr ? P::rows(g.pre_ln_out, s.row0 * g.ldc, p16) : nullptr, p16, cwave, g.ldc);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// fused two-GEMM block, d = 64, p = 128: mode 0 = FFN forward + residual + LayerNorm, mode 1 = dX half of its backward.  HH: the hidden (mode 0:
// h_out, mode 1: gate and h_out) is stored as bf16.  Weights: first matrix pairs (k chunk c of 4, hidden tile t of 4) at pair c * 4 + t,
// second matrix pairs (k chunk c of 8, output tile ot of 2) at pair 16 + c * 2 + ot; two workgroups per CU.
// ---------------------------------------------------------------------------------------------------------------------
template <typename P>
struct SmallMlpCfg {
  static constexpr int WBYTES = 32 * P::PAIR_BYTES;
  static constexpr int PRM = 128 + 64 + 128;                           // b1 | b2 | gamma | beta
  static constexpr int LDS = WBYTES + 4 * PRM + 4 * P::STAGE_BYTES;
};

template <typename P, int MODE, bool HH>
__device__ __forceinline__ void small_mlp(const hftt_ffn_desc& g, unsigned char* smem) {
  using Cfg = SmallMlpCfg<P>;
  constexpr int PT = 4, p = 128;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const long nblk = ((long)g.M + 127) / 128;
  float* prm = reinterpret_cast<float*>(smem + Cfg::WBYTES);
  unsigned char* stg = smem + Cfg::WBYTES + 4 * Cfg::PRM + wave * P::STAGE_BYTES;
  const bool has_res = (MODE == 1) && g.residual != nullptr;

  P::copy_weights(smem, g.w, 32, tid);
  if (tid < 128) prm[tid] = (MODE == 0 && g.b1 != nullptr) ? g.b1[tid] : 0.f;
  if (tid < 64) {
    prm[128 + tid] = (MODE == 0 && g.b2 != nullptr) ? g.b2[tid] : 0.f;
    if (MODE == 0) { prm[192 + tid] = g.ln_gamma[tid]; prm[256 + tid] = g.ln_beta[tid]; }
  }
  __syncthreads();

  const uint32_t thr = hftt_keep_thr(g.drop_p);
  const float inv_keep = hftt_keep_scale(g.drop_p);
  const unsigned char* wl = smem + lane * 16;
  for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const SmallLane s = small_lane(blk, wave, j, h, g.M);
    const int hb = s.hb;
    typename P::Chunk xr[4];
    P::load_strip(xr, g.x, s.tokc * g.ldx + 16 * hb);
    const uint64_t rowq_h = ((uint64_t)s.tok * (uint64_t)p) >> 2;
    void* hwave = P::rows(g.h_out, s.row0 * g.ldh, HH);
    f32x16 yacc[2];
#pragma unroll
    for (int ot = 0; ot < 2; ot++) small_bias(yacc[ot], prm + 128 + ot * 32 + 16 * hb);
#pragma unroll
    for (int t = 0; t < PT; t++) {
      // ---- first GEMM, hidden tile t ----
      f32x16 hacc;
      small_bias(hacc, prm + t * 32 + 16 * hb);
      float gcur[16];
      if (MODE == 1) P::load16(g.gate, s.tokc * g.ldg + t * 32 + 16 * hb, HH, gcur);
#pragma unroll
      for (int c = 0; c < 4; c++) P::tile_mac(wl, c * 4 + t, xr[c], hacc);
      // ---- middle epilogue: the lane's 16 hidden features of tile t become the B operand of the second GEMM ----
      float v[16];
      if (MODE == 0) {
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] = fmaxf(hacc[q], 0.f);
        if (g.drop_p > 0.f) drop16(v, g.drop_seed, g.site_h, rowq_h + ((t * 32 + 16 * hb) >> 2), thr, inv_keep);
      } else {
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] = gcur[q] > 0.f ? hacc[q] * g.gate_scale : 0.f;
      }
      typename P::Chunk hf[2];
      P::split16(v, hf);
      if (g.h_out != nullptr && (s.wave_ok || P::STAGES_OUTSIDE)) P::emit(stg, v, j, hb, lane, hwave, g.ldh, t, s.wave_ok, HH);      // (wave-uniform)
      // ---- second GEMM, K-slice t (chunks 2t, 2t + 1) ----
#pragma unroll
      for (int u = 0; u < 2; u++)
#pragma unroll
        for (int ot = 0; ot < 2; ot++) P::tile_mac(wl, 16 + (2 * t + u) * 2 + ot, hf[u], yacc[ot]);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---------------- final epilogue of the block ----------------
    const uint64_t rowq = ((uint64_t)s.tok * 64ull) >> 2;
    void* ywave = P::rows(g.y, s.row0 * g.ldy, false);
    const long roff = has_res ? s.tokc * g.ldr + 16 * hb : 0;
#pragma unroll
    for (int ot = 0; ot < 2; ot++) {
      float v[16];
#pragma unroll
      for (int q = 0; q < 16; q++) v[q] = yacc[ot][q];
      if (MODE == 0 && g.drop_p > 0.f) drop16(v, g.drop_seed, g.site_o, rowq + ((ot * 32 + 16 * hb) >> 2), thr, inv_keep);
      if (MODE == 0) {                                  // residual = the block input, still in the strip registers
        float r[16];
        P::values8(xr[2 * ot], r); P::values8(xr[2 * ot + 1], r + 8);
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] += r[q];
      } else if (has_res) {
        float r[16];
        P::load16(g.residual, roff + ot * 32, false, r);
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] += r[q];
      }
      if (MODE == 0) {
#pragma unroll
        for (int q = 0; q < 16; q++) yacc[ot][q] = v[q];
      } else {
        P::emit(stg, v, j, hb, lane, ywave, g.ldy, ot, s.wave_ok, false);
      }
    }
    if (MODE == 0) {
      const bool p16 = g.flags & HFTT_SL_PRE_BF16;
      small_ln_rows<P>(yacc, prm + 192, prm + 256, stg, j, lane, s, g.ln_mean, g.ln_rstd,
                       g.pre_ln_out != nullptr ? P::rows(g.pre_ln_out, s.row0 * g.ldy, p16) : nullptr, p16, ywave, g.ldy);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: a persistent grid over the 128-token blocks, and the shapes of the d = 64 model
// ---------------------------------------------------------------------------------------------------------------------
template <typename P, int K32, int NT, bool LN, bool HR>
int small_launch_linear(const hftt_strip_desc& d, hipStream_t st) {
  using Cfg = SmallCfg<P, K32, NT, LN>;
  const long grid = hftt_persistent_grid(P::LINEAR_WHAT, ((long)d.M + 127) / 128, P::wgs(Cfg::LDS));
  if (grid < 0) return 2;
  return P::template launch_linear<K32, NT, LN, HR>(dim3((unsigned)grid), Cfg::LDS, st, d);
}
template <typename P, int MODE, bool HH>
int small_launch_mlp(const hftt_ffn_desc& d, hipStream_t st) {
  const long grid = hftt_persistent_grid(P::MLP_WHAT, ((long)d.M + 127) / 128, 2);
  if (grid < 0) return 2;
  return P::template launch_mlp<MODE, HH>(dim3((unsigned)grid), SmallMlpCfg<P>::LDS, st, d);
}

// K x N: forward 64x192 (q, k, v), 64x128 (cross k, v), 64x64 (cross q; fc_o + LayerNorm), backward 64x64 (dX of fc_o, of the cross q),
// 192x64 / 128x64 (dX of the fused projections, + residual)
template <typename P>
int small_dispatch_linear(const hftt_strip_desc& d, hipStream_t st) {
  const int k32 = d.K / 32, nt = d.N / 32;
  const bool hr = d.residual != nullptr;
  if (d.ln_gamma != nullptr) {
    if (k32 == 2 && nt == 2) return hr ? small_launch_linear<P, 2, 2, true, true>(d, st) : small_launch_linear<P, 2, 2, true, false>(d, st);
  } else if (k32 == 2) {
    if (nt == 2) return hr ? small_launch_linear<P, 2, 2, false, true>(d, st) : small_launch_linear<P, 2, 2, false, false>(d, st);
    if (nt == 4 && !hr) return small_launch_linear<P, 2, 4, false, false>(d, st);
    if (nt == 6 && !hr) return small_launch_linear<P, 2, 6, false, false>(d, st);
  } else if (nt == 2) {
    if (k32 == 4) return hr ? small_launch_linear<P, 4, 2, false, true>(d, st) : small_launch_linear<P, 4, 2, false, false>(d, st);
    if (k32 == 6) return hr ? small_launch_linear<P, 6, 2, false, true>(d, st) : small_launch_linear<P, 6, 2, false, false>(d, st);
  }
  hftt_set_error("%s: shape N=%d K=%d%s is not covered (K x N in {64x64, 64x128, 64x192, 128x64, 192x64}; LayerNorm: 64x64)", P::LINEAR_WHAT, d.N, d.K,
                 d.ln_gamma != nullptr ? " with LayerNorm" : "");
  return 1;
}
