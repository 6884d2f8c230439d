// NT GEMM with fused epilogue on MFMA (gfx950).
//   C[M,N] = epi(A[M,K] . W[N,K]^T + bias)        -- see include/hftt_hip.h (hftt_gemm_nt)
// Tile: BM=128 x BN in {64,128,256} x BK=32, 512 threads (8 waves, 2 per SIMD), double-buffered LDS,
// register-staged global->LDS.
//   npass == 1 ("bf16"):  fp32 activations are rounded to bf16 on the way into LDS, weights come as a prepared bf16
//                         plane; v_mfma_f32_32x32x16_bf16; LDS rows padded to 80 B (conflict-free ds_read_b128).
//   npass == 3 ("parity"): operands stay fp32 in LDS (rows of 33 floats: conflict-free ds_read_b32), weights come as a
//                         prepared fp32 matrix; v_mfma_f32_32x32x2_f32 = exact fp32 FMA chains (<= 1e-3 parity mode).
// bf16 mode with N a multiple of 256 and K <= 768 takes the A-stationary kernel further down (gemm_nt_as1_kernel), the split modes with
// N <= 256 and K <= 256 theirs (gemm_nt_as3_kernel); both and the split modes' full tiles finish their rows in one shared row pass (row_pass).
#include <cstdlib>
#include <type_traits>
#include "hftt_common.h"
#include "x3_common.h"
#include "hftt_launch.h"
#include "../../include/hftt_hip.h"

namespace {

// gate value > 0 for an fp32 or a bf16 gate tensor (4 consecutive elements at element offset `off`)
__device__ __forceinline__ float4 load_gate4(const float* gate, bool bf, long off) {
  if (bf) {
    const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(gate) + off);
    return make_float4(bf2f(u.x & 0xFFFFu), bf2f(u.x >> 16), bf2f(u.y & 0xFFFFu), bf2f(u.y >> 16));
  }
  return *reinterpret_cast<const float4*>(gate + off);
}
// store 4 consecutive outputs as fp32 (16 B) or bf16 (8 B)
__device__ __forceinline__ void store_c4(float* C, bool bf, long off, float a, float b, float c, float d) {
  if (bf) {
    uint2 u;
    u.x = f2bf(a) | ((unsigned)f2bf(b) << 16); u.y = f2bf(c) | ((unsigned)f2bf(d) << 16);
    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(C) + off) = u;
  } else {
    *reinterpret_cast<float4*>(C + off) = make_float4(a, b, c, d);
  }
}

// Row pass: finishes the rows of a staged 256-column tile (stage[row_l * ld + col_l], rows m0 .., columns n0 ..) -- one wave per row, 16 B
// per lane: table add, gate, dropout, residual, LayerNorm, one 16-byte (bf16: 8-byte) store.  Each wave takes RPW rows, RB at a time: all
// table / gate / residual loads of the RB rows are issued (from a clamped row: the wave-uniform pointer tests are the only branches), then
// the arithmetic runs.  Dropout hashes once per quad: col % 4 == 0 and N % 4 == 0 here, so element e of the quad is byte e of that hash.
//   BF     gate, residual and C may be stored as bf16 (io_flags)
//   LNORM  LayerNorm where g.ln_gamma is set (N == 256: the row is complete)
//   col_ok this lane's four columns exist (always where N % 256 == 0)
template <int RPW, int RB, bool BF, bool LNORM>
__device__ __forceinline__ void row_pass(const hftt_gemm_nt_desc g, const long m0, const int n0, const float* stage, const int ld, const bool col_ok,
                                         const uint32_t thr, const float inv_keep) {
  static_assert(RPW % RB == 0, "whole groups of rows");
  // The bf16 forms add the table / residual registers even when no tensor was loaded into them (zeros: a -0 of the stage leaves as +0);
  // the fp32 form adds only what exists (a -0 stays).  Kept apart from BF: it is a property of the results, not of the storage.
  constexpr bool ADD_ZEROS = BF;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool c_bf = BF && (g.io_flags & HFTT_NT_C_BF16), gate_bf = BF && (g.io_flags & HFTT_NT_GATE_BF16), res_bf = BF && (g.io_flags & HFTT_NT_RES_BF16);
  const bool ln = LNORM && g.ln_gamma != nullptr;
  const int c4 = n0 + lane * 4;
  float4 ga = make_float4(1.f, 1.f, 1.f, 1.f), be = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ln) {
    ga = *reinterpret_cast<const float4*>(g.ln_gamma + c4);
    be = *reinterpret_cast<const float4*>(g.ln_beta + c4);
  }
#pragma unroll 1
  for (int rb = 0; rb < RPW; rb += RB) {
    if (RB == 1 && m0 + wave * RPW + rb >= g.M) break;      // (wave-uniform) this row and every later one lie past M
    float4 tab[RB], gat[RB], res[RB];
#pragma unroll
    for (int rr = 0; rr < RB; rr++) {
      const long row = m0 + wave * RPW + rb + rr;
      tab[rr] = make_float4(0.f, 0.f, 0.f, 0.f); gat[rr] = tab[rr]; res[rr] = tab[rr];
      const long rc = row < g.M ? row : (long)g.M - 1;
      if (col_ok) {
        if (g.add_table != nullptr) tab[rr] = *reinterpret_cast<const float4*>(g.add_table + (long)(rc % g.add_mod) * g.N + c4);
        if (g.gate != nullptr) gat[rr] = load_gate4(g.gate, gate_bf, rc * g.ldg + c4);
        if (g.residual != nullptr) res[rr] = load_gate4(g.residual, res_bf, (long)(rc % g.res_mod) * g.ldr + c4);
      }
    }
#pragma unroll
    for (int rr = 0; rr < RB; rr++) {
      const int row_l = wave * RPW + rb + rr;
      const long row = m0 + row_l;
      if (row < g.M && col_ok) {         // (row: wave-uniform)
        const float4 sv = *reinterpret_cast<const float4*>(stage + row_l * ld + lane * 4);
        float v[4] = {sv.x, sv.y, sv.z, sv.w};
        if (ADD_ZEROS || g.add_table != nullptr) { v[0] += tab[rr].x; v[1] += tab[rr].y; v[2] += tab[rr].z; v[3] += tab[rr].w; }
        if (g.gate != nullptr) {
          v[0] = gat[rr].x > 0.f ? v[0] * g.gate_scale : 0.f; v[1] = gat[rr].y > 0.f ? v[1] * g.gate_scale : 0.f;
          v[2] = gat[rr].z > 0.f ? v[2] * g.gate_scale : 0.f; v[3] = gat[rr].w > 0.f ? v[3] * g.gate_scale : 0.f;
        }
        if (g.drop_p > 0.f) {
          const uint32_t k4 = hftt_keep_quad(g.drop_seed, g.drop_site, ((uint64_t)row * (uint64_t)g.N + (uint64_t)c4) >> 2, thr);
#pragma unroll
          for (int e = 0; e < 4; e++) v[e] = ((k4 >> e) & 1u) ? v[e] * inv_keep : 0.f;
        }
        if (ADD_ZEROS || g.residual != nullptr) { v[0] += res[rr].x; v[1] += res[rr].y; v[2] += res[rr].z; v[3] += res[rr].w; }
        if (ln) {
          const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / 256);
          float q = 0.f;
#pragma unroll
          for (int e = 0; e < 4; e++) { const float dlt = v[e] - mean; q += dlt * dlt; }
          const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / 256) + 1e-5f);
          if (g.pre_ln_out != nullptr) *reinterpret_cast<float4*>(g.pre_ln_out + row * g.ldc + c4) = make_float4(v[0], v[1], v[2], v[3]);
          v[0] = (v[0] - mean) * rstd * ga.x + be.x; v[1] = (v[1] - mean) * rstd * ga.y + be.y;
          v[2] = (v[2] - mean) * rstd * ga.z + be.z; v[3] = (v[3] - mean) * rstd * ga.w + be.w;
          if (lane == 0) {
            if (g.ln_mean != nullptr) g.ln_mean[row] = mean;
            if (g.ln_rstd != nullptr) g.ln_rstd[row] = rstd;
          }
        }
        store_c4(g.C, c_bf, row * g.ldc + c4, v[0], v[1], v[2], v[3]);
      }
    }
  }
}

constexpr int BM = 128;
constexpr int BK = 32;

// PREC: 1 = bf16 operands, 3 = exact fp32 MFMA, 2 / 4 = split operands in three passes (x3_common.h: fp16 / bf16 halves; the A tile
// is split on its way into LDS, the weights arrive as two prepared 16-bit planes W / W_lo)
template <int BN, int PREC>
struct NtCfg {
  static constexpr bool F32 = (PREC == 3);
  static constexpr bool X3M = (PREC == 2 || PREC == 4 || PREC == 5);   // 5 = npass 4 with HFTT_NT_A_HI: A (a gradient) enters as its bf16 rounding
  static constexpr int WM = (BN == 64) ? 4 : 2;
  static constexpr int WN = 8 / WM;
  static constexpr int TM = BM / WM / 32;
  static constexpr int TN = BN / WN / 32;
  static constexpr int RS = F32 ? 33 : 40;                 // row stride in elements (floats / bf16)
  static constexpr int ESZ = F32 ? 4 : 2;
  static constexpr int PLANES = X3M ? 2 : 1;               // x3: hi plane, then lo plane
  static constexpr int A_ELEMS = PLANES * BM * RS;
  static constexpr int W_ELEMS = PLANES * BN * RS;
  static constexpr int BUF_ELEMS = A_ELEMS + W_ELEMS;
  static constexpr int LOOP_BYTES = 2 * BUF_ELEMS * ESZ;
  static constexpr int STAGE_LD = BN + 4;
  static constexpr int STAGE_BYTES = BM * STAGE_LD * 4;
  static constexpr int WCHP = (BN * 4 + 511) / 512;        // 16-byte chunks per thread of one 16-bit weight plane
  static constexpr int WCH = F32 ? (BN * 8 + 511) / 512 : PLANES * WCHP;   // 16-byte weight chunks per thread
};

template <int BN, int PREC, bool LN>
__global__ __launch_bounds__(512) void gemm_nt_kernel(const hftt_gemm_nt_desc g) {
  using Cfg = NtCfg<BN, PREC>;
  constexpr bool F32 = Cfg::F32, X3M = Cfg::X3M;
  constexpr int XE = X3M ? (PREC == 5 ? 4 : PREC) : X3_BF16;          // element type of the split (unused otherwise)
  constexpr bool AH = (PREC == 5);
  constexpr int WN = Cfg::WN, TM = Cfg::TM, TN = Cfg::TN, RS = Cfg::RS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned short* sm16 = reinterpret_cast<unsigned short*>(smem);
  float* sm32 = reinterpret_cast<float*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int nk = g.K / BK;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  float4 areg[2];
  uint4 abreg = make_uint4(0u, 0u, 0u, 0u);        // A tile chunk when A is stored as bf16 (16 B = 8 elements per thread)
  const bool a_bf = !F32 && !X3M && (g.io_flags & HFTT_NT_A_BF16);
  const bool c_bf = !F32 && !X3M && (g.io_flags & HFTT_NT_C_BF16);
  const bool gate_bf = !F32 && !X3M && (g.io_flags & HFTT_NT_GATE_BF16);
  uint4 wreg[Cfg::WCH];
#pragma unroll
  for (int j = 0; j < Cfg::WCH; j++) wreg[j] = make_uint4(0u, 0u, 0u, 0u);
  const float* Wf = reinterpret_cast<const float*>(g.W);
  const unsigned short* Wb = reinterpret_cast<const unsigned short*>(g.W);
  const unsigned short* Wlo = reinterpret_cast<const unsigned short*>(g.W_lo);

  auto gload = [&](int kt) {
    const int k0 = kt * BK;
    if (a_bf) {
      const int row = tid >> 2, ch = tid & 3;
      const long grow = m0 + row;
      const long gr = grow < g.M ? grow : (long)g.M - 1;
      const uint4 t = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(g.A) + gr * g.lda + k0 + ch * 8);
      abreg = grow < g.M ? t : make_uint4(0u, 0u, 0u, 0u);
    } else
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int i = tid + 512 * j;
      const int row = i >> 3, c4 = i & 7;
      const long grow = m0 + row;
      // unconditional load from a clamped row + select (a branch around the load makes hipcc serialise the loads)
      const long gr = grow < g.M ? grow : (long)g.M - 1;
      const float4 t = *reinterpret_cast<const float4*>(g.A + gr * g.lda + k0 + c4 * 4);
      areg[j] = grow < g.M ? t : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < Cfg::WCH; j++) {
      const int i = tid + 512 * j;
      if (F32) {
        if (i < BN * 8) {
          const int row = i >> 3, ch = i & 7;
          wreg[j] = *reinterpret_cast<const uint4*>(Wf + (long)(n0 + row) * g.K + k0 + ch * 4);
        }
      } else if (X3M) {
        const int pl = j / Cfg::WCHP, ip = tid + 512 * (j % Cfg::WCHP);
        if (ip < BN * 4) {
          const int row = ip >> 2, ch = ip & 3;
          wreg[j] = *reinterpret_cast<const uint4*>((pl ? Wlo : Wb) + (long)(n0 + row) * g.K + k0 + ch * 8);
        }
      } else {
        if (i < BN * 4) {
          const int row = i >> 2, ch = i & 3;
          wreg[j] = *reinterpret_cast<const uint4*>(Wb + (long)(n0 + row) * g.K + k0 + ch * 8);
        }
      }
    }
  };
  auto sstore = [&](int buf) {
    if (F32) {
      float* As = sm32 + buf * Cfg::BUF_ELEMS;
      float* Ws = As + Cfg::A_ELEMS;
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int i = tid + 512 * j;
        const int row = i >> 3, c4 = i & 7;
        float* d = As + row * RS + c4 * 4;
        d[0] = areg[j].x; d[1] = areg[j].y; d[2] = areg[j].z; d[3] = areg[j].w;
      }
#pragma unroll
      for (int j = 0; j < Cfg::WCH; j++) {
        const int i = tid + 512 * j;
        if (i < BN * 8) {
          const int row = i >> 3, ch = i & 7;
          float* d = Ws + row * RS + ch * 4;
          d[0] = __uint_as_float(wreg[j].x); d[1] = __uint_as_float(wreg[j].y);
          d[2] = __uint_as_float(wreg[j].z); d[3] = __uint_as_float(wreg[j].w);
        }
      }
    } else if (X3M) {
      unsigned short* As = sm16 + buf * Cfg::BUF_ELEMS;
      unsigned short* Ws = As + Cfg::A_ELEMS;
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int i = tid + 512 * j;
        const int row = i >> 3, c4 = i & 7;
        uint2 hi, lo;
        x3_split4<XE>(areg[j], hi, lo);
        *reinterpret_cast<uint2*>(As + row * RS + c4 * 4) = hi;
        if (!AH) *reinterpret_cast<uint2*>(As + BM * RS + row * RS + c4 * 4) = lo;
      }
#pragma unroll
      for (int j = 0; j < Cfg::WCH; j++) {
        const int pl = j / Cfg::WCHP, ip = tid + 512 * (j % Cfg::WCHP);
        if (ip < BN * 4) {
          const int row = ip >> 2, ch = ip & 3;
          *reinterpret_cast<uint4*>(Ws + pl * BN * RS + row * RS + ch * 8) = wreg[j];
        }
      }
    } else {
      unsigned short* As = sm16 + buf * Cfg::BUF_ELEMS;
      unsigned short* Ws = As + Cfg::A_ELEMS;
      if (a_bf) {
        *reinterpret_cast<uint4*>(As + (tid >> 2) * RS + (tid & 3) * 8) = abreg;
      } else
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int i = tid + 512 * j;
        const int row = i >> 3, c4 = i & 7;
        uint2 ph;
        ph.x = f2bf(areg[j].x) | ((unsigned)f2bf(areg[j].y) << 16);
        ph.y = f2bf(areg[j].z) | ((unsigned)f2bf(areg[j].w) << 16);
        *reinterpret_cast<uint2*>(As + row * RS + c4 * 4) = ph;
      }
#pragma unroll
      for (int j = 0; j < Cfg::WCH; j++) {
        const int i = tid + 512 * j;
        if (i < BN * 4) {
          const int row = i >> 2, ch = i & 3;
          *reinterpret_cast<uint4*>(Ws + row * RS + ch * 8) = wreg[j];
        }
      }
    }
  };

  gload(0);
  sstore(0);
  __syncthreads();

  for (int kt = 0; kt < nk; kt++) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
    if (F32) {
      const float* As = sm32 + buf * Cfg::BUF_ELEMS;
      const float* Ws = As + Cfg::A_ELEMS;
      // Two-level summation: the 32 k values of a stage are accumulated from zero (16 MFMA steps), then added to the running sum -- a
      // chain of 16 + K/32 roundings instead of K/2.  One running accumulator over K = 256 measured 1.35x (rms) / 2x (max) the error of a
      // CPU sgemm on the first encoder layer's Q / K projections (|x| ~ 600), and those feed logits of ~1e5 whose near-ties decide the
      // first layer's gradients (tests/dev_layer_diff.py).
      f32x16 part[TM][TN];
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
          for (int r = 0; r < 16; r++) part[i][j][r] = 0.f;
#pragma unroll
      for (int t = 0; t < 16; t++) {
        float a[TM], b[TN];
#pragma unroll
        for (int i = 0; i < TM; i++) a[i] = As[(wm * TM * 32 + i * 32 + lr) * RS + 16 * lh + t];
#pragma unroll
        for (int j = 0; j < TN; j++) b[j] = Ws[(wn * TN * 32 + j * 32 + lr) * RS + 16 * lh + t];
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
          for (int j = 0; j < TN; j++) part[i][j] = mfma32_f32(a[i], b[j], part[i][j]);
      }
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) acc[i][j] += part[i][j];
    } else if (X3M) {
      const unsigned short* As = sm16 + buf * Cfg::BUF_ELEMS;
      const unsigned short* Ws = As + Cfg::A_ELEMS;
#pragma unroll
      for (int s = 0; s < 2; s++) {
        bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
        for (int i = 0; i < TM; i++) {
          const unsigned short* p = As + (wm * TM * 32 + i * 32 + lr) * RS + s * 16 + lh * 8;
          ah[i] = lds_read_b128(p);
          if (!AH) al[i] = lds_read_b128(p + BM * RS);
        }
#pragma unroll
        for (int j = 0; j < TN; j++) {
          const unsigned short* p = Ws + (wn * TN * 32 + j * 32 + lr) * RS + s * 16 + lh * 8;
          bh[j] = lds_read_b128(p); bl[j] = lds_read_b128(p + BN * RS);
        }
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
          for (int j = 0; j < TN; j++) {
            if (AH) { acc[i][j] = X3<XE>::mma(ah[i], bl[j], acc[i][j]); acc[i][j] = X3<XE>::mma(ah[i], bh[j], acc[i][j]); }
            else acc[i][j] = x3_mma<XE>(ah[i], al[i], bh[j], bl[j], acc[i][j]);
          }
      }
    } else {
      const unsigned short* As = sm16 + buf * Cfg::BUF_ELEMS;
      const unsigned short* Ws = As + Cfg::A_ELEMS;
#pragma unroll
      for (int s = 0; s < 2; s++) {
        bf16x8 a[TM], b[TN];
#pragma unroll
        for (int i = 0; i < TM; i++) a[i] = lds_read_b128(As + (wm * TM * 32 + i * 32 + lr) * RS + s * 16 + lh * 8);
#pragma unroll
        for (int j = 0; j < TN; j++) b[j] = lds_read_b128(Ws + (wn * TN * 32 + j * 32 + lr) * RS + s * 16 + lh * 8);
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
          for (int j = 0; j < TN; j++) acc[i][j] = mfma32(a[i], b[j], acc[i][j]);
      }
    }
    if (kt + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }

  // ------------------------------- epilogue -------------------------------
  const uint32_t thr = hftt_keep_thr(g.drop_p);
  const float inv_keep = hftt_keep_scale(g.drop_p);
  float* stage = reinterpret_cast<float*>(smem);
  // Split modes, full 256-column tiles: the fp32 result leaves through LDS as whole rows (one wave per row, 16 bytes per lane) and the
  // table add / gate / dropout / residual run there per QUAD of columns.  From the accumulator layout every element paid its own
  // `row % add_mod`, its own hash and a 4-byte store: the embedding GEMM (K = 96, all epilogue) took 440 us for 268 MB at S_e.
  const bool rowpass = X3M && !LN && BN == 256 && (g.N % 4 == 0) && (g.ldc % 4 == 0) && (g.gate == nullptr || g.ldg % 4 == 0) &&
                       (g.residual == nullptr || g.ldr % 4 == 0) && ((((uintptr_t)g.C | (uintptr_t)g.gate | (uintptr_t)g.residual | (uintptr_t)g.add_table) & 15) == 0);

#pragma unroll
  for (int i = 0; i < TM; i++) {
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int col_l = wn * TN * 32 + j * 32 + lr;
      const int col = n0 + col_l;
      const bool col_ok = col < g.N;
      const float bv = (g.bias != nullptr && col_ok) ? g.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row_l = wm * TM * 32 + i * 32 + acc_row32(r, lh);
        const long row = m0 + row_l;
        const bool ok = col_ok && row < g.M;
        float v = acc[i][j][r] + bv;
        if (g.act == 1) v = fmaxf(v, 0.f);
        v *= g.out_scale;
        if (rowpass) { stage[row_l * Cfg::STAGE_LD + col_l] = v; continue; }      // (wave-uniform)
        if (ok) {
          if (g.add_table != nullptr) v += g.add_table[(long)(row % g.add_mod) * g.N + col];
          if (g.gate != nullptr) {
            const float gv = gate_bf ? bf2f(reinterpret_cast<const unsigned short*>(g.gate)[row * g.ldg + col]) : g.gate[row * g.ldg + col];
            v = (gv > 0.f) ? v * g.gate_scale : 0.f;
          }
          if (g.drop_p > 0.f) v = hftt_keep(g.drop_seed, g.drop_site, (uint64_t)row * g.N + col, thr) ? v * inv_keep : 0.f;
          if (g.residual != nullptr) v += g.residual[(long)(row % g.res_mod) * g.ldr + col];
        }
        if (LN) {
          stage[row_l * Cfg::STAGE_LD + col_l] = v;
        } else if (ok) {
          if (c_bf) reinterpret_cast<unsigned short*>(g.C)[row * g.ldc + col] = f2bf(v);
          else g.C[row * g.ldc + col] = v;
        }
      }
    }
  }

  if (rowpass) {
    __syncthreads();
    row_pass<BM / 8, 1, false, false>(g, m0, n0, stage, Cfg::STAGE_LD, n0 + lane * 4 < g.N, thr, inv_keep);
  }

  if (LN) {
    __syncthreads();
    constexpr int VPL = BN / 64;
    for (int rr = 0; rr < BM / 8; rr++) {
      const int row_l = wave * (BM / 8) + rr;
      const long row = m0 + row_l;
      if (row >= g.M) break;   // wave-uniform
      float v[VPL];
#pragma unroll
      for (int e = 0; e < VPL; e++) v[e] = stage[row_l * Cfg::STAGE_LD + lane * VPL + e];
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < VPL; e++) s += v[e];
      const float mean = wave_sum(s) * (1.0f / BN);
      float q = 0.f;
#pragma unroll
      for (int e = 0; e < VPL; e++) { const float dlt = v[e] - mean; q += dlt * dlt; }
      const float var = wave_sum(q) * (1.0f / BN);
      const float rstd = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
      for (int e = 0; e < VPL; e++) {
        const int col = lane * VPL + e;
        if (g.pre_ln_out != nullptr) g.pre_ln_out[row * g.ldc + col] = v[e];
        g.C[row * g.ldc + col] = (v[e] - mean) * rstd * g.ln_gamma[col] + g.ln_beta[col];
      }
      if (lane == 0) {
        if (g.ln_mean != nullptr) g.ln_mean[row] = mean;
        if (g.ln_rstd != nullptr) g.ln_rstd[row] = rstd;
      }
    }
  }
}

// A block of the A-stationary form: BM_ rows x K of A (row-major) -> bf16 in LDS (row stride RSA), every load of up to 8 chunks per thread
// in flight before the first LDS write.  CH is the 16-byte chunk as it is stored: uint4 = 8 bf16, copied; float4 = 4 fp32, rounded to bf16.
// Thread t owns chunks t, t + 512, ... of the block; (row, chunk) advance incrementally -- one integer division per thread instead of one
// per load (the index math was ~20 % of the kernel's VALU time).  Rows past M or past the block read a clamped address and become zeros:
// the loads stay unconditional (no branch, no early vmcnt wait).
// The walk itself: (row, chunk) of this thread's next chunk of a block with cpr chunks per row.
struct AWalk {
  int cpr, drow, dch, row, ch;
  __device__ __forceinline__ AWalk(int cpr_) : cpr(cpr_), drow(512 / cpr_), dch(512 - (512 / cpr_) * cpr_) {
    row = threadIdx.x / cpr; ch = threadIdx.x - row * cpr;
  }
  __device__ __forceinline__ void next() {
    row += drow; ch += dch;
    if (ch >= cpr) { ch -= cpr; row++; }
  }
};
// The loads of the next NCH chunks of the walk, all issued, none waited for (the split form keeps them in flight under its MFMA loop).  A chunk
// past M or past the block reads a clamped row and is NOT zeroed here: a select on the loaded value makes hipcc branch around the load and wait
// for each one in turn.  a_chunk_live() says at the LDS write whether the chunk counts.
template <int BM_, typename CH, int NCH>
__device__ __forceinline__ void a_block_issue(const hftt_gemm_nt_desc& g, const long m0, AWalk& w, CH (&v)[NCH]) {
  constexpr bool ABF = std::is_same<CH, uint4>::value;
  using T = typename std::conditional<ABF, unsigned short, float>::type;
  constexpr int E = 16 / sizeof(T);                // elements per chunk
  const T* A = reinterpret_cast<const T*>(g.A);
#pragma unroll
  for (int u = 0; u < NCH; u++) {
    const long grow = m0 + w.row;
    const long gr = (w.row < BM_ && grow < g.M) ? grow : (m0 < g.M ? m0 : 0);
    v[u] = *reinterpret_cast<const CH*>(A + gr * g.lda + w.ch * E);
    w.next();
  }
}
template <int BM_>
__device__ __forceinline__ bool a_chunk_live(const hftt_gemm_nt_desc& g, const long m0, const AWalk& w) { return w.row < BM_ && m0 + w.row < g.M; }
template <int BM_, typename CH>
__device__ __forceinline__ void load_a_block(const hftt_gemm_nt_desc g, const long m0, unsigned short* As, const int RSA) {
  constexpr bool ABF = std::is_same<CH, uint4>::value;
  AWalk w(g.K / (ABF ? 8 : 4));
  const int total = BM_ * w.cpr;
  for (int base = 0; base < total; base += 512 * 8) {
    CH v[8];
    AWalk at = w;
    a_block_issue<BM_, CH, 8>(g, m0, w, v);
#pragma unroll
    for (int u = 0; u < 8; u++) {
      if (at.row < BM_) {
        // (fp32: the address as chunk pair + half -- with row * RSA + ch * 4 hipcc keeps fewer loads in flight)
        unsigned short* dst = ABF ? As + at.row * RSA + (at.ch << 3) : As + at.row * RSA + ((at.ch >> 1) << 3) + (at.ch & 1) * 4;
        const bool live = a_chunk_live<BM_>(g, m0, at);
        if constexpr (ABF) {
          *reinterpret_cast<uint4*>(dst) = live ? v[u] : make_uint4(0u, 0u, 0u, 0u);
        } else {
          typedef __bf16 bf4_t __attribute__((ext_vector_type(4)));
          const f32x4 fv = {live ? v[u].x : 0.f, live ? v[u].y : 0.f, live ? v[u].z : 0.f, live ? v[u].w : 0.f};
          *reinterpret_cast<uint2*>(dst) = __builtin_bit_cast(uint2, __builtin_convertvector(fv, bf4_t));
        }
      }
      at.next();
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// bf16 mode, A-stationary form (N a multiple of 256, K <= 768).  These GEMMs are tall and short-K (M ~ 10^5 tokens): a
// streaming kernel with the MFMA work hidden underneath.  One workgroup per BM-row block; the block of A is read from HBM
// ONCE regardless of N (all loads in flight), rounded to bf16 and kept in LDS; the (L2-resident) weight tiles stream
// through a double-buffered LDS ring shared by the 8 waves (a per-wave L2 -> register stream was measured 30 % slower:
// twice the L2 traffic in 32-byte pieces).
//   MODE 0  plain (bias / ReLU / scale): stores straight from the accumulators;
//   MODE 1  staged, single N tile (N == 256): tile -> LDS -> row_pass() (direct 4-byte stores from the accumulator layout
//           were measured at 2.8 TB/s; the staged 16-byte form reaches > 4 TB/s);
//   MODE 2  staged, several N tiles (BM = 32): the same row pass per N tile, staged in the weight ring.
// ------------------------------------------------------------------------------------------------------------------
// Waves per SIMD: at least 4 (128 VGPRs), and for the staged forms at most 4 -- their row pass holds ~100 VGPRs or more, so a fifth wave
// is not to be had, and a scheduler left to hope for one (it cannot see the dynamic LDS either) gives up the k loop's overlap of the
// LDS reads with the MFMAs for it: every MFMA of a step's first half then waits for lgkmcnt(0), measured +3 % at N = K = 256 with LayerNorm.
template <int BM_, int MODE, bool EW = false, int PF = 1>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, MODE == 0 ? 8 : 4))) void gemm_nt_as1_kernel(const hftt_gemm_nt_desc g) {
  constexpr int BN = 256;
  constexpr int WM = (BM_ == 32) ? 1 : 2;
  constexpr int WN = 8 / WM;
  constexpr int TN = BN / (32 * WN);
  static_assert(BM_ == 32 * WM, "one 32-row MFMA tile per wave row");
  constexpr int RSW = 40;
  constexpr int W_ELEMS = BN * RSW;
  constexpr int WCH = 2;
  constexpr int STAGE_LD = BN + 4;
  static_assert(MODE != 2 || BM_ * STAGE_LD * 4 <= 2 * W_ELEMS * 2, "stage must fit the weight ring");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int K = g.K;
  const int RSA = K + 8;
  unsigned short* As = reinterpret_cast<unsigned short*>(smem);
  unsigned short* Ws = As + BM_ * RSA;
  float* stage = (MODE == 2) ? reinterpret_cast<float*>(Ws) : reinterpret_cast<float*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const long m0 = (long)blockIdx.x * BM_;
  const int KT = K / 32;
  const int NT = (g.N + BN - 1) / BN;
  const int steps = NT * KT;
  const unsigned short* Wb = reinterpret_cast<const unsigned short*>(g.W);

  // weight tiles travel global -> registers -> LDS ring; the global load of tile s + PF is issued at step s into one of PF
  // register sets, so an L2 round trip (~700 ns) has PF steps of MFMA work to hide behind
  uint4 wr[PF][WCH];
#pragma unroll
  for (int i = 0; i < PF; i++)
#pragma unroll
    for (int j = 0; j < WCH; j++) wr[i][j] = make_uint4(0u, 0u, 0u, 0u);
  auto wload = [&](uint4 (&w)[WCH], int s) {
    const int nt = s / KT, kt = s - nt * KT;
#pragma unroll
    for (int j = 0; j < WCH; j++) {
      const int i = tid + 512 * j;
      const int row = i >> 2, ch = i & 3;
      w[j] = *reinterpret_cast<const uint4*>(Wb + (long)(nt * BN + row) * K + kt * 32 + ch * 8);
    }
  };
  auto wstore = [&](const uint4 (&w)[WCH], int buf) {
#pragma unroll
    for (int j = 0; j < WCH; j++) {
      const int i = tid + 512 * j;
      const int row = i >> 2, ch = i & 3;
      *reinterpret_cast<uint4*>(Ws + buf * W_ELEMS + row * RSW + ch * 8) = w[j];
    }
  };
#pragma unroll
  for (int i = 0; i < PF; i++) wload(wr[i], i < steps ? i : steps - 1);
  const bool c_bf = g.io_flags & HFTT_NT_C_BF16;
  if (g.io_flags & HFTT_NT_A_BF16) load_a_block<BM_, uint4>(g, m0, As, RSA);
  else load_a_block<BM_, float4>(g, m0, As, RSA);
  wstore(wr[0], 0);
  __syncthreads();

  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[j][r] = 0.f;

  const uint32_t thr = hftt_keep_thr(g.drop_p);
  const float inv_keep = hftt_keep_scale(g.drop_p);

  // per k step u of an unrolled group of PF (so the register sets are named statically; PF must divide K / 32): set u held tile s
  // (already in the ring) and receives tile s + PF; set u + 1 holds tile s + 1, written to the ring once this step's MFMAs are issued
  constexpr int U = PF;
  int s = 0;
  for (int nt = 0; nt < NT; nt++) {
    for (int kt0 = 0; kt0 < KT; kt0 += U) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int kt = kt0 + u;
        uint4 (&wl)[WCH] = wr[u];
        const uint4 (&wnext)[WCH] = wr[(u + 1) % PF];
        const int buf = (U % 2 == 0) ? (u & 1) : (s & 1);
        // unconditional (index clamped to the last tile): a load inside a conditional block makes hipcc's s_waitcnt insertion
        // fall back to vmcnt(0) at the ring write, which would drain the younger prefetch too
        wload(wl, s + PF < steps ? s + PF : steps - 1);
        const unsigned short* Wt = Ws + buf * W_ELEMS;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
          const bf16x8 a = lds_read_b128(As + (wm * 32 + lr) * RSA + kt * 32 + ks * 16 + lh * 8);
#pragma unroll
          for (int j = 0; j < TN; j++) {
            const bf16x8 b = lds_read_b128(Wt + (wn * TN * 32 + j * 32 + lr) * RSW + ks * 16 + lh * 8);
            acc[j] = mfma32(a, b, acc[j]);
          }
        }
        const bool tile_end = (kt == KT - 1);
        if (MODE == 0) wstore(wnext, buf ^ 1);            // past the last tile this rewrites a dead buffer
        else if (!tile_end && s + 1 < steps) wstore(wnext, buf ^ 1);
        if (!tile_end) {
          __syncthreads();
          s++;
        }
      }
    }
    {                                  // N tile finished: s = its last step, tile s + 1 (if any) sits in set 0
      const int buf = s & 1;
      const int n0 = nt * BN;
      if (MODE != 0) __syncthreads();
      if (MODE == 0 && c_bf) {
        // bf16 C straight from the accumulators: lanes 2i / 2i+1 hold adjacent columns and every lane two rows per register pair;
        // pair_rows_to_cols() (cvt_pk + DPP + byte permute) gives each lane one packed pair of adjacent columns = one 4-byte store.
        // Instruction count matters here: the VALU, not HBM, was the busiest unit of this kernel (SQ_ACTIVE_INST_VALU ~ 48 %).
        const bool odd = lane & 1;
        unsigned short* Cb = reinterpret_cast<unsigned short*>(g.C);
        const float lo_clamp = (g.act == 1) ? 0.f : -INFINITY;
        const bool gated = EW && g.gate != nullptr;
        const float oscale = gated ? g.out_scale * g.gate_scale : g.out_scale;
        auto tile_out = [&](auto full_c) {
          constexpr bool FULL = decltype(full_c)::value;       // every row of the block is inside M: no per-store bounds test
#pragma unroll
          for (int j = 0; j < TN; j++) {
            const int col = n0 + wn * TN * 32 + j * 32 + lr;
            const float bv = (g.bias != nullptr) ? g.bias[col] : 0.f;
            unsigned rbase = (unsigned)(wm * 32 + 4 * lh);
            asm volatile("" : "+v"(rbase));       // opaque: keeps the per-row address / index terms from being hoisted out of the k loop
            const uint64_t ebase = (uint64_t)(m0 + rbase) * (unsigned)g.N + (unsigned)col;
            const long row0 = m0 + rbase + (odd ? 1 : 0);
            const long row0c = FULL ? row0 : (row0 < g.M ? row0 : (long)g.M - 1);
            unsigned short* cp = Cb + row0 * g.ldc + (col & ~1);
            const unsigned short* gpt = reinterpret_cast<const unsigned short*>(g.gate) + row0c * g.ldg + (col & ~1);
            unsigned gpk[8];
            if (gated) {                     // all eight gate pairs of this column block in flight before the first one is used
#pragma unroll
              for (int rp = 0; rp < 8; rp++) {
                const int rofs = ((2 * rp) & 3) + 8 * ((2 * rp) >> 2);
                const bool ok = FULL || (row0 + rofs < g.M);
                gpk[rp] = *reinterpret_cast<const unsigned*>(gpt + (ok ? (long)rofs * g.ldg : 0L));
              }
            }
#pragma unroll
            for (int rp = 0; rp < 8; rp++) {
              const int rofs = ((2 * rp) & 3) + 8 * ((2 * rp) >> 2);     // acc_row32(2 * rp, lh) - 4 * lh: the even register's row
              float own0 = fmaxf(acc[j][2 * rp] + bv, lo_clamp) * oscale, own1 = fmaxf(acc[j][2 * rp + 1] + bv, lo_clamp) * oscale;
              acc[j][2 * rp] = 0.f; acc[j][2 * rp + 1] = 0.f;
              if (EW && g.drop_p > 0.f) {    // elementwise extras stay in registers (no staging pass): dropout on the own elements ...
                const uint64_t i0 = ebase + (uint64_t)((unsigned)rofs * (unsigned)g.N);      // element index = row * N + col
                own0 = hftt_keep(g.drop_seed, g.drop_site, i0, thr) ? own0 * inv_keep : 0.f;
                own1 = hftt_keep(g.drop_seed, g.drop_site, i0 + (unsigned)g.N, thr) ? own1 * inv_keep : 0.f;
              }
              unsigned pk = pair_rows_to_cols(own0, own1, odd);
              const bool ok = FULL || (row0 + rofs < g.M);
              if (gated) {                   // ... and the bf16 ReLU gate as one packed pair per lane, same footprint as the store
                const unsigned gp = gpk[rp];
                // keep a half iff its gate is a positive bf16: bits in [0x0001, 0x7FFF]
                const unsigned m = (((gp & 0xFFFFu) - 1u) < 0x7FFFu ? 0x0000FFFFu : 0u) | ((((gp >> 16) - 1u) < 0x7FFFu) ? 0xFFFF0000u : 0u);
                pk &= m;
              }
              if (ok) *reinterpret_cast<unsigned*>(cp + (long)rofs * g.ldc) = pk;
              if (EW) __builtin_amdgcn_sched_barrier(0);      // keep the hash chains of different pairs from overlapping (registers)
            }
          }
        };
        if (m0 + BM_ <= (long)g.M) tile_out(std::true_type{}); else tile_out(std::false_type{});
      } else
#pragma unroll
      for (int j = 0; j < TN; j++) {
        const int col_l = wn * TN * 32 + j * 32 + lr;
        const int col = n0 + col_l;
        const float bv = (g.bias != nullptr) ? g.bias[col] : 0.f;       // N % 256 == 0 on this path: every column exists
        const float lo_clamp = (g.act == 1) ? 0.f : -INFINITY;
        int rb0 = wm * 32 + 4 * lh;
        if (MODE == 0) asm volatile("" : "+v"(rb0));     // opaque: the 16 row addresses are formed here, not hoisted above the k loop
        float* cp = g.C + (m0 + rb0) * g.ldc + col;
        float* sp = stage + rb0 * STAGE_LD + col_l;
        const bool full = m0 + BM_ <= (long)g.M;           // block-uniform
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int rofs = (r & 3) + 8 * (r >> 2);           // row = wm * 32 + acc_row32(r, lh) = rb0 + rofs
          const float v = fmaxf(acc[j][r] + bv, lo_clamp) * g.out_scale;
          acc[j][r] = 0.f;
          if (MODE != 0) {
            sp[rofs * STAGE_LD] = v;
          } else {
            if (full || m0 + rb0 + rofs < g.M) cp[(long)rofs * g.ldc] = v;
          }
        }
      }
      if (MODE != 0) {
        __syncthreads();
        row_pass<BM_ / 8, (BM_ / 8 < 4 ? BM_ / 8 : 4), true, true>(g, m0, n0, stage, STAGE_LD, true, thr, inv_keep);
        if (s + 1 < steps) {
          __syncthreads();
          wstore(wr[0], buf ^ 1);
        }
      }
    }
    __syncthreads();
    s++;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Split modes (npass 2 / 4), A-stationary form: N <= 256 (one N tile), K <= 256.  The same tall, short-K products as above -- the
// embedding (K = 96), the heads and their dX (K = 256 / 192) -- in three MFMA passes on split operands.  A persistent grid of one
// workgroup per CU walks the 64-row blocks (blk += gridDim.x; the workgroups never talk to each other).  Per block: the A rows are read
// from HBM once, split once (x3_split4) into a hi and a lo plane in LDS, and the prepared weight planes W / W_lo stream from L2 through
// a double-buffered ring that keeps running across the blocks (one N tile: k tile 0 follows k tile KT - 1).  The next block's A loads
// are issued in the last k step, behind the last weight load, and stay in flight in registers under that step's MFMAs and the row pass.
// Per accumulator the MFMAs come in gemm_nt_kernel's order (k ascending in k16 chunks; lo.hi, hi.lo, hi.hi within a chunk) and the epilogue
// is its text -- acc + bias, ReLU, out_scale, stage, row_pass -- so the results are its results bit for bit.
//   XE   X3_F16 / X3_BF16 (the descriptor's npass)
//   NCH  16-byte A chunks per thread: 4 (K <= 128) or 8 (K <= 256)
//   PF2  K / 32 is even: weight tiles are loaded two k steps ahead (see WRegs)
// LDS: the A planes, 64 x (K + 8) x 2 x 2 B <= 66 KB, and in the same bytes, once the k loop is done, the staged 64 x 260 fp32 tile
// (65 KB) + the ring, 2 x 2 planes x 256 x 40 x 2 B = 80 KB: 145 - 146 KB, ONE workgroup per CU.  Registers: 8 waves = two per SIMD, up
// to 256 VGPRs each (32 accumulators, 16 or 32 of weight staging, 4 * NCH of prefetched A, the row pass with 8 (NCH 4) or 4 rows in
// flight: 216 - 249 as built); no scratch (tests/test_nt_streaming_resources.py).
// ------------------------------------------------------------------------------------------------------------------
constexpr int AS3_BM = 64;
constexpr int AS3_RSW = 40;
constexpr int AS3_W_ELEMS = 2 * 256 * AS3_RSW;           // one ring buffer: hi plane, then lo plane
constexpr int AS3_STAGE_LD = 256 + 4;
constexpr int as3_a_bytes(int nch) {                     // A planes at the largest K of the form, or the stage
  const int a = AS3_BM * (nch * 32 + 8) * 2 * 2, s = AS3_BM * AS3_STAGE_LD * 4;
  return a > s ? a : s;
}
constexpr int as3_lds_bytes(int nch) { return as3_a_bytes(nch) + 2 * AS3_W_ELEMS * 2; }

template <int XE, int NCH, bool PF2>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_nt_as3_kernel(const hftt_gemm_nt_desc g, const int nblk) {
  constexpr int BM_ = AS3_BM, BN = 256, WN = 4, TN = 2, RSW = AS3_RSW, STAGE_LD = AS3_STAGE_LD;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int K = g.K;
  const int RSA = K + 8;
  unsigned short* As = reinterpret_cast<unsigned short*>(smem);                          // hi plane, lo plane at + BM_ * RSA
  unsigned short* Ws = reinterpret_cast<unsigned short*>(smem + as3_a_bytes(NCH));
  float* stage = reinterpret_cast<float*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int KT = K / 32;
  const unsigned short* Wb = reinterpret_cast<const unsigned short*>(g.W);
  const unsigned short* Wlo = reinterpret_cast<const unsigned short*>(g.W_lo);

  // weight tile kt: two 16-byte chunks of the hi plane and two of the lo plane per thread (zeroed at the start: left undefined, hipcc kept the
  // sets in scratch).  Rows past N read row N - 1 (their columns are never stored).  PF2 (K / 32 even): two sets -- tile kt waits in set kt & 1,
  // loaded two k steps before it is read from the ring, so an L2 round trip has a whole step of MFMAs to hide behind; an odd K / 32 (the
  // embedding's 3) would swap the sets' roles from block to block and loads one step ahead into one set.  The scheduling barrier keeps
  // the loads where they are written: left alone, hipcc sinks them to the ring write at the end of the step.
  struct WRegs { uint4 h0, h1, l0, l1; };
  const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
  WRegs w0 = {z4, z4, z4, z4}, w1 = {z4, z4, z4, z4};
  const int wrow = tid >> 2, wch = tid & 3;
  const long wg0 = (long)(wrow < g.N ? wrow : g.N - 1) * K + wch * 8, wg1 = (long)(wrow + 128 < g.N ? wrow + 128 : g.N - 1) * K + wch * 8;
  const int ws0 = wrow * RSW + wch * 8, ws1 = ws0 + 128 * RSW;
  auto wload = [&](WRegs& w, int kt) __attribute__((always_inline)) {
    w.h0 = *reinterpret_cast<const uint4*>(Wb + wg0 + kt * 32); w.h1 = *reinterpret_cast<const uint4*>(Wb + wg1 + kt * 32);
    w.l0 = *reinterpret_cast<const uint4*>(Wlo + wg0 + kt * 32); w.l1 = *reinterpret_cast<const uint4*>(Wlo + wg1 + kt * 32);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto wstore = [&](const WRegs& w, int buf) __attribute__((always_inline)) {
    unsigned short* d = Ws + buf * AS3_W_ELEMS;
    *reinterpret_cast<uint4*>(d + ws0) = w.h0; *reinterpret_cast<uint4*>(d + ws1) = w.h1;
    *reinterpret_cast<uint4*>(d + BN * RSW + ws0) = w.l0; *reinterpret_cast<uint4*>(d + BN * RSW + ws1) = w.l1;
  };
  float4 av[NCH];
  auto a_issue = [&](long m0) __attribute__((always_inline)) {
    AWalk w(K / 4);
    a_block_issue<BM_, float4, NCH>(g, m0, w, av);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto a_commit = [&](long m0) __attribute__((always_inline)) {
    AWalk w(K / 4);
#pragma unroll
    for (int u = 0; u < NCH; u++) {
      if (w.row < BM_) {
        uint2 hi, lo;
        x3_split4<XE>(a_chunk_live<BM_>(g, m0, w) ? av[u] : make_float4(0.f, 0.f, 0.f, 0.f), hi, lo);
        unsigned short* dst = As + w.row * RSA + w.ch * 4;
        *reinterpret_cast<uint2*>(dst) = hi;
        *reinterpret_cast<uint2*>(dst + BM_ * RSA) = lo;
      }
      w.next();
    }
  };

  f32x16 acc[TN];
  auto k_step = [&](int kt, int buf) __attribute__((always_inline)) {
    const unsigned short* Wt = Ws + buf * AS3_W_ELEMS;
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      const unsigned short* pa = As + (wm * 32 + lr) * RSA + kt * 32 + ks * 16 + lh * 8;
      const bf16x8 ah = lds_read_b128(pa), al = lds_read_b128(pa + BM_ * RSA);
#pragma unroll
      for (int j = 0; j < TN; j++) {
        const unsigned short* pb = Wt + (wn * TN * 32 + j * 32 + lr) * RSW + ks * 16 + lh * 8;
        const bf16x8 bh = lds_read_b128(pb), bl = lds_read_b128(pb + BN * RSW);
        acc[j] = x3_mma<XE>(ah, al, bh, bl, acc[j]);
      }
    }
  };

  const uint32_t thr = hftt_keep_thr(g.drop_p);
  const float inv_keep = hftt_keep_scale(g.drop_p);
  // whole-row 16-byte stores with the table add / gate / dropout / residual per quad (gemm_nt_kernel's condition); the dispatch sends
  // here only what either meets it or has none of the four (the heads: N = 131, bias only)
  const bool rowpass = (g.N % 4 == 0) && (g.gate == nullptr || g.ldg % 4 == 0) && (g.residual == nullptr || g.ldr % 4 == 0) &&
                       ((((uintptr_t)g.gate | (uintptr_t)g.residual | (uintptr_t)g.add_table) & 15) == 0);

  float bv[TN];                                  // (loaded once: a load inside the block loop would wait for the prefetched A as well)
#pragma unroll
  for (int j = 0; j < TN; j++) {
    const int col_l = wn * TN * 32 + j * 32 + lr;
    bv[j] = (g.bias != nullptr && col_l < g.N) ? g.bias[col_l] : 0.f;
  }
  long blk = blockIdx.x;
  wload(w0, 0);
  if constexpr (PF2) wload(w1, 1);
  a_issue(blk * BM_);
  wstore(w0, 0);
  int s = 0;                                     // !PF2: k steps so far -- tile s of the endless sequence sits in ring buffer s & 1
  for (; blk < nblk; blk += gridDim.x) {
    const long m0 = blk * BM_;
    a_commit(m0);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
    // In the last k step the first tile(s) of the next block go on their way, and behind them the next block's A (past the last block: a
    // clamped row, unused) into registers.  The barrier behind the last step also says that every wave is done with the A planes: the
    // stage may overwrite them.
    if constexpr (PF2) {                           // tile kt in ring buffer kt & 1; at the top of a block tile 0 is in the ring, tile 1 in w1
      for (int kt = 0; kt + 2 < KT; kt += 2) {
        wload(w0, kt + 2); k_step(kt, 0); wstore(w1, 1);
        __syncthreads();
        wload(w1, kt + 3); k_step(kt + 1, 1); wstore(w0, 0);
        __syncthreads();
      }
      wload(w0, 0); k_step(KT - 2, 0); wstore(w1, 1);
      __syncthreads();
      wload(w1, 1);
      a_issue((blk + gridDim.x) * BM_);
      k_step(KT - 1, 1); wstore(w0, 0);
      __syncthreads();
    } else {
      for (int kt = 0; kt + 1 < KT; kt++) {
        wload(w0, kt + 1); k_step(kt, s & 1); wstore(w0, (s & 1) ^ 1);
        __syncthreads();
        s++;
      }
      wload(w0, 0);
      a_issue((blk + gridDim.x) * BM_);
      k_step(KT - 1, s & 1); wstore(w0, (s & 1) ^ 1);
      __syncthreads();
      s++;
    }

#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int col_l = wn * TN * 32 + j * 32 + lr;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row_l = wm * 32 + acc_row32(r, lh);
        float v = acc[j][r] + bv[j];
        if (g.act == 1) v = fmaxf(v, 0.f);
        v *= g.out_scale;
        stage[row_l * STAGE_LD + col_l] = v;
      }
    }
    __syncthreads();
    if (rowpass) {
      // (a wave's rows in flight: all eight where the registers allow it -- one wait for the table / residual loads per block instead of two)
      row_pass<BM_ / 8, NCH == 4 ? 8 : 4, false, false>(g, m0, 0, stage, STAGE_LD, lane * 4 < g.N, thr, inv_keep);
    } else {
      const int c4 = lane * 4;
#pragma unroll 1
      for (int rr = 0; rr < BM_ / 8; rr++) {
        const int row_l = wave * (BM_ / 8) + rr;
        const long row = m0 + row_l;
        if (row >= g.M) break;                   // (wave-uniform)
        const float4 sv = *reinterpret_cast<const float4*>(stage + row_l * STAGE_LD + c4);
        float* cp = g.C + row * g.ldc + c4;
        if (c4 + 4 <= g.N) {
          *reinterpret_cast<float4*>(cp) = sv;
        } else {                                 // the quad that N cuts: the columns [N, ldc) keep what they hold
          if (c4 < g.N) cp[0] = sv.x;
          if (c4 + 1 < g.N) cp[1] = sv.y;
          if (c4 + 2 < g.N) cp[2] = sv.z;
        }
      }
    }
    __syncthreads();                             // the stage is read: the next block's A planes may take its place
  }
}

// 0 = off: every split-mode product takes gemm_nt_kernel, as before the A-stationary form existed.  Read at every qualifying call, so one
// process can run both (hftt_hip/plan.py nt_meta reads the same variable for the kernel's name).
bool nt_as3_enabled() {
  const char* e = getenv("HFTT_NT_STREAM");
  return !(e != nullptr && e[0] == '0');
}
// does the A-stationary split form take this product?  (npass 2 / 4 without HFTT_NT_A_HI is the caller's test)
bool nt_as3_takes(const hftt_gemm_nt_desc& d) {
  if (d.ln_gamma != nullptr || d.K > 256 || !(d.N == 256 || (d.K == 256 && d.N <= 256))) return false;
  if (d.ldc % 4 != 0 || ((uintptr_t)d.C & 15) != 0) return false;
  const bool rich = d.add_table || d.gate || d.drop_p > 0.f || d.residual;
  const bool quads = (d.N % 4 == 0) && (!d.gate || d.ldg % 4 == 0) && (!d.residual || d.ldr % 4 == 0) &&
                     ((((uintptr_t)d.gate | (uintptr_t)d.residual | (uintptr_t)d.add_table) & 15) == 0);
  return (quads || !rich) && nt_as3_enabled();
}
template <int XE, int NCH, bool PF2>
int launch_nt_as3(const hftt_gemm_nt_desc& d, hipStream_t st) {
  constexpr int lds = as3_lds_bytes(NCH);
  const int nblk = (d.M + AS3_BM - 1) / AS3_BM;
  int wgs = 0;
  if (int rc = hftt_resident_wgs<gemm_nt_as3_kernel<XE, NCH, PF2>>("gemm_nt", 512, lds, &wgs)) return rc;
  dim3 grid((unsigned)(nblk < wgs ? nblk : wgs), 1, 1);
  return hftt_launch<gemm_nt_as3_kernel<XE, NCH, PF2>>("gemm_nt", grid, dim3(512), lds, st, d, nblk);
}
template <int XE>
int dispatch_nt_as3(const hftt_gemm_nt_desc& d, hipStream_t st) {
  const bool pf2 = (d.K / 32) % 2 == 0;
  if (d.K <= 128) return pf2 ? launch_nt_as3<XE, 4, true>(d, st) : launch_nt_as3<XE, 4, false>(d, st);
  return pf2 ? launch_nt_as3<XE, 8, true>(d, st) : launch_nt_as3<XE, 8, false>(d, st);
}

template <int BM_, int MODE, bool EW = false, int PF = 1>
int launch_nt_as1(const hftt_gemm_nt_desc& d, hipStream_t st) {
  int lds = (BM_ * (d.K + 8) + 2 * 256 * 40) * 2;
  const int stage = BM_ * 260 * 4;
  if (MODE == 1 && stage > lds) lds = stage;
  dim3 grid((unsigned)((d.M + BM_ - 1) / BM_), 1, 1);
  return hftt_launch<gemm_nt_as1_kernel<BM_, MODE, EW, PF>>("gemm_nt", grid, dim3(512), lds, st, d);
}

template <int BN, int PREC, bool LN>
int launch_nt(const hftt_gemm_nt_desc& d, hipStream_t st) {
  using Cfg = NtCfg<BN, PREC>;
  int lds = Cfg::LOOP_BYTES;
  if ((LN || (Cfg::X3M && BN == 256)) && Cfg::STAGE_BYTES > lds) lds = Cfg::STAGE_BYTES;      // (split modes: the row-pass epilogue stages the tile)
  const int n_pad = ((d.N + 63) / 64) * 64;
  dim3 grid((unsigned)((d.M + BM - 1) / BM), (unsigned)((n_pad + BN - 1) / BN), 1);
  return hftt_launch<gemm_nt_kernel<BN, PREC, LN>>("gemm_nt", grid, dim3(512), lds, st, d);
}

template <int PREC>
int dispatch_nt(const hftt_gemm_nt_desc& d, hipStream_t st) {
  const int n_pad = ((d.N + 63) / 64) * 64;
  if (d.ln_gamma != nullptr) {
    if (d.N == 256) return launch_nt<256, PREC, true>(d, st);
    if (d.N == 128) return launch_nt<128, PREC, true>(d, st);
    if (d.N == 64) return launch_nt<64, PREC, true>(d, st);
    hftt_set_error("gemm_nt: fused LayerNorm needs N in {64,128,256}, got %d", d.N);
    return 1;
  }
  if (n_pad % 256 == 0) return launch_nt<256, PREC, false>(d, st);
  if (n_pad % 128 == 0) return launch_nt<128, PREC, false>(d, st);
  return launch_nt<64, PREC, false>(d, st);
}

// weight-tile prefetch distance in k steps: the kernel unrolls groups of PF steps, so PF divides K / 32 -- 2 where that is even, else 1
template <int BM_, int MODE, bool EW>
int launch_nt_as1_pf(const hftt_gemm_nt_desc& d, hipStream_t st) {
  return (d.K / 32) % 2 == 0 ? launch_nt_as1<BM_, MODE, EW, 2>(d, st) : launch_nt_as1<BM_, MODE, EW, 1>(d, st);
}

// bf16-mode dispatch
int dispatch_nt_bf16(const hftt_gemm_nt_desc& d, hipStream_t st) {
  const bool vec_ok = (d.ldc % 4 == 0) && (((uintptr_t)d.C & 15) == 0) &&
                      (!d.residual || (d.ldr % 4 == 0 && ((uintptr_t)d.residual & 15) == 0)) &&
                      (!d.gate || (d.ldg % 4 == 0 && ((uintptr_t)d.gate & 15) == 0)) &&
                      (!d.add_table || ((uintptr_t)d.add_table & 15) == 0) &&
                      (!d.pre_ln_out || ((uintptr_t)d.pre_ln_out & 15) == 0) &&
                      (!d.ln_gamma || d.N == 256);
  if (d.N % 256 == 0 && d.K <= 768 && d.M >= 256 && vec_ok) {
    const bool pf2 = (d.K / 32) % 2 == 0;
    if (d.K <= 256) {
      const bool rich = d.add_table || d.gate || d.drop_p > 0.f || d.residual || d.ln_gamma;
      if (!rich) return launch_nt_as1_pf<64, 0, false>(d, st);
      // dropout / bf16 ReLU gate on a bf16 C are elementwise: they ride in the direct packed-store epilogue (no staging pass)
      const bool elementwise = !d.add_table && !d.residual && !d.ln_gamma && (d.io_flags & HFTT_NT_C_BF16) && d.ldc % 2 == 0 &&
                               (!d.gate || ((d.io_flags & HFTT_NT_GATE_BF16) && d.ldg % 2 == 0));
      if (elementwise) return launch_nt_as1_pf<64, 0, true>(d, st);
      if (d.N == 256) return launch_nt_as1_pf<64, 1, false>(d, st);
      return launch_nt_as1<32, 2>(d, st);
    }
    // N = 256, measured at M = 262144 (us): K = 768: BM=64 504 | BM=32 713;  K = 512: BM=64 (1 WG/CU) 254 | BM=32 275 without LayerNorm,
    // with it 354 | 340
    if (d.N == 256 && d.K > 512) return launch_nt_as1_pf<64, 1, false>(d, st);
    if (d.N == 256 && pf2) return d.ln_gamma ? launch_nt_as1<32, 1, false, 2>(d, st) : launch_nt_as1<64, 1, false, 2>(d, st);
    // Every other shape (N = 512, 768, ..; N = 256 with an odd K / 32) takes the BM = 32 form: one N tile after another over the resident A
    // block.  Measured at M = 262144 (us, median of 60; in brackets a persistent form of the same loop -- 1 or 2 workgroups per CU walking
    // the blocks, the next block's A loads under the MFMA loop -- whose own run-to-run spread was <= 11 us):
    //   (N, K)        bf16 A, plain   bf16 A, +res -> bf16 C   fp32 A, plain   fp32 A, +res -> bf16 C
    //   (512, 512)     490  (499)       502  (521)              493  (521)       521  (560)
    //   (768, 512)     655  (673)       729  (764)              693  (729)       759  (810)
    //   (512, 768)    1088 (1108)      1160 (1199)             1153 (1260)      1241 (1354)
    //   (768, 768)    1623 (1690)      1718 (1815)             1687 (1853)      1770 (1961)
    return launch_nt_as1<32, 2>(d, st);
  }
  if (d.io_flags & HFTT_NT_RES_BF16) { hftt_set_error("gemm_nt: a bf16 residual needs the A-stationary path (N %% 256 == 0, M >= 256, K <= 768)"); return 1; }
  return dispatch_nt<1>(d, st);      // small / ragged shapes: the k-tiled streaming kernel
}

}  // namespace

extern "C" int hftt_gemm_nt(const hftt_gemm_nt_desc* d, void* stream) {
  HFTT_REQUIRE(d != nullptr, "gemm_nt: null descriptor");
  HFTT_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0, "gemm_nt: bad shape M=%d N=%d K=%d", d->M, d->N, d->K);
  HFTT_REQUIRE(d->K % 32 == 0, "gemm_nt: K=%d must be a multiple of 32", d->K);
  HFTT_REQUIRE((d->io_flags & ~HFTT_NT_A_HI) == 0 || d->npass == 1, "gemm_nt: bf16-stored operands need npass == 1");
  HFTT_REQUIRE(!(d->io_flags & HFTT_NT_A_HI) || d->npass == 4, "gemm_nt: HFTT_NT_A_HI goes with npass == 4");
  HFTT_REQUIRE(!(d->io_flags & HFTT_NT_C_BF16) || d->ln_gamma == nullptr, "gemm_nt: a bf16 C cannot be combined with LayerNorm");
  HFTT_REQUIRE(d->lda % ((d->io_flags & HFTT_NT_A_BF16) ? 8 : 4) == 0, "gemm_nt: lda=%ld breaks 16-byte row alignment", (long)d->lda);
  HFTT_REQUIRE(((uintptr_t)d->A & 15) == 0 && ((uintptr_t)d->W & 15) == 0, "gemm_nt: A/W must be 16-byte aligned");
  HFTT_REQUIRE(d->npass >= 1 && d->npass <= 4, "gemm_nt: npass must be 1 (bf16), 2 (split fp16), 3 (fp32) or 4 (split bf16)");
  HFTT_REQUIRE((d->npass != 2 && d->npass != 4) || d->W_lo != nullptr, "gemm_nt: the split modes need the lo weight plane (W_lo)");
  HFTT_REQUIRE(d->A != nullptr && d->W != nullptr && d->C != nullptr, "gemm_nt: null operand");
  HFTT_REQUIRE(d->add_table == nullptr || d->add_mod > 0, "gemm_nt: add_mod must be > 0");
  HFTT_REQUIRE(d->residual == nullptr || d->res_mod > 0, "gemm_nt: res_mod must be > 0");
  HFTT_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, "gemm_nt: drop_p out of range");
  HFTT_REQUIRE(d->ln_gamma == nullptr || (d->ln_beta != nullptr && d->ldc == d->N), "gemm_nt: LN needs beta and ldc == N");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->npass == 3) return dispatch_nt<3>(*d, st);
  if (d->npass == 2) return nt_as3_takes(*d) ? dispatch_nt_as3<X3_F16>(*d, st) : dispatch_nt<2>(*d, st);
#ifdef HFTT_GRAD_HI_BUILD
  if (d->npass == 4 && (d->io_flags & HFTT_NT_A_HI)) return dispatch_nt<5>(*d, st);
#else
  HFTT_REQUIRE(!(d->io_flags & HFTT_NT_A_HI), "gemm_nt: this library was built without the gradient-rounding option (HFTT_BUILD_GRAD_HI=1 python nylon-amt_amd/build.py)");
#endif
  if (d->npass == 4) return nt_as3_takes(*d) ? dispatch_nt_as3<X3_BF16>(*d, st) : dispatch_nt<4>(*d, st);
  return dispatch_nt_bf16(*d, st);
}
