// LayerNorm backward of the hFT-Transformer path (gfx950): HBM-bound, fp32 or bf16 storage per tensor, the gamma / beta gradients as
// per-workgroup partials and one reduce launch in a fixed order (deterministic, no float atomics).  The row arithmetic, the dropped copy and
// the flush of the partials are written once; the four kernels are the loaders around them: the lane-to-column map, the width of the loads
// and stores, the prefetch and the tree of the row sum.  Entry points and reference citations: include/hftt_hip.h.
#include "hftt_common.h"
#include "hftt_launch.h"
#include "../../include/hftt_hip.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------ the row arithmetic, once
// Every product and sum below is written out with contraction switched off, so the bits do not depend on what a compiler fuses.  Where the
// kernels differ, they differ in historical bits that are kept: before the arithmetic was written once, each kernel's fusing was the
// compiler's choice, made per element, and these are the choices it had made (bit e of a mask = element e of the lane):
//                                  S2 (s2 = fma(xh, gg, s2))   T (gg - s1 as fma(dy, gamma, -s1))   DG (dg = fma(dy, xh, dg))
//   ln_bwd_kernel<1>               none                        none                                  no
//   ln_bwd_kernel<2>, <4>          none                        none                                  yes
//   ln_bwd64_kernel                none                        elements 0, 1                         yes
//   ln_bwd256_bf16_kernel          elements 8, 9               none                                  yes
//   ln_bwd256_rows_kernel<2, *>    none                        none                                  yes
// Everything else is the same in all of them: s1 is a sum of the rounded gg, xh * s2 always joins its subtraction in one fma.
template <unsigned S2, unsigned T, bool DG>
struct ln_fused { static constexpr unsigned s2 = S2, t = T; static constexpr bool dg = DG; };

// Row terms.  In: the lane's dy, r (in xh), gamma, the row's mean / rstd and whether the row exists (a clamped row contributes nothing).
// Out: xh, gg = dy * gamma, the lane's partial row sums s1 = sum gg and s2 = sum gg * xh in element order, dg / db accumulated.
template <int E, class F>
__device__ __forceinline__ void ln_row_terms(float (&dy)[E], float (&xh)[E], const float (&gam)[E], float mean, float rstd, bool valid,
                                             float (&gg)[E], float& s1, float& s2, float (&dg)[E], float (&db)[E]) {
#pragma clang fp contract(off)
  s1 = 0.f; s2 = 0.f;
#pragma unroll
  for (int e = 0; e < E; e++) {
    if (!valid) dy[e] = 0.f;
    xh[e] = (xh[e] - mean) * rstd;
    gg[e] = dy[e] * gam[e];
    s1 += gg[e];
    s2 = ((F::s2 >> e) & 1u) ? __builtin_fmaf(xh[e], gg[e], s2) : s2 + gg[e] * xh[e];
    dg[e] = F::dg ? __builtin_fmaf(dy[e], xh[e], dg[e]) : dg[e] + dy[e] * xh[e];
    db[e] += dy[e];
  }
}

// Row output o = rstd * (gg - s1 - xh * s2); s1 and s2 are the row sums after the caller's lane reduction and its * (1 / N).
template <int E, class F>
__device__ __forceinline__ void ln_row_out(const float (&dy)[E], const float (&gam)[E], const float (&gg)[E], const float (&xh)[E], float s1, float s2,
                                           float rstd, float (&o)[E]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < E; e++) {
    const float t = ((F::t >> e) & 1u) ? __builtin_fmaf(dy[e], gam[e], -s1) : gg[e] - s1;
    o[e] = rstd * __builtin_fmaf(-s2, xh[e], t);
  }
}

// ------------------------------------------------------------------ the dropped copy, from the unrounded o
struct ln_drop {
  uint32_t thr; float inv_keep;
  bool on;                                  // a dropped copy is asked for and something is dropped
};
__device__ __forceinline__ ln_drop ln_drop_of(const hftt_ln_bwd_desc& g) {
  return {hftt_keep_thr(g.drop_p), hftt_keep_scale(g.drop_p), g.dr_drop != nullptr && g.drop_p > 0.f};
}
// one hash decision per element (the element-wise form: no alignment to rely on); base = element offset of v[0]
template <int E>
__device__ __forceinline__ void ln_drop_elems(const hftt_ln_bwd_desc& g, const ln_drop& dp, long base, float (&v)[E]) {
#pragma unroll
  for (int e = 0; e < E; e++) v[e] = hftt_keep(g.drop_seed, g.drop_site, (uint64_t)(base + e), dp.thr) ? v[e] * dp.inv_keep : 0.f;
}
// one hash for an aligned group of four (the same decisions, hftt_common.h); base = element offset of v[0], a multiple of 4
__device__ __forceinline__ void ln_drop_quad(const hftt_ln_bwd_desc& g, const ln_drop& dp, long base, float* v) {
  const uint32_t k4 = hftt_keep_quad(g.drop_seed, g.drop_site, (uint64_t)base >> 2, dp.thr);
#pragma unroll
  for (int f = 0; f < 4; f++) v[f] = ((k4 >> f) & 1u) ? v[f] * dp.inv_keep : 0.f;
}

// ------------------------------------------------------------------ the flush of dgamma / dbeta
// red[q][0 / 1][c]: the partial of row group q of the workgroup for column c, written by the kernel in its own column map.  Summed in the
// fixed order q = 0 .. ROWS - 1 (reproducible) into this workgroup's 2N entries of ws.
template <int N, int ROWS>
__device__ __forceinline__ void ln_flush(const float (&red)[ROWS][2][N], float* __restrict__ ws) {
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * N; i += 256) {
    const int which = i / N, c = i % N;
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < ROWS; q++) acc += red[q][which][c];
    ws[(long)blockIdx.x * 2 * N + i] = acc;
  }
}

// ------------------------------------------------------------------ the four forms
// one row per wave, element-wise accesses only: N = 128, and the form hftt_ln_bwd falls back to at N = 64 / 256 when an operand is not
// 16-byte aligned (a view offset by one element), so no access here may be wider than the element.
template <int VPL>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const hftt_ln_bwd_desc g) {
  constexpr int N = VPL * 64;
  using F = ln_fused<0u, 0u, (VPL > 1)>;
  __shared__ float red[4][2][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ln_drop dp = ln_drop_of(g);
  const bool dy_bf = g.io_flags & HFTT_LNB_DY_BF16, dr_bf = g.io_flags & HFTT_LNB_DR_BF16, r_bf = g.io_flags & HFTT_LNB_R_BF16;
  float gam[VPL], dg[VPL], db[VPL];
#pragma unroll
  for (int e = 0; e < VPL; e++) { gam[e] = g.gamma[lane * VPL + e]; dg[e] = 0.f; db[e] = 0.f; }
  for (long row = (long)blockIdx.x * 4 + wave; row < g.M; row += (long)gridDim.x * 4) {
    float dy[VPL], xh[VPL];
    const long base = row * N + lane * VPL;
#pragma unroll
    for (int e = 0; e < VPL; e++) { dy[e] = dy_bf ? bf2f(reinterpret_cast<const unsigned short*>(g.dy)[base + e]) : g.dy[base + e]; xh[e] = r_bf ? bf2f(reinterpret_cast<const unsigned short*>(g.r)[base + e]) : g.r[base + e]; }
    const float rstd = g.rstd[row];
    float gg[VPL], s1, s2, o[VPL];
    ln_row_terms<VPL, F>(dy, xh, gam, g.mean[row], rstd, true, gg, s1, s2, dg, db);
    s1 = wave_sum(s1) * (1.0f / N);
    s2 = wave_sum(s2) * (1.0f / N);
    ln_row_out<VPL, F>(dy, gam, gg, xh, s1, s2, rstd, o);
#pragma unroll
    for (int e = 0; e < VPL; e++) hftt_store1(g.dr, dr_bf, base + e, o[e]);
    if (g.dr_drop != nullptr) {
      if (dp.on) ln_drop_elems<VPL>(g, dp, base, o);
#pragma unroll
      for (int e = 0; e < VPL; e++) hftt_store1(g.dr_drop, g.drop_bf16 != 0, base + e, o[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < VPL; e++) { red[wave][0][lane * VPL + e] = dg[e]; red[wave][1][lane * VPL + e] = db[e]; }
  ln_flush<N, 4>(red, g.ws);
}

// N = 64 (the reference's default width): a wave takes FOUR rows per step -- 16 lanes x 4 elements per row, one 16-byte (fp32) or 8-byte
// (bf16) access per lane and tensor, a 16-lane reduction -- instead of one row of 4-byte accesses and a 64-lane reduction: the row-per-wave
// form above sat at 3.4 TB/s at this width (13 launches, 0.66 ms of the tiny configuration's 5.4 ms step).
__global__ __launch_bounds__(256) void ln_bwd64_kernel(const hftt_ln_bwd_desc g) {
  constexpr int N = 64;
  using F = ln_fused<0u, 0x3u, true>;
  __shared__ float red[4][2][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane >> 4, c0 = (lane & 15) * 4;
  const ln_drop dp = ln_drop_of(g);
  const bool dy_bf = g.io_flags & HFTT_LNB_DY_BF16, dr_bf = g.io_flags & HFTT_LNB_DR_BF16, r_bf = g.io_flags & HFTT_LNB_R_BF16;
  const float4 gm = *reinterpret_cast<const float4*>(g.gamma + c0);
  const float gam[4] = {gm.x, gm.y, gm.z, gm.w};
  float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
  for (long row0 = ((long)blockIdx.x * 4 + wave) * 4; row0 < g.M; row0 += (long)gridDim.x * 16) {
    const long row = row0 + sub;
    const bool ok = row < g.M;                       // (uniform over the 16 lanes of a row)
    const long rc = ok ? row : (long)g.M - 1;
    const long base = rc * N + c0;
    const float4 a = hftt_load4(g.dy, dy_bf, base);
    const float4 b = hftt_load4(g.r, r_bf, base);
    const float rstd = g.rstd[rc];
    float dy[4] = {a.x, a.y, a.z, a.w}, xh[4] = {b.x, b.y, b.z, b.w};
    float gg[4], s1, s2, o[4];
    ln_row_terms<4, F>(dy, xh, gam, g.mean[rc], rstd, ok, gg, s1, s2, dg, db);
    s1 = group_sum<16>(s1) * (1.0f / N);
    s2 = group_sum<16>(s2) * (1.0f / N);
    ln_row_out<4, F>(dy, gam, gg, xh, s1, s2, rstd, o);
    if (ok) {
      hftt_store4(g.dr, dr_bf, base, o[0], o[1], o[2], o[3]);
      if (g.dr_drop != nullptr) {
        if (dp.on) ln_drop_quad(g, dp, base, o);
        hftt_store4(g.dr_drop, g.drop_bf16 != 0, base, o[0], o[1], o[2], o[3]);
      }
    }
  }
  // the four row groups of the wave hold partial sums of the same columns: folded across the lanes before the flush (the one variant of it)
#pragma unroll
  for (int e = 0; e < 4; e++) {
    dg[e] += __shfl_xor(dg[e], 16); dg[e] += __shfl_xor(dg[e], 32);
    db[e] += __shfl_xor(db[e], 16); db[e] += __shfl_xor(db[e], 32);
  }
  if (lane < 16) {
#pragma unroll
    for (int e = 0; e < 4; e++) { red[wave][0][c0 + e] = dg[e]; red[wave][1][c0 + e] = db[e]; }
  }
  ln_flush<N, 4>(red, g.ws);
}

// N = 256 with dy, r, dr (and the dropped copy) all stored as bf16 -- the bf16 gradient stream of the strip plans.  The row-per-wave form
// above moves 8 bytes per lane and per tensor and goes through a 64-lane reduction for every row, one row at a time: it sat at 3.7 TB/s.
// Here a wave takes FOUR rows per step (16 lanes x 16 elements per row: two 16-byte loads per lane and tensor, a 16-lane reduction) and the
// next step's loads are issued before the current step is computed.
__device__ __forceinline__ void unpack16(const uint4& a, const uint4& b, float* v) {
  const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int e = 0; e < 8; e++) { v[2 * e] = __uint_as_float(w[e] << 16); v[2 * e + 1] = __uint_as_float(w[e] & 0xFFFF0000u); }
}
__device__ __forceinline__ void pack16(const float* v, uint4& a, uint4& b) {
  unsigned w[8];
#pragma unroll
  for (int e = 0; e < 8; e++) w[e] = f2bf(v[2 * e]) | ((unsigned)f2bf(v[2 * e + 1]) << 16);
  a = make_uint4(w[0], w[1], w[2], w[3]); b = make_uint4(w[4], w[5], w[6], w[7]);
}
__global__ __launch_bounds__(256) void ln_bwd256_bf16_kernel(const hftt_ln_bwd_desc g) {
  constexpr int N = 256;
  using F = ln_fused<0x0300u, 0u, true>;
  __shared__ float red[16][2][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane >> 4, cl = lane & 15;               // row within the group of four, 16-column chunk
  const ln_drop dp = ln_drop_of(g);
  const unsigned short* dyp = reinterpret_cast<const unsigned short*>(g.dy);
  const unsigned short* rp = reinterpret_cast<const unsigned short*>(g.r);
  unsigned short* drp = reinterpret_cast<unsigned short*>(g.dr);
  unsigned short* ddp = reinterpret_cast<unsigned short*>(g.dr_drop);
  float gam[16], dg[16], db[16];
#pragma unroll
  for (int e = 0; e < 16; e++) { gam[e] = g.gamma[cl * 16 + e]; dg[e] = 0.f; db[e] = 0.f; }
  const long ngrp = ((long)g.M + 3) / 4;
  const long stride = (long)gridDim.x * 4;
  long grp = (long)blockIdx.x * 4 + wave;
  uint4 y0, y1, r0, r1;
  float mean, rstd;
  auto load = [&](long gq) {
    const long row = gq * 4 + sub;
    const long rc = row < g.M ? row : (long)g.M - 1;       // clamped: loads stay unconditional
    const uint4* py = reinterpret_cast<const uint4*>(dyp + rc * N + cl * 16);
    const uint4* pr = reinterpret_cast<const uint4*>(rp + rc * N + cl * 16);
    y0 = py[0]; y1 = py[1]; r0 = pr[0]; r1 = pr[1];
    mean = g.mean[rc]; rstd = g.rstd[rc];
  };
  if (grp < ngrp) load(grp);
  for (; grp < ngrp; grp += stride) {
    float dy[16], xh[16];
    unpack16(y0, y1, dy);
    unpack16(r0, r1, xh);
    const float mu = mean, rs = rstd;
    const long row = grp * 4 + sub;
    const long nxt = grp + stride;
    load(nxt < ngrp ? nxt : ngrp - 1);                     // the next step's rows are in flight while this step is computed
    const bool valid = row < g.M;
    float gg[16], s1, s2, o[16];
    ln_row_terms<16, F>(dy, xh, gam, mu, rs, valid, gg, s1, s2, dg, db);
    s1 = group_sum<16>(s1) * (1.0f / N);
    s2 = group_sum<16>(s2) * (1.0f / N);
    ln_row_out<16, F>(dy, gam, gg, xh, s1, s2, rs, o);
    if (valid) {
      const long base = row * N + cl * 16;
      uint4 a, b;
      pack16(o, a, b);
      uint4* po = reinterpret_cast<uint4*>(drp + base);
      po[0] = a; po[1] = b;
      if (g.dr_drop != nullptr) {
        if (dp.on) {
#pragma unroll
          for (int q = 0; q < 4; q++) ln_drop_quad(g, dp, base + 4 * q, o + 4 * q);
          pack16(o, a, b);
        }
        uint4* pd = reinterpret_cast<uint4*>(ddp + base);
        pd[0] = a; pd[1] = b;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 16; e++) { red[wave * 4 + sub][0][cl * 16 + e] = dg[e]; red[wave * 4 + sub][1][cl * 16 + e] = db[e]; }
  ln_flush<N, 16>(red, g.ws);
}

// N = 256, any mix of fp32 / bf16 storage (the x3 plans: fp32 dy and dr, bf16 saved sums): R rows per wave, the lane's columns taken as
// groups of four at a stride of 4 * (64 / R) so that the lanes of a row cover CONTIGUOUS bytes with every access; PF: the next step's rows
// are in flight while the current step is computed.  Measured at 262,144 rows in that storage mix (tools/bench_ln_bwd.py): the row-per-wave
// kernel above (64-lane reduction with four v_readlane per sum) 5.1 TB/s, R = 4 4.2 .. 4.4 TB/s (16 elements per lane in four arrays:
// registers cost it the occupancy that hides the latency), R = 2 5.3 TB/s with or without PF -- the form instantiated.
template <int R, bool PF>
__global__ __launch_bounds__(256) void ln_bwd256_rows_kernel(const hftt_ln_bwd_desc g) {
  constexpr int N = 256, L = 64 / R, G = N / (4 * L), E = 4 * G;      // lanes per row, float4 groups and elements per lane
  using F = ln_fused<0u, 0u, true>;
  __shared__ float red[4 * R][2][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / L, cl = lane % L;
  const ln_drop dp = ln_drop_of(g);
  const bool dy_bf = g.io_flags & HFTT_LNB_DY_BF16, dr_bf = g.io_flags & HFTT_LNB_DR_BF16, r_bf = g.io_flags & HFTT_LNB_R_BF16;
  float gam[E], dg[E], db[E];
#pragma unroll
  for (int k = 0; k < G; k++) {
    const float4 t = *reinterpret_cast<const float4*>(g.gamma + cl * 4 + 4 * L * k);
    gam[4 * k] = t.x; gam[4 * k + 1] = t.y; gam[4 * k + 2] = t.z; gam[4 * k + 3] = t.w;
  }
#pragma unroll
  for (int e = 0; e < E; e++) { dg[e] = 0.f; db[e] = 0.f; }
  const long ngrp = ((long)g.M + R - 1) / R;
  const long stride = (long)gridDim.x * 4;
  long grp = (long)blockIdx.x * 4 + wave;
  float4 yv[G], rv[G];
  float mean, rstd;
  auto load = [&](long gq) {
    const long row = gq * R + sub;
    const long rc = row < g.M ? row : (long)g.M - 1;       // clamped: loads stay unconditional
    const long base = rc * N + cl * 4;
#pragma unroll
    for (int k = 0; k < G; k++) { yv[k] = hftt_load4(g.dy, dy_bf, base + 4 * L * k); rv[k] = hftt_load4(g.r, r_bf, base + 4 * L * k); }
    mean = g.mean[rc]; rstd = g.rstd[rc];
  };
  if (PF && grp < ngrp) load(grp);
  for (; grp < ngrp; grp += stride) {
    if (!PF) load(grp);
    float dy[E], xh[E];
#pragma unroll
    for (int k = 0; k < G; k++) {
      dy[4 * k] = yv[k].x; dy[4 * k + 1] = yv[k].y; dy[4 * k + 2] = yv[k].z; dy[4 * k + 3] = yv[k].w;
      xh[4 * k] = rv[k].x; xh[4 * k + 1] = rv[k].y; xh[4 * k + 2] = rv[k].z; xh[4 * k + 3] = rv[k].w;
    }
    const float mu = mean, rs = rstd;
    const long row = grp * R + sub;
    if (PF) {
      const long nxt = grp + stride;
      load(nxt < ngrp ? nxt : ngrp - 1);                   // the next step's rows are in flight while this step is computed
    }
    const bool valid = row < g.M;
    float gg[E], s1, s2, o[E];
    ln_row_terms<E, F>(dy, xh, gam, mu, rs, valid, gg, s1, s2, dg, db);
    s1 = group_sum<16>(s1); s2 = group_sum<16>(s2);
    if (L == 32) { s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16); }
    s1 *= (1.0f / N); s2 *= (1.0f / N);
    ln_row_out<E, F>(dy, gam, gg, xh, s1, s2, rs, o);
    if (valid) {
      const long base = row * N + cl * 4;
#pragma unroll
      for (int k = 0; k < G; k++) hftt_store4(g.dr, dr_bf, base + 4 * L * k, o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
      if (g.dr_drop != nullptr) {
#pragma unroll
        for (int k = 0; k < G; k++) {
          if (dp.on) ln_drop_quad(g, dp, base + 4 * L * k, o + 4 * k);
          hftt_store4(g.dr_drop, g.drop_bf16 != 0, base + 4 * L * k, o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < G; k++)
#pragma unroll
    for (int f = 0; f < 4; f++) {
      red[wave * R + sub][0][cl * 4 + 4 * L * k + f] = dg[4 * k + f];
      red[wave * R + sub][1][cl * 4 + 4 * L * k + f] = db[4 * k + f];
    }
  ln_flush<N, 4 * R>(red, g.ws);
}

// out[c] = beta*out[c] + sum_w ws[w][c]   (c over 2N entries: dgamma then dbeta)
__global__ __launch_bounds__(256) void ln_bwd_reduce_kernel(const float* __restrict__ ws, int n_wg, int N, float* dgamma, float* dbeta, float beta) {
  __shared__ float red[16][17];
  const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float acc = 0.f;
  if (c < 2 * N) {
    // eight independent loads in flight per thread (the plain loop was one dependent L2 round trip per partial: ~20 us for 2 MB)
    float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int w = rg;
    for (; w + 16 * 7 < n_wg; w += 16 * 8) {
#pragma unroll
      for (int u = 0; u < 8; u++) a8[u] += ws[(long)(w + 16 * u) * 2 * N + c];
    }
    for (; w < n_wg; w += 16) a8[0] += ws[(long)w * 2 * N + c];
    acc = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
  }
  red[rg][cl] = acc;
  __syncthreads();
  if (rg == 0 && c < 2 * N) {
    float s = 0.f;
    for (int q = 0; q < 16; q++) s += red[q][cl];
    float* dst = (c < N) ? (dgamma + c) : (dbeta + (c - N));
    *dst = (beta != 0.f) ? (*dst * beta + s) : s;
  }
}

}  // namespace

extern "C" int32_t hftt_ln_bwd_wgs(int32_t M) {
  int w = (M + 3) / 4;
  if (w > 1024) w = 1024;
  if (w < 1) w = 1;
  return w;
}
extern "C" int hftt_ln_bwd(const hftt_ln_bwd_desc* d, void* stream) {
  HFTT_REQUIRE(d && d->dy && d->r && d->mean && d->rstd && d->gamma && d->dr && d->ws, "ln_bwd: null operand");
  HFTT_REQUIRE(d->N == 64 || d->N == 128 || d->N == 256, "ln_bwd: N=%d must be 64, 128 or 256", d->N);
  const int wgs = hftt_ln_bwd_wgs(d->M);
  const uint32_t all_bf = HFTT_LNB_DY_BF16 | HFTT_LNB_DR_BF16 | HFTT_LNB_R_BF16;
  const bool fast = d->N == 256 && (d->io_flags & all_bf) == all_bf && (d->dr_drop == nullptr || d->drop_bf16) &&
                    ((((uintptr_t)d->dy | (uintptr_t)d->r | (uintptr_t)d->dr | (uintptr_t)d->dr_drop) & 15) == 0);
  if (fast) return hftt_launch<ln_bwd256_bf16_kernel>("ln_bwd", dim3(wgs), dim3(256), 0, (hipStream_t)stream, *d);
  if (d->N == 256 && ((((uintptr_t)d->dy | (uintptr_t)d->r | (uintptr_t)d->dr | (uintptr_t)d->dr_drop | (uintptr_t)d->gamma) & 15) == 0))
    return hftt_launch<ln_bwd256_rows_kernel<2, true>>("ln_bwd", dim3(wgs), dim3(256), 0, (hipStream_t)stream, *d);
  if (d->N == 256) return hftt_launch<ln_bwd_kernel<4>>("ln_bwd", dim3(wgs), dim3(256), 0, (hipStream_t)stream, *d);
  if (d->N == 128) return hftt_launch<ln_bwd_kernel<2>>("ln_bwd", dim3(wgs), dim3(256), 0, (hipStream_t)stream, *d);
  if (((((uintptr_t)d->dy | (uintptr_t)d->r | (uintptr_t)d->dr | (uintptr_t)d->dr_drop | (uintptr_t)d->gamma) & 15) == 0))
    return hftt_launch<ln_bwd64_kernel>("ln_bwd", dim3(wgs), dim3(256), 0, (hipStream_t)stream, *d);
  return hftt_launch<ln_bwd_kernel<1>>("ln_bwd", dim3(wgs), dim3(256), 0, (hipStream_t)stream, *d);
}
extern "C" int hftt_ln_bwd_reduce(const float* ws, int32_t n_wg, int32_t N, float* dgamma, float* dbeta, float beta, void* stream) {
  HFTT_REQUIRE(ws && dgamma && dbeta && n_wg > 0 && N > 0, "ln_bwd_reduce: bad arguments");
  return hftt_launch<ln_bwd_reduce_kernel>("ln_bwd_reduce", dim3((2 * N + 15) / 16), dim3(256), 0, (hipStream_t)stream, ws, n_wg, N, dgamma, dbeta, beta);
}
