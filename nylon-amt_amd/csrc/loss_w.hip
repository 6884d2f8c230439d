// Fused loss with class-balanced and focal criteria (gfx950): hftt_loss's 6x BCE + 2x CE pass with a per-pitch positive weight and a focal
// modulation on the BCE heads and class weights, ignore_index and label smoothing on the velocity cross-entropy.  Definitions, the W = 0
// deviation from torch and the launch count: include/hftt_hip.h.  loss.hip is not touched; its half-wave helpers are restated here because
// they live in that file's anonymous namespace.
//
// Neutrality, bit for bit: a head (a side) whose options are neutral produces hftt_loss's bits.  The compiler is free to contract a * b + c
// differently in two kernels, so contraction is OFF in this file and the roundings hftt_loss's kernels perform are written out: the BCE value
// as two rounded products, their sum, and a subtraction from the running part; the CE gradient as fma(ex, 1 / s, -onehot) times the scale;
// the total as fma(weight_A, la, weight_B * lb).  With a == 1, gamma == 0, eps == 0 and W == (float)n every extra factor is an exact 1 or 0.
#include "hftt_common.h"
#include "hftt_launch.h"
#include "../../include/hftt_hip.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int LOSSW_WGS = 4096;      // workgroups of the main pass (as hftt_loss: the same workspace size, the same reduce order)
constexpr int PRE_WGS = 256;         // workgroups of the label pre-pass: one partial pair per thread of the 256-thread blocks that sum them

// what every kernel of this file needs beyond the descriptor: which sides take W from the pre-pass (bit s), and its workgroup count
struct LossWArgs {
  hftt_loss_w_desc d;
  int pre_mask;
  int n_pre;
};

__device__ __forceinline__ float hw_sum(float v) {      // over the 32 lanes of a half wave (loss.hip: half_sum)
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64);
  return v;
}
__device__ __forceinline__ float hw_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64));
  v = fmaxf(v, __shfl_xor(v, 8, 64)); v = fmaxf(v, __shfl_xor(v, 16, 64));
  return v;
}

// ------------------------------------------------------------------ W_s = sum over the rows that count of w[c_i]
// Pre-pass: every thread adds its labels' weights in index order, then lanes, waves -- a fixed tree, no atomics.  A label that is ignored or
// outside [0, V) counts 0 (it is never used as an index).
__global__ __launch_bounds__(256) void loss_w_pre_kernel(const LossWArgs a) {
  __shared__ float red[4][2];
  const hftt_loss_w_desc& g = a.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float w0 = 0.f, w1 = 0.f;
  for (long el = (long)blockIdx.x * 256 + threadIdx.x; el < g.base.n; el += (long)gridDim.x * 256) {
    const long lab = g.base.label_velocity[el];
    const bool in = lab >= 0 && lab < g.base.V;
    if (lab != g.ignore_index[0] && in) w0 += g.class_weight[0] != nullptr ? g.class_weight[0][lab] : 1.f;
    if (lab != g.ignore_index[1] && in) w1 += g.class_weight[1] != nullptr ? g.class_weight[1][lab] : 1.f;
  }
  w0 = wave_sum(w0); w1 = wave_sum(w1);
  if (lane == 0) { red[wave][0] = w0; red[wave][1] = w1; }
  __syncthreads();
  if (threadIdx.x < 2) g.ws_w[(long)blockIdx.x * 2 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
// The pre-pass partials summed by one 256-thread block in a fixed order: every workgroup of the main pass and the reduce launch form the same
// bits.  A side outside pre_mask has W = (float)n, hftt_loss's divisor.  Ends with a barrier (red may be reused).
__device__ __forceinline__ void loss_w_total(const LossWArgs& a, float (*red)[2], float& WA, float& WB) {
  const float nf = (float)a.d.base.n;
  WA = nf; WB = nf;
  if (a.pre_mask == 0) return;                          // (uniform)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float w0 = 0.f, w1 = 0.f;
  if ((int)threadIdx.x < a.n_pre) { w0 = a.d.ws_w[2 * threadIdx.x]; w1 = a.d.ws_w[2 * threadIdx.x + 1]; }
  w0 = wave_sum(w0); w1 = wave_sum(w1);
  if (lane == 0) { red[wave][0] = w0; red[wave][1] = w1; }
  __syncthreads();
  if (a.pre_mask & 1) WA = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
  if (a.pre_mask & 2) WB = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
  __syncthreads();
}

// ------------------------------------------------------------------ one BCE head, one element
struct BceHead {
  const float* p; const float* y; float* d; const float* pw;
  float gamma, scale;      // scale = weight_A|B / n * grad_scale, formed as hftt_loss forms it
};
__device__ __forceinline__ BceHead bce_head(const hftt_loss_w_desc& g, int h, float inv_n) {
  BceHead b;
  b.p = g.base.prob[h];
  b.y = (h % 3 == 0) ? g.base.label_onset : ((h % 3 == 1) ? g.base.label_offset : g.base.label_mpe);
  b.d = g.base.d_prob[h];
  b.pw = g.pos_weight[h];
  b.gamma = g.gamma[h];
  b.scale = ((h < 3) ? g.base.weight_A : g.base.weight_B) * inv_n * g.base.grad_scale;
  return b;
}
// part -= m * (a y lp + (1 - y) l1p); the gradient is stored when the head has one.  a == 1 and gamma == 0: hftt_loss's roundings.
__device__ __forceinline__ void bce_element(const BceHead& b, long el, int Nn, float& part) {
  const float p = b.p[el], y = b.y[el];
  float a = 1.f;
  if (b.pw != nullptr) a = b.pw[el < 0x7fffffffL ? (long)((unsigned)el % (unsigned)Nn) : el % Nn];
  const float lp = fmaxf(logf(p), -100.f), l1p = fmaxf(log1pf(-p), -100.f);
  const float t1 = (a * y) * lp, t2 = (1.f - y) * l1p;
  const float nbase = t1 + t2;                                       // -base
  const float num = (p - y) - ((a - 1.f) * y) * (1.f - p);
  const float den = fmaxf((1.f - p) * p, 1e-12f);
  if (b.gamma == 0.f) {
    part = part - nbase;
    if (b.d != nullptr) b.d[el] = num / den * b.scale;
    return;
  }
  // m = |y - p|^gamma = |y - p| * |y - p|^(gamma - 1); logf(0) = -inf and expf(-inf) = 0 carry |y - p| = 0 through (gamma == 1: no 0 * inf)
  const float df = y - p, ad = fabsf(df);
  const float m1 = (b.gamma == 1.f) ? 1.f : expf((b.gamma - 1.f) * logf(ad));
  const float m = ad * m1;
  part = part - m * nbase;
  if (b.d != nullptr) {
    const float sg = (df > 0.f) ? 1.f : ((df < 0.f) ? -1.f : 0.f);
    b.d[el] = ((m * num) / den + nbase * ((b.gamma * m1) * sg)) * b.scale;
  }
}

// ------------------------------------------------------------------ per-side constants of the cross-entropy
struct CeSide {
  float omeps, epsV, wfac;      // 1 - eps; eps / V; weight_A|B / W * grad_scale (0 when W == 0)
  bool on;                      // W > 0
};
__device__ __forceinline__ CeSide ce_side(const hftt_loss_w_desc& g, int side, float W) {
  CeSide c;
  c.on = W > 0.f;
  c.omeps = 1.f - g.smoothing[side];
  c.epsV = g.smoothing[side] / (float)g.base.V;
  const float inv_W = c.on ? 1.0f / W : 0.f;
  c.wfac = (side == 0 ? g.base.weight_A : g.base.weight_B) * inv_W * g.base.grad_scale;
  return c;
}

// ------------------------------------------------------------------ general form (any V <= 256, any alignment): one wave per element
// CEW: some side has class weights or smoothing (decided on the host).  Without, the class-weight registers, their sums and the smoothing
// branches are compiled out: the neutral and the BCE-only call keep hftt_loss's register budget.
template <bool CEW>
__global__ __launch_bounds__(256) void loss_w_kernel(const LossWArgs a) {
  __shared__ float red[4][8];
  __shared__ float redw[4][2];
  const hftt_loss_w_desc& g = a.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long n = g.base.n;
  const int V = g.base.V;
  float W[2];
  loss_w_total(a, redw, W[0], W[1]);
  const float inv_n = 1.0f / (float)n;
  const BceHead bh = bce_head(g, lane < 6 ? lane : 0, inv_n);
  CeSide cs[2] = {ce_side(g, 0, W[0]), ce_side(g, 1, W[1])};
  float cw[2][4], sumw[2];      // this lane's class weights (classes lane + 64 e), loop-invariant, and their sum over the classes
#pragma unroll
  for (int side = 0; side < 2; side++) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int c = lane + 64 * e;
      cw[side][e] = (c < V) ? (CEW && g.class_weight[side] != nullptr ? g.class_weight[side][c] : 1.f) : 0.f;
      s += cw[side][e];
    }
    sumw[side] = wave_sum(s);
  }
  float part = 0.f;    // lanes 0..5: BCE terms; lanes 6,7: CE terms (A, B)
  for (long el = (long)blockIdx.x * 4 + wave; el < n; el += (long)gridDim.x * 4) {
    if (lane < 6) bce_element(bh, el, g.Nn, part);
    const long lab = g.base.label_velocity[el];
    const int label = (int)lab;
#pragma unroll
    for (int side = 0; side < 2; side++) {
      const float* lg = g.base.vel[side] + el * V;
      float v[4], mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int c = lane + 64 * e;
        v[e] = (c < V) ? lg[c] : -INFINITY;
        mx = fmaxf(mx, v[e]);
      }
      mx = wave_max(mx);
      float s = 0.f, ex[4];
#pragma unroll
      for (int e = 0; e < 4; e++) { ex[e] = (lane + 64 * e < V) ? expf(v[e] - mx) : 0.f; s += ex[e]; }
      s = wave_sum(s);
      const float lse = mx + logf(s);
      float picked = 0.f, wl = 0.f;
#pragma unroll
      for (int e = 0; e < 4; e++) if (lane + 64 * e == label) { picked = v[e]; wl = cw[side][e]; }
      picked = wave_sum(picked);
      if (CEW && g.class_weight[side] != nullptr) wl = wave_sum(wl); else wl = 1.f;
      const bool live = cs[side].on && lab != g.ignore_index[side];
      const float coef = cs[side].omeps * wl;
      float row = coef * (lse - picked);
      if (CEW && cs[side].epsV != 0.f) {                // (uniform)
        float sw = 0.f;
#pragma unroll
        for (int e = 0; e < 4; e++) if (lane + 64 * e < V) sw += cw[side][e] * (lse - v[e]);
        row = row + cs[side].epsV * wave_sum(sw);
      }
      if (lane == 6 + side && live) part += row;
      if (g.base.d_vel[side] != nullptr) {
        float* dst = g.base.d_vel[side] + el * V;
        const float inv_s = 1.0f / s;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int c = lane + 64 * e;
          if (c < V) {
            float o = __builtin_fmaf(ex[e], inv_s, c == label ? -1.f : -0.f) * coef;
            if (CEW && cs[side].epsV != 0.f) o = o + cs[side].epsV * ((ex[e] * inv_s) * sumw[side] - cw[side][e]);
            dst[c] = live ? o * cs[side].wfac : 0.f;
          }
        }
      }
    }
  }
  if (lane < 8) red[wave][lane] = part;
  __syncthreads();
  if (threadIdx.x < 8) g.base.ws[(long)blockIdx.x * 8 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// ------------------------------------------------------------------ half-wave form (V <= 128, V % 4 == 0, aligned): 16-byte loads and stores
template <bool CEW>
__global__ __launch_bounds__(256) void loss_w_v4_kernel(const LossWArgs a) {
  __shared__ float red[4][8];
  __shared__ float redw[4][2];
  const hftt_loss_w_desc& g = a.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l32 = lane & 31, hf = lane >> 5;
  const long n = g.base.n;
  const int V = g.base.V;
  float W[2];
  loss_w_total(a, redw, W[0], W[1]);
  const float inv_n = 1.0f / (float)n;
  const BceHead bh = bce_head(g, l32 < 6 ? l32 : 0, inv_n);
  CeSide cs[2] = {ce_side(g, 0, W[0]), ce_side(g, 1, W[1])};
  const int c0 = 4 * l32;
  const bool cok = c0 < V;
  float4 cw[2];                 // this lane's four class weights, loop-invariant (four 4-byte loads, once: the table needs no alignment)
  float sumw[2];
#pragma unroll
  for (int side = 0; side < 2; side++) {
    cw[side] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cok) {
      const float* t = g.class_weight[side];
      cw[side] = (CEW && t != nullptr) ? make_float4(t[c0], t[c0 + 1], t[c0 + 2], t[c0 + 3]) : make_float4(1.f, 1.f, 1.f, 1.f);
    }
    sumw[side] = hw_sum((cw[side].x + cw[side].y) + (cw[side].z + cw[side].w));
  }
  float part = 0.f;    // per half: lanes 0..5 BCE terms; lanes 6,7 CE terms (A, B)
  for (long el0 = ((long)blockIdx.x * 4 + wave) * 2; el0 < n; el0 += (long)gridDim.x * 8) {
    const long el = el0 + hf;
    const bool ok = el < n;                         // (odd n: the second half of the last pair idles, but takes part in the shuffles)
    const long elc = ok ? el : n - 1;
    if (l32 < 6 && ok) bce_element(bh, el, g.Nn, part);
    const long lab = g.base.label_velocity[elc];
    const int label = (int)lab;
    const int k = label - c0;
#pragma unroll
    for (int side = 0; side < 2; side++) {
      const float* lg = g.base.vel[side] + elc * V;
      float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      if (cok) v = *reinterpret_cast<const float4*>(lg + c0);
      const float mx = hw_max(fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
      float4 ex = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cok) ex = make_float4(expf(v.x - mx), expf(v.y - mx), expf(v.z - mx), expf(v.w - mx));
      const float s = hw_sum((ex.x + ex.y) + (ex.z + ex.w));
      const float lse = mx + logf(s);
      float picked = (k == 0) ? v.x : (k == 1) ? v.y : (k == 2) ? v.z : (k == 3) ? v.w : 0.f;
      picked = hw_sum(picked);
      float wl = 1.f;
      if (CEW && g.class_weight[side] != nullptr)       // (uniform)
        wl = hw_sum((k == 0) ? cw[side].x : (k == 1) ? cw[side].y : (k == 2) ? cw[side].z : (k == 3) ? cw[side].w : 0.f);
      const bool live = cs[side].on && lab != g.ignore_index[side];
      const float coef = cs[side].omeps * wl;
      float row = coef * (lse - picked);
      if (CEW && cs[side].epsV != 0.f) {                // (uniform)
        float sw = 0.f;
        if (cok) sw = (cw[side].x * (lse - v.x) + cw[side].y * (lse - v.y)) + (cw[side].z * (lse - v.z) + cw[side].w * (lse - v.w));
        row = row + cs[side].epsV * hw_sum(sw);
      }
      if (l32 == 6 + side && ok && live) part += row;
      if (g.base.d_vel[side] != nullptr && cok && ok) {
        const float inv_s = 1.0f / s;
        float4 o;
        o.x = __builtin_fmaf(ex.x, inv_s, k == 0 ? -1.f : -0.f) * coef; o.y = __builtin_fmaf(ex.y, inv_s, k == 1 ? -1.f : -0.f) * coef;
        o.z = __builtin_fmaf(ex.z, inv_s, k == 2 ? -1.f : -0.f) * coef; o.w = __builtin_fmaf(ex.w, inv_s, k == 3 ? -1.f : -0.f) * coef;
        if (CEW && cs[side].epsV != 0.f) {
          const float e = cs[side].epsV, sm = sumw[side];
          o.x = o.x + e * ((ex.x * inv_s) * sm - cw[side].x); o.y = o.y + e * ((ex.y * inv_s) * sm - cw[side].y);
          o.z = o.z + e * ((ex.z * inv_s) * sm - cw[side].z); o.w = o.w + e * ((ex.w * inv_s) * sm - cw[side].w);
        }
        const float f = cs[side].wfac;
        o = live ? make_float4(o.x * f, o.y * f, o.z * f, o.w * f) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(g.base.d_vel[side] + el * V + c0) = o;
      }
    }
  }
  part += __shfl_xor(part, 32, 64);                 // the two halves' terms
  if (lane < 8) red[wave][lane] = part;
  __syncthreads();
  if (threadIdx.x < 8) g.base.ws[(long)blockIdx.x * 8 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// ------------------------------------------------------------------ reduce: loss_reduce_kernel's order; the CE terms divided by W_s
__global__ __launch_bounds__(256) void loss_w_reduce_kernel(const LossWArgs a, int n_wg) {
  __shared__ float red[32][8];
  __shared__ float redw[4][2];
  const hftt_loss_desc& g = a.d.base;
  float WA, WB;
  loss_w_total(a, redw, WA, WB);
  const int term = threadIdx.x & 7, grp = threadIdx.x >> 3;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;      // four independent chains (fixed order: the sum is reproducible), loads in flight together
  int w = grp;
  for (; w + 96 < n_wg; w += 128) {
    const float v0 = g.ws[(long)w * 8 + term], v1 = g.ws[(long)(w + 32) * 8 + term], v2 = g.ws[(long)(w + 64) * 8 + term], v3 = g.ws[(long)(w + 96) * 8 + term];
    a0 += v0; a1 += v1; a2 += v2; a3 += v3;
  }
  for (; w < n_wg; w += 32) a0 += g.ws[(long)w * 8 + term];
  red[grp][term] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (threadIdx.x < 8) {
    float s = 0.f;
    for (int q = 0; q < 32; q++) s += red[q][threadIdx.x];
    const float div = (threadIdx.x == 6) ? WA : ((threadIdx.x == 7) ? WB : (float)g.n);
    red[0][threadIdx.x] = (div > 0.f) ? s / div : 0.f;           // W == 0: the term is 0 (torch: NaN)
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // order of loss_out[1..8]: onset_A, offset_A, mpe_A, velocity_A, onset_B, offset_B, mpe_B, velocity_B; [9], [10]: W_A, W_B
    const float t[8] = {red[0][0], red[0][1], red[0][2], red[0][6], red[0][3], red[0][4], red[0][5], red[0][7]};
    float la = (t[0] + t[1]) + t[2];
    la += t[3];
    float lb = (t[4] + t[5]) + t[6];
    lb += t[7];
    g.loss_out[0] = __builtin_fmaf(g.weight_A, la, g.weight_B * lb);
    for (int i = 0; i < 8; i++) g.loss_out[1 + i] = t[i];
    g.loss_out[9] = WA;
    g.loss_out[10] = WB;
  }
}

}  // namespace

extern "C" int64_t hftt_loss_w_ws_bytes(int64_t n) { (void)n; return (int64_t)PRE_WGS * 2 * 4; }
extern "C" int hftt_loss_w(const hftt_loss_w_desc* dw, void* stream) {
  HFTT_REQUIRE(dw != nullptr, "loss_w: null descriptor");
  const hftt_loss_desc* d = &dw->base;
  HFTT_REQUIRE(d->n > 0 && d->V > 0 && d->V <= 256, "loss_w: bad shape");
  for (int i = 0; i < 6; i++) HFTT_REQUIRE(d->prob[i] != nullptr, "loss_w: null probability tensor %d", i);
  HFTT_REQUIRE(d->vel[0] && d->vel[1] && d->label_onset && d->label_offset && d->label_mpe && d->label_velocity && d->loss_out && d->ws, "loss_w: null operand");
  HFTT_REQUIRE(dw->Nn > 0, "loss_w: Nn=%d must be positive", dw->Nn);
  HFTT_REQUIRE(d->n % dw->Nn == 0, "loss_w: n=%lld must be a multiple of Nn=%d", (long long)d->n, dw->Nn);
  for (int i = 0; i < 6; i++)
    HFTT_REQUIRE(dw->gamma[i] == 0.f || (dw->gamma[i] >= 1.f && dw->gamma[i] <= 4.f), "loss_w: head %d: gamma=%g must be 0 or in [1, 4]", i, (double)dw->gamma[i]);
  int pre_mask = 0;
  bool cew = false;
  for (int s = 0; s < 2; s++) {
    HFTT_REQUIRE(dw->smoothing[s] >= 0.f && dw->smoothing[s] < 1.f, "loss_w: side %d: smoothing=%g must be in [0, 1)", s, (double)dw->smoothing[s]);
    // a side needs the pre-pass when a label can weigh other than 1: class weights, or an ignore_index that a label can take
    cew = cew || dw->class_weight[s] != nullptr || dw->smoothing[s] != 0.f;
    if (dw->class_weight[s] != nullptr || (dw->ignore_index[s] >= 0 && dw->ignore_index[s] < d->V)) pre_mask |= 1 << s;
  }
  HFTT_REQUIRE(pre_mask == 0 || dw->ws_w != nullptr, "loss_w: the pre-pass workspace ws_w is null (class weights or an ignore_index inside [0, V) need it)");
  LossWArgs a;
  a.d = *dw;
  a.pre_mask = pre_mask;
  a.n_pre = grid_for(d->n, 256, PRE_WGS);
  hipStream_t st = (hipStream_t)stream;
  if (pre_mask != 0)
    if (int rc = hftt_launch<loss_w_pre_kernel>("loss_w_pre", dim3(a.n_pre), dim3(256), 0, st, a)) return rc;
  int wgs = (int)((d->n + 3) / 4);
  const bool v4 = d->V <= 128 && d->V % 4 == 0 && (((uintptr_t)d->vel[0] | (uintptr_t)d->vel[1] | (uintptr_t)d->d_vel[0] | (uintptr_t)d->d_vel[1]) & 15) == 0;
  if (v4) wgs = (int)((d->n + 7) / 8);
  if (wgs > LOSSW_WGS) wgs = LOSSW_WGS;
  int rc;
  if (v4) rc = cew ? hftt_launch<loss_w_v4_kernel<true>>("loss_w", dim3(wgs), dim3(256), 0, st, a) : hftt_launch<loss_w_v4_kernel<false>>("loss_w", dim3(wgs), dim3(256), 0, st, a);
  else rc = cew ? hftt_launch<loss_w_kernel<true>>("loss_w", dim3(wgs), dim3(256), 0, st, a) : hftt_launch<loss_w_kernel<false>>("loss_w", dim3(wgs), dim3(256), 0, st, a);
  if (rc) return rc;
  return hftt_launch<loss_w_reduce_kernel>("loss_w_reduce", dim3(1), dim3(256), 0, st, a, wgs);
}
