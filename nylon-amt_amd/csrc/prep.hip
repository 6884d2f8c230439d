// Weight preparation of the hFT-Transformer path (gfx950): the parameter table copied into the layouts the GEMM kernels read (bf16, fp32 or
// the two 16-bit planes of the split form), the encoder-front fold (conv + flatten + linear as one matrix) with its backward, and the window
// materialisation of the spectrogram.  Entry points and reference citations: include/hftt_hip.h.
#include "hftt_common.h"
#include "x3_common.h"
#include "hftt_launch.h"
#include "../../include/hftt_hip.h"
#include <math.h>

namespace {

// one fp32 value -> the two 16-bit halves of the split ("x3") operand form
template <int E>
__device__ __forceinline__ void x3_split1(float x, uint16_t& hi, uint16_t& lo) {
  unsigned h, l;
  x3_split2_checked<E>(x, 0.f, h, l);      // (weight preparation: a NaN / Inf parameter must poison the planes)
  hi = (uint16_t)(h & 0xFFFFu); lo = (uint16_t)(l & 0xFFFFu);
}

// ------------------------------------------------------------------ weight preparation
__global__ void prep_weights_kernel(const float* __restrict__ params, uint16_t* __restrict__ wbf, float* __restrict__ wf32,
                                    float* __restrict__ fdst, const hftt_prep_entry* __restrict__ table) {
  const hftt_prep_entry e = table[blockIdx.x];
  const long total = (long)e.rows * e.cols;
  for (long i = (long)blockIdx.y * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.y * blockDim.x) {
    const int r = (int)(i / e.cols), c = (int)(i % e.cols);
    const float x = params[e.src_off + (long)r * e.src_ld + c];
    if (e.kind == 2) {
      fdst[e.dst_off + (long)r * e.dst_ld + c] = x;
    } else {
      const long d = (e.kind == 1) ? (e.dst_off + (long)c * e.dst_ld + r) : (e.dst_off + (long)r * e.dst_ld + c);
      if (wbf != nullptr) wbf[d] = f2bf(x);
      if (wf32 != nullptr) wf32[d] = x;
    }
  }
}

// the same table, matrices as two 16-bit planes (hi + lo ~ the fp32 value); e.pad = element type (2 fp16, 4 bf16)
__global__ void prep_weights_x3_kernel(const float* __restrict__ params, uint16_t* __restrict__ whi, uint16_t* __restrict__ wlo,
                                       float* __restrict__ fdst, const hftt_prep_entry* __restrict__ table) {
  const hftt_prep_entry e = table[blockIdx.x];
  const long total = (long)e.rows * e.cols;
  for (long i = (long)blockIdx.y * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.y * blockDim.x) {
    const int r = (int)(i / e.cols), c = (int)(i % e.cols);
    const float x = params[e.src_off + (long)r * e.src_ld + c];
    if (e.kind == 2) {
      fdst[e.dst_off + (long)r * e.dst_ld + c] = x;
    } else {
      const long d = (e.kind == 1) ? (e.dst_off + (long)c * e.dst_ld + r) : (e.dst_off + (long)r * e.dst_ld + c);
      uint16_t hi, lo;
      if (e.pad == X3_BF16) x3_split1<X3_BF16>(x, hi, lo); else x3_split1<X3_F16>(x, hi, lo);
      whi[d] = hi; wlo[d] = lo;
    }
  }
}

// ------------------------------------------------------------------ encoder front fold (conv + flatten + linear)
__global__ void fold_fwd_kernel(const hftt_fold_desc f) {
  const int nw = f.n_proc - f.kw + 1;
  const int cd = f.C * nw;
  const long total = (long)f.d_pad * f.Kp;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int j = (int)(i / f.Kp), u = (int)(i % f.Kp);
    float acc = 0.f;
    if (j < f.d && u < f.n_proc) {
      for (int c = 0; c < f.C; c++)
        for (int kk = 0; kk < f.kw; kk++) {
          const int w = u - kk;
          if (w >= 0 && w < nw) acc += f.wtok[(long)j * cd + c * nw + w] * f.wconv[c * f.kw + kk];
        }
    }
    if (f.weff_bf != nullptr) f.weff_bf[i] = f2bf(acc);
    if (f.weff_f32 != nullptr) f.weff_f32[i] = acc;
    if (f.weff_hi != nullptr) x3_split1<X3_F16>(acc, f.weff_hi[i], f.weff_lo[i]);
    if (u == 0 && j < f.d) {
      float b = f.btok[j];
      for (int c = 0; c < f.C; c++) {
        float s = 0.f;
        for (int w = 0; w < nw; w++) s += f.wtok[(long)j * cd + c * nw + w];
        b += f.bconv[c] * s;
      }
      f.beff[j] = b;
    }
  }
}

// grads of tok_embedding_freq.{weight,bias}
__global__ void fold_bwd_tok_kernel(const hftt_fold_desc f) {
  const int nw = f.n_proc - f.kw + 1;
  const int cd = f.C * nw;
  const long total = (long)f.d * cd;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int j = (int)(i / cd), cw = (int)(i % cd);
    const int c = cw / nw, w = cw % nw;
    float acc = f.dbeff[j] * f.bconv[c];
    for (int kk = 0; kk < f.kw; kk++) acc += f.dweff[(long)j * f.Kp + w + kk] * f.wconv[c * f.kw + kk];
    f.g_wtok[i] = acc;
    if (cw == 0) f.g_btok[j] = f.dbeff[j];
  }
}
// grads of conv.{weight,bias}: one workgroup per (c,kk) plus one per c for the bias
__global__ __launch_bounds__(256) void fold_bwd_conv_kernel(const hftt_fold_desc f) {
  __shared__ float red[256];
  const int nw = f.n_proc - f.kw + 1;
  const int cd = f.C * nw;
  const int b = blockIdx.x;
  const bool is_bias = b >= f.C * f.kw;
  const int c = is_bias ? (b - f.C * f.kw) : (b / f.kw);
  const int kk = is_bias ? 0 : (b % f.kw);
  float acc = 0.f;
  for (int i = threadIdx.x; i < f.d * nw; i += 256) {
    const int j = i / nw, w = i % nw;
    const float wt = f.wtok[(long)j * cd + c * nw + w];
    acc += is_bias ? f.dbeff[j] * wt : f.dweff[(long)j * f.Kp + w + kk] * wt;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (is_bias) f.g_bconv[c] = red[0];
    else f.g_wconv[c * f.kw + kk] = red[0];
  }
}

// A[(b,t,f), u] = spec[b, f, t+u]
__global__ void im2win_kernel(const float* __restrict__ spec, float* __restrict__ win, int B, int F, int T, int n_proc, int Kp) {
  const int W = T + n_proc - 1;
  const int q4 = Kp / 4;
  const long total = (long)B * T * F * q4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int u4 = (int)(i % q4);
    const long row = i / q4;
    const int f = (int)(row % F);
    const int t = (int)((row / F) % T);
    const int b = (int)(row / ((long)F * T));
    const float* src = spec + ((long)b * F + f) * W + t;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int u = u4 * 4 + e;
      v[e] = (u < n_proc) ? src[u] : 0.f;
    }
    *reinterpret_cast<float4*>(win + row * Kp + u4 * 4) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

}  // namespace

extern "C" int hftt_prep_weights(const float* params, uint16_t* wbf, float* wf32, float* fdst,
                                 const hftt_prep_entry* table_dev, int n_entries, void* stream) {
  HFTT_REQUIRE(params && (wbf || wf32 || fdst) && table_dev && n_entries > 0, "prep_weights: null operand");
  return hftt_launch<prep_weights_kernel>("prep_weights", dim3((unsigned)n_entries, 48), dim3(256), 0, (hipStream_t)stream, params, wbf, wf32, fdst, table_dev);
}

extern "C" int hftt_prep_weights_x3(const float* params, uint16_t* whi, uint16_t* wlo, float* fdst,
                                    const hftt_prep_entry* table_dev, int n_entries, void* stream) {
  HFTT_REQUIRE(params && whi && wlo && table_dev && n_entries > 0, "prep_weights_x3: null operand");
  return hftt_launch<prep_weights_x3_kernel>("prep_weights_x3", dim3((unsigned)n_entries, 48), dim3(256), 0, (hipStream_t)stream, params, whi, wlo, fdst, table_dev);
}

extern "C" int hftt_embed_fold_fwd(const hftt_fold_desc* d, void* stream) {
  HFTT_REQUIRE(d && d->wconv && d->bconv && d->wtok && d->btok && (d->weff_bf || d->weff_f32 || d->weff_hi) && d->beff, "embed_fold_fwd: null operand");
  HFTT_REQUIRE((d->weff_hi == nullptr) == (d->weff_lo == nullptr), "embed_fold_fwd: the split planes come as a pair");
  HFTT_REQUIRE(d->Kp % 32 == 0 && d->Kp >= d->n_proc && d->d_pad >= d->d && d->n_proc >= d->kw, "embed_fold_fwd: bad shape");
  return hftt_launch<fold_fwd_kernel>("embed_fold_fwd", dim3(grid_for((long)d->d_pad * d->Kp, 256)), dim3(256), 0, (hipStream_t)stream, *d);
}
extern "C" int hftt_embed_fold_bwd(const hftt_fold_desc* d, void* stream) {
  HFTT_REQUIRE(d && d->dweff && d->dbeff && d->g_wconv && d->g_bconv && d->g_wtok && d->g_btok, "embed_fold_bwd: null operand");
  const int nw = d->n_proc - d->kw + 1;
  if (int rc = hftt_launch<fold_bwd_tok_kernel>("embed_fold_bwd(tok)", dim3(grid_for((long)d->d * d->C * nw, 256)), dim3(256), 0, (hipStream_t)stream, *d)) return rc;
  return hftt_launch<fold_bwd_conv_kernel>("embed_fold_bwd(conv)", dim3((unsigned)(d->C * d->kw + d->C)), dim3(256), 0, (hipStream_t)stream, *d);
}
extern "C" int hftt_im2win(const float* spec, float* win, int32_t B, int32_t F, int32_t T, int32_t n_proc, int32_t Kp, void* stream) {
  HFTT_REQUIRE(spec && win && B > 0 && F > 0 && T > 0 && n_proc > 0 && Kp % 4 == 0 && Kp >= n_proc, "im2win: bad arguments");
  return hftt_launch<im2win_kernel>("im2win", dim3(grid_for((long)B * T * F * (Kp / 4), 256, 8192)), dim3(256), 0, (hipStream_t)stream, spec, win, B, F, T, n_proc, Kp);
}
