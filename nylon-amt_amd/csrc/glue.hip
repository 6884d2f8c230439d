// HBM-bound glue kernels of the hFT-Transformer path (gfx950): the decoder time transpose (+scale, +pos, dropout) and its backward, the dropout
// backward, the two-stage column sums (deterministic, no float atomics) and the split of the output heads.  They stream 16-byte accesses
// where the layout allows.  Entry points and reference citations: include/hftt_hip.h.
#include "hftt_common.h"
#include "hftt_launch.h"
#include "../../include/hftt_hip.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------ decoder time transpose (+scale, +pos, dropout)
__global__ void time_embed_fwd_kernel(const float* __restrict__ x, const float* __restrict__ pos, float* __restrict__ y,
                                      int B, int T, int Nn, int d, float scale, float drop_p, uint32_t site, uint64_t seed, uint32_t io_flags) {
  const bool x_bf = io_flags & HFTT_TE_X_BF16, y_bf = io_flags & HFTT_TE_Y_BF16;
  const int d4 = d / 4;
  const long total = (long)B * Nn * T * d4;
  const uint32_t thr = hftt_keep_thr(drop_p);
  const float inv_keep = hftt_keep_scale(drop_p);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % d4);
    const long orow = i / d4;                      // (b*Nn + n)*T + t
    const int t = (int)(orow % T);
    const int n = (int)((orow / T) % Nn);
    const int b = (int)(orow / ((long)T * Nn));
    const long irow = ((long)b * T + t) * Nn + n;
    const float4 a = hftt_load4(x, x_bf, irow * d + c4 * 4);
    const float4 p = *reinterpret_cast<const float4*>(pos + (long)t * d + c4 * 4);
    float v[4] = {a.x * scale + p.x, a.y * scale + p.y, a.z * scale + p.z, a.w * scale + p.w};
    if (drop_p > 0.f) {
#pragma unroll
      for (int e = 0; e < 4; e++) v[e] = hftt_keep(seed, site, (uint64_t)(orow * d + c4 * 4 + e), thr) ? v[e] * inv_keep : 0.f;
    }
    hftt_store4(y, y_bf, orow * d + c4 * 4, v[0], v[1], v[2], v[3]);
  }
}
__global__ void time_embed_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, float* __restrict__ dym,
                                      int B, int T, int Nn, int d, float scale, float drop_p, uint32_t site, uint64_t seed, int accumulate, uint32_t io_flags) {
  const bool dy_bf = io_flags & HFTT_TE_X_BF16, dx_bf = io_flags & HFTT_TE_Y_BF16, dym_bf = io_flags & HFTT_TE_M_BF16;
  const int d4 = d / 4;
  const long total = (long)B * Nn * T * d4;
  const uint32_t thr = hftt_keep_thr(drop_p);
  const float inv_keep = hftt_keep_scale(drop_p);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % d4);
    const long orow = i / d4;
    const int t = (int)(orow % T);
    const int n = (int)((orow / T) % Nn);
    const int b = (int)(orow / ((long)T * Nn));
    const long irow = ((long)b * T + t) * Nn + n;
    const float4 a = hftt_load4(dy, dy_bf, orow * d + c4 * 4);
    float v[4] = {a.x, a.y, a.z, a.w};
    if (drop_p > 0.f) {
#pragma unroll
      for (int e = 0; e < 4; e++) v[e] = hftt_keep(seed, site, (uint64_t)(orow * d + c4 * 4 + e), thr) ? v[e] * inv_keep : 0.f;
    }
    if (dym != nullptr) hftt_store4(dym, dym_bf, orow * d + c4 * 4, v[0], v[1], v[2], v[3]);
    float4 o = make_float4(v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale);
    if (accumulate) { const float4 old = hftt_load4(dx, dx_bf, irow * d + c4 * 4); o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w; }
    hftt_store4(dx, dx_bf, irow * d + c4 * 4, o.x, o.y, o.z, o.w);
  }
}
__global__ void dropout_bwd_kernel(float* __restrict__ gbuf, long n, float drop_p, uint32_t site, uint64_t seed, uint32_t bf) {
  const uint32_t thr = hftt_keep_thr(drop_p);
  const float inv_keep = hftt_keep_scale(drop_p);
  const long n4 = n >> 2;                          // n % 4 == 0 (host check): 4 consecutive elements = one hash quad per thread
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 a = hftt_load4(gbuf, bf, i * 4);
    float v[4] = {a.x, a.y, a.z, a.w};
    const uint32_t k4 = hftt_keep_quad(seed, site, (uint64_t)i, thr);
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = ((k4 >> e) & 1u) ? v[e] * inv_keep : 0.f;
    hftt_store4(gbuf, bf, i * 4, v[0], v[1], v[2], v[3]);
  }
}

// ------------------------------------------------------------------ column sums (two-stage)
constexpr int CS_SPLITS = 16;
__global__ void colsum_stage1_kernel(const float* __restrict__ x, long rows, long n, long ld, float* __restrict__ ws, uint32_t bf) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int sp = blockIdx.y;
  const long per = (rows + CS_SPLITS - 1) / CS_SPLITS;
  const long r0 = sp * per;
  long r1 = r0 + per; if (r1 > rows) r1 = rows;
  float acc = 0.f;
  if (bf) { for (long r = r0; r < r1; r++) acc += bf2f(reinterpret_cast<const unsigned short*>(x)[r * ld + j]); }
  else { for (long r = r0; r < r1; r++) acc += x[r * ld + j]; }
  ws[(long)sp * n + j] = acc;
}
// Stage 1 with the dropout backward in it: the same 16 row splits and the same row order per column as colsum_stage1_kernel, one quad of
// columns per thread.  A quad is read once, masked by its site's keep decisions (one hash per quad: the element index is its offset r * ld + j
// in the buffer, as dropout_bwd_kernel counts it), written back in place and added -- as the value that was stored, so a bf16 buffer adds its
// rounding and the product never fuses into the sum.  DCS_RB rows are in flight per thread: the loads may not pass the stores of the same
// buffer on their own.  drop_p == 0: nothing is masked or written.
constexpr int DCS_RB = 8;
__global__ __launch_bounds__(256) void dropout_bwd_colsum_stage1_kernel(float* gbuf, long rows, long n, long ld, float drop_p, uint32_t site, uint64_t seed,
                                                                        float* __restrict__ ws, uint32_t bf) {
  const long j = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (j >= n) return;                               // n % 4 == 0 (host check): a quad is inside the row or outside it
  const uint32_t thr = hftt_keep_thr(drop_p);
  const float inv_keep = hftt_keep_scale(drop_p);
  const bool mask = drop_p > 0.f;
  const int sp = blockIdx.y;
  const long per = (rows + CS_SPLITS - 1) / CS_SPLITS;
  const long r0 = sp * per;
  long r1 = r0 + per; if (r1 > rows) r1 = rows;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (long r = r0; r < r1; r += DCS_RB) {
    float4 a[DCS_RB];
#pragma unroll
    for (int u = 0; u < DCS_RB; u++) {              // unconditional, from a clamped row
      const long rc = r + u < r1 ? r + u : r1 - 1;
      a[u] = hftt_load4(gbuf, bf, rc * ld + j);
    }
#pragma unroll
    for (int u = 0; u < DCS_RB; u++) {
      if (r + u < r1) {
        const long off = (r + u) * ld + j;
        float v[4] = {a[u].x, a[u].y, a[u].z, a[u].w};
        if (mask) {
          const uint32_t k4 = hftt_keep_quad(seed, site, (uint64_t)off >> 2, thr);
#pragma unroll
          for (int e = 0; e < 4; e++) v[e] = ((k4 >> e) & 1u) ? __fmul_rn(v[e], inv_keep) : 0.f;
          hftt_store4(gbuf, bf, off, v[0], v[1], v[2], v[3]);
          if (bf) {
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = bf2f(f2bf(v[e]));
          }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) acc[e] += v[e];
      }
    }
  }
  *reinterpret_cast<float4*>(ws + (long)sp * n + j) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}
__global__ void colsum_stage2_kernel(const float* __restrict__ ws, long n, float* __restrict__ out, float beta) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  float acc = 0.f;
#pragma unroll
  for (int s = 0; s < CS_SPLITS; s++) acc += ws[(long)s * n + j];
  out[j] = (beta != 0.f) ? (out[j] * beta + acc) : acc;
}

// ------------------------------------------------------------------ output heads
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ void heads_split_kernel(const float* __restrict__ logits, long ldl, float* __restrict__ onset, float* __restrict__ offset,
                                   float* __restrict__ mpe, float* __restrict__ velocity, int B, int T, int Nn, int V, int time_major) {
  const int v4 = V / 4;
  const long total = (long)B * T * Nn * v4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % v4);
    const long s = i / v4;
    long o = s;
    if (time_major) {
      const int t = (int)(s % T);
      const int n = (int)((s / T) % Nn);
      const int b = (int)(s / ((long)T * Nn));
      o = ((long)b * T + t) * Nn + n;
    }
    *reinterpret_cast<float4*>(velocity + o * V + c4 * 4) = *reinterpret_cast<const float4*>(logits + s * ldl + c4 * 4);
    if (c4 == 0) {
      onset[o] = sigmoidf_(logits[s * ldl + V]);
      offset[o] = sigmoidf_(logits[s * ldl + V + 1]);
      mpe[o] = sigmoidf_(logits[s * ldl + V + 2]);
    }
  }
}
__global__ void heads_split_bwd_kernel(const float* __restrict__ p_on, const float* __restrict__ p_of, const float* __restrict__ p_mp,
                                       const float* __restrict__ d_on, const float* __restrict__ d_of, const float* __restrict__ d_mp,
                                       const float* __restrict__ d_vel, float* __restrict__ dlogits, long ldl,
                                       int B, int T, int Nn, int V, int time_major) {
  const int l4 = (int)(ldl / 4);
  const int v4 = V / 4;
  const long total = (long)B * T * Nn * l4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % l4);
    const long s = i / l4;
    long o = s;
    if (time_major) {
      const int t = (int)(s % T);
      const int n = (int)((s / T) % Nn);
      const int b = (int)(s / ((long)T * Nn));
      o = ((long)b * T + t) * Nn + n;
    }
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < v4) {
      v = *reinterpret_cast<const float4*>(d_vel + o * V + c4 * 4);
    } else if (c4 == v4) {
      const float a = p_on[o], b2 = p_of[o], c = p_mp[o];
      v.x = d_on[o] * a * (1.f - a);
      v.y = d_of[o] * b2 * (1.f - b2);
      v.z = d_mp[o] * c * (1.f - c);
    }
    *reinterpret_cast<float4*>(dlogits + s * ldl + c4 * 4) = v;
  }
}

}  // namespace

extern "C" int hftt_time_embed_fwd(const float* x, const float* pos, float* y, int32_t B, int32_t T, int32_t Nn, int32_t d,
                                   float scale, float drop_p, uint32_t site, uint64_t seed, uint32_t io_flags, void* stream) {
  HFTT_REQUIRE(x && pos && y && d % 4 == 0, "time_embed_fwd: bad arguments");
  return hftt_launch<time_embed_fwd_kernel>("time_embed_fwd", dim3(grid_for((long)B * T * Nn * (d / 4), 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                                                              x, pos, y, B, T, Nn, d, scale, drop_p, site, seed, io_flags);
}
extern "C" int hftt_time_embed_bwd(const float* dy, float* dx, float* dym, int32_t B, int32_t T, int32_t Nn, int32_t d,
                                   float scale, float drop_p, uint32_t site, uint64_t seed, int32_t accumulate, uint32_t io_flags, void* stream) {
  HFTT_REQUIRE(dy && dx && d % 4 == 0, "time_embed_bwd: bad arguments");
  return hftt_launch<time_embed_bwd_kernel>("time_embed_bwd", dim3(grid_for((long)B * T * Nn * (d / 4), 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                                                              dy, dx, dym, B, T, Nn, d, scale, drop_p, site, seed, accumulate, io_flags);
}
extern "C" int hftt_dropout_bwd(float* g, int64_t n, float drop_p, uint32_t site, uint64_t seed, uint32_t bf16, void* stream) {
  HFTT_REQUIRE(g && n > 0 && n % 4 == 0 && drop_p >= 0.f && drop_p < 1.f && ((uintptr_t)g & 15) == 0, "dropout_bwd: bad arguments (n %% 4 == 0, 16-byte aligned)");
  if (drop_p == 0.f) return 0;
  return hftt_launch<dropout_bwd_kernel>("dropout_bwd", dim3(grid_for(n / 4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, g, (long)n, drop_p, site, seed, bf16);
}
extern "C" int64_t hftt_colsum_ws_bytes(int64_t rows, int64_t n) { (void)rows; return (int64_t)CS_SPLITS * n * 4; }
extern "C" int hftt_colsum(const float* x, int64_t rows, int64_t n, int64_t ld, float* out, float beta, float* ws, uint32_t x_bf16, void* stream) {
  HFTT_REQUIRE(x && out && ws && rows > 0 && n > 0 && ld >= n, "colsum: bad arguments");
  // whole quads, 16-byte aligned: the quad-per-thread stage 1 with nothing to mask (drop_p = 0: x is only read) -- the same splits, the same
  // row order per column, the same sums, in 16-byte loads with eight rows in flight
  if (n % 4 == 0 && ld % 4 == 0 && (((uintptr_t)x | (uintptr_t)ws) & 15) == 0) {
    if (int rc = hftt_launch<dropout_bwd_colsum_stage1_kernel>("colsum(1)", dim3((unsigned)((n / 4 + 255) / 256), CS_SPLITS), dim3(256), 0, (hipStream_t)stream,
                                                               const_cast<float*>(x), (long)rows, (long)n, (long)ld, 0.f, 0u, (uint64_t)0, ws, x_bf16)) return rc;
    return hftt_launch<colsum_stage2_kernel>("colsum(2)", dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, (long)n, out, beta);
  }
  if (int rc = hftt_launch<colsum_stage1_kernel>("colsum(1)", dim3((unsigned)((n + 255) / 256), CS_SPLITS), dim3(256), 0, (hipStream_t)stream, x, (long)rows, (long)n, (long)ld, ws, x_bf16)) return rc;
  return hftt_launch<colsum_stage2_kernel>("colsum(2)", dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, (long)n, out, beta);
}
extern "C" int hftt_dropout_bwd_colsum(float* g, int64_t rows, int64_t n, int64_t ld, float drop_p, uint32_t site, uint64_t seed, float* out, float beta,
                                       float* ws, uint32_t bf16, void* stream) {
  HFTT_REQUIRE(g && out && ws && rows > 0 && n > 0 && ld >= n && drop_p >= 0.f && drop_p < 1.f, "dropout_bwd_colsum: bad arguments");
  HFTT_REQUIRE(n % 4 == 0 && ld % 4 == 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)ws & 15) == 0, "dropout_bwd_colsum: n %% 4 == 0, ld %% 4 == 0, g and ws 16-byte aligned");
  if (int rc = hftt_launch<dropout_bwd_colsum_stage1_kernel>("dropout_bwd_colsum(1)", dim3((unsigned)((n / 4 + 255) / 256), CS_SPLITS), dim3(256), 0, (hipStream_t)stream,
                                                             g, (long)rows, (long)n, (long)ld, drop_p, site, seed, ws, bf16)) return rc;
  return hftt_launch<colsum_stage2_kernel>("dropout_bwd_colsum(2)", dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, (long)n, out, beta);
}
extern "C" int hftt_heads_split(const float* logits, int64_t ldl, float* onset, float* offset, float* mpe, float* velocity,
                                int32_t B, int32_t T, int32_t Nn, int32_t V, int32_t time_major, void* stream) {
  HFTT_REQUIRE(logits && onset && offset && mpe && velocity, "heads_split: null operand");
  HFTT_REQUIRE(V % 4 == 0 && ldl % 4 == 0 && ldl >= V + 3, "heads_split: V=%d / ldl=%ld unsupported", V, (long)ldl);
  return hftt_launch<heads_split_kernel>("heads_split", dim3(grid_for((long)B * T * Nn * (V / 4), 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                                                        logits, (long)ldl, onset, offset, mpe, velocity, B, T, Nn, V, time_major);
}
extern "C" int hftt_heads_split_bwd(const float* p_onset, const float* p_offset, const float* p_mpe,
                                    const float* d_onset, const float* d_offset, const float* d_mpe, const float* d_velocity,
                                    float* dlogits, int64_t ldl, int32_t B, int32_t T, int32_t Nn, int32_t V, int32_t time_major, void* stream) {
  HFTT_REQUIRE(p_onset && p_offset && p_mpe && d_onset && d_offset && d_mpe && d_velocity && dlogits, "heads_split_bwd: null operand");
  HFTT_REQUIRE(V % 4 == 0 && ldl % 4 == 0 && ldl >= V + 4, "heads_split_bwd: V=%d / ldl=%ld unsupported", V, (long)ldl);
  return hftt_launch<heads_split_bwd_kernel>("heads_split_bwd", dim3(grid_for((long)B * T * Nn * (ldl / 4), 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                                                                p_onset, p_offset, p_mpe, d_onset, d_offset, d_mpe, d_velocity, dlogits, (long)ldl, B, T, Nn, V, time_major);
}
