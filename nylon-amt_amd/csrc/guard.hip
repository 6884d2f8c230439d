// Guarded optimizer step (gfx950): the global L2 norm of the flat gradient as a two-launch fp64 reduction that leaves its verdict (norm, clip
// factor, apply / skip, counters) in a 32-byte device record, and the Adam kernel that reads the record: it skips a step whose norm is not
// finite, scales the gradient by the clip factor on the fly and applies decoupled weight decay.  No float atomics, no cross-workgroup
// tickets: every sum has one fixed order, so the record is bitwise reproducible.  Entry points and the torch definitions they restate:
// include/hftt_hip.h.  The unguarded step (hftt_adam_step / adam_kernel) stays the default path; all three Adam kernels share one update.
// The grouped forms (hftt_grad_norm_groups, hftt_adam_step_groups) read a per-quad group map: per-group learning rate and decay, and frozen
// groups whose quads are neither loaded nor stored (fine-tuning).  hftt_adam_step_ema is the grouped step with the exponential moving average
// of the parameters carried in the same launch (a compensated fp32 sum); it is opt-in and shares the update with the three kernels above.
#include "hftt_common.h"
#include "hftt_launch.h"
#include "../../include/hftt_hip.h"
#include <math.h>

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_MAX_WGS = 2048;          // the grid cap of adam_kernel: one fp64 partial per workgroup

// lanes of a wave: xor butterfly (the addition commutes, so every lane ends with the same bits)
__device__ __forceinline__ double wave_sum64(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// lanes, then the four waves in order; the result is valid in thread 0
__device__ __forceinline__ double block_sum64(double x) {
  __shared__ double red[GN_THREADS / 64];
  x = wave_sum64(x);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------------ stage 1: one fp64 partial of sum g^2 per workgroup
// The product of two fp32 values is exact in fp64 and |g| <= 3.4e38 squares to 1.2e77, far inside fp64: the partial is non-finite exactly
// when some element is Inf / NaN, and squares cannot cancel.
__global__ __launch_bounds__(GN_THREADS) void grad_sqsum_kernel(const float* __restrict__ g, long n, double* __restrict__ ws) {
  const long n4 = n / 4;
  const long stride = (long)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    const double x = gg.x, y = gg.y, z = gg.z, w = gg.w;
    acc += x * x; acc += y * y; acc += z * z; acc += w * w;
  }
  for (long i = n4 * 4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double x = g[i];
    acc += x * x;
  }
  const double s = block_sum64(acc);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// ------------------------------------------------------------------ stage 2: the partials in fixed order, the verdict, the record
__global__ __launch_bounds__(GN_THREADS) void grad_norm_finalize_kernel(const double* __restrict__ ws, int n_wg, double abs_scale, double max_norm,
                                                                        hftt_guard_ctl* __restrict__ ctl) {
  double acc = 0.0;
  for (int w = threadIdx.x; w < n_wg; w += GN_THREADS) acc += ws[w];
  const double sum = block_sum64(acc);
  if (threadIdx.x == 0) {
    const double norm64 = abs_scale * sqrt(sum);
    const bool apply = isfinite(norm64);
    const float coef = apply ? (float)fmin(1.0, max_norm / (norm64 + 1e-6)) : 0.f;
    ctl->norm = (float)norm64;
    ctl->coef = coef;
    ctl->apply = apply ? 1u : 0u;
    ctl->skipped += apply ? 0u : 1u;
    ctl->clipped += (apply && coef < 1.f) ? 1u : 0u;
  }
}

// ------------------------------------------------------------------ Adam: one update, three kernels
// m = beta1 * m + omb1 * gr;  v = beta2 * v + omb2 * gr * gr;  p = p * d - lr_c * m / (sqrtf(v) * inv_sqrt_bc2 + eps)  on gr = g * s, with
// d = 1 - lr * weight_decay (decoupled decay; the unguarded step passes d = 1, and p * 1.0f is exact) and s = grad_scale (* the clip factor
// in the guarded forms).  The rule: the update is written out, with contraction switched off around it, so that which product joins which
// sum in one fma is this text's choice and never a compiler's -- the default optimizer's bits do not move with a compiler update, and the
// three kernels agree by construction (tests/test_guard_gpu.py::test_inactive_guard_is_bit_identical_to_adam_step).  The quad loops and the
// tails use two operand orders; they are historical bits that are kept: QUAD m = fma(beta1, m, omb1 gr), v = fma(gr, omb2 gr, beta2 v);
// tail m = fma(omb1, gr, beta1 m), v = gr (omb2 gr) + beta2 v unfused; both den = fma(sqrt v, inv_sqrt_bc2, eps) and an unfused p - q.
template <bool QUAD>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float s, float d, float lr_c, float beta1, float beta2,
                                                    float omb1, float omb2, float eps, float inv_sqrt_bc2) {
#pragma clang fp contract(off)
  const float gr = g * s;
  const float pd = p * d;
  if (QUAD) {
    m = __builtin_fmaf(beta1, m, omb1 * gr);
    v = __builtin_fmaf(gr, omb2 * gr, beta2 * v);
  } else {
    m = __builtin_fmaf(omb1, gr, beta1 * m);
    v = gr * (omb2 * gr) + beta2 * v;
  }
  const float den = __builtin_fmaf(sqrtf(v), inv_sqrt_bc2, eps);
  p = pd - lr_c * m / den;
}

// the unguarded step: nothing to read but the operands
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                            float lr_c, float beta1, float beta2, float omb1, float omb2, float eps, float inv_sqrt_bc2, float grad_scale) {
  const long n4 = n / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* pe = &pp.x; const float* ge = &gg.x; float* me = &mm.x; float* ve = &vv.x;
#pragma unroll
    for (int e = 0; e < 4; e++) adam_update<true>(pe[e], ge[e], me[e], ve[e], grad_scale, 1.0f, lr_c, beta1, beta2, omb1, omb2, eps, inv_sqrt_bc2);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  const long tail = n4 * 4;
  for (long i = tail + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_update<false>(pi, g[i], mi, vi, grad_scale, 1.0f, lr_c, beta1, beta2, omb1, omb2, eps, inv_sqrt_bc2);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

// the guarded step: gr = g * (grad_scale * coef) behind p *= d; nothing is written when the record says skip
__global__ void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                                    float lr_c, float beta1, float beta2, float omb1, float omb2, float eps, float inv_sqrt_bc2, float grad_scale,
                                    float d, const hftt_guard_ctl* __restrict__ ctl) {
  if (ctl->apply == 0u) return;               // (uniform: every lane of every workgroup reads the same word)
  const float s = grad_scale * ctl->coef;
  const long n4 = n / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* pe = &pp.x; const float* ge = &gg.x; float* me = &mm.x; float* ve = &vv.x;
#pragma unroll
    for (int e = 0; e < 4; e++) adam_update<true>(pe[e], ge[e], me[e], ve[e], s, d, lr_c, beta1, beta2, omb1, omb2, eps, inv_sqrt_bc2);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  const long tail = n4 * 4;
  for (long i = tail + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_update<false>(pi, g[i], mi, vi, s, d, lr_c, beta1, beta2, omb1, omb2, eps, inv_sqrt_bc2);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

// ------------------------------------------------------------------ parameter groups (fine-tuning)
// One uint8 per quad of the flat buffer names the quad's group; parameter offsets are multiples of 8 elements, so a quad never straddles two
// parameters.  The per-group constants arrive by value and are staged in LDS with constant indices, so that the dynamic index gi never
// reaches a register array (ScratchSize 0).  A quad of a frozen group is neither loaded nor stored.
struct adam_group_consts {
  float lr_c[HFTT_ADAM_MAX_GROUPS];       // lr / (1 - beta1^t) per group
  float d[HFTT_ADAM_MAX_GROUPS];          // 1 - lr * weight_decay per group
  unsigned frozen_mask;                   // bit k: group k keeps its bits
};

__global__ __launch_bounds__(GN_THREADS) void grad_sqsum_groups_kernel(const float* __restrict__ g, long n4, const uint8_t* __restrict__ quad_group,
                                                                       unsigned frozen_mask, double* __restrict__ ws) {
  const long stride = (long)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    if ((frozen_mask >> (quad_group[i] & (HFTT_ADAM_MAX_GROUPS - 1))) & 1u) continue;
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    const double x = gg.x, y = gg.y, z = gg.z, w = gg.w;
    acc += x * x; acc += y * y; acc += z * z; acc += w * w;
  }
  const double s = block_sum64(acc);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

__global__ __launch_bounds__(GN_THREADS) void adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                 float* __restrict__ v, long n4, const uint8_t* __restrict__ quad_group,
                                                                 adam_group_consts c, float beta1, float beta2, float omb1, float omb2, float eps,
                                                                 float inv_sqrt_bc2, float grad_scale, const hftt_guard_ctl* __restrict__ ctl) {
  if (ctl != nullptr && ctl->apply == 0u) return;          // (uniform, as in adam_guarded_kernel)
  __shared__ float s_lr[HFTT_ADAM_MAX_GROUPS], s_d[HFTT_ADAM_MAX_GROUPS];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < HFTT_ADAM_MAX_GROUPS; k++) { s_lr[k] = c.lr_c[k]; s_d[k] = c.d[k]; }
  }
  __syncthreads();
  const float s = grad_scale * (ctl != nullptr ? ctl->coef : 1.f);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const unsigned gi = quad_group[i] & (HFTT_ADAM_MAX_GROUPS - 1);      // (values >= n_groups are the caller's error; the LDS index stays in range)
    if ((c.frozen_mask >> gi) & 1u) continue;
    const float lr_c = s_lr[gi], d = s_d[gi];
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* pe = &pp.x; const float* ge = &gg.x; float* me = &mm.x; float* ve = &vv.x;
#pragma unroll
    for (int e = 0; e < 4; e++) adam_update<true>(pe[e], ge[e], me[e], ve[e], s, d, lr_c, beta1, beta2, omb1, omb2, eps, inv_sqrt_bc2);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
}

// ------------------------------------------------------------------ the averaged weights (EMA) behind the update
// e += omd (p - e), omd = 1 - beta, on the NEW p, carried with a running compensation c (Kahan): in plain fp32 the sum stops moving once
// omd |p - e| < ulp(e) / 2, which with beta = 0.9999 is |p - e| < 6e-4 |e| -- the end of a decayed schedule.  c holds what the last sum
// dropped and hands it to the next.  Contraction off as in adam_update: (t - e) - y is the rounding error of t = e + y only as written.
__device__ __forceinline__ void ema_update(float& e, float& c, float p, float omd) {
#pragma clang fp contract(off)
  const float y = omd * (p - e) - c;
  const float t = e + y;
  c = (t - e) - y;
  e = t;
}

// adam_groups_kernel's step, then ema_update per element on the p still in registers: six 16-byte loads and five 16-byte stores per quad
// (44 B per element against 28).  quad_group == nullptr: one group (index 0), which the host admits only unfrozen.  Skip and frozen quads as in
// adam_groups_kernel: neither loads nor stores, ema and ema_c included.
__global__ __launch_bounds__(GN_THREADS) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, float* __restrict__ ema, float* __restrict__ ema_c, long n4,
                                                              const uint8_t* __restrict__ quad_group, adam_group_consts c, float beta1, float beta2,
                                                              float omb1, float omb2, float eps, float inv_sqrt_bc2, float grad_scale, float omd,
                                                              const hftt_guard_ctl* __restrict__ ctl) {
  if (ctl != nullptr && ctl->apply == 0u) return;          // (uniform, as in adam_guarded_kernel)
  __shared__ float s_lr[HFTT_ADAM_MAX_GROUPS], s_d[HFTT_ADAM_MAX_GROUPS];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < HFTT_ADAM_MAX_GROUPS; k++) { s_lr[k] = c.lr_c[k]; s_d[k] = c.d[k]; }
  }
  __syncthreads();
  const float s = grad_scale * (ctl != nullptr ? ctl->coef : 1.f);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const unsigned gi = quad_group != nullptr ? quad_group[i] & (HFTT_ADAM_MAX_GROUPS - 1) : 0u;
    if ((c.frozen_mask >> gi) & 1u) continue;
    const float lr_c = s_lr[gi], d = s_d[gi];
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ee = reinterpret_cast<float4*>(ema)[i];
    float4 cc = reinterpret_cast<float4*>(ema_c)[i];
    float* pe = &pp.x; const float* ge = &gg.x; float* me = &mm.x; float* ve = &vv.x; float* ee4 = &ee.x; float* ce = &cc.x;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      adam_update<true>(pe[e], ge[e], me[e], ve[e], s, d, lr_c, beta1, beta2, omb1, omb2, eps, inv_sqrt_bc2);
      ema_update(ee4[e], ce[e], pe[e], omd);
    }
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(ema)[i] = ee;
    reinterpret_cast<float4*>(ema_c)[i] = cc;
  }
}

// workgroups over n elements read four at a time: the grid of all Adam kernels (ceil((n / 4 + 1) / 256), at most GN_MAX_WGS)
inline int guard_grid(long n) {
  long b = (n / 4 + 1 + GN_THREADS - 1) / GN_THREADS;
  if (b < 1) b = 1;
  if (b > GN_MAX_WGS) b = GN_MAX_WGS;
  return (int)b;
}

// What hftt_adam_step_groups and hftt_adam_step_ema refuse alike (`who` names the entry point in the message), and the constants both kernels
// take: everything that is a function of the hyper-parameters alone is formed in double and rounded once, as in hftt_adam_step_guarded.
// map_optional: a null map stands for one unfrozen group.
int adam_groups_host(const char* who, const hftt_adam_groups_desc& a, bool map_optional, adam_group_consts& c, float& inv_sqrt_bc2) {
  HFTT_REQUIRE(a.p && a.g && a.m && a.v && a.n > 0 && a.step >= 1, "%s: bad arguments", who);
  HFTT_REQUIRE((((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)a.m | (uintptr_t)a.v) & 15) == 0, "%s: buffers must be 16-byte aligned", who);
  HFTT_REQUIRE(a.n % 4 == 0, "%s: n=%ld must be a multiple of 4 (one map entry per quad)", who, (long)a.n);
  HFTT_REQUIRE(a.n_groups >= 1 && a.n_groups <= HFTT_ADAM_MAX_GROUPS, "%s: n_groups=%d must be in 1..%d", who, (int)a.n_groups, HFTT_ADAM_MAX_GROUPS);
  HFTT_REQUIRE(a.quad_group != nullptr || (map_optional && a.n_groups == 1 && a.frozen[0] == 0), "%s: the group map is null", who);
  HFTT_REQUIRE(((uintptr_t)a.ctl & 15) == 0, "%s: ctl must be 16-byte aligned (NULL: unguarded)", who);
  const double bc1 = 1.0 - pow(a.beta1, (double)a.step);
  const double bc2 = 1.0 - pow(a.beta2, (double)a.step);
  c.frozen_mask = 0u;
  for (int k = 0; k < HFTT_ADAM_MAX_GROUPS; k++) {
    c.lr_c[k] = 0.f; c.d[k] = 1.f;
    if (k >= a.n_groups) continue;
    HFTT_REQUIRE(a.weight_decay[k] >= 0.0, "%s: group %d: weight_decay must be >= 0", who, k);                  // (false for NaN too)
    HFTT_REQUIRE(a.lr[k] * a.weight_decay[k] < 1.0, "%s: group %d: lr * weight_decay must be below 1", who, k);
    c.lr_c[k] = (float)(a.lr[k] / bc1);
    c.d[k] = (float)(1.0 - a.lr[k] * a.weight_decay[k]);
    if (a.frozen[k]) c.frozen_mask |= 1u << k;
  }
  inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  return 0;
}

// do [a, a + bytes) and [b, b + bytes) share a byte?
inline bool ranges_overlap(const void* a, const void* b, uint64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

}  // namespace

extern "C" int64_t hftt_grad_norm_ws_bytes(int64_t n) { (void)n; return (int64_t)GN_MAX_WGS * 8; }

extern "C" int hftt_grad_norm(const float* g, int64_t n, double grad_scale, double max_norm, void* ws, hftt_guard_ctl* ctl, void* stream) {
  HFTT_REQUIRE(g && ws && ctl, "grad_norm: null operand");
  HFTT_REQUIRE(n > 0, "grad_norm: n=%ld must be positive", (long)n);
  HFTT_REQUIRE((((uintptr_t)g | (uintptr_t)ws | (uintptr_t)ctl) & 15) == 0, "grad_norm: g, ws and ctl must be 16-byte aligned");
  HFTT_REQUIRE(isfinite(grad_scale), "grad_norm: grad_scale must be finite");
  HFTT_REQUIRE(max_norm > 0.0, "grad_norm: max_norm must be positive (+inf: no clipping)");         // (false for NaN too)
  const int wgs = guard_grid((long)n);
  if (int rc = hftt_launch<grad_sqsum_kernel>("grad_norm(1)", dim3(wgs), dim3(GN_THREADS), 0, (hipStream_t)stream, g, (long)n, (double*)ws)) return rc;
  return hftt_launch<grad_norm_finalize_kernel>("grad_norm(2)", dim3(1), dim3(GN_THREADS), 0, (hipStream_t)stream, (const double*)ws, wgs, fabs(grad_scale), max_norm, ctl);
}

extern "C" int hftt_adam_step(float* p, const float* g, float* m, float* v, int64_t n, int32_t step,
                              double lr, double beta1, double beta2, double eps, double grad_scale, void* stream) {
  HFTT_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adam_step: bad arguments");
  HFTT_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adam_step: buffers must be 16-byte aligned");
  // hyper-parameters arrive as doubles (python floats) and 1-beta is formed BEFORE rounding to fp32, as torch.optim.Adam does: 1.f - 0.999f is
  // off by 1.3e-5 relative and would show in exp_avg_sq of every step
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const float lr_c = (float)(lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  return hftt_launch<adam_kernel>("adam_step", dim3(guard_grid((long)n)), dim3(GN_THREADS), 0, (hipStream_t)stream, p, g, m, v, (long)n,
                                               lr_c, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, inv_sqrt_bc2, (float)grad_scale);
}

extern "C" int hftt_adam_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, int32_t step,
                                      double lr, double beta1, double beta2, double eps, double grad_scale,
                                      double weight_decay, const hftt_guard_ctl* ctl, void* stream) {
  HFTT_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adam_step_guarded: bad arguments");
  HFTT_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adam_step_guarded: buffers must be 16-byte aligned");
  HFTT_REQUIRE(ctl != nullptr, "adam_step_guarded: ctl is null");
  HFTT_REQUIRE(((uintptr_t)ctl & 15) == 0, "adam_step_guarded: ctl must be 16-byte aligned");
  HFTT_REQUIRE(weight_decay >= 0.0, "adam_step_guarded: weight_decay must be >= 0");                  // (false for NaN too)
  HFTT_REQUIRE(lr * weight_decay < 1.0, "adam_step_guarded: lr * weight_decay must be below 1");
  // as hftt_adam_step: everything that is a function of the hyper-parameters alone is formed in double and rounded once
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const float lr_c = (float)(lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  const float d = (float)(1.0 - lr * weight_decay);
  return hftt_launch<adam_guarded_kernel>("adam_step_guarded", dim3(guard_grid((long)n)), dim3(GN_THREADS), 0, (hipStream_t)stream, p, g, m, v, (long)n,
                                                                lr_c, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, inv_sqrt_bc2,
                                                                (float)grad_scale, d, ctl);
}

extern "C" int hftt_grad_norm_groups(const float* g, int64_t n, const uint8_t* quad_group, uint32_t frozen_mask, double grad_scale, double max_norm,
                                     void* ws, hftt_guard_ctl* ctl, void* stream) {
  HFTT_REQUIRE(g && ws && ctl, "grad_norm_groups: null operand");
  HFTT_REQUIRE(n > 0, "grad_norm_groups: n=%ld must be positive", (long)n);
  HFTT_REQUIRE(n % 4 == 0, "grad_norm_groups: n=%ld must be a multiple of 4 (one map entry per quad)", (long)n);
  HFTT_REQUIRE(quad_group != nullptr, "grad_norm_groups: the group map is null");
  HFTT_REQUIRE((frozen_mask >> HFTT_ADAM_MAX_GROUPS) == 0, "grad_norm_groups: frozen_mask names a group beyond %d", HFTT_ADAM_MAX_GROUPS);
  HFTT_REQUIRE((((uintptr_t)g | (uintptr_t)ws | (uintptr_t)ctl) & 15) == 0, "grad_norm_groups: g, ws and ctl must be 16-byte aligned");
  HFTT_REQUIRE(isfinite(grad_scale), "grad_norm_groups: grad_scale must be finite");
  HFTT_REQUIRE(max_norm > 0.0, "grad_norm_groups: max_norm must be positive (+inf: no clipping)");
  const int wgs = guard_grid((long)n);
  if (int rc = hftt_launch<grad_sqsum_groups_kernel>("grad_norm_groups(1)", dim3(wgs), dim3(GN_THREADS), 0, (hipStream_t)stream, g, (long)(n / 4), quad_group,
                                                     (unsigned)frozen_mask, (double*)ws)) return rc;
  return hftt_launch<grad_norm_finalize_kernel>("grad_norm_groups(2)", dim3(1), dim3(GN_THREADS), 0, (hipStream_t)stream, (const double*)ws, wgs, fabs(grad_scale), max_norm, ctl);
}

extern "C" int hftt_adam_step_groups(const hftt_adam_groups_desc* dsc, void* stream) {
  HFTT_REQUIRE(dsc != nullptr, "adam_step_groups: null descriptor");
  const hftt_adam_groups_desc& a = *dsc;
  adam_group_consts c;
  float inv_sqrt_bc2;
  if (int rc = adam_groups_host("adam_step_groups", a, false, c, inv_sqrt_bc2)) return rc;
  return hftt_launch<adam_groups_kernel>("adam_step_groups", dim3(guard_grid((long)a.n)), dim3(GN_THREADS), 0, (hipStream_t)stream, a.p, a.g, a.m, a.v,
                                         (long)(a.n / 4), a.quad_group, c, (float)a.beta1, (float)a.beta2, (float)(1.0 - a.beta1), (float)(1.0 - a.beta2),
                                         (float)a.eps, inv_sqrt_bc2, (float)a.grad_scale, a.ctl);
}

extern "C" int hftt_adam_step_ema(const hftt_adam_ema_desc* dsc, void* stream) {
  HFTT_REQUIRE(dsc != nullptr, "adam_step_ema: null descriptor");
  const hftt_adam_groups_desc& a = dsc->a;
  adam_group_consts c;
  float inv_sqrt_bc2;
  if (int rc = adam_groups_host("adam_step_ema", a, true, c, inv_sqrt_bc2)) return rc;
  float* const ema = dsc->ema; float* const ema_c = dsc->ema_c;
  HFTT_REQUIRE(ema != nullptr && ema_c != nullptr, "adam_step_ema: ema or ema_c is null");
  HFTT_REQUIRE((((uintptr_t)ema | (uintptr_t)ema_c) & 15) == 0, "adam_step_ema: ema and ema_c must be 16-byte aligned");
  const uint64_t bytes = (uint64_t)a.n * 4;
  for (const void* q : {(const void*)a.p, (const void*)a.g, (const void*)a.m, (const void*)a.v})
    HFTT_REQUIRE(!ranges_overlap(ema, q, bytes) && !ranges_overlap(ema_c, q, bytes), "adam_step_ema: ema and ema_c must not overlap p, g, m or v");
  HFTT_REQUIRE(!ranges_overlap(ema, ema_c, bytes), "adam_step_ema: ema and ema_c must not overlap each other");
  HFTT_REQUIRE(dsc->ema_decay >= 0.0 && dsc->ema_decay < 1.0, "adam_step_ema: ema_decay=%g must be in [0, 1)", dsc->ema_decay);          // (false for NaN too)
  // 1 - beta in double, rounded once: 1.f - (float)0.9999 is 1.0001659e-4, off by 1.7e-4 relative
  const float omd = (float)(1.0 - dsc->ema_decay);
  return hftt_launch<adam_ema_kernel>("adam_step_ema", dim3(guard_grid((long)a.n)), dim3(GN_THREADS), 0, (hipStream_t)stream, a.p, a.g, a.m, a.v, ema, ema_c,
                                      (long)(a.n / 4), a.quad_group, c, (float)a.beta1, (float)a.beta2, (float)(1.0 - a.beta1), (float)(1.0 - a.beta2),
                                      (float)a.eps, inv_sqrt_bc2, (float)a.grad_scale, omd, a.ctl);
}
