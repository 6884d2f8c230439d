/* libhftt_hip.so -- C ABI of the MI355X (gfx950) hFT-Transformer hot path.
 *
 * The reference (d-f/nylon-amt, vendored Sony hFT-Transformer) has no FFI: its hot path is the Python
 * classes of hftt_code/model/model_spec2midi.py driven by hftt_code/training/train.py and
 * hftt_code/model/amt.py.  This header is the boundary a replacement binds instead of the stock
 * torch.nn ops those classes call; every entry point cites the reference lines whose arithmetic it
 * replaces (paths relative to /root/reference/hftt_code).  Rules of the ABI:
 *   - extern "C", plain device pointers + sizes (+ one POD descriptor per call), no torch types;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); no allocation, no sync:
 *     the caller owns all buffers, including workspaces sized by the *_ws_bytes helpers;
 *   - return value 0 = ok, non-zero = error (message via hftt_last_error(), thread-local);
 *   - activations / gradients are fp32 row-major in HBM; in the bf16 mode (npass 1) tensors that are consumed ONLY as MFMA
 *     operands may be stored as bf16 (`io_flags` of each descriptor; leading dimensions and strides then count bf16
 *     elements) -- numerically identical to rounding at load time, half the traffic.  `npass` selects the MFMA arithmetic:
 *       1 = operands rounded to bf16, fp32 accumulate (v_mfma_f32_32x32x16_bf16): the "bf16" throughput mode,
 *       2 = "x3", split fp16: every fp32 operand is carried as fp16 hi + fp16 lo and a product as three MFMA passes
 *           (lo.hi + hi.lo + hi.hi, v_mfma_f32_32x32x16_f16, fp32 accumulate): ~22 significant bits, outputs within 1.3e-4 of the
 *           fp32 reference at paper size (budget 1e-3) at 3/16 of the cost of (3).  All tensors fp32 in HBM.  Forward products.
 *       3 = exact fp32 products and accumulation (v_mfma_f32_32x32x2_f32, 1/16 of the bf16 rate): the round-1 parity mode,
 *       4 = "x3", split bf16 (bf16 hi + bf16 lo, three passes): ~16 significant bits with fp32's exponent range: products with a
 *           GRADIENT operand (1e-4 .. 1e-10 in magnitude: subnormal or zero as fp16).  On the forward it is not enough for the
 *           reference's first encoder layer, whose attention logits reach ~1e5 on raw log-mel input (velocity logits 1.2e-3 off).
 *     hftt_attn_bwd with npass 2 recomputes the scores in split fp16 (bit for bit the forward's) and forms the four gradient
 *     products in split bf16.
 */
#ifndef HFTT_HIP_H
#define HFTT_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HFTT_ABI_VERSION 8

int hftt_abi_version(void);
/* bit 0: the library carries the opt-in gradient-rounding forms (HFTT_SL_X3_GRAD_HI, HFTT_TN_DY_HI, HFTT_NT_A_HI: a gradient operand enters a
 * backward product as its bf16 rounding -- faster, outside the 1e-3 the default keeps for gradients).  They are built only with
 * HFTT_BUILD_GRAD_HI=1 (nylon-amt_amd/build.py); the default library rejects those flags. */
int hftt_build_options(void);
const char* hftt_last_error(void);
/* ONE PROCESS DRIVES ONE DEVICE (one process per GPU, as torch.distributed launches them): the launchers keep per-kernel state -- dynamic-LDS
 * attributes, the CU count, the resident-workgroup grids of the persistent kernels -- in process-wide caches made for the device of the
 * first launch.  A launch from the same process with another device current is refused before anything is enqueued: it returns 3 with a
 * message instead of running with the first device's cached state.  Every entry point may be called from any host thread; launches go to the stream that is passed in. */
/* number of compute units of the process's device (for workspace sizing on the host side).  Counts as the process's first use of the current
 * device, as a launch does; -1 (with a message) from another device, or when the device query fails. */
int hftt_device_cus(void);

/* ---------------------------------------------------------------------------------------------
 * Dropout (nn.Dropout of model_spec2midi.py:95,236,242,372 and the attention probabilities :345).  Every kernel that drops takes
 * (drop_p, drop_site, drop_seed) and decides element `idx` of its site (idx = row*N + col of the tensor it produces; attention:
 * ((seq*H + head)*Lq + q)*Lk + k) with the counter-based generator of csrc/hftt_common.h:
 *     key  = splitmix64 round over (drop_seed + 0x9E3779B97F4A7C15 * (drop_site + 1))
 *     word = 32-bit two-multiply mix of (idx >> 2) with key          (one word per FOUR consecutive elements)
 *     keep = byte (idx & 3) of word  <  round((1 - drop_p) * 256)
 * with thr = round((1 - drop_p) * 256); kept elements are scaled by 256 / thr -- the reciprocal of the keep probability ACTUALLY applied
 * (p = 0.1: thr = 230, scale 1.11304, not 1/0.9 = 1.11111), so E[dropout(x)] = x exactly (csrc/hftt_common.h: hftt_keep_scale); drop_p
 * so small that thr = 256 drops nothing and scales by 1.  The backward of a site regenerates the same decisions from the same three numbers
 * (no mask tensor exists); tests/util.py::keep_mask is the numpy restatement the tests compare against.
 * --------------------------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------------------------
 * Weight preparation.  fp32 parameters -> the layouts the GEMMs consume (concatenated / transposed), as a bf16
 * plane `wbf` (npass 1) and/or an fp32 copy `wf32` (npass 3); either may be NULL.
 * (replaces nothing in the reference: it is the operand format of the MFMA kernels).
 * Each entry copies a [rows, cols] fp32 matrix (row stride src_ld) from `params + src_off` to
 * `dst + dst_off`, either as-is (dst[r*dst_ld + c]) or transposed (dst[c*dst_ld + r]).
 * Entries may also write fp32 vectors (bias concatenation): kind 2 copies `rows*cols` floats to
 * `fdst + dst_off`.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t src_off;   /* element offset into params */
  int64_t dst_off;   /* element offset into the destination plane(s) */
  int32_t rows, cols, src_ld, dst_ld;
  int32_t kind;      /* 0 = copy, 1 = transposed copy (both into wbf/wf32), 2 = fp32 copy into fdst */
  int32_t pad;
} hftt_prep_entry;
int hftt_prep_weights(const float* params, uint16_t* wbf, float* wf32, float* fdst,
                      const hftt_prep_entry* table_dev, int n_entries, void* stream);
/* The same table for the split ("x3") modes: every matrix entry is written as TWO 16-bit planes, whi[dst] + wlo[dst] ~ the fp32 value,
 * with the entry's `pad` field naming the element type (2 = fp16 for the forward matrices, 4 = bf16 for the transposed matrices of
 * the dX products); kind 2 entries copy fp32 vectors into fdst as above. */
int hftt_prep_weights_x3(const float* params, uint16_t* whi, uint16_t* wlo, float* fdst,
                         const hftt_prep_entry* table_dev, int n_entries, void* stream);

/* ---------------------------------------------------------------------------------------------
 * NT GEMM with fused epilogue:  C[M,N] = epi( A[M,K] . W[N,K]^T + bias )
 * Replaces nn.Linear in MultiHeadAttentionLayer.fc_q/k/v/o (model_spec2midi.py:328-330,357),
 * PositionwiseFeedforwardLayer.fc_1/fc_2 (:372,375), Encoder tok_embedding_freq (:85, after the
 * conv fold), the output heads (:172-175, :203-206) and, with transposed weights, every dX = dY.W of
 * loss.backward() (training/train.py:158).
 * epilogue, in this order:  v = acc + bias[col];  if act==1 v = max(v,0);  v *= out_scale;
 *   if add_table: v += add_table[(row % add_mod)*N + col]              (position embedding, :95)
 *   if gate:      v = gate[row*ldg+col] > 0 ? v*gate_scale : 0          (ReLU/dropout backward)
 *   if drop_p>0:  v = keep(seed,site,row*N+col) ? v*256/thr : 0         (nn.Dropout, :95,236,242,372; thr: see Dropout above)
 *   if residual:  v += residual[(row % res_mod)*ldr + col]              (:236,242)
 *   if ln_gamma:  pre_ln_out = v;  v = LayerNorm(v)*gamma+beta (eps 1e-5, over N; needs N in {64,128,256})
 *                 mean/rstd written per row                              (nn.LayerNorm, :225,236)
 *   C[row*ldc+col] = v
 * W is the prepared matrix [N_pad, K] (K % 32 == 0, N_pad % 64 == 0, rows >= N zero): bf16 when npass == 1,
 * fp32 when npass == 3 (passed through the same pointer); npass 2 / 4: the hi plane in W and the lo plane in W_lo
 * (hftt_prep_weights_x3), A / C / residual / gate fp32.
 * npass 2 / 4 without LayerNorm, K <= 256 and N == 256 (or K == 256 and N <= 256) take an A-stationary streaming form of the kernel with
 * the same results to the bit.  Environment variable HFTT_NT_STREAM=0 (read at every such call, so one process can run both) keeps
 * them on the tiled kernel.
 * --------------------------------------------------------------------------------------------- */
#define HFTT_NT_A_BF16 1u
#define HFTT_NT_C_BF16 2u      /* not with LayerNorm */
#define HFTT_NT_GATE_BF16 4u
#define HFTT_NT_A_HI 16u       /* npass 4: A (a gradient) enters as its bf16 rounding only -- two MFMA passes against the weight pair */
#define HFTT_NT_RES_BF16 8u    /* residual stored as bf16 (A-stationary bf16-mode kernels: N % 256 == 0, M >= 256, K <= 768) */
typedef struct {
  int32_t M, N, K, npass;
  const float* A; int64_t lda;
  const void* W;                                  /* [N_pad, K] bf16 (npass 1) or fp32 (npass 3) */
  uint32_t io_flags;                              /* HFTT_NT_* (npass 1 only): A / C / gate stored as bf16 */
  uint32_t debug;
  const float* bias;                              /* [N] or NULL */
  float* C; int64_t ldc;
  int32_t act; float out_scale;
  const float* add_table; int32_t add_mod;
  const float* gate; int64_t ldg; float gate_scale;
  float drop_p; uint32_t drop_site; uint64_t drop_seed;
  const float* residual; int64_t ldr; int32_t res_mod;
  const float* ln_gamma; const float* ln_beta; float* pre_ln_out; float* ln_mean; float* ln_rstd;
  const void* W_lo;                               /* npass 2 / 4: lo plane of the prepared weights (same layout as W) */
} hftt_gemm_nt_desc;
int hftt_gemm_nt(const hftt_gemm_nt_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * "Strip" kernels (bf16 mode): the MI355X-first form of every nn.Linear on the path whose output width is a multiple of
 * 256 -- MultiHeadAttentionLayer.fc_q/k/v/o (model_spec2midi.py:328-330,357), PositionwiseFeedforwardLayer (:362-378),
 * the post-norm residual blocks of EncoderLayer / DecoderLayer (:236,242,262,268,289,295,301) and their dX in backward.
 *
 * Geometry: a workgroup of 4 waves owns 128 consecutive tokens; a wave owns a 32-token strip and keeps it in registers as the
 * MFMA *B* operand (lane = (token, half): for every 32-feature group it holds 16 consecutive features).  The weights are the
 * *A* operand: pre-packed once per step into 1 KB MFMA fragments in consumption order ("strip pack"), streamed L2 -> LDS by
 * LDS-DMA through a 4 x 16 KB ring shared by the four waves.  v_mfma_f32_32x32x16_bf16 then leaves C^T in the same
 * (token, half) x 16-consecutive-features layout, so bias / ReLU / dropout / gate / residual / LayerNorm are per-lane register
 * work (row statistics = 128 own values + one v_permlane32_swap), the result of one GEMM is directly the B operand of the
 * next (fused FFN: the p-wide hidden never leaves the registers), and every global access is 16 bytes per lane.
 *
 * strip pack: logical weight matrix Wl[N, K] (out x in features, i.e. the nn.Linear weight for a forward GEMM, its transpose
 * for a dX GEMM).  Fragment(tile, pt, u), 64 lanes x 8 bf16: lane (i = lane & 31, hk = lane >> 5) holds
 *   Wl[32*tile + c(i)][32*pt + 16*hk + 8*u + 0..7],   c(i) = 16*((i >> 2) & 1) + (i & 3) + 4*(i >> 3).
 * Slots of 16 fragments (16 KB), order 0 ("linear"): slot = pass*(K/32) + pt, fragment = u*8 + (tile & 7), pass = tile >> 3;
 * order 1 ("tile-major", K == 256): slot = tile, fragment = 2*pt + u.  The stream position of a slot is
 * slot_offset + slot_stride*slot (the fused FFN interleaves fc_1 tiles with fc_2 K-slices: stride 2, offsets 0 / 1).
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t src_off;              /* element offset of the fp32 source matrix inside params */
  int64_t dst_off;              /* bf16-element offset of stream slot 0 inside wstrip */
  int32_t rows, cols, src_ld;   /* source [rows, cols], row stride src_ld */
  int32_t transpose;            /* 0: Wl[n0 + r][k0 + c] = src[r][c];  1: Wl[n0 + c][k0 + r] = src[r][c] */
  int32_t n0, k0;               /* position inside the logical matrix (k0 % 8 == 0) */
  int32_t K;                    /* logical K (multiple of 32) */
  int32_t order;                /* 0 linear, 1 tile-major */
  int32_t slot_stride, slot_offset;
} hftt_strip_pack_entry;
int hftt_strip_pack(const float* params, uint16_t* wstrip, const hftt_strip_pack_entry* table_dev, int n_entries, void* stream);
/* The split-operand form of the pack (same table type; elem = 2: fp16 halves, 4: bf16 halves).  Every fragment(tile, chunk) of the bf16
 * pack becomes a (hi, lo) pair of 1 KB fragments, chunk = 2*pt + u naming the 16-deep k step; a 16 KB slot holds the pairs of 8 tiles for
 * one chunk (order 0: slot = (tile >> 3)*(K/16) + chunk, fragment = 2*(tile & 7) + plane) or of 8 chunks for one tile (order 1, K == 256:
 * slot = 2*tile + (chunk >> 3), fragment = 2*(chunk & 7) + plane); slots come in pairs: stream position = slot_offset +
 * slot_stride*(slot >> 1) + (slot & 1) (plain stream: stride 2, offset 0; the fused block interleaves two pairs per hidden tile:
 * stride 4, offsets 0 / 2).  A packed matrix takes 2 * rows * cols 16-bit elements. */
int hftt_x3_strip_pack(const float* params, uint16_t* wstrip, const hftt_strip_pack_entry* table_dev, int n_entries, int elem, void* stream);

#define HFTT_SL_X_BF16 1u       /* x stored as bf16 (else fp32, rounded to bf16 on load) */
#define HFTT_SL_C_BF16 2u       /* C (and pre_ln_out) stored as bf16 */
#define HFTT_SL_RES_BF16 4u     /* residual stored as bf16 */
#define HFTT_SL_RELU 8u
/* split-operand ("x3") forms of the strip kernels: x, C, residual, pre_ln_out (and the fused block's h_out / gate) are fp32, `w` is an
 * hftt_x3_strip_pack stream of fp16 (HFTT_SL_X3_F16: forward products) or bf16 (HFTT_SL_X3_BF16: products with a gradient operand)
 * hi / lo fragment pairs; every product runs in three MFMA passes.  Shapes: K, N multiples of 256 with N/256 x K/256 in
 * {1x1, 2x1, 3x1, 1x2, 1x3} (LayerNorm form: N == 256, K in {256, 512}), M % 32 == 0, no gate; fused block: d == 256, p == 512.
 * Pack order: K == 256 without LayerNorm takes the TILE-MAJOR pack (order 1: the kernel walks one 32-column output tile at a time), every
 * other form the linear pack (order 0). */
#define HFTT_SL_X3_F16 16u
#define HFTT_SL_X3_BF16 32u
/* fused block in a split mode: h_out / gate are bf16 [M, p] instead of fp32.  The hidden feeds fc_2 from registers at full width either way;
 * the STORED copy is read only as the ReLU / dropout gate and as an operand of the weight-gradient products (hftt_gemm_tn, npass 4 with
 * HFTT_TN_X_BF16 / HFTT_TN_DY_BF16), where 8 mantissa bits of one factor leave the gradient's direction untouched. */
#define HFTT_SL_H_BF16 64u
/* with HFTT_SL_X3_BF16: the strip x (hftt_ffn_bwd_dx: dy and the dh it forms) is a gradient and enters as its bf16 rounding only */
#define HFTT_SL_X3_GRAD_HI 256u
/* split modes, LayerNorm forms (hftt_strip_linear with ln_gamma, hftt_ffn_res_ln_fwd): pre_ln_out is bf16 [M, 256] -- it is read only by
 * hftt_ln_bwd (HFTT_LNB_R_BF16), as xhat = (r - mean) * rstd against the fp32 statistics. */
#define HFTT_SL_PRE_BF16 128u
/* Small widths (split modes): K, N <= 192, multiples of 32, with K x N in {64x64, 64x128, 64x192, 128x64, 192x64} (LayerNorm form: 64x64) and
 * the fused block at d == 64, p == 128 -- the reference's default model (training/m_training.py:56-61).  `w` is then an
 * hftt_x3_strip_pack stream of order 2 ("compact": the (hi, lo) pair of (k chunk c, output tile t) at pair index slot_offset + c * NT + t with
 * NT = slot_stride = N / 32, 2 KB per pair; fused block: first matrix at pairs 0 .. 15, second at 16 .. 31): the whole matrix sits in LDS for the
 * launch (csrc/small_strip.h).
 * The same shapes WITHOUT a split flag and with all-bf16 storage (HFTT_SL_X_BF16 | HFTT_SL_C_BF16, a bf16 residual, M % 32 == 0) run the bf16
 * small-width family (the same csrc/small_strip.h on the bf16 stream of csrc/bs_strip.hip, round 5: BASELINE config 2 -- the reference's default model in the bf16 mode): same compact pack, made
 * with bf16 halves (hftt_x3_strip_pack element type 4), of which these kernels read the hi fragment; one MFMA pass; every tensor bf16, statistics
 * fp32; results leave as whole 128-byte lines. */
/* HFTT_SL_X3_F16 without LayerNorm, K == 256 (the output-tile-major kernel): C is written as f16-pair planes per 32-column group (see
 * HFTT_ATTN_Q_F16PAIR) -- the q / k / v projections of the attention layers (model_spec2midi.py:328-330).  N = 256, 512, 768 and, since
 * round 6, 1024 / 1536: the cross-attention K / V projections of two / three decoder layers stacked along N (they share their input, the
 * encoder output: model_spec2midi.py:259,296), one launch that reads it once. */
#define HFTT_SL_C_F16PAIR 512u
/* ABI v7, HFTT_SL_X3_BF16 (backward products), N == K == 256 without LayerNorm / residual: the strip x is the gradient of a dropout OUTPUT of
 * width K and is masked with (drop_p, drop_site, drop_seed) while it is loaded (element (m, k) = element m * K + k of the site); no epilogue
 * dropout in this form.  hftt_ffn_bwd_dx does the same with site_o when drop_p > 0 (the gradient of the block's output dropout). */
#define HFTT_SL_X_DROP 2048u
/* C[M,N] = epi(x[M,K] . Wl[N,K]^T + bias): same epilogue order as hftt_gemm_nt (relu, out_scale, gate, dropout, residual,
 * LayerNorm over N == 256).  N % 256 == 0; K % 32 == 0 and (K <= 256 or K % 256 == 0); gate is bf16. */
typedef struct {
  int32_t M, N, K; uint32_t flags;
  const void* x; int64_t ldx;
  const uint16_t* w;                  /* strip pack, order 0 */
  const float* bias;                  /* [N] or NULL */
  void* C; int64_t ldc;
  float out_scale;
  float gate_scale;
  const uint16_t* gate; int64_t ldg;  /* bf16 [M, N] or NULL: v = gate > 0 ? v*gate_scale : 0 */
  float drop_p; uint32_t drop_site; uint64_t drop_seed;
  const void* residual; int64_t ldr; int32_t res_mod; int32_t pad;
  const float* ln_gamma; const float* ln_beta; void* pre_ln_out; float* ln_mean; float* ln_rstd;
} hftt_strip_desc;
int hftt_strip_linear(const hftt_strip_desc* d, void* stream);

/* Fused position-wise feed-forward block (model_spec2midi.py:369-378 + the post-norm of :242/:268/:301), d == 256:
 *   h = dropout_h(relu(x W1^T + b1))      [M, p] stays in registers (optionally also written as bf16 for backward)
 *   y = LayerNorm(x + dropout_o(h W2^T + b2)) * gamma + beta
 * and, with mode 1, the dX half of its backward:
 *   dh = gate(h) * (dy W2) * gate_scale   (written as bf16 for the weight-gradient GEMMs)
 *   dx = dh W1 + residual
 * w = ONE interleaved strip stream: slot 2t = tile t of the first matrix (order 1), slot 2t+1 = K-slice t of the second
 * (order 0).  p % 32 == 0. */
typedef struct {
  int32_t M, d, p; uint32_t flags;    /* HFTT_SL_X_BF16 / C_BF16 / RES_BF16 */
  int32_t mode; int32_t pad;
  const void* x; int64_t ldx;
  const uint16_t* w;
  const float* b1; const float* b2;   /* [p], [d] (mode 0) */
  uint16_t* h_out; int64_t ldh;       /* mode 0: post-dropout hidden (bf16) or NULL; mode 1: dh (bf16, required) */
  const uint16_t* gate; int64_t ldg;  /* mode 1: stored hidden (bf16) */
  float gate_scale;
  float drop_p; uint32_t site_h, site_o; uint64_t drop_seed;
  const void* residual; int64_t ldr;  /* mode 0: NULL = x itself; mode 1: added to dx (or NULL) */
  const float* ln_gamma; const float* ln_beta; void* pre_ln_out; float* ln_mean; float* ln_rstd;   /* mode 0 */
  void* y; int64_t ldy;
} hftt_ffn_desc;
int hftt_ffn_res_ln_fwd(const hftt_ffn_desc* d, void* stream);   /* mode 0 */
int hftt_ffn_bwd_dx(const hftt_ffn_desc* d, void* stream);       /* mode 1 */
/* ABI v8 (split mode, HFTT_SL_X3_F16; d == 256, p == 512): the second half of a layer behind its attention as ONE launch --
 *   x1 = LayerNorm(residual + dropout(ctx Wo^T + bo))          model_spec2midi.py:236-237 / :262-263 / :295-296   (descriptor o, exactly as for hftt_strip_linear)
 *   y  = LayerNorm(x1 + dropout(FFN(x1)))                       model_spec2midi.py:240-242 / :266-268 / :299-301   (descriptor f, exactly as for hftt_ffn_res_ln_fwd)
 * x1 stays in registers between the two halves: o->C may be NULL (inference plan: x1 is not written at all); when it is given it must be f->x.
 * f->w must be o->w + 16 slots (one weight stream of 80 slots per 128-token block: fc_o in order 0, then the FFN's interleaved pair).
 * Results are bit-identical to hftt_strip_linear(o) followed by hftt_ffn_res_ln_fwd(f). */
int hftt_attn_out_ffn_fwd(const hftt_strip_desc* o, const hftt_ffn_desc* f, void* stream);

/* ---------------------------------------------------------------------------------------------
 * TN GEMM (weight gradient):  dW[N,K] = out_scale * dY[M,N]^T . X[M,K],  db[N] = colsum(dY)
 * Replaces the weight/bias gradient of every nn.Linear in loss.backward() (training/train.py:158).
 * Two launches: partial products per M-split into `ws`, then a reduce that writes (beta=0) or
 * accumulates (beta=1) into up to 8 row segments of the destination (fused QKV / packed heads / stacked cross-attention K, V).
 * --------------------------------------------------------------------------------------------- */
#define HFTT_TN_DY_BF16 1u
#define HFTT_TN_X_BF16 2u
#define HFTT_TN_DY_HI 4u       /* npass 4: dY (the gradient) enters as its bf16 rounding only; X keeps its bf16 pair (two MFMA passes) */
/* ABI v7, npass 4, fp32 dY with N == lddy == the width of the dropped tensor: dY is the gradient of a dropout OUTPUT and the kernel applies
 * the mask of (drop_p, drop_site, drop_seed) while it loads it -- element (m, n) is element m * N + n of the site -- so that the LayerNorm
 * backward does not have to write a masked copy of its result for this product (hftt_ln_bwd with dr_drop == NULL); db = colsum of the
 * masked rows.  Tiles: N >= 256 and K >= 256; the loader indexes the site's hash quads in 32 bits: M < 2^24 and M * N < 2^34 (status 1 beyond). */
#define HFTT_TN_DY_DROP 8u
typedef struct {
  int32_t M, N, K, npass;
  const float* dY; int64_t lddy;
  const float* X; int64_t ldx;
  float out_scale; float beta;
  int32_t n_seg;             /* 1 .. 8 (ABI v7; 4 before: the cross-attention K / V gradients of three decoder layers are six segments of one product) */
  int32_t seg_row0[8]; int32_t seg_rows[8];
  float* seg_dw[8];          /* [seg_rows, K] row-major (ld = K_out) */
  float* seg_db[8];          /* [seg_rows] or NULL */
  int32_t K_out;             /* number of K columns to write (<= K), destination leading dim */
  uint32_t io_flags;         /* HFTT_TN_*: npass 1 (either / both), npass 4 (ONE of them: that operand is its own hi half, two MFMA passes) */
  void* ws; int64_t ws_bytes;
  float drop_p; uint32_t drop_site; uint64_t drop_seed;      /* HFTT_TN_DY_DROP (ABI v7) */
} hftt_gemm_tn_desc;          /* npass 4 (split bf16): dY and X fp32, split on their way into LDS (or one of them stored as bf16) */
int64_t hftt_gemm_tn_ws_bytes(int32_t M, int32_t N, int32_t K);
int hftt_gemm_tn(const hftt_gemm_tn_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused multi-head attention, one workgroup per (sequence, head); Lq, Lk <= 256, dh in {32, 64}.
 * forward:  P = softmax(Q K^T / sqrt(dh));  out = dropout(P) V;  lse = per-row (max score, 1/sum exp) pairs;
 *           probs (optional) = P (pre-dropout)         -- model_spec2midi.py:335-354, returned P :360
 * backward: recomputes P from (Q,K,lse); dQ,dK,dV      -- autograd of the same lines
 * Q/K/V/out element (seq, row, head, c) lives at  base + seq*seq_stride + row*ld + head*dh + c.
 * --------------------------------------------------------------------------------------------- */
#define HFTT_ATTN_Q_BF16 1u       /* q */
#define HFTT_ATTN_KV_BF16 2u      /* k, v */
#define HFTT_ATTN_O_BF16 4u       /* out, dout */
#define HFTT_ATTN_DQ_BF16 8u      /* dq */
#define HFTT_ATTN_DKV_BF16 16u    /* dk, dv */
/* npass 2 only, dh == 64: q / k, v are "f16-pair planes" -- the 32 fp32 slots (128 bytes) of every aligned 32-column group of a row hold
 * the group's 32 fp16 hi halves followed by its 32 fp16 lo halves (x = hi + lo to 2^-22), written ONCE by the projection that produced them
 * (hftt_strip_linear with HFTT_SL_C_F16PAIR, hftt_x3_to_planes) instead of being split by every kernel that reads them; pointers and
 * strides keep their fp32 meaning.  Both flags or neither.  The forward then stages K / V by LDS-DMA (csrc/x3_attn_pl.hip: persistent
 * workgroups, ceil(Lq / 32) <= 8 at Lk > 128 and <= 4 below).  The FORWARD's results (output, row statistics, attention map) are bit-identical
 * to the fp32-operand form's.  The backward recomputes P bitwise as the forward did, but forms the bf16 (hi, lo) operands of its gradient
 * products from the stored fp16 pair (hi + lo, exact in fp32) instead of from the fp32 value: dq / dk / dv agree with the fp32-operand
 * backward to 4e-5 of each tensor's maximum (tests/test_x3_gpu.py::test_attention_on_planes_equals_attention_on_fp32_operands, 12 geometries
 * x dropout on / off). */
#define HFTT_ATTN_Q_F16PAIR 32u
#define HFTT_ATTN_KV_F16PAIR 64u
typedef struct {
  int32_t n_seq, n_heads, Lq, Lk, dh, npass;
  const float* q; int64_t q_seq_stride; int64_t ldq;
  const float* k; int64_t k_seq_stride; int64_t ldk;
  const float* v; int64_t v_seq_stride; int64_t ldv;
  float* out; int64_t o_seq_stride; int64_t ldo;
  float* lse;                 /* [n_seq, n_heads, Lq, 2]: (row max, 1 / sum(exp(score - max))); the max is of the scaled scores, except
                                 in the npass == 2 kernels and the npass == 1 kernels with q, k, v AND out stored as bf16, which keep the
                                 max of the RAW Q.K^T (before the 1/sqrt(dh)) -- an opaque pair between a forward and the backward of
                                 the SAME npass, storage flags AND strides (the all-bf16 form also needs every row / sequence stride of
                                 q, k, v, out to be a multiple of 8 elements; forward and backward test that with one shared predicate) */
  float* probs;               /* [n_seq, n_heads, Lq, Lk] or NULL */
  float drop_p; uint32_t drop_site; uint64_t drop_seed;
  /* backward only */
  const float* dout;          /* same layout as out */
  float* dq; int64_t dq_seq_stride; int64_t lddq;
  float* dk; int64_t dk_seq_stride; int64_t lddk;
  float* dv; int64_t dv_seq_stride; int64_t lddv;
  uint32_t io_flags;          /* HFTT_ATTN_* (the BF16 flags: npass 1 only; the F16PAIR flags: npass 2 only) */
  uint32_t pad;
} hftt_attn_desc;
int hftt_attn_fwd(const hftt_attn_desc* d, void* stream);
int hftt_attn_bwd(const hftt_attn_desc* d, void* stream);
/* fp32 [rows, cols] (row stride lds) -> f16-pair planes [rows, cols] (row stride ldd, both in fp32 slots), per 32-column group; cols % 32 == 0,
 * dst != src.  For operands no strip kernel produces (the shared query of DecoderLayer_Zero, model_spec2midi.py:154-155; tests). */
int hftt_x3_to_planes(const float* src, int64_t lds, float* dst, int64_t ldd, int32_t rows, int32_t cols, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Encoder front: fold of Conv2d(1,C,(1,k)) + window flatten + Linear(C*(n_proc-k+1), d)
 * (model_spec2midi.py:65-85) into one Linear over the n_proc-wide window:
 *   tok[j] = sum_u Weff[j,u] * spec[f, t+u] + beff[j],
 *   Weff[j,u] = sum_{c, kk, w+kk=u} Wtok[j, c*nw + w] * wconv[c,kk],  beff[j] = btok[j] + sum_c bconv[c] sum_w Wtok[j,c*nw+w]
 * fold_fwd writes Weff [d_pad, Kp] (Kp = n_proc rounded up to 32, zero padded) as bf16 and/or fp32, + beff.
 * fold_bwd maps (dWeff [d, Kp] fp32, dbeff [d]) back to the four reference parameters' gradients.
 * im2win materialises A[(b,t,f), u] = spec[b, f, t+u] (zero for u >= n_proc), row stride Kp.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t d, C, kw, n_proc, Kp, d_pad;
  const float* wconv;   /* [C, kw] */
  const float* bconv;   /* [C] */
  const float* wtok;    /* [d, C*(n_proc-kw+1)] */
  const float* btok;    /* [d] */
  uint16_t* weff_bf; float* weff_f32;     /* [d_pad, Kp]; either may be NULL */
  float* beff;          /* [d] */
  /* backward */
  const float* dweff;   /* [d, Kp] */
  const float* dbeff;   /* [d] */
  float* g_wconv; float* g_bconv; float* g_wtok; float* g_btok;
  uint16_t* weff_hi; uint16_t* weff_lo;   /* split fp16 planes of Weff for the x3 mode (both or neither) */
} hftt_fold_desc;
int hftt_embed_fold_fwd(const hftt_fold_desc* d, void* stream);
int hftt_embed_fold_bwd(const hftt_fold_desc* d, void* stream);
int hftt_im2win(const float* spec, float* win, int32_t B, int32_t F, int32_t T, int32_t n_proc, int32_t Kp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm backward (shared gamma/beta per layer, model_spec2midi.py:225,250,277):
 *   dr = rstd * (g - mean(g) - xhat*mean(g*xhat)),  g = dy*gamma,  xhat = (r-mean)*rstd
 *   dr_drop (optional) = dropout-masked dr for the residual branch (site/seed of the forward dropout)
 *   partial dgamma/dbeta per workgroup -> ws; hftt_ln_bwd_reduce sums them into the parameter grads.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t M, N;
  const float* dy; const float* r; const float* mean; const float* rstd; const float* gamma;
  float* dr; float* dr_drop;
  float drop_p; uint32_t drop_site; uint64_t drop_seed;
  float* ws;            /* [n_wg, 2, N] partial sums; n_wg = hftt_ln_bwd_wgs(M) */
  uint32_t drop_bf16;   /* dr_drop is stored as bf16 */
  uint32_t io_flags;    /* HFTT_LNB_DY_BF16: dy stored as bf16; HFTT_LNB_DR_BF16: dr stored as bf16 (bf16 gradient stream);
                           HFTT_LNB_R_BF16: the saved pre-LayerNorm sum r stored as bf16 (strip forward kernels) */
} hftt_ln_bwd_desc;
#define HFTT_LNB_DY_BF16 1u
#define HFTT_LNB_DR_BF16 2u
#define HFTT_LNB_R_BF16 4u
int32_t hftt_ln_bwd_wgs(int32_t M);
int hftt_ln_bwd(const hftt_ln_bwd_desc* d, void* stream);
int hftt_ln_bwd_reduce(const float* ws, int32_t n_wg, int32_t N, float* dgamma, float* dbeta, float beta, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Small data-movement kernels of the decoder (model_spec2midi.py:189-191, :172-175, :203-206).
 * --------------------------------------------------------------------------------------------- */
/* y[(b,n), t, :] = dropout( x[(b,t), n, :]*scale + pos[t, :] );  io_flags: HFTT_TE_X_BF16 (x), HFTT_TE_Y_BF16 (y) stored as bf16 */
#define HFTT_TE_X_BF16 1u
#define HFTT_TE_Y_BF16 2u
#define HFTT_TE_M_BF16 4u
int hftt_time_embed_fwd(const float* x, const float* pos, float* y, int32_t B, int32_t T, int32_t Nn, int32_t d,
                        float scale, float drop_p, uint32_t site, uint64_t seed, uint32_t io_flags, void* stream);
/* dx[(b,t), n, :] (+)= mask*dy[(b,n), t, :]*scale ; dym (optional, [(b,n),t,:]) = masked dy (for the pos-emb colsum);
 * io_flags: HFTT_TE_X_BF16 (dy), HFTT_TE_Y_BF16 (dx), HFTT_TE_M_BF16 (dym) stored as bf16 */
int hftt_time_embed_bwd(const float* dy, float* dx, float* dym, int32_t B, int32_t T, int32_t Nn, int32_t d,
                        float scale, float drop_p, uint32_t site, uint64_t seed, int32_t accumulate, uint32_t io_flags, void* stream);
/* in-place dropout backward: g *= mask*256/thr, thr = round((1-p)*256) (same indexing as the forward epilogue: idx = row*N+col); n % 4 == 0; bf16 != 0: g is bf16 */
int hftt_dropout_bwd(float* g, int64_t n, float drop_p, uint32_t site, uint64_t seed, uint32_t bf16, void* stream);
/* colsum: out[j] = beta*out[j] + sum_r x[r*ld + j], j < n (x fp32, or bf16 when x_bf16 != 0; out fp32) */
int hftt_colsum(const float* x, int64_t rows, int64_t n, int64_t ld, float* out, float beta, float* ws, uint32_t x_bf16, void* stream);
int64_t hftt_colsum_ws_bytes(int64_t rows, int64_t n);
/* hftt_dropout_bwd and hftt_colsum in one pass over g (rows x n, row stride ld): every quad of g is read once, masked in place and summed.
 * The element index of the keep decision is the element's offset r*ld + j in g (hftt_dropout_bwd over the rows*ld elements of the buffer
 * counts the same); the columns [n, ld) of a row are neither read nor written.  g (masked) and out are bit-identical to the two calls;
 * drop_p == 0: g is only read.  n % 4 == 0, ld % 4 == 0, g and ws 16-byte aligned, ws of hftt_colsum_ws_bytes(rows, n) bytes.  ADDED at ABI 8;
 * HFTT_ABI_VERSION stays 8. */
int hftt_dropout_bwd_colsum(float* g, int64_t rows, int64_t n, int64_t ld, float drop_p, uint32_t site, uint64_t seed, float* out, float beta,
                            float* ws, uint32_t bf16, void* stream);
/* heads: logits [S, ldl] with cols [0,V) velocity, V onset, V+1 offset, V+2 mpe ->
 *   velocity [.,V] raw, onset/offset/mpe sigmoid; time_major!=0: rows are (b,n,t) and outputs are (b,t,n). */
int hftt_heads_split(const float* logits, int64_t ldl, float* onset, float* offset, float* mpe, float* velocity,
                     int32_t B, int32_t T, int32_t Nn, int32_t V, int32_t time_major, void* stream);
/* backward of hftt_heads_split: dlogits[., ldl] from d(onset,offset,mpe probabilities) and d(velocity logits) */
int hftt_heads_split_bwd(const float* p_onset, const float* p_offset, const float* p_mpe,
                         const float* d_onset, const float* d_offset, const float* d_mpe, const float* d_velocity,
                         float* dlogits, int64_t ldl, int32_t B, int32_t T, int32_t Nn, int32_t V, int32_t time_major,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Loss (training/train.py:141-153): 6x BCELoss(mean) + 2x CrossEntropyLoss(mean), weighted sum.
 * loss_out[0] = total, [1..8] = the eight terms.  Gradients w.r.t. the eight model outputs are
 * written when the d_* pointers are non-NULL (scaled by grad_scale, normally 1).
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t n;            /* B*T*Nn label elements */
  int32_t V; int32_t pad;
  const float* prob[6]; /* onset_A, offset_A, mpe_A, onset_B, offset_B, mpe_B : [n] */
  const float* vel[2];  /* velocity_A, velocity_B : [n, V] logits */
  const float* label_onset; const float* label_offset; const float* label_mpe; const int64_t* label_velocity;
  float weight_A, weight_B, grad_scale; float pad2;
  float* d_prob[6]; float* d_vel[2];
  float* loss_out;      /* [9] */
  float* ws;            /* hftt_loss_ws_bytes(n) */
} hftt_loss_desc;
int64_t hftt_loss_ws_bytes(int64_t n);
int hftt_loss(const hftt_loss_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused Adam over one flat parameter buffer (torch.optim.Adam defaults, m_training.py:146):
 *   m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * Hyper-parameters are doubles (python floats): 1-b1, 1-b2 and the bias corrections are formed in double and rounded once, like torch.
 * --------------------------------------------------------------------------------------------- */
int hftt_adam_step(float* p, const float* g, float* m, float* v, int64_t n, int32_t step,
                   double lr, double beta1, double beta2, double eps, double grad_scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Log-mel front end (model/amt.py:55-63 after resampling): frames of n_fft with hop, centred,
 * zero padded, periodic hann, |rDFT|^2, sparse slaney/htk mel filterbank, log(. + offset).
 * feat [n_frames, n_mels], n_frames = 1 + n_samples/hop.  fb is given in CSR-by-mel form.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  const float* wave; int64_t n_samples;
  int32_t n_fft, hop, n_mels, n_frames;
  const float* window;       /* [n_fft] */
  const float* twiddle;      /* [n_fft/2] cos, then [n_fft/2] sin of 2*pi*k/n_fft */
  const int32_t* fb_start;   /* [n_mels] first frequency bin of each mel filter */
  const int32_t* fb_len;     /* [n_mels] number of bins */
  const int32_t* fb_off;     /* [n_mels] offset into fb_w */
  const float* fb_w;         /* packed weights */
  float log_offset; int32_t pad;
  float* feat;
} hftt_logmel_desc;
int hftt_logmel(const hftt_logmel_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Resampling in front of the log-mel (model/amt.py:57-58: torchaudio.transforms.Resample(sr, 16000) with its defaults -- Hann-windowed sinc,
 * lowpass_filter_width 6, rolloff 0.99; torchaudio is un-vendored and absent: published algorithm, parity unpinned).  With g = gcd(sr_in,
 * sr_out), down = sr_in / g, up = sr_out / g, width = ceil(6 * down / (min(down, up) * 0.99)): the host builds the kernel table
 * kernel[up, taps], taps = 2 * width + down (row p = the windowed sinc sampled for output phase p), and
 *     out[f * up + p] = sum_t wave[f * down - width + t] * kernel[p, t]          (samples outside [0, n_in) are zeros)
 * for the first n_out = ceil(n_in * up / down) outputs.  fp32 accumulate, four interleaved partial sums over the taps (t mod 4), added at the end.
 * The input window of 256 consecutive outputs, (255 / up + 1) * down + taps samples, is staged in LDS: it must fit 64 KB (it does for every
 * audio rate down to 16 kHz from <= 768 kHz).
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  const float* wave; int64_t n_in;
  const float* kernel;       /* [up, taps] */
  int32_t up, down, width, taps;
  float* out; int64_t n_out;
} hftt_resample_desc;
int hftt_resample(const hftt_resample_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Note decoding on the device (csrc/notes.hip).  These entry points were ADDED at ABI 8: HFTT_ABI_VERSION stays 8, because nothing that an
 * ABI-8 caller binds changed -- a caller that needs them looks the symbols up and treats their absence as an older library.
 *
 * Stitch (model/amt.py:104-113 transcript, :155-176 transcript_stride; the velocity argmax of :107,113): per clip c < b of one model call,
 * rows src0 .. src0 + len of the [b, T, N] fp32 posteriors onset / offset / mpe go to rows dst[c] .. dst[c] + len of the [F, N] fp32 rolls,
 * and for the same rows roll_velocity [F, N] int8 receives the argmax over the last axis of the [b, T, N, V] fp32 velocity logits (ties: the
 * lowest index, as torch.argmax / numpy.argmax; NaN counts as the maximum).  transcript: src0 = 0, len = T; transcript_stride:
 * src0 = n_offset, len = T / 2.  Rows that no clip covers are not touched.  No atomics: every element has one writer, so the row ranges of
 * the clips must not overlap.  `dst` is a HOST array of b ints (read during the call, b <= HFTT_STITCH_MAX_CLIPS); every other pointer is
 * device memory.  With V % 4 == 0 and a 16-byte aligned `velocity` the logits are read with 16-byte loads.
 * --------------------------------------------------------------------------------------------- */
#define HFTT_STITCH_MAX_CLIPS 64
typedef struct {
  int32_t b, T, N, V;          /* clips of this call, frames per clip, notes (1..128), velocity classes (1..128) */
  int32_t src0, len;           /* 1 <= len <= T, 0 <= src0 <= T - len */
  int64_t F;                   /* rows of the rolls */
  const void* onset; const void* offset; const void* mpe;        /* fp32 [b, T, N] */
  const void* velocity;                                          /* fp32 [b, T, N, V] logits */
  void* roll_onset; void* roll_offset; void* roll_mpe;           /* fp32 [F, N] */
  void* roll_velocity;                                           /* int8 [F, N] */
  const int32_t* dst;          /* HOST [b]: first roll row of each clip, 0 <= dst[c] <= F - len */
} hftt_stitch_desc;
int hftt_stitch(const hftt_stitch_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Notes (model/amt.py:179-341 mpe2note, up to but without the final sort of :343): the rolls of one file -> its notes, in caller-supplied
 * arrays of capacity `cap`, pitch-major and by ascending onset frame within a pitch (the order of a_note in front of :343).
 *   peaks (:193-253)   every frame of a plateau is a peak when its value is >= the threshold and the nearest DIFFERENT value on each side is
 *                      smaller or absent (a constant track above the threshold has F peaks: up to N * F notes exist).  Time: loc * hop_sec in
 *                      double at frame 0, at F - 1 and between equal neighbours l == r; else float32(loc * hop_sec) - h2 * (l - r) / (c - r)
 *                      for l > r, + h2 * (r - l) / (c - l) for l < r, with h2 = float32(hop_sec / 2), in fp32 (subtract, multiply,
 *                      correctly rounded divide, subtract; no contraction), widened to double.
 *   per onset (:255-336)  next onset = the next onset peak, or (F, (F - 1) * hop_sec); offset peak = the first with loc > loc_onset, clipped
 *                      to the next onset; mpe end = the first frame of [loc_onset + 1, loc_next) below thred_mpe, at loc * hop_sec; the note's
 *                      offset by the two flags and mode_offset; mode_velocity 0 drops velocity 0.
 *   trim (:338-341)    between consecutive KEPT notes of one pitch: prev.offset = next.onset when next.onset < prev.offset.
 * Thresholds are floats: the reference compares float32 rolls with a Python scalar, i.e. in float32.  *n_notes receives the number of notes
 * that EXIST; when it exceeds cap, records 0 .. cap are written, nothing behind them, and the caller repeats the call with more room.
 * The order is deterministic (prefix sums, no atomics).  ws: hftt_notes_ws_bytes(F, N) bytes, contents irrelevant on entry.  F == 0: *n_notes
 * = 0, no kernel.  Frames are handled in chunks of HFTT_NOTES_CHUNK: one workgroup per pitch walks the chunks once forward and once backward
 * carrying two ints per track, then one workgroup per (chunk, pitch) writes the notes.
 * --------------------------------------------------------------------------------------------- */
#define HFTT_NOTES_CHUNK 256
typedef struct {
  int64_t F; int32_t N; int32_t note_min;                        /* frames, notes (1..128), pitch of note 0 */
  const void* onset; const void* offset; const void* mpe;        /* fp32 [F, N] */
  const void* velocity;                                          /* int8 [F, N] */
  float thred_onset, thred_offset, thred_mpe;
  int32_t mode_velocity;       /* 0 = ignore_zero, 1 = org */
  int32_t mode_offset;         /* 0 = shorter, 1 = longer, 2 = offset */
  int32_t cap;                 /* capacity of the four output arrays, >= 0 */
  double hop_sec;
  void* out_pitch; void* out_velocity;                           /* int32 [cap] */
  void* out_onset; void* out_offset;                             /* double [cap] */
  void* n_notes;                                                 /* int32 [1] */
  void* ws; int64_t ws_bytes;
} hftt_notes_desc;
int64_t hftt_notes_ws_bytes(int64_t F, int32_t N);
int hftt_notes_decode(const hftt_notes_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Many files at once (the file loop of evaluation/m_inference.py:77-165 around model/amt.py:66-176): the clip windows of a whole file list
 * in one launch, and one decode over rolls that hold all files back to back.  Like the entry points above these were ADDED at ABI 8 and
 * HFTT_ABI_VERSION stays 8.
 *
 * Clip windows (model/amt.py:89 a_input[i:i+width].T, with the min_value padding of :71-79 / :126-137 applied per window, not per file):
 * `feature` holds the files' feature rows concatenated, file f = rows file_row0[f] .. file_row0[f + 1] (n_f rows, 0 allowed).  Window b shows
 * frames win_start[b] .. win_start[b] + width of file win_file[b], counted from the file's frame 0 (the start may be negative or lie behind
 * the file):
 *     out[b, k, t] = feature[file_row0[f] + s + t, k]   when 0 <= s + t < n_f,   else fill
 * and every element of a window whose file index is outside 0 .. n_files is fill: a window never shows a neighbouring file's frames.  A file
 * whose rows do not lie inside 0 .. R is treated as outside as well (nothing is read there).  All pointers are DEVICE memory, nothing is read
 * on the host.  One launch: a workgroup moves a tile of 64 frames x 64 bins through LDS -- read along the bins, written along the frames, both
 * as whole 256-byte wave accesses; the tile row is padded by one word, so the column read meets 64 different banks.  One writer per element,
 * no atomics, 64-bit indexing (R * n_bins may pass 2^31); n_bins and width need not be multiples of the tile.
 * Refused in front of the launch: null pointers; B, width or n_bins < 1; n_files < 0; R < 0; B * n_bins * width >= 2^31.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  const void* feature;                                           /* fp32 [R, n_bins] */
  const int32_t* file_row0;                                      /* [n_files + 1] */
  const int32_t* win_file; const int32_t* win_start;             /* [B] */
  int32_t B, width, n_bins, n_files;
  int64_t R;
  float fill; int32_t pad;     /* fill: the config's min_value */
  void* out;                                                     /* fp32 [B, n_bins, width] */
} hftt_clip_windows_desc;
int hftt_clip_windows(const hftt_clip_windows_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Segmented notes: `notes` describes rolls of F rows that hold n_seg segments (files) back to back, segment s = rows seg_row0[s] ..
 * seg_row0[s + 1].  For every segment the notes are EXACTLY those of the one-file decode above on these rows alone, with F equal to the
 * segment's length F_s: plateaus, peaks, the "next onset" default (F_s, (F_s - 1) * hop_sec), the edge rule of the peak time (frame 0 and
 * F_s - 1) and every time loc * hop_sec are counted inside the segment; nothing is looked up across a border.  Order: segment-major, then
 * pitch-major, then ascending onset frame.  seg_notes[s] = the number of notes in front of segment s; seg_notes[n_seg] == *n_notes = the
 * number that exist; records behind cap are not written.  Segments of zero rows are legal and empty; n_seg == 0 or F == 0: zero notes.
 * seg_row0_host is a HOST array, read and checked during the call ([0] == 0, non-decreasing, [n_seg] == F); seg_row0 holds the same values
 * in DEVICE memory (uploaded by the caller) and is what the kernels read.  A segment whose device rows disagree with the host table's bounds
 * is skipped, never followed out of the rolls or the workspace.
 * Kernels: a table kernel writes the prefix of the per-segment chunk counts ceil(F_s / HFTT_NOTES_CHUNK) into ws; the scan runs one workgroup
 * per (pitch, segment); counts lie [segment][pitch][chunk], so one prefix sum yields the order above and, at the segment heads, seg_notes; the
 * emit kernel runs one workgroup per (chunk of any segment, pitch) and finds its segment in the table.  No atomics.
 * Refused on top of the one-file decode's rejections: n_seg < 0 (or n_seg * N >= 2^31); a table pointer null at n_seg > 0; a table check
 * failing; seg_notes null;
 * ws_bytes below the value of the workspace helper (which is 0 for arguments outside the domain).
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  hftt_notes_desc notes;       /* F = rows of all segments; ws sized by the helper below */
  int32_t n_seg; int32_t pad;
  const int32_t* seg_row0_host;                                  /* HOST [n_seg + 1] */
  const void* seg_row0;                                          /* DEVICE int32 [n_seg + 1], the same values */
  void* seg_notes;                                               /* DEVICE int32 [n_seg + 1], output */
} hftt_notes_seg_desc;
int64_t hftt_notes_seg_ws_bytes(int64_t F, int32_t N, int32_t n_seg);
int hftt_notes_decode_seg(const hftt_notes_seg_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Streaming notes (csrc/notes_stream.hip; model/amt.py:179-341 mpe2note, mode_offset 'shorter' ONLY): the decode above with its state
 * carried forward.  S streams each keep their four rolls as a RING of H rows, [S, H, N]; row r of stream s lives at ring row r % H.
 * row_end[s] (DEVICE int64) is the number of rows delivered so far, closed[s] (DEVICE int32) != 0 says that the stream has ended and
 * row_end[s] is its F.  One call returns every note that NO LATER ROW CAN CHANGE and that no earlier call returned: over all calls of a
 * stream, the closing one included, the notes are exactly those of hftt_notes_decode on the whole rolls, none missing, none twice, for any
 * split of the rows into calls (calls without new rows and calls of one row included).  ADDED at ABI 8; HFTT_ABI_VERSION stays 8.
 *
 * When a note is final.  A frame of a track is DECIDED when its peak status cannot change: its value is below the threshold, or not above the
 * run in front of it, or its run has ended.  Only the trailing run can be undecided.  For the kept onset peak f of a pitch:
 *   A  a next onset peak ln is decided: the mpe end comes from rows < ln; the offset peak p <= ln when one is decided, else "clipped to ln" as
 *      soon as every offset frame <= ln is decided (under 'shorter' clipped and absent give the same value); the trim uses ln when it is kept,
 *      else frame ln + 1 of the same plateau when that is kept -- from ln + 2 on every onset time lies a whole hop above the value.
 *   B  none is decided: the deciding event ev is the first decided offset peak with no frame below thred_mpe in front of it, or the first such
 *      frame with every offset frame up to it decided; the note is final once the onset frames <= ev + 1 are decided and hold no peak.
 *   At the close the horizon is F and what is pending follows the offline rules, with F in the peak time's edge rule and the last "next onset".
 * With 'longer' / 'offset' a note may depend on whether an offset peak occurs anywhere later: the number of pending notes is unbounded, so
 * these modes are refused by name.
 *
 * State: hftt_notes_stream_state_bytes(S, N) bytes, ALL ZERO for fresh streams; 64 bytes per (stream, pitch) -- the commit frame c (every
 * onset peak in front of it is returned or is the one pending head), the last row_end, the head's frame, time and velocity, on / off[c - 1]
 * and the value of the run in front of theirs -- plus one int32 each that is zero between calls.  Its size does not depend on the stream's age,
 * and a call reads rows c .. row_end only: its cost depends on the new rows and the undecided stretch, never on the age.
 * Outputs: records within cap in stream-major, pitch-major, ascending-onset-frame order (prefix sums, no atomics), stream s = records
 * stream_notes[s] .. stream_notes[s + 1]; *n_notes = stream_notes[S] = the number that this call found.  When it exceeds cap NOTHING is
 * written to the records and the state STAYS AS IT WAS: the caller repeats the call with more room.  overflow[s] != 0: the rows that stream s
 * still needs (an undecided plateau at or above a threshold, or more new rows than H) no longer lie in the ring; the stream returns nothing
 * from then on -- a status, not a fault.  A closed stream that has been decoded returns nothing more.
 * Kernels: one lane per (stream, pitch), one workgroup of 128 per stream, walks its rows sequentially (N is the contiguous axis: a wave reads
 * whole rows); a count pass, a prefix sum, and an emit pass that alone commits the state.  Frame indices are int64.
 * Refused in front of the launch: null pointers; S < 1 (or S * N >= 2^24); N outside 1..128; H < 4; max_new outside 0..H (the largest number
 * of rows any stream received since its last call, as the host knows it); mode_offset != 0; mode_velocity outside 0..1; cap < 0; state_bytes
 * below the helper's value (0 for arguments outside the domain).
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t S, N, H, note_min;                                     /* streams, notes (1..128), ring rows (>= 4), pitch of note 0 */
  const void* onset; const void* offset; const void* mpe;        /* fp32 [S, H, N] */
  const void* velocity;                                          /* int8 [S, H, N] */
  const void* row_end;                                           /* DEVICE int64 [S] */
  const void* closed;                                            /* DEVICE int32 [S] */
  float thred_onset, thred_offset, thred_mpe;
  int32_t mode_velocity;       /* 0 = ignore_zero, 1 = org */
  int32_t mode_offset;         /* 0 = shorter; nothing else */
  int32_t cap;                 /* capacity of the four output arrays, >= 0 */
  int32_t max_new; int32_t pad;
  double hop_sec;
  void* state; int64_t state_bytes;
  void* out_pitch; void* out_velocity;                           /* int32 [cap] */
  void* out_onset; void* out_offset;                             /* double [cap] */
  void* stream_notes;                                            /* int32 [S + 1] */
  void* n_notes;                                                 /* int32 [1] */
  void* overflow;                                                /* int32 [S] */
} hftt_notes_stream_desc;
int64_t hftt_notes_stream_state_bytes(int32_t S, int32_t N);
int hftt_notes_stream_step(const hftt_notes_stream_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Label rendering on the device (csrc/labels.hip): note lists -> the frame labels that training consumes, the opposite direction of the
 * decoder above (corpus/conv_note2label.py:8-111 note2label).  Like the note decoder this entry point was ADDED at ABI 8 and HFTT_ABI_VERSION
 * stays 8: a caller that needs it looks the symbol up.
 *
 * Note table (device memory, corpus-wide, built once by the caller): `notes` holds the records of every file grouped by (file, pitch) -- group
 * g = file * N + pitch is records row_ptr[g] .. row_ptr[g + 1] -- and inside a group in the ORDER OF THE CALLER'S NOTE LIST (never sorted by
 * time: the order decides the velocity where onset triangles overlap).  flags bit 0 = "no offset target": the note's offset equals, as a
 * double, the onset of a note of the same pitch in the same file (:76-83).  file_nframe[file] = int(max offset * fps + 0.5) + 1 (:20-27), 1
 * for a file without notes.
 *
 * Request: B windows of `len` frames; window b shows frames win_start[b] .. win_start[b] + len of file win_file[b], counted from the file's
 * frame 0 (win_start may be negative or lie behind the file).  win_file / win_start are DEVICE arrays: nothing is read on the host.  Frames
 * outside [0, file_nframe) -- and every frame of a window whose file index is outside 0 .. n_files -- are zero in all four tracks.
 *
 * One output element = frame f of one pitch: walk the group's notes in table order carrying o, off (fp32), mpe, vel (all 0 at the start):
 *   on_f = (int)(onset * fps + 0.5), off_f = (int)(offset * fps + 0.5), on_ms = onset * 1000.0, off_ms = offset * 1000.0            (:37-43)
 *   sharp = tol, with duration_tolerance: max(tol, (int)((off_ms - on_ms) * 0.2 / hop_ms + 0.5))                                    (:46-48)
 *   |f - on_f| <= tol:  o = max(o, (float)max(0.0, 1.0 - fabs(f * hop_ms - on_ms) / (tol * hop_ms)));                               (:53-70)
 *                       o >= 0.5f and (f >= on_f or vel == 0): vel = velocity     (the VALUE vel == 0 is tested, after the max)
 *   on_f <= f <= off_f: mpe = 1                                                                                                     (:72-74)
 *   bit 0 clear and |f - off_f| <= sharp: off = max(off, the same triangle around off_ms with half-width sharp)                     (:85-97)
 * in fp64 without contraction and with IEEE division: operation for operation the reference's arithmetic, so the result is bit-identical to
 * it.  hop_ms = 1000 * hop_sample / sr, fps = sr / hop_sample and tol = int(50.0 / hop_ms + 0.5) come from the host, computed as there.
 *
 * form HFTT_LABELS_TRAIN: onset / offset / mpe fp32 [B, len, N], velocity int64 (what the loss takes); HFTT_LABELS_STORE: onset / offset fp32,
 * mpe uint8, velocity int8 (the dtypes of the stored tracks).  One launch; a workgroup owns (window, pitch, HFTT_LABELS_CHUNK frames), filters
 * the pitch's notes against its frame range HFTT_LABELS_CHUNK at a time into LDS in order (prefix sum), and each frame walks the survivors.
 * One writer per element, no atomics, no workspace.
 * --------------------------------------------------------------------------------------------- */
#define HFTT_LABELS_CHUNK 256
#define HFTT_LABELS_TRAIN 0
#define HFTT_LABELS_STORE 1
typedef struct {
  double onset_sec, offset_sec;
  int32_t velocity;
  int32_t flags;               /* bit 0: no offset target */
} hftt_label_note;
typedef struct {
  const hftt_label_note* notes;                                  /* [n_notes] (may be NULL when n_notes == 0) */
  const int32_t* row_ptr;                                        /* [n_files * N + 1] */
  const int32_t* file_nframe;                                    /* [n_files] */
  const int32_t* win_file; const int32_t* win_start;             /* [B] */
  int32_t n_files, n_notes;
  int32_t B, len, N;           /* windows, frames per window, notes (1..128); B * len * N < 2^31 */
  int32_t tol;                 /* >= 1 */
  int32_t duration_tolerance;  /* 0 / 1 */
  int32_t form;                /* HFTT_LABELS_TRAIN / HFTT_LABELS_STORE */
  double hop_ms, fps;
  void* onset; void* offset; void* mpe; void* velocity;          /* [B, len, N] */
} hftt_labels_desc;
int hftt_labels_render(const hftt_labels_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Clip log-mel (csrc/clip_logmel.hip): the spectrogram windows of a training batch computed from a resident WAVEFORM corpus when the batch is
 * gathered -- what the clip windows above cut out of stored features, without the stored features.  ADDED at ABI 8; HFTT_ABI_VERSION stays 8.
 *
 * Corpus (device memory): `wave` holds the files' samples at the feature rate, concatenated without padding, as fp32 (wave_i16 = 0) or int16
 * (wave_i16 = 1: the sample value is (float)s * (1 / 32768), exact); file f owns samples file_samp0[f] .. file_samp0[f + 1] (n of them, 0
 * allowed).  Request: B windows of `width` frames; window b shows frames win_start[b] .. win_start[b] + width of file f = win_file[b], counted
 * from the file's frame 0 (the start may be negative or lie behind the file: the convention of the clip windows and the label renderer).
 *     out[b, m, c] = log-mel bin m of frame t = win_start[b] + c of THAT FILE'S waveform alone       when 0 <= t < 1 + n / hop
 *                  = fill (to the bit)                                                               otherwise
 * with the frame as the log-mel front end above defines it: samples t * hop - n_fft / 2 .. + n_fft, zeros outside [0, n) -- a neighbouring
 * file's samples never enter -- times the window, |rDFT|^2, CSR mel sum, logf(. + log_offset); the tables have the formats of
 * hftt_logmel_desc.  A window whose file index is outside 0 .. n_files, or whose file does not lie inside 0 .. total_samples, is fill.
 *
 * Augmentation, per window, on the sample in front of the window product (both pointers may be NULL; with both NULL the sample is untouched):
 *     gain [B]       x <- fmul(x, gain[b])                                              (one rounding)
 *     noise_std [B]  x <- fadd(x, fmul((float)(b0 + b1 + b2 + b3 - 510), fmul(noise_std[b], C)))        (one rounding each, never an fma)
 * b0 .. b3 = the four bytes of the library's counter hash (csrc/hftt_common.h) of (seed, site = file, index = the sample's position inside its
 * file); C = 1 / sqrt(21845) rounded to fp32 (the sum of four uniform bytes has mean 510 and variance 21845, so the term has standard
 * deviation noise_std[b]).  The noise is keyed on the sample: the frames that overlap it, and two windows of one call that overlap, see the same
 * noisy waveform.  The zeros outside the file stay zeros.
 *
 * One launch: a workgroup owns a window and HFTT_CLIP_LOGMEL_RUN consecutive frames, stages the (RUN - 1) * hop + n_fft samples they cover once
 * in LDS, transforms frame after frame, and stores its [n_mels, RUN] tile along the frame axis (64 contiguous bytes per row).  One writer per
 * element, no atomics, no workspace, 64-bit sample indices.
 * Refused in front of the launch: null pointers (gain / noise_std excepted); wave_i16 outside 0 / 1; n_fft != 2048; B, width, hop or n_files
 * < 1; n_mels outside 1 .. HFTT_CLIP_LOGMEL_MAX_MELS; total_samples < 0; a hop whose staged samples pass 64 KB of LDS (hop <= 324 fits).
 * --------------------------------------------------------------------------------------------- */
#define HFTT_CLIP_LOGMEL_RUN 16
#define HFTT_CLIP_LOGMEL_MAX_MELS 256
typedef struct {
  const void* wave;                                              /* fp32 or int16 [total_samples] */
  const int64_t* file_samp0;                                     /* [n_files + 1] */
  const int32_t* win_file; const int32_t* win_start;             /* [B] */
  int64_t total_samples;
  int32_t wave_i16, n_files, B, width;
  int32_t n_fft, hop, n_mels;
  float log_offset;
  const float* window; const float* twiddle;                     /* as hftt_logmel_desc */
  const int32_t* fb_start; const int32_t* fb_len; const int32_t* fb_off; const float* fb_w;
  float fill; int32_t pad;     /* fill: the config's min_value */
  const float* gain; const float* noise_std;                     /* [B] or NULL */
  uint64_t seed;
  void* out;                                                     /* fp32 [B, n_mels, width] */
} hftt_clip_logmel_desc;
int hftt_clip_logmel(const hftt_clip_logmel_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pitch-shift and timing augmentation (csrc/wave_warp.h, csrc/wave_warp.hip, csrc/clip_logmel.hip, csrc/labels.hip): a clip played back at
 * rate r = 2^((k + c) / 12) -- every pitch moves by k semitones plus a detune c, every note time scales by 1 / r -- resampled while the clip's
 * samples are staged, and the labels rendered under the matching map.  Three entry points ADDED at ABI 8; HFTT_ABI_VERSION stays 8 and every
 * descriptor above keeps its layout.
 *
 * The warp of one window b -- fixed point, no floating-point positions:
 *     step_q24[b]   int32, r * 2^24, HFTT_WARP_STEP_MIN <= step <= HFTT_WARP_STEP_MAX (2^23 .. 2^25: one octave either way)
 *     delay_q24[b]  int64, source samples * 2^24, 0 <= delay <= HFTT_WARP_DELAY_MAX (2^48): a DELAY, so warped note times never go negative
 *     cut[b]        float, the cutoff relative to the source's Nyquist rate: 0.99 * min(1, 2^24 / step), supplied by the host
 * A window whose step or delay lies outside these ranges, or whose cut lies outside 0.25 .. 1 (a NaN included), is treated as a window
 * without a file (fill / zeros).
 * Warped sample j of a file with n source samples reads source position pos = j * step - delay (int64, Q24).  The warped file has
 *     n' = 0 for n = 0, else floor((((n - 1) << 24) + delay) / step) + 1 samples       and 1 + n' / hop frames;
 * warped samples outside [0, n') are zeros.  Inside, with `#pragma clang fp contract(off)` (every operation below is one fp32 rounding):
 *     acc = 0; for i = (pos >> 24) - H .. (pos >> 24) + H + 1 in INCREASING order, skipping i outside [0, n) (zeros outside the file: a
 *     neighbouring file's samples never enter), with d = |pos - (i << 24)| (int64):
 *         q = fmul((float)d, cut[b])                     (int64 -> fp32 round-to-nearest, then one product)
 *         skipped unless q <= Z * 2^24                   (Z = HFTT_WARP_ZEROS = 6 zero crossings either side)
 *         x = fmul(q, L / 2^24)                          (L = HFTT_WARP_TABLE_L = 512 entries per zero crossing: a power of two, exact)
 *         e = (int)x; f = x - (float)e                   (truncation; the difference is exact)
 *         w = fadd(T[e], fmul(f, fsub(T[e + 1], T[e])))  (the prototype, linearly interpolated)
 *         acc = fadd(acc, fmul(fmul(w, cut[b]), s_i))    (s_i: the source sample, an int16 one dequantised first as (float)s * (1 / 32768))
 * H = (int)(Z / cut[b]) + 2 only has to cover every i that passes the test on q (at most 2 Z / cut + 1 <= 26 of them do).
 * T = the prototype sinc(u) * cos^2(pi u / 2Z) at u = e / L, e = 0 .. Z L, built by the host in fp64 and rounded once to fp32
 * (HFTT_WARP_TABLE_LEN = Z L + 2 entries; the last two are exact zeros).  This is a Hann-windowed sinc with the published defaults
 * (lowpass_filter_width 6, rolloff 0.99) scaled to the cutoff.
 * Identity bypass: a window with step == 2^24 and delay a multiple of 2^24 takes source sample j - (delay >> 24) directly (zero outside
 * [0, n)).  The condition is uniform per window.
 *
 * hftt_wave_warp: out[b, c] (fp32 [B, len]) = warped sample win_start[b] + c (win_start int64) of file win_file[b] under window b's warp, BEFORE
 * gain and noise; 0 outside [0, n') and for a window without a (valid) file.  It makes the interpolation observable and writes an augmented copy
 * of a file.  One thread per output sample; the sample is the ONE device function (csrc/wave_warp.h) that the staging loop below calls.
 * Refused: null pointers; wave_i16 outside 0 / 1; B, len or n_files < 1; total_samples outside 0 .. 2^38; B * ceil(len / 256) >= 2^31.
 *
 * hftt_clip_logmel_warp: hftt_clip_logmel (`base`: outputs, fill rule, tile store and refusals as there) with win_start counted in frames of
 * the WARPED file (1 + n' / hop of them) and the staged sample j = the warped sample j.  Gain and noise are applied to the warped sample by
 * the same two operations, the noise keyed on (seed, file, j): it stays white and does not pass through the filter.  A window that takes the
 * identity bypass is bit-identical to hftt_clip_logmel on the file with delay >> 24 zeros put in front: with delay = 0 the same window, with
 * delay = m * hop samples (and no noise, which is keyed on j) the window at win_start - m.  The taps are read from global memory (neighbouring lanes
 * read overlapping spans); the LDS arrays are hftt_clip_logmel's.  Also refused: null step_q24 / delay_q24 / cut / proto; total_samples > 2^38.
 *
 * hftt_labels_render_warp: hftt_labels_render (`base`) under the map of the same warp:
 *     output pitch j of window b walks group file * N + (j - shift[b]); a source pitch outside 0 .. N gives an all-zero column
 *     every note time t becomes t' = fmul(fadd(t, t_delay[b]), t_scale[b]) (fp64, two roundings, never an fma); the arithmetic of
 *     hftt_labels_render then runs on t' unchanged
 *     file_nframe' = (int)(fmul(fmul(fadd(file_end_sec[file], t_delay[b]), t_scale[b]), fps) + 0.5) + 1, and 1 for a file without notes
 *     (row_ptr[file * N] == row_ptr[file * N + N]); file_end_sec[file] = the largest offset over ALL the file's notes, 0 without notes
 *     flags bit 0 is the table's, that is, the unwarped list's; win_start counts frames of the warped file; base.file_nframe is not read
 * with t_scale = 2^24 / step and t_delay = delay / 2^24 / sr formed by the caller in fp64.  Also refused: null shift / t_delay / t_scale /
 * file_end_sec.
 * --------------------------------------------------------------------------------------------- */
#define HFTT_WARP_ZEROS 6
#define HFTT_WARP_TABLE_L 512
#define HFTT_WARP_TABLE_LEN (HFTT_WARP_ZEROS * HFTT_WARP_TABLE_L + 2)
#define HFTT_WARP_STEP_MIN (1 << 23)
#define HFTT_WARP_STEP_MAX (1 << 25)
#define HFTT_WARP_DELAY_MAX ((int64_t)1 << 48)
typedef struct {
  const int32_t* step_q24;     /* [B] */
  const int64_t* delay_q24;    /* [B] */
  const float* cut;            /* [B] */
  const float* proto;          /* [HFTT_WARP_TABLE_LEN] */
} hftt_warp_args;
typedef struct {
  hftt_clip_logmel_desc base;
  hftt_warp_args warp;
} hftt_clip_logmel_warp_desc;
int hftt_clip_logmel_warp(const hftt_clip_logmel_warp_desc* d, void* stream);
typedef struct {
  const void* wave;                                              /* fp32 or int16 [total_samples] */
  const int64_t* file_samp0;                                     /* [n_files + 1] */
  const int32_t* win_file; const int64_t* win_start;             /* [B]; win_start in warped samples */
  int64_t total_samples;
  int32_t wave_i16, n_files, B, len;
  hftt_warp_args warp;
  void* out;                                                     /* fp32 [B, len] */
} hftt_wave_warp_desc;
int hftt_wave_warp(const hftt_wave_warp_desc* d, void* stream);
typedef struct {
  hftt_labels_desc base;
  const int32_t* shift;                                          /* [B] semitones */
  const double* t_delay; const double* t_scale;                  /* [B] */
  const double* file_end_sec;                                    /* [n_files] */
} hftt_labels_warp_desc;
int hftt_labels_render_warp(const hftt_labels_warp_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Clip mixing (csrc/clip_logmel.hip, csrc/labels.hip): two clips summed while the samples are
 * staged, and the labels of the sum -- the one augmentation that changes the polyphony.  Three entry points ADDED at ABI 8; HFTT_ABI_VERSION
 * stays 8 and every descriptor above keeps its layout and its results.
 *
 * Window b has its PRIMARY (win_file[b], win_start[b]) with its optional warp entry, exactly as above, and an optional PARTNER:
 *     mix_file[b]   int32: an index outside 0 .. n_files (negative included), or a file that leaves the corpus, contributes nothing
 *     mix_start[b]  int32: column c shows primary frame win_start[b] + c and partner frame mix_start[b] + c, each counted in its own (warped) file
 *     mix_gain[b]   float
 *     under the warp forms the partner's own step_q24 / delay_q24 / cut (a partner whose warp lies outside the ranges above contributes
 *     nothing) and its own label map shift / t_delay / t_scale
 *
 * hftt_clip_logmel_mix / hftt_clip_logmel_mix_warp: hftt_clip_logmel / hftt_clip_logmel_warp (`base`, `warp`: outputs, fill rule, tile store and
 * refusals as there) with the staged sample at primary position i, 0 <= i < n'_A (n' = n without a warp), formed as
 *     s = sA;  s = fmul(s, gain[b]) when gain is given;  s = fadd(s, fmul(sB, mix_gain[b])) when the window has a partner;  then the noise term
 *     as above, keyed on (seed, PRIMARY file, i)                              (one rounding per operation, never an fma)
 * sB = the partner's (warped) sample at i + (mix_start[b] - win_start[b]) * hop (int64), zero outside [0, n'_B).  Outside [0, n'_A) the staged
 * sample is zero: the partner is added ONTO the primary's extent, and which columns are `fill` follows the primary alone.  A window without a
 * partner is bit-identical to hftt_clip_logmel[_warp].  In the warp form both sources go through the one warped-sample function; its identity
 * bypass keeps an unwarped source exact.  The LDS arrays are hftt_clip_logmel's (the partner is added into the same staged slot), so hop 324
 * is still admitted.  Also refused: null mix_file / mix_start / mix_gain; in the warp form a null table of either warp.
 *
 * hftt_labels_render_mix: hftt_labels_render (`base`) with either source optionally under a warp map (shift / t_delay / t_scale all set or all
 * NULL for the primary; mix_shift / mix_t_delay / mix_t_scale likewise for the partner).  Cell (frame t of the window, pitch j):
 *     walks the primary's group at frame f = win_start[b] + t exactly as hftt_labels_render[_warp] does; its notes count where 0 <= f < nframe_A
 *     then walks the partner's group mix_file * N + (j - mix_shift[b]) at partner frame fB = mix_start[b] + t, CARRYING the same o, off, mpe,
 *     vel -- the reference writes velocity from the combined onset track and a carried vel == 0 test, so two separate renders combined
 *     afterwards are not this rule; the partner's notes count where 0 <= fB < nframe_B AND 0 <= f < a_frames[b]
 * nframe of a source = file_nframe[file] without a map, the warped count of hftt_labels_render_warp with one.  a_frames[b] (int64) is the
 * primary's AUDIO frame count 1 + n'_A / hop, formed by the caller on the device from the wave table and the warp (0 for a window without a
 * valid primary): the audio of a partner shows wherever the primary has audio frames, also behind the primary's last note.  flags bit 0 stays a
 * property of a note inside its own file.  The frame shift between the sources is an integer on purpose: seconds added to the partner's note
 * times would move frame_of and the fp64 triangle by an ulp.  With no partner the four tracks are bit-identical to hftt_labels_render[_warp].
 * Also refused: null mix_file / mix_start / a_frames; a warp map of which only a part is given; file_end_sec null with a map; file_nframe null
 * while a source has no map.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  const int32_t* mix_file; const int32_t* mix_start;             /* [B] */
  const float* mix_gain;                                         /* [B] */
} hftt_clip_mix_args;
typedef struct {
  hftt_clip_logmel_desc base;
  hftt_clip_mix_args mix;
} hftt_clip_logmel_mix_desc;
int hftt_clip_logmel_mix(const hftt_clip_logmel_mix_desc* d, void* stream);
typedef struct {
  hftt_clip_logmel_desc base;
  hftt_warp_args warp;                                           /* the primaries' */
  hftt_clip_mix_args mix;
  hftt_warp_args mix_warp;                                       /* the partners' */
} hftt_clip_logmel_mix_warp_desc;
int hftt_clip_logmel_mix_warp(const hftt_clip_logmel_mix_warp_desc* d, void* stream);
typedef struct {
  hftt_labels_desc base;
  const int32_t* shift; const double* t_delay; const double* t_scale;                    /* [B]: the primaries' map, or all NULL */
  const int32_t* mix_file; const int32_t* mix_start;                                     /* [B] */
  const int32_t* mix_shift; const double* mix_t_delay; const double* mix_t_scale;        /* [B]: the partners' map, or all NULL */
  const double* file_end_sec;                                                            /* [n_files]; NULL allowed without a map */
  const int64_t* a_frames;                                                               /* [B] */
} hftt_labels_mix_desc;
int hftt_labels_render_mix(const hftt_labels_mix_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Clip room (csrc/clip_room.hip, csrc/clip_dry.h): reverb and equalisation -- each window's dry signal convolved with one impulse response of
 * a device-resident bank while the batch is gathered.  It augments the clip log-mel above (hftt_clip_logmel and its warp / mix forms) and
 * touches none of their kernels: it writes a scratch corpus of WET samples that a plain, unchanged hftt_clip_logmel reads in a second launch.
 * One entry point ADDED at ABI 8; HFTT_ABI_VERSION stays 8 and every descriptor above keeps its layout and its results.
 *
 * Inputs: the corpus and window tables of hftt_clip_logmel_desc -- wave, wave_i16, file_samp0, n_files, total_samples, win_file, win_start, B,
 * width, hop, n_fft -- and gain [B] or NULL; `warp` (the primaries'), `mix` (the partners) and `mix_warp` (the partners' warps) exactly as the
 * four entry points above take them, a table with all pointers NULL being absent; mix_warp is given exactly when warp and mix both are.
 *     ir        fp32 [n_ir, L] in device memory, 1 <= L <= HFTT_ROOM_MAX_TAPS (0.5 s at 16 kHz); tap 0 is the direct path
 *     ir_taps   int32 [n_ir]: response r has taps k < ir_taps[r]; the entries at or behind it are not read.  Values outside 1 .. L cannot be
 *               refused by the host: the kernel clamps them into that range
 *     ir_index  int32 [B]: window b's response; negative: the window stays dry; >= n_ir: a window without a file (fill)
 * Dry signal of window b over its (warped) file of n' samples: dry_b[i], 0 <= i < n', is the value clip_logmel_kernel stages for file sample i
 * in front of the noise term (the primary through the warp or read directly, fmul by gain[b], fadd of fmul(partner, mix_gain[b]): one device
 * function, csrc/clip_dry.h, called by both kernels); dry_b[i] = 0 outside [0, n').
 * Wet signal:  wet_b[i] = sum over k < taps of h[k] * dry_b[i - k],  0 <= i < n',  taps = clamp(ir_taps[r], 1, L), formed in fp32 as
 *     acc = 0; for k = 0 .. taps - 1 in INCREASING order: acc = fma(h[k], dry_b[i - k], acc)            (one rounding per tap)
 * The tail behind the file's end is cut: the wet file is as long as the dry one, so its frame count 1 + n' / hop and every fill column are
 * what they were, and with tap 0 the direct path no onset moves: the labels are unchanged.  wet_b[i] depends on the window's sources, warps,
 * gains, its response and i only -- not on win_start, on where a workgroup's tile begins or on the launch geometry: two overlapping windows
 * with equal draws see the same wet waveform.  No atomics, one writer per element, the same bits from run to run.  A dry window
 * (ir_index[b] < 0) gets dry_b bit for bit.
 *
 * Outputs: out fp32 [B, span], span >= (P + width - 1) * hop + n_fft / 2 with P = ceil((n_fft / 2) / hop); and three tables that the kernel
 * writes itself: out_samp0 int64 [2 B + 1], out_win_file int32 [B], out_win_start int32 [B].  Row b of `out` holds two pseudo-files:
 *     2 b      wet_b[o_b .. e_b),   o_b = max(0, win_start[b] - P) * hop,   e_b = min(n', (win_start[b] + width - 1) * hop + n_fft / 2)
 *              (empty when e_b <= o_b)
 *     2 b + 1  the unused remainder of the row (not written), which keeps out_samp0 a gap-free prefix table: out_samp0[2 b] = b * span
 *     out_win_file[b] = 2 b,   out_win_start[b] = win_start[b] - o_b / hop
 * A window without a valid file, with o_b > n', or with a warp outside its ranges or ir_index[b] >= n_ir gets out_win_file[b] = -1.  With
 * these tables a plain hftt_clip_logmel over `out` (wave_i16 = 0, n_files = 2 B, total_samples = B * span, win_file = out_win_file, win_start =
 * out_win_start, gain NULL: it is already applied) gives, bit for bit and in the fill columns too, the result of hftt_clip_logmel on a file that
 * IS wet_b: a frame the clip shows never reads in front of o_b unless o_b = 0 (P * hop >= n_fft / 2), o_b is a multiple of hop, so
 * 1 + (n' - o_b) / hop counts the same last frame, and a pseudo-file cut at e_b < n' still holds every sample the last shown frame reads.
 * At o_b == n' the pseudo-file is empty and its one frame is pseudo-frame 0, in front of the P >= 1 the clip starts at: fill, as on the whole
 * file.  With n' == 0 a window at win_start <= P shows the empty file's one frame of zeros, a later one is fill.
 * Noise under a room is the SECOND launch's (its noise_std / seed): the microphone's, added behind the room.  It is keyed on (seed,
 * pseudo-file 2 b, position inside the pseudo-file), not on the source file and sample: two windows of one call no longer share it.
 *
 * One launch: a workgroup owns a window and a tile of 2,048 wet samples, stages the dry span they need once in LDS (taps rounded up to a
 * multiple of four, + 2,048 samples: 40 KB for the longest response) and walks the taps four at a time with eight outputs per thread in
 * registers; the taps are read from the bank in global memory.
 * Refused in front of the launch: null pointers (gain and absent tables excepted); a warp, mix or mix_warp table of which only a part is
 * given; mix_warp without both of the others or missing with both; wave_i16 outside 0 / 1; n_fft != 2048; B outside 1 .. 2^30; width, hop
 * or n_files < 1; total_samples < 0, or > 2^38 with a warp; n_ir < 1; L outside 1 .. HFTT_ROOM_MAX_TAPS; span below the bound above.
 * --------------------------------------------------------------------------------------------- */
#define HFTT_ROOM_MAX_TAPS 8192
typedef struct {
  const void* wave;                                              /* fp32 or int16 [total_samples] */
  const int64_t* file_samp0;                                     /* [n_files + 1] */
  const int32_t* win_file; const int32_t* win_start;             /* [B] */
  int64_t total_samples;
  int32_t wave_i16, n_files, B, width;
  int32_t n_fft, hop;
  int32_t n_ir, L;
  const float* gain;                                             /* [B] or NULL */
  hftt_warp_args warp;                                           /* the primaries', or all NULL */
  hftt_clip_mix_args mix;                                        /* the partners, or all NULL */
  hftt_warp_args mix_warp;                                       /* the partners' warps: given exactly when warp and mix are */
  const float* ir;                                               /* [n_ir, L] */
  const int32_t* ir_taps;                                        /* [n_ir] */
  const int32_t* ir_index;                                       /* [B] */
  int64_t span;
  void* out;                                                     /* fp32 [B, span] */
  int64_t* out_samp0;                                            /* [2 B + 1] */
  int32_t* out_win_file; int32_t* out_win_start;                 /* [B] */
} hftt_clip_room_desc;
int hftt_clip_room(const hftt_clip_room_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Clip synth (csrc/clip_synth.hip, csrc/clip_synth_fn.h): modal synthesis -- the windows of a training batch RENDERED from the note table of
 * the label renderer above under one voice of a device-resident bank each, so that a corpus needs note lists only: no audio is collected,
 * aligned or stored.  It writes the scratch corpus and the three tables of hftt_clip_room, under which the unchanged hftt_clip_logmel reads
 * device-made samples as files.  One entry point ADDED at ABI 8; HFTT_ABI_VERSION stays 8 and every descriptor above keeps its layout.
 *
 * Inputs: the note table of hftt_labels_desc -- notes, row_ptr, n_files, n_notes, N -- and file_nsamp int64 [n_files], the length n' of each
 * synthetic file in samples (negative: 0); the window tables win_file / win_start [B] and width, hop, n_fft with the meaning they have in
 * hftt_clip_logmel; sr, the sample rate; lead >= 0, further frames rendered in front of each window (below); and the VOICE BANK, V voices of H
 * partials, 1 <= H <= HFTT_SYNTH_MAX_PARTIALS, all tables built on the host and in device memory:
 *     inc       uint32 [V, N, H]  phase increment of a partial in turns per sample, Q32 (frequency / sr * 2^32)
 *     amp       fp32   [V, N, H]  0 switches a partial off (the host zeroes partials at or above Nyquist)
 *     dec       fp32   [V, N, H]  >= 0: decay in log2 units per sample
 *     vel_gain  fp32   [V, 128]   the velocity curve
 *     rel       fp32   [V]        >= 0: additional decay per sample behind the note's offset
 *     attack    int32  [V]        samples, >= 1          release  int32 [V]  samples, >= 0: how long a note sounds behind its offset
 *     voice_index int32 [B]: window b's voice; outside 0 .. V - 1: a window without a file
 * attack < 1, release < 0 and a velocity outside 0 .. 127 cannot be refused by the host: the kernel clamps them (to 1, to 0, into 0 .. 127).
 * The kernel is a generic modal synthesizer; the instrument lives in the host function that fills the bank (corpus/synth_audio.py).
 *
 * The sample.  A record of pitch index p in file f has n_on = (int64)(onset_sec * sr + 0.5), n_off = (int64)(offset_sec * sr + 0.5) (fp64,
 * the product and the sum rounded separately) and D = max(n_off - n_on, 1).  Under voice v it sounds at file sample i when
 * 0 <= tau = i - n_on < D + release[v], and there its partial h contributes c * S(u) with, every operation in fp32 and rounded once:
 *     u   = (float)(int32)(inc[v,p,h] * (uint32)tau) * 2^-32            the product wraps: the phase is exact at any tau; u in [-0.5, 0.5]
 *     tf  = (float)tau,  rf = (float)max(0, tau - D)                    (exact below 2^24)
 *     x   = min(dec[v,p,h] * tf + rel[v] * rf, 126)                     two products, one sum
 *     ra  = (float)min(tau + 1, attack[v]) / (float)attack[v]           IEEE division
 *     c   = ((amp[v,p,h] * vel_gain[v, velocity]) * ra) * E(-x)
 * S(u) = sin(2 pi u) is the hardware's v_sin_f32, which takes its argument in turns; E(y) = 2^y is v_exp_f32, whose argument the clamp keeps
 * inside [-126, 0] (no denormal result).  Both are defined once in csrc/clip_synth_fn.h; their errors against fp64 as measured on an MI355X
 * are in profiles/clip_synth_mi355x.txt.  The sample of file f under voice v at i, 0 <= i < n', is
 *     acc = +0;  acc = fma(c, S(u), acc)  over the file's records in TABLE order -- pitch group after pitch group, list order inside a
 *     group -- and inside a record over h = 0 .. H - 1; a record that does not sound at i contributes no operation
 * so a sample where nothing sounds is +0.0f.  The value depends on (f, v, i) only -- not on win_start, on lead, on where a workgroup's tile
 * begins or on the launch geometry: S and E are evaluated per sample, there is no recurrence.  Two overlapping windows with equal voices see
 * the same waveform, bit for bit and from run to run.
 *
 * Outputs: the room's convention.  out fp32 [B, span], span >= (P + lead + width - 1) * hop + n_fft / 2 with P = ceil((n_fft / 2) / hop);
 * out_samp0 int64 [2 B + 1], out_win_file / out_win_start int32 [B].  Row b holds pseudo-file 2 b = samples [o_b, e_b) of the synthetic file,
 *     o_b = max(0, win_start[b] - P - lead) * hop,   e_b = min(n', (win_start[b] + width - 1) * hop + n_fft / 2)     (empty when e_b <= o_b)
 * and pseudo-file 2 b + 1, the unused remainder of the row (not written); out_samp0[2 b] = b * span, out_win_file[b] = 2 b,
 * out_win_start[b] = win_start[b] - o_b / hop.  A window without a valid file, with voice_index[b] outside 0 .. V - 1 or with o_b > n' gets
 * out_win_file[b] = -1.  With lead = 0 these are the tables hftt_clip_room writes, and a plain hftt_clip_logmel over `out` (wave_i16 = 0, n_files =
 * 2 B, total_samples = B * span) gives, bit for bit and in the fill columns too, the log-mel of the whole synthetic file (the room's argument).
 * lead exists so that a room can follow: with lead >= ceil(taps / hop), hftt_clip_room run over this scratch corpus as ITS corpus (win_file =
 * out_win_file, win_start = out_win_start) has the full history of every wet sample the clip shows.
 *
 * One launch: a workgroup owns a window and a tile of 2,048 consecutive samples.  It scans the file's records, which are contiguous (row_ptr[f N]
 * .. row_ptr[(f + 1) N]), HFTT_SYNTH_CHUNK at a time, keeps those whose sounding range meets the tile in LDS in table order (prefix sum; the
 * pitch of a record from the file's N + 1 row pointers staged in LDS), and every thread walks the survivors with eight samples in registers; the
 * bank rows are uniform over the workgroup and are read on the scalar unit.  More sounding records than a chunk holds are further passes.
 * One writer per element, no atomics, no workspace, 64-bit sample indices.
 * Refused in front of the launch: null pointers (notes excepted at n_notes == 0); n_fft != 2048; B, width, hop, n_files or V < 1; n_notes
 * < 0; N outside 1 .. 128; H outside 1 .. HFTT_SYNTH_MAX_PARTIALS; a bank of 2^31 entries (V N H) or more; lead < 0; sr <= 0 (or
 * not finite); span below the bound above; B above 2^30, or 2^31 workgroups and more.
 * --------------------------------------------------------------------------------------------- */
#define HFTT_SYNTH_MAX_PARTIALS 32
#define HFTT_SYNTH_CHUNK 256
typedef struct {
  const hftt_label_note* notes;                                  /* [n_notes] (may be NULL when n_notes == 0) */
  const int32_t* row_ptr;                                        /* [n_files * N + 1] */
  const int64_t* file_nsamp;                                     /* [n_files] */
  const int32_t* win_file; const int32_t* win_start;             /* [B] */
  int32_t n_files, n_notes;
  int32_t B, width, N;
  int32_t n_fft, hop, lead;
  double sr;
  int32_t V, H;
  const uint32_t* inc;                                           /* [V, N, H] */
  const float* amp; const float* dec;                            /* [V, N, H] */
  const float* vel_gain;                                         /* [V, 128] */
  const float* rel;                                              /* [V] */
  const int32_t* attack; const int32_t* release;                 /* [V] */
  const int32_t* voice_index;                                    /* [B] */
  int64_t span;
  void* out;                                                     /* fp32 [B, span] */
  int64_t* out_samp0;                                            /* [2 B + 1] */
  int32_t* out_win_file; int32_t* out_win_start;                 /* [B] */
} hftt_clip_synth_desc;
int hftt_clip_synth(const hftt_clip_synth_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Clip synth, played (csrc/clip_synth_parts.hip): hftt_clip_synth under a per-window PERFORMANCE -- transposition, a time map (tempo and
 * delay), a tuning offset -- and with a SECOND PART, another file's notes under its own voice and its own performance, summed onto the first:
 * every key, tempo, tuning and pairing of a note corpus at no resident cost.  The label side is hftt_labels_render_warp / _mix, which take the
 * same per-window shift, t_delay, t_scale and partner tables.  One entry point ADDED at ABI 8; HFTT_ABI_VERSION stays 8, every descriptor
 * above keeps its layout, and hftt_clip_synth (its file, its kernel, its results) is untouched: the kernel here is a second copy of its walk,
 * held to it by the identity equality below.
 *
 * It is the hftt_clip_synth contract -- `base` with every field as there, except that base.file_nsamp is NOT read (it may be NULL) -- with
 * nsamp int64 [B], the length n'_A of window b's synthetic file under its map (negative: 0), and four changes per part.  A part's play is an
 * hftt_synth_play_args: shift / t_delay / t_scale [B], all three set or all three NULL (the rule of hftt_labels_render_mix; NULL: 0, 0, 1),
 * and tune_q31 uint32 [B] or NULL (NULL: 2^31).
 *   Time map.  Every note time t of the part becomes t' = fmul(fadd(t, t_delay[b]), t_scale[b]) -- fp64, two roundings, never an fma: the
 *     expression of hftt_labels_render_warp, so audio and labels are formed from the same bits of t' -- and then n_on = (int64)(t'_on * sr +
 *     0.5), n_off likewise, D = max(n_off - n_on, 1).  t_delay = 0, t_scale = 1 gives the unmapped bits.  Decay rates, attack and release stay
 *     per sample: a string does not know the tempo.
 *   Transposition.  A record of table pitch p sounds with bank row p + shift[b]; a row outside 0 .. N - 1 contributes no operation (the labels
 *     give an all-zero column there).
 *   Tuning.  inc' = (uint32)(((uint64)inc[v, p + shift, h] * tune_q31[b]) >> 31): exact integer arithmetic, 2^31 = unison leaves inc
 *     unchanged; the phase is u = (float)(int32)(inc' * (uint32)tau) * 2^-32 as before.  The product is NOT checked against Nyquist: the
 *     host leaves the headroom when it fills the bank.
 *   The second part.  part_file / part_start / part_voice int32 [B] and part_gain fp32 [B], all four set or all four NULL, with part_nsamp
 *     int64 [B] (n'_B, the partner file's length under ITS map; given exactly when the partner tables are) and part_play.  The sample at
 *     primary position i, 0 <= i < n'_A, is acc = +0, then the primary's records in table order exactly as in hftt_clip_synth, and then,
 *     CARRYING THE SAME ACCUMULATOR, the partner's records in table order at partner position iB = i + (part_start[b] - win_start[b]) * hop
 *     (int64): a partner record sounds when 0 <= iB < n'_B and 0 <= tau_B = iB - n_on_B < D_B + release[vB], with
 *         c = (((amp * vel_gain[vB, velocity]) * part_gain[b]) * ra) * E(-x)
 *     -- one further rounding, formed once per (record, partial) -- and everything of the voice (vel_gain, rel, attack, release, the bank
 *     rows) the partner's vB = part_voice[b].  A part_file outside 0 .. n_files - 1 or a part_voice outside 0 .. V - 1 contributes nothing:
 *     such a window is bit-identical to one without partner tables.  Outside [0, n'_A) nothing is rendered: the partner is added ONTO the
 *     primary's extent, as in hftt_clip_logmel_mix.
 * Pseudo-files, the three output tables, lead, span, invalid windows and the never-written remainder of a row are hftt_clip_synth's with
 * n' = nsamp[b].  The value depends on (files, voices, plays, gain, part_start - win_start, i) only -- not on tile origin, lead or geometry:
 * overlapping windows with equal draws see the same bits.  With every group NULL, or with identity values (shift 0, t_delay 0, t_scale 1,
 * tune 2^31, part_file -1) and nsamp[b] = file_nsamp[win_file[b]], all four outputs equal hftt_clip_synth's bit for bit.
 *
 * One launch of hftt_clip_synth's shape (a workgroup per window and tile of 2,048 samples, eight samples per thread): one device function
 * filters a part's records against the tile -- for the partner the tile in partner coordinates, cut to [0, n'_B) -- and walks the survivors;
 * it runs for the primary and, under a branch uniform over the workgroup, for the partner on the same registers, re-using the survivor list
 * and re-staging the partner file's row pointers.  The tuning product is scalar arithmetic.  One writer per element, no atomics, no workspace.
 * Refused in front of the launch: everything hftt_clip_synth refuses except a null base.file_nsamp; null nsamp; a play or part_play map of
 * which only a part is given; partner tables of which only a part is given; part_nsamp or part_play given without partner tables; part_nsamp
 * missing with partner tables.
 * --------------------------------------------------------------------------------------------- */
typedef struct {                                                 /* how one part is played; [B] each */
  const int32_t* shift;                                          /* semitones           } all three set, or all three NULL */
  const double*  t_delay;                                        /* seconds             }   (the rule of hftt_labels_render_mix) */
  const double*  t_scale;                                        /*                     } */
  const uint32_t* tune_q31;                                      /* or NULL: 2^31 = unison */
} hftt_synth_play_args;
typedef struct {
  hftt_clip_synth_desc base;                                     /* everything as in hftt_clip_synth; base.file_nsamp is NOT read */
  const int64_t* nsamp;                                          /* [B] n'_A: length of window b's synthetic file under its map (negative: 0) */
  hftt_synth_play_args play;                                     /* the primaries' */
  const int32_t* part_file; const int32_t* part_start; const int32_t* part_voice;        /* [B], all four set or all four NULL */
  const float*   part_gain;
  const int64_t* part_nsamp;                                     /* [B] n'_B; given exactly when the partner tables are */
  hftt_synth_play_args part_play;                                /* the partners' */
} hftt_clip_synth_parts_desc;
int hftt_clip_synth_parts(const hftt_clip_synth_parts_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Guarded optimizer step (csrc/guard.hip): global-norm gradient clipping, a non-finite guard and decoupled weight decay around the fused
 * Adam.  Like the note decoder and the label renderer these entry points were ADDED at ABI 8 and HFTT_ABI_VERSION stays 8: nothing that an
 * ABI-8 caller binds changed (hftt_adam_step above is untouched and remains the default step); a caller that needs them looks the symbols up.
 *
 * The record: 32 bytes of DEVICE memory, 16-byte aligned, zeroed once by the caller.  The norm kernels write it, the Adam kernel reads it,
 * the host never has to: a training loop that only wants the step guarded does not synchronise.
 *
 * Norm (torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=2): total_norm = || g ||_2 over ALL parameters,
 * clip_coef = max_norm / (total_norm + 1e-6), clamped to 1) over the flat gradient, with grad_scale folded in (the 1 / world of the
 * all-reduced sum: the norm is that of the gradient Adam will see).  Two launches, no atomics: 256-thread workgroups (at most 2048, the grid
 * of the Adam kernels) read g once with 16-byte loads (scalar tail for n % 4), every lane sums g * g in fp64, lanes then waves are combined in
 * a fixed order into one fp64 partial per workgroup in ws; one workgroup then sums the partials in a fixed order and one lane stores
 *     norm64 = |grad_scale| * sqrt(sum)                                   (double)
 *     apply  = isfinite(norm64)
 *     coef   = apply ? (float)min(1.0, max_norm / (norm64 + 1e-6)) : 0    (formed in double, rounded once)
 *     skipped += !apply;  clipped += apply && coef < 1
 * fp64 on purpose: |g| = 1e30 does not overflow and |g| = 1e-30 does not vanish, so "the norm is not finite" is the same statement as
 * "some element is Inf or NaN" (squares cannot cancel).  max_norm = +inf switches clipping off (coef is exactly 1).  The record is bitwise
 * reproducible from run to run.  ws: hftt_grad_norm_ws_bytes(n) bytes, 16-byte aligned, contents irrelevant on entry.
 * Refused in front of the launch: null operands; n <= 0; g, ws or ctl not 16-byte aligned; grad_scale not finite; max_norm NaN or <= 0.
 *
 * Step: hftt_adam_step's update, one launch, read through the record.  apply == 0: the kernel returns without a store -- p, m, v keep their
 * bits.  Otherwise per element
 *     gr = g * ((float)grad_scale * coef)
 *     p *= d,  d = (float)(1 - lr * weight_decay)        (torch.optim.AdamW: param.mul_(1 - lr * weight_decay), the decay first)
 *     m = b1*m + (1-b1)*gr; v = b2*v + (1-b2)*gr*gr; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * with 1 - b, the bias corrections and d formed in double on the host and rounded once.  g is NOT rewritten: the clip factor lives in the
 * kernel (clip_grad_norm_ scales the gradients in place).  With coef == 1 and weight_decay == 0 the result is bit-identical to
 * hftt_adam_step.  `step` is the number of CALLS, as for hftt_adam_step: a skipped step still advances it, so the caller's step counter
 * and checkpoints keep their meaning.  torch.amp.GradScaler differs: it does not count the steps it skips.  The effect here is a slightly
 * smaller bias correction during the first few hundred steps after a skip.
 * Refused in front of the launch: what hftt_adam_step refuses; ctl null or not 16-byte aligned; weight_decay NaN or negative;
 * lr * weight_decay >= 1.
 * --------------------------------------------------------------------------------------------- */
typedef struct {            /* 32 bytes of DEVICE memory, 16-byte aligned, zeroed once by the caller */
  float    norm;            /* || grad_scale * g ||_2 of the last call, fp32 rounding of the fp64 value (may be inf / nan) */
  float    coef;            /* factor applied on top of grad_scale: min(1, max_norm / (norm + 1e-6)); 1 when clipping is off */
  uint32_t apply;           /* 1: the step is applied; 0: the norm was not finite, the step is skipped */
  uint32_t skipped;         /* cumulative count of skipped steps */
  uint32_t clipped;         /* cumulative count of applied steps with coef < 1 */
  uint32_t pad[3];
} hftt_guard_ctl;
int64_t hftt_grad_norm_ws_bytes(int64_t n);
int hftt_grad_norm(const float* g, int64_t n, double grad_scale, double max_norm,
                   void* ws, hftt_guard_ctl* ctl, void* stream);
int hftt_adam_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, int32_t step,
                           double lr, double beta1, double beta2, double eps, double grad_scale,
                           double weight_decay, const hftt_guard_ctl* ctl, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Parameter groups for the guarded step (csrc/guard.hip): per-group learning rate and decoupled decay, and frozen groups, in ONE launch over
 * the flat buffer (fine-tuning: a frozen encoder, no decay on biases and LayerNorm parameters).  ADDED at ABI 8 like the section above;
 * HFTT_ABI_VERSION stays 8 and hftt_adam_step / hftt_grad_norm / hftt_adam_step_guarded are untouched.
 *
 * The group map: one uint8 per QUAD (4 consecutive fp32 elements) of the flat buffer, in device memory: the index of the quad's group,
 * n / 4 entries.  Parameter offsets in the flat buffer are multiples of 8 elements, so a quad never straddles two parameters; a quad in the
 * alignment gap behind a parameter takes that parameter's group (its p, g, m, v are zero and stay zero).  Values >= n_groups are the
 * caller's error.
 *
 * hftt_adam_step_groups: hftt_adam_step_guarded's update per quad with the constants of the quad's group,
 *     lr_c[k] = (float)(lr[k] / (1 - b1^t)),   d[k] = (float)(1 - lr[k] * weight_decay[k])        (formed in double, rounded once)
 * through the record `ctl` (apply == 0: nothing is stored; gr = g * ((float)grad_scale * coef)).  ctl == NULL: unguarded -- always applied,
 * clip factor 1.  A quad whose group has frozen[k] != 0 is neither loaded nor stored: p, m, v keep their bits and the step's traffic drops
 * with the frozen share.  With one group and nothing frozen the result is bit-identical to hftt_adam_step_guarded (and hence, with clip
 * factor 1 and no decay, to hftt_adam_step).  Same grid rule as the guarded kernel.
 * Refused in front of the launch: what hftt_adam_step_guarded refuses, per group (weight_decay NaN or negative, lr * weight_decay >= 1);
 * n % 4 != 0; n_groups outside 1..HFTT_ADAM_MAX_GROUPS; a null map; ctl given but not 16-byte aligned.
 *
 * hftt_grad_norm_groups: hftt_grad_norm with the quads of the groups in frozen_mask (bit k: group k) left out of the sum -- the norm of
 * torch.nn.utils.clip_grad_norm_ over the parameters that HAVE a gradient.  Same two launches, same fixed orders, same record; with
 * frozen_mask == 0 the record equals hftt_grad_norm's bit for bit.  Consequence: an Inf or NaN in a frozen range does not skip the step.
 * Refused in front of the launch: what hftt_grad_norm refuses; n % 4 != 0; a null map; a frozen_mask bit beyond HFTT_ADAM_MAX_GROUPS.
 * --------------------------------------------------------------------------------------------- */
#define HFTT_ADAM_MAX_GROUPS 8
typedef struct {
  float* p; const float* g; float* m; float* v;      /* flat parameters, gradients, first and second moments: n fp32 each, 16-byte aligned */
  int64_t n;                                          /* elements, a multiple of 4 */
  const uint8_t* quad_group;                          /* [n / 4] device bytes: group index of every quad */
  int32_t n_groups;                                   /* 1..HFTT_ADAM_MAX_GROUPS */
  int32_t step;                                       /* number of calls so far, >= 1 (bias corrections) */
  double beta1, beta2, eps, grad_scale;               /* shared by all groups */
  double lr[HFTT_ADAM_MAX_GROUPS];
  double weight_decay[HFTT_ADAM_MAX_GROUPS];          /* decoupled */
  int32_t frozen[HFTT_ADAM_MAX_GROUPS];               /* != 0: the group's quads are neither loaded nor stored */
  const hftt_guard_ctl* ctl;                          /* the guard record; NULL: unguarded */
} hftt_adam_groups_desc;
int hftt_adam_step_groups(const hftt_adam_groups_desc* d, void* stream);
int hftt_grad_norm_groups(const float* g, int64_t n, const uint8_t* quad_group, uint32_t frozen_mask, double grad_scale, double max_norm,
                          void* ws, hftt_guard_ctl* ctl, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Averaged weights inside the Adam step (csrc/guard.hip): the exponential moving average (EMA) of the parameters,
 * torch.optim.swa_utils.get_ema_multi_avg_fn(beta): e = beta * e + (1 - beta) * p on the parameters AFTER the step, in the launch that
 * already visits every element.  ADDED at ABI 8 like the two sections above; HFTT_ABI_VERSION stays 8 and hftt_adam_step,
 * hftt_adam_step_guarded and hftt_adam_step_groups are untouched.
 *
 * hftt_adam_step_ema: ONE launch.  Per quad hftt_adam_step_groups' update, unchanged (the same constants formed the same way on the host,
 * the same reading of `ctl`, the same frozen-quad skip, the same grid rule), then on the new p still in registers, contraction off,
 *     y = omd * (p - e) - c;   t = e + y;   c = (t - e) - y;   e = t;          omd = (float)(1 - ema_decay)   (formed in double, rounded once)
 * with e = ema[i] and c = ema_c[i], both loaded and stored with 16-byte accesses (44 B of traffic per element against 28).  c is the running
 * compensation (Kahan): the plain fp32 form e += omd (p - e) stops moving once omd |p - e| < ulp(e) / 2 -- with beta = 0.9999 that is
 * |p - e| < 6e-4 |e|, weights that jitter round a mean at the end of a decayed schedule -- while the compensated sum follows the fp64
 * recurrence to a few ulp over thousands of calls.  ema_decay is the beta of THIS call, so a warm-up schedule costs nothing.
 * Consequences:
 *   - p, m, v after the call are bit-identical to the non-EMA entry point of the same configuration: hftt_adam_step (one group, no decay,
 *     ctl NULL), hftt_adam_step_guarded (one group, ctl given), hftt_adam_step_groups.
 *   - apply == 0: nothing is stored, ema and ema_c included.
 *   - a frozen quad's ema and ema_c are neither loaded nor stored.
 * a.quad_group may be NULL when a.n_groups == 1 and a.frozen[0] == 0 (one group over the whole buffer needs no map).
 * Refused in front of the launch: what hftt_adam_step_groups refuses (but for that null map); a null descriptor; ema or ema_c null or not
 * 16-byte aligned; ema or ema_c overlapping p, g, m, v or each other; ema_decay NaN, negative or >= 1; n % 4 != 0.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  hftt_adam_groups_desc a;   /* as hftt_adam_step_groups; a.quad_group may be NULL when a.n_groups == 1 and a.frozen[0] == 0 */
  float* ema;                /* [n] the average, 16-byte aligned */
  float* ema_c;              /* [n] its running compensation, 16-byte aligned */
  double ema_decay;          /* beta of THIS call, 0 <= beta < 1; omd = (float)(1 - beta), formed in double, rounded once */
} hftt_adam_ema_desc;
int hftt_adam_step_ema(const hftt_adam_ema_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Class-balanced and focal criteria inside the fused loss (csrc/loss_w.hip; training/train.py:141-153 with the criteria exchanged):
 * hftt_loss's pass with a per-pitch positive weight and a focal modulation on the six BCE heads, and class weights, ignore_index and label
 * smoothing on the two velocity cross-entropies.  Two entry points ADDED at ABI 8; HFTT_ABI_VERSION stays 8, hftt_loss_desc keeps its
 * layout and hftt_loss is untouched.
 *
 * BCE head h (the order of prob[6]), element i, pitch j = i mod Nn, posterior p, target y in [0, 1], a = pos_weight[h][j] > 0 (NULL: 1),
 * g = gamma[h] (0, or in [1, 4]):
 *     lp = max(log p, -100), l1p = max(log1p(-p), -100)                  (hftt_loss's clamps)
 *     base = -(a y lp + (1 - y) l1p)          a weighs the positive part only: BCEWithLogitsLoss(pos_weight=)'s definition
 *     m = |y - p|^g                           the soft-label focal factor (quality focal loss; g = 0: m = 1 exactly, no pow evaluated)
 *     term_h = (1 / n) sum_i m base
 *     d term_h / d p = m ((p - y) - (a - 1) y (1 - p)) / max((1 - p) p, 1e-12) - base g |y - p|^(g - 1) sign(y - p)        (sign(0) = 0)
 * d_prob[h] carries weight_A|B * grad_scale / n as in hftt_loss.
 *
 * Velocity side s: logits z[i, :V], label c_i, w = class_weight[s] >= 0 (NULL: 1), e = smoothing[s] in [0, 1), k = ignore_index[s];
 * q = softmax(z_i), ok_i = (c_i != k), W_s = sum_ok w[c_i]:
 *     term_s = [ (1 - e) sum_ok w[c_i] (-log q[c_i]) + (e / V) sum_ok sum_c w[c] (-log q[c]) ] / W_s
 *     d term_s / d z[i, c] = ok_i [ (1 - e) w[c_i] (q[c] - [c == c_i]) + (e / V) (q[c] sum_k w[k] - w[c]) ] / W_s
 * which is torch.nn.functional.cross_entropy(weight=, ignore_index=, label_smoothing=, reduction='mean').  ONE deliberate deviation: when
 * W_s == 0 (every row ignored or of weight zero) torch returns NaN; here the term and its gradient are 0, so that no NaN runs through the
 * backward into an unguarded Adam.  A label outside [0, V) that is not k is the caller's error, as in hftt_loss (it is never used as an
 * index).
 *
 * loss_out[0..8] as hftt_loss (the CE terms divided by W_s), loss_out[9] = W_A, loss_out[10] = W_B: loss_out holds ELEVEN floats.
 * Launches: a label pre-pass that sums W_s in a fixed order (no float atomics: two runs are bit-identical), the main pass, the reduce.  The
 * pre-pass is left out (W_s = n, two launches) when no side has class weights or an ignore_index inside [0, V).  The two forms of the main
 * pass are hftt_loss's, chosen by its predicate (each compiled with and without the class-weight registers: a call without class weights
 * and smoothing keeps hftt_loss's register budget).
 * Neutrality, bit for bit: a head with pos_weight NULL or all ones and gamma 0 produces hftt_loss's bits in loss_out and d_prob[h]; a side
 * with class_weight NULL, smoothing 0 and an ignore_index outside [0, V) produces hftt_loss's bits in loss_out and d_vel[s] -- whatever the
 * other heads and sides of the same call are given.
 * Refused in front of the launch: a null descriptor; what hftt_loss refuses; Nn <= 0; n % Nn != 0; a gamma that is neither 0 nor in [1, 4];
 * a smoothing outside [0, 1); ws_w NULL when the pre-pass is needed.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  hftt_loss_desc base;             /* as hftt_loss, but loss_out is [11] */
  int32_t Nn; int32_t pad;         /* pitches: the period of the pos_weight tables, n % Nn == 0 */
  const float* pos_weight[6];      /* device [Nn] per head, NULL: 1 */
  float gamma[6];                  /* focal exponent per head: 0, or in [1, 4] */
  const float* class_weight[2];    /* device [V] per side, NULL: 1 */
  float smoothing[2];              /* label smoothing per side, in [0, 1) */
  int64_t ignore_index[2];         /* per side; outside [0, V): nothing is ignored (torch's default is -100) */
  float* ws_w;                     /* hftt_loss_w_ws_bytes(n): the pre-pass partials; may be NULL when no pre-pass is needed */
} hftt_loss_w_desc;
int64_t hftt_loss_w_ws_bytes(int64_t n);
int hftt_loss_w(const hftt_loss_w_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Streaming resampler (csrc/resample_stream.hip): hftt_resample with its state carried forward, S streams in ONE launch -- the front end of
 * audio that arrives in pieces at any rate.  One entry point ADDED at ABI 8; HFTT_ABI_VERSION stays 8 and hftt_resample keeps its descriptor
 * and its results.
 *
 * The FIR has finite support: with up, down, width, taps of the kernel table above, output o reads input samples
 * [(o / up) * down - width, + taps) and nothing else, summed in an order that depends on o % up alone.  So output o is final once input sample
 * (o / up) * down + width + down - 1 has arrived, and a kernel that stages the same window from a carried tail produces the bits of the
 * whole-file kernel.  Adopted as the definition: after n_in samples a live stream owns its first up * max(0, (n_in - width) / down) outputs
 * (capped at ceil(n_in * up / down)), a closing stream all ceil(n_in * up / down); the added latency is (width + down) / sr_in.  The host
 * keeps the counters (they are a function of what was pushed: nothing is read back) and, per stream, the input samples from
 * (next_output / up) * down - width on -- fewer than taps + down of them.
 *
 * Per call the host packs every stream's [carried tail | new samples] into `wave` (fp32, or int16 when wave_i16: converted while it is staged as
 * (float)s * (1.0f / 32768.0f)) and uploads ONE table, tab: DEVICE int64 [HFTT_RESAMPLE_STREAM_ROWS, S], row-major, per stream
 *   row 0 in_off     where the stream's packed input begins inside `wave`
 *   row 1 in_first   the absolute index, in the stream's own timeline, of its first packed sample
 *   row 2 in_end     the absolute index one past the last sample present
 *   row 3 closing    != 0: the stream ends with this call
 *   row 4 out_first  the first output to produce            row 5 count   how many (0: nothing to do, the workgroups return at once)
 *   row 6 out_pos    where inside `store` output out_first goes: outputs lie at out_pos .. out_pos + count
 *   row 7 fill       closing only: that many zeros are written behind the last output -- up to the last sample the file's final log-mel frame
 *                    reads, so that a kernel reading the slot sees the zeros the whole-file kernel takes from its bounds test
 * Samples in front of absolute index 0 and at or beyond in_end are zeros; for a stream that is not closing the host never asks for an output
 * whose window reaches in_end.  Grid (max(1, ceil(max_count / 256)), S); max_count = the largest count of the table, as the host knows it.
 * Indices derived from the table are held inside [0, wave_len) and [0, store_len): a wrong table cannot leave the two buffers.
 * Refused in front of the launch, each with its own text: a null descriptor or operand; S outside 1..65535; up or down <= 0; taps != 2 * width
 * + down; max_count < 0; wave_i16 outside 0..1; negative wave_len / store_len; an LDS window of 256 outputs, ((255 / up + 1) * down + taps) * 4
 * bytes, beyond 64 KB (hftt_resample's expression).
 * --------------------------------------------------------------------------------------------- */
#define HFTT_RESAMPLE_STREAM_ROWS 8
typedef struct {
  const void* wave; int64_t wave_len;        /* packed input of all streams, fp32 or int16; its samples */
  const float* kernel;                   /* [up, taps] */
  const int64_t* tab;                    /* DEVICE int64 [HFTT_RESAMPLE_STREAM_ROWS, S] */
  float* store; int64_t store_len;       /* the resampled store (all slots); its samples */
  int64_t max_count;
  int32_t S, up, down, width, taps, wave_i16;
} hftt_resample_stream_desc;
int hftt_resample_stream(const hftt_resample_stream_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HFTT_HIP_H */
