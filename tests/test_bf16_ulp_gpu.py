"""The bf16 mode's forward kernels at the ulp: each bf16 output against its kernel's own fp64 rounding model (tests/bf16_emul.py), on inputs
that are exact in bf16.  The older tests of these kernels hold them to 6e-3 .. 3e-2 of the output's maximum, many bf16 ulps: a kernel that
truncated instead of rounding to nearest even, rounded an intermediate twice, or rounded P at another point would pass them.

Criterion (bf16_emul.excess / ulp_stats; calibrated on CPU by test_bf16_emul_bound.py, where the same models summed in fp32 must pass it):
  * a fraction >= IDENT of the elements bit-identical to rne(model64);
  * no element further from rne(model64) than one bf16 ulp plus EXCESS units of 2^-24 times the magnitude of its terms (a result that cancels
    carries the fp32 summation error of its terms; the attention output and the fused FFN's fc_2 also carry the rounding of a bf16 operand
    made in the kernel, P or the hidden, at near-ties, which fp32 and fp64 resolve differently);
  * fp32 row statistics within a few fp32 ulps of fp64."""
import math

import pytest
import torch
import torch.nn.functional as F

import bf16_emul as E
from util import keep_scale, keep_mask_t

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _ops():
    from hftt_hip import ops
    return ops


def _check(name, dev_out, ref, absref, ident=E.IDENT_STREAM, excess=None, row_ident=E.ROW_IDENT_STREAM):
    exc = E.excess(dev_out, ref, absref)
    _, frac = E.ulp_stats(dev_out, ref)
    row = E.row_ident_min(dev_out, ref)
    print('%-44s identical %.5f  worst row %.4f  excess %.1f' % (name, frac, row, exc))
    assert frac >= ident, (name, frac)
    assert row >= row_ident, (name, row)
    if excess is not None:
        assert exc <= excess, (name, exc)
    return frac


# ---------------------------------------------------------------------------------------------------------------------------- attention
FWD8_SHAPES = [(3, 4, 256, 256), (3, 4, 129, 129), (3, 4, 200, 256), (3, 4, 256, 130), (3, 4, 255, 255), (2, 4, 160, 200)]
DEC_SHAPES = [(3, 4, 88, 256, 64), (3, 4, 128, 128, 64), (3, 2, 88, 256, 32)]


def _attn_inputs(n, H, Lq, Lk, dh):
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    d = H * dh
    q = (torch.randn(n, Lq, d, generator=g) * 0.5).to(BF)     # logits of std ~0.5: P spread over the row, every element's rounding counts
    return q, torch.randn(n, Lk, d, generator=g).to(BF), torch.randn(n, Lk, d, generator=g).to(BF)


def _attn_case(dev, n, H, Lq, Lk, dh, p, want_probs):
    from hftt_hip.engine import attn_fwd8_takes
    ops = _ops()
    q, k, v = _attn_inputs(n, H, Lq, Lk, dh)
    site, seed = 5, 777
    mask = keep_mask_t(seed, site, (n, H, Lq, Lk), p) if p > 0 else None
    res = ops.attn_fwd(q.to(dev), k.to(dev), v.to(dev), H, npass=1, want_probs=want_probs, drop_p=p, drop_site=site, drop_seed=seed, out_dtype=BF)
    out, lse = res[0].cpu(), res[1].cpu()
    form = 'fwd8' if attn_fwd8_takes(1, True, dh, Lq, Lk, want_probs) else 'fwd'
    o64, mx64, inv64, ab = E.attention(q, k, v, H, form, mask, keep_scale(p), want_abs=True)
    tag = '%s %s p=%.1f%s' % (form, (n, H, Lq, Lk, dh), p, ' map' if want_probs else '')
    _check(tag, out, o64, ab, ident=E.IDENT_ATTN, excess=E.EXCESS_ROUNDED, row_ident=E.ROW_IDENT_ROUNDED)
    emx, einv = E.fp32_ulps(lse[..., 0], mx64), E.fp32_ulps(lse[..., 1], inv64)
    print('%-44s lse max %.1f ulp  1/sum %.1f ulp' % (tag, emx, einv))
    assert emx <= E.LSE_MAX_ULPS and einv <= E.LSE_INV_ULPS, (emx, einv)
    other = E.attention(q, k, v, H, 'fwd' if form == 'fwd8' else 'fwd8', mask, keep_scale(p))[0]
    _, f_other = E.ulp_stats(out, other)
    print('%-44s identical to the other form\'s model %.5f' % (tag, f_other))
    assert f_other < E.IDENT_OTHER_FORM, 'the output matches the other attention forward\'s rounding of P: %.4f' % f_other
    return form


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('n,H,Lq,Lk', FWD8_SHAPES)
def test_attn_fwd8_at_the_ulp(dev, n, H, Lq, Lk, p):
    """attn_fwd8_kernel (no attention map, 128 < Lq, Lk <= 256): idle waves and clamped query rows (Lq % 32), -inf key padding (Lk < 256),
    the per-element dropout form (Lk % 4), and its (raw max, 1/sum) pair.  The output must meet the fwd8 model (P rounded before 1/sum) and
    not attn_fwd_kernel's (P rounded after): at these shapes the two models share about half their bits (CPU calibration)."""
    assert _attn_case(dev, n, H, Lq, Lk, 64, p, want_probs=False) == 'fwd8'


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('n,H,Lq,Lk,dh', [s + (64,) for s in FWD8_SHAPES] + DEC_SHAPES)
def test_attn_fwd_kernel_at_the_ulp(dev, n, H, Lq, Lk, dh, p):
    """attn_fwd_kernel<KT, dh, 1, true>: the same shapes through want_probs=True, and the decoder's shapes (88 x 256, 128 x 128, dh 32)"""
    assert _attn_case(dev, n, H, Lq, Lk, dh, p, want_probs=True) == 'fwd'


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('n,H,Lq,Lk,dh', DEC_SHAPES)
def test_attn_fwd_kernel_without_map_at_the_ulp(dev, n, H, Lq, Lk, dh, p):
    """attn_fwd_kernel with probs == nullptr (the decoder's attentions when no map is wanted): normalisation and dropout in ONE fp32 multiply
    by inv * keep_scale (attn_fwd.hip, `nrm`), or `*= inv` without dropout, before P is rounded"""
    assert _attn_case(dev, n, H, Lq, Lk, dh, p, want_probs=False) == 'fwd'


# ---------------------------------------------------------------------------------------------------------------------------- the stream
PAPER_M = 2 * 128 * 256          # tokens of one encoder launch at paper size, B = 2 (n_frame x n_bin per clip)


def _b(t):
    return t.to(BF).double()


def _ln64(r, gam, bet, absr):
    """LayerNorm in fp64 and the magnitude of its terms: rstd |gamma| (|r| + |mean| + absr) + |beta|"""
    mu = r.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(r.var(1, unbiased=False, keepdim=True) + 1e-5)
    y = (r - mu) * rstd * gam.double() + bet.double()
    return y, rstd * gam.double().abs() * (r.abs() + mu.abs() + absr) + bet.double().abs()


@pytest.mark.parametrize('M,N,K', [(1000, 256, 256), (700, 768, 256), (515, 256, 512), (300, 256, 768), (257, 192, 96), (4096, 512, 256),
                                   (515, 512, 512), (300, 768, 768)])     # N, K > 256: the BM = 32 form, two / three N tiles, a ragged last block
def test_gemm_nt_bf16_at_the_ulp(dev, M, N, K):
    """dispatch_nt_bf16: bf16 A, bf16 C, with bias + ReLU and (where the A-stationary path takes it) with a bf16 residual"""
    ops = _ops()
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(BF); W = torch.randn(N, K, generator=g) / math.sqrt(K); b = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(BF)
    lin = _b(A) @ _b(W).T + b.double()
    ab = _b(A).abs() @ _b(W).abs().T + b.double().abs()
    out = ops.gemm_nt(A.to(dev), W.to(dev), b.to(dev), npass=1, act=1, out_dtype=BF).cpu()
    _check('gemm_nt relu %s' % ((M, N, K),), out, torch.relu(lin), ab, excess=K + 16)
    if N % 256 or M < 256 or K > 768:
        return                                   # (a bf16 residual needs the A-stationary path: host check)
    out = ops.gemm_nt(A.to(dev), W.to(dev), b.to(dev), npass=1, residual=res.to(dev), res_mod=M, out_dtype=BF).cpu()
    _check('gemm_nt residual %s' % ((M, N, K),), out, lin + _b(res), ab + _b(res).abs(), excess=K + 16)


@pytest.mark.parametrize('M,N,K', [(1000, 768, 256), (333, 256, 512), (4096, 512, 256), (130, 256, 768), (256, 256, 128), (PAPER_M, 768, 256)])
def test_strip_linear_bf16_at_the_ulp(dev, M, N, K):
    ops = _ops()
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(BF); W = torch.randn(N, K, generator=g) / math.sqrt(K); b = torch.randn(N, generator=g)
    lin = _b(x) @ _b(W).T + b.double()
    ab = _b(x).abs() @ _b(W).abs().T + b.double().abs()
    out = ops.strip_linear(x.to(dev), ops.strip_pack(W.to(dev)), N, bias=b.to(dev), out_dtype=BF).cpu()
    _check('strip_linear %s' % ((M, N, K),), out, lin, ab, excess=K + 16)


@pytest.mark.parametrize('M,K,p', [(1000, 256, 0.0), (515, 256, 0.2), (384, 512, 0.1), (256, 768, 0.0), (PAPER_M, 256, 0.1)])
def test_strip_linear_residual_layernorm_at_the_ulp(dev, M, K, p):
    """fc_o + dropout + bf16 residual + LayerNorm: the pre-LayerNorm sum and the output each rounded once from fp32"""
    ops = _ops()
    N = 256
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(BF); W = torch.randn(N, K, generator=g) / math.sqrt(K); b = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(BF); gam = 1 + 0.3 * torch.randn(N, generator=g); bet = torch.randn(N, generator=g)
    site, seed = 4, 99
    out, pre, _, _ = ops.strip_linear(x.to(dev), ops.strip_pack(W.to(dev)), N, bias=b.to(dev), drop_p=p, drop_site=site, drop_seed=seed,
                                      residual=res.to(dev), ln=(gam.to(dev), bet.to(dev)))
    m = keep_mask_t(seed, site, (M, N), p).double() * keep_scale(p) if p > 0 else 1.0
    r = (_b(x) @ _b(W).T + b.double()) * m + _b(res)
    absr = (_b(x).abs() @ _b(W).abs().T + b.double().abs()) * m + _b(res).abs()
    _check('strip_linear+LN pre %s' % ((M, K, p),), pre.cpu(), r, absr, excess=K + 16)
    y, absy = _ln64(r, gam, bet, absr)
    _check('strip_linear+LN out %s' % ((M, K, p),), out.cpu(), y, absy, excess=K + N + 16)


@pytest.mark.parametrize('M,pf,p', [(1000, 512, 0.0), (643, 512, 0.1), (256, 128, 0.25), (4096, 1024, 0.0), (PAPER_M, 512, 0.1)])
def test_fused_ffn_at_the_ulp(dev, M, pf, p):
    """strip_mlp2 forward: the hidden rounded to bf16 once (stored, and the operand of fc_2), then the residual sum and LayerNorm"""
    ops = _ops()
    d = 256
    g = torch.Generator().manual_seed(M + pf)
    x = torch.randn(M, d, generator=g).to(BF)
    W1 = torch.randn(pf, d, generator=g) / math.sqrt(d); b1 = 0.5 * torch.randn(pf, generator=g)
    W2 = torch.randn(d, pf, generator=g) / math.sqrt(pf); b2 = 0.5 * torch.randn(d, generator=g)
    gam = 1 + 0.3 * torch.randn(d, generator=g); bet = torch.randn(d, generator=g)
    site_h, site_o, seed = 11, 12, 424242
    y, hid, pre, _, _ = ops.ffn_res_ln_fwd(x.to(dev), ops.ffn_pack(W1.to(dev), W2.to(dev)), pf, b1.to(dev), b2.to(dev), gam.to(dev), bet.to(dev),
                                           drop_p=p, site_h=site_h, site_o=site_o, seed=seed)
    mh = keep_mask_t(seed, site_h, (M, pf), p).double() * keep_scale(p) if p > 0 else 1.0
    mo = keep_mask_t(seed, site_o, (M, d), p).double() * keep_scale(p) if p > 0 else 1.0
    h = torch.relu(_b(x) @ _b(W1).T + b1.double()) * mh
    absh = (_b(x).abs() @ _b(W1).abs().T + b1.double().abs()) * mh
    _check('ffn hidden %s' % ((M, pf, p),), hid.cpu(), h, absh, excess=d + 16)
    hb = E.rne(h)
    r = (hb @ _b(W2).T + b2.double()) * mo + _b(x)
    absr = (hb.abs() @ _b(W2).abs().T + b2.double().abs()) * mo + _b(x).abs()
    _check('ffn pre %s' % ((M, pf, p),), pre.cpu(), r, absr, excess=E.EXCESS_ROUNDED, row_ident=E.ROW_IDENT_ROUNDED)   # (near-ties of the hidden)
    yr, absy = _ln64(r, gam, bet, absr)
    _check('ffn out %s' % ((M, pf, p),), y.cpu(), yr, absy, excess=E.EXCESS_ROUNDED, row_ident=E.ROW_IDENT_ROUNDED)


@pytest.mark.parametrize('M,N,K', [(1120, 192, 64), (4096 + 96, 128, 64), (256, 64, 64), (1120, 64, 128), (90112, 64, 192), (262144, 192, 64)])
def test_bf16_small_strip_linear_at_the_ulp(dev, M, N, K):
    """bs_strip (d = 64, ff = 128): plain, ReLU + scale + residual, dropout + broadcast residual, transposed pack"""
    ops = _ops()
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(BF); W = torch.randn(N, K, generator=g) / math.sqrt(K); b = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(BF)
    wp = ops.x3s_pack(W.to(dev), 4)
    lin = _b(x) @ _b(W).T + b.double()
    ab = _b(x).abs() @ _b(W).abs().T + b.double().abs()
    _check('bs_strip %s' % ((M, N, K),), ops.strip_linear(x.to(dev), wp, N, b.to(dev)).cpu(), lin, ab, excess=K + 16)
    if N == 64:
        out = ops.strip_linear(x.to(dev), wp, N, b.to(dev), relu=True, out_scale=0.5, residual=res.to(dev)).cpu()
        _check('bs_strip relu+res %s' % ((M, N, K),), out, torch.relu(lin) * 0.5 + _b(res), ab * 0.5 + _b(res).abs(), excess=K + 16)
        p, site, seed = 0.1, 3, 4242
        m = keep_mask_t(seed, site, (M, N), p).double() * keep_scale(p)
        rr = _b(res)[torch.arange(M) % 7]
        out = ops.strip_linear(x.to(dev), wp, N, b.to(dev), drop_p=p, drop_site=site, drop_seed=seed, residual=res[:7].contiguous().to(dev), res_mod=7).cpu()
        _check('bs_strip drop+res %s' % ((M, N, K),), out, lin * m + rr, ab * m + rr.abs(), excess=K + 16)
    if K == 64:
        dy = (torch.randn(M, N, generator=g) * 1e-5).to(BF)
        out = ops.strip_linear(dy.to(dev), ops.x3s_pack(W.to(dev), 4, transpose=True), K, None).cpu()
        _check('bs_strip transposed %s' % ((M, N, K),), out, _b(dy) @ _b(W), _b(dy).abs() @ _b(W).abs(), excess=N + 16)


@pytest.mark.parametrize('M', [1120, 2 * 128 * 88])
def test_bf16_small_strip_linear_layernorm_at_the_ulp(dev, M):
    ops = _ops()
    N = K = 64
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(BF); W = torch.randn(N, K, generator=g) / math.sqrt(K); b = torch.randn(N, generator=g)
    res = (torch.randn(M, N, generator=g) * 3.0).to(BF); gam = torch.randn(N, generator=g); bet = torch.randn(N, generator=g)
    p, site, seed = 0.1, 11, 99
    m = keep_mask_t(seed, site, (M, N), p).double() * keep_scale(p)
    out, pre, _, _ = ops.strip_linear(x.to(dev), ops.x3s_pack(W.to(dev), 4), N, b.to(dev), drop_p=p, drop_site=site, drop_seed=seed,
                                      residual=res.to(dev), ln=(gam.to(dev), bet.to(dev)))
    r = (_b(x) @ _b(W).T + b.double()) * m + _b(res)
    absr = (_b(x).abs() @ _b(W).abs().T + b.double().abs()) * m + _b(res).abs()
    _check('bs_strip+LN pre %d' % M, pre.cpu(), r, absr, excess=K + 16)
    y, absy = _ln64(r, gam, bet, absr)
    _check('bs_strip+LN out %d' % M, out.cpu(), y, absy, excess=K + N + 16)
