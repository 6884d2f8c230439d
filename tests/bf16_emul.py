"""An fp64 model of the bf16 (single-pass) mode's forward roundings, kernel by kernel (test infrastructure, CPU).

Each model takes the kernel's inputs (exact in bf16) and evaluates its arithmetic in a working dtype: float64 gives what the kernel's roundings
predict; float32 (summed in fp32, like the matrix cores) stands in for a correct device and calibrates the criterion (see ulp_stats).  The
bf16 stores are modelled by rne(), a single correctly rounded step from the working dtype (torch's double -> bfloat16 goes through float and
can round twice).

Rounding points of the two attention forwards (csrc/attn_fwd.hip, attn_fwd8.hip), all-bf16 io, npass == 1:
  * S = Q.K^T summed in fp32 from the bf16 operands; the row maximum is taken over the RAW scores and 1/sqrt(dh) is folded with log2(e) into
    the multiply in front of exp2: p = 2^((s - max) * c2).  lse = (raw max, 1/sum), sum over every key (dropped ones included);
  * attn_fwd_kernel (every shape, and the attention map): P = bf16(p * (1/sum) * keep_scale * mask) -- the NORMALISED probability is rounded
    (attn_fwd.hip, the `nrm` multiply before the P.V operand conversion); out = bf16(P.V);
  * attn_fwd8_kernel (dh 64, 128 < Lq, Lk <= 256, no attention map): P = bf16(p * keep_scale * mask) -- the UNNORMALISED probability is
    rounded, 1/sum is applied to the fp32 accumulator at the end; out = bf16((P.V) * (1/sum)).

Deliberately wrong variants (Switches) for the tests that prove the criterion has resolution:
  p_unrounded    P enters P.V at full width;
  p_norm_late    attn_fwd8 applies 1/sum before rounding P (i.e. attn_fwd_kernel's rounding point in the fwd8 model);
  drop_late      the dropout scale is applied after P is rounded;
  trunc          every bf16 store truncates instead of rounding to nearest even.
"""
import math
from dataclasses import dataclass

import torch


@dataclass(frozen=True)
class Switches:
    p_unrounded: bool = False
    p_norm_late: bool = False
    drop_late: bool = False
    trunc: bool = False


def rne(x):
    """x rounded to the nearest bf16 value, ties to even, in ONE step from x's dtype (finite, normal range)"""
    m, e = torch.frexp(x)                                    # x = m 2^e, 0.5 <= |m| < 1: bf16 keeps 8 significant bits
    return torch.ldexp(torch.round(m * 256.0), e - 8).to(x.dtype)


def trunc(x):
    """x with its mantissa cut to bf16's 8 significant bits (round toward zero)"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.trunc(m * 256.0), e - 8).to(x.dtype)


# the per-kernel criterion (tests/test_bf16_ulp_gpu.py), set from the CPU calibration of test_bf16_emul_bound.py: the models summed in fp32 keep
# >= 99.92 % of the attention outputs and >= 99.9 % of the stream outputs bit-identical to rne(model64); each wrong variant keeps <= 73 %
# (a tail variant: its rows <= 50 %)
IDENT_ATTN = 0.998          # attention output: fraction bit-identical (device, worst case: 99.84 % at dh 32)
EXCESS_ROUNDED = 8192       # ... and beyond one ulp by at most 2^-11 of its terms' magnitude where a ROUNDED intermediate is an operand (P in
                            # P.V, the FFN hidden in fc_2): fp32 and fp64 round its near-ties differently (fp32 models: up to 2.4e3 for attention,
                            # 3.8e3 for the fused FFN at M = 65536)
IDENT_OTHER_FORM = 0.9      # the other attention forward's model shares ~50 % of the bits: below this, the output is not that form's
LSE_MAX_ULPS = 16           # raw row max against fp64, fp32 ulps (fp32 model: 2.2)
LSE_INV_ULPS = 32           # 1/sum (fp32 model: 3.4; the device's exp2 is not correctly rounded)
IDENT_STREAM = 0.999        # strip / gemm / LayerNorm outputs: fraction bit-identical (the excess bound is K (+ N) units: the fp32 sums)
ROW_IDENT_STREAM = 0.9      # every ROW (a token's outputs) on its own: a defect confined to a tail -- the last partial strip, a clamped query
                            # row -- moves the whole fraction by less than 1 % but empties its rows (truncation: ~50 % of a row identical)
ROW_IDENT_ROUNDED = 0.65    # ... where a ROUNDED intermediate is an operand (P, the FFN hidden): a near-tie of one of its elements moves the
                            # row's outputs together (fp32 models: attention rows down to 84 %, fused FFN down to 78 % at M = 65536); a row
                            # whose output store truncates keeps <= 50 %


def store(x, sw=Switches()):
    return trunc(x) if sw.trunc else rne(x)


# ---------------------------------------------------------------------------------------------------------------------------- attention
def attention(q, k, v, H, form, mask=None, keep=1.0, dtype=torch.float64, sw=Switches(), want_abs=False):
    """The attention forward of `form` ('fwd8': attn_fwd8_kernel, 'fwd': attn_fwd_kernel<KT, dh, 1, true>) on q [n, Lq, d], k / v [n, Lk, d].
    mask: the device's keep mask [n, H, Lq, Lk] (bool) or None; keep: the kept elements' scale (util.keep_scale).
    Returns (out before its bf16 store [n, Lq, d], raw row max [n, H, Lq], 1/sum [n, H, Lq]) in `dtype`; want_abs: also the magnitude of the
    output's terms, |P|.|V| (times 1/sum for fwd8), the scale of its fp32 summation error (see excess)."""
    n, Lq, d = q.shape
    Lk = k.shape[1]
    dh = d // H

    def heads(t, L):
        return t.to(dtype).reshape(n, L, H, dh).transpose(1, 2)
    qh, kh, vh = heads(q, Lq), heads(k, Lk), heads(v, Lk)
    s = torch.matmul(qh, kh.transpose(-1, -2))
    mx = s.amax(-1, keepdim=True)
    scale = 1.0 / math.sqrt(dh) if dtype == torch.float64 else torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32).item()
    p = torch.exp((s - mx) * scale)
    inv = 1.0 / p.sum(-1, keepdim=True)
    m = mask.to(dtype) if mask is not None else None

    def dropped(t, sc):
        if m is None:
            return t
        return t * m * sc

    rnd = (lambda t: t) if sw.p_unrounded else (lambda t: store(t, sw))
    if form == 'fwd8' and not sw.p_norm_late:
        P = rnd(p) * m * keep if (sw.drop_late and m is not None) else rnd(dropped(p, keep))
        o = torch.matmul(P, vh) * inv
        ab = torch.matmul(P.abs(), vh.abs()) * inv if want_abs else None
    else:
        P = rnd(p * inv) * m * keep if (sw.drop_late and m is not None) else rnd(dropped(p * inv, keep))
        o = torch.matmul(P, vh)
        ab = torch.matmul(P.abs(), vh.abs()) if want_abs else None

    def flat(t):
        return t.transpose(1, 2).reshape(n, Lq, d)
    res = (flat(o), mx.squeeze(-1), inv.squeeze(-1))
    return res + (flat(ab),) if want_abs else res


# ---------------------------------------------------------------------------------------------------------------------------- the criterion
def _ordered(t):
    """bf16 values -> integers whose differences count bf16 ulps (sign-magnitude bit patterns made monotone; +0 == -0)"""
    b = t.to(torch.bfloat16).view(torch.int16).to(torch.int32)
    mag = b & 0x7FFF
    return torch.where(b < 0, -mag, mag)


def ulp_stats(dev_bf16, ref):
    """(max ulp distance, fraction of bit-identical elements) of the bf16 tensor dev_bf16 against rne(ref) (ref in float64 / float32)"""
    a = _ordered(dev_bf16.detach().cpu())
    b = _ordered(rne(ref.detach().cpu().to(torch.float64)).to(torch.float32))
    dist = (a - b).abs()
    return int(dist.max().item()), (dist == 0).double().mean().item()


def row_ident_min(dev_bf16, ref):
    """the smallest fraction of bit-identical elements over the rows (last dimension) of dev_bf16 against rne(ref)"""
    a = _ordered(dev_bf16.detach().cpu())
    b = _ordered(rne(ref.detach().cpu().to(torch.float64)).to(torch.float32))
    same = (a == b).reshape(-1, a.shape[-1]).double()
    return same.mean(1).min().item()


def fp32_ulps(x, ref):
    """max |x - ref| in units of the fp32 spacing at ref (2^-23 |ref|, floored at the smallest normal)"""
    x = x.detach().cpu().double()
    ref = ref.detach().cpu().double()
    return ((x - ref).abs() / (ref.abs().clamp_min(2.0 ** -126) * 2.0 ** -23)).max().item()


def bf16_spacing(x):
    """the spacing of bf16 values at |x| (2^(e-8) for |x| in [2^(e-1), 2^e))"""
    _, e = torch.frexp(x.double())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


def excess(dev_bf16, ref, absref):
    """max over the elements of (|dev - rne(ref)| - one bf16 spacing at ref) / (2^-24 absref): how far beyond ONE bf16 ulp the stored value
    lies, in units of fp32 rounding of the terms' magnitude absref (sum |a_i b_i| of the element's product; a result that cancels to far
    below absref carries the fp32 summation error of its terms, which one ulp at its own size cannot hold).  <= 0: every element within 1 ulp."""
    d = dev_bf16.detach().cpu().double()
    r = ref.detach().cpu().double()
    over = (d - rne(r)).abs() - bf16_spacing(torch.maximum(r.abs(), rne(r).abs()))
    return (over / (absref.detach().cpu().double() * 2.0 ** -24)).max().item()
