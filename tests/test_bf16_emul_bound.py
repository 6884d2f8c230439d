"""The per-kernel criterion of the bf16 forward (tests/test_bf16_ulp_gpu.py, constants in tests/bf16_emul.py) has the resolution it is meant
to have, without a GPU.

Each kernel model evaluated in fp32 (summed in fp32 like the matrix cores: a stand-in for a correct device) must pass the criterion against
the same model in fp64; deliberately wrong variants must fail it -- P left unrounded, P rounded after normalisation in attn_fwd8's model, the
dropout scale applied after rounding, truncating stores, a LayerNorm read from the rounded pre-LayerNorm sum.  The attention variants and
the second rounding stay inside the bands the older tests use (2e-2 of the max for attention, 6e-3 / 8e-3 for the strip outputs)."""
import math

import pytest
import torch

import bf16_emul as E
from util import keep_scale, keep_mask_t, rel_err

BF = torch.bfloat16
# (n, H, Lq, Lk, dh, p): an attn_fwd8 shape with partial query and key blocks and the per-element dropout form, a decoder shape at dh 32
ATTN = [(2, 4, 160, 200, 64, 0.1), (2, 4, 255, 255, 64, 0.1), (3, 2, 88, 256, 32, 0.0), (3, 4, 129, 129, 64, 0.0)]
VARIANTS = {'p_unrounded': E.Switches(p_unrounded=True), 'p_norm_late': E.Switches(p_norm_late=True),
            'drop_late': E.Switches(drop_late=True), 'trunc': E.Switches(trunc=True)}


@pytest.fixture(scope='module')
def attn_cases():
    out = {}
    for n, H, Lq, Lk, dh, p in ATTN:
        g = torch.Generator().manual_seed(Lq * 1000 + Lk)
        d = H * dh
        q = (torch.randn(n, Lq, d, generator=g) * 0.5).to(BF)
        k, v = torch.randn(n, Lk, d, generator=g).to(BF), torch.randn(n, Lk, d, generator=g).to(BF)
        mask = keep_mask_t(777, 5, (n, H, Lq, Lk), p) if p > 0 else None
        out[(n, H, Lq, Lk, dh, p)] = (q, k, v, H, mask, keep_scale(p))
    return out


def _applies(kind, form, p):
    """variants that change nothing in this (form, p): p_norm_late is attn_fwd_kernel's own rounding point; drop_late needs dropout"""
    return not ((kind == 'p_norm_late' and form == 'fwd') or (kind == 'drop_late' and p == 0.0))


@pytest.mark.parametrize('form', ['fwd8', 'fwd'])
@pytest.mark.parametrize('case', ATTN)
def test_attention_models_separate(attn_cases, case, form):
    q, k, v, H, mask, keep = attn_cases[case]
    p = case[-1]
    o64, mx64, inv64, ab = E.attention(q, k, v, H, form, mask, keep, want_abs=True)
    o32, mx32, inv32 = E.attention(q, k, v, H, form, mask, keep, dtype=torch.float32)
    d32 = E.rne(o32).to(BF)
    _, f32 = E.ulp_stats(d32, o64)
    x32 = E.excess(d32, o64, ab)
    emx, einv = E.fp32_ulps(mx32, mx64), E.fp32_ulps(inv32, inv64)
    print('\n%s %s  model in fp32: identical %.5f  excess %.0f  lse %.1f / %.1f ulp' % (form, case, f32, x32, emx, einv))
    r32 = E.row_ident_min(d32, o64)
    print('   worst row of the fp32 model: %.4f' % r32)
    assert f32 >= E.IDENT_ATTN and x32 <= E.EXCESS_ROUNDED and r32 >= E.ROW_IDENT_ROUNDED
    assert emx <= E.LSE_MAX_ULPS / 4 and einv <= E.LSE_INV_ULPS / 4
    other = E.attention(q, k, v, H, 'fwd' if form == 'fwd8' else 'fwd8', mask, keep)[0]
    _, fo = E.ulp_stats(E.rne(other).to(BF), o64)
    print('   the other form: identical %.5f' % fo)
    assert fo < E.IDENT_OTHER_FORM
    for kind, sw in VARIANTS.items():
        if not _applies(kind, form, p):
            continue
        ov = E.store(E.attention(q, k, v, H, form, mask, keep, dtype=torch.float32, sw=sw)[0], sw).to(BF)
        _, fv = E.ulp_stats(ov, o64)
        band = rel_err(ov.float(), o64)
        print('   %-12s identical %.5f  excess %.0f  old band (rel. to max) %.1e' % (kind, fv, E.excess(ov, o64, ab), band))
        assert fv < E.IDENT_ATTN, kind
        assert band < 2e-2, kind
    # a defect confined to the tail: the last query row (at Lq = 129 the clamped row of a wave whose other 31 rows idle) truncated
    tail = E.rne(o32)
    tail[:, -1] = E.trunc(o32[:, -1])
    ft, rt = E.ulp_stats(tail.to(BF), o64)[1], E.row_ident_min(tail.to(BF), o64)
    print('   last row truncated: identical %.5f  worst row %.4f  old band %.1e' % (ft, rt, rel_err(tail, o64)))
    assert rt < E.ROW_IDENT_ROUNDED and rel_err(tail, o64) < 2e-2
    if case[2] % 32 == 1:
        assert ft < E.IDENT_ATTN, 'one truncated row of %d not seen by the whole-tensor fraction' % case[2]


def test_strip_layernorm_criterion_separates():
    """the strip_linear + residual + LayerNorm outputs: the fp32 evaluation passes; a truncating store, a truncating store in the last partial
    strip only (8 of 1000 rows) and a LayerNorm computed from the ROUNDED pre-LayerNorm sum (a second rounding of the stream) fail; the last two
    stay inside the old 6e-3 / 8e-3 bands"""
    M, N, K = 1000, 256, 256
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(BF); W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF); b = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(BF); gam = 1 + 0.3 * torch.randn(N, generator=g); bet = torch.randn(N, generator=g)

    def tail_trunc(t):
        out = E.rne(t)
        out[-8:] = E.trunc(t[-8:])
        return out

    def run(dt, pre_rounded=False, store=E.rne):
        r = x.to(dt) @ W.to(dt).T + b.to(dt) + res.to(dt)
        absr = x.to(dt).abs() @ W.to(dt).abs().T + b.to(dt).abs() + res.to(dt).abs()
        rr = E.rne(r) if pre_rounded else r
        mu = rr.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(rr.var(1, unbiased=False, keepdim=True) + 1e-5)
        y = (rr - mu) * rstd * gam.to(dt) + bet.to(dt)
        absy = rstd * gam.to(dt).abs() * (r.abs() + mu.abs() + absr) + bet.to(dt).abs()
        return store(r), store(y), r, y, absr, absy
    _, _, r64, y64, absr, absy = run(torch.float64)
    rows = {'fp32': run(torch.float32), 'trunc': run(torch.float32, store=E.trunc), 'trunc_last_strip': run(torch.float32, store=tail_trunc),
            'ln_of_rounded_pre': run(torch.float32, pre_rounded=True)}
    for kind, (pre, y, *_rest) in rows.items():
        _, fp = E.ulp_stats(pre.to(BF), r64)
        _, fy = E.ulp_stats(y.to(BF), y64)
        wp, wy = E.row_ident_min(pre.to(BF), r64), E.row_ident_min(y.to(BF), y64)
        xp, xy = E.excess(pre.to(BF), r64, absr), E.excess(y.to(BF), y64, absy)
        print('%-18s pre: identical %.5f row %.3f excess %.1f   out: identical %.5f row %.3f excess %.1f   old bands %.1e / %.1e' % (
            kind, fp, wp, xp, fy, wy, xy, rel_err(pre, r64), rel_err(y, y64)))
        if kind == 'fp32':
            assert min(fp, fy) >= E.IDENT_STREAM and min(wp, wy) >= E.ROW_IDENT_STREAM and xp <= K + 16 and xy <= K + N + 16
        else:
            assert min(fp, fy) < E.IDENT_STREAM, kind
            if kind != 'ln_of_rounded_pre':
                assert min(wp, wy) < E.ROW_IDENT_STREAM, kind
            if kind != 'trunc':                      # (a truncating store of pre everywhere reaches 7e-3 of the max: the old band sees that one)
                assert rel_err(pre, r64) < 6e-3 and rel_err(y, y64) < 8e-3, kind
