"""CPU calibration of the backward plan's link check (tests/bwd_plan_emul.py; the device side is tests/test_bwd_plan_gpu.py).

(a) For every launch kind of the x3 / parity backward plans a record at the smallest shapes; the stand-in for a correct device -- the same
    contract summed in fp32 on x3's operand splits (x3_emul.x3mm), bf16 stores rounded -- passes every bound of its kind.
(b) Each planted defect, applied to the stand-in of its own kind, fails there.  The size of each defect at its launch (largest change of an
    output over that output's maximum) is printed: the plan-level defects of the list change a whole launch (a gate scale of 1 instead of
    256 / 230 is 10 % of dh), so at their own launch they are not small; what reaches a parameter's gradient is what the whole-model bands
    (2e-2 .. 3e-2 on the first-layer tensors) have to see through every launch behind it.
(c) The score conditioning (bwd_plan_emul.condition) brings every attention of the two small configurations inside the table's figure, and
    that figure is what the ATTN_CASES give.
No defect is invisible today (bwd_plan_emul.DEFECTS_INVISIBLE is empty; the mechanism of tests/bf16_plan_emul.py is kept)."""
import math

import pytest
import torch

import bwd_plan_emul as PE
import util
from util import keep_scale

BF = torch.bfloat16
SEED, P = 20250101, 0.1


def _g(k):
    return torch.Generator().manual_seed(1000 + k)


def _rnd(g, *s, scale=1.0):
    return torch.randn(*s, generator=g) * scale


def rec_gemm_nt():
    """a block-plan dX launch: gradient A, the transposed weights, the stored hidden as gate x gate_scale, dr as residual"""
    g = _g(1)
    M, N, K = 40, 96, 64
    return dict(kind='gemm_nt', npass=4, A=_rnd(g, M, K, scale=1e-5), W=_rnd(g, N, K) / 8.0, gate=_rnd(g, M, N), gate_scale=keep_scale(P), out_scale=1.0,
                act=0, drop_p=0.0, site=0, seed=SEED, residual=_rnd(g, M, N, scale=1e-5), res_mod=M, prior={})


def rec_gemm_nt_epilogue():
    """every epilogue term of the contract in its documented order: bias, ReLU, out_scale, add_table[row % add_mod], dropout, residual[row % res_mod]"""
    g = _g(13)
    M, N, K = 40, 64, 32
    return dict(kind='gemm_nt', npass=2, A=_rnd(g, M, K), W=_rnd(g, N, K) / 6.0, bias=_rnd(g, 1, N), act=1, out_scale=8.0, add_table=_rnd(g, 8, N), add_mod=8,
                drop_p=P, site=3, seed=SEED, residual=_rnd(g, 12, N), res_mod=12, prior={})


def rec_strip_linear(x_drop=False):
    g = _g(2)
    M, N, K = 64, 64, 64
    r = dict(kind='strip_linear', npass=4, A=_rnd(g, M, K, scale=1e-5), W=_rnd(g, N, K) / 8.0, out_scale=1.0, gate_scale=1.0, drop_p=P if x_drop else 0.0,
             site=5, seed=SEED, x_drop=x_drop, res_mod=0, prior={})
    if not x_drop:
        r['residual'] = _rnd(g, M, N, scale=1e-5)
    return r


def rec_ffn_bwd_dx():
    g = _g(3)
    M, d, p = 64, 64, 128
    return dict(kind='ffn_bwd_dx', x=_rnd(g, M, d, scale=1e-5), W_a=_rnd(g, p, d) / 8.0, W_b=_rnd(g, d, p) / 11.0, gate=_rnd(g, M, p).to(BF),
                gate_scale=keep_scale(P), drop_p=P, site_o=7, seed=SEED, residual=_rnd(g, M, d, scale=1e-5), h_bf=True, prior={})


def rec_gemm_tn(beta=0.0, dy_drop=False, K_out=None, out_scale=1.0, segs=None, M=200, N=64, K=32):
    g = _g(4)
    segs = segs or [(0, N)]
    K_out = K_out or K
    mag = 1e-6 * math.sqrt(M)
    prior = {}
    for i, (r0, rows) in enumerate(segs):
        prior['dw%d' % i] = _rnd(g, rows, K_out, scale=mag)
        prior['db%d' % i] = _rnd(g, 1, rows, scale=mag)
    return dict(kind='gemm_tn', npass=4, dY=_rnd(g, M, N, scale=1e-6), X=_rnd(g, M, K), out_scale=out_scale, beta=beta, K_out=K_out, segs=segs,
                has_db=[True] * len(segs), dy_hi=False, dy_drop=dy_drop, drop_p=P if dy_drop else 0.0, site=9, seed=SEED, prior=prior)


def rec_attn_bwd():
    g = _g(5)
    n, H, Lq, Lk, dh = 2, 2, 12, 16, 32
    d = H * dh
    return dict(kind='attn_bwd', q=_rnd(g, n, Lq, d), k=_rnd(g, n, Lk, d), v=_rnd(g, n, Lk, d), dout=_rnd(g, n, Lq, d, scale=1e-5), H=H, drop_p=P, site=11,
                seed=SEED, planes=False, mode='x3', prior={})


def rec_ln_bwd():
    g = _g(6)
    M, N = 33, 64
    r = (_rnd(g, M, N) * 2 + 0.5).to(BF)
    r64 = r.double()
    return dict(kind='ln_bwd', dy=_rnd(g, M, N, scale=1e-5), r=r, mean=r64.mean(1).float(), rstd=(1.0 / torch.sqrt(r64.var(1, unbiased=False) + 1e-5)).float(),
                gamma=1 + 0.2 * _rnd(g, N), drop_p=P, site=13, seed=SEED, has_drop=True, drop_bf=False, prior={})


def rec_ln_bwd_reduce():
    g = _g(7)
    N = 64
    return dict(kind='ln_bwd_reduce', N=N, beta=1.0, ws=_rnd(g, 17, 2 * N, scale=1e-5), prior=dict(dg=_rnd(g, 1, N, scale=1e-4), db=_rnd(g, 1, N, scale=1e-4)))


def rec_heads_split_bwd():
    g = _g(8)
    B, T, N, V = 2, 4, 3, 4
    return dict(kind='heads_split_bwd', B=B, T=T, N=N, V=V, ldl=64, tm=1, prob=[torch.rand(B, T, N, generator=g) for _ in range(3)],
                d_prob=[_rnd(g, B, T, N, scale=1e-3) for _ in range(3)], d_vel=_rnd(g, B * T * N, V, scale=1e-3), prior={})


def rec_time_embed_bwd():
    g = _g(9)
    B, T, N, d = 2, 4, 3, 64
    return dict(kind='time_embed_bwd', shape=(B, T, N, d), scale=math.sqrt(d), dy=_rnd(g, B * N * T, d, scale=1e-5), drop_p=P, site=15, seed=SEED, has_dym=True,
                prior=dict(dx=_rnd(g, B * T * N, d, scale=1e-4)))


def rec_colsum():
    """the time position table's gradient: the column sum of the MASKED gradient (time_embed_bwd's dym), rows (b, n), columns (t, c)"""
    g = _g(10)
    rows, n = 24, 96
    raw = _rnd(g, rows, n, scale=1e-5)
    masked = raw * PE.scaled_mask(SEED, 15, (rows, n), P, torch.float32)
    return dict(kind='colsum', x=masked, x_unmasked=raw, beta=0.0, prior=dict(out=torch.full((1, n), float('nan'))))


def rec_dropout_bwd_colsum():
    g = _g(11)
    rows, n = 8, 128
    return dict(kind='dropout_bwd_colsum', beta=0.0, ld=n, drop_p=P, site=1, seed=SEED, prior=dict(g=_rnd(g, rows, n, scale=1e-5), out=torch.zeros(1, n)))


def rec_embed_fold_bwd():
    g = _g(12)
    d, C_, kw, n_proc, Kp = 64, 4, 5, 9, 32
    nw = n_proc - kw + 1
    return dict(kind='embed_fold_bwd', n_proc=n_proc, dweff=_rnd(g, d, Kp, scale=1e-4), dbeff=_rnd(g, 1, d, scale=1e-4), wconv=_rnd(g, C_, kw),
                bconv=_rnd(g, 1, C_), wtok=_rnd(g, d, C_ * nw) / 4.0, btok=_rnd(g, 1, d), prior={})


RECORDS = {
    'gemm_nt': rec_gemm_nt, 'gemm_nt_epilogue': rec_gemm_nt_epilogue, 'gemm_nt_parity': lambda: dict(rec_gemm_nt(), npass=3),
    'strip_linear': rec_strip_linear, 'strip_linear_x_drop': lambda: rec_strip_linear(True), 'ffn_bwd_dx': rec_ffn_bwd_dx,
    'gemm_tn': rec_gemm_tn, 'gemm_tn_dy_drop': lambda: rec_gemm_tn(dy_drop=True),
    'gemm_tn_beta_segs': lambda: rec_gemm_tn(beta=1.0, segs=[(0, 16), (16, 1), (17, 1), (18, 1)]),
    'gemm_tn_k_out_scale': lambda: rec_gemm_tn(K_out=9, out_scale=8.0, M=100),
    'gemm_tn_dy_hi': lambda: dict(rec_gemm_tn(), dy_hi=True),                     # HFTT_TN_DY_HI: against the product of bf16(dY)
    'gemm_tn_bf16_operands': lambda: (lambda r: dict(r, dY=r['dY'].to(BF), X=r['X'].to(BF)))(rec_gemm_tn()),      # the stored hidden / its gradient
    'gemm_tn_parity': lambda: dict(rec_gemm_tn(segs=[(0, 32), (32, 32)]), npass=3),
    'attn_bwd': rec_attn_bwd, 'attn_bwd_parity': lambda: dict(rec_attn_bwd(), mode='parity'), 'ln_bwd': rec_ln_bwd, 'ln_bwd_reduce': rec_ln_bwd_reduce,
    'heads_split_bwd': rec_heads_split_bwd, 'heads_split_bwd_freq': lambda: dict(rec_heads_split_bwd(), tm=0), 'time_embed_bwd': rec_time_embed_bwd,
    'colsum': rec_colsum, 'dropout_bwd_colsum': rec_dropout_bwd_colsum, 'embed_fold_bwd': rec_embed_fold_bwd,
}
# the record each defect is planted in
DEFECT_RECORD = {
    'gate_scale_left_at_1': 'ffn_bwd_dx', 'dy_drop_mask_ignored': 'gemm_tn_dy_drop', 'beta0_on_accumulating_segment': 'gemm_tn_beta_segs',
    'seg_row0_off_by_one': 'gemm_tn_beta_segs', 'k_out_columns_from_k': 'gemm_tn_k_out_scale', 'out_scale_sqrt_d_dropped': 'gemm_tn_k_out_scale',
    'dx_residual_dropped': 'strip_linear', 'delta_without_dropout_mask': 'attn_bwd', 'time_embed_bwd_overwrites': 'time_embed_bwd',
    'pos_colsum_reads_unmasked': 'colsum', 'ln_dr_drop_wrong_site': 'ln_bwd', 'heads_sigmoid_from_logits': 'heads_split_bwd',
}


def test_every_kind_has_a_contract_a_record_and_every_defect_a_kind():
    assert set(PE.KINDS) == set(PE.CONTRACTS) == {r()['kind'] for r in RECORDS.values()}
    assert set(PE.DEFECTS) == set(DEFECT_RECORD) and set(PE.DEFECTS_INVISIBLE) <= set(PE.DEFECTS)
    for name, kind in PE.DEFECTS.items():
        assert RECORDS[DEFECT_RECORD[name]]()['kind'] == kind, name


@pytest.mark.parametrize('name', list(RECORDS))
def test_the_stand_in_passes_every_bound_of_its_kind(name):
    rec = RECORDS[name]()
    figs = PE.check(rec, PE.CONTRACTS[rec['kind']](rec, emul=True))
    print('\n'.join('%-24s %-14s %.3e (bound %.3e)' % ((name,) + f) for f in figs))
    assert not PE.failures(figs), PE.failures(figs)


def _size(a, b):
    """the largest change of an output, over that output's maximum"""
    worst = 0.0
    for k, v in b.items():
        if torch.is_tensor(v) and k in a and v.numel():
            worst = max(worst, ((PE.D(a[k]).reshape(-1) - PE.D(v).reshape(-1)).abs().max() / (PE.D(v).abs().max() + 1e-300)).item())
    return worst


@pytest.mark.parametrize('defect', list(PE.DEFECTS))
def test_planted_defect_fails_at_its_own_kind(defect):
    rec = RECORDS[DEFECT_RECORD[defect]]()
    fn = PE.CONTRACTS[rec['kind']]
    good, wrong = fn(rec, emul=True), fn(rec, emul=True, defect=defect)
    figs = PE.check(rec, wrong)
    print('%-32s at %-18s size %.2e   %s' % (defect, rec['kind'], _size(wrong, good), ['%s %.2e / %.1e' % f for f in PE.failures(figs)]))
    if defect in PE.DEFECTS_INVISIBLE:
        assert not PE.failures(figs), 'the defect %s has become visible: take it out of DEFECTS_INVISIBLE' % defect
        return
    assert _size(wrong, good) > 0.0, 'the defect changed nothing'
    assert PE.failures(figs), defect
    assert not PE.failures(PE.check(rec, good))


def test_conditioning_brings_every_attention_inside_the_table():
    from test_model_gpu import DROPOUT_CASES, OTHER_CONFIGS
    from util import O
    table = PE.attn_table_lmax()
    assert 5.0 < table < 6.0, table                 # (the largest of ~1e6 unit-variance scores: a figure outside is a changed table)
    seed = (1234 * 1000003 + 1) & 0xFFFFFFFFFFFFFFFF
    for name, cfg in (('x3_small', DROPOUT_CASES['x3_small'][1]), ('d128_ff256', OTHER_CONFIGS['d128_ff256'])):
        model = util.build_model(cfg, 31, dropout=P)
        util.perturb(model, 32)
        sd = util.sd_cpu(model)
        x = O.synth_spec(2, cfg, salt=13) * PE.INPUT_SCALE
        before = PE.model_lmax(sd, x, cfg, seed, P)
        lm, factors, _ = PE.condition(sd, x, cfg, seed, P, table)
        print(name, 'before', ['%.1f' % v for v in before.values()], 'after', ['%.2f' % v for v in lm.values()], factors)
        assert max(before.values()) > table and max(lm.values()) <= table and factors
        assert PE.model_lmax(sd, x, cfg, seed, P) == lm
