"""CPU calibration of the forward plan's link check (tests/fwd_plan_emul.py; the device side is tests/test_fwd_plan_gpu.py).

(a) An fp64 free-running model of the two smallest configurations (x3_small, d128_ff256 of tests/test_model_gpu.py) is walked in the launch
    order of PlanBuilder.forward and leaves one launch record per launch: in the strip form (strip_linear with planes and the LayerNorm
    epilogue, the one-descriptor FFN block in the encoder and in layer zero, the two-descriptor fused launch elsewhere, x3_to_planes on
    the shared query, the merged cross K / V where there are two decoder layers) and in the block form (every linear a gemm_nt), in both
    modes, with dropout 0.1 and -- x3 -- without.  The stand-in for a correct device passes every check of every record.
(b) Each planted defect, applied to the stand-in of its own kind, fails there; its size at its launch is printed.
No defect is invisible (fwd_plan_emul.DEFECTS_INVISIBLE is empty; the mechanism of tests/bf16_plan_emul.py is kept)."""
import math

import pytest
import torch

import bf16_plan_emul as BP
import engine_layouts as L
import fwd_plan_emul as FE
import util
from test_model_gpu import DROPOUT_CASES, OTHER_CONFIGS
from util import O

F64 = torch.float64
SEED, P = (1234 * 1000003 + 1) & 0xFFFFFFFFFFFFFFFF, 0.1
CONFIGS = {'x3_small': DROPOUT_CASES['x3_small'][1], 'd128_ff256': OTHER_CONFIGS['d128_ff256']}
_SD, _WALKS = {}, {}


def _inputs(name):
    if name not in _SD:
        cfg = CONFIGS[name]
        model = util.build_model(cfg, 31, dropout=P)
        util.perturb(model, 32)
        _SD[name] = ({k: v.double() for k, v in util.sd_cpu(model).items()}, O.synth_spec(2, cfg, salt=13) * FE.INPUT_SCALE, O.synth_labels(2, cfg, salt=14))
    return _SD[name]


def model_records(name, mode, strip, p):
    """the launch records of one forward + loss, free-running in fp64: every launch's outputs are its contract's, stored as the plan stores them"""
    key = (name, mode, strip, p)
    if key in _WALKS:
        return _WALKS[key]
    cfg = CONFIGS[name]
    sd, spec, labels = _inputs(name)
    npass = 2 if mode == 'x3' else 3
    B, T, F_, N, V, d = spec.shape[0], cfg.n_frame, cfg.n_bin, cfg.n_note, cfg.n_velocity, cfg.hid_dim
    Kp = (cfg.n_proc + 31) // 32 * 32
    Sn, BT, BN = B * T * N, B * T, B * N
    recs, site = [], [0]

    def new_site():
        site[0] += 1
        return site[0]

    def emit(tag, **rec):
        rec.update(tag=tag, prior={})
        recs.append(rec)
        return FE.CONTRACTS[rec['kind']](rec)

    def lin(tag, A, W, b, block=False, **kw):
        s = kw.pop('site', 0)
        return emit(tag, kind='gemm_nt' if (block or not strip) else 'strip_linear', npass=npass, A=A.float(), W=W, bias=b.reshape(1, -1), act=kw.pop('act', 0),
                    out_scale=kw.pop('out_scale', 1.0), drop_p=p if s else 0.0, site=s, seed=SEED, res_mod=kw.pop('res_mod', 0),
                    pre_bf=strip and mode == 'x3', **kw)

    def val(out, planes):
        return out['C']                             # (the contract's fp64 value: hi + lo of a plane store is that value to 2^-22)

    def attention(tag, q, k, v, H, n, Lq, Lk, **kw):
        s = new_site()
        return emit(tag, kind='attn_fwd', q=q.reshape(-1, Lq, d), k=k.reshape(n, Lk, d), v=v.reshape(n, Lk, d), H=H, drop_p=p, site=s, seed=SEED, mode=mode,
                    planes=strip, has_probs=kw.pop('has_probs', False), **kw)['out'].reshape(n * Lq, d)

    def ffn_part(tag, pre):
        pf = pre + 'positionwise_feedforward.'
        return dict(W1=sd[pf + 'fc_1.weight'], W2=sd[pf + 'fc_2.weight'], b1=sd[pf + 'fc_1.bias'].reshape(1, -1), b2=sd[pf + 'fc_2.bias'].reshape(1, -1),
                    gamma2=sd[pre + 'layer_norm.weight'], beta2=sd[pre + 'layer_norm.bias'], h_bf=mode == 'x3', pre_bf=mode == 'x3', npass=npass, seed=SEED)

    def out_and_ffn(tag, pre, pa, ctx, res, res_mod, fuse):
        """fc_o + dropout + residual + LayerNorm, then the FFN block: fused, as two strip launches, or as three block GEMMs"""
        so, sh, sf = new_site(), new_site(), new_site()
        Wo, bo, gam, bet = sd[pa + 'fc_o.weight'], sd[pa + 'fc_o.bias'], sd[pre + 'layer_norm.weight'], sd[pre + 'layer_norm.bias']
        if strip and fuse:
            return emit(tag + '.offn', kind='ffn_fwd', fused=True, A=ctx.float(), W=Wo, bias=bo.reshape(1, -1), act=0, out_scale=1.0, site=so, residual=res.float(),
                        res_mod=res_mod, gamma1=gam, beta1=bet, drop_p=p, site_h=sh, site_o=sf, **ffn_part(tag, pre))['y']
        x1 = lin(tag + '.o', ctx, Wo, bo, site=so, residual=res.float(), res_mod=res_mod, gamma=gam, beta=bet)['C']
        if strip:
            return emit(tag + '.ffn', kind='ffn_fwd', fused=False, x=x1.float(), drop_p=p, site_h=sh, site_o=sf, **ffn_part(tag, pre))['y']
        f = ffn_part(tag, pre)
        h = lin(tag + '.f1', x1, f['W1'], f['b1'], act=1, site=sh)['C']
        return lin(tag + '.f2', h, f['W2'], f['b2'], site=sf, residual=x1.float(), gamma=gam, beta=bet)['C']

    def self_attention(tag, pre, x, n, Lq, H):
        pa = pre + 'self_attention.'
        W = torch.cat([sd[pa + 'fc_%s.weight' % c] for c in 'qkv'])
        b = torch.cat([sd[pa + 'fc_%s.bias' % c] for c in 'qkv'])
        qkv = val(lin(tag + '.qkv', x, W, b, c_planes=strip), strip)
        return attention(tag + '.attn', qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], H, n, Lq, Lq), pa

    def layer(tag, pre, x, n, Lq, H, fuse):
        ctx, pa = self_attention(tag, pre, x, n, Lq, H)
        return out_and_ffn(tag, pre, pa, ctx, x, 0, fuse)

    e_, dd = 'encoder_spec2midi.', 'decoder_spec2midi.'
    win = emit('im2win', kind='im2win', spec=spec.float().reshape(B * F_, -1), B=B, F=F_, T=T, n_proc=cfg.n_proc, Kp=Kp)['win']
    weff, _, beff, _ = BP.embed_fold(sd[e_ + 'conv.weight'], sd[e_ + 'conv.bias'], sd[e_ + 'tok_embedding_freq.weight'], sd[e_ + 'tok_embedding_freq.bias'],
                                     cfg.n_proc, Kp, F64)
    x = lin('embed', win, weff, beff, block=True, out_scale=math.sqrt(d), add_table=sd[e_ + 'pos_embedding_freq.weight'][:F_], add_mod=F_, site=new_site())['C']
    for i in range(cfg.enc_layer):
        x = layer('enc%d' % i, '%slayers_freq.%d.' % (e_, i), x, BT, F_, cfg.enc_head, False)
    enc = x
    H = cfg.dec_head
    pos_dec = sd[dd + 'pos_embedding_freq.weight'][:N]
    cross = [dd + ('layer_zero_freq.' if j == 0 else 'layers_freq.%d.' % (j - 1)) for j in range(cfg.dec_layer)]
    merged = strip and cfg.dec_layer >= 2
    if merged:
        Wkv = torch.cat([sd[c + 'encoder_attention.fc_%s.weight' % n_] for c in cross for n_ in 'kv'])
        bkv = torch.cat([sd[c + 'encoder_attention.fc_%s.bias' % n_] for c in cross for n_ in 'kv'])
        ckv_all = val(lin('dec.kv_all', enc, Wkv, bkv, c_planes=True), True)
    trg = None
    for j, pre in enumerate(cross):
        tag, pa = 'dec%d' % j, pre + 'encoder_attention.'
        if j == 0:
            q = lin(tag + '.q', pos_dec, sd[pa + 'fc_q.weight'], sd[pa + 'fc_q.bias'], block=True)['C']
            if strip:                                 # (hi + lo is the fp32 value to 2^-22: the walk goes on with the value)
                emit(tag + '.q_planes', kind='x3_to_planes', src=q.float())
            res, res_mod = pos_dec, N
        else:
            res, _ = self_attention(tag, pre, trg, BT, N, H)
            res = lin(tag + '.so', res, sd[pre + 'self_attention.fc_o.weight'], sd[pre + 'self_attention.fc_o.bias'], site=new_site(), residual=trg.float(),
                      gamma=sd[pre + 'layer_norm.weight'], beta=sd[pre + 'layer_norm.bias'])['C']
            q = val(lin(tag + '.q', res, sd[pa + 'fc_q.weight'], sd[pa + 'fc_q.bias'], c_planes=strip), strip)
            res_mod = 0
        if merged:
            kv = ckv_all[:, 2 * j * d:2 * (j + 1) * d]
            extra = dict(k_prev=ckv_all[:, 2 * (j - 1) * d:(2 * j - 1) * d].reshape(BT, F_, d), v_prev=ckv_all[:, (2 * j - 1) * d:2 * j * d].reshape(BT, F_, d)) if j else {}
        else:
            W = torch.cat([sd[pa + 'fc_k.weight'], sd[pa + 'fc_v.weight']])
            kv = val(lin(tag + '.kv', enc, W, torch.cat([sd[pa + 'fc_k.bias'], sd[pa + 'fc_v.bias']]), c_planes=strip), strip)
            extra = {}
        ctx = attention(tag + '.cross', q, kv[:, :d], kv[:, d:], H, BT, N, F_, has_probs=j == cfg.dec_layer - 1, **extra)
        trg = out_and_ffn(tag, pre, pa, ctx, res, res_mod, j > 0)
    outs = {}

    def heads(tag, z, side, tm):
        names = ['velocity', 'onset', 'offset', 'mpe']
        W = torch.cat([sd['%sfc_%s_%s.weight' % (dd, n_, side)] for n_ in names])
        b = torch.cat([sd['%sfc_%s_%s.bias' % (dd, n_, side)] for n_ in names])
        logits = lin(tag, z, W, b, block=True)['C']
        outs[side] = emit(tag + '.split', kind='heads_split', logits=logits.float(), B=B, T=T, N=N, V=V, tm=tm)
    heads('heads_f', trg, 'freq', 0)
    y = emit('time_embed', kind='time_embed_fwd', x=trg.float(), pos=sd[dd + 'pos_embedding_time.weight'][:T].float(), shape=(B, T, N, d), scale=math.sqrt(d),
             drop_p=p, site=new_site(), seed=SEED)['y']
    for i in range(cfg.dec_layer):
        y = layer('time%d' % i, '%slayers_time.%d.' % (dd, i), y, BN, T, H, True)
    heads('heads_t', y, 'time', 1)
    lo, lf, lm, lv = labels
    emit('loss', kind='loss', probs=[outs[s][n_].float() for s in ('freq', 'time') for n_ in ('onset', 'offset', 'mpe')],
         vel=[outs[s]['velocity'].float() for s in ('freq', 'time')], lo=lo.float(), lf=lf.float(), lm=lm.float(), lv=lv.long(), n=Sn, V=V)
    _WALKS[key] = recs
    return recs


WALKS = [(name, mode, strip, p) for name in CONFIGS for mode in ('x3', 'parity') for strip in (True, False) for p in (P,)] + [('x3_small', 'x3', True, 0.0)]


def test_every_kind_has_a_contract_a_record_and_every_defect_a_kind():
    recs = model_records('x3_small', 'x3', True, P)
    assert set(FE.KINDS) == set(FE.CONTRACTS) == {r['kind'] for r in recs}
    assert set(FE.DEFECTS) == set(DEFECT_RECORD) and set(FE.DEFECTS_INVISIBLE) <= set(FE.DEFECTS) and len(FE.DEFECTS_INVISIBLE) <= 1
    assert len(FE.DEFECTS) >= 12
    for name, kind in FE.DEFECTS.items():
        assert _defect_record(name)['kind'] == kind, name
    assert any(r.get('fused') for r in recs) and any(r['kind'] == 'ffn_fwd' and not r.get('fused') for r in recs)
    assert {r['kind'] for r in model_records('d128_ff256', 'parity', False, P)} == set(FE.KINDS) - {'strip_linear', 'ffn_fwd', 'x3_to_planes'}


@pytest.mark.parametrize('name,mode,strip,p', WALKS, ids=['%s-%s-%s-p%g' % (n, m, 'strip' if s else 'block', p) for n, m, s, p in WALKS])
def test_the_stand_in_passes_every_check_of_every_launch(name, mode, strip, p):
    by_kind = {}
    for rec in model_records(name, mode, strip, p):
        figs = FE.check(rec, FE.CONTRACTS[rec['kind']](rec, emul=True))
        assert not FE.failures(figs), (rec['tag'], rec['kind'], FE.failures(figs))
        ratio, fig = FE.worst(figs)
        if ratio >= by_kind.get(rec['kind'], (0.0,))[0]:
            by_kind[rec['kind']] = (ratio, rec['tag'], fig)
    print('\n'.join('%-10s %-6s %-14s worst measured / bound %.3g at %s %s' % ((name, mode, k) + v) for k, v in sorted(by_kind.items())))


# the record each defect is planted in: (tag of the launch in the x3_small / x3 / strip walk)
DEFECT_RECORD = {
    'embed_out_scale_dropped': 'embed', 'pos_table_indexed_by_token': 'embed', 'layer0_residual_not_broadcast': 'dec0.o',
    'ln_stats_from_rounded_sum': 'enc0.o', 'hidden_saved_before_dropout': 'enc0.ffn', 'hidden_and_output_sites_swapped': 'enc0.ffn',
    'attn_out_without_keep_scale': 'enc0.attn', 'attention_map_after_dropout': 'dec1.cross', 'shared_query_per_sequence_stride': 'dec0.cross',
    'merged_ckv_previous_layer_block': 'dec1.cross', 'time_embed_scale_dropped': 'time_embed', 'heads_columns_shifted_by_one': 'heads_t.split',
    'fused_launch_saves_ln2_stats_as_ln1': 'time0.offn',
}


def _defect_record(defect):
    (rec,) = [r for r in model_records('x3_small', 'x3', True, P) if r['tag'] == DEFECT_RECORD[defect]]
    return rec


def _size(a, b):
    """the largest change of an output, over that output's maximum"""
    worst = 0.0
    for k, v in b.items():
        if torch.is_tensor(v) and k in a and v.numel():
            va, vb = (L.planes_decode(t) if k == 'dst' else FE.D(t) for t in (a[k], v))
            worst = max(worst, ((va.reshape(-1) - vb.reshape(-1)).abs().max() / (vb.abs().max() + 1e-300)).item())
    return worst


@pytest.mark.parametrize('defect', list(FE.DEFECTS))
def test_planted_defect_fails_at_its_own_kind(defect):
    rec = _defect_record(defect)
    fn = FE.CONTRACTS[rec['kind']]
    good, wrong = fn(rec, emul=True), fn(rec, emul=True, defect=defect)
    figs = FE.check(rec, wrong)
    print('%-38s at %-14s %-12s size %.2e   %s' % (defect, rec['kind'], rec['tag'], _size(wrong, good), ['%s %.2e / %.1e' % f for f in FE.failures(figs)]))
    if defect in FE.DEFECTS_INVISIBLE:
        assert not FE.failures(figs), 'the defect %s has become visible: take it out of DEFECTS_INVISIBLE' % defect
        return
    assert _size(wrong, good) > 0.0, 'the defect changed nothing'
    assert FE.failures(figs), defect
    assert not FE.failures(FE.check(rec, good))


def test_the_derived_statistics_bound_sees_the_rounded_sum_and_passes_the_stand_in():
    """on every LayerNorm record of the walk: the stand-in is inside the per-row bound of mean / rstd, statistics from the bf16 copy are not"""
    n = 0
    for rec in model_records('x3_small', 'x3', True, P):
        if rec['kind'] != 'strip_linear' or rec.get('gamma') is None:
            continue
        assert rec['pre_bf']
        per_row = lambda out: {f[0] for f in FE.failures(FE.check(rec, out))} & {'mean per row', 'rstd per row'}          # noqa: E731
        assert not per_row(FE.strip_linear(rec, emul=True)), rec['tag']
        assert per_row(FE.strip_linear(rec, emul=True, defect='ln_stats_from_rounded_sum')) == {'mean per row', 'rstd per row'}, rec['tag']
        n += 1
    assert n >= 3
