"""The x3 / parity forward plans, launch by launch, against fp64 (test infrastructure, CPU; no GPU import).

The forward twin of tests/bwd_plan_emul.py, whose record / contract / check machinery it reuses (Spans, the weight read-back through the
layout's table entries, _mm, _epilogue, _elem, the figure helpers, the score conditioning).  One fp64 CONTRACT per launch kind of ws['fwd'] /
ws['fwd_inf'] and of the hftt_loss launch behind them, written from include/hftt_hip.h -- never from a kernel.  With emul=True a contract
is the STAND-IN for a correct device: x3_emul.x3mm on fp16 pairs for npass 2, exact fp32 products for parity, summed in fp32, stores rounded
as the descriptor declares.  tests/test_fwd_plan_emul_bound.py shows on the CPU that the stand-in passes every check and that each planted
defect fails at its kind; tests/test_fwd_plan_gpu.py builds the records from the engine's own descriptors while it steps a forward plan.

Bounds, by kind (figures are (name, measured, bound); a figure fails when it is not below its bound).  No tolerance is new:
  im2win                  exact to the bit, padded columns included
  gemm_nt, strip_linear   max |C - ref| / max |ref| below engine_layouts.TOL_X3[2] (forward products) resp. TOL_K[3] (parity); f16-pair
                          planes: the decoded pair, same bound (engine_layouts.check_sl).  LayerNorm forms (check_nt / check_sl): the
                          pre-LayerNorm sum 4e-3 where it is stored as bf16, else the product's bound; C, mean, rstd 1e-4
  ffn_fwd                 engine_layouts.check_offn: hidden and pre-LayerNorm sums 4e-3 (bf16 stores; the product's bound when fp32), x1, y,
                          mean, rstd 1e-4.  The two-descriptor form runs fc_o, dropout, residual, LayerNorm 1, the FFN, LayerNorm 2 from ctx;
                          x1 is checked only where o.C is given
  attn_fwd                engine_layouts.check_attn: out bo, map bp.  p = 0: x3 (2 ptol, ptol) with ptol = 4e-6 + 4e-7 lmax, lmax measured
                          on the launch's own operands; parity (2 TOL_K[3], 2e-6).  With dropout: (1e-4, 2e-5) in both modes.  The map is
                          pre-dropout.  lse has no bound of its own in the suite: it is held through its consumer -- the probabilities
                          rebuilt from the fp64 scores and the device's pair (max, 1 / sum), the header's RAW-score maximum for npass 2, are
                          held to the map bound bp
  x3_to_planes            hi + lo reconstructs the source to 2^-22 per element (the header's figure); the layout: the first 32 halves of a
                          group alone are the source to fp16's 2^-11
  time_embed_fwd          tests/test_elementwise_fp64_gpu.py: per element 3 U32 (|x| sqrt(d) + |pos|) keep-scale on kept elements, zero elsewhere
  heads_split             tests/test_elementwise_fp64_gpu.py: the sigmoid (C_EXP + 1 + C_DIV) U32 of the result + F32_TINY; the velocity logits
                          an exact copy (tests/test_small_kernels_gpu.py holds both to 2e-6)
  loss                    elementwise_emul.loss_ref / loss_check on the device's own nine outputs

The saved tensors -- what only the backward reads, and what the backward plan's check takes on trust -- per element, from a derivation:
  e_prod = tol_of(rec) max |ref| x keep scale (where a dropout mask applies): what the product's own bound allows an element.
  e      = e_prod + 2 U32 |ref|: the keep-scale product and the residual sum round once each in fp32.
  bf16 saves (hidden, pre-LayerNorm sums) and f16-pair planes:  |got - ref| <= u (|ref| + e) + e,  u = UBF (bf16: one rounding of the
      device's fp32 value, which is within e of ref -- hence u e, second order, but a term) resp. 2^-22 (planes) + 2^-24 absolute (the lo
      half's fp16 subnormal spacing).
  hidden: exactly zero where the keep mask drops the element; positive where ref > e (the backward gates on h > 0).
  mean, rstd of a row r_1 .. r_N whose device values carry e_i (any summation order has depth <= N):
      b_mean = mean(e_i) + (N + 1) U32 mean |r_i|                                      (the sum's N roundings and the division)
      b_var  = 2 mean(|r_i - mean| (e_i + b_mean)) + (N + 3) U32 (var + mean^2)       (d var = 2 mean((r_i - mean)(dr_i - dmean)); the
               subtraction, the square, the sum and the division; var + mean^2 = E[r^2]: the header does not say whether the variance
               is summed around the mean or as E[r^2] - mean^2, and the second form rounds at that size)
      b_rstd = rstd^3 b_var / 2 + (1 + C_SQRT + C_DIV) U32 rstd                        (d rstd = -rstd^3 dvar / 2; + eps, sqrt, 1 / x)
  The stand-in passes these; statistics taken from the bf16-rounded sum (ln_stats_from_rounded_sum) do not.
"""
import math
from collections import OrderedDict

import numpy as np
import torch

import attn_drop_emul as AD
import bf16_plan_emul as BP
import bwd_plan_emul as PE
import elementwise_emul as EE
import engine_layouts as L
from bwd_plan_emul import (INPUT_SCALE, Spans, _elem, _epilogue, _mm, _plane_weight, _strip_weight, condition, describe,  # noqa: F401
                           engine_spans, failures, sites_of, worst)
from bwd_plan_emul import BF, D, F64, _wd, f32c, keep, rel_err, tol_of
from util import keep_scale

U32, UBF = EE.U32, EE.UBF
U_PLANES, A_PLANES = 2.0 ** -22, 2.0 ** -24
EPS = 1e-5

KINDS = ('im2win', 'gemm_nt', 'strip_linear', 'ffn_fwd', 'attn_fwd', 'x3_to_planes', 'time_embed_fwd', 'heads_split', 'loss')

# planted defects -> the kind each must fail at (tests/test_fwd_plan_emul_bound.py)
DEFECTS = OrderedDict([
    ('embed_out_scale_dropped', 'gemm_nt'),                 # the folded embedding without its sqrt(d)
    ('pos_table_indexed_by_token', 'gemm_nt'),              # add_mod = M: row r takes table row r, not r % F
    ('layer0_residual_not_broadcast', 'strip_linear'),      # res_mod = M on layer zero's [N, d] residual
    ('ln_stats_from_rounded_sum', 'strip_linear'),          # mean / rstd (and the normalisation) from the bf16 copy of the sum
    ('hidden_saved_before_dropout', 'ffn_fwd'),             # h_out written in front of dropout_h
    ('hidden_and_output_sites_swapped', 'ffn_fwd'),         # site_h <-> site_o
    ('attn_out_without_keep_scale', 'attn_fwd'),            # out = mask(P) V without the 1 / keep
    ('attention_map_after_dropout', 'attn_fwd'),            # probs = dropout(P)
    ('shared_query_per_sequence_stride', 'attn_fwd'),       # q_seq_stride = Lq ldq on the one query block of layer zero
    ('merged_ckv_previous_layer_block', 'attn_fwd'),        # layer j reads column block j - 1 of dec.ckv_all
    ('time_embed_scale_dropped', 'time_embed_fwd'),         # x + pos without the sqrt(d)
    ('heads_columns_shifted_by_one', 'heads_split'),        # onset / offset / mpe from columns V + 1 ..
    ('fused_launch_saves_ln2_stats_as_ln1', 'ffn_fwd'),     # hftt_attn_out_ffn_fwd: o's mean / rstd overwritten with f's
])
# defects no criterion of this file can see, and why (none; the test asserts that a listed one still passes)
DEFECTS_INVISIBLE = {}


def planes_encode(v):
    """values [rows, cols] -> fp32 slots holding f16-pair planes (the inverse of engine_layouts.planes_decode): per 32-column group the 32
    fp16 hi halves, then the 32 lo halves"""
    v = v.double()
    R, C_ = v.shape
    hi = v.half()
    lo = (v - hi.double()).half()
    return torch.cat([hi.reshape(R, C_ // 32, 32), lo.reshape(R, C_ // 32, 32)], -1).reshape(R, 2 * C_).contiguous().view(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------- contracts
def im2win(rec, emul=False, defect=None):
    """hftt_im2win: win[(b, t, f), u] = spec[b, f, t + u], zero for u >= n_proc, row stride Kp"""
    return {'win': BP.im2win(rec['spec'].reshape(rec['B'], rec['F'], -1), rec['T'], rec['n_proc'], rec['Kp'])}


def _layer_norm(v, gamma, beta, stats_from=None):
    src = v if stats_from is None else stats_from
    mean = src.mean(1)
    rstd = 1.0 / torch.sqrt(((src - mean[:, None]) ** 2).mean(1) + EPS)
    return (v - mean[:, None]) * rstd[:, None] * gamma.to(v.dtype).reshape(1, -1) + beta.to(v.dtype).reshape(1, -1), mean, rstd


def _ln_tail(v, rec, emul, defect, sfx=''):
    """the LayerNorm end of the epilogue: pre_ln_out = v; C = LayerNorm(v) gamma + beta (eps 1e-5, over N); mean / rstd per row.
    Returns (C, {pre, mean, rstd}): every tensor the launch may store (the caller keeps the ones its descriptor names)"""
    pre_bf = bool(rec.get('pre_bf'))
    rounded = v.to(BF).to(v.dtype)
    y, mean, rstd = _layer_norm(v, rec['gamma' + sfx], rec['beta' + sfx], rounded if defect == 'ln_stats_from_rounded_sum' else None)
    return y, {'pre' + sfx: v.to(BF) if (emul and pre_bf) else v, 'mean' + sfx: mean, 'rstd' + sfx: rstd}


def _planted(rec, defect):
    """the plan-level defects of the shared epilogue, as the record a wrong descriptor would make"""
    M = rec['A'].shape[0]
    if defect == 'embed_out_scale_dropped':
        return dict(rec, out_scale=1.0)
    if defect == 'pos_table_indexed_by_token':        # rows behind the table read what lies there: zeros in the stand-in
        t = rec['add_table']
        return dict(rec, add_table=torch.cat([t, torch.zeros(M - t.shape[0], t.shape[1], dtype=t.dtype)]), add_mod=M)
    if defect == 'layer0_residual_not_broadcast':
        r = rec['residual']
        return dict(rec, residual=torch.cat([r, torch.zeros(M - r.shape[0], r.shape[1], dtype=r.dtype)]), res_mod=M)
    return rec


def _linear(rec, emul, defect):
    rec = _planted(rec, defect)
    acc = _mm(rec['A'], rec['W'].t(), rec['npass'], emul)
    v = _epilogue(acc, rec, emul)
    if rec.get('gamma') is None:
        return {'C': planes_encode(v) if (emul and rec.get('c_planes')) else v}
    y, saved = _ln_tail(v, rec, emul, defect)
    return dict(saved, C=y)


def gemm_nt(rec, emul=False, defect=None):
    """hftt_gemm_nt, the forward form: bias, act, out_scale, add_table[row % add_mod], dropout, residual[row % res_mod], LayerNorm"""
    return _linear(rec, emul, defect)


def strip_linear(rec, emul=False, defect=None):
    """hftt_strip_linear, the forward forms: the same epilogue; HFTT_SL_C_F16PAIR: C as f16-pair planes; HFTT_SL_PRE_BF16: pre_ln_out bf16"""
    return _linear(rec, emul, defect)


def _ffn_half(x, rec, emul, defect):
    """hftt_ffn_res_ln_fwd: h = dropout_h(relu(x W1^T + b1)); y = LayerNorm(residual + dropout_o(h W2^T + b2)) gamma + beta, residual NULL = x.
    The hidden feeds fc_2 at full width; the stored copy is post-dropout (bf16 with HFTT_SL_H_BF16)"""
    dt = _wd(emul)
    M, p_, d_ = x.shape[0], rec['W1'].shape[0], rec['W2'].shape[0]
    p, seed = rec.get('drop_p', 0.0), rec.get('seed', 0)
    sh, so = (rec['site_o'], rec['site_h']) if defect == 'hidden_and_output_sites_swapped' else (rec['site_h'], rec['site_o'])
    a = torch.relu(_mm(x, rec['W1'].t(), rec['npass'], emul) + rec['b1'].to(dt).reshape(1, -1))
    h = a * PE.scaled_mask(seed, sh, (M, p_), p, dt) if (p > 0.0 and sh) else a
    f = _mm(h, rec['W2'].t(), rec['npass'], emul) + rec['b2'].to(dt).reshape(1, -1)
    if p > 0.0 and so:
        f = f * PE.scaled_mask(seed, so, (M, d_), p, dt)
    r2 = (rec['residual2'].to(dt) if rec.get('residual2') is not None else x.to(dt)) + f
    y, saved = _ln_tail(r2, dict(rec, pre_bf=rec.get('pre_bf')), emul, None, '2')
    hs = a if defect == 'hidden_saved_before_dropout' else h
    return dict(saved, y=y, h=(hs.to(BF) if (emul and rec.get('h_bf')) else hs), _a=a)


def ffn_fwd(rec, emul=False, defect=None):
    """hftt_ffn_res_ln_fwd (one descriptor: x given) and hftt_attn_out_ffn_fwd (two: x1 = LayerNorm(residual + dropout(ctx Wo^T + bo)) first,
    exactly as hftt_strip_linear(o), then the block on x1; results bit-identical to the two launches)"""
    if not rec.get('fused'):
        out = _ffn_half(rec['x'].to(_wd(emul)), rec, emul, defect)
        out.pop('_a')
        return out
    first = _linear(dict(rec, gamma=rec['gamma1'], beta=rec['beta1']), emul, None)
    out = _ffn_half(first['C'], rec, emul, defect)
    out.pop('_a')
    out.update(x1=first['C'], pre1=first['pre'], mean1=first['mean'], rstd1=first['rstd'])
    if defect == 'fused_launch_saves_ln2_stats_as_ln1':
        out['mean1'], out['rstd1'] = out['mean2'], out['rstd2']
    return out


def _attn_operands(rec, defect):
    q, k, v = D(rec['q']), D(rec['k']), D(rec['v'])
    n = k.shape[0]
    if defect == 'merged_ckv_previous_layer_block':
        k, v = D(rec['k_prev']), D(rec['v_prev'])
    if q.shape[0] == 1 and n > 1:
        if defect == 'shared_query_per_sequence_stride':           # sequences behind the first read what lies behind the block: zeros here
            q = torch.cat([q, torch.zeros(n - 1, q.shape[1], q.shape[2], dtype=F64)])
        else:
            q = q.expand(n, q.shape[1], q.shape[2])
    return q, k, v


def _scores(q, k, H):
    """scaled scores [n, H, Lq, Lk] in fp64"""
    n, Lq, w = q.shape
    dh = w // H
    qh = q.reshape(n, Lq, H, dh).transpose(1, 2)
    kh = k.reshape(n, k.shape[1], H, dh).transpose(1, 2)
    return qh @ kh.transpose(-1, -2) / math.sqrt(dh), dh


def attn_fwd(rec, emul=False, defect=None):
    """hftt_attn_fwd: P = softmax(Q K^T / sqrt(dh)); out = dropout(P) V with the keep mask of (drop_p, drop_site, drop_seed), flat index
    ((seq H + head) Lq + q) Lk + k; lse = per row (max score, 1 / sum exp(score - max)) -- npass 2: the max of the RAW Q K^T; probs = P,
    pre-dropout.  q [1, Lq, d] with q_seq_stride 0: one query block shared by all sequences"""
    q, k, v = _attn_operands(rec, defect)
    n, Lq, Lk, H, p = k.shape[0], q.shape[1], k.shape[1], rec['H'], rec.get('drop_p', 0.0)
    mask = keep(rec['seed'], rec['site'], (n, H, Lq, Lk), p) if p > 0.0 else torch.ones(n, H, Lq, Lk, dtype=torch.bool)
    mk = AD.ModelKernel(AD._applied(mask, map_dropped=defect == 'attention_map_after_dropout'), p, H, mode=(rec['mode'] if emul else None))
    if defect == 'attn_out_without_keep_scale':
        mk.ks = 1.0
    out, _, pm = mk.fwd(q, k, v, True)
    s, dh = _scores(q, k, H)
    mx = s.max(-1).values
    inv = 1.0 / torch.exp(s - mx[..., None]).sum(-1)
    raw = rec['mode'] != 'parity'
    lse = torch.stack([mx * math.sqrt(dh) if raw else mx, inv], -1)
    o = {'out': out, 'lse': lse.float() if emul else lse}
    if rec.get('has_probs'):
        o['probs'] = pm.float() if emul else pm
    return o


def x3_to_planes(rec, emul=False, defect=None):
    """hftt_x3_to_planes: fp32 [rows, cols] -> f16-pair planes per 32-column group"""
    return {'dst': planes_encode(rec['src']) if emul else D(rec['src'])}


def time_embed_fwd(rec, emul=False, defect=None):
    """hftt_time_embed_fwd: y[(b, n), t, :] = dropout(x[(b, t), n, :] scale + pos[t, :])"""
    B, T, N, d = rec['shape']
    dt = _wd(emul)
    sc = 1.0 if defect == 'time_embed_scale_dropped' else f32c(rec['scale'])
    xs = rec['x'].to(dt).reshape(B, T, N, d).permute(0, 2, 1, 3).reshape(B * N, T, d) * sc
    pos = rec['pos'].to(dt)[:T].reshape(1, T, d)
    p = rec.get('drop_p', 0.0)
    m = PE.scaled_mask(rec['seed'], rec['site'], (B * N, T, d), p, dt) if p > 0.0 else torch.ones((), dtype=dt)
    return {'y': ((xs + pos) * m).reshape(B * N * T, d), 'mag': ((xs.abs() + pos.abs()) * m).reshape(B * N * T, d)}


def heads_split(rec, emul=False, defect=None):
    """hftt_heads_split: logits [S, ldl], columns [0, V) velocity (raw), V onset, V + 1 offset, V + 2 mpe (sigmoid); time_major: rows are
    (b, n, t), the outputs (b, t, n)"""
    B, T, N, V, tm = rec['B'], rec['T'], rec['N'], rec['V'], rec['tm']
    lg = rec['logits'].to(_wd(emul))
    sh = 1 if defect == 'heads_columns_shifted_by_one' else 0

    def order(t, *tail):
        return (t.reshape(B, N, T, *tail).permute(0, 2, 1, *range(3, 3 + len(tail))) if tm else t.reshape(B, T, N, *tail)).reshape(B * T * N, *tail)
    out = {'velocity': order(lg[:, :V], V)}
    for i, nm in enumerate(('onset', 'offset', 'mpe')):
        c = min(V + i + sh, lg.shape[1] - 1)
        out[nm] = order(torch.sigmoid(lg[:, c]))
    return out


def _loss_case(rec):
    return dict(probs=[t.reshape(-1) for t in rec['probs']], vel=[t.reshape(-1, rec['V']) for t in rec['vel']], lo=rec['lo'].reshape(-1),
                lf=rec['lf'].reshape(-1), lm=rec['lm'].reshape(-1), lv=rec['lv'].reshape(-1), n=rec['n'], V=rec['V'])


def loss(rec, emul=False, defect=None):
    """hftt_loss with the weights elementwise_emul.LOSS_W: loss_out[0 .. 8], d_prob[6], d_vel[2]"""
    if not emul:
        return EE.loss_ref(_loss_case(rec))
    out, dp, dv = EE.loss_emul(_loss_case(rec))
    return dict(out=out, d_prob=dp, d_vel=dv)


CONTRACTS = dict(im2win=im2win, gemm_nt=gemm_nt, strip_linear=strip_linear, ffn_fwd=ffn_fwd, attn_fwd=attn_fwd, x3_to_planes=x3_to_planes,
                 time_embed_fwd=time_embed_fwd, heads_split=heads_split, loss=loss)


# ---------------------------------------------------------------------------------------------------------------------------- checks
def _abs_err(name, got, ref, bound):
    """max |got - ref| against an absolute bound (engine_layouts.max_err: the attention map)"""
    e = D(got).reshape(-1) - D(ref).reshape(-1)
    return (name, float(e.abs().max()) if bool(torch.isfinite(e).all()) else float('inf'), bound)


def _count(name, n):
    """an exact rule as a figure: the number of elements that break it must be zero"""
    return (name, float('inf') if n else 0.0, 1.0)


def e_prod(rec, ref, masked):
    """what the product's own bound allows an element of `ref` (module docstring)"""
    return tol_of(rec) * float(D(ref).abs().max()) * (keep_scale(rec.get('drop_p', 0.0)) if masked else 1.0)


def save_bound(ref, e, u, floor=0.0):
    ref = D(ref)
    return u * (ref.abs() + e) + e + floor


def stats_bound(r, e):
    """(mean, b_mean, rstd, b_rstd) of the rows of r [M, N] whose device values carry the per-element error e (module docstring)"""
    r = D(r)
    e = e if torch.is_tensor(e) else torch.full_like(r, e)
    N = r.shape[1]
    mean = r.mean(1)
    c = r - mean[:, None]
    var = (c * c).mean(1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    b_mean = e.mean(1) + (N + 1) * U32 * r.abs().mean(1)
    b_var = 2.0 * (c.abs() * (e + b_mean[:, None])).mean(1) + (N + 3) * U32 * (var + mean * mean)
    b_rstd = 0.5 * rstd ** 3 * b_var + (1 + EE.C_SQRT + EE.C_DIV) * U32 * rstd
    return mean, b_mean, rstd, b_rstd


def _ln_figs(rec, got, ref, sfx, out_name, masked):
    """the LayerNorm form's figures (check_nt / check_sl / check_offn) and the per-element check of what it saves"""
    pre, figs = 'pre' + sfx, []
    pre_bf = bool(rec.get('pre_bf'))
    if out_name in got:
        figs.append((out_name, rel_err(got[out_name], ref[out_name]), 1e-4))
    if pre in got:
        figs.append((pre, rel_err(got[pre].float(), ref[pre]), 4e-3 if pre_bf else tol_of(rec)))
    for nm in ('mean' + sfx, 'rstd' + sfx):
        if nm in got:
            figs.append((nm, rel_err(got[nm], ref[nm]), 1e-4))
    r = D(ref[pre])
    e = e_prod(rec, r, masked) + 2 * U32 * r.abs()
    if pre in got and pre_bf:
        figs.append(_elem(pre + ' per element', got[pre].float(), r, save_bound(r, e, UBF)))
    mean, b_mean, rstd, b_rstd = stats_bound(r, e)
    if 'mean' + sfx in got:
        figs.append(_elem('mean%s per row' % sfx, got['mean' + sfx], mean, b_mean))
    if 'rstd' + sfx in got:
        figs.append(_elem('rstd%s per row' % sfx, got['rstd' + sfx], rstd, b_rstd))
    return figs


def _hidden_figs(rec, got_h, x):
    """the stored hidden, from the block's own input x (the device's: hftt_attn_out_ffn_fwd is hftt_strip_linear, then hftt_ffn_res_ln_fwd
    on its result, to the bit)"""
    half = _ffn_half(D(x), rec, False, None)
    h, a = D(half['h']), half['_a']
    p = rec.get('drop_p', 0.0)
    masked = p > 0.0 and bool(rec['site_h'])
    e = tol_of(rec) * float(a.abs().max()) * (keep_scale(p) if masked else 1.0)
    g = D(got_h.float())
    figs = [('h', rel_err(g, h), 4e-3 if rec.get('h_bf') else tol_of(rec))]
    if rec.get('h_bf'):
        figs.append(_elem('h per element', g, h, save_bound(h, e + 2 * U32 * h.abs(), UBF)))
    if masked:
        dropped = ~keep(rec['seed'], rec['site_h'], tuple(h.shape), p)
        figs.append(_count('h: non-zero where the mask drops', int(((g != 0) & dropped).sum())))
    figs.append(_count('h: not positive where the hidden is', int(((h > e) & ~(g > 0)).sum())))
    return figs


def attn_lmax(rec):
    q, k, _ = _attn_operands(rec, None)
    return float(_scores(q, k, rec['H'])[0].abs().max())


def attn_bounds(rec):
    """(bo, bp) of engine_layouts.check_attn"""
    p = rec.get('drop_p', 0.0)
    if p > 0.0:
        return 1e-4, 2e-5
    if rec['mode'] == 'parity':
        return 2 * L.TOL_K[3], 2e-6
    ptol = 4e-6 + 4e-7 * attn_lmax(rec)
    return 2 * ptol, ptol


def check(rec, got=None):
    """[(figure, measured, bound)] of one launch record; got: its outputs (default rec['got'])"""
    kind = rec['kind']
    got = rec['got'] if got is None else got
    ref = CONTRACTS[kind](rec)
    if kind == 'im2win':
        g, r = got['win'].float().contiguous(), ref['win'].float().contiguous()
        return [_count('win: elements that differ to the bit', int((g.view(torch.int32) != r.view(torch.int32)).sum()))]
    if kind in ('gemm_nt', 'strip_linear'):
        masked = rec.get('drop_p', 0.0) > 0.0 and bool(rec.get('site'))
        if rec.get('gamma') is not None:
            return _ln_figs(rec, got, ref, '', 'C', masked)
        if rec.get('c_planes'):
            dec, r = L.planes_decode(got['C']), D(ref['C'])
            return [('C', rel_err(dec, r), tol_of(rec)),
                    _elem('C planes per element', dec, r, save_bound(r, e_prod(rec, r, masked) + 2 * U32 * r.abs(), U_PLANES, A_PLANES))]
        figs = [('C', rel_err(got['C'], ref['C']), tol_of(rec))]
        if masked and rec.get('residual') is None:
            dropped = ~keep(rec['seed'], rec['site'], tuple(ref['C'].shape), rec['drop_p'])
            figs.append(_count('C: non-zero where the mask drops', int(((D(got['C']) != 0) & dropped).sum())))
        return figs
    if kind == 'ffn_fwd':
        masked = rec.get('drop_p', 0.0) > 0.0
        figs = []
        x = rec.get('x')
        if rec.get('fused'):
            figs += _ln_figs(dict(rec, gamma=rec['gamma1']), {k: v for k, v in got.items() if k in ('x1', 'pre1', 'mean1', 'rstd1')}, ref, '1', 'x1',
                             masked and bool(rec.get('site')))
            x = got.get('x1')
        figs += _ln_figs(rec, got, ref, '2', 'y', masked and bool(rec['site_o']))
        if 'h' in got:
            figs += _hidden_figs(rec, got['h'], x) if x is not None else [('h', rel_err(got['h'].float(), ref['h']), 4e-3 if rec.get('h_bf') else tol_of(rec))]
        return figs
    if kind == 'attn_fwd':
        bo, bp = attn_bounds(rec)
        figs = [('out', rel_err(got['out'], ref['out']), bo)]
        q, k, _ = _attn_operands(rec, None)
        s, dh = _scores(q, k, rec['H'])
        pr = torch.softmax(s, -1)
        if rec.get('has_probs'):
            figs.append(_abs_err('map', got['probs'], pr, bp))
        lse = D(got['lse']).reshape(s.shape[0], s.shape[1], s.shape[2], 2)
        mx = lse[..., 0] / (math.sqrt(dh) if rec['mode'] != 'parity' else 1.0)
        figs.append(_abs_err('lse (the map it rebuilds)', torch.exp(s - mx[..., None]) * lse[..., 1:2], pr, bp))
        return figs
    if kind == 'x3_to_planes':
        src = D(rec['src'])
        h = got['dst'].contiguous().view(torch.float16).reshape(src.shape[0], src.shape[1] // 32, 64)
        hi = h[..., :32].double().reshape(src.shape)
        return [_elem('hi + lo', L.planes_decode(got['dst']), src, U_PLANES * src.abs() + A_PLANES),
                _elem('hi halves first', hi, src, 2.0 ** -11 * src.abs() + A_PLANES)]
    if kind == 'time_embed_fwd':
        return [_elem('y', got['y'], ref['y'], 3 * U32 * ref['mag'])]
    if kind == 'heads_split':
        figs = [_count('velocity: elements that are no exact copy', int((D(got['velocity']).reshape(-1) != D(ref['velocity']).reshape(-1)).sum()))]
        for nm in ('onset', 'offset', 'mpe'):
            r = D(ref[nm])
            figs.append(_elem(nm, got[nm], r, (EE.C_EXP + 1 + EE.C_DIV) * U32 * r + EE.F32_TINY))
        return figs
    if kind == 'loss':
        figs = [_elem('loss_out', got['out'], ref['out'], ref['b_out'])]
        for i in range(6):
            figs.append(_elem('d_prob[%d]' % i, got['d_prob'][i], ref['d_prob'][i], ref['b_dprob'][i]))
        for i in range(2):
            figs.append(_elem('d_vel[%d]' % i, got['d_vel'][i], ref['d_vel'][i], ref['b_dvel'][i]))
        return figs + PE._from_violations('loss_check', EE.loss_check(got['out'], got['d_prob'], got['d_vel'], ref))
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------------------- descriptors -> records
SL_RELU, SL_H_BF16, SL_PRE_BF16, SL_C_F16PAIR, SL_X3_F16 = 8, 64, 128, 512, 16
ATTN_PLANES = 32 | 64


def _descs(entry):
    return [a._obj for a in entry[1] if hasattr(a, '_obj')] if not isinstance(entry[0], str) else []


def _ln_out(d, M, N, pre_bf, sfx, Oo):
    if d.pre_ln_out: Oo['pre' + sfx] = (d.pre_ln_out, M, N, N, pre_bf)
    if d.ln_mean: Oo['mean' + sfx] = (d.ln_mean, 1, M, M, False)
    if d.ln_rstd: Oo['rstd' + sfx] = (d.ln_rstd, 1, M, M, False)


def launch_io(entry, eng, ws):
    """(inputs, outputs) of one forward plan entry: {name: (address, rows, cols, ld, stored as bf16)}; the dtype each descriptor flag
    declares is asserted against the tensor when the block is fetched"""
    fn, args, name, meta = entry
    ds = _descs(entry)
    d = ds[0] if ds else None
    B, T, F_, N, V, dm = ws['B'], eng.T, eng.F, eng.N, eng.V, eng.d
    Sn = B * T * N
    I, Oo = {}, {}
    if name == 'im2win':
        win, B_, F2, T2, n_proc, Kp = args
        I['spec'] = (ws['spec_ptr'], B_ * F2, eng.W, eng.W, False)
        Oo['win'] = (win, B_ * T2 * F2, Kp, Kp, False)
    elif name == 'gemm_nt':
        assert not (d.io_flags & 31), 'bf16 storage or a gradient operand in an x3 / parity forward plan'
        I['A'] = (d.A, d.M, d.K, d.lda, False)
        if d.add_table: I['add_table'] = (d.add_table, d.add_mod, d.N, d.N, False)
        if d.residual: I['residual'] = (d.residual, d.res_mod or d.M, d.N, d.ldr, False)
        if d.ln_gamma:
            I['gamma'], I['beta'] = (d.ln_gamma, 1, d.N, d.N, False), (d.ln_beta, 1, d.N, d.N, False)
            _ln_out(d, d.M, d.N, False, '', Oo)
        Oo['C'] = (d.C, d.M, d.N, d.ldc, False)
    elif name == 'strip_linear':
        assert d.flags & SL_X3_F16 and not d.gate, 'a backward form in a forward plan'
        I['A'] = (d.x, d.M, d.K, d.ldx, False)
        if d.residual: I['residual'] = (d.residual, d.res_mod or d.M, d.N, d.ldr, False)
        if d.ln_gamma:
            I['gamma'], I['beta'] = (d.ln_gamma, 1, d.N, d.N, False), (d.ln_beta, 1, d.N, d.N, False)
            _ln_out(d, d.M, d.N, bool(d.flags & SL_PRE_BF16), '', Oo)
        Oo['C'] = (d.C, d.M, d.N, d.ldc, False)
    elif name == 'ffn_fwd':
        f = ds[-1]
        assert f.mode == 0 and f.flags & SL_X3_F16
        if len(ds) == 2:
            o = ds[0]
            assert o.M == f.M and o.N == f.d and f.w == o.w + 2 * 2 * o.N * o.K and (not o.C or o.C == f.x) and not f.residual
            I['A'] = (o.x, o.M, o.K, o.ldx, False)
            I['residual'] = (o.residual, o.res_mod or o.M, o.N, o.ldr, False)
            I['gamma1'], I['beta1'] = (o.ln_gamma, 1, o.N, o.N, False), (o.ln_beta, 1, o.N, o.N, False)
            if o.C: Oo['x1'] = (o.C, o.M, o.N, o.ldc, False)
            _ln_out(o, o.M, o.N, bool(o.flags & SL_PRE_BF16), '1', Oo)
        else:
            I['x'] = (f.x, f.M, f.d, f.ldx, False)
            if f.residual: I['residual2'] = (f.residual, f.M, f.d, f.ldr, False)
        I['gamma2'], I['beta2'] = (f.ln_gamma, 1, f.d, f.d, False), (f.ln_beta, 1, f.d, f.d, False)
        I['b1'], I['b2'] = (f.b1, 1, f.p, f.p, False), (f.b2, 1, f.d, f.d, False)
        Oo['y'] = (f.y, f.M, f.d, f.ldy, False)
        if f.h_out: Oo['h'] = (f.h_out, f.M, f.p, f.ldh, bool(f.flags & SL_H_BF16))
        _ln_out(f, f.M, f.d, bool(f.flags & SL_PRE_BF16), '2', Oo)
    elif name == 'attn_fwd':
        w = d.n_heads * d.dh
        assert d.q_seq_stride in (0, d.Lq * d.ldq) and d.k_seq_stride == d.Lk * d.ldk and d.v_seq_stride == d.Lk * d.ldv and d.o_seq_stride == d.Lq * d.ldo
        assert not (d.io_flags & 31)
        I['q'] = (d.q, (1 if d.q_seq_stride == 0 else d.n_seq) * d.Lq, w, d.ldq, False)
        I['k'] = (d.k, d.n_seq * d.Lk, w, d.ldk, False)
        I['v'] = (d.v, d.n_seq * d.Lk, w, d.ldv, False)
        Oo['out'] = (d.out, d.n_seq * d.Lq, w, d.ldo, False)
        n_rows = d.n_seq * d.n_heads * d.Lq
        Oo['lse'] = (d.lse, 1, n_rows * 2, n_rows * 2, False)
        if d.probs: Oo['probs'] = (d.probs, 1, n_rows * d.Lk, n_rows * d.Lk, False)
    elif name == 'x3_to_planes':
        src, lds, dst, ldd, rows, cols = args
        I['src'] = (src, rows, cols, lds, False)
        Oo['dst'] = (dst, rows, cols, ldd, False)
    elif name == 'time_embed_fwd':
        x, pos, y, site, iof = args
        assert iof == 0
        I['x'], I['pos'] = (x, Sn, dm, dm, False), (pos, T, dm, dm, False)
        Oo['y'] = (y, Sn, dm, dm, False)
    elif name == 'heads_split':
        logits, tm = args
        I['logits'] = (logits, Sn, eng.NH, eng.NHp, False)
        o = ws['outs'][5:9] if tm else ws['outs'][0:4]
        for t, nm in zip(o[:3], ('onset', 'offset', 'mpe')):
            Oo[nm] = (t.data_ptr(), 1, Sn, Sn, False)
        Oo['velocity'] = (o[3].data_ptr(), Sn, V, V, False)
    else:
        raise AssertionError('a launch kind the forward harness does not know: %s' % name)
    return I, Oo


def _param(eng, name):
    o = eng.poff[name]
    shape = eng.pshape[name]
    return eng.flat_params.detach().cpu().double()[o:o + int(np.prod(shape))].reshape(shape)


def embed_fold(eng):
    """(Weff [d, Kp], beff [d]) in fp64: the fold of conv.weight, conv.bias, tok_embedding_freq.weight and .bias (bf16_plan_emul.embed_fold)"""
    e = 'encoder_spec2midi.'
    weff, _, beff, _ = BP.embed_fold(_param(eng, e + 'conv.weight'), _param(eng, e + 'conv.bias'), _param(eng, e + 'tok_embedding_freq.weight'),
                                     _param(eng, e + 'tok_embedding_freq.bias'), eng.n_proc, eng.Kp, F64)
    return weff, beff


def _vector(eng, addr, n):
    """fp64 values of the vector [n] at device address `addr`: a parameter, or a region of the prepared vector plane rebuilt from
    flat_params through the layout's entries (the folded embedding's bias: from the fold)"""
    P = eng.flat_params
    lo = P.data_ptr()
    if lo <= addr < lo + 4 * P.numel():
        o = (addr - lo) // 4
        return P.detach().cpu().double()[o:o + n].reshape(1, n)
    lay = eng.layout
    off = (addr - eng.fprep.data_ptr()) // 4
    assert 0 <= off < eng.fprep.numel() and (addr - eng.fprep.data_ptr()) % 4 == 0, 'vector address %#x is neither a parameter nor prepared' % addr
    if off == lay.Woff['embed_b']:
        return embed_fold(eng)[1].reshape(1, n)
    Pc = P.detach().cpu().double()
    v, hit = torch.zeros(n, dtype=F64), 0
    for so, do, rows, cols, sld, dld, kind in lay.prep:
        if kind == 2 and off <= do < off + n:
            v[do - off:do - off + cols] = Pc[so:so + cols]
            hit += 1
    assert hit, 'no vector entry of the layout writes %#x' % addr
    return v.reshape(1, n)


def _nt_weight(eng, addr, N, K):
    lay = eng.layout
    base, esz = (eng.whi.data_ptr(), 2) if eng.npass == 2 else (eng.wf32.data_ptr(), 4)
    if (addr - base) // esz == lay.Woff['embed']:
        return 'embed', embed_fold(eng)[0][:N, :K].clone()
    return _plane_weight(eng, addr, N, K)


def make_record(entry, arrays, prior, eng, ws):
    """the launch record of one forward plan entry from its descriptor(s) and the captured arrays"""
    fn, args, name, meta = entry
    ds = _descs(entry)
    d = ds[0] if ds else None
    B, T, F_, N, V, dm = ws['B'], eng.T, eng.F, eng.N, eng.V, eng.d
    rec = dict(kind=name, prior=prior, **arrays)
    mode = 'parity' if eng.npass == 3 else 'x3'
    if name == 'im2win':
        rec.update(B=args[1], F=args[2], T=args[3], n_proc=args[4], Kp=args[5])
    elif name == 'gemm_nt':
        rec['wkey'], rec['W'] = _nt_weight(eng, d.W, d.N, d.K)
        assert d.npass == eng.npass and not d.gate
        rec.update(npass=d.npass, act=d.act, out_scale=d.out_scale, add_mod=d.add_mod, drop_p=d.drop_p, site=d.drop_site, seed=d.drop_seed, res_mod=d.res_mod,
                   bias=_vector(eng, d.bias, d.N) if d.bias else None)
    elif name == 'strip_linear':
        rec['wkey'], (rec['W'],) = _strip_weight(eng, d.w, [(d.N, d.K)])
        rec.update(npass=2, act=1 if d.flags & SL_RELU else 0, out_scale=d.out_scale, drop_p=d.drop_p, site=d.drop_site, seed=d.drop_seed, res_mod=d.res_mod,
                   bias=_vector(eng, d.bias, d.N) if d.bias else None, c_planes=bool(d.flags & SL_C_F16PAIR), pre_bf=bool(d.flags & SL_PRE_BF16))
    elif name == 'ffn_fwd':
        f = ds[-1]
        rec['wkey'], (rec['W1'], rec['W2']) = _strip_weight(eng, f.w, [(f.p, f.d), (f.d, f.p)])
        rec.update(npass=2, drop_p=f.drop_p, site_h=f.site_h, site_o=f.site_o, seed=f.drop_seed, h_bf=bool(f.flags & SL_H_BF16), pre_bf=bool(f.flags & SL_PRE_BF16),
                   fused=len(ds) == 2)
        if len(ds) == 2:
            o = ds[0]
            rec['wkey'], (rec['W'],) = _strip_weight(eng, o.w, [(o.N, o.K)])
            assert o.drop_p == f.drop_p and o.drop_seed == f.drop_seed and bool(o.flags & SL_PRE_BF16) == rec['pre_bf'] and not (o.flags & (SL_RELU | SL_C_F16PAIR))
            rec.update(out_scale=o.out_scale, site=o.drop_site, res_mod=o.res_mod, bias=_vector(eng, o.bias, o.N) if o.bias else None, act=0)
    elif name == 'attn_fwd':
        w, planes = d.n_heads * d.dh, bool(d.io_flags & 32)
        assert bool(d.io_flags & 64) == planes and d.npass == eng.npass
        dec = L.planes_decode if planes else (lambda t: t)
        for k_, L_ in (('q', d.Lq), ('k', d.Lk), ('v', d.Lk)):
            rec[k_] = dec(rec[k_]).reshape(-1, L_, w)
        rec.update(H=d.n_heads, drop_p=d.drop_p, site=d.drop_site, seed=d.drop_seed, planes=planes, mode=mode, has_probs=bool(d.probs),
                   shape=(d.n_seq, d.n_heads, d.Lq, d.Lk))
    elif name == 'time_embed_fwd':
        rec.update(shape=(B, T, N, dm), scale=math.sqrt(dm), drop_p=ws['p'], site=args[3], seed=ws['seed'])
    elif name == 'heads_split':
        rec.update(B=B, T=T, N=N, V=V, tm=args[1])
    return rec


def step_plan(eng, ws, plan, launch, spans):
    """bwd_plan_emul.step_plan for a forward plan: yields (index, entry, record, {input: block}, {output: block}, figures), block = (tensor
    name, first element, rows, cols, row stride)"""
    for i, entry in enumerate(plan):
        I, Oo = launch_io(entry, eng, ws)
        arrays = {k: spans.fetch(*v) for k, v in I.items()}
        prior = {k: spans.fetch(*v) for k, v in Oo.items()}
        rec = make_record(entry, arrays, prior, eng, ws)
        launch(i, entry)
        rec['got'] = {k: spans.fetch(*v) for k, v in Oo.items()}
        blocks = [{k: spans.where(v[0], v[1], v[2], v[3])[:2] + (v[1], v[2], v[3]) for k, v in io.items()} for io in (I, Oo)]
        yield i, entry, rec, blocks[0], blocks[1], check(rec)


# ---------------------------------------------------------------------------------------------------------------------------- the plan's own scalars
class PlanRules:
    """The link check reads a launch's scalars from its descriptor, so a descriptor that is wrong in itself would be held to its own
    mistake.  These rules say what the descriptors of a forward plan must carry from the GRAPH -- which weight a launch multiplies with
    (read back through the layout: rec['wkey']) and which buffer it writes name the layer:
      * the dropout sites are unique per launch and cover 1 .. eng._site; every descriptor of ws['drop'] carries the step's p and seed, and so
        does every descriptor of the plan that names a site (a site _patch does not reach would run at the p it was built with);
      * the inference plan names no pre_ln_out, statistics or h_out, and runs with drop_p = 0;
      * out_scale = sqrt(d) is on the embedding alone, with add_mod = F on the encoder's position table; no other launch adds a table;
      * res_mod = N is on layer zero's attention output alone, whose residual is the decoder's position table;
      * q_seq_stride = 0 is on layer zero's attention alone, whose query is what the 'dec0.ca.q' product (or its plane copy) wrote;
      * a cross attention of layer j reads K at column block j of dec.ckv_all (ldk = Ld 2d) or at its own dec<j>.ckv, V one d behind."""

    def __init__(self, eng, ws, plan, inference):
        self.eng, self.ws, self.plan, self.inference = eng, ws, plan, inference
        self.producer = {}
        self.seen = {'embed': 0, 'layer0_out': 0, 'layer0_attn': 0, 'cross': 0}

    def static(self):
        eng, ws, bad = self.eng, self.ws, []
        per_launch = [set(sites_of(e, True)) for e in self.plan]
        flat = [s for ss in per_launch for s in ss]
        if len(flat) != len(set(flat)):
            bad.append('two launches share a dropout site: %s' % sorted(s for s in set(flat) if flat.count(s) > 1))
        if set(flat) != set(range(1, eng._site + 1)):
            bad.append('the sites %s are not 1 .. %d' % (sorted(set(flat)), eng._site))
        for dsc in ws['drop']:
            if f32c(dsc.drop_p) != f32c(ws['p']) or dsc.drop_seed != ws['seed']:
                bad.append('a descriptor of ws[drop] carries p %g seed %d, the step has %g / %d' % (dsc.drop_p, dsc.drop_seed, ws['p'], ws['seed']))
        for i, e in enumerate(self.plan):                # which sites _patch reaches: every descriptor of the plan that names a site
            for dsc in _descs(e):
                named = [s for s in (getattr(dsc, 'drop_site', 0), getattr(dsc, 'site_h', 0), getattr(dsc, 'site_o', 0)) if s]
                if named and (f32c(dsc.drop_p) != f32c(ws['p']) or dsc.drop_seed != ws['seed']):
                    bad.append('plan[%d] %s names site %s and carries p %g seed %d, the step has %g / %d: _patch does not reach it' % (
                        i, e[2], named, dsc.drop_p, dsc.drop_seed, ws['p'], ws['seed']))
        if self.inference:
            if ws['p'] != 0.0:
                bad.append('the inference plan runs with p = %g' % ws['p'])
            for i, e in enumerate(self.plan):
                for dsc in _descs(e):
                    if getattr(dsc, 'pre_ln_out', 0) or getattr(dsc, 'ln_mean', 0) or getattr(dsc, 'ln_rstd', 0) or (hasattr(dsc, 'h_out') and dsc.h_out):
                        bad.append('plan[%d] %s of the inference plan names a saved tensor' % (i, e[2]))
        return bad

    def check(self, i, entry, rec, ins, outs):
        fn, args, name, meta = entry
        eng, ws, bad = self.eng, self.ws, []
        ds = _descs(entry)
        pos_dec = eng.poff['decoder_spec2midi.pos_embedding_freq.weight']
        if name in ('gemm_nt', 'strip_linear', 'ffn_fwd'):
            o = ds[0]
            wkey = rec['wkey']
            if hasattr(o, 'out_scale'):
                embed = wkey == 'embed'
                want = f32c(math.sqrt(eng.d)) if embed else 1.0
                if f32c(o.out_scale) != want:
                    bad.append('out_scale %g on %s, the graph has %g' % (o.out_scale, wkey, want))
                if name == 'gemm_nt':
                    if embed:
                        self.seen['embed'] += 1
                        if o.add_mod != eng.F or ins.get('add_table', (None,))[:2] != ('flat_params', eng.poff['encoder_spec2midi.pos_embedding_freq.weight']):
                            bad.append('the embedding adds table %s with add_mod %d; the graph has the encoder\'s position table and F = %d' % (
                                ins.get('add_table'), o.add_mod, eng.F))
                    elif o.add_table:
                        bad.append('a position table on %s' % wkey)
                layer0 = wkey == 'dec0.ca.o'
                M = o.M
                if layer0:
                    self.seen['layer0_out'] += 1
                    if o.res_mod != eng.N or ins['residual'][:2] != ('flat_params', pos_dec):
                        bad.append('layer zero\'s residual is %s with res_mod %d; the graph has the decoder\'s position table, N = %d' % (ins['residual'], o.res_mod, eng.N))
                elif o.residual and (o.res_mod or M) != M:
                    bad.append('res_mod %d on %s' % (o.res_mod, wkey))
        elif name == 'attn_fwd':
            d = ds[0]
            oname = outs['out'][0]
            if oname.endswith('.cctx'):
                self.seen['cross'] += 1
                j = int(oname[3:-5])
                kname, koff = ins['k'][:2]
                vname, voff = ins['v'][:2]
                merged = 'dec.ckv_all' in ws['bufs']
                want = ('dec.ckv_all', j * 2 * eng.d, eng.Ld * 2 * eng.d) if merged else ('dec%d.ckv' % j, 0, 2 * eng.d)
                if (kname, koff, d.ldk) != want or (vname, voff, d.ldv) != (want[0], want[1] + eng.d, want[2]):
                    bad.append('layer %d reads K at %s+%d (ld %d), V at %s+%d; the graph has %s+%d (ld %d), V one d behind' % (
                        j, kname, koff, d.ldk, vname, voff, want[0], want[1], want[2]))
                src = self.producer.get(ins['q'][:2])
                if j == 0:
                    self.seen['layer0_attn'] += 1
                    if d.q_seq_stride != 0:
                        bad.append('layer zero\'s query has sequence stride %d' % d.q_seq_stride)
                    if src is None or src[1] not in ('gemm_nt', 'x3_to_planes'):
                        bad.append('layer zero\'s query is what %s wrote' % (src,))
                elif d.q_seq_stride == 0:
                    bad.append('q_seq_stride 0 on layer %d' % j)
            elif d.q_seq_stride == 0:
                bad.append('q_seq_stride 0 on the self attention %s' % oname)
            if bool(d.probs) != (oname == 'dec%d.cctx' % (eng.Ld - 1)):
                bad.append('the attention map is written by %s; the graph returns the last cross attention\'s' % oname)
        elif name == 'x3_to_planes':
            src = self.producer.get(ins['src'][:2])
            if src is None or src[1] != 'gemm_nt' or src[3] != 'dec0.ca.q':
                bad.append('converts what %s wrote, not layer zero\'s query' % (src,))
        elif name == 'time_embed_fwd':
            if args[3] != ws['sites']['time_embed'] or ins['pos'][:2] != ('flat_params', eng.poff['decoder_spec2midi.pos_embedding_time.weight']):
                bad.append('site %d / table %s; the graph has site %d and the time position table' % (args[3], ins['pos'], ws['sites']['time_embed']))
        for out, w in outs.items():
            self.producer[w[:2]] = (i, name, out, rec.get('wkey'))
        return bad

    def finish(self):
        want = {'embed': 1, 'layer0_out': 1, 'layer0_attn': 1, 'cross': self.eng.Ld}
        return ['%s: met %d times, the graph has %d' % (k, self.seen[k], v) for k, v in want.items() if self.seen[k] != v]
