"""The x3 / parity training backward, launch by launch, against fp64 (test infrastructure, CPU; no GPU import).

A LAUNCH RECORD is a plain dict: 'kind', the scalar fields of the launch, its operand arrays (CPU tensors in their storage dtype), 'prior' (what
the outputs held before the launch: read where the launch accumulates or writes in place) and, once it ran, 'got' (its outputs).  One fp64
CONTRACT function per launch kind of ws['bwd'] / ws['bwd_dec'], written from include/hftt_hip.h -- never from a kernel --, and one CHECK per
kind that holds 'got' to the contract under the bound that kind's kernel test already carries (the table below: no tolerance is new).
With emul=True a contract runs as the STAND-IN for a correct device: the same operations summed in fp32 on x3's operand splits
(x3_emul.x3mm; exact fp32 products in the parity mode), stores rounded as the descriptor declares them.  tests/test_bwd_plan_emul_bound.py shows
on the CPU that the stand-in passes every check and that each planted defect fails at its kind; tests/test_bwd_plan_gpu.py builds the records
from the engine's own descriptors (`launch_io`, `make_record`) while it steps a backward plan one entry at a time.

Bounds, by kind (figures are (name, measured, bound); a figure fails when it is not below its bound):
  gemm_nt, strip_linear   max |C - ref| / max |ref| below engine_layouts.TOL_X3[npass] (2: forward products, 4: a gradient operand) resp. TOL_K[3]
  gemm_tn                 every segment's dW the same way; db: max error over out_scale sqrt(M) max|dY| below 1e-5 -- engine_layouts.check_tn's
                          figure for gradient-sized operands (its parity form is the same expression on unit-variance operands; db is a
                          plain fp32 column sum in every mode).  db is out_scale times a sum, so its error carries that factor (check_tn runs
                          at 0.5 and 1; the embedding product at sqrt(d)).  The scale stands on the terms, not on db: the fc_k bias gradients
                          are zero in exact arithmetic.  DY_HI: the same bounds against the product of bf16(dY), as
                          tests/test_x3_gpu.py::test_gemm_tn
  ffn_bwd_dx              engine_layouts.check_ffn: dh 4e-3 (a bf16 store; TOL_X3[4] when the hidden is fp32), dx 6e-5
  attn_bwd                engine_layouts.check_attn: bg = 3e-4 with dropout, 2e-4 + 3 (4e-6 + 4e-7 lmax) without, + 4e-5 on f16-pair planes;
                          parity: 2e-4 resp. 4 TOL_K[3]
  ln_bwd, ln_bwd_reduce, colsum, time_embed_bwd     the elementwise_emul criteria (per element, first-order rounding models)
  dropout_bwd_colsum      the masked gradient: one rounding per kept element, exact zeros elsewhere (elementwise_emul.te_bwd_ref's dym rule);
                          the column sum: elementwise_emul.colsum_ref over the device's own masked values
  heads_split_bwd         tests/test_small_kernels_gpu.py: 2e-6 (there absolute on unit-sized operands: here of the output's maximum), padding
                          columns exactly zero
  embed_fold_bwd          tests/test_small_kernels_gpu.py: 2e-5 of each of the four gradients' maximum
"""
import math
from collections import OrderedDict

import numpy as np
import torch

import attn_drop_emul as AD
import elementwise_emul as EE
import engine_layouts as L
import util
from util import keep_mask_t, keep_scale
from x3_emul import x3mm

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U32 = EE.U32

KINDS = ('gemm_nt', 'strip_linear', 'ffn_bwd_dx', 'gemm_tn', 'attn_bwd', 'ln_bwd', 'ln_bwd_reduce', 'heads_split_bwd', 'time_embed_bwd', 'colsum',
         'dropout_bwd_colsum', 'embed_fold_bwd')

# planted defects -> the kind each must fail at (tests/test_bwd_plan_emul_bound.py)
DEFECTS = OrderedDict([
    ('gate_scale_left_at_1', 'ffn_bwd_dx'),                 # the run-time 1 / keep of the hidden dropout never patched into the dX launch
    ('dy_drop_mask_ignored', 'gemm_tn'),                    # HFTT_TN_DY_DROP set, dY summed unmasked
    ('beta0_on_accumulating_segment', 'gemm_tn'),           # a segment that must accumulate overwrites
    ('seg_row0_off_by_one', 'gemm_tn'),                     # the second segment starts one row of dY^T late
    ('k_out_columns_from_k', 'gemm_tn'),                    # the destination walked with leading dimension K instead of K_out
    ('out_scale_sqrt_d_dropped', 'gemm_tn'),                # the embedding product without its sqrt(d)
    ('dx_residual_dropped', 'strip_linear'),                # a dX launch without the LayerNorm backward's dr
    ('delta_without_dropout_mask', 'attn_bwd'),             # delta = rowsum(dO * O) from an O formed without the keep mask
    ('time_embed_bwd_overwrites', 'time_embed_bwd'),        # accumulate = 0
    ('pos_colsum_reads_unmasked', 'colsum'),                # the position table's gradient summed from the gradient in front of the dropout
    ('ln_dr_drop_wrong_site', 'ln_bwd'),                    # the masked copy made with the neighbouring site's decisions
    ('heads_sigmoid_from_logits', 'heads_split_bwd'),       # s (1 - s) with s = sigmoid(input): the stored posteriors taken for logits
])
# defects no criterion of this file can see, and why (none today; the test asserts that a listed one still passes)
DEFECTS_INVISIBLE = {}


def f32c(x):
    return float(np.float32(x))


def D(t):
    return t.detach().cpu().to(F64)


def rel_err(a, b):
    b = D(b)
    a = D(a).reshape(b.shape)
    if not bool(torch.isfinite(a).all()):
        return float('inf')
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


_MASKS = {}


def keep(seed, site, shape, p):
    """bool keep mask of a dropout site (util.keep_mask_t), cached: the consumers of one site ask for the same decisions"""
    key = (int(seed), int(site), tuple(int(s) for s in shape), float(p))
    if key not in _MASKS:
        if len(_MASKS) > 6:
            _MASKS.pop(next(iter(_MASKS)))
        _MASKS[key] = keep_mask_t(int(seed), int(site), key[2], float(p))
    return _MASKS[key]


def scaled_mask(seed, site, shape, p, dtype):
    return keep(seed, site, shape, p).to(dtype) * keep_scale(p)


def _mm(a, b, npass, emul, a_hi=False, b_hi=False):
    """a @ b: fp64, or (emul) as the matrix cores run it -- npass 2: fp16 pairs, 4: bf16 pairs (a_hi / b_hi: that operand is its hi half alone),
    3: fp32 products; summed in fp32"""
    if not emul:
        return D(a) @ D(b)
    a, b = a.float(), b.float()
    if npass == 3:
        return a @ b
    return x3mm(a, b, 'f16' if npass == 2 else 'bf16', a_hi=a_hi, b_hi=b_hi)


def _store(v, like, emul):
    """the stand-in's store: rounded to the dtype the descriptor declares"""
    return v.to(like).float() if (emul and like == BF) else v


def _wd(emul):
    return F32 if emul else F64


# ---------------------------------------------------------------------------------------------------------------------------- contracts
def _epilogue(acc, rec, emul, defect=None):
    """include/hftt_hip.h, hftt_gemm_nt: bias, act, out_scale, add_table, gate, dropout, residual -- in this order"""
    dt = _wd(emul)
    M, N = acc.shape
    rows = torch.arange(M)
    v = acc
    if rec.get('bias') is not None:
        v = v + rec['bias'].to(dt).reshape(1, N)
    if rec.get('act'):
        v = torch.relu(v)
    v = v * f32c(rec.get('out_scale', 1.0))
    if rec.get('add_table') is not None:
        v = v + rec['add_table'].to(dt)[rows % rec['add_mod']]
    if rec.get('gate') is not None:
        v = torch.where(rec['gate'].to(dt) > 0, v * f32c(rec['gate_scale']), torch.zeros((), dtype=dt))
    if rec.get('drop_p', 0.0) > 0.0 and not rec.get('x_drop'):
        v = v * scaled_mask(rec['seed'], rec['site'], (M, N), rec['drop_p'], dt)
    if rec.get('residual') is not None and defect != 'dx_residual_dropped':
        res = rec['residual'].to(dt)
        v = v + res[rows % (rec.get('res_mod') or M)]
    return v


def gemm_nt(rec, emul=False, defect=None):
    acc = _mm(rec['A'], rec['W'].t(), rec['npass'], emul, a_hi=bool(rec.get('a_hi')))
    return {'C': _epilogue(acc, rec, emul, defect)}


def strip_linear(rec, emul=False, defect=None):
    """hftt_strip_linear: the same epilogue; HFTT_SL_X_DROP: x is the gradient of a dropout output [M, K] and is masked while it is loaded"""
    x = rec['A'].to(_wd(emul))
    if rec.get('x_drop') and rec.get('drop_p', 0.0) > 0.0:
        x = x * scaled_mask(rec['seed'], rec['site'], tuple(x.shape), rec['drop_p'], x.dtype)
    acc = _mm(x, rec['W'].t(), rec['npass'], emul, a_hi=bool(rec.get('a_hi')))
    return {'C': _epilogue(acc, rec, emul, defect)}


def ffn_bwd_dx(rec, emul=False, defect=None):
    """hftt_ffn_bwd_dx: dh = gate(h) * (dy W2) * gate_scale, dx = dh W1 + residual; dy masked through site_o when drop_p > 0.
    W_a = fc_2.weight^T [p, d], W_b = fc_1.weight^T [d, p] (the two logical matrices of the interleaved stream)"""
    dt = _wd(emul)
    dy = rec['x'].to(dt)
    if rec.get('drop_p', 0.0) > 0.0 and rec.get('site_o'):
        dy = dy * scaled_mask(rec['seed'], rec['site_o'], tuple(dy.shape), rec['drop_p'], dt)
    t = _mm(dy, rec['W_a'].t(), 4, emul)
    gs = 1.0 if defect == 'gate_scale_left_at_1' else f32c(rec['gate_scale'])
    dh = torch.where(rec['gate'].to(dt) > 0, t * gs, torch.zeros((), dtype=dt))
    dx = _mm(dh, rec['W_b'].t(), 4, emul)                 # (the hidden's gradient feeds fc_1's dX from registers at full width)
    if rec.get('residual') is not None:
        dx = dx + rec['residual'].to(dt)
    return {'dh': _store(dh, BF if rec['h_bf'] else F32, emul), 'dx': dx}


def gemm_tn(rec, emul=False, defect=None):
    """hftt_gemm_tn: dW[seg] = out_scale dY[:, row0 : row0 + rows]^T X[:, :K_out] (+ beta prior), db[seg] = out_scale colsum(dY[:, rows]) (+ beta
    prior); HFTT_TN_DY_DROP: dY masked with its site (element m N + n) while it is loaded; HFTT_TN_DY_HI: dY enters the product as bf16(dY)"""
    dt = _wd(emul)
    dY, X = rec['dY'].to(dt), rec['X'].to(dt)
    M, N = dY.shape
    K, K_out = X.shape[1], rec['K_out']
    if rec.get('dy_drop') and rec.get('drop_p', 0.0) > 0.0 and defect != 'dy_drop_mask_ignored':
        dY = dY * scaled_mask(rec['seed'], rec['site'], (M, N), rec['drop_p'], dt)
    dYp = dY.to(BF).to(dt) if rec.get('dy_hi') else dY
    sc = 1.0 if defect == 'out_scale_sqrt_d_dropped' else f32c(rec.get('out_scale', 1.0))
    beta = f32c(rec.get('beta', 0.0))
    out = {}
    for i, (r0, rows) in enumerate(rec['segs']):
        if defect == 'seg_row0_off_by_one' and i == len(rec['segs']) - 1:
            r0 = min(r0 + 1, N - rows)
        full = _mm(dYp[:, r0:r0 + rows].t(), X, rec['npass'], emul, a_hi=bool(rec.get('dy_hi') or rec['dY'].dtype == BF), b_hi=rec['X'].dtype == BF) * sc
        dw = full.reshape(-1)[:rows * K_out].reshape(rows, K_out) if defect == 'k_out_columns_from_k' else full[:, :K_out]
        db = dY[:, r0:r0 + rows].sum(0) * sc
        if beta != 0.0 and not (defect == 'beta0_on_accumulating_segment' and i == 0):
            dw = dw + beta * rec['prior']['dw%d' % i].to(dt)
            if rec['has_db'][i]:
                db = db + beta * rec['prior']['db%d' % i].to(dt).reshape(-1)
        out['dw%d' % i] = dw
        if rec['has_db'][i]:
            out['db%d' % i] = db
    return out


def attn_bwd(rec, emul=False, defect=None):
    """hftt_attn_bwd: P = softmax(Q K^T / sqrt(dh)) from q, k in fp64; the keep mask of (drop_p, drop_site, drop_seed), flat index
    ((seq H + head) Lq + q) Lk + k; dQ (per sequence), dK, dV of sum(out * dout).  q [n or 1, Lq, d]: one query block shared by all sequences.
    The stand-in is attn_drop_emul.ModelKernel with the mode's operand roundings."""
    q, k, v, do = (D(rec[n]) for n in ('q', 'k', 'v', 'dout'))
    n, Lq, Lk, H, p = k.shape[0], q.shape[1], k.shape[1], rec['H'], rec.get('drop_p', 0.0)
    mask = keep(rec['seed'], rec['site'], (n, H, Lq, Lk), p) if p > 0.0 else torch.ones(n, H, Lq, Lk, dtype=torch.bool)
    mk = AD.ModelKernel(AD._applied(mask), p, H, mode=(rec['mode'] if emul else None))
    _, st, _ = mk.fwd(q, k, v, False)
    if defect == 'delta_without_dropout_mask':
        clean = AD.ModelKernel(AD._applied(torch.ones_like(mask)), 0.0, H, mode=rec['mode'])
        st = st[:4] + (clean.fwd(q, k, v, False)[0],)
    dq, dk, dv = mk.bwd(st, do)
    return {'dq': dq, 'dk': dk, 'dv': dv}


def attn_lmax(rec):
    q, k = D(rec['q']), D(rec['k'])
    H = rec['H']
    dh = q.shape[-1] // H
    qh = q.reshape(q.shape[0], q.shape[1], H, dh).transpose(1, 2)
    kh = k.reshape(k.shape[0], k.shape[1], H, dh).transpose(1, 2)
    return float((qh @ kh.transpose(-1, -2)).abs().max()) / math.sqrt(dh)


def _ln_case(rec):
    return dict(dy=rec['dy'].float(), r=rec['r'].float(), mean=rec['mean'].float().reshape(-1), rstd=rec['rstd'].float().reshape(-1),
                gamma=rec['gamma'].float().reshape(-1))


def _ln_mask(rec, site_shift=0):
    p = rec.get('drop_p', 0.0)
    if not (p > 0.0 and rec.get('has_drop')):
        return None
    return keep(rec['seed'], rec['site'] + site_shift, tuple(rec['dy'].shape), p)


def ln_bwd(rec, emul=False, defect=None):
    """hftt_ln_bwd: dr, the dropout-masked copy dr_drop (when the descriptor names one), the dgamma / dbeta partials.  fp64:
    elementwise_emul.ln_bwd_ref (with the magnitudes its bound needs); stand-in: ln_bwd_emul, its sums as ONE workspace row"""
    c = _ln_case(rec)
    p = rec.get('drop_p', 0.0)
    if not emul:
        return EE.ln_bwd_ref(c, _ln_mask(rec), p)
    mask = _ln_mask(rec, 1 if defect == 'ln_dr_drop_wrong_site' else 0)
    o = EE.ln_bwd_emul(c, R=2, dr_bf=False, drop=('bf16' if rec.get('drop_bf') else 'f32') if mask is not None else None, mask=mask, p=p)
    out = {'dr': o['dr'], 'ws': torch.cat([o['dg'], o['db']]).reshape(1, -1)}
    if 'drd' in o:
        out['dr_drop'] = o['drd']
    return out


def ln_bwd_reduce(rec, emul=False, defect=None):
    """hftt_ln_bwd_reduce: out[c] = beta out[c] + sum_w ws[w][c], ws [n_wg, 2 N]: dgamma partials, then dbeta partials"""
    N, beta = rec['N'], f32c(rec['beta'])
    ws = rec['ws'].to(_wd(emul))
    prior = torch.cat([rec['prior']['dg'].reshape(-1), rec['prior']['db'].reshape(-1)]).to(ws.dtype) if beta != 0.0 else torch.zeros(2 * N, dtype=ws.dtype)
    if emul:
        s = prior * beta + ws.sum(0)
        return {'dg': s[:N], 'db': s[N:]}
    ref, bound = EE.ln_reduce_bound(ws, prior, beta)
    return {'dg': ref[:N], 'db': ref[N:], 'bound': bound}


def heads_split_bwd(rec, emul=False, defect=None):
    """hftt_heads_split_bwd: dlogits[row, :V] = d_velocity, [row, V + i] = d_prob_i p_i (1 - p_i) from the stored posteriors, the padding columns
    zero; time_major: the outputs are (b, t, n), the logits' rows (b, n, t)"""
    dt = _wd(emul)
    B, T, N, V, ldl, tm = rec['B'], rec['T'], rec['N'], rec['V'], rec['ldl'], rec['tm']
    S = B * T * N

    def rows(t, *tail):
        t = t.to(dt).reshape(B, T, N, *tail)
        return (t.permute(0, 2, 1, *range(3, 3 + len(tail))) if tm else t).reshape(S, *tail)
    out = torch.zeros(S, ldl, dtype=dt)
    out[:, :V] = rows(rec['d_vel'], V)
    for i in range(3):
        p_ = rows(rec['prob'][i])
        if defect == 'heads_sigmoid_from_logits':
            p_ = torch.sigmoid(p_)
        out[:, V + i] = rows(rec['d_prob'][i]) * (p_ * (1.0 - p_))
    return {'dlog': out}


def _te_case(rec):
    B, T, N, d = rec['shape']
    return dict(dy=rec['dy'].float().reshape(B * N, T, d), dx0=rec['prior']['dx'].float().reshape(B * T, N, d), shape=rec['shape'], scale=rec['scale'])


def _te_mask(rec):
    B, T, N, d = rec['shape']
    p = rec.get('drop_p', 0.0)
    return keep(rec['seed'], rec['site'], (B * N, T, d), p) if p > 0.0 else None


def time_embed_bwd(rec, emul=False, defect=None):
    """hftt_time_embed_bwd with accumulate = 1: dx[(b, t), n] += mask dy[(b, n), t] scale; dym = the masked dy"""
    c, mask, p = _te_case(rec), _te_mask(rec), rec.get('drop_p', 0.0)
    if not emul:
        return EE.te_bwd_ref(c, mask, p, False)
    dx, dym = EE.te_bwd_emul(c, mask, p, False, defect='accumulate_overwrites' if defect == 'time_embed_bwd_overwrites' else None)
    out = {'dx': dx}
    if rec.get('has_dym'):
        out['dym'] = dym
    return out


def _cs_case(rec, x=None):
    x = rec['x'] if x is None else x
    prior = rec['prior']['out'].float().reshape(-1)
    if f32c(rec['beta']) == 0.0:
        prior = torch.zeros_like(prior)                  # (not read: may be anything, NaN included)
    return dict(x=x.float(), out0=prior, rows=x.shape[0], n=x.shape[1])


def colsum(rec, emul=False, defect=None):
    """hftt_colsum: out[j] = beta out[j] + sum_r x[r ld + j]"""
    beta = f32c(rec['beta'])
    if emul:
        return {'out': EE.colsum_emul(_cs_case(rec, rec['x_unmasked'] if defect == 'pos_colsum_reads_unmasked' else None), beta)}
    ref, bound = EE.colsum_ref(_cs_case(rec), beta)
    return {'out': ref, 'bound': bound}


def dropout_bwd_colsum(rec, emul=False, defect=None):
    """hftt_dropout_bwd_colsum: g masked in place (the decision of element r ld + j), out = beta out + colsum(masked g)"""
    dt = _wd(emul)
    g0 = rec['prior']['g'].to(dt)
    rows, n = g0.shape
    p = rec.get('drop_p', 0.0)
    g = g0 * scaled_mask(rec['seed'], rec['site'], (rows, rec['ld']), p, dt)[:, :n] if p > 0.0 else g0
    if emul:
        return {'g': g, 'out': EE.colsum_emul(_cs_case(rec, g), f32c(rec['beta']))}
    return {'g': g}


def embed_fold_bwd(rec, emul=False, defect=None):
    """hftt_embed_fold_bwd: (dWeff [d, Kp], dbeff [d]) -> the gradients of conv.weight, conv.bias, tok_embedding_freq.weight and .bias through
    Weff[j, u] = sum_{c, kk, w + kk = u} Wtok[j, c nw + w] wconv[c, kk], beff[j] = btok[j] + sum_c bconv[c] sum_w Wtok[j, c nw + w]"""
    dt = _wd(emul)
    wconv, bconv, wtok, btok = (rec[k].to(dt).clone().requires_grad_(True) for k in ('wconv', 'bconv', 'wtok', 'btok'))
    C_, kk = wconv.shape
    n_proc = rec['n_proc']
    nw = n_proc - (kk - 1)
    d = wtok.shape[0]
    tw3 = wtok.view(d, C_, nw)
    weff = sum(torch.nn.functional.pad(tw3[:, c, :] * wconv[c, t], (t, kk - 1 - t)) for c in range(C_) for t in range(kk))
    beff = btok + (tw3 * bconv.view(1, C_, 1)).sum((1, 2))
    ((weff * rec['dweff'].to(dt)[:, :n_proc]).sum() + (beff * rec['dbeff'].to(dt).reshape(-1)).sum()).backward()
    return {'g_wconv': wconv.grad, 'g_bconv': bconv.grad, 'g_wtok': wtok.grad, 'g_btok': btok.grad}


CONTRACTS = dict(gemm_nt=gemm_nt, strip_linear=strip_linear, ffn_bwd_dx=ffn_bwd_dx, gemm_tn=gemm_tn, attn_bwd=attn_bwd, ln_bwd=ln_bwd,
                 ln_bwd_reduce=ln_bwd_reduce, heads_split_bwd=heads_split_bwd, time_embed_bwd=time_embed_bwd, colsum=colsum,
                 dropout_bwd_colsum=dropout_bwd_colsum, embed_fold_bwd=embed_fold_bwd)


# ---------------------------------------------------------------------------------------------------------------------------- checks
def _elem(name, got, ref, bound):
    """per-element criterion as one figure: the largest |got - ref| / bound (0 / 0 counts as 0, a NaN or an error on a zero bound as inf)"""
    got, ref, bound = D(got).reshape(-1), D(ref).reshape(-1), D(bound).reshape(-1)
    err = (got - ref).abs()
    ratio = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, float('inf')))
    ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(err), ratio)
    return (name, float(ratio.max()) if ratio.numel() else 0.0, 1.0)


def _from_violations(name, bad):
    return [(name + ' ' + b[0], float('inf'), 1.0) for b in bad]


def tol_of(rec):
    return L.TOL_K[3] if rec['npass'] == 3 else L.TOL_X3[rec['npass']]


def check(rec, got=None):
    """[(figure, measured, bound)] of one launch record; got: its outputs (default rec['got'])"""
    kind = rec['kind']
    got = rec['got'] if got is None else got
    ref = CONTRACTS[kind](rec)
    if kind in ('gemm_nt', 'strip_linear'):
        return [('C', rel_err(got['C'], ref['C']), tol_of(rec))]
    if kind == 'ffn_bwd_dx':
        return [('dh', rel_err(got['dh'], ref['dh']), 4e-3 if rec['h_bf'] else L.TOL_X3[4]), ('dx', rel_err(got['dx'], ref['dx']), 6e-5)]
    if kind == 'gemm_tn':
        dY = D(rec['dY'])
        figs = []
        for i, (r0, rows) in enumerate(rec['segs']):
            figs.append(('dw%d' % i, rel_err(got['dw%d' % i], ref['dw%d' % i]), tol_of(rec)))
            if rec['has_db'][i]:
                scale = abs(f32c(rec.get('out_scale', 1.0))) * math.sqrt(dY.shape[0]) * float(dY.abs().max()) + 1e-300
                e = D(got['db%d' % i]).reshape(-1) - ref['db%d' % i]
                figs.append(('db%d' % i, float(e.abs().max()) / scale if bool(torch.isfinite(e).all()) else float('inf'), 1e-5))
        return figs
    if kind == 'attn_bwd':
        p, lmax = rec.get('drop_p', 0.0), attn_lmax(rec)
        ptol = 4e-6 + 4e-7 * lmax
        if rec['mode'] == 'parity':
            bg = 4 * L.TOL_K[3] if p == 0 else 2e-4
        else:
            bg = (2e-4 + 3 * ptol if p == 0 else 3e-4) + (4e-5 if rec.get('planes') else 0.0)
        return [(n, rel_err(got[n], ref[n]), bg) for n in ('dq', 'dk', 'dv')]
    if kind == 'ln_bwd':
        mask, p = _ln_mask(rec), rec.get('drop_p', 0.0)
        N = rec['dy'].shape[1]
        ws = D(got['ws'])
        g = dict(dr=got['dr'], dg=ws[:, :N].sum(0), db=ws[:, N:].sum(0))
        drop = None
        if mask is not None:
            g['drd'], drop = got['dr_drop'], ('bf16' if rec.get('drop_bf') else 'f32')
        b = EE.K_DR * U32 * ref['dr_scale']
        figs = [_elem('dr', g['dr'], ref['dr'], b), _elem('dgamma', g['dg'], ref['dg'], EE.K_DG * U32 * ref['dg_scale']),
                _elem('dbeta', g['db'], ref['db'], EE.K_DB * U32 * ref['db_scale'])]
        if drop is not None:
            bd = (b * keep_scale(p) + U32 * ref['drd'].abs()) * mask.double()
            figs.append(_elem('dr_drop', g['drd'], ref['drd'], bd * (1 + EE.UBF) + EE.UBF * ref['drd'].abs() if drop == 'bf16' else bd))
        # the verdict is elementwise_emul.ln_bwd_check's own; the figures above restate its bounds for the report
        return figs + _from_violations('ln_bwd_check', EE.ln_bwd_check(g, ref, False, drop, mask, p))
    if kind == 'ln_bwd_reduce':
        N = rec['N']
        return [_elem('dgamma', got['dg'], ref['dg'], ref['bound'][:N]), _elem('dbeta', got['db'], ref['db'], ref['bound'][N:])]
    if kind == 'heads_split_bwd':
        V = rec['V']
        pad = D(got['dlog'])[:, V + 3:]
        return [('dlog', rel_err(D(got['dlog'])[:, :V + 3], ref['dlog'][:, :V + 3]), 2e-6),
                ('padding', float(pad.abs().max()) if bool(torch.isfinite(pad).all()) else float('inf'), 1e-300)]
    if kind == 'time_embed_bwd':
        figs = [_elem('dx', D(got['dx']).reshape(ref['dx'].shape), ref['dx'], ref['b_dx'])]
        if rec.get('has_dym'):
            figs.append(_elem('dym', D(got['dym']).reshape(ref['dym'].shape), ref['dym'], ref['b_dym']))
        return figs + _from_violations('te_bwd_check', EE.te_bwd_check(D(got['dx']).reshape(ref['dx'].shape),
                                                                      D(got['dym']).reshape(ref['dym'].shape) if rec.get('has_dym') else None, ref))
    if kind == 'colsum':
        return [_elem('out', got['out'], ref['out'], ref['bound'])]
    if kind == 'dropout_bwd_colsum':
        r2, b2 = EE.colsum_ref(_cs_case(rec, got['g']), f32c(rec['beta']))
        return [_elem('g', got['g'], ref['g'], U32 * ref['g'].abs()), _elem('out', got['out'], r2, b2)]
    if kind == 'embed_fold_bwd':
        return [(n, rel_err(got[n], ref[n]), 2e-5) for n in ('g_wconv', 'g_bconv', 'g_wtok', 'g_btok')]
    raise KeyError(kind)


def failures(figs):
    return [f for f in figs if not f[1] < f[2]]


def worst(figs):
    """(measured / bound, figure name) of the figure nearest its bound"""
    return max(((f[1] / f[2] if f[2] > 0 else (0.0 if f[1] == 0 else float('inf'))), f[0]) for f in figs)


# ---------------------------------------------------------------------------------------------------------------------------- conditioning
def attn_table_lmax():
    """The largest |scaled score| the ATTN_CASES of engine_layouts.py reach on their x3 operands (build_attn's generator, restated): the
    conditioning up to which the fixed attention bands with dropout were calibrated"""
    worst_ = 0.0
    for c in L.ATTN_CASES.values():
        if 'x3' not in c['modes']:
            continue
        H, Lq, Lk, dh = c['H'], c['Lq'], c['Lk'], c['dh']
        d, n = H * dh, L.ATTN_N
        g = torch.Generator().manual_seed(Lq * 1000 + Lk + dh)
        nq = 1 if c['lay'] == 'shared' else n
        q, k = torch.randn(nq * Lq, d, generator=g), torch.randn(n * Lk, d, generator=g)
        worst_ = max(worst_, attn_lmax(dict(q=q.reshape(nq, Lq, d), k=k.reshape(n, Lk, d), H=H)))
    return worst_


def model_lmax(sd, x, cfg, seed, p):
    """{attention's parameter prefix: largest |scaled score|} of one training forward, in the fp64 model on the CPU (oracle graph, the
    device's masks for `seed`), in launch order"""
    from util import O
    from x3_emul import _Proxy
    found = OrderedDict()
    cur, site = [None], [0]

    def softmax(t, dim):
        found[cur[0]] = float(t.detach().abs().max())
        return torch.softmax(t, dim)

    def drop(t, pp, training):
        if not (training and pp > 0.0):
            return t
        site[0] += 1
        return t * keep_mask_t(seed, site[0], tuple(t.shape), pp).to(t.dtype) * keep_scale(pp)
    mha_ = O.mha

    def mha(sd_, pre, *a, **kw):
        cur[0] = pre
        return mha_(sd_, pre, *a, **kw)
    T_, d_ = O.torch, O._drop
    O.torch, O._drop, O.mha = _Proxy(torch, softmax=softmax), drop, mha
    try:
        with torch.no_grad():
            O.model_forward({k: v.double() for k, v in sd.items()}, x.double(), cfg, p=p, training=True)
    finally:
        O.torch, O._drop, O.mha = T_, d_, mha_
    return found


INPUT_SCALE = 0.02          # of util.O.synth_spec's log-mel range
LMAX_TARGET = 0.8           # an attention beyond the table's reach is brought to this share of it


def condition(sd, x, cfg, seed, p, table=None):
    """Bring every attention of the training forward inside the conditioning the fixed attention bands were calibrated on.  The input scale
    alone cannot: the first encoder layer reads sqrt(d) x the token embedding + the position table (largest |score| 40 at a vanishing input)
    and the first time layer sqrt(d) x a LayerNorm output (1200 .. 1600 at any input).  Scores are linear in fc_q, so an attention whose
    largest |score| in the fp64 model exceeds the table's gets its fc_q weight and bias scaled by LMAX_TARGET table / lmax -- repeated until
    every attention is inside (an earlier layer's scale moves the later ones a little).  Changes `sd` in place; returns
    ({prefix: lmax}, {prefix: factor}, table lmax)."""
    table = attn_table_lmax() if table is None else table
    factors = {}
    for _ in range(6):
        lm = model_lmax(sd, x, cfg, seed, p)
        over = {k: v for k, v in lm.items() if v > table}
        if not over:
            return lm, factors, table
        for pre, v in over.items():
            f = LMAX_TARGET * table / v
            for what in ('weight', 'bias'):
                sd[pre + 'fc_q.' + what].mul_(f)
            factors[pre] = factors.get(pre, 1.0) * f
    raise AssertionError('conditioning did not converge: %s' % lm)


# ---------------------------------------------------------------------------------------------------------------------------- descriptors -> records
class Spans:
    """device address -> named tensor.  fetch / store move a [rows, cols] block with row stride ld (elements of the tensor's dtype)"""

    def __init__(self):
        self.items = []

    def add(self, name, t):
        assert t.is_contiguous(), name
        self.items.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name, t))

    def find(self, addr):
        hit = [(lo, name, t) for lo, hi, name, t in self.items if lo <= addr < hi]
        assert len({h[1] for h in hit}) == 1, 'address %#x resolves to %s' % (addr, [h[1] for h in hit] or 'nothing')
        lo, name, t = hit[0]
        assert (addr - lo) % t.element_size() == 0, (name, addr - lo)
        return name, t, (addr - lo) // t.element_size()

    def _view(self, addr, rows, cols, ld, bf16):
        name, t, off = self.find(addr)
        if bf16 is not None:
            assert (t.dtype == BF) == bool(bf16), '%s is %s, the descriptor says %s' % (name, t.dtype, 'bf16' if bf16 else 'fp32')
        need = (rows - 1) * ld + cols
        flat = t.reshape(-1)
        assert off + need <= flat.numel(), '%s: [%d, %d] ld %d at element %d passes the end (%d)' % (name, rows, cols, ld, off, flat.numel())
        seg = flat[off:off + need]
        return name, off, torch.as_strided(seg, (rows, cols), (ld, 1), seg.storage_offset())

    def fetch(self, addr, rows, cols, ld=None, bf16=None):
        return self._view(addr, rows, cols, ld or cols, bf16)[2].detach().cpu().clone()

    def store(self, addr, rows, cols, ld, value):
        v = self._view(addr, rows, cols, ld or cols, None)[2]
        v.copy_(value.reshape(rows, cols).to(v.dtype))

    def where(self, addr, rows, cols, ld=None):
        """(tensor name, first element, row stride) of a block"""
        name, off, _ = self._view(addr, rows, cols, ld or cols, None)
        return name, off, ld or cols


def engine_spans(eng, ws):
    sp = Spans()
    for k, t in ws['bufs'].items():
        sp.add(k, t)
    for n, t in zip(util.OUT_NAMES, ws['outs']):
        sp.add(n, t)
    sp.add('flat_params', eng.flat_params)
    sp.add('flat_grads', eng.flat_grads)
    sp.add('dweff', eng.dweff)
    sp.add('dbeff', eng.dbeff)
    return sp


def _plane_weight(eng, addr, N, K):
    """fp32 value of the prepared matrix [N, K] at device address `addr`, from flat_params through the layout's prep entries"""
    lay = eng.layout
    base, esz = (eng.whi.data_ptr(), 2) if eng.npass == 2 else (eng.wf32.data_ptr(), 4)
    off = (addr - base) // esz
    keys = [k for k, o in lay.wl.items.items() if o == off]
    assert (addr - base) % esz == 0 and len(keys) == 1, 'weight address %#x is no region of the matrix planes' % addr
    key = keys[0]
    plane = torch.zeros(lay.wl.sizes[key], dtype=F64)
    P = eng.flat_params.detach().cpu().double()
    n = 0
    for (so, do, rows, cols, sld, dld, kind), k in zip(lay.prep, lay.prep_keys):
        if k != key:
            continue
        src = P[so:so + rows * sld].reshape(rows, sld)[:, :cols]
        r, c = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
        idx = (do - off) + (r * dld + c if kind == 0 else c * dld + r)
        plane[idx.reshape(-1)] = src.reshape(-1)
        n += 1
    assert n, key
    return key, plane[:(plane.numel() // K) * K].reshape(-1, K)[:N].clone()


def _strip_weight(eng, addr, shapes):
    """fp32 values of the logical matrices Wl[N, K] of the strip-pack stream at `addr` (shapes: [(N, K)], in stream order), from flat_params
    through the layout's strip-pack entries: Wl[n0 + r][k0 + c] = src[r][c], transposed entries Wl[n0 + c][k0 + r]"""
    lay = eng.layout
    off = (addr - eng.wstrip.data_ptr()) // 2
    keys = [k for k, o in lay.sl.items.items() if o == off]
    assert len(keys) == 1, 'weight address %#x is no strip-pack stream' % addr
    key = keys[0]
    P = eng.flat_params.detach().cpu().double()
    entries = [e for es, ks in ((lay.spack, lay.spack_keys), (lay.spack_t, lay.spack_t_keys)) for e, k in zip(es, ks) if k == key]
    offsets = sorted({e[11] for e in entries})
    assert len(offsets) == len(shapes), (key, offsets, shapes)
    mats = []
    for o, (N, K) in zip(offsets, shapes):
        Wl = torch.zeros(N, K, dtype=F64)
        for (so, base, rows, cols, sld, tr, n0, k0, Ktot, order, stride, offset) in entries:
            if offset != o:
                continue
            assert Ktot == K, (key, Ktot, K)
            src = P[so:so + rows * sld].reshape(rows, sld)[:, :cols]
            if tr:
                Wl[n0:n0 + cols, k0:k0 + rows] = src.t()
            else:
                Wl[n0:n0 + rows, k0:k0 + cols] = src
        mats.append(Wl)
    return key, mats


def _dsc(entry):
    a = entry[1]
    return a[0]._obj if (a and hasattr(a[0], '_obj')) else None


SL_X3_BF16, SL_X3_GRAD_HI, SL_H_BF16, SL_X_DROP, SL_RELU, SL_C_F16PAIR = 32, 256, 64, 2048, 8, 512


def launch_io(entry, eng, ws):
    """(inputs, outputs) of one plan entry: {name: (address, rows, cols, ld, stored as bf16 or None)}.  The prior contents of every output are
    captured too (the caller fetches the outputs before and after the launch)."""
    fn, args, name, meta = entry
    d = _dsc(entry)
    B, T, N, V, dm = ws['B'], eng.T, eng.N, eng.V, eng.d
    Sn = B * T * N
    I, Oo = {}, {}
    if name == 'gemm_nt':
        assert not d.ln_gamma, 'a LayerNorm epilogue in a backward plan'
        I['A'] = (d.A, d.M, d.K, d.lda, bool(d.io_flags & 1))
        if d.bias: I['bias'] = (d.bias, 1, d.N, d.N, False)
        if d.add_table: I['add_table'] = (d.add_table, d.add_mod, d.N, d.N, False)
        if d.gate: I['gate'] = (d.gate, d.M, d.N, d.ldg, bool(d.io_flags & 4))
        if d.residual: I['residual'] = (d.residual, d.res_mod or d.M, d.N, d.ldr, bool(d.io_flags & 8))
        Oo['C'] = (d.C, d.M, d.N, d.ldc, bool(d.io_flags & 2))
    elif name == 'strip_linear':
        assert not d.ln_gamma and not (d.flags & SL_C_F16PAIR), 'a forward form in a backward plan'
        I['A'] = (d.x, d.M, d.K, d.ldx, False)
        if d.bias: I['bias'] = (d.bias, 1, d.N, d.N, False)
        if d.gate: I['gate'] = (d.gate, d.M, d.N, d.ldg, True)
        if d.residual: I['residual'] = (d.residual, d.res_mod or d.M, d.N, d.ldr, False)
        Oo['C'] = (d.C, d.M, d.N, d.ldc, False)
    elif name == 'ffn_bwd_dx':
        hb = bool(d.flags & SL_H_BF16)
        I['x'] = (d.x, d.M, d.d, d.ldx, False)
        I['gate'] = (d.gate, d.M, d.p, d.ldg, hb)
        if d.residual: I['residual'] = (d.residual, d.M, d.d, d.ldr, False)
        Oo['dx'] = (d.y, d.M, d.d, d.ldy, False)
        Oo['dh'] = (d.h_out, d.M, d.p, d.ldh, hb)
    elif name == 'gemm_tn':
        I['dY'] = (d.dY, d.M, d.N, d.lddy, bool(d.io_flags & 1))
        I['X'] = (d.X, d.M, d.K, d.ldx, bool(d.io_flags & 2))
        for i in range(d.n_seg):
            Oo['dw%d' % i] = (d.seg_dw[i], d.seg_rows[i], d.K_out, d.K_out, False)
            if d.seg_db[i]:
                Oo['db%d' % i] = (d.seg_db[i], 1, d.seg_rows[i], d.seg_rows[i], False)
    elif name == 'attn_bwd':
        w = d.n_heads * d.dh
        assert d.q_seq_stride in (0, d.Lq * d.ldq) and d.k_seq_stride == d.Lk * d.ldk and d.v_seq_stride == d.Lk * d.ldv and d.o_seq_stride == d.Lq * d.ldo
        assert d.dq_seq_stride == d.Lq * d.lddq and d.dk_seq_stride == d.Lk * d.lddk and d.dv_seq_stride == d.Lk * d.lddv
        I['q'] = (d.q, (1 if d.q_seq_stride == 0 else d.n_seq) * d.Lq, w, d.ldq, False)
        I['k'] = (d.k, d.n_seq * d.Lk, w, d.ldk, False)
        I['v'] = (d.v, d.n_seq * d.Lk, w, d.ldv, False)
        I['dout'] = (d.dout, d.n_seq * d.Lq, w, d.ldo, False)
        Oo['dq'] = (d.dq, d.n_seq * d.Lq, w, d.lddq, False)
        Oo['dk'] = (d.dk, d.n_seq * d.Lk, w, d.lddk, False)
        Oo['dv'] = (d.dv, d.n_seq * d.Lk, w, d.lddv, False)
    elif name == 'ln_bwd':
        I['dy'] = (d.dy, d.M, d.N, d.N, bool(d.io_flags & 1))
        I['r'] = (d.r, d.M, d.N, d.N, bool(d.io_flags & 4))
        I['mean'] = (d.mean, 1, d.M, d.M, False)
        I['rstd'] = (d.rstd, 1, d.M, d.M, False)
        I['gamma'] = (d.gamma, 1, d.N, d.N, False)
        Oo['dr'] = (d.dr, d.M, d.N, d.N, bool(d.io_flags & 2))
        if d.dr_drop:
            Oo['dr_drop'] = (d.dr_drop, d.M, d.N, d.N, bool(d.drop_bf16))
        Oo['ws'] = (d.ws, eng.lib.hftt_ln_bwd_wgs(d.M), 2 * d.N, 2 * d.N, False)
    elif name == 'ln_bwd_reduce':
        n_wg, n, dg, db, beta = args
        I['ws'] = (ws['ln_ws_ptr'], n_wg, 2 * n, 2 * n, False)
        Oo['dg'] = (dg, 1, n, n, False)
        Oo['db'] = (db, 1, n, n, False)
    elif name == 'heads_split_bwd':
        side, dlog, tm = args
        b = ws['bufs']
        outs = ws['outs'][5:8] if tm else ws['outs'][0:3]
        for i, (t, nm) in enumerate(zip(outs, ('onset', 'offset', 'mpe'))):
            I['prob%d' % i] = (t.data_ptr(), 1, Sn, Sn, False)
            I['d_prob%d' % i] = (b['d.%s_%s' % (nm, side)].data_ptr(), 1, Sn, Sn, False)
        I['d_vel'] = (b['d.velocity_' + side].data_ptr(), Sn, V, V, False)
        Oo['dlog'] = (dlog, Sn, eng.NHp, eng.NHp, False)
    elif name == 'time_embed_bwd':
        dy, dx, dym, site, iof = args
        assert iof == 0
        I['dy'] = (dy, Sn, dm, dm, False)
        Oo['dx'] = (dx, Sn, dm, dm, False)
        if dym:
            Oo['dym'] = (dym, Sn, dm, dm, False)
    elif name == 'colsum':
        x, rows, n, ld, out, beta, wsp, xbf = args
        I['x'] = (x, rows, n, ld, bool(xbf))
        Oo['out'] = (out, 1, n, n, False)
    elif name == 'dropout_bwd_colsum':
        g, rows, n, ld, site, out, beta, wsp, gbf = args
        Oo['g'] = (g, rows, n, ld, bool(gbf))
        Oo['out'] = (out, 1, n, n, False)
    elif name == 'embed_fold_bwd':
        f = d
        nw = f.n_proc - f.kw + 1
        I['dweff'] = (f.dweff, f.d, f.Kp, f.Kp, False)
        I['dbeff'] = (f.dbeff, 1, f.d, f.d, False)
        I['wconv'] = (f.wconv, f.C, f.kw, f.kw, False)
        I['bconv'] = (f.bconv, 1, f.C, f.C, False)
        I['wtok'] = (f.wtok, f.d, f.C * nw, f.C * nw, False)
        I['btok'] = (f.btok, 1, f.d, f.d, False)
        Oo['g_wconv'] = (f.g_wconv, f.C, f.kw, f.kw, False)
        Oo['g_bconv'] = (f.g_bconv, 1, f.C, f.C, False)
        Oo['g_wtok'] = (f.g_wtok, f.d, f.C * nw, f.C * nw, False)
        Oo['g_btok'] = (f.g_btok, 1, f.d, f.d, False)
    else:
        raise AssertionError('a launch kind the backward harness does not know: %s' % name)
    return I, Oo


def accumulates(entry):
    """does the launch read the prior contents of its (gradient) outputs?  tn / reduce / colsum: beta; a dX launch: C == residual"""
    fn, args, name, meta = entry
    d = _dsc(entry)
    if name == 'gemm_tn':
        return d.beta != 0.0
    if name == 'ln_bwd_reduce':
        return args[4] != 0.0
    if name == 'colsum':
        return args[5] != 0.0
    if name == 'dropout_bwd_colsum':
        return args[6] != 0.0
    if name in ('gemm_nt', 'strip_linear'):
        return bool(d.residual) and d.residual == d.C
    return False


def sites_of(entry, forward):
    """the dropout sites a plan entry names"""
    fn, args, name, meta = entry
    s = []
    for a in args if not isinstance(fn, str) else ():
        d = getattr(a, '_obj', None)
        if d is None:
            continue
        if hasattr(d, 'site_h'):
            s += [d.site_h, d.site_o] if forward else [d.site_o]
        elif hasattr(d, 'drop_site'):
            s.append(d.drop_site)
    if name == 'time_embed_fwd':
        s.append(args[3])
    elif name == 'time_embed_bwd':
        s.append(args[3])
    elif name == 'dropout_bwd_colsum':
        s.append(args[4])
    return [int(x) for x in s if x]


def make_record(entry, arrays, prior, eng, ws):
    """the launch record of one plan entry from its descriptor and the captured arrays"""
    fn, args, name, meta = entry
    d = _dsc(entry)
    p, seed = ws['p'], ws['seed']
    B, T, N, V, dm = ws['B'], eng.T, eng.N, eng.V, eng.d
    rec = dict(kind=name, prior=prior, **arrays)
    mode = 'parity' if eng.npass == 3 else 'x3'
    if name == 'gemm_nt':
        rec['wkey'], rec['W'] = _plane_weight(eng, d.W, d.N, d.K)
        rec.update(npass=d.npass, a_hi=bool(d.io_flags & 16), act=d.act, out_scale=d.out_scale, add_mod=d.add_mod, gate_scale=d.gate_scale, drop_p=d.drop_p,
                   site=d.drop_site, seed=d.drop_seed, res_mod=d.res_mod)
    elif name == 'strip_linear':
        rec['wkey'], (rec['W'],) = _strip_weight(eng, d.w, [(d.N, d.K)])
        assert not (d.flags & SL_RELU)
        rec.update(npass=4 if d.flags & SL_X3_BF16 else 2, a_hi=bool(d.flags & SL_X3_GRAD_HI), out_scale=d.out_scale, gate_scale=d.gate_scale, drop_p=d.drop_p,
                   site=d.drop_site, seed=d.drop_seed, res_mod=d.res_mod, x_drop=bool(d.flags & SL_X_DROP))
    elif name == 'ffn_bwd_dx':
        rec['wkey'], (rec['W_a'], rec['W_b']) = _strip_weight(eng, d.w, [(d.p, d.d), (d.d, d.p)])
        rec.update(gate_scale=d.gate_scale, drop_p=d.drop_p, site_o=d.site_o, seed=d.drop_seed, h_bf=bool(d.flags & SL_H_BF16))
    elif name == 'gemm_tn':
        rec.update(npass=d.npass, out_scale=d.out_scale, beta=d.beta, K_out=d.K_out, segs=[(d.seg_row0[i], d.seg_rows[i]) for i in range(d.n_seg)],
                   has_db=[bool(d.seg_db[i]) for i in range(d.n_seg)], dy_hi=bool(d.io_flags & 4), dy_drop=bool(d.io_flags & 8), drop_p=d.drop_p,
                   site=d.drop_site, seed=d.drop_seed)
        assert not rec['dy_drop'] or d.lddy == d.N
    elif name == 'attn_bwd':
        w, planes = d.n_heads * d.dh, bool(d.io_flags & 32)
        assert bool(d.io_flags & 64) == planes
        dec = L.planes_decode if planes else (lambda t: t)
        for k_, L_ in (('q', d.Lq), ('k', d.Lk), ('v', d.Lk), ('dout', d.Lq)):
            t = rec[k_] if k_ == 'dout' else dec(rec[k_])
            rec[k_] = t.reshape(-1, L_, w)
        rec.update(H=d.n_heads, drop_p=d.drop_p, site=d.drop_site, seed=d.drop_seed, planes=planes, mode=mode, shape=(d.n_seq, d.n_heads, d.Lq, d.Lk))
    elif name == 'ln_bwd':
        rec.update(drop_p=d.drop_p, site=d.drop_site, seed=d.drop_seed, has_drop=bool(d.dr_drop), drop_bf=bool(d.drop_bf16))
    elif name == 'ln_bwd_reduce':
        rec.update(N=args[1], beta=args[4])
    elif name == 'heads_split_bwd':
        rec.update(B=B, T=T, N=N, V=V, ldl=eng.NHp, tm=args[2], prob=[rec.pop('prob%d' % i).reshape(B, T, N) for i in range(3)],
                   d_prob=[rec.pop('d_prob%d' % i).reshape(B, T, N) for i in range(3)])
    elif name == 'time_embed_bwd':
        rec.update(shape=(B, T, N, dm), scale=math.sqrt(dm), drop_p=p, site=args[3], seed=seed, has_dym=bool(args[2]))
    elif name == 'colsum':
        rec.update(beta=args[5])
    elif name == 'dropout_bwd_colsum':
        rec.update(beta=args[6], ld=args[3], drop_p=p, site=args[4], seed=seed)
    elif name == 'embed_fold_bwd':
        rec.update(n_proc=d.n_proc)
    return rec


# ---------------------------------------------------------------------------------------------------------------------------- stepping
def step_plan(eng, ws, plan, launch):
    """Walks `plan` one entry at a time: copies every input span and the prior contents of every output to the host, builds the record, calls
    launch(i, entry, rec, spans, outputs) -- which runs that one entry and returns when it is complete --, copies the outputs and checks them.
    Yields (index, entry, record, {output: (tensor name, first element, rows, cols, row stride)}, figures)."""
    sp = engine_spans(eng, ws)
    for i, entry in enumerate(plan):
        I, Oo = launch_io(entry, eng, ws)
        arrays = {k: sp.fetch(*v) for k, v in I.items()}
        prior = {k: sp.fetch(*v) for k, v in Oo.items()}
        rec = make_record(entry, arrays, prior, eng, ws)
        launch(i, entry, rec, sp, Oo)
        rec['got'] = {k: sp.fetch(*v) for k, v in Oo.items()}
        where = {k: sp.where(v[0], v[1], v[2], v[3])[:2] + (v[1], v[2], v[3]) for k, v in Oo.items()}
        yield i, entry, rec, where, check(rec)


def describe(i, entry, where):
    """a failing link names itself: plan index, op, kernel, output buffers"""
    return 'plan[%d] %s %s -> %s' % (i, entry[2], (entry[3] or {}).get('kernel', '-'), ', '.join('%s=%s+%d' % (k, w[0], w[1]) for k, w in where.items()))


# ---------------------------------------------------------------------------------------------------------------------------- the plan's own scalars
class PlanRules:
    """The link check reads a launch's scalars from its descriptor, so a descriptor that is wrong in itself (an out_scale the builder forgot,
    a mask applied twice) would be held to its own mistake.  These rules say what the descriptors of a backward plan must carry from the
    GRAPH: the forward plan of the same workspace, the parameters' shapes, and which launch produced the buffer a launch reads.
      * a LayerNorm backward regenerates the site of the forward launch that saved the pre-LayerNorm sum it reads; an attention backward
        the site of the forward attention that wrote its row statistics; time_embed_bwd / dropout_bwd_colsum the forward's own sites;
      * the gradient operand of a product is masked exactly once: one that was written as a LayerNorm backward's UNMASKED dr (dropout on) is
        masked on load with that site (HFTT_TN_DY_DROP, HFTT_SL_X_DROP, site_o), anything else -- the masked copy included -- is not;
      * every LayerNorm backward's dr comes back exactly once as the residual of a dX launch (layer zero: as the operand of the position
        table's column sum) before the next LayerNorm backward overwrites it or the plan ends;
      * a gated launch carries the run-time 1 / keep of HfttEngine._patch;
      * a weight-gradient segment is one whole parameter [rows, K_out], starts at the row where the forward stacks that parameter (the
        layout's own entries), and its bias is the same module's; out_scale is sqrt(d) on the
        embedding product (the forward's out_scale on x0) and 1 elsewhere."""

    def __init__(self, eng, ws):
        self.eng, self.ws, self.sp = eng, ws, engine_spans(eng, ws)
        self.producer, self.pending = {}, {}
        self.site_of_r, self.site_of_lse = {}, {}
        for fn, args, name, meta in ws['fwd']:
            for a in (args if not isinstance(fn, str) else ()):
                d = getattr(a, '_obj', None)
                if d is None:
                    continue
                if getattr(d, 'pre_ln_out', None):
                    self.site_of_r[d.pre_ln_out] = d.site_o if hasattr(d, 'site_o') else d.drop_site
                if name == 'attn_fwd':
                    self.site_of_lse[d.lse] = d.drop_site
        self.param_at = {o: n for n, _, o, _ in eng._bound}
        # the row at which a weight sits in the (stacked) matrices the forward multiplies with: where its block of dY^T starts
        lay, self.rows_of = eng.layout, {}
        for (so, do, rows, cols, sld, dld, kind), key in zip(lay.prep, lay.prep_keys):
            if kind == 0 and so in self.param_at:
                self.rows_of.setdefault(self.param_at[so], set()).add((do - lay.wl.items[key]) // cols)
        for e in lay.spack:
            if not e[5] and e[0] in self.param_at:
                self.rows_of.setdefault(self.param_at[e[0]], set()).add(e[6])

    def _src(self, addr, rows, cols, ld):
        return self.producer.get(self.sp.where(addr, rows, cols, ld)[:2])

    def check(self, i, entry, where):
        """violations of launch i (call it after the launch: `where` are its outputs)"""
        fn, args, name, meta = entry
        d = _dsc(entry)
        eng, ws = self.eng, self.ws
        p, bad = ws['p'], []
        ks = f32c(keep_scale(p))
        operand = residual = None
        masked_site = 0
        if name == 'ln_bwd':
            if p > 0 and d.drop_site != self.site_of_r.get(d.r):
                bad.append('regenerates site %d; the forward launch that saved its pre-LayerNorm sum dropped with site %s' % (d.drop_site, self.site_of_r.get(d.r)))
            key = where['dr'][:2]
            if key in self.pending:
                bad.append('overwrites the dr of plan[%d], which no launch has added back as a residual' % self.pending[key])
            self.pending[key] = i
        elif name == 'attn_bwd':
            if d.drop_site != self.site_of_lse.get(d.lse):
                bad.append('regenerates site %d; the forward attention of these row statistics dropped with site %s' % (d.drop_site, self.site_of_lse.get(d.lse)))
        elif name == 'time_embed_bwd':
            if args[3] != ws['sites']['time_embed']:
                bad.append('site %d, the forward time embedding has %d' % (args[3], ws['sites']['time_embed']))
        elif name == 'dropout_bwd_colsum':
            if args[4] != ws['sites']['embed']:
                bad.append('site %d, the forward embedding has %d' % (args[4], ws['sites']['embed']))
        elif name == 'gemm_tn':
            operand = (d.dY, d.M, d.N, d.lddy)
            masked_site = d.drop_site if (d.io_flags & 8) else 0
            embed = d.seg_dw[0] == eng.dweff.data_ptr()
            want = f32c(math.sqrt(eng.d)) if embed else 1.0
            if f32c(d.out_scale) != want:
                bad.append('out_scale %g, the graph has %g' % (d.out_scale, want))
            for s in range(d.n_seg):
                tname, off = where['dw%d' % s][:2]
                if embed:
                    if not (d.n_seg == 1 and d.seg_rows[0] == eng.d and d.K_out == eng.Kp and where['db0'][:2] == ('dbeff', 0)):
                        bad.append('the embedding product does not fill dWeff [d, Kp] and dbeff')
                    continue
                pname = self.param_at.get(off) if tname == 'flat_grads' else None
                if pname is None or tuple(eng.pshape[pname]) != (d.seg_rows[s], d.K_out):
                    bad.append('segment %d [%d, %d] is not one whole parameter (%s)' % (s, d.seg_rows[s], d.K_out, pname))
                elif d.seg_row0[s] not in self.rows_of.get(pname, ()):
                    bad.append('segment %d takes rows %d .. of dY^T for %s, which the forward stacks at %s' % (s, d.seg_row0[s], pname, sorted(self.rows_of.get(pname, ()))))
                elif ('db%d' % s) in where:
                    bname = self.param_at.get(where['db%d' % s][1])
                    if bname != pname[:-len('weight')] + 'bias':
                        bad.append('segment %d: the bias gradient of %s goes to %s' % (s, pname, bname))
        elif name == 'strip_linear':
            operand = (d.x, d.M, d.K, d.ldx)
            masked_site = d.drop_site if (d.flags & SL_X_DROP) else 0
            residual = (d.residual, d.res_mod or d.M, d.N, d.ldr) if d.residual else None
            if d.gate and f32c(d.gate_scale) != ks:
                bad.append('gate_scale %g, 1 / keep is %g' % (d.gate_scale, ks))
        elif name == 'gemm_nt':
            operand = (d.A, d.M, d.K, d.lda)
            residual = (d.residual, d.res_mod or d.M, d.N, d.ldr) if d.residual else None
            if d.gate and f32c(d.gate_scale) != ks:
                bad.append('gate_scale %g, 1 / keep is %g' % (d.gate_scale, ks))
            if d.drop_site or f32c(d.out_scale) != 1.0 or d.act or d.add_table:
                bad.append('a forward epilogue (dropout / out_scale / act / add_table) on a backward product')
        elif name == 'ffn_bwd_dx':
            operand = (d.x, d.M, d.d, d.ldx)
            masked_site = d.site_o
            residual = (d.residual, d.M, d.d, d.ldr) if d.residual else None
            if f32c(d.gate_scale) != ks:
                bad.append('gate_scale %g, 1 / keep is %g' % (d.gate_scale, ks))
        elif name == 'colsum':
            key = self.sp.where(args[0], args[1], args[2], args[3])[:2]
            self.pending.pop(key, None)                   # (layer zero: its residual is the position table, whose gradient is this sum)
        if operand is not None:
            src = self._src(*operand)
            want = src[3] if (src is not None and src[1:3] == ('ln_bwd', 'dr') and p > 0) else 0
            if masked_site != want:
                bad.append('masks its gradient operand with site %d; it reads what %s wrote: the graph has site %d' % (masked_site, src, want))
        if residual is not None and residual[0] != getattr(d, 'C', getattr(d, 'y', None)):
            key = self.sp.where(*residual)[:2]
            src = self.producer.get(key)
            if src is None or src[1:3] != ('ln_bwd', 'dr'):
                bad.append('its residual is what %s wrote, not a LayerNorm backward\'s dr' % (src,))
            elif key not in self.pending:
                bad.append('adds back the dr of plan[%d] a second time' % src[0])
            self.pending.pop(key, None)
        site = d.drop_site if name == 'ln_bwd' else 0
        for out, w in where.items():
            self.producer[w[:2]] = (i, name, out, site)
        return bad

    def finish(self):
        return ['the dr of plan[%d] is never added back as a residual' % i for i in self.pending.values()]
