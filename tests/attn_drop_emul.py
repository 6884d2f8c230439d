"""Attention dropout, decision by decision (CPU; no GPU import): the shapes, the operand constructions that turn an attention kernel's outputs
into the keep mask it applied, their decoders, the fp64 reference, a model of "a kernel that applies mask m'", and the planted defects.

With q = 0 every score is 0 and P = 1 / Lk exactly, in every precision mode; key padding and the row maximum drop out.  Write ks =
keep_scale(p), m = the applied mask [n, H, Lq, Lk], and let `base` run over blocks of dh indices.  Per head:
  * forward:        v_j = e_(j - base) for base <= j < base + dh, 0 elsewhere     ->  out[i, c] = ks / Lk * m[i, base + c]
  * backward, dV:   any v, dO_i = e_(i - base)                                    ->  dV[j, c]  = ks / Lk * m[base + c, j]
  * backward, dS:   k_j = e_(j - base), v_j = A * 1, dO_i = B * 1, c0 = A B dh    ->  dq[i, c] sqrt(dh) = (m[i, base + c] ks c0 - delta_i) / Lk,
                    delta_i = rowsum(dO * O): the backward's second select (dP), read with the delta of the forward's own output
A dropped element of the first two is one term that is exactly zero.  The contract is the flat index ((seq H + head) Lq + row) Lk + key of
include/hftt_hip.h, emulated by util.keep_mask.

tests/test_attn_drop_emul_bound.py calibrates the decoders on the model (the true mask comes back exactly at every shape and store precision,
every planted defect is reported); tests/test_attn_dropout_gpu.py runs the same decoders on the kernels."""
import math

import numpy as np
import torch

import util

N_SEQ, HEADS = 3, 2             # sequence and head order both show in the flat index
SEED, SITE = 20240611, 11
P_MAIN, P_ALT = 0.1, 0.25       # thresholds 230 and 192 of 256
A_V, B_DO = 1.0, 1.0            # the constants of the dS construction (exact in every operand format)

# (Lq, Lk, layout): 'cross' q [n, Lq, d] and a fused k | v [n, Lk, 2d]; 'self' one fused [n, L, 3d]; 'shared' one query block for all
# sequences (sequence stride 0) with a per-sequence dq.  Lk % 4 in {1, 2, 3}; Lk % 32 != 0 at every key-tile count 1, 2, 3, 4, 8;
# Lq % 32 != 0 with one, several and more than four query blocks; idle waves.  Below the line: quad-form (Lk % 4 == 0) partners, one per
# key-tile count (16: KT 1, 48: KT 2, 88: KT 3, 128: KT 4, 132: KT 8 with more than four query blocks).
SHAPES = [
    (12, 15, 'cross'), (15, 15, 'self'), (33, 34, 'cross'), (88, 70, 'cross'), (88, 70, 'shared'), (40, 97, 'cross'), (100, 129, 'cross'),
    (200, 250, 'cross'), (255, 255, 'self'),
    (16, 16, 'self'), (16, 48, 'cross'), (88, 88, 'self'), (128, 128, 'self'), (136, 132, 'cross'),
]
OLD_CASE = (4, 4, 88, 256)         # the one shape with an independent mask in the suite before this file (n, H, Lq, Lk)

# value bands of part 2 (relative to the output's maximum): the bounds each mode's dropout test already had
BANDS = {'x3': dict(out=1e-4, grad=3e-4, map=2e-5), 'parity': dict(out=1e-4, grad=2e-4, map=2e-5), 'bf16': dict(out=2e-2, grad=3e-2, map=2e-2)}
PLANES_VS_FP32_OPERANDS = 4e-5

# store precisions of the modes: P as the P.V operand, dS as the dQ / dK operand, the outputs
PREC = {'parity': dict(p='f32', pb='f32', ds='f32', store='f32'),
        'x3': dict(p='f16pair', pb='bf16pair', ds='bf16pair', store='f32'),
        'bf16': dict(p='bf16', pb='bf16', ds='bf16', store='bf16')}


def key_tiles(Lk):
    kt = (Lk + 31) // 32
    return kt if kt <= 4 else 8


def rnd(x, kind):
    """x (float64) through a store format and back"""
    if kind == 'f64':
        return x
    if kind == 'f32':
        return x.float().double()
    if kind == 'bf16':
        return x.float().bfloat16().double()
    dt = torch.float16 if kind == 'f16pair' else torch.bfloat16
    hi = x.float().to(dt).double()
    return hi + (x - hi).float().to(dt).double()


def kept_tol(mode, Lk, p):
    """relative band of a kept element's ks / Lk: the mode's store precision (1e-5: fp32 stores behind fp16 / bf16 pairs of 2^-18; bf16: one ulp)"""
    if mode != 'bf16':
        return 1e-5
    x = util.keep_scale(p) / Lk
    return 2.0 ** (math.floor(math.log2(x)) - 7) / x


def ds_tol(mode):
    """absolute band of the decoded dS read-off (whose two values are 0 and 1).  bf16 (unit roundoff 2^-8: eight significant bits): P as the
    forward's P.V operand -- every element of a row is the same ks / Lk, so its rounding is common to the row and does not average out --, O,
    dS, K - mean(K) and dq are each rounded to bf16, five roundings of quantities below 1 in decoded units (the row's kept fraction ~0.9,
    which also leaves room for the fp32 arithmetic between them); fp32 stores: as kept_tol"""
    return 5 * 2.0 ** -8 if mode == 'bf16' else 1e-5


# ------------------------------------------------------------------------------------------------------------------ masks
def _grid(n, H, Lq, Lk):
    return np.meshgrid(*(np.arange(x, dtype=np.uint64) for x in (n, H, Lq, Lk)), indexing='ij')


def _keep(idx, p):
    return torch.from_numpy(util.keep_mask(SEED, SITE, idx.ravel(), p).reshape(idx.shape))


def true_mask(n, H, Lq, Lk, p):
    return util.keep_mask_t(SEED, SITE, (n, H, Lq, Lk), p)


def _applied(fwd, dv=None, ds=None, **kw):
    d = dict(fwd=fwd, dv=fwd if dv is None else dv, ds=fwd if ds is None else ds, map_dropped=False, ds_scaled=True)
    d.update(kw)
    return d


def _backward_right(n, H, Lq, Lk, p):
    return dict(dv=true_mask(n, H, Lq, Lk, p), ds=true_mask(n, H, Lq, Lk, p))


def no_defect(n, H, Lq, Lk, p):
    return _applied(true_mask(n, H, Lq, Lk, p))


def quads_from_row_start(n, H, Lq, Lk, p):
    """forward: the quad form where it does not apply -- quads counted from the row's first element instead of the flat index (Lk % 4 != 0)"""
    s, h, i, j = _grid(n, H, Lq, Lk)
    prow = ((s * H + h) * Lq + i) * Lk
    return _applied(_keep(((prow >> 2) + (j >> 2)) * 4 + (j & 3), p), **_backward_right(n, H, Lq, Lk, p))


def bwd_padded_row_stride(n, H, Lq, Lk, p):
    """backward: (row, key) indexed with the row stride 32 KT (padded keys counted)"""
    s, h, i, j = _grid(n, H, Lq, Lk)
    m = _keep(((s * H + h) * Lq + i) * np.uint64(32 * key_tiles(Lk)) + j, p)
    return _applied(true_mask(n, H, Lq, Lk, p), dv=m, ds=m)


def bwd_transposed_4x4(n, H, Lq, Lk, p):
    """backward: its 4 rows (registers) x 4 keys (lanes) block of decisions transposed"""
    s, h, i, j = _grid(n, H, Lq, Lk)
    four = np.uint64(3)
    i2, j2 = (i & ~four) + (j & four), (j & ~four) + (i & four)
    ok = (i2 < Lq) & (j2 < Lk)
    i2, j2 = np.where(ok, i2, i), np.where(ok, j2, j)
    m = _keep(((s * H + h) * Lq + i2) * Lk + j2, p)
    return _applied(true_mask(n, H, Lq, Lk, p), dv=m, ds=m)


def key_off_by_one_behind_tile_border(n, H, Lq, Lk, p):
    """forward: the first key of every 32-key tile but the first takes its left neighbour's decision"""
    s, h, i, j = _grid(n, H, Lq, Lk)
    j2 = np.where((j > 0) & (j % 32 == 0), j - 1, j)
    return _applied(_keep(((s * H + h) * Lq + i) * Lk + j2, p), **_backward_right(n, H, Lq, Lk, p))


def head_and_sequence_swapped(n, H, Lq, Lk, p):
    """forward and backward alike: (head n + seq) where the contract has (seq H + head)"""
    s, h, i, j = _grid(n, H, Lq, Lk)
    return _applied(_keep(((h * n + s) * Lq + i) * Lk + j, p))


def clamped_row_takes_neighbour(n, H, Lq, Lk, p):
    """forward: the last row of a ragged query block (Lq % 32) takes the decisions of the row before it"""
    s, h, i, j = _grid(n, H, Lq, Lk)
    i2 = np.where((i == Lq - 1) & (Lq % 32 != 0) & (i > 0), i - 1, i)
    return _applied(_keep(((s * H + h) * Lq + i2) * Lk + j, p), **_backward_right(n, H, Lq, Lk, p))


def map_dropped(n, H, Lq, Lk, p):
    return _applied(true_mask(n, H, Lq, Lk, p), map_dropped=True)


def ds_select_unscaled(n, H, Lq, Lk, p):
    """backward: the kept dP without the keep scale (the dV select has it)"""
    return _applied(true_mask(n, H, Lq, Lk, p), ds_scaled=False)


DEFECTS = {f.__name__: f for f in (quads_from_row_start, bwd_padded_row_stride, bwd_transposed_4x4, key_off_by_one_behind_tile_border,
                                   head_and_sequence_swapped, clamped_row_takes_neighbour, map_dropped, ds_select_unscaled)}


# ------------------------------------------------------------------------------------------------------------------ the model kernel
def _heads(t, n, H):
    L, d = t.shape[1], t.shape[2]
    return t.double().expand(n, L, d).reshape(n, L, H, d // H).transpose(1, 2)


def _flat(t):
    n, H, L, dh = t.shape
    return t.transpose(1, 2).reshape(n, L, H * dh)


class ModelKernel:
    """Attention forward and backward in fp64 that apply the masks of `applied` (see _applied) with the store roundings of `mode`
    (None: none -- with the true mask that is the fp64 reference).  The interface the read-offs drive: fwd -> (out, state, map),
    bwd(state, dO) -> (dq [n, Lq, d] per sequence, dk, dv)."""

    def __init__(self, applied, p, H, mode=None):
        self.a, self.ks, self.H = applied, util.keep_scale(p), H
        self.prec = PREC[mode] if mode else dict(p='f64', pb='f64', ds='f64', store='f64')

    def fwd(self, q, k, v, want_probs=False):
        n, H = k.shape[0], self.H
        qh, kh, vh = _heads(q, n, H), _heads(k, n, H), _heads(v, n, H)
        pr = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(qh.shape[-1]), -1)
        out = rnd(_flat(rnd(pr * self.a['fwd'] * self.ks, self.prec['p']) @ vh), self.prec['store'])
        pm = (pr * self.a['fwd'] * self.ks if self.a['map_dropped'] else pr) if want_probs else None
        return out, (qh, kh, vh, pr, out), pm

    def bwd(self, state, dO):
        qh, kh, vh, pr, out = state
        n, H = kh.shape[0], self.H
        dh = qh.shape[-1]
        doh, oh = _heads(dO, n, H), _heads(out, n, H)
        dv = rnd(_flat(rnd(pr * self.a['dv'] * self.ks, self.prec['pb']).transpose(-1, -2) @ doh), self.prec['store'])
        delta = (doh * oh).sum(-1, keepdim=True)
        dS = rnd(pr * ((doh @ vh.transpose(-1, -2)) * self.a['ds'] * (self.ks if self.a['ds_scaled'] else 1.0) - delta) / math.sqrt(dh), self.prec['ds'])
        return rnd(_flat(dS @ kh), self.prec['store']), rnd(_flat(dS.transpose(-1, -2) @ qh), self.prec['store']), dv


def reference(q, k, v, dO, H, mask, p):
    """fp64 attention with dropout mask `mask` and its gradients for the loss sum(out * dO); q [n or 1, Lq, d]: dq is summed over the sequences
    that share a query block"""
    mk = ModelKernel(_applied(mask), p, H)
    out, st, pm = mk.fwd(q, k, v, True)
    dq, dk, dv = mk.bwd(st, dO)
    if q.shape[0] == 1:
        dq = dq.sum(0, keepdim=True)
    return dict(out=out, map=pm, dq=dq, dk=dk, dv=dv)


# ------------------------------------------------------------------------------------------------------------------ operands
def unit_rows(n, L, H, dh, base):
    """[n, L, H dh]: row r holds e_(r - base) in every head for base <= r < base + dh, zero elsewhere"""
    t = torch.zeros(n, L, H, dh)
    r = torch.arange(base, min(L, base + dh))
    for h in range(H):
        t[:, r, h, r - base] = 1.0
    return t.reshape(n, L, H * dh)


def _q0(n, Lq, d, layout):
    return torch.zeros(1 if layout == 'shared' else n, Lq, d)


def fwd_operands(n, H, Lq, Lk, layout, dh, base, gen):
    return _q0(n, Lq, H * dh, layout), torch.randn(n, Lk, H * dh, generator=gen), unit_rows(n, Lk, H, dh, base)


def dv_operands(n, H, Lq, Lk, layout, dh, base, gen):
    d = H * dh
    return _q0(n, Lq, d, layout), torch.randn(n, Lk, d, generator=gen), torch.randn(n, Lk, d, generator=gen), unit_rows(n, Lq, H, dh, base)


def ds_operands(n, H, Lq, Lk, layout, dh, base):
    d = H * dh
    return _q0(n, Lq, d, layout), unit_rows(n, Lk, H, dh, base), torch.full((n, Lk, d), A_V), torch.full((n, Lq, d), B_DO)


def random_operands(n, H, Lq, Lk, layout, dh, mode, gen):
    """part 2: q, k, v, dO (gradient-sized in the x3 forms, bf16-valued on the bf16 stream)"""
    d = H * dh
    q = torch.randn(1 if layout == 'shared' else n, Lq, d, generator=gen)
    k, v = torch.randn(n, Lk, d, generator=gen), torch.randn(n, Lk, d, generator=gen)
    dO = torch.randn(n, Lq, d, generator=gen) * (1e-5 if mode == 'x3' else 1.0)
    if mode == 'bf16':
        q, k, v, dO = (t.bfloat16().float() for t in (q, k, v, dO))
    return q, k, v, dO


# ------------------------------------------------------------------------------------------------------------------ decoders
def _per_head(t, H):
    n, L, d = t.shape
    return t.double().reshape(n, L, H, d // H).permute(0, 2, 1, 3)            # [n, H, L, dh]


def decode_fwd(outs, H, Lk, dh, ks):
    """outs[b]: the forward's out [n, Lq, d] of block base = b dh  ->  m ks / Lk * (Lk / ks) = the applied mask as 0 / 1 values [n, H, Lq, Lk]"""
    return torch.cat([_per_head(o, H) for o in outs], -1)[..., :Lk] * (Lk / ks)


def decode_dv(dvs, H, Lq, Lk, dh, ks):
    """dvs[b]: dV [n, Lk, d] with dO_i = e_(i - b dh): dV[j, c] = ks / Lk * m[base + c, j]"""
    return torch.cat([_per_head(t, H).transpose(-1, -2) for t in dvs], -2)[..., :Lq, :] * (Lk / ks)


def decode_ds(dqs, outs, H, Lk, dh, ks):
    """dqs[b], outs[b]: dq and the forward's out, both [n, Lq, d], with k_j = e_(j - b dh): m = (dq sqrt(dh) Lk + delta) / (ks c0)"""
    c0 = A_V * B_DO * dh
    vals = [(_per_head(dq, H) * (math.sqrt(dh) * Lk) + B_DO * _per_head(o, H).sum(-1, keepdim=True)) / (ks * c0) for dq, o in zip(dqs, outs)]
    return torch.cat(vals, -1)[..., :Lk]


def read_offs(kern, n, H, Lq, Lk, layout, dh, p, want_probs=False):
    """The three read-offs of one kernel form (`kern`: ModelKernel's interface; tensors come back on the CPU).  The forward runs with or
    without the attention map (two kernel forms); the backward reads the statistics of a forward of its own settings."""
    ks = util.keep_scale(p)
    gen = torch.Generator().manual_seed(Lq * 1000 + Lk)
    res = {'map': []}
    outs = []
    for base in range(0, Lk, dh):
        out, _, pm = kern.fwd(*fwd_operands(n, H, Lq, Lk, layout, dh, base, gen), want_probs)
        outs.append(out)
        if want_probs:
            res['map'].append(pm)
    res['fwd'] = decode_fwd(outs, H, Lk, dh, ks)
    dvs = []
    for base in range(0, Lq, dh):
        q, k, v, dO = dv_operands(n, H, Lq, Lk, layout, dh, base, gen)
        _, st, _ = kern.fwd(q, k, v, False)
        dvs.append(kern.bwd(st, dO)[2])
    res['dv'] = decode_dv(dvs, H, Lq, Lk, dh, ks)
    dqs, outs = [], []
    for base in range(0, Lk, dh):
        q, k, v, dO = ds_operands(n, H, Lq, Lk, layout, dh, base)
        out, st, _ = kern.fwd(q, k, v, False)
        outs.append(out)
        dqs.append(kern.bwd(st, dO)[0])
    res['ds'] = decode_ds(dqs, outs, H, Lk, dh, ks)
    return res


def failures(res, mask, Lk, p, mode):
    """what the read-offs `res` hold against the contract's mask: [] when every decision and every kept value is right"""
    bad = []
    mk = mask.bool()
    for name in ('fwd', 'dv', 'ds'):
        val = res[name].double()
        got = val > 0.5
        if not torch.equal(got, mk):
            w = (got != mk).nonzero()
            bad.append('%s: %d of %d decisions differ, first at (seq, head, row, key) = %s' % (name, len(w), mk.numel(), tuple(w[0].tolist())))
            continue
        if name == 'ds':
            err = (val - mk.double()).abs().max().item()
            if not err <= ds_tol(mode):
                bad.append('ds: a decoded value is %.3e from 0 / 1 (band %.1e)' % (err, ds_tol(mode)))
        else:
            err = ((val - 1.0).abs() * mk).max().item()
            if not err <= kept_tol(mode, Lk, p):
                bad.append('%s: a kept element is %.3e (relative) from ks / Lk (band %.1e)' % (name, err, kept_tol(mode, Lk, p)))
            if not bool((val[~mk] == 0).all()):
                bad.append('%s: a dropped element is not exactly zero' % name)
    for pm in res['map']:
        # pre-dropout (model_spec2midi.py:360): 1 / Lk everywhere; exp2(0) = 1 and the sum Lk are exact, the reciprocal is within an ulp
        err = (pm.double() * Lk - 1.0).abs().max().item()
        if not err <= 1e-6:
            bad.append('map: %.3e (relative) from 1 / Lk' % err)
    return bad
