"""Attention dropout in every kernel form, through ops.attn_fwd / ops.attn_bwd (tests/attn_drop_emul.py has the constructions, the decoders
and their CPU calibration):
  1. the mask each kernel APPLIES, read off its outputs decision by decision -- the forward, the backward's dV select and the backward's dP
     select -- must equal util.keep_mask_t in every element, a kept element must carry keep_scale / Lk to the mode's store precision, the
     returned attention map must stay pre-dropout, and nothing may be written behind Lq rows or Lk keys (sentinel tails);
  2. random operands against fp64 with the same mask, inside the band each mode's dropout test already had;
  3. the kernel forms the cases reach (from plan.attn_meta, which mirrors the C dispatch; a kernel trace of this file is on record in
     profiles/attn_dropout_mi355x.txt).
Modes: parity (npass 3), x3 on fp32 operands (npass 2), x3 on f16-pair planes (dh 64), the bf16 stream with every tensor bf16."""
import functools

import pytest
import torch

import attn_drop_emul as A
import util
from util import rel_err, max_err

pytestmark = pytest.mark.gpu

N, H = A.N_SEQ, A.HEADS
BF = torch.bfloat16
SENTINEL = -77.0                 # (exact in bf16)
GUARD = 3                        # sentinel rows behind Lq / Lk in every sequence
MODES = [('parity', 64), ('parity', 32), ('x3', 64), ('x3', 32), ('x3p', 64), ('bf16', 64), ('bf16', 32)]
NPASS = {'parity': 3, 'x3': 2, 'x3p': 2, 'bf16': 1}


def _id(s):
    return '%dx%d-%s' % s


def _ops():
    from hftt_hip import ops
    return ops


def kernel_names(mode, dh, Lq, Lk, p, want_probs):
    """(forward, backward) kernel of one case by the dispatch rule of plan.attn_meta"""
    from hftt_hip import plan
    bf = mode == 'bf16'
    dm = 0 if not p > 0 else (1 if Lk % 4 == 0 else 2)
    args = (N, H, Lq, Lk, H * dh)
    f = plan.attn_meta(NPASS[mode], False, *args, 7 if bf else 0, mode == 'x3p', want_probs, dm)['kernel']
    b = plan.attn_meta(NPASS[mode], True, *args, 31 if bf else 0, mode == 'x3p', False, dm)['kernel']
    return f, b


class DeviceKernel:
    """the read-offs' kernel interface (attn_drop_emul.ModelKernel) on the device: operands laid out as the engine lays them out ('self': one
    fused [n, L, 3d] and interleaved gradients; 'cross' / 'shared': q alone, or one block for all sequences, and a fused k | v), every output
    in a caller-owned buffer with a sentinel tail"""

    def __init__(self, dev, mode, layout, p):
        self.dev, self.mode, self.layout, self.p = dev, mode, layout, p
        self.dt = BF if mode == 'bf16' else torch.float32
        self.kw = dict(npass=NPASS[mode], drop_p=p, drop_site=A.SITE, drop_seed=A.SEED)
        if mode == 'x3p':
            self.kw['planes'] = True
        self.bad = []                # sentinel violations

    def _tail(self, what, buf, L):
        if not bool((buf[:, L:] == SENTINEL).all()):
            self.bad.append('%s: written behind row %d' % (what, L))

    def _flat_tail(self, what, buf, numel):
        if not bool((buf[numel:] == SENTINEL).all()):
            self.bad.append('%s: written behind its last element' % what)

    def _operands(self, q, k, v):
        ops, dev = _ops(), self.dev
        prep = ops.to_planes if self.mode == 'x3p' else (lambda t: t)
        d = k.shape[-1]
        if self.layout == 'self':
            f = prep(torch.cat([q, k, v], -1).to(dev).to(self.dt).contiguous())
            return f[..., :d], f[..., d:2 * d], f[..., 2 * d:]
        kv = prep(torch.cat([k, v], -1).to(dev).to(self.dt).contiguous())
        qd = prep(q.to(dev).to(self.dt).contiguous())
        return qd.expand(N, -1, -1), kv[..., :d], kv[..., d:]

    def fwd(self, q, k, v, want_probs=False):
        ops, dev = _ops(), self.dev
        Lq, Lk, d = q.shape[1], k.shape[1], k.shape[-1]
        qd, kd, vd = self._operands(q, k, v)
        obuf = torch.full((N, Lq + GUARD, d), SENTINEL, device=dev, dtype=self.dt)
        n_lse, n_map = N * H * Lq * 2, N * H * Lq * Lk
        lbuf = torch.full((n_lse + 64,), SENTINEL, device=dev)
        pbuf = torch.full((n_map + 64,), SENTINEL, device=dev) if want_probs else None
        out, lse = obuf[:, :Lq], lbuf[:n_lse].view(N, H, Lq, 2)
        probs = pbuf[:n_map].view(N, H, Lq, Lk) if want_probs else None
        ops.attn_fwd(qd, kd, vd, H, want_probs=want_probs, outs=(out, lse, probs), **self.kw)
        self._tail('out', obuf, Lq)
        self._flat_tail('row statistics', lbuf, n_lse)
        if want_probs:
            self._flat_tail('map', pbuf, n_map)
        return out.float().cpu(), (qd, kd, vd, out, lse), (probs.cpu() if want_probs else None)

    def bwd(self, state, dO):
        ops, dev = _ops(), self.dev
        qd, kd, vd, out, lse = state
        Lq, Lk, d = qd.shape[1], kd.shape[1], kd.shape[-1]
        dbuf = torch.zeros((N, Lq + GUARD, d), device=dev, dtype=self.dt)          # dO in out's strides
        dbuf[:, :Lq] = dO.to(dev).to(self.dt)
        if self.layout == 'self':
            g = torch.full((N, Lq + GUARD, 3 * d), SENTINEL, device=dev, dtype=self.dt)
            bufs = (g, g, g)
            grads = tuple(g[:, :Lq, i * d:(i + 1) * d] for i in range(3))
        else:
            bufs = tuple(torch.full((N, L + GUARD, d), SENTINEL, device=dev, dtype=self.dt) for L in (Lq, Lk, Lk))
            grads = tuple(b[:, :L] for b, L in zip(bufs, (Lq, Lk, Lk)))
        ops.attn_bwd(qd, kd, vd, out, lse, dbuf[:, :Lq], H, grads_out=grads, **self.kw)
        for name, b, L in zip(('dq', 'dk', 'dv'), bufs, (Lq, Lk, Lk)):
            self._tail(name, b, L)
        return tuple(t.float().cpu() for t in grads)


# ---------------------------------------------------------------------------------------------------------------- 1. the applied mask
@pytest.mark.parametrize('mode,dh', MODES)
@pytest.mark.parametrize('shape', A.SHAPES, ids=_id)
def test_applied_mask_equals_the_contract(dev, shape, mode, dh):
    Lq, Lk, layout = shape
    emul_mode = 'x3' if mode == 'x3p' else mode
    for p in (A.P_MAIN, A.P_ALT):
        truth = A.true_mask(N, H, Lq, Lk, p)
        for want_probs in (False, True):
            kern = DeviceKernel(dev, mode, layout, p)
            res = A.read_offs(kern, N, H, Lq, Lk, layout, dh, p, want_probs)
            bad = A.failures(res, truth, Lk, p, emul_mode) + kern.bad
            assert bad == [], (mode, dh, shape, p, want_probs, kernel_names(mode, dh, Lq, Lk, p, want_probs))


# ---------------------------------------------------------------------------------------------------------------- 2. values
@functools.lru_cache(maxsize=None)
def _case(shape, dh, mode):
    """operands and the fp64 reference (test_x3_gpu._attn_ref with the emulated mask, gradients by autograd), once per shape and input kind"""
    from test_x3_gpu import _attn_ref
    Lq, Lk, layout = shape
    gen = torch.Generator().manual_seed(Lq * 1000 + Lk + dh)
    q, k, v, dO = A.random_operands(N, H, Lq, Lk, layout, dh, mode, gen)
    mask = A.true_mask(N, H, Lq, Lk, A.P_MAIN).double()
    q64, k64, v64 = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    o_ref, p_ref, _ = _attn_ref(q64.expand(N, Lq, H * dh), k64, v64, H, mask, util.keep_scale(A.P_MAIN))
    (o_ref * dO.double()).sum().backward()
    return (q, k, v, dO), dict(out=o_ref.detach(), map=p_ref.detach(), dq=q64.grad, dk=k64.grad, dv=v64.grad)


def _run(dev, mode, shape, ops_):
    q, k, v, dO = ops_
    kern = DeviceKernel(dev, mode, shape[2], A.P_MAIN)
    out_m, _, pm = kern.fwd(q, k, v, True)
    out, st, _ = kern.fwd(q, k, v, False)
    dq, dk, dv = kern.bwd(st, dO)
    assert kern.bad == []
    return dict(out_with_map=out_m, map=pm, out=out, dq=dq.sum(0, keepdim=True) if shape[2] == 'shared' else dq, dk=dk, dv=dv)


@pytest.mark.parametrize('mode,dh', MODES)
@pytest.mark.parametrize('shape', A.SHAPES, ids=_id)
def test_values_against_fp64_with_the_same_mask(dev, shape, mode, dh):
    emul_mode = 'x3' if mode == 'x3p' else mode
    ops_, ref = _case(shape, dh, emul_mode)
    got = _run(dev, mode, shape, ops_)
    band = A.BANDS[emul_mode]
    errs = [('out', rel_err(got['out'], ref['out']), band['out']), ('out (map form)', rel_err(got['out_with_map'], ref['out']), band['out']),
            ('map', max_err(got['map'], ref['map']), band['map'])]
    errs += [(x, rel_err(got[x], ref[x]), band['grad']) for x in ('dq', 'dk', 'dv')]
    if mode == 'x3p':               # the backward on planes against the backward on fp32 operands (the forwards are bit-identical)
        base = _run(dev, 'x3', shape, ops_)
        assert torch.equal(got['out'], base['out']) and torch.equal(got['map'], base['map'])
        errs += [(x + ' vs fp32 operands', rel_err(got[x], base[x].double()), A.PLANES_VS_FP32_OPERANDS) for x in ('dq', 'dk', 'dv')]
    print('%-6s dh %2d %-16s %s' % (mode, dh, _id(shape), '  '.join('%s %.2e / %.0e' % e for e in errs)))
    for name, err, bound in errs:
        assert err < bound, (name, err, bound)


# ---------------------------------------------------------------------------------------------------------------- 3. kernel forms
def test_the_cases_reach_every_dropout_form():
    """the (forward, backward) kernels of every case above, by the dispatch rule the plans use; what a trace of this file recorded is listed in
    profiles/attn_dropout_mi355x.txt"""
    names = set()
    for mode, dh in MODES:
        for Lq, Lk, _ in A.SHAPES:
            for want_probs in (False, True):
                names.update(kernel_names(mode, dh, Lq, Lk, A.P_MAIN, want_probs))
    tf = ('false', 'true')
    want = {'attn_fwd8_kernel'}
    for kt in (1, 2, 3, 4, 8):
        for dm in (1, 2):
            want.update('x3p_attn_fwd_kernel<%d, %d, %s, %d>' % (kt, 8 if kt == 8 else 4, m, dm) for m in tf)
            want.update('x3_attn_bwd_kernel<%d, 64, %s, %d>' % (kt, pl, dm) for pl in tf)
            want.add('x3_attn_bwd_kernel<%d, 32, false, %d>' % (kt, dm))
        for dh in (64, 32):
            want.update('x3_attn_fwd_kernel<%d, %d, %d, %s>' % (kt, dh, 8 if kt == 8 else 4, m) for m in tf)
            for npass, hb in ((3, 'false'), (1, 'true')):
                want.add('attn_fwd_kernel<%d, %d, %d, %s>' % (kt, dh, npass, hb))
                want.add('attn_bwd_kernel<%d, %d, %d, %s>' % (kt, dh, npass, hb))
    want.update('x3p_attn_fwd_kernel<8, 4, %s, 2>' % m for m in tf)          # eight key tiles with at most four query blocks: four waves
    assert want <= names, sorted(want - names)
