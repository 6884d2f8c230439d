"""An fp64 model of the x3 precision mode's roundings on the oracle graph (test infrastructure, CPU).

The oracle's primitives are patched, not restated: every F.linear / torch.matmul of oracle/hftt_oracle.py runs on the operands x3 gives the
matrix cores, every F.layer_norm saves the input its backward really reads, and the conv + token embedding runs in the fused form the device
runs.  The graph, the loss and the order of the dropout sites stay the oracle's (so O._drop can still be answered with the device's masks).
The working dtype is the parameters' dtype: float64 gives the error x3's roundings predict; float32 (summed in fp32, like the matrix cores) is a
stand-in for a correct device.

Roundings modelled (csrc/x3_common.h, gemm_tn.hip, x3_strip.hip, x3_attn_bwd.h):
  * forward products (every linear, Q.K^T, P.V): both operands split into fp16 hi + lo after the clamp to +-65504 (x3_split2), three passes
    hi.hi + hi.lo + lo.hi (the lo.lo term is dropped);
  * backward products with a gradient operand (dX, dW; dQ, dK, dV, dP): both operands split into bf16 hi + lo, the same three passes;
  * the attention backward's delta = rowsum(dO * O) from the forward's output, not rowsum(P * dP) (x3_attn_bwd.h; see _Softmax);
  * the x3 strip plans (Switches.hidden_bf16 / pre_ln_bf16) store three tensors as bf16 for the backward only:
      - the FFN hidden after ReLU and dropout: the ReLU / dropout gate and the X factor of dW2 (fc_2's forward product reads it at full width
        from registers, x3_mlp_kernel<0>);
      - its gradient dh after the gate: the dY factor of dW1 and the source of db1 (the dX product of fc_1 reads dh at full width from
        registers, x3_mlp_kernel<1>);
      - every pre-LayerNorm sum: the LayerNorm backward recomputes x_hat = (bf16(r) - mean) * rstd with the fp32 statistics of the forward
        (ln_bwd.hip);
    a bf16-stored factor enters its product as its bf16 value alone (no lo half).
  * the conv + token embedding as ONE Linear(n_proc -> d) on the folded weights (the device's hftt_fold + one x3 product).
Not modelled (2^-22 and below): the f16-pair storage of q / k / v, the fp16 pair of the FFN block's residual.  That figure is RELATIVE and
holds for |x| >= 2^-3 only: below it the lo half is an fp16 subnormal and the stored pair is off by up to 2^-25 absolute, which in the
attention backward (bf16 pairs formed from the stored hi + lo) is more than any relative unit on an operand element near zero --
tests/attn_peaked_emul.py models it (chain(planes=True)) and carries it in its bound; the whole-model bound of this file is max-normalised
per tensor and does not resolve it.

Deliberately wrong variants (for the tests that prove the bound has resolution): Switches.grad_hi (the gradient operand of every GEMM-shaped
backward product as its bf16 rounding only: HFTT_X3_GRAD_HI's arithmetic), Switches.ffn_dw_drop_lohi (the lo(dY).hi(X) pass dropped in the
FFN weight-gradient products).
"""
import contextlib
from dataclasses import dataclass

import torch
import torch.nn.functional as _F

import util
from util import O


@dataclass(frozen=True)
class Switches:
    hidden_bf16: bool = False           # FFN hidden and its gradient dh stored as bf16 (engine.hh in a strip workspace)
    pre_ln_bf16: bool = False           # pre-LayerNorm sums stored as bf16 (the same switch in the engine: HfttEngine._lnb r_bf)
    grad_hi: bool = False               # defect / option: the gradient operand as bf16 only
    ffn_dw_drop_lohi: bool = False      # defect: lo(dY).hi(X) dropped in the FFN weight-gradient products


def switches_from_engine(eng, B):
    """The storage switches of the plans the engine built for batch B (a workspace that falls back to the block plans stores nothing as bf16).
    The opt-in HFTT_X3_GRAD_HI is NOT taken over: the model is of what the default arithmetic should give, the option is one of the
    departures from it the bound has to see."""
    hh = bool(eng.hh and eng._ws[B]['strip'])
    return Switches(hidden_bf16=hh, pre_ln_bf16=hh)


FIRST = ('encoder_spec2midi.conv', 'tok_embedding_freq', 'encoder_spec2midi.pos_embedding_freq',
         'layers_freq.0.self_attention.fc_q', 'layers_freq.0.self_attention.fc_k')


def is_first_layer(name):
    """the tensors behind the first encoder layer's attention (ill-conditioned on raw log-mel input: DESIGN.md section 3)"""
    return name.startswith('encoder') and any(t in name for t in FIRST)


# ---------------------------------------------------------------------------------------------------------------------------- split products
def _split(x, fmt):
    dt = x.dtype
    if fmt == 'f16':
        xc = x.clamp(-65504.0, 65504.0)
        hi = xc.half().to(dt)
        return hi, (xc - hi).half().to(dt)
    hi = x.bfloat16().to(dt)
    return hi, (x - hi).bfloat16().to(dt)


def x3mm(a, b, fmt, a_hi=False, b_hi=False, drop_lohi=False):
    """a @ b as x3 runs it: hi.hi + hi.lo + lo.hi, summed in the working dtype.  a_hi / b_hi: that operand enters as its hi half alone
    (bf16-stored, or rounded on purpose); drop_lohi: the lo(a).hi(b) pass is left out."""
    ah, al = _split(a, fmt)
    bh, bl = _split(b, fmt)
    out = torch.matmul(ah, bh)
    if not b_hi:
        out = out + torch.matmul(ah, bl)
    if not (a_hi or drop_lohi):
        out = out + torch.matmul(al, bh)
    return out


def _bf16(x):
    return x.bfloat16().to(x.dtype)


class _Linear(torch.autograd.Function):
    """y = x W^T + b.  role: 'fc1' / 'fc2' (the FFN's two products), 'plain' otherwise."""

    @staticmethod
    def forward(ctx, x, w, b, role, sw):
        ctx.role, ctx.sw = role, sw
        ctx.save_for_backward(x, w)
        y = x3mm(x, w.t(), 'f16')
        return y + b if b is not None else y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        sw, role = ctx.sw, ctx.role
        hh = sw.hidden_bf16
        dx = x3mm(dy, w, 'bf16', a_hi=sw.grad_hi)
        K, N = x.shape[-1], dy.shape[-1]
        x2, dy2 = x.reshape(-1, K), dy.reshape(-1, N)
        dy_hi = sw.grad_hi
        if role == 'fc1' and hh:                 # dh: stored as bf16 after the gate; the dY factor of dW1 and the source of db1
            dy2, dy_hi = _bf16(dy2), True
        x_hi = False
        if role == 'fc2' and hh:                 # the stored hidden: the X factor of dW2
            x2, x_hi = _bf16(x2), True
        dw = x3mm(dy2.t(), x2, 'bf16', a_hi=dy_hi, b_hi=x_hi, drop_lohi=sw.ffn_dw_drop_lohi and role in ('fc1', 'fc2'))
        db = dy2.sum(0) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None, None


class _Matmul(torch.autograd.Function):
    """attention products: Q.K^T and P.V forward (fp16 pairs), dQ / dK / dP / dV backward (bf16 pairs).  link: this is the P.V product of
    the softmax that made the link; its backward leaves delta = rowsum(dO * O) there (see _Softmax)."""

    @staticmethod
    def forward(ctx, a, b, link):
        out = x3mm(a, b, 'f16')
        ctx.link = link
        ctx.save_for_backward(a, b, out)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, out = ctx.saved_tensors
        if ctx.link is not None:
            ctx.link['delta'] = (g * out).sum(-1, keepdim=True)
        return x3mm(g, b.transpose(-1, -2), 'bf16'), x3mm(a.transpose(-1, -2), g, 'bf16'), None


class _Softmax(torch.autograd.Function):
    """The attention softmax.  Its backward dS = P * (dP - delta) takes delta = rowsum(dO * O) from the forward's output O, as the attention
    backward does (x3_attn_bwd.h, phase (a)), not rowsum(P * dP) from the dP it has just formed: dP carries the bf16 pairs' 2^-16 and delta
    does not, so the two no longer cancel where dP - delta is small against dP (the decoder's note self-attention, tested at paper size)."""

    @staticmethod
    def forward(ctx, x, link):
        p = torch.softmax(x, -1)
        ctx.link = link
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, gp):
        p, = ctx.saved_tensors
        delta = ctx.link.pop('delta', None)
        if delta is None:
            delta = (p * gp).sum(-1, keepdim=True)
        return p * (gp - delta), None


class _LayerNorm(torch.autograd.Function):
    """LayerNorm whose backward recomputes x_hat from the SAVED pre-LayerNorm sum (bf16 in the strip plans) and the forward's statistics"""

    @staticmethod
    def forward(ctx, x, w, b, eps, pre_bf16):
        mean = x.mean(-1, keepdim=True)
        rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
        ctx.save_for_backward(_bf16(x) if pre_bf16 else x, mean, rstd, w)
        return (x - mean) * rstd * w + b

    @staticmethod
    def backward(ctx, dy):
        xs, mean, rstd, w = ctx.saved_tensors
        xh = (xs - mean) * rstd
        gy = dy * w
        dx = rstd * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))
        red = tuple(range(dy.dim() - 1))
        return dx, (dy * xh).sum(red), dy.sum(red), None, None


def _folded(cw, cb, tw, tb, n_proc):
    """conv (C x 1 x 1 x k) + flatten + Linear(C * nw -> d) as one Linear(n_proc -> d), differentiable in all four parameters"""
    C_, kk = cw.shape[0], cw.shape[3]
    nw = n_proc - (kk - 1)
    d = tw.shape[0]
    tw3 = tw.view(d, C_, nw)
    weff = sum(_F.pad(tw3[:, c, :] * cw[c, 0, 0, t], (t, kk - 1 - t)) for c in range(C_) for t in range(kk))
    beff = tb + (tw3 * cb.view(1, C_, 1)).sum((1, 2))
    return weff, beff


class _Proxy:
    def __init__(self, base, **over):
        self._base, self._over = base, over

    def __getattr__(self, k):
        return self._over[k] if k in self._over else getattr(self._base, k)


@contextlib.contextmanager
def emulate(sd, sw=Switches()):
    """Within this context the oracle (O.model_forward with the parameter dict `sd`) runs x3's arithmetic."""
    role = {}
    for k, v in sd.items():
        role[id(v)] = ('fc1' if k.endswith('positionwise_feedforward.fc_1.weight') else 'fc2' if k.endswith('positionwise_feedforward.fc_2.weight')
                       else 'tok' if k.endswith('tok_embedding_freq.weight') else 'plain')
    conv = {}

    def conv2d(x, w, b, *a, **kw):
        conv['win'], conv['w'], conv['b'] = x, w, b
        return _F.conv2d(x, w, b, *a, **kw)            # (its value feeds nothing but the token linear below, which does not read it)

    def linear(x, w, b=None):
        r = role.get(id(w), 'plain')
        if r == 'tok':
            win = conv.pop('win')
            n_proc = win.shape[-1]
            weff, beff = _folded(conv.pop('w'), conv.pop('b'), w, b, n_proc)
            return _Linear.apply(win.reshape(win.shape[0], win.shape[2], n_proc), weff, beff, 'plain', sw)
        return _Linear.apply(x, w, b, r, sw)

    def layer_norm(x, shape, w, b, eps):
        return _LayerNorm.apply(x, w, b, eps, sw.pre_ln_bf16)

    pending = []

    def softmax(x, dim):
        assert dim in (-1, x.dim() - 1) and not pending
        link = {}
        pending.append(link)                           # the next product is this softmax's P.V (oracle mha: softmax -> dropout -> matmul)
        return _Softmax.apply(x, link)

    def matmul(a, b):
        return _Matmul.apply(a, b, pending.pop() if pending else None)

    F_, T_ = O.F, O.torch
    O.F = _Proxy(_F, linear=linear, layer_norm=layer_norm, conv2d=conv2d)
    O.torch = _Proxy(torch, matmul=matmul, softmax=softmax)
    try:
        yield
    finally:
        O.F, O.torch = F_, T_


# ---------------------------------------------------------------------------------------------------------------------------- evaluations
def grads(sd, x, labels, cfg, dtype, sw=None, p=0.0, training=False, wA=1.0, wB=1.0):
    """(outputs, loss, {name: gradient as a flat float64 tensor}) of one oracle step in `dtype`; sw: run x3's arithmetic (see emulate)"""
    prm = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    ctx = emulate(prm, sw) if sw is not None else contextlib.nullcontext()
    with ctx:
        out = O.model_forward(prm, x.to(dtype), cfg, p=p, training=training)
        loss = O.spec2midi_loss(out, *labels, wA, wB)
        loss.backward()
    g = {k: v.grad.detach().double().reshape(-1) for k, v in prm.items() if v.grad is not None}
    return [t.detach() for t in out], loss.item(), g


def rel(g, g64):
    """max |g - g64| / max |g64|"""
    return ((g.double() - g64).abs().max() / g64.abs().max()).item()


def fp64_bound(g_dev, g64, g32, gx3, factor=3.0, report=None, label=''):
    """The per-tensor bound e_dev <= factor * (e32 + e_x3) + 1e-6 over every gradient tensor with max |g64| >= 1e-7 (the fc_k biases have an
    exactly-zero gradient).  Returns the list of (name, e_dev, e32, e_x3) that break it; prints one line per tensor when report is given
    (a list that collects the lines)."""
    bad = []
    for name, r in g64.items():
        if r.abs().max().item() < 1e-7 or name.endswith('fc_k.bias'):
            continue
        e_dev, e32, ex3 = rel(g_dev[name], r), rel(g32[name], r), rel(gx3[name], r)
        resid = ((g_dev[name].double() - gx3[name]).abs().max() / r.abs().max()).item()
        if report is not None:
            report.append('%s%-66s e_dev %.2e  e32 %.2e  e_x3 %.2e  e_dev/e32 %7.2f  e_dev/(e32+e_x3) %5.2f  dev-x3 %.2e%s' % (
                label, name, e_dev, e32, ex3, e_dev / max(e32, 1e-30), e_dev / (e32 + ex3 + 1e-30), resid,
                '  FIRST' if is_first_layer(name) else ''))
        if not e_dev <= factor * (e32 + ex3) + 1e-6:
            bad.append((name, e_dev, e32, ex3))
    return bad


def summary(g_dev, g64, g32, gx3):
    """(worst e_dev, worst e_dev / (e32 + e_x3)) over the tensors the bound covers"""
    we, wr = 0.0, 0.0
    for name, r in g64.items():
        if r.abs().max().item() < 1e-7 or name.endswith('fc_k.bias'):
            continue
        e_dev = rel(g_dev[name], r)
        we, wr = max(we, e_dev), max(wr, e_dev / (rel(g32[name], r) + rel(gx3[name], r) + 1e-30))
    return we, wr


def masked_drop(seed, n_sites, scale_of=None):
    """An O._drop that answers the oracle's dropout calls, in order, with the device generator's masks for sites 1 .. n_sites (computed once,
    kept for the next pass; scale_of(site) -> the kept elements' scale, default util.keep_scale(p))"""
    cache = {}
    state = {'site': 0}

    def drop(t, pp, training):
        if not (training and pp > 0.0):
            return t
        state['site'] += 1
        s = state['site']
        assert s <= n_sites, 'the oracle made more dropout calls than the engine has sites'
        if s not in cache:
            cache[s] = util.keep_mask_t(seed, s, tuple(t.shape), pp)
        sc = scale_of(s) if scale_of is not None else util.keep_scale(pp)
        return t * cache[s].to(t.dtype) * sc

    def reset():
        assert state['site'] in (0, n_sites), 'the oracle made %d dropout calls, the engine has %d sites' % (state['site'], n_sites)
        state['site'] = 0
    drop.reset = reset
    return drop
