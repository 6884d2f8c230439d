"""The per-tensor fp64 bound of the x3 gradients (tests/x3_emul.py) has the resolution it is meant to have, without a GPU.

For every gradient tensor t:  e_dev <= 3 * (e32 + e_x3) + 1e-6,  each e the max error against an fp64 evaluation relative to max |g64|:
e32 of the CPU fp32 oracle (fp32 summation noise), e_x3 of the fp64 model of x3's roundings (what x3's operand and storage roundings predict).
Here x3's arithmetic summed in fp32 stands in for a correct device and must pass; three deliberately wrong variants must fail beyond the first
encoder layer while passing the old 3e-2-of-the-tensor-max band against the fp32 oracle -- the defects that band cannot see."""
import dataclasses

import pytest
import torch

import util
import x3_emul as X
from util import O, MINI

_WIDE = dict(n_margin=4, cnn_channel=4, cnn_kernel=5, hid_dim=256, pf_dim=512, enc_layer=1, dec_layer=2, enc_head=4, dec_head=4, n_velocity=16)
# MINI runs on the block plans (FFN hidden and pre-LayerNorm sums fp32); d = 256 / ff = 512 on the strip plans (both stored as bf16)
CONFIGS = {'mini': (MINI, X.Switches()),
           'd256': (O.HfttConfig(n_frame=16, n_bin=32, n_note=8, **_WIDE), X.Switches(hidden_bf16=True, pre_ln_bf16=True))}
B, P, SEED = 2, 0.1, 777
OLD_BAND = 3e-2


@pytest.fixture(scope='module')
def runs():
    """the reference passes of each configuration, computed once per module"""
    return {}


def _case(runs, name):
    if name in runs:
        return runs[name]
    cfg, sw = CONFIGS[name]
    model = util.build_model(cfg, 31, dropout=P)
    util.perturb(model, 32)
    sd = util.sd_cpu(model)
    x = O.synth_spec(B, cfg, salt=13) * 0.5
    labels = O.synth_labels(B, cfg, salt=14)
    n = [0]

    def count(t, pp, training):
        n[0] += bool(training and pp > 0.0)
        return t
    mp = pytest.MonkeyPatch()
    mp.setattr(O, '_drop', count)
    O.model_forward(sd, x, cfg, p=P, training=True)
    drop = X.masked_drop(SEED, n[0])
    mp.setattr(O, '_drop', drop)
    ref = {}
    for key, dt, s in (('g64', torch.float64, None), ('g32', torch.float32, None), ('gx3', torch.float64, sw)):
        ref[key] = X.grads(sd, x, labels, cfg, dt, s, p=P, training=True)[2]
        drop.reset()
    mp.undo()
    runs[name] = dict(cfg=cfg, sw=sw, sd=sd, x=x, labels=labels, n_sites=n[0], **ref)
    return runs[name]


def _device_standin(c, sw, scale_of=None):
    """x3's arithmetic summed in fp32, with the same masks (scale_of: the kept elements' scale per site)"""
    mp = pytest.MonkeyPatch()
    mp.setattr(O, '_drop', X.masked_drop(SEED, c['n_sites'], scale_of))
    try:
        return X.grads(c['sd'], c['x'], c['labels'], c['cfg'], torch.float32, sw, p=P, training=True)[2]
    finally:
        mp.undo()


def _old_band(g, c):
    """the dropout-on test's old check: max |g - g32| < 3e-2 of max |g32|, every tensor"""
    return max(X.rel(g[k], c['g32'][k]) for k, r in c['g64'].items() if r.abs().max().item() >= 1e-7 and not k.endswith('fc_k.bias'))


@pytest.mark.parametrize('name', list(CONFIGS))
def test_x3_arithmetic_summed_in_fp32_passes_the_bound(runs, name):
    c = _case(runs, name)
    g = _device_standin(c, c['sw'])
    rep = []
    bad = X.fp64_bound(g, c['g64'], c['g32'], c['gx3'], report=rep)
    print('\n'.join(rep))
    print('%s: worst e_dev %.2e, worst e_dev / (e32 + e_x3) %.2f' % ((name,) + X.summary(g, c['g64'], c['g32'], c['gx3'])))
    assert not bad, bad
    assert _old_band(g, c) < OLD_BAND


def _variant(c, kind):
    if kind == 'grad_hi':                        # HFTT_X3_GRAD_HI's arithmetic: the gradient operand of every GEMM-shaped product as bf16 only
        return _device_standin(c, dataclasses.replace(c['sw'], grad_hi=True))
    if kind == 'ffn_dw_lohi':                    # the lo(dY).hi(X) pass dropped in the FFN weight-gradient products
        return _device_standin(c, dataclasses.replace(c['sw'], ffn_dw_drop_lohi=True))
    # the last dropout site (the FFN output of the last time layer) scales its kept elements by 256/229 instead of 256/230: 0.44 %
    last = c['n_sites']
    return _device_standin(c, c['sw'], lambda s: 256.0 / 229.0 if s == last else util.keep_scale(P))


# ffn_dw_lohi at d = 256 is left out on purpose: the strip plans store the FFN hidden (dW2's X) and dh (dW1's dY) as bf16, so a correct
# implementation already carries a 2^-9 rounding of one factor in those products -- dropping lo(dY) adds one of the same size (measured:
# e_dev / (e32 + e_x3) = 1.7 at worst here, inside the bound).  The bound resolves it where the hidden is fp32, the block plans (MINI: 12 tensors fail).
@pytest.mark.parametrize('name,kind', [('mini', 'grad_hi'), ('d256', 'grad_hi'), ('mini', 'ffn_dw_lohi'), ('mini', 'drop_scale'), ('d256', 'drop_scale')])
def test_defective_x3_variant_fails_the_bound_and_passes_the_old_band(runs, name, kind):
    c = _case(runs, name)
    g = _variant(c, kind)
    bad = [b for b in X.fp64_bound(g, c['g64'], c['g32'], c['gx3']) if not X.is_first_layer(b[0])]
    old = _old_band(g, c)
    worst = max(bad, key=lambda b: b[1] / (b[2] + b[3])) if bad else None
    print('%s / %s: %d tensors beyond the first layer break the bound (worst %s); old band %.2e' % (name, kind, len(bad), worst, old))
    assert bad, 'the bound does not see %s at %s' % (kind, name)
    assert old < OLD_BAND, old
