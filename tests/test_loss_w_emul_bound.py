"""What the criteria of tests/loss_w_emul.py resolve, on the CPU: the fp32 restatement of csrc/loss_w.hip passes its bounds on every case,
every defect of DEFECTS fails on at least one, neutral options reproduce elementwise_emul's loss reference, bounds and restatement exactly,
and the criterion modules (hftt_hip.criteria.BalancedBCELoss, nn.CrossEntropyLoss) evaluated in fp64 are the reference's values, their
autograd gradients its closed forms."""
import pytest
import torch
import torch.nn as nn

import elementwise_emul as E
import loss_w_emul as W

BIG = 10000          # the shapes past a grid pass run the two option sets that cover everything; the small ones run all
CASES = [(sh, op) for sh in W.SHAPES for op in W.OPTION_SETS if sh[2] < BIG or op in ('neutral', 'all')]


@pytest.fixture(scope='module')
def refs():
    cache = {}

    def get(sh, op):
        if (sh, op) not in cache:
            c = W.case(sh, op)
            cache[(sh, op)] = (c, W.loss_w_ref(c))
        return cache[(sh, op)]
    return get


@pytest.mark.parametrize('sh,op', CASES, ids=['%s-V%d-n%d-Nn%d-%s' % (sh[0], sh[1], sh[2], sh[3], op) for sh, op in CASES])
def test_restatement_passes_its_bounds(refs, sh, op):
    c, ref = refs(sh, op)
    out, dp, dv = W.loss_w_emul(c)
    bad = W.loss_w_check(out, dp, dv, ref)
    assert not bad, bad
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t).all()) for t in dp + dv)


DEFECT_CASES = [(sh, op) for sh in W.SHAPES if sh[2] < BIG for op in ('bce', 'ce', 'all')]


@pytest.mark.parametrize('defect', W.DEFECTS)
def test_every_defect_fails_somewhere(refs, defect):
    failing = []
    for sh, op in DEFECT_CASES:
        c, ref = refs(sh, op)
        if W.loss_w_check(*W.loss_w_emul(c, defect=defect), ref):
            failing.append((sh, op))
    print(defect, len(failing), 'of', len(DEFECT_CASES))
    assert failing, defect


@pytest.mark.parametrize('sh', [s for s in W.SHAPES if s[2] < BIG], ids=lambda s: '%s-V%d-n%d' % s[:3])
def test_neutral_options_are_the_existing_yardstick(refs, sh):
    """reference and bounds of the neutral case equal elementwise_emul's for hftt_loss term by term (to fp64 rounding: the two references
    multiply in another order), the fp32 restatement bit by bit"""
    c, ref = refs(sh, 'neutral')
    old = E.loss_ref(c, c['gs'])
    assert torch.allclose(ref['out'][:9], old['out'], rtol=1e-13, atol=0) and torch.allclose(ref['b_out'][:9], old['b_out'], rtol=1e-12, atol=0)
    assert float(ref['out'][9]) == float(ref['out'][10]) == c['n'] and float(ref['b_out'][9]) == 0.0
    for k in ('d_prob', 'd_vel'):
        for a, b in zip(ref[k], old[k]):
            assert torch.allclose(a, b, rtol=1e-13, atol=0)
    for k in ('b_dprob', 'b_dvel'):
        for a, b in zip(ref[k], old[k]):
            assert torch.allclose(a, b, rtol=1e-12, atol=0)
    out, dp, dv = W.loss_w_emul(c)
    out0, dp0, dv0 = E.loss_emul(c, c['gs'])
    assert torch.equal(out[:9], out0) and all(torch.equal(a, b) for a, b in zip(dp + dv, dp0 + dv0))


def _modules(o):
    from hftt_hip.criteria import BalancedBCELoss
    bce = [BalancedBCELoss(pos_weight=1.0 if o['pos_weight'][h] is None else o['pos_weight'][h], gamma=o['gamma'][h]) for h in range(6)]
    ce = [nn.CrossEntropyLoss(weight=None if o['class_weight'][s] is None else o['class_weight'][s].double(), ignore_index=o['ignore'][s],
                              label_smoothing=E.f32(o['smoothing'][s])) for s in range(2)]      # (the fp32 value the kernel is handed)
    return bce, ce


@pytest.mark.parametrize('op', ['bce', 'ce', 'ce_b', 'all'])
@pytest.mark.parametrize('sh', [W.SHAPES[1], W.SHAPES[5], W.SHAPES[9]], ids=lambda s: '%s-V%d-n%d' % s[:3])
def test_the_criterion_modules_are_the_reference(sh, op):
    """fp64: module values equal the reference's terms, autograd gradients its closed forms (posteriors inside [1e-6, 1 - 1e-6], where
    neither the log clamps nor the denominator clamp act); tolerance 1e-12 relative to the tensor's largest entry: fp64 roundings only"""
    c = W.case(sh, op)
    c = dict(c, probs=[q.clamp(1e-6, 1 - 1e-6) for q in c['probs']], gs=1.0)
    ref = W.loss_w_ref(c)
    n = c['n']
    bce, ce = _modules(c['opts'])
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)      # noqa: E731
    for h in range(6):
        p = c['probs'][h].double().requires_grad_(True)
        v = bce[h].double()(p, E._bce_labels(c, h).double())
        k = (1, 2, 3, 5, 6, 7)[h]
        assert close(v.detach(), ref['out'][k]), (h, float(v), float(ref['out'][k]))
        g, = torch.autograd.grad(v, p)
        assert close(g * E.LOSS_W[h // 3], ref['d_prob'][h]), h
    for s in range(2):
        z = c['vel'][s].double().requires_grad_(True)
        v = ce[s](z, c['lv'])
        assert close(v.detach(), ref['out'][(4, 8)[s]]), s
        g, = torch.autograd.grad(v, z)
        assert close(g * E.LOSS_W[s], ref['d_vel'][s]), s
    assert n % c['opts']['Nn'] == 0
