"""The guarded optimizer step on the device (csrc/guard.hip; hftt_hip.ops.grad_norm / adam_step_guarded; FusedAdam's max_grad_norm, guard and
weight_decay) against the criteria of tests/guard_emul.py.

Shapes: n in guard_emul.GUARD_N = 1, 3, 4, 5 (tail only, one quad, quad + tail), 1023, 1025 (one workgroup and a partial second one) and
2048 * 256 * 4 + 5 (one quad and one tail element behind the first grid pass of both new kernels).  Families: adam_grad's log-uniform stream,
zeros, +-1e30, +-1e-30, and +Inf / -Inf / NaN planted at element 0, at the last (tail) element and at the end of the last full quad.
"""
import math

import pytest
import torch

import elementwise_emul as E
import guard_emul as G

pytestmark = pytest.mark.gpu

S0 = 5                                              # first step number of the update runs (bias corrections well away from 1)
NORM_CASES = [(n, fam) for n in G.GUARD_N for fam in G.FAMILIES if '@' not in fam or G.plant_index(n, fam.split('@')[1]) is not None]
UPDATE_FAMILIES = ('log_uniform', 'zeros') + G.PLANTED_FAMILIES         # (+-1e30 / +-1e-30: gr * gr leaves fp32 in the second moment of ANY Adam)
UPDATE_CASES = [(n, fam) for n, fam in NORM_CASES if fam in UPDATE_FAMILIES]


def _record(ctl):
    """(norm, coef, apply, skipped, clipped) of the 32-byte record: one copy to the host"""
    w = ctl.cpu()
    f = w.view(torch.float32)
    return float(f[0]), float(f[1]), int(w[2]), int(w[3]) & 0xFFFFFFFF, int(w[4]) & 0xFFFFFFFF


def _buffers(n, dev):
    from hftt_hip import ops
    ctl, ws = ops.guard_buffers(n, dev)
    ws.fill_(float('nan'))                          # the workspace's contents are irrelevant on entry
    return ctl, ws


@pytest.mark.parametrize('n,fam', NORM_CASES, ids=['%d-%s' % c for c in NORM_CASES])
def test_norm_coef_apply_and_counters(dev, n, fam):
    from hftt_hip import ops
    g = G.guard_grad(n, fam).to(dev)
    g0 = g.clone()
    ctl, ws = _buffers(n, dev)
    seen = (0, 0)
    for gs in G.GRAD_SCALES:
        for mx in G.MAX_NORMS:
            ref = G.gnorm_ref(g, gs, mx)
            ops.grad_norm(g, ctl, ws, grad_scale=gs, max_norm=mx)
            norm, coef, apply, skipped, clipped = _record(ctl)
            print('n=%d %s gs=%g max_norm=%g: norm %.9g (fp64 %.17g) coef %.9g (fp64 %.17g) apply %d skipped %d clipped %d'
                  % (n, fam, gs, mx, norm, ref['norm'], coef, ref['coef'], apply, skipped, clipped))
            bad = G.gnorm_check(norm, coef, apply, ref) + G.counters_check(skipped - seen[0], clipped - seen[1], coef, ref)
            assert not bad, (n, fam, gs, mx, bad)
            seen = (skipped, clipped)
            if fam in G.FINITE_FAMILIES:
                assert apply == 1                                       # +-1e30 everywhere is a finite gradient
                assert (norm > 0.0) == (fam != 'zeros')                 # +-1e-30 does not vanish
                if fam == 'zeros':
                    assert coef == 1.0 and norm == 0.0
                if mx == math.inf:
                    assert coef == 1.0
    assert torch.equal(g, g0) or fam.startswith('nan')                  # the gradient is read, never written
    if fam.startswith('nan'):
        assert torch.equal(g.view(torch.int32), g0.view(torch.int32))
    # reproducible: two fresh records from the same input hold the same bits
    a, _ = _buffers(n, dev); b, wsb = _buffers(n, dev)
    ops.grad_norm(g, a, ws, grad_scale=0.25, max_norm=1e-3)
    ops.grad_norm(g, b, wsb, grad_scale=0.25, max_norm=1e-3)
    assert torch.equal(a, b)
    assert int(a[5:].abs().sum()) == 0                                  # the padding words stay zero


def _grad_of_step(n, fam, k, dev):
    """a planted family alternates planted, clean, planted: the skipped steps must leave no trace and the clean one is step number S0 + 1"""
    return G.guard_grad(n, fam if (fam in G.FINITE_FAMILIES or k != 1) else 'log_uniform', seed=k).to(dev)


@pytest.mark.parametrize('n,fam', UPDATE_CASES, ids=['%d-%s' % c for c in UPDATE_CASES])
def test_update_against_fp64_and_skip_leaves_every_bit(dev, n, fam):
    from hftt_hip import ops
    grads = [_grad_of_step(n, fam, k, dev) for k in range(3)]
    state0 = [t.to(dev) for t in E.adam_state(n, 17 + n % 1000)]
    for wd in G.WEIGHT_DECAYS:
        for gs in G.GRAD_SCALES:
            for mx in (math.inf, 1e-3):
                p, m, v = (t.clone() for t in state0)
                ctl, ws = _buffers(n, dev)
                skipped_before = 0
                for k, g in enumerate(grads):
                    ops.grad_norm(g, ctl, ws, grad_scale=gs, max_norm=mx)
                    norm, coef, apply, skipped, clipped = _record(ctl)
                    before = (p.clone(), m.clone(), v.clone())
                    ops.adam_step_guarded(p, g, m, v, S0 + k, ctl, lr=E.ADAM_LR, beta1=E.ADAM_B1, beta2=E.ADAM_B2, eps=1e-8, grad_scale=gs, weight_decay=wd)
                    planted = fam in G.PLANTED_FAMILIES and k != 1
                    assert apply == (0 if planted else 1), (n, fam, k)
                    if apply:
                        ref = G.guarded_adam_ref(before[0], g, before[1], before[2], S0 + k, coef, grad_scale=gs, weight_decay=wd)
                        bad = G.guarded_adam_check(p, m, v, ref)
                        assert skipped == skipped_before
                    else:
                        bad = G.skip_check(before, (p, m, v))
                        assert skipped == skipped_before + 1
                    assert not bad, (n, fam, wd, gs, mx, k, coef, bad)
                    skipped_before = skipped
                if fam == 'log_uniform' and mx == 1e-3 and n >= 1023:
                    assert clipped == 3                                  # coef < 1 did occur in this test


@pytest.mark.parametrize('n', G.GUARD_N)
def test_inactive_guard_is_bit_identical_to_adam_step(dev, n):
    '''max_norm = inf, weight_decay = 0, finite gradients: the guarded kernel reproduces adam_kernel's bits'''
    from hftt_hip import ops
    for gs in G.GRAD_SCALES:
        a = [t.to(dev) for t in E.adam_state(n, 3 + n % 1000)]
        b = [t.clone() for t in a]
        ctl, ws = _buffers(n, dev)
        for k in range(3):
            g = E.adam_grad(n, 9, k).to(dev)
            ops.adam_step(*a[:1], g, *a[1:], S0 + k, lr=E.ADAM_LR, grad_scale=gs)
            ops.grad_norm(g, ctl, ws, grad_scale=gs)
            ops.adam_step_guarded(*b[:1], g, *b[1:], S0 + k, ctl, lr=E.ADAM_LR, grad_scale=gs)
            for name, x, y in zip('pmv', a, b):
                assert torch.equal(x, y), (n, gs, k, name, int((x != y).sum()))
        assert _record(ctl)[1:] == (1.0, 1, 0, 0)


# ------------------------------------------------------------------------------------------------ optimizer level
B = 2


@pytest.fixture(scope='module')
def batch(dev):
    import bench
    cfg = bench.CONFIGS['tiny']
    spec, labels = bench.synthetic_batch(cfg, B, 5, dev)
    return cfg, spec, labels


def _train_step(batch, dev, seed=11, **opt_kw):
    import bench
    from hftt_hip.trainer import FusedAdam, TrainStep
    cfg, spec, labels = batch
    model = bench.build_model(cfg, seed, 0.0, dev)             # default precision mode, dropout 0
    model.train()
    opt = FusedAdam(model.parameters(), lr=1e-3, **opt_kw)
    return TrainStep(model, optimizer=opt)


def _state(ts):
    return ts.engine.flat_params.clone(), ts.opt.exp_avg.clone(), ts.opt.exp_avg_sq.clone()


def test_guard_alone_changes_no_bit_of_three_training_steps(dev, batch):
    _, spec, labels = batch
    plain, guarded = _train_step(batch, dev), _train_step(batch, dev, guard=True)
    assert all(torch.equal(a, b) for a, b in zip(_state(plain), _state(guarded)))
    for _ in range(3):
        la, lb = plain(spec, *labels), guarded(spec, *labels)
        assert torch.equal(la, lb)
    for name, a, b in zip(('parameters', 'exp_avg', 'exp_avg_sq'), _state(plain), _state(guarded)):
        assert torch.equal(a, b), name
    assert guarded.opt.skipped_steps == 0 and guarded.opt.clipped_steps == 0
    assert guarded.opt.grad_norm.device.type == 'cuda' and guarded.opt.grad_norm.dim() == 0
    assert 0.0 < float(guarded.opt.grad_norm) < math.inf and float(guarded.opt.clip_coef) == 1.0


def test_an_inf_in_the_flat_gradient_skips_the_step(dev, batch):
    _, spec, labels = batch
    ts = _train_step(batch, dev, guard=True)
    ts.forward_backward(spec, *labels)
    ts.engine.flat_grads[ts.engine.flat_grads.numel() // 2] = float('inf')
    before = _state(ts)
    ts.opt.step()
    assert not G.skip_check(before, _state(ts))
    assert ts.opt.skipped_steps == 1 and ts.opt.clipped_steps == 0
    assert float(ts.opt.clip_coef) == 0.0 and not math.isfinite(float(ts.opt.grad_norm))
    assert ts.opt.step_count == 1 and float(ts.opt.state[ts.opt._params()[0]]['step']) == 1.0        # a skipped step still counts as a call
    ts(spec, *labels)                                            # a clean step moves the parameters
    after = _state(ts)
    assert not torch.equal(before[0], after[0]) and bool(torch.isfinite(after[0]).all())
    assert ts.opt.skipped_steps == 1 and ts.opt.step_count == 2


def test_clipping_to_a_tenth_of_the_norm(dev, batch):
    _, spec, labels = batch
    ts = _train_step(batch, dev, guard=True)
    ts.forward_backward(spec, *labels)
    grads = ts.engine.flat_grads.clone()
    measured = G.gnorm_ref(grads)['norm']
    assert measured > 0.0
    ts.opt.param_groups[0]['max_grad_norm'] = measured / 10.0
    ts.opt.step()
    ref = G.gnorm_ref(grads, 1.0, measured / 10.0)
    coef = float(ts.opt.clip_coef)
    print('norm %.9g (fp64 %.17g), coef %.9g (fp64 %.17g)' % (float(ts.opt.grad_norm), ref['norm'], coef, ref['coef']))
    assert not G.gnorm_check(float(ts.opt.grad_norm), coef, 1, ref)
    assert abs(coef - 0.1) <= 0.1 * 1e-6 / measured + ref['b_coef']     # 0.1 up to the 1e-6 of the formula: 0.1 norm / (norm + 1e-6)
    assert ts.opt.clipped_steps == 1 and ts.opt.skipped_steps == 0
    assert torch.equal(ts.engine.flat_grads, grads)              # the factor lives in the Adam kernel: g is not rewritten
    ts.expose_grads()
    for name, p, o, n in ts.engine._bound:
        assert torch.equal(p.grad.reshape(-1), grads[o:o + n]), name


def test_grad_scale_is_part_of_the_norm(dev, batch):
    _, spec, labels = batch
    ts = _train_step(batch, dev, guard=True)
    ts.forward_backward(spec, *labels)
    full = G.gnorm_ref(ts.engine.flat_grads, 1.0)
    half = G.gnorm_ref(ts.engine.flat_grads, 0.5)
    ts.opt.step(grad_scale=0.5)
    assert not G.gnorm_check(float(ts.opt.grad_norm), float(ts.opt.clip_coef), 1, half)
    assert abs(float(ts.opt.grad_norm) - full['norm'] / 2) <= half['b_norm']


def test_state_dict_round_trip_keeps_counters_options_and_the_next_step(dev, batch):
    import bench
    from hftt_hip.trainer import FusedAdam, TrainStep
    cfg, spec, labels = batch
    a = _train_step(batch, dev, max_grad_norm=1e-4, weight_decay=0.01)
    a.forward_backward(spec, *labels)
    a.engine.flat_grads[3] = float('nan')
    a.opt.step()                                                 # skipped
    a(spec, *labels)                                             # clipped (the norm of a batch at initialisation is far above 1e-4)
    assert (a.opt.skipped_steps, a.opt.clipped_steps) == (1, 1)
    sd = a.opt.state_dict()
    assert sd['hftt_guard'] == {'skipped': 1, 'clipped': 1}
    model_b = bench.build_model(cfg, 99, 0.0, dev)
    model_b.load_state_dict(a.model.state_dict())
    model_b.train()
    opt_b = FusedAdam(model_b.parameters(), lr=5e-4)             # built WITHOUT the options: the state brings them
    b = TrainStep(model_b, optimizer=opt_b)
    opt_b.load_state_dict(sd)
    ga, gb = a.opt.param_groups[0], opt_b.param_groups[0]
    for k in ('lr', 'max_grad_norm', 'weight_decay', 'decoupled_weight_decay', 'guard', 'betas', 'eps'):
        assert ga[k] == gb[k], k
    assert gb['max_grad_norm'] == 1e-4 and gb['weight_decay'] == 0.01 and gb['decoupled_weight_decay'] is True
    assert (opt_b.skipped_steps, opt_b.clipped_steps) == (1, 1) and opt_b.step_count == a.opt.step_count == 2
    assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))
    la, lb = a(spec, *labels), b(spec, *labels)
    assert torch.equal(la, lb)
    for name, x, y in zip(('parameters', 'exp_avg', 'exp_avg_sq'), _state(a), _state(b)):
        assert torch.equal(x, y), name
    assert (opt_b.skipped_steps, opt_b.clipped_steps) == (a.opt.skipped_steps, a.opt.clipped_steps) == (1, 2)
