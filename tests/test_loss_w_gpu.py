"""hftt_loss_w (csrc/loss_w.hip) on the device against fp64 under the rounding-model criteria of tests/loss_w_emul.py (derivations there;
tests/test_loss_w_emul_bound.py shows on the CPU what they resolve): both kernel forms with their grid-stride loops, every option, the label
pre-pass and its W = 0 case, null gradient pointers, run-to-run bits, bit-for-bit neutrality against hftt_loss head by head and side by side,
then the engine (eng.loss(spec=...)) and training.train.train on the fused path with a BalancedBCELoss + weighted CrossEntropyLoss tuple."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import elementwise_emul as E
import loss_w_emul as W

pytestmark = pytest.mark.gpu
GUARD = -8192.0


def _lib():
    from hftt_hip import _capi
    return _capi, _capi.lib()


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _guarded(dev, numel, off, fill=None):
    """a flat buffer with one guard element after (and `off` before) the view the kernel gets; off = 1: the view is not 16-byte aligned"""
    buf = torch.full((numel + off + 1,), GUARD, device=dev)
    view = buf[off:off + numel]
    if fill is not None:
        view.copy_(fill.reshape(-1))
    return buf, view


def _launch(dev, c, kernel, grads=True, opts='own'):
    """opts='own': hftt_loss_w with the case's options; None: hftt_loss itself on the same inputs.
    Returns out[11], d_prob[6], d_vel[2] and the d_vel buffers with their guards."""
    capi, L = _lib()
    n, V = c['n'], c['V']
    off = 1 if kernel == 'general_unaligned' else 0
    dw = capi.LossWDesc()
    d = dw.base
    d.n, d.V = n, V
    dp = [q.to(dev).contiguous() for q in c['probs']]
    gp = [torch.full((n,), float('nan'), device=dev) for _ in range(6)]
    vel = [_guarded(dev, n * V, off, t.to(dev)) for t in c['vel']]
    gv = [_guarded(dev, n * V, off) for _ in range(2)]
    for i in range(6):
        d.prob[i], d.d_prob[i] = dp[i].data_ptr(), (gp[i].data_ptr() if grads else None)
    for i in range(2):
        d.vel[i], d.d_vel[i] = vel[i][1].data_ptr(), (gv[i][1].data_ptr() if grads else None)
    labs = (c['lo'].to(dev), c['lf'].to(dev), c['lm'].to(dev), c['lv'].to(dev))
    d.label_onset, d.label_offset, d.label_mpe, d.label_velocity = (t.data_ptr() for t in labs)
    d.weight_A, d.weight_B, d.grad_scale = E.LOSS_W[0], E.LOSS_W[1], c['gs']
    out = torch.full((16,), GUARD, device=dev)
    ws = torch.empty(L.hftt_loss_ws_bytes(n) // 4 + 16, device=dev)
    d.loss_out, d.ws = out.data_ptr(), ws.data_ptr()
    if opts is None:
        capi.check(L.hftt_loss(C.byref(d), _st(dev)), 'loss')
    else:
        o = c['opts']
        tabs = [None if t is None else t.to(dev).contiguous() for t in o['pos_weight'] + o['class_weight']]
        ws_w = torch.empty(L.hftt_loss_w_ws_bytes(n) // 4, device=dev)
        dw.Nn, dw.ws_w = o['Nn'], ws_w.data_ptr()
        for i in range(6):
            dw.pos_weight[i], dw.gamma[i] = (None if tabs[i] is None else tabs[i].data_ptr()), o['gamma'][i]
        for s in range(2):
            dw.class_weight[s] = None if tabs[6 + s] is None else tabs[6 + s].data_ptr()
            dw.smoothing[s], dw.ignore_index[s] = o['smoothing'][s], o['ignore'][s]
        capi.check(L.hftt_loss_w(C.byref(dw), _st(dev)), 'loss_w')
    torch.cuda.synchronize(dev)
    assert bool((out[11 if opts is not None else 9:] == GUARD).all())          # loss_out: eleven floats (hftt_loss: nine), no more
    assert (gv[0][1].data_ptr() % 16 != 0) == (kernel == 'general_unaligned')
    return out[:11].clone(), gp, [b[1].view(n, V) for b in gv], [b[0] for b in gv]


def _on(dev, c):
    return dict(c, probs=[t.to(dev) for t in c['probs']], vel=[t.to(dev) for t in c['vel']], lo=c['lo'].to(dev), lf=c['lf'].to(dev),
                lm=c['lm'].to(dev), lv=c['lv'].to(dev))


# every shape under the two option sets that cover everything, the others on one shape of each kernel form
CASES = ([(sh, op) for sh in W.SHAPES for op in ('neutral', 'all')]
         + [(sh, op) for sh in (W.SHAPES[1], W.SHAPES[5], W.SHAPES[9], W.SHAPES[10]) for op in ('onset_A_only', 'bce', 'ce', 'ce_b', 'ignore_all')])
IDS = ['%s-V%d-n%d-Nn%d-%s' % (sh[0], sh[1], sh[2], sh[3], op) for sh, op in CASES]


@pytest.mark.parametrize('sh,op', CASES, ids=IDS)
def test_loss_w_against_fp64(dev, sh, op):
    """loss_out[0..10] and all eight gradient tensors within the derived bounds; nothing written past the views; everything finite (W = 0: zeros)"""
    c = W.case(sh, op)
    ref = W.loss_w_ref(_on(dev, c))
    out, gp, gv, bufs = _launch(dev, c, sh[0])
    print(op, sh, out.tolist())
    bad = W.loss_w_check(out, gp, gv, ref)
    assert not bad, (sh, op, bad)
    off = 1 if sh[0] == 'general_unaligned' else 0
    assert all(float(b[-1]) == GUARD and (off == 0 or float(b[0]) == GUARD) for b in bufs)
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t).all()) for t in gp + gv)
    if op == 'ignore_all':
        assert float(out[4]) == 0.0 and float(out[9]) == 0.0 and not bool(gv[0].any())          # W_A = 0: the term and its gradient are zeros
        assert float(out[10]) == sh[2] and float(out[8]) > 0.0                                    # side B ignores an index no label has


@pytest.mark.parametrize('sh', W.SHAPES, ids=lambda s: '%s-V%d-n%d-Nn%d' % s[:4])
def test_neutral_options_are_hftt_loss_bit_for_bit(dev, sh):
    """all options neutral: every output equals hftt_loss's; only onset_A weighted: the other seven terms and gradient tensors still do;
    a neutral side A beside a weighted, smoothed, ignoring side B (a call WITH the pre-pass): side A and the six BCE heads still do"""
    c = W.case(sh, 'neutral')
    out0, gp0, gv0, _ = _launch(dev, c, sh[0], opts=None)
    out, gp, gv, _ = _launch(dev, c, sh[0])
    assert torch.equal(out[:9], out0[:9]) and float(out[9]) == float(out[10]) == sh[2]
    assert all(torch.equal(a, b) for a, b in zip(gp + gv, gp0 + gv0))
    # a table of ones is as neutral as no table
    ones = dict(c, opts=dict(c['opts'], pos_weight=[torch.ones(sh[3])] * 6))
    out1, gp1, gv1, _ = _launch(dev, ones, sh[0])
    assert torch.equal(out1, out) and all(torch.equal(a, b) for a, b in zip(gp1 + gv1, gp + gv))
    c1 = W.case(sh, 'onset_A_only')
    out1, gp1, gv1, _ = _launch(dev, c1, sh[0])
    assert torch.equal(out1[2:9], out0[2:9]) and not torch.equal(out1[1], out0[1])
    assert all(torch.equal(a, b) for a, b in zip(gp1[1:] + gv1, gp0[1:] + gv0)) and not torch.equal(gp1[0], gp0[0])
    c2 = W.case(sh, 'ce_b')                                  # (its labels differ: hftt_loss on ITS labels is the yardstick)
    out0, gp0, gv0, _ = _launch(dev, c2, sh[0], opts=None)
    out2, gp2, gv2, _ = _launch(dev, c2, sh[0])
    assert torch.equal(out2[1:8], out0[1:8]) and float(out2[9]) == sh[2] and float(out2[10]) != sh[2]      # (W_B: a sum of weights)
    assert all(torch.equal(a, b) for a, b in zip(gp2 + gv2[:1], gp0 + gv0[:1])) and not torch.equal(gv2[1], gv0[1])


@pytest.mark.parametrize('sh', [W.SHAPES[1], W.SHAPES[9], W.SHAPES[10]], ids=lambda s: '%s-V%d-n%d' % s[:3])
def test_null_gradient_pointers_and_run_to_run_bits(dev, sh):
    """the validation loss: every d_* NULL writes nothing and gives the same eleven values, bit for bit; two runs are bit-identical (the W
    pre-pass has a fixed summation order)"""
    c = W.case(sh, 'all')
    full, gp, gv, _ = _launch(dev, c, sh[0])
    again, gp2, gv2, _ = _launch(dev, c, sh[0])
    assert torch.equal(full, again) and all(torch.equal(a, b) for a, b in zip(gp + gv, gp2 + gv2))
    out, gpn, _, bufs = _launch(dev, c, sh[0], grads=False)
    assert torch.equal(out, full)
    assert all(bool(torch.isnan(t).all()) for t in gpn) and all(bool((b == GUARD).all()) for b in bufs)


# ------------------------------------------------------------------------------------------------ engine and trainer
B = 2


def _criteria(cfg, dev, smoothing=0.125):
    """BalancedBCELoss on five heads (one plain nn.BCELoss), weighted / smoothed / ignoring cross-entropies (smoothing 1/8: exact in fp32)"""
    from hftt_hip.criteria import BalancedBCELoss
    ramp = (0.5 * 16.0 ** (torch.arange(cfg.n_note, dtype=torch.float64) / (cfg.n_note - 1))).float()
    cw = torch.ones(cfg.n_velocity)
    cw[0] = 0.1
    return (BalancedBCELoss(pos_weight=4.0, gamma=2.0), BalancedBCELoss(pos_weight=ramp, gamma=1.0), nn.BCELoss(),
            nn.CrossEntropyLoss(weight=cw.to(dev)),
            BalancedBCELoss(pos_weight=ramp, gamma=1.5), BalancedBCELoss(gamma=2.0), BalancedBCELoss(pos_weight=0.5),
            nn.CrossEntropyLoss(weight=cw.to(dev), label_smoothing=smoothing, ignore_index=3))


@pytest.fixture(scope='module')
def forwarded(dev):
    import bench
    cfg = bench.CONFIGS['tiny']
    spec, labels = bench.synthetic_batch(cfg, B, 5, dev)
    model = bench.build_model(cfg, 11, 0.0, dev)
    model.train()
    eng = model.hftt_engine()
    with torch.cuda.device(dev):
        eng.forward(spec, training=True, save=True)
    return cfg, model, eng, labels


def test_engine_loss_with_a_spec_against_the_criterion_modules(dev, forwarded):
    """eng.forward -> eng.loss(spec=...): loss9, W and the d.* buffers against the fp64 evaluation of the criterion modules (value and autograd
    gradient) on the engine's own outputs, within the bounds of loss_w_ref for those inputs"""
    from hftt_hip.criteria import LossSpec
    cfg, model, eng, labels = forwarded
    crits = _criteria(cfg, dev)
    spec = LossSpec.from_criteria(crits, eng.N, eng.V, dev)
    assert isinstance(spec, LossSpec) and spec.needs_prepass
    n, V = B * eng.T * eng.N, eng.V
    loss9 = eng.loss(B, labels, E.LOSS_W[0], E.LOSS_W[1], with_grad=True, spec=spec)
    torch.cuda.synchronize(dev)
    outs, bufs = eng._ws[B]['outs'], eng._ws[B]['bufs']
    probs = [outs[k].reshape(-1).float() for k in (0, 1, 2, 5, 6, 7)]
    vel = [outs[k].reshape(n, V).float() for k in (3, 8)]
    lo, lf, lm, lv = (t.reshape(-1) for t in labels)
    c = dict(probs=probs, vel=vel, lo=lo, lf=lf, lm=lm, lv=lv, n=n, V=V, gs=1.0,
             opts=dict(Nn=eng.N, pos_weight=spec.pos_weight, gamma=spec.gamma, class_weight=spec.class_weight, smoothing=spec.smoothing,
                       ignore=spec.ignore_index))
    ref = W.loss_w_ref(c)
    # the modules in fp64 are the yardstick: their values and autograd gradients replace the closed forms, the bounds stay
    vals, dps, dvs = [], [], []
    for h, k in enumerate((0, 1, 2, 4, 5, 6)):
        p = probs[h].double().requires_grad_(True)
        v = crits[k].double()(p, E._bce_labels(c, h).double())
        vals.append(v.detach()); dps.append(torch.autograd.grad(v, p)[0] * E.LOSS_W[h // 3])
    for s, k in enumerate((3, 7)):
        z = vel[s].double().requires_grad_(True)
        v = crits[k].double()(z, lv)
        vals.append(v.detach()); dvs.append(torch.autograd.grad(v, z)[0] * E.LOSS_W[s])
    t = [vals[0], vals[1], vals[2], vals[6], vals[3], vals[4], vals[5], vals[7]]
    total = E.LOSS_W[0] * sum(t[:4]) + E.LOSS_W[1] * sum(t[4:])
    ref = dict(ref, out=torch.stack([total] + t + [ref['out'][9], ref['out'][10]]), d_prob=dps, d_vel=dvs)
    got = torch.cat([loss9, bufs['loss_out'][9:11]])
    names = ('onset_A', 'offset_A', 'mpe_A', 'onset_B', 'offset_B', 'mpe_B')
    gp = [bufs['d.' + nm].reshape(-1).float() for nm in names]
    gv = [bufs['d.velocity_' + s].reshape(n, V).float() for s in 'AB']
    print(got.tolist())
    bad = W.loss_w_check(got, gp, gv, ref)
    assert not bad, bad
    assert float(got[9]) < n and float(got[10]) < n          # class 0 weighs 0.1, and side B ignores the rows of class 3


def test_engine_loss_without_a_spec_keeps_its_bits(dev, forwarded):
    """eng.loss(spec=None) launches hftt_loss as ever: its nine values and d.* buffers are those of hftt_loss called on the engine's buffers
    directly, and those of a neutral spec"""
    from hftt_hip.criteria import BalancedBCELoss, LossSpec
    capi, L = _lib()
    cfg, model, eng, labels = forwarded
    n, V = B * eng.T * eng.N, eng.V
    outs, bufs = eng._ws[B]['outs'], eng._ws[B]['bufs']
    names = ['d.' + nm for nm in ('onset_A', 'offset_A', 'mpe_A', 'onset_B', 'offset_B', 'mpe_B', 'velocity_A', 'velocity_B')]
    loss9 = eng.loss(B, labels, 0.75, 1.25, with_grad=True).clone()
    grads = [bufs[k].clone() for k in names]
    # hftt_loss, by hand, into buffers of its own
    d = capi.LossDesc()
    d.n, d.V = n, V
    mine = [torch.empty_like(g) for g in grads]
    for i, k in enumerate((0, 1, 2, 5, 6, 7)):
        d.prob[i], d.d_prob[i] = outs[k].data_ptr(), mine[i].data_ptr()
    d.vel[0], d.vel[1], d.d_vel[0], d.d_vel[1] = outs[3].data_ptr(), outs[8].data_ptr(), mine[6].data_ptr(), mine[7].data_ptr()
    d.label_onset, d.label_offset, d.label_mpe, d.label_velocity = (t.data_ptr() for t in labels)
    d.weight_A, d.weight_B, d.grad_scale = 0.75, 1.25, 1.0
    out = torch.zeros(16, device=dev)
    ws = torch.empty(L.hftt_loss_ws_bytes(n) // 4 + 16, device=dev)
    d.loss_out, d.ws = out.data_ptr(), ws.data_ptr()
    capi.check(L.hftt_loss(C.byref(d), _st(dev)), 'loss')
    torch.cuda.synchronize(dev)
    assert torch.equal(out[:9], loss9) and all(torch.equal(a, b) for a, b in zip(mine, grads))
    crits = [nn.BCELoss(), nn.BCELoss(), BalancedBCELoss(), nn.CrossEntropyLoss()] * 2
    neutral = LossSpec.from_criteria(crits, eng.N, eng.V, dev)
    assert isinstance(neutral, LossSpec) and not neutral.needs_prepass
    lossn = eng.loss(B, labels, 0.75, 1.25, with_grad=True, spec=neutral)
    torch.cuda.synchronize(dev)
    assert torch.equal(lossn, loss9) and all(torch.equal(bufs[k], g) for k, g in zip(names, grads))


def test_training_train_takes_the_fused_path_for_a_spec(dev, monkeypatch):
    """training.train.train with BalancedBCELoss + weighted CrossEntropyLoss criteria and FusedAdam: a TrainStep carrying a LossSpec runs every
    batch, the model's autograd forward is never called, and the epoch loss is the mean of the per-step loss9[0]; valid() reads the same spec"""
    import bench
    from hftt_hip.criteria import LossSpec
    from hftt_hip.trainer import FusedAdam, TrainStep
    from training import train as T
    cfg = bench.CONFIGS['tiny']
    batches = [(lambda s, l: (s,) + tuple(l))(*bench.synthetic_batch(cfg, B, 20 + i, dev)) for i in range(2)]
    model = bench.build_model(cfg, 13, 0.0, dev)
    crits = _criteria(cfg, dev)
    opt = FusedAdam(model, lr=1e-3)
    seen = []
    call = TrainStep.__call__

    def recording(self, *a):
        loss9 = call(self, *a)
        seen.append((self.loss_spec, loss9.clone()))
        return loss9
    monkeypatch.setattr(TrainStep, '__call__', recording)

    def no_autograd(self, *a, **k):
        raise AssertionError('the compatibility path ran: the model was called')
    monkeypatch.setattr(type(model), 'forward', no_autograd)
    before = model.hftt_engine().flat_params.clone() if hasattr(model.hftt_engine(), 'flat_params') else None
    epoch = T.train(model, batches, opt, *crits, 1.0, 1.0, dev, False)
    assert len(seen) == 2 and all(isinstance(s, LossSpec) for s, _ in seen) and isinstance(opt._train_step.loss_spec, LossSpec)
    per_step = [float(l[0].double()) for _, l in seen]
    assert all(torch.isfinite(l).all() for _, l in seen) and epoch == sum(per_step) / 2
    assert epoch > 0.0
    if before is not None:
        assert not torch.equal(model.hftt_engine().flat_params, before)          # the fused Adam stepped
    monkeypatch.undo()
    # valid(): the fused loss with the same criteria, no gradients; and the reference's criteria still launch hftt_loss (spec None)
    total, nb = T.valid(model, batches, *crits, 1.0, 1.0, dev, False)
    assert nb == 2 and total > 0.0 and total == total
    ref = [nn.BCELoss(), nn.BCELoss(), nn.BCELoss(), nn.CrossEntropyLoss()] * 2
    T.train(model, batches, opt, *ref, 1.0, 1.0, dev, False)
    assert opt._train_step.loss_spec is None
