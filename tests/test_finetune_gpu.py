"""Fine-tuning on the device: the pruned backward (HfttEngine.backward(frozen_stages=...)), FusedAdam's parameter groups and frozen stages,
TrainStep with both.  Tiny configuration, B = 2, dropout 0 unless stated; prune level 1 also runs once at paper dimensions with B = 1 in the
x3 mode, the only shape that builds the merged cross-K/V backward."""
import math

import pytest
import torch

import guard_emul as G

pytestmark = pytest.mark.gpu

B = 2
MODES = ('x3', 'parity', 'bf16')


@pytest.fixture(scope='module')
def batch(dev):
    import bench
    cfg = bench.CONFIGS['tiny']
    spec, labels = bench.synthetic_batch(cfg, B, 5, dev)
    return cfg, spec, labels


def _model(cfg, dev, seed=11, dropout=0.0, mode=None):
    import bench
    model = bench.build_model(cfg, seed, dropout, dev)
    if mode is not None:
        model.hftt_precision = mode
    model.train()
    return model


def _ts(batch, dev, groups=None, seed=11, lr=1e-3, mode=None, **opt_kw):
    """groups: None (the plain one-group form) or a function model -> parameter groups"""
    from hftt_hip.trainer import FusedAdam, TrainStep
    model = _model(batch[0], dev, seed, mode=mode)
    opt = FusedAdam(model.parameters() if groups is None else groups(model), lr=lr, **opt_kw)
    return TrainStep(model, optimizer=opt)


def _state(ts):
    return ts.engine.flat_params.clone(), ts.opt.exp_avg.clone(), ts.opt.exp_avg_sq.clone()


def _eq(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _borders(eng):
    return eng.frozen_border(1), eng.frozen_border(2), eng.flat_grads.numel()


# ------------------------------------------------------------------------------------------------ the pruned backward
def _forward_loss(eng, spec, labels, counter):
    eng.step_counter = counter                       # the same dropout stream position for every repetition
    eng.forward(spec, training=True, save=True)
    return eng.loss(spec.shape[0], labels, 1.0, 1.0, with_grad=True).clone()


def _pruned_against_full(model, spec, labels, levels):
    eng = model.hftt_engine()
    nb = spec.shape[0]
    loss = _forward_loss(eng, spec, labels, 3)
    eng.backward(nb)
    full = eng.flat_grads.clone()
    assert bool(torch.isfinite(full).all()) and bool(torch.isfinite(loss).all())
    for k in levels:
        border = eng.frozen_border(k)
        assert 0 < border < full.numel()
        assert float(full[:border].abs().max()) > 0.0 and float(full[border:].abs().max()) > 0.0
        assert _eq(_forward_loss(eng, spec, labels, 3), loss)
        eng.flat_grads[:border] = 12345.0            # must survive
        eng.flat_grads[border:] = -777.0             # must be rewritten
        ready = []
        eng.backward(nb, frozen_stages=k, on_ready=lambda lo, hi: ready.append((lo, hi)))
        for name, _, o, n in eng._bound:                 # (the alignment gaps behind the parameters are nobody's to write)
            if o >= border:
                assert _eq(eng.flat_grads[o:o + n], full[o:o + n]), (k, name, int((eng.flat_grads[o:o + n] != full[o:o + n]).sum()))
        assert bool((eng.flat_grads[:border] == 12345.0).all()), k
        assert ready == [(lo, hi) for _, lo, hi in eng._ws[nb]['bwd_marks']][:3 - k] and min(lo for lo, _ in ready) == border
    return eng


# (dropout once, in the default mode: the masks come from the seed in every mode alike)
@pytest.mark.parametrize('mode,dropout', [(m, 0.0) for m in MODES] + [('x3', 0.1)])
def test_pruned_backward_values(dev, batch, mode, dropout):
    cfg, spec, labels = batch
    _pruned_against_full(_model(cfg, dev, dropout=dropout, mode=mode), spec, labels, (1, 2))


def _plan_key(plan):
    return [(e[2], None if e[3] is None else (e[3]['kernel'], e[3]['shape'])) for e in plan]


def _check_plan_shape(eng, nb):
    ws = eng._ws[nb]
    full, marks = eng.backward_plan(nb, 0)
    assert full is ws['bwd'] and marks is ws['bwd_marks'] and len(marks) == 3 and marks[-1][0] == len(full)
    p2, m2 = eng.backward_plan(nb, 2)
    assert len(p2) == marks[0][0] and all(a is b for a, b in zip(p2, full)) and m2 == marks[:1]
    p1, m1 = eng.backward_plan(nb, 1)
    assert eng.backward_plan(nb, 1)[0] is p1         # built once
    assert [m[1:] for m in m1] == [m[1:] for m in marks[:2]]
    eGA = ws['bufs']['g.eA'].data_ptr()
    prefix = full[:marks[1][0]]
    onto = [i for i, e in enumerate(prefix) if e[2] in ('strip_linear', 'gemm_nt') and e[1][0]._obj.C == eGA]
    merged = bool(ws['strip'] and eng.merge_ckv_bwd)
    assert len(onto) == (2 if merged else eng.Ld)
    want = [e for i, e in enumerate(prefix) if i not in onto]
    assert _plan_key(p1) == _plan_key(want)
    assert len(p1) == marks[1][0] - len(onto) and m1[1][0] == len(p1) and m1[0][0] == marks[0][0]
    for e in p1:                                     # nothing in the pruned plan writes the encoder-output gradient
        if e[2] in ('strip_linear', 'gemm_nt'):
            assert e[1][0]._obj.C != eGA
    return merged


@pytest.mark.parametrize('mode', MODES)
def test_pruned_backward_shape(dev, batch, mode):
    cfg, spec, labels = batch
    model = _model(cfg, dev, mode=mode)
    eng = model.hftt_engine()
    _forward_loss(eng, spec, labels, 1)
    n_bufs = len(eng._ws[B]['bufs'])
    assert 'bwd_dec' not in eng._ws[B]               # lazily: the default path's workspace does not grow
    assert not _check_plan_shape(eng, B)
    assert len(eng._ws[B]['bufs']) == n_bufs
    from hftt_hip import HfttError
    with pytest.raises(HfttError):
        eng.backward(B, frozen_stages=3)


def test_pruned_backward_at_paper_dimensions_merged_form(dev):
    import bench
    cfg = bench.CONFIGS['paper']
    spec, labels = bench.synthetic_batch(cfg, 1, 5, dev)
    eng = _pruned_against_full(_model(cfg, dev, dropout=0.1, mode='x3'), spec, labels, (1,))
    assert _check_plan_shape(eng, 1)                 # the merged cross-K/V form: two launches onto the encoder-output gradient


# ------------------------------------------------------------------------------------------------ training steps
def _enc_frozen(model):
    from hftt_hip.trainer import stage_groups
    return stage_groups(model, encoder=dict(frozen=True))


@pytest.mark.parametrize('mode', MODES)
def test_three_steps_with_a_frozen_encoder(dev, batch, mode):
    _, spec, labels = batch
    fz, plain = _ts(batch, dev, _enc_frozen, mode=mode), _ts(batch, dev, mode=mode)
    assert fz.engine.precision == mode and fz.opt.frozen_stages() == 1
    b0, b1, n = _borders(fz.engine)
    start = _state(fz)
    assert all(_eq(a, b) for a, b in zip(start, _state(plain)))
    fz.engine.flat_grads[:b0] = 3.0                  # stale values below the border: zeroed once when the level changes
    prev = start
    for k in range(3):
        loss = fz(spec, *labels)
        assert loss.shape == (9,) and bool(torch.isfinite(loss).all())
        now = _state(fz)
        for name, a, b in zip(('parameters', 'exp_avg', 'exp_avg_sq'), start, now):
            assert _eq(a[:b0], b[:b0]), (k, name)
            assert bool(torch.isfinite(b).all())
            assert not _eq(prev[('parameters', 'exp_avg', 'exp_avg_sq').index(name)][b0:], b[b0:]), (k, name)
        assert bool((fz.engine.flat_grads[:b0] == 0.0).all())
        if k == 0:
            lp = plain(spec, *labels)
            assert _eq(loss, lp)
            for name, a, b in zip(('parameters', 'exp_avg', 'exp_avg_sq'), now, _state(plain)):
                assert _eq(a[b0:], b[b0:]), name
            assert not _eq(now[0][:b0], _state(plain)[0][:b0])
        prev = now
    assert 'bwd_dec' in fz.engine._ws[B] and 'bwd_dec' not in plain.engine._ws[B]
    fz.expose_grads()
    assert all(float(p.grad.abs().max()) == 0.0 for name, p, o, _ in fz.engine._bound if o < b0)


def _flags_only(model):
    names = [n for n, _ in model.named_parameters()]
    cut = names.index('decoder_spec2midi.pos_embedding_freq.weight')
    for _, p in list(model.named_parameters())[:cut]:
        p.requires_grad_(False)
    return model.parameters()


def _enc_freq_frozen(model):
    from hftt_hip.trainer import stage_groups
    return stage_groups(model, encoder=dict(frozen=True), freq=dict(frozen=True))


@pytest.mark.parametrize('case', ('encoder+freq', 'requires_grad'))
def test_three_steps_per_prune_level(dev, batch, case):
    _, spec, labels = batch
    fz, plain = _ts(batch, dev, _enc_freq_frozen if case == 'encoder+freq' else _flags_only), _ts(batch, dev)
    level = 2 if case == 'encoder+freq' else 1
    assert fz.opt.frozen_stages() == level and len(fz.opt.param_groups) == (3 if level == 2 else 1)
    border = _borders(fz.engine)[level - 1]
    assert fz.opt._group_map()['borders'][level] == border
    start = _state(fz)
    fz.engine.flat_grads[:border] = 3.0
    for k in range(3):
        loss = fz(spec, *labels)
        assert bool(torch.isfinite(loss).all())
        now = _state(fz)
        for a, b in zip(start, now):
            assert _eq(a[:border], b[:border]) and not _eq(a[border:], b[border:]) and bool(torch.isfinite(b).all())
        assert bool((fz.engine.flat_grads[:border] == 0.0).all())
        if k == 0:
            plain(spec, *labels)
            for a, b in zip(now, _state(plain)):
                assert _eq(a[border:], b[border:])
    assert fz.opt.step_count == 3 and ('bwd_dec' in fz.engine._ws[B]) == (level == 1)
    if case == 'requires_grad':                      # the flags come back: the next step is a full one again
        for p in fz.model.parameters():
            p.requires_grad_(True)
        assert fz.opt.frozen_stages() == 0
        fz(spec, *labels)
        assert not _eq(start[0][:border], fz.engine.flat_params[:border]) and float(fz.engine.flat_grads[:border].abs().max()) > 0.0


def test_per_group_learning_rates(dev, batch):
    from hftt_hip import ops
    from hftt_hip.trainer import stage_groups
    _, spec, labels = batch
    rates = (1e-5, 1e-4, 1e-3)
    ts = _ts(batch, dev, lambda m: stage_groups(m, encoder=dict(lr=rates[0]), freq=dict(lr=rates[1]), time=dict(lr=rates[2])), lr=7e-2)
    assert ts.opt.frozen_stages() == 0
    b0, b1, n = _borders(ts.engine)
    ts(spec, *labels)
    got = _state(ts)
    for (lo, hi), lr in zip(((0, b0), (b0, b1), (b1, n)), rates):
        one = _ts(batch, dev, lr=lr)
        one(spec, *labels)
        for name, a, b in zip('pmv', got, _state(one)):
            assert _eq(a[lo:hi], b[lo:hi]), (lr, name)
    # a scheduler writes param_groups[i]['lr']: the next step takes it, the map stays
    the_map = ts.opt._map
    ts.opt.param_groups[1]['lr'] = 5e-4
    ts.forward_backward(spec, *labels)
    before, g = _state(ts), ts.engine.flat_grads.clone()
    ts.opt.step()
    assert ts.opt._map is the_map and ts.opt.step_count == 2
    for (lo, hi), lr in zip(((0, b0), (b0, b1), (b1, n)), (rates[0], 5e-4, rates[2])):
        p, m, v = (t[lo:hi].clone() for t in before)
        ops.adam_step(p, g[lo:hi].clone(), m, v, 2, lr=lr)
        for name, a, b in zip('pmv', _state(ts), (p, m, v)):
            assert _eq(a[lo:hi], b), (lr, name)


@pytest.mark.parametrize('guard', (False, True))
def test_one_group_in_list_form_is_todays_step(dev, batch, guard):
    _, spec, labels = batch
    plain = _ts(batch, dev, guard=guard)
    listed = _ts(batch, dev, lambda m: [{'params': list(m.parameters())}], guard=guard)
    assert listed.opt._group_map()['trivial'] and listed.opt.frozen_stages() == 0
    for _ in range(3):
        assert _eq(plain(spec, *labels), listed(spec, *labels))
    for name, a, b in zip(('parameters', 'exp_avg', 'exp_avg_sq'), _state(plain), _state(listed)):
        assert _eq(a, b), name
    assert 'bwd_dec' not in listed.engine._ws[B]


def test_no_decay_1d(dev, batch):
    from hftt_hip.trainer import stage_groups
    _, spec, labels = batch
    twin = _ts(batch, dev, lambda m: stage_groups(m, no_decay_1d=True), weight_decay=0.01)
    decayed, plain = _ts(batch, dev, weight_decay=0.01), _ts(batch, dev)
    assert len(twin.opt.param_groups) == 6
    for ts in (twin, decayed, plain):
        ts(spec, *labels)
    n1 = 0
    for (name, p, o, n), (_, pd, _, _), (_, pz, _, _) in zip(twin.engine._bound, decayed.engine._bound, plain.engine._bound):
        if p.dim() <= 1:
            n1 += 1
            assert _eq(p.data, pz.data), name
        else:
            assert _eq(p.data, pd.data) and not _eq(p.data, pz.data), name
    assert n1 > 0
    assert _eq(twin.opt.exp_avg, decayed.opt.exp_avg) and _eq(twin.opt.exp_avg_sq, plain.opt.exp_avg_sq)


def test_state_dict_round_trip(dev, batch):
    from hftt_hip.trainer import FusedAdam, TrainStep, stage_groups
    cfg, spec, labels = batch
    groups = lambda m: stage_groups(m, encoder=dict(frozen=True), freq=dict(lr=1e-4), time=dict(lr=1e-3))          # noqa: E731
    a = _ts(batch, dev, groups, lr=5e-5)
    a(spec, *labels); a(spec, *labels)
    sd = a.opt.state_dict()
    assert [g['frozen'] for g in sd['param_groups']] == [True, False, False]
    model_b = _model(cfg, dev, seed=99)
    model_b.load_state_dict(a.model.state_dict())
    opt_b = FusedAdam(groups(model_b), lr=5e-5)
    b = TrainStep(model_b, optimizer=opt_b)
    opt_b.load_state_dict(sd)
    assert opt_b.step_count == 2 and opt_b.frozen_stages() == 1
    assert all(_eq(x, y) for x, y in zip(_state(a), _state(b)))
    assert _eq(a(spec, *labels), b(spec, *labels))
    for name, x, y in zip(('parameters', 'exp_avg', 'exp_avg_sq'), _state(a), _state(b)):
        assert _eq(x, y), name
    with pytest.raises(ValueError):
        FusedAdam(_model(cfg, dev, seed=99).parameters(), lr=5e-5).load_state_dict(sd)


def test_guard_with_a_frozen_range(dev, batch):
    _, spec, labels = batch
    ts = _ts(batch, dev, guard=True)
    name, p, o, n = ts.engine._bound[4]
    assert name.startswith('encoder_spec2midi.')
    p.requires_grad_(False)                          # an optimizer-level freeze of one encoder tensor: nothing to prune
    assert ts.opt.frozen_stages() == 0 and not ts.opt._group_map()['trivial']
    ts.forward_backward(spec, *labels)
    assert float(ts.engine.flat_grads[:o].abs().max()) > 0.0          # the backward was not pruned
    ts.engine.flat_grads[o + n // 2] = float('inf')
    before = _state(ts)
    ts.opt.step()
    after = _state(ts)
    assert ts.opt.skipped_steps == 0 and float(ts.opt.clip_coef) == 1.0 and math.isfinite(float(ts.opt.grad_norm))
    for x, y in zip(before, after):
        assert _eq(x[o:o + n], y[o:o + n]) and not _eq(x, y) and bool(torch.isfinite(y).all())
    ts.forward_backward(spec, *labels)
    ts.engine.flat_grads[ts.engine._bound[5][2]] = float('inf')      # the next tensor is trainable
    before = _state(ts)
    ts.opt.step()
    assert not G.skip_check(before, _state(ts))
    assert ts.opt.skipped_steps == 1 and ts.opt.step_count == 2


def test_the_lazily_built_plan_does_not_keep_the_engine_alive(dev, batch):
    """the workspace must not refer back to its engine (through a kept builder, say): an engine nobody uses any more gives its device memory
    back at once, not when the garbage collector next looks at cycles"""
    import gc
    import weakref
    cfg, spec, labels = batch
    model = _model(cfg, dev)
    eng = model.hftt_engine()
    _forward_loss(eng, spec, labels, 1)
    eng.backward(B, frozen_stages=1)
    torch.cuda.synchronize()
    ref = weakref.ref(eng)
    gc.collect()
    gc.disable()
    try:
        del eng, model
        assert ref() is None
    finally:
        gc.enable()
