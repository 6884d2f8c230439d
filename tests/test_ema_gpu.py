"""The averaged weights on the device (csrc/guard.hip: hftt_adam_step_ema; hftt_hip.ops.adam_step_ema; FusedAdam's ema_decay / ema_warmup,
averaged_weights() and averaged_model()) against the criteria of tests/ema_emul.py.

Kernel level, n in ema_emul.EMA_N = 4, 8 (one quad, two), 1020, 1028 (a workgroup less a quad, a workgroup and a quad) and 2048 * 256 * 4 + 8
(two quads behind the first grid pass), in the three configurations the optimizer launches: 'plain' (one group, no map, no record: against
hftt_adam_step), 'guarded' (one group, no map, the record of a norm clipped at 1e-3, decay 0.01: against hftt_adam_step_guarded) and 'groups'
(three groups by quad index mod 3, the second frozen, per-group rate and decay, guarded: against hftt_adam_step_groups).
Engine level: the tiny config and batch of tests/test_guard_gpu.py.
"""
import math
import pickle

import pytest
import torch

import elementwise_emul as E
import ema_emul as M
import guard_emul as G

pytestmark = pytest.mark.gpu

S0 = 5                                              # first step number (bias corrections well away from 1)
STEPS = 3
CONFIGS = ('plain', 'guarded', 'groups')
GROUP_LR, GROUP_WD, GROUP_FROZEN = (1e-3, 5e-4, 2e-3), (0.01, 0.0, 0.02), (False, True, False)


class _Run:
    """one configuration's buffers on the device and its two steps: the entry point of before (`step`) and hftt_adam_step_ema (`step_ema`)"""

    def __init__(self, kind, n, dev, seed=0):
        from hftt_hip import ops
        self.kind, self.n, self.dev = kind, n, dev
        p, m, v, e0 = M.ema_start(n, seed)
        self.p, self.m, self.v = p.to(dev), m.to(dev), v.to(dev)
        self.e0 = e0
        self.e, self.c = e0.to(dev), torch.zeros(n, device=dev)
        self.ctl, self.ws = ops.guard_buffers(n, dev)
        self.qmap = (torch.arange(n // 4) % 3).to(torch.uint8).to(dev) if kind == 'groups' else None
        self.frozen = M.frozen_elements(self.qmap, GROUP_FROZEN) if kind == 'groups' else torch.zeros(n, dtype=torch.bool)

    def _norm(self, g):
        from hftt_hip import ops
        if self.kind == 'guarded':
            ops.grad_norm(g, self.ctl, self.ws, max_norm=1e-3)
        elif self.kind == 'groups':
            ops.grad_norm_groups(g, self.qmap, 2, self.ctl, self.ws, max_norm=1e-3)

    def step(self, g, k):
        from hftt_hip import ops
        self._norm(g)
        if self.kind == 'plain':
            ops.adam_step(self.p, g, self.m, self.v, S0 + k, lr=E.ADAM_LR)
        elif self.kind == 'guarded':
            ops.adam_step_guarded(self.p, g, self.m, self.v, S0 + k, self.ctl, lr=E.ADAM_LR, weight_decay=0.01)
        else:
            ops.adam_step_groups(self.p, g, self.m, self.v, S0 + k, self.qmap, lr=GROUP_LR, weight_decay=GROUP_WD, frozen=GROUP_FROZEN, ctl=self.ctl)

    def step_ema(self, g, k, beta):
        from hftt_hip import ops
        self._norm(g)
        if self.kind == 'plain':
            ops.adam_step_ema(self.p, g, self.m, self.v, self.e, self.c, S0 + k, beta, lr=[E.ADAM_LR])
        elif self.kind == 'guarded':
            ops.adam_step_ema(self.p, g, self.m, self.v, self.e, self.c, S0 + k, beta, lr=[E.ADAM_LR], weight_decay=[0.01], ctl=self.ctl)
        else:
            ops.adam_step_ema(self.p, g, self.m, self.v, self.e, self.c, S0 + k, beta, lr=GROUP_LR, quad_group=self.qmap, weight_decay=GROUP_WD,
                              frozen=GROUP_FROZEN, ctl=self.ctl)


def _grad(n, k, dev):
    return E.adam_grad(n, 9, k).to(dev)


@pytest.mark.parametrize('kind', CONFIGS)
@pytest.mark.parametrize('n', M.EMA_N)
def test_the_average_against_fp64_and_the_restatement(dev, n, kind):
    """three chained calls per decay: after each, e and e - c within ema_ref's bounds over the parameters the kernel itself produced, and
    (printed, and asserted) the bits of the fp32 restatement"""
    for beta in M.EMA_DECAYS:
        r = _Run(kind, n, dev)
        keep = ~r.frozen
        ps, ee, cc = [], r.e0.clone(), torch.zeros(n)
        for k in range(STEPS):
            r.step_ema(_grad(n, k, dev), k, beta)
            ps.append(r.p.cpu())
            ref = M.ema_ref(r.e0, ps, [beta] * len(ps))
            bad = M.ema_check(r.e, r.c, ref, keep=keep)
            ee, cc = M.ema_emul(ee, cc, ps[-1], beta, frozen=r.frozen)
            off = int((ee != r.e.cpu()).sum()), int((cc != r.c.cpu()).sum())
            err = ((r.e.cpu().double() - ref['e']).abs() / (ref['b_e'] + 1e-300))[keep]
            print('n=%d %s beta=%g call %d: worst |e - fp64| / bound %.3f; elements off the restatement: e %d, c %d' % (n, kind, beta, k, float(err.max()), *off))
            assert not bad, (n, kind, beta, k, bad)
            assert off == (0, 0), (n, kind, beta, k, off)
        if kind != 'plain' and n >= 1020:
            assert int(r.ctl.cpu()[4]) == STEPS                         # the clip at 1e-3 did act in the guarded configurations


@pytest.mark.parametrize('kind', CONFIGS)
@pytest.mark.parametrize('n', M.EMA_N)
def test_parameters_and_moments_keep_the_bits_of_the_step_without_the_average(dev, n, kind):
    a, b = _Run(kind, n, dev), _Run(kind, n, dev)
    for k in range(STEPS):
        g = _grad(n, k, dev)
        a.step(g, k)
        b.step_ema(g, k, 0.9999)
        for name, x, y in zip('pmv', (a.p, a.m, a.v), (b.p, b.m, b.v)):
            assert torch.equal(x, y), (n, kind, k, name, int((x != y).sum()))
    assert torch.equal(a.ctl, b.ctl)
    assert not torch.equal(b.e.cpu(), b.e0)                              # (the average did move)


@pytest.mark.parametrize('kind', ('guarded', 'groups'))
@pytest.mark.parametrize('n', M.EMA_N)
def test_a_planted_inf_skips_the_step_and_the_average_keeps_its_bits(dev, n, kind):
    r = _Run(kind, n, dev)
    r.step_ema(_grad(n, 0, dev), 0, 0.9)                                 # one applied call: c is no longer all zeros
    g = _grad(n, 1, dev)
    g[int((~r.frozen).nonzero()[-1])] = math.inf                         # the last element that has a gradient (an Inf in a frozen quad does not skip)
    before = [t.clone() for t in (r.p, r.m, r.v, r.e, r.c)]
    r.step_ema(g, 1, 0.9)
    w = r.ctl.cpu()
    assert int(w[2]) == 0 and int(w[3]) == 1                             # apply == 0, skipped == 1
    bad = G.skip_check(before[:3], (r.p, r.m, r.v)) + M.bits_check('ema', before[3], r.e) + M.bits_check('ema_c', before[4], r.c)
    assert not bad, (n, kind, bad)
    r.step_ema(_grad(n, 2, dev), 2, 0.9)                                 # a clean call moves it again
    assert not torch.equal(before[3], r.e)


@pytest.mark.parametrize('n', M.EMA_N)
def test_frozen_quads_keep_the_sentinel(dev, n):
    r = _Run('groups', n, dev)
    fz = r.frozen.to(dev)
    sent = torch.full((n,), M.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    r.e, r.c = torch.where(fz, sent, r.e), torch.where(fz, sent, r.c)
    before = [t.clone() for t in (r.p, r.m, r.v, r.e, r.c)]
    ps = []
    for k in range(STEPS):
        r.step_ema(_grad(n, k, dev), k, 0.9)
        ps.append(r.p.cpu())
    bad = []
    for name, x, y in zip(('p', 'm', 'v', 'ema', 'ema_c'), before, (r.p, r.m, r.v, r.e, r.c)):
        bad += M.bits_check('frozen ' + name, x, y, r.frozen)
    assert not bad, (n, bad)
    assert not M.ema_check(r.e, r.c, M.ema_ref(r.e0, ps, [0.9] * STEPS), keep=~r.frozen)
    if n >= 8:
        assert int(r.frozen.sum()) >= 4


def test_stagnation_2000_calls_follow_the_fp64_average(dev):
    """the test the plain fp32 form cannot pass: g = 0 and zero moments leave p fixed 2e-4 |e| away, beta = 0.9999; the fp64 average moves
    by about 300 ulp, e += omd (p - e) in fp32 by none"""
    from hftt_hip import ops
    n = M.STAG_N
    p0, e0 = M.stagnation_start(n)
    p, e = p0.to(dev), e0.to(dev)
    g, m, v, c = (torch.zeros(n, device=dev) for _ in range(4))
    for k in range(M.STAG_K):
        ops.adam_step_ema(p, g, m, v, e, c, 1 + k, M.STAG_BETA, lr=[E.ADAM_LR])
    assert torch.equal(p.cpu(), p0) and not bool(m.any()) and not bool(v.any())          # Adam left p where it was
    ref = M.ema_ref(e0, [p0] * M.STAG_K, [M.STAG_BETA] * M.STAG_K)
    ulp = 2.0 ** (torch.floor(torch.log2(e0.abs().double())) - 23)
    moved = (e.cpu().double() - e0.double()).abs() / ulp
    err = (e.cpu().double() - ref['e']).abs() / ulp
    print('the average moved by %.0f .. %.0f ulp; worst distance from fp64 %.3f ulp (bound %.3f ulp)'
          % (float(moved.min()), float(moved.max()), float(err.max()), float((ref['b_e'] / ulp).max())))
    assert float(moved.min()) > 150
    bad = M.ema_check(e, c, ref)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ optimizer level
B = 2


@pytest.fixture(scope='module')
def batch(dev):
    import bench
    cfg = bench.CONFIGS['tiny']
    spec, labels = bench.synthetic_batch(cfg, B, 5, dev)
    return cfg, spec, labels


def _train_step(batch, dev, seed=11, groups=None, **opt_kw):
    import bench
    from hftt_hip.trainer import FusedAdam, TrainStep, stage_groups
    cfg, spec, labels = batch
    model = bench.build_model(cfg, seed, 0.0, dev)             # default precision mode, dropout 0
    model.train()
    params = model.parameters() if groups is None else stage_groups(model, **groups)
    opt = FusedAdam(params, lr=1e-3, model=model, **opt_kw)
    return TrainStep(model, optimizer=opt)


def _state(ts):
    return ts.engine.flat_params.clone(), ts.opt.exp_avg.clone(), ts.opt.exp_avg_sq.clone()


OPT_CASES = {'plain': {}, 'guarded': dict(max_grad_norm=1e-2, weight_decay=0.01),
             'grouped': dict(groups=dict(encoder=dict(frozen=True), time=dict(lr=2e-3)), guard=True)}


@pytest.mark.parametrize('case', sorted(OPT_CASES))
def test_three_training_steps_with_and_without_the_average(dev, batch, case):
    """parameters and moments bit-identical; the average IS the restatement run over the recorded parameters (warm-up schedule included)"""
    _, spec, labels = batch
    kw = OPT_CASES[case]
    plain, avg = _train_step(batch, dev, **kw), _train_step(batch, dev, ema_decay=0.99, ema_warmup=True, **kw)
    assert plain.opt.ema is None and 'ema' not in plain.opt.state[plain.opt._params()[0]]
    e0 = avg.opt.ema.cpu()
    assert torch.equal(e0, avg.engine.flat_params.cpu()) and not bool(avg.opt.ema_c.any())          # starts as a copy of the parameters
    mp = avg.opt._group_map()
    frozen = torch.zeros(e0.numel(), dtype=torch.bool) if mp['trivial'] else M.frozen_elements(mp['host'], mp['frozen'])
    ee, cc, ps, betas = e0.clone(), torch.zeros_like(e0), [], []
    for t in range(3):
        la, lb = plain(spec, *labels), avg(spec, *labels)
        assert torch.equal(la, lb)
        ps.append(avg.engine.flat_params.cpu())
        betas.append(M.warmup_decay(0.99, t))
        ee, cc = M.ema_emul(ee, cc, ps[-1], betas[-1], frozen=frozen)
    for name, a, b in zip(('parameters', 'exp_avg', 'exp_avg_sq'), _state(plain), _state(avg)):
        assert torch.equal(a, b), name
    assert avg.opt.ema_updates == 3 and betas[0] == 0.1
    assert not M.ema_check(avg.opt.ema, avg.opt.ema_c, M.ema_ref(e0, ps, betas), keep=~frozen)
    assert torch.equal(avg.opt.ema.cpu(), ee) and torch.equal(avg.opt.ema_c.cpu(), cc)
    if case == 'grouped':
        assert int(frozen.sum()) > 0 and torch.equal(avg.opt.ema.cpu()[frozen], e0[frozen])
    # the per-parameter state entries are views into the flat buffers
    name, p, o, n = avg.engine._bound[1]
    st = avg.opt.state[p]
    assert st['ema'].data_ptr() == avg.opt.ema.data_ptr() + 4 * o and st['ema_c'].data_ptr() == avg.opt.ema_c.data_ptr() + 4 * o
    assert st['ema'].shape == p.shape


def _forward(model, spec):
    model.eval()
    with torch.no_grad():
        out = model(spec)
    model.train()
    return [o.clone() for o in out]


def test_averaged_weights_context_and_averaged_model(dev, batch):
    from hftt_hip import HfttError
    _, spec, labels = batch
    ts = _train_step(batch, dev, ema_decay=0.9)
    for _ in range(3):
        ts(spec, *labels)
    raw = _forward(ts.model, spec)
    params, ema = ts.engine.flat_params.clone(), ts.opt.ema.clone()
    assert not torch.equal(params, ema)
    twin = pickle.loads(pickle.dumps(ts.opt.averaged_model(), protocol=4))          # picklable the way tools/train_config5.py --out pickles
    assert all(p.device.type == 'cpu' for p in twin.parameters())
    for (name, p, o, n), q in zip(ts.engine._bound, twin.parameters()):
        assert torch.equal(q.detach().reshape(-1), ema[o:o + n].cpu()), name
    assert torch.equal(ts.engine.flat_params, params) and torch.equal(ts.opt.ema, ema)          # the model on the device was not touched
    want = _forward(twin.to(dev), spec)
    with ts.opt.averaged_weights():
        assert torch.equal(ts.engine.flat_params, ema) and torch.equal(ts.opt.ema, params)
        inside = _forward(ts.model, spec)
        with pytest.raises(HfttError, match='inside averaged_weights'):
            ts.opt.step()
        with pytest.raises(HfttError, match='does not nest'):
            with ts.opt.averaged_weights():
                pass
        with pytest.raises(HfttError, match='inside averaged_weights'):
            ts(spec, *labels)
        with pytest.raises(HfttError, match='inside averaged_weights'):
            ts.opt.state_dict()                                                      # (it would save the two swapped)
    assert len(inside) == len(want) == len(raw)
    for a, b in zip(inside, want):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(inside, raw))                  # (the average is not the raw iterate)
    assert torch.equal(ts.engine.flat_params.view(torch.int32), params.view(torch.int32))
    assert torch.equal(ts.opt.ema.view(torch.int32), ema.view(torch.int32))
    for a, b in zip(_forward(ts.model, spec), raw):
        assert torch.equal(a, b)
    ts(spec, *labels)                                                                # and training goes on
    assert ts.opt.ema_updates == 4


def test_state_dict_round_trip_keeps_the_average_and_the_next_step(dev, batch):
    import bench
    from hftt_hip.trainer import FusedAdam, TrainStep
    cfg, spec, labels = batch
    a = _train_step(batch, dev, ema_decay=0.99, ema_warmup=True)
    for _ in range(3):
        a(spec, *labels)
    sd = a.opt.state_dict()
    assert sd['hftt_ema'] == {'decay': 0.99, 'warmup': True, 'updates': 3}
    assert all('ema' in s and 'ema_c' in s for s in sd['state'].values())
    model_b = bench.build_model(cfg, 99, 0.0, dev)
    model_b.load_state_dict(a.model.state_dict())
    model_b.train()
    opt_b = FusedAdam(model_b.parameters(), lr=5e-4)             # built WITHOUT the option: the state brings it
    b = TrainStep(model_b, optimizer=opt_b)
    assert opt_b.ema is None
    opt_b.load_state_dict(sd)
    assert opt_b.param_groups[0]['ema_decay'] == 0.99 and opt_b.param_groups[0]['ema_warmup'] is True and opt_b.ema_updates == 3
    assert torch.equal(a.opt.ema, opt_b.ema) and torch.equal(a.opt.ema_c, opt_b.ema_c)
    assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))
    la, lb = a(spec, *labels), b(spec, *labels)
    assert torch.equal(la, lb)
    for name, x, y in zip(('parameters', 'exp_avg', 'exp_avg_sq'), _state(a), _state(b)):
        assert torch.equal(x, y), name
    assert torch.equal(a.opt.ema, opt_b.ema) and torch.equal(a.opt.ema_c, opt_b.ema_c)
    assert opt_b.ema_updates == a.opt.ema_updates == 4
    # a state WITHOUT the average into an optimizer with the option: the average restarts from the parameters
    plain_sd = FusedAdam(a.model.parameters(), lr=1e-3).state_dict()
    a.opt.load_state_dict(plain_sd)
    assert a.opt.param_groups[0]['ema_decay'] == 0.99 and a.opt.ema_updates == 0
    assert torch.equal(a.opt.ema, a.engine.flat_params) and not bool(a.opt.ema_c.any())
