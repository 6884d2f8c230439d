"""The grouped optimizer kernels on the device (csrc/guard.hip: hftt_adam_step_groups, hftt_grad_norm_groups) against the single-group
kernels, bit for bit, and against the fp64 criteria of tests/guard_emul.py.

Sizes: 8 (one workgroup, two quads: one segment), 1024 (one workgroup), 1032 (a partial second one), 2048 * 256 * 4 + 8 (two quads behind the
first grid pass).  Three groups laid out as A | B | A | C with borders on multiples of 8; at n = 8 the only segment is A's.  State: random
non-zero p / m / v, step 5, gradients from guard_grad's log-uniform stream."""
import math

import pytest
import torch

import elementwise_emul as E
import guard_emul as G

pytestmark = pytest.mark.gpu

S0 = 5
SIZES = (8, 1024, 1032, G.GRID_PASS + 8)
A, B, C_ = 0, 1, 2
OPTS = {A: dict(lr=1e-3, weight_decay=0.01), B: dict(lr=3e-4, weight_decay=0.0), C_: dict(lr=2e-5, weight_decay=0.1)}


def _segments(n):
    """[(lo, hi, group)]: A | B | A | C, borders rounded down to multiples of 8 (empty segments dropped)"""
    cuts = [0] + [n * k // 4 // 8 * 8 for k in (1, 2, 3)] + [n]
    if n == 8:
        return [(0, 8, A)]
    return [(lo, hi, g) for lo, hi, g in zip(cuts[:-1], cuts[1:], (A, B, A, C_)) if hi > lo]


def _qmap(n, dev):
    from hftt_hip import ops
    return ops.adam_group_map([(lo, hi - lo, g) for lo, hi, g in _segments(n)], n, dev)


def _record(ctl):
    w = ctl.cpu()
    f = w.view(torch.float32)
    return float(f[0]), float(f[1]), int(w[2]), int(w[3]) & 0xFFFFFFFF, int(w[4]) & 0xFFFFFFFF


def _buffers(n, dev):
    from hftt_hip import ops
    ctl, ws = ops.guard_buffers(n, dev)
    ws.fill_(float('nan'))
    return ctl, ws


def _state(n, dev):
    return [t.to(dev) for t in E.adam_state(n, 17 + n % 1000)]


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('n', SIZES)
def test_one_group_is_bit_identical_to_the_guarded_and_the_plain_step(dev, n):
    from hftt_hip import ops
    g = G.guard_grad(n, 'log_uniform').to(dev)
    qmap = torch.zeros(n // 4, dtype=torch.uint8, device=dev)
    for mx in (math.inf, 1e-3):
        for wd in (0.0, 0.01):
            a, b = _state(n, dev), _state(n, dev)
            ctl, ws = _buffers(n, dev)
            ops.grad_norm(g, ctl, ws, grad_scale=0.25, max_norm=mx)
            coef = _record(ctl)[1]
            assert (coef < 1.0) == (mx != math.inf)
            ops.adam_step_guarded(a[0], g, a[1], a[2], S0, ctl, lr=E.ADAM_LR, grad_scale=0.25, weight_decay=wd)
            ops.adam_step_groups(b[0], g, b[1], b[2], S0, qmap, lr=[E.ADAM_LR], weight_decay=[wd], ctl=ctl, grad_scale=0.25)
            for name, x, y in zip('pmv', a, b):
                assert _same(x, y), (n, mx, wd, name, int((x != y).sum()))
    # ctl = None, no decay: adam_step's bits
    a, b = _state(n, dev), _state(n, dev)
    ops.adam_step(a[0], g, a[1], a[2], S0, lr=E.ADAM_LR, grad_scale=0.5)
    ops.adam_step_groups(b[0], g, b[1], b[2], S0, qmap, lr=[E.ADAM_LR], grad_scale=0.5)
    for name, x, y in zip('pmv', a, b):
        assert _same(x, y), (n, name, int((x != y).sum()))
    assert not _same(a[0], _state(n, dev)[0])


def _grouped_case(dev, n, frozen):
    """the grouped step (B frozen or not) against the guarded step on every slice alone, with the group's options and the same record"""
    from hftt_hip import ops
    g = G.guard_grad(n, 'log_uniform').to(dev)
    qmap = _qmap(n, dev)
    ctl, ws = _buffers(n, dev)
    mask = (1 << B) if frozen else 0
    ops.grad_norm_groups(g, qmap, mask, ctl, ws, grad_scale=0.25, max_norm=1e-3)
    norm, coef, apply, _, _ = _record(ctl)
    assert apply == 1
    start = _state(n, dev)
    got = [t.clone() for t in start]
    ops.adam_step_groups(got[0], g, got[1], got[2], S0, qmap, lr=[OPTS[k]['lr'] for k in (A, B, C_)], weight_decay=[OPTS[k]['weight_decay'] for k in (A, B, C_)],
                         frozen=[False, frozen, False], ctl=ctl, grad_scale=0.25)
    want = [t.clone() for t in start]
    for lo, hi, k in _segments(n):
        if frozen and k == B:
            for name, x, y in zip('pmv', got, start):
                assert _same(x[lo:hi], y[lo:hi]), (n, 'frozen', name)
            continue
        ops.adam_step_guarded(want[0][lo:hi], g[lo:hi], want[1][lo:hi], want[2][lo:hi], S0, ctl, lr=OPTS[k]['lr'], grad_scale=0.25, weight_decay=OPTS[k]['weight_decay'])
        for name, x, y in zip('pmv', got, want):
            assert _same(x[lo:hi], y[lo:hi]), (n, k, name, int((x[lo:hi] != y[lo:hi]).sum()))
        ref = G.guarded_adam_ref(start[0][lo:hi], g[lo:hi], start[1][lo:hi], start[2][lo:hi], S0, coef, lr=OPTS[k]['lr'], grad_scale=0.25,
                                 weight_decay=OPTS[k]['weight_decay'])
        bad = G.guarded_adam_check(got[0][lo:hi], got[1][lo:hi], got[2][lo:hi], ref)
        assert not bad, (n, k, bad)
        assert not _same(got[0][lo:hi], start[0][lo:hi])
    return g, norm, coef


@pytest.mark.parametrize('n', SIZES)
def test_three_groups_equal_the_guarded_step_on_every_slice(dev, n):
    _grouped_case(dev, n, frozen=False)


@pytest.mark.parametrize('n', SIZES)
def test_a_frozen_group_keeps_every_bit(dev, n):
    _grouped_case(dev, n, frozen=True)


@pytest.mark.parametrize('n', SIZES)
def test_norm_with_no_frozen_group_leaves_grad_norms_record(dev, n):
    from hftt_hip import ops
    g = G.guard_grad(n, 'log_uniform').to(dev)
    qmap = _qmap(n, dev)
    a, wa = _buffers(n, dev)
    b, wb = _buffers(n, dev)
    for gs, mx in ((1.0, math.inf), (0.25, 1e-3), (1.0, 1.0)):
        ops.grad_norm(g, a, wa, grad_scale=gs, max_norm=mx)
        ops.grad_norm_groups(g, qmap, 0, b, wb, grad_scale=gs, max_norm=mx)
        assert torch.equal(a, b), (n, gs, mx, _record(a), _record(b))
    assert _record(b)[4] >= 1 or n == 8


@pytest.mark.parametrize('n', SIZES)
def test_norm_leaves_the_frozen_group_out(dev, n):
    from hftt_hip import ops
    g = G.guard_grad(n, 'log_uniform').to(dev)
    qmap = _qmap(n, dev)
    keep = torch.ones(n, dtype=torch.bool)
    for lo, hi, k in _segments(n):
        if k == B:
            keep[lo:hi] = False
    ctl, ws = _buffers(n, dev)
    for gs, mx in ((1.0, math.inf), (0.25, 1e-3)):
        ref = G.gnorm_ref(g.cpu()[keep], gs, mx)
        ops.grad_norm_groups(g, qmap, 1 << B, ctl, ws, grad_scale=gs, max_norm=mx)
        norm, coef, apply, _, _ = _record(ctl)
        print('n=%d gs=%g max_norm=%g: norm %.9g (fp64 %.17g) coef %.9g (fp64 %.17g)' % (n, gs, mx, norm, ref['norm'], coef, ref['coef']))
        assert not G.gnorm_check(norm, coef, apply, ref), (n, gs, mx)
        if n > 8:
            assert abs(norm - G.gnorm_ref(g.cpu(), gs, mx)['norm']) > ref['b_norm']         # B's share is visible at these sizes


@pytest.mark.parametrize('n', SIZES[1:])
@pytest.mark.parametrize('value', (math.nan, math.inf))
def test_a_non_finite_value_counts_only_where_it_is_trainable(dev, n, value):
    from hftt_hip import ops
    segs = _segments(n)
    in_b = next((lo + hi) // 2 for lo, hi, k in segs if k == B)
    in_a = next(hi - 1 for lo, hi, k in reversed(segs) if k == A)
    qmap = _qmap(n, dev)
    ctl, ws = _buffers(n, dev)
    g = G.guard_grad(n, 'log_uniform').to(dev)
    g[in_b] = value
    ops.grad_norm_groups(g, qmap, 1 << B, ctl, ws)
    assert _record(ctl)[2:4] == (1, 0)                      # planted in the frozen group: applied
    ops.grad_norm_groups(g, qmap, 0, ctl, ws)
    assert _record(ctl)[2:4] == (0, 1)                      # ... and it does count when B is trainable
    g = G.guard_grad(n, 'log_uniform').to(dev)
    g[in_a] = value
    ops.grad_norm_groups(g, qmap, 1 << B, ctl, ws)
    assert _record(ctl)[2:4] == (0, 2)
    start = _state(n, dev)
    got = [t.clone() for t in start]
    ops.adam_step_groups(got[0], g, got[1], got[2], S0, qmap, lr=[1e-3, 1e-3, 1e-3], weight_decay=[0.01, 0.0, 0.0], frozen=[False, True, False], ctl=ctl)
    assert not G.skip_check(start, got)


def test_a_non_finite_value_in_the_only_segment_skips(dev):
    """n = 8: one segment, A's"""
    from hftt_hip import ops
    n = 8
    qmap = _qmap(n, dev)
    ctl, ws = _buffers(n, dev)
    g = G.guard_grad(n, 'log_uniform').to(dev)
    g[5] = math.nan
    ops.grad_norm_groups(g, qmap, 1 << B, ctl, ws)
    assert _record(ctl)[2:4] == (0, 1)
    start = _state(n, dev)
    got = [t.clone() for t in start]
    ops.adam_step_groups(got[0], g, got[1], got[2], S0, qmap, lr=[1e-3, 1e-3, 1e-3], frozen=[False, True, False], ctl=ctl)
    assert not G.skip_check(start, got)
