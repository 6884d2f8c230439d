"""CPU: the fp32 restatement of the averaged weights (tests/ema_emul.py) passes every criterion on every input family, every defect fails on
a named family, the definition is torch's (torch.optim.swa_utils.get_ema_multi_avg_fn), and the warm-up schedule's first values are pinned.

Families: 'random' (adam_state parameters under adam_grad's gradient stream, an average that starts elsewhere, three calls, both decays);
'skip' (the same with a step the guard skips); 'frozen' (the same under a three-group map with one group frozen); 'stagnation' (2000 calls
at beta = 0.9999 towards a p that sits 2e-4 |e| away and does not move)."""
import pytest
import torch

import elementwise_emul as E
import ema_emul as M

N = 1028
STEPS = 3


def _adam_sequence(n, steps=STEPS, seed=0):
    """[(p_old, p_new)] of `steps` Adam calls in fp32 (adam_emul, step numbers 5 ..), and the average's start"""
    p, m, v, e0 = M.ema_start(n, seed)
    seq = []
    for k in range(steps):
        p1, m, v = E.adam_emul(p, E.adam_grad(n, 9 + seed, k), m, v, 5 + k)
        seq.append((p, p1))
        p = p1
    return seq, e0


def _run_random(beta, defect=None, n=N):
    seq, e0 = _adam_sequence(n)
    e, c = e0.clone(), torch.zeros(n)
    bad = []
    for k, (p_old, p_new) in enumerate(seq):
        e, c = M.ema_emul(e, c, p_new, beta, p_old=p_old, defect=defect)
        bad += M.ema_check(e, c, M.ema_ref(e0, [b for _, b in seq[:k + 1]], [beta] * (k + 1)))
    return bad


def _run_skip(beta, defect=None, n=N):
    """call 2 of 3 is skipped: p stays, and e and c must keep their bits"""
    seq, e0 = _adam_sequence(n)
    e, c = M.ema_emul(e0.clone(), torch.zeros(n), seq[0][1], beta, p_old=seq[0][0], defect=defect)
    e1, c1 = M.ema_emul(e, c, seq[0][1], beta, p_old=seq[0][1], apply=False, defect=defect)
    return M.bits_check('ema', e, e1) + M.bits_check('ema_c', c, c1)


def _run_frozen(beta, defect=None, n=N):
    seq, e0 = _adam_sequence(n)
    qmap = (torch.arange(n // 4) % 3).to(torch.uint8)
    fz = M.frozen_elements(qmap, (False, True, False))
    sent = torch.full((n,), M.SENTINEL, dtype=torch.int32).view(torch.float32)
    e, c = torch.where(fz, sent, e0), torch.where(fz, sent, torch.zeros(n))
    e1, c1 = M.ema_emul(e, c, seq[0][1], beta, p_old=seq[0][0], frozen=fz, defect=defect)
    bad = M.bits_check('frozen ema', e, e1, fz) + M.bits_check('frozen ema_c', c, c1, fz)
    return bad + M.ema_check(e1, c1, M.ema_ref(e0, [seq[0][1]], [beta]), keep=~fz)


def _run_stagnation(defect=None):
    p, e0 = M.stagnation_start()
    e, c = e0.clone(), torch.zeros_like(e0)
    for _ in range(M.STAG_K):
        e, c = M.ema_emul(e, c, p, M.STAG_BETA, p_old=p, defect=defect)
    ref = M.ema_ref(e0, [p] * M.STAG_K, [M.STAG_BETA] * M.STAG_K)
    return M.ema_check(e, c, ref), e, ref


FAMILIES = {'random': lambda d: [b for beta in M.EMA_DECAYS for b in _run_random(beta, d)],
            'skip': lambda d: _run_skip(0.9, d),
            'frozen': lambda d: _run_frozen(0.9, d),
            'stagnation': lambda d: _run_stagnation(d)[0]}

# which family sees which defect (recorded: the others pass it)
SEEN_BY = {'uncompensated': ('random', 'frozen', 'stagnation'),
           'averages_old_p': ('random', 'frozen'),
           'skip_still_averages': ('skip',),
           'frozen_quad_written': ('frozen',),
           'decay_rounded_before_subtraction': ('random', 'frozen')}       # (through e - c: the error is below e's own last rounding)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_the_restatement_passes_every_criterion(family):
    assert FAMILIES[family](None) == []


@pytest.mark.parametrize('n', [4, 8, 1020])
def test_the_restatement_passes_at_the_small_sizes(n):
    for beta in M.EMA_DECAYS:
        assert _run_random(beta, n=n) == []


@pytest.mark.parametrize('defect', M.DEFECTS)
def test_every_defect_fails_on_its_families_and_only_there(defect):
    seen = tuple(f for f in sorted(FAMILIES) if FAMILIES[f](defect))
    print(defect, '->', seen)
    assert seen == tuple(sorted(SEEN_BY[defect]))
    assert seen


def test_the_stagnation_family_is_what_it_says():
    """the fp64 average moves by about 300 ulp, the plain fp32 sum by none, the compensated sum follows within the bound (about an ulp)"""
    bad, e, ref = _run_stagnation()
    p, e0 = M.stagnation_start()
    ulp = 2.0 ** (torch.floor(torch.log2(e0.abs().double())) - 23)          # fp32 ulp of e0
    moved = ((ref['e'] - e0.double()).abs() / ulp)
    print('fp64 average moved by %.0f .. %.0f ulp; bound %.2f ulp at the most' % (float(moved.min()), float(moved.max()), float((ref['b_e'] / ulp).max())))
    assert float(moved.min()) > 150 and float(moved.max()) < 650
    assert float((ref['b_e'] / ulp).max()) < 3.0
    assert bad == []
    _, plain, _ = _run_stagnation('uncompensated')
    assert torch.equal(plain, e0)                     # not one element moved by one bit in 2000 calls
    assert float(((e.double() - e0.double()).abs() / ulp).min()) > 150


def test_the_definition_is_torchs_ema():
    """50 calls: torch.optim.swa_utils.get_ema_multi_avg_fn(beta) in fp64 from the same start IS ema_ref, and the restatement follows it
    within the bound"""
    from torch.optim.swa_utils import get_ema_multi_avg_fn
    n, steps = 1028, 50
    seq, e0 = _adam_sequence(n, steps)
    for beta in M.EMA_DECAYS:
        avg_fn = get_ema_multi_avg_fn(beta)
        t64 = [e0.double().clone()]
        e, c = e0.clone(), torch.zeros(n)
        for k, (p_old, p_new) in enumerate(seq):
            avg_fn(t64, [p_new.double()], k + 1)
            e, c = M.ema_emul(e, c, p_new, beta, p_old=p_old)
        ref = M.ema_ref(e0, [b for _, b in seq], [beta] * steps)
        assert float((t64[0] - ref['e']).abs().max()) <= 1e-13 * float(ref['e'].abs().max())
        assert E.violations('e against torch', e, t64[0], ref['b_e']) == []


def test_the_warmup_schedule_is_pinned():
    from hftt_hip.trainer import FusedAdam
    want = [0.1, 2.0 / 11.0, 0.25, 4.0 / 13.0, 5.0 / 14.0]
    for f in (M.warmup_decay, lambda d, t: FusedAdam.ema_decay_at(d, t, warmup=True)):
        assert [f(0.9999, t) for t in range(5)] == want
        assert f(0.9999, 89989) == 89990.0 / 89999.0 < 0.9999 and f(0.9999, 10 ** 6) == 0.9999       # the schedule meets the decay at t = 89990
        assert f(0.2, 0) == 0.1 and f(0.2, 2) == 0.2
    assert FusedAdam.ema_decay_at(0.9999, 0) == 0.9999
