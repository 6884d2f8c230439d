"""The criteria of tests/guard_emul.py, on the CPU: each passes the restatement of its kernel on every case of tests/test_guard_gpu.py and
fails every listed defect.  Which input family sees which defect (cases = n x family x grad_scale x max_norm for the norm, n = 1025 x family
x grad_scale x max_norm x weight_decay, three steps, for the update; a planted family gives the update planted, clean, planted gradients):

  norm                              families whose cases fail (number of failing cases)
    squares_summed_in_fp32          huge 42, tiny 42            (1e60 overflows to a skipped step, 1e-60 vanishes to norm 0; on log_uniform an
                                                                 fp32 sum of <= 2^21 positive terms stays inside 2 U32: range is what fp64 buys)
    tail_dropped                    log_uniform 24, huge 36, tiny 36 (n = 1, 3, 5 and wherever the tail carries weight), +-inf / nan @tail 36
                                    each (the planted element is never read: the step is applied), +-inf / nan @first 12 each (n < 4: all tail)
    norm_of_unscaled_gradient       log_uniform 21, huge 21, tiny 21  (every case with grad_scale = 0.25; zeros and the planted ones cannot tell)
    clip_eps_missing                log_uniform 9               (coef < 1 and norm < 8: the 1e-6 moves coef by 1e-6 / norm > 2 U32)
  update
    clip_not_in_v                   log_uniform 4, each planted family 4 (its clean step)   (the cases with coef < 1)
    skip_still_updates_v            each planted family 12      (all their cases: skip_check compares bits)
    decay_after_update              log_uniform 6, zeros 6, each planted family 6           (all cases with weight_decay 0.01: seen where p is an
                                                                 exact zero, there p = -update and update * lr * wd stands against ~17 U32 of it)
    decay_coupled_into_gradient     log_uniform 6, zeros 6, each planted family 6           (p misses its factor 1 - lr wd: 1e-5 |p| against 3 U32 |p|)
"""
import math

import pytest
import torch

import elementwise_emul as E
import guard_emul as G


_GRADS = {}


def _grad(n, fam):
    if (n, fam) not in _GRADS:
        _GRADS[(n, fam)] = G.guard_grad(n, fam)              # computed once, shared, never written
    return _GRADS[(n, fam)]


def _gnorm_cases():
    for n in G.GUARD_N:
        for fam in G.FAMILIES:
            g = _grad(n, fam)
            if g is None:
                continue
            for gs in G.GRAD_SCALES:
                for mx in G.MAX_NORMS:
                    yield n, fam, gs, mx, g


def _gnorm_bad(g, gs, mx, defect):
    ref = G.gnorm_ref(g, gs, mx)
    norm, coef, apply = G.gnorm_emul(g, gs, mx, defect=defect)
    bad = G.gnorm_check(norm, coef, apply, ref)
    # the counters of a zeroed record after this one call
    bad += G.counters_check(int(not apply), int(bool(apply) and coef < 1.0), coef, ref)
    return bad


def test_gnorm_restatement_passes_every_case():
    seen = set()
    for n, fam, gs, mx, g in _gnorm_cases():
        bad = _gnorm_bad(g, gs, mx, None)
        assert not bad, (n, fam, gs, mx, bad)
        ref = G.gnorm_ref(g, gs, mx)
        seen.add((ref['apply'], ref['clipped']))
        if fam in G.FINITE_FAMILIES:
            assert ref['apply'] == 1, (n, fam)                   # +-1e30 everywhere is NOT skipped
            if fam == 'tiny':
                assert ref['norm'] > 0.0
            if fam == 'zeros':
                assert ref['coef'] == 1.0 and ref['norm'] == 0.0
        else:
            assert ref['apply'] == 0, (n, fam)
    assert {(1, 0), (1, 1), (0, 0)} <= seen                      # coef == 1, coef < 1 and skipped all occur


@pytest.mark.parametrize('defect', G.DEFECTS['gnorm'])
def test_gnorm_defect_fails(defect):
    caught = {}
    for n, fam, gs, mx, g in _gnorm_cases():
        if _gnorm_bad(g, gs, mx, defect):
            caught[fam] = caught.get(fam, 0) + 1
    print('gnorm %-28s caught by %s' % (defect, sorted(caught.items())))
    assert caught, 'the criterion does not see ' + defect
    must = {'squares_summed_in_fp32': ('huge', 'tiny'), 'tail_dropped': ('log_uniform', '+inf@tail', '-inf@tail', 'nan@tail'),
            'norm_of_unscaled_gradient': ('log_uniform', 'huge', 'tiny'), 'clip_eps_missing': ('log_uniform',)}[defect]
    assert all(f in caught for f in must), (defect, sorted(caught))


ADAM_N = 1025
STEPS = 3


def _adam_run(fam, gs, mx, wd, defect, s0=5):
    """three steps from adam_state; every step against the fp64 step from ITS OWN previous state; a planted family alternates with clean
    gradients (planted, clean, planted): the skipped steps must leave no trace, the clean one must equal the model at its step number"""
    n = ADAM_N
    p, m, v = E.adam_state(n, 17)
    bad = []
    for k in range(STEPS):
        g = G.guard_grad(n, fam if (fam in G.FINITE_FAMILIES or k != 1) else 'log_uniform', seed=k)
        norm, coef, apply = G.gnorm_emul(g, gs, mx)
        q = G.guarded_adam_emul(p, g, m, v, s0 + k, coef, apply, grad_scale=gs, weight_decay=wd, defect=defect)
        if apply:
            ref = G.guarded_adam_ref(p, g, m, v, s0 + k, coef, grad_scale=gs, weight_decay=wd)
            bad += G.guarded_adam_check(*q, ref)
        else:
            bad += G.skip_check((p, m, v), q)
        p, m, v = q
        if bad:
            break
    return bad


def _adam_cases():
    # (huge / tiny are the norm's families: gr * gr leaves fp32 in the second moment of any Adam, guarded or not, and no bound models that)
    for fam in ('log_uniform', 'zeros', 'nan@first', '+inf@tail', '-inf@last_quad'):
        for gs in G.GRAD_SCALES:
            for mx in G.MAX_NORMS:
                for wd in G.WEIGHT_DECAYS:
                    yield fam, gs, mx, wd


def test_guarded_adam_restatement_passes_every_case():
    for c in _adam_cases():
        bad = _adam_run(*c, None)
        assert not bad, (c, bad)


def test_guarded_adam_restatement_is_adam_emul_when_inactive():
    '''coef == 1 and weight_decay == 0: the restatement is elementwise_emul.adam_emul bit for bit (what the device test asks of the kernels)'''
    p, m, v = E.adam_state(ADAM_N, 3)
    for gs in G.GRAD_SCALES:
        g = G.guard_grad(ADAM_N, 'log_uniform')
        a = G.guarded_adam_emul(p, g, m, v, 7, 1.0, 1, grad_scale=gs)
        b = E.adam_emul(p, g, m, v, 7, grad_scale=gs)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('defect', G.DEFECTS['adam'])
def test_guarded_adam_defect_fails(defect):
    caught = {}
    for fam, gs, mx, wd in _adam_cases():
        if _adam_run(fam, gs, mx, wd, defect):
            caught[fam] = caught.get(fam, 0) + 1
    print('adam  %-28s caught by %s' % (defect, sorted(caught.items())))
    assert caught, 'the criterion does not see ' + defect
    must = {'clip_not_in_v': ('log_uniform',), 'skip_still_updates_v': ('nan@first', '+inf@tail', '-inf@last_quad'),
            'decay_after_update': ('log_uniform', 'zeros'), 'decay_coupled_into_gradient': ('log_uniform', 'zeros')}[defect]
    assert all(f in caught for f in must), (defect, sorted(caught))


def test_the_bound_of_the_norm_is_tight_enough_to_matter():
    '''2 U32 relative: a norm accumulated in fp32 the way clip_flat_gradient_ of the old tool did (vector_norm) is NOT what fails here -- the
    criterion is about range and the missing pieces; but it does reject a value one fp32 ulp pair away'''
    g = G.guard_grad(1025, 'log_uniform')
    ref = G.gnorm_ref(g, 1.0, 1e-3)
    norm, coef, apply = G.gnorm_emul(g, 1.0, 1e-3)
    assert not G.gnorm_check(norm, coef, apply, ref)
    assert G.gnorm_check(norm * (1 + 4 * E.U32), coef, apply, ref) and G.gnorm_check(norm, coef * (1 - 4 * E.U32), apply, ref)
    assert math.isfinite(ref['norm']) and 0.0 < ref['coef'] < 1.0
