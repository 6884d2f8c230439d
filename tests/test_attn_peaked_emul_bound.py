"""The peaked-row attention criterion on the CPU (tests/attn_peaked_emul.py): the input conditions hold, the fp32 stand-in of the x3 chain, the
plain fp32 chain (parity) and the fp64 x3 model pass both layers at every family x magnitude x geometry, every planted defect fails at the
figure it names, and the one defect that cannot be seen is shown not to be.  Last: the existing peaked kernel case
(test_x3_gpu.py::test_attention_fwd_bwd[qk_scale=40]) restated -- its own inequality on dq / dk is passed by dq = dk = 0."""
import math

import pytest
import torch

import attn_peaked_emul as A

GEOM_IDS = ['-'.join(map(str, g)) for g in A.GEOMS]
SMALL = A.GEOMS[0]


def _setting(gi, vi):
    """dropout of the (geometry, v form) pair: both v forms and both dropout settings at every geometry, crossed the other way at the next one"""
    return 0.1 if (gi + vi) % 2 else 0.0


def _case(family, geom, L, v_form, drop, shared=False):
    q, k, v, do = A.make(family, geom, L, v_form, shared)
    mask, ks = A.dropout_mask(geom, drop, 7, 99) if drop > 0 else (None, 1.0)
    return A.Case(q, k, v, do, geom[1], mask, ks), (q, k, v, do)


@pytest.mark.parametrize('geom', A.GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize('L', A.MAGS)
@pytest.mark.parametrize('family', A.FAMILIES)
def test_models_pass_and_input_conditions_hold(family, L, geom):
    gi = A.GEOMS.index(geom)
    worst = {}
    for vi, v_form in enumerate(A.V_FORMS):
        for shared in ((False, True) if geom == (2, 4, 88, 256, 64) else (False,)):
            drop = _setting(gi, vi)
            case, (q, k, v, do) = _case(family, geom, L, v_form, drop, shared)
            mag = A.magnitude(q, k, geom[1])
            tag = '%s L %g %s %s drop %g%s' % (family, L, geom, v_form, drop, ' shared' if shared else '')
            assert 0.5 * L <= mag <= 5.0 * L, (tag, mag)
            for t in (q, k, v, do):
                assert t.dtype == torch.float32
            if drop == 0.0:
                case.assert_conditions(tag)
            else:
                A.Case(q, k, v, do, geom[1]).assert_conditions(tag)          # the conditions are those of the undropped rows
            for name, got, mode in (('stand-in x3/fp32', A.chain(q, k, v, do, geom[1], A.F32, 'x3', case.mask, case.keep_sc), 'x3'),
                                    ('model x3/fp64', case.x3, 'x3'),
                                    ('stand-in parity/fp32', case.e32, 'parity')):
                figs, bad = A.check(case, got, mode)
                assert not bad, (tag, name, bad)
                for f, (ratio, e_dev, allow) in figs.items():
                    w = worst.setdefault((name, f), [0.0, 0.0])
                    w[0], w[1] = max(w[0], ratio), max(w[1], e_dev / allow)
            print('PEAKED-CPU %-60s reached %.4g  conditions %s' % (tag, mag, ' '.join('%.2f' % c for c in A.Case.conditions(case))))
    for name in ('stand-in x3/fp32', 'model x3/fp64', 'stand-in parity/fp32'):
        print('PEAKED-CPU %s L %g %s %-22s worst measured / bound: %s' % (family, L, geom, name, '  '.join('%s %.3g' % (f, worst[(name, f)][0]) for f in A.FIGURES)))


@pytest.mark.parametrize('defect', list(A.DEFECTS))
def test_each_planted_defect_fails_at_its_named_figure(defect):
    family, L, v_form, drop, figure = A.DEFECTS[defect]
    case, (q, k, v, do) = _case(family, SMALL, L, v_form, drop)
    clean = A.chain(q, k, v, do, SMALL[1], A.F32, 'x3', case.mask, case.keep_sc)
    assert not A.check(case, clean, 'x3')[1]
    got = A.chain(q, k, v, do, SMALL[1], A.F32, 'x3', case.mask, case.keep_sc, defect=defect)
    figs, bad = A.check(case, got, 'x3')
    print('PEAKED-CPU defect %-20s %s L %g %s drop %g: %s' % (defect, family, L, v_form, drop, '; '.join(bad)))
    assert any(b.startswith(figure + ':') for b in bad), (defect, figure, figs)


def test_the_defect_that_cannot_be_seen():
    """scale_then_subtract: (s c) - (max c) in fp32.  Its error is U32 |s| per score, (dh + 16) x below the score term of the bound, and the
    fp32 evaluation that e32 comes from rounds in the same place: it passes at every magnitude, here shown at the two largest.  (Its failure
    mode -- the whole row underflowing at |score| 1e9 -- is held on exact inputs by test_x3_gpu.py::test_attention_with_scores_of_1e9;
    max_from_hi above is the nearest defect this criterion does see.)"""
    for L in (1500.0, 1.0e5):
        for family in A.FAMILIES:
            case, (q, k, v, do) = _case(family, SMALL, L, 'randn', 0.0)
            got = A.chain(q, k, v, do, SMALL[1], A.F32, 'x3', defect='scale_then_subtract')
            figs, bad = A.check(case, got, 'x3')
            assert not bad
            assert figs['map'][0] < 1.0 / 16


def test_layer_a_alone_is_loose_and_layer_b_alone_is_blind():
    """why the criterion has two layers.  near_dup: the derived bound on dq does not cancel, so the fp64 x3 model sits far below it -- a
    dq error 10 x the model's own still passes (a) and fails (b).  One wrong row of the map passes (b)'s max-normalised figure when the row
    is not the one that carries the maximum, and fails (a)."""
    case, (q, k, v, do) = _case('near_dup', SMALL, 1500.0, 'common', 0.0)
    figs, bad = A.check(case, case.x3, 'x3')
    assert not bad and figs['dq'][0] < 0.1
    worse = dict(case.x3)
    worse['dq'] = case.ref['dq'] + 10.0 * (case.x3['dq'] - case.ref['dq'])
    figs, bad = A.check(case, worse, 'x3')
    assert figs['dq'][0] <= 1.0 and any(b.startswith('dq: (b)') for b in bad)
    case, (q, k, v, do) = _case('solved_ties', SMALL, 45.0, 'randn', 0.0)
    dv = case.ref['dv'].clone()
    row = dv.abs().amax(-1).view(-1).argsort()[dv.shape[0] * dv.shape[1] // 4]          # a small (but live) row of dv
    allow = A.check(case, case.x3, 'x3')[0]['dv'][2]
    dv.view(-1, dv.shape[-1])[row] += 0.5 * allow * dv.abs().max()
    figs, bad = A.check(case, dict(case.x3, dv=dv), 'x3')
    assert figs['dv'][1] <= figs['dv'][2] and any(b.startswith('dv: (a)') for b in bad)


def test_plane_storage_needs_its_absolute_term():
    """The case the device found (solved_ties, magnitude 45, 88 x 256, dropout 0.1, q / k / v as f16-pair planes): the backward forms its
    bf16 pairs from the stored hi + lo, which is off by up to 2^-25 ABSOLUTE where lo is subnormal.  An element of q near zero then moves dk by
    more than any relative unit on |q| allows: without the term the planes model is 2.38 x the bound on dk (as the kernel was), with it
    0.34 -- and the fp32-operand chain never needed it."""
    geom = (2, 4, 88, 256, 64)
    case, (q, k, v, do) = _case('solved_ties', geom, 45.0, 'randn', 0.1)
    for dtype in (A.F32, A.F64):
        got = A.chain(q, k, v, do, geom[1], dtype, 'x3', case.mask, case.keep_sc, planes=True)
        figs, bad = A.check(case, got, 'x3', planes=False)
        assert figs['dk'][0] > 2.0 and any(b.startswith('dk: (a)') for b in bad)
        figs, bad = A.check(case, got, 'x3', planes=True)
        assert not bad and figs['dk'][0] < 0.5
    assert A.check(case, A.chain(q, k, v, do, geom[1], A.F32, 'x3', case.mask, case.keep_sc), 'x3', planes=False)[0]['dk'][0] < 0.05


@pytest.mark.parametrize('n,H,Lq,Lk,dh', [(5, 4, 256, 256, 64), (4, 2, 48, 48, 32), (5, 4, 88, 256, 64)])
def test_the_qk_scale_40_case_of_the_kernel_test_cannot_see_a_gradient(n, H, Lq, Lk, dh):
    """test_x3_gpu.py::test_attention_fwd_bwd[qk_scale=40], its inputs and its inequality restated: dq / dk are judged against
    gtol * nat, nat a product of operand maxima.  dq = dk = 0 passes; the allowed error is several times the largest element of the true
    dq; hardly a row has a second live key."""
    d = H * dh
    g = torch.Generator().manual_seed(Lq * 1000 + Lk + dh)
    if Lq == Lk:
        qkv = torch.randn(n, Lq, 3 * d, generator=g)
        qkv[..., :2 * d] *= 40.0
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    else:
        q = torch.randn(n, Lq, d, generator=g) * 40.0
        kv = torch.randn(n, Lk, 2 * d, generator=g)
        kv[..., :d] *= 40.0
        k, v = kv[..., :d], kv[..., d:]
    do = torch.randn(n, Lq, d, generator=g) * 1e-5
    ref = A.chain(q, k, v, do, H, A.F64, 'plain')
    lmax = A.magnitude(q, k, H)
    ptol = 4e-6 + 4e-7 * lmax
    gtol = 2e-4 + 3 * ptol
    nat = do.abs().max().item() * v.abs().max().item() * max(q.abs().max().item(), k.abs().max().item()) * math.sqrt(dh)
    zero = torch.zeros_like(ref['dq'])
    assert (zero - ref['dq']).abs().max().item() < gtol * nat            # the test's own assert on dq, met by dq = 0
    assert (torch.zeros_like(ref['dk']) - ref['dk']).abs().max().item() < gtol * nat
    times = gtol * nat / ref['dq'].abs().max().item()
    live = (ref['map'].topk(2, -1).values[..., 1] > 1e-3).double().mean().item()
    print('PEAKED-CPU qk_scale=40 %s: allowed error = %.1f x max |dq|, rows with a second probability above 1e-3: %.2f %%' % ((n, H, Lq, Lk, dh), times, 100 * live))
    assert times > 2.0 and live < 0.03
