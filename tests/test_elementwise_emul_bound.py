"""The fp64 criteria of tests/elementwise_emul.py separate right from wrong, without a GPU.

For every case of the GPU tests' input tables (tests/test_elementwise_fp64_gpu.py reads the same tables) the defect-free fp32 restatement of
each kernel passes its criterion -- for Adam torch.optim.Adam in fp32 does too, an independent implementation of the same step -- and every
named defect fails it on at least one case.  No criterion excludes an element; the references are asserted finite everywhere (excluded
share 0, below the 1 % allowed).

What the first-generation assertions (tensor-maximum / absolute tolerances, the sorted loss terms) make of the same defects ON THESE
INPUTS, as counted by the tests below (each prints its line): cases where the new criterion fails, and how many of those the old
assertion passes.

  LayerNorm backward (150 cases with M < 100)
    mean_over_n_minus_1             new fails 149   old passes 52 of them   (every row but the all-zero one; the old band sees it only on the fp32 streams)
    ragged_last_row_drops_s2        new fails  62   old passes 25           (a small last row is below the tensor maximum's resolution)
    clamped_row_counted             new fails  79   old passes 10
    r_rounded_to_bf16               new fails  53   old passes  0           (the fp32-r branches; seen by the old band too -- on inputs it never ran)
  Adam (n = 1027, 12 cases of 20 steps)
    eps_inside_bias_correction      new fails  12   old passes  0
    one_minus_beta2_in_fp32         new fails  12   old passes  0
    grad_scale_not_in_v             new fails   8   old passes  0           (the 4 cases with grad_scale = 1 are no defect)
    bias_correction_step_minus_1    new fails  12   old passes  0
    On the old test's OWN inputs (zero state, steps 1-3, gradients of 0.1, grad_scale 1: test_adam_old_inputs_hide_the_defects) its two
    bounds pass one_minus_beta2_in_fp32 and grad_scale_not_in_v; on the log-uniform gradients here they would see all four.
  loss (21 cases with n < 2000)
    log1p_clamp_missing             new fails  21   old passes  0           (NaN / Inf: any comparison sees it once a posterior is exactly 1)
    ce_grad_mean_over_nV            new fails  21   old passes  0
    terms_swapped                   new fails  21   old passes 21           (the sorted comparison cannot see it)
    grad_scale_missing_from_d_vel   new fails   9   old passes  0           (the cases with grad_scale = 0.25; the old test never set it)
  column sum (10 cases)
    last_split_dropped              new fails   6   old passes  0           (rows % 16 != 0)
    beta_on_partials                new fails   4   old passes  0           (beta = 0 onto a non-zero destination, which the old test never ran)
  time-embedding backward (8 cases at the small shape)
    accumulate_overwrites           new fails   8   old passes  4           (the bf16 stream: the lost dx0 is inside the 6e-3 band)
    scale_on_dym                    new fails   4   old passes  0           (the cases that pass dym)

Transcendentals, measured by test_cpu_transcendentals_are_within_the_margin: the restatement's fp32 log / log1p / exp (torch on the CPU)
are within 0.546 / 0.620 / 0.554 ulp of fp64 over 2^20 arguments; the HIP math API documents 1 ulp for logf, log1pf and expf; the criteria
allow 2 ulp per call (elementwise_emul.C_LOG, C_EXP = 4 U32): the documented ulp plus one of margin.  No figure comes from a kernel's output.

The bf16 unit roundoff is 2^-8 (8 significand bits), not 2^-9: with 2^-9 the correctly rounded store of the restatement itself fails
(|err| = 2^-15 on a value just above 2^-7, whose bf16 ulp is 2^-14).
"""
import pytest
import torch

import util
import elementwise_emul as E


def _report(kernel, defect, new_fail, old_pass, total):
    print('%s / %s: the new criterion fails %d of %d cases; the old assertion passes %d of those' % (kernel, defect, new_fail, total, old_pass))


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_run(branch, family, M, defect=None):
    spec = E.LN_BRANCHES[branch]
    c = E.ln_inputs(branch, family, M)
    p = E.LN_DROP['p'] if spec['drop'] else 0.0
    mask = E.ln_mask(M, spec['N'], p, E.LN_DROP['site'], E.LN_DROP['seed']) if spec['drop'] else None
    ref = E.ln_bwd_ref(c, mask, p)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    got = E.ln_bwd_emul(c, R=spec['R'], dr_bf=spec['dr_bf'], drop=spec['drop'], mask=mask, p=p, defect=defect)
    bad = E.ln_bwd_check(got, ref, dr_bf=spec['dr_bf'], drop=spec['drop'], mask=mask, p=p)
    return bad, E.ln_old_passes(got, ref, dr_bf=spec['dr_bf'], drop=spec['drop'])


@pytest.mark.parametrize('branch', list(E.LN_BRANCHES))
def test_ln_bwd_restatement_passes(branch):
    for family in E.LN_FAMILIES:
        for M in E.LN_BRANCHES[branch]['Ms']:
            bad, _ = _ln_run(branch, family, M)
            assert not bad, (branch, family, M, bad)


@pytest.mark.parametrize('defect', E.DEFECTS['ln_bwd'])
def test_ln_bwd_defect_fails(defect):
    cases = [(b, f, M) for b, f, M in E.ln_cases() if M < 100]
    res = [_ln_run(b, f, M, defect) for b, f, M in cases]
    new_fail = [r for r in res if r[0]]
    _report('ln_bwd', defect, len(new_fail), sum(r[1] for r in new_fail), len(cases))
    assert new_fail, 'the criterion does not see ' + defect


# ------------------------------------------------------------------------------------------------ Adam
def _adam_run(n, gs, eps, s0, step_fn, steps=E.ADAM_STEPS):
    """`steps` steps of step_fn from the shared state; every step is held to the fp64 step from ITS OWN previous state"""
    seed = n % 1000 + int(gs * 12) + s0
    p, m, v = E.adam_state(n, seed)
    p0, idle = p.clone(), E.adam_idle(n)
    bad, old_ok = [], True
    for k in range(steps):
        g = E.adam_grad(n, seed, k)
        ref = E.adam_ref(p, g, m, v, s0 + k, eps=eps, grad_scale=gs)
        assert all(bool(torch.isfinite(t).all()) for t in ref.values())
        p, m, v = step_fn(p, g, m, v, s0 + k, eps, gs)
        bad += E.adam_check(p, m, v, ref)
        old_ok = old_ok and util.max_err(p, ref['p']) < 1e-6 and util.max_err(v, ref['v']) < 1e-8       # test_colsum_and_adam's two bounds
        if bad:
            break
    if not bad:
        assert torch.equal(p[idle], p0[idle])
    return bad, old_ok


def _torch_adam(p, g, m, v, step, eps, gs):
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([q], lr=E.ADAM_LR, betas=(E.ADAM_B1, E.ADAM_B2), eps=eps, foreach=False)
    opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    q.grad = g * E.f32(gs)
    opt.step()
    st = opt.state[q]
    return q.detach(), st['exp_avg'], st['exp_avg_sq']


@pytest.mark.parametrize('impl', ['restatement', 'torch.optim.Adam'])
def test_adam_implementations_pass(impl):
    fn = _torch_adam if impl != 'restatement' else (lambda p, g, m, v, s, eps, gs: E.adam_emul(p, g, m, v, s, eps=eps, grad_scale=gs))
    for n, gs, eps, s0 in E.adam_cases():
        bad, _ = _adam_run(n, gs, eps, s0, fn, steps=E.ADAM_STEPS if n < 10 ** 6 else 2)      # (the large n: two steps here, twenty on the device)
        assert not bad, (impl, n, gs, eps, s0, bad)


@pytest.mark.parametrize('defect', E.DEFECTS['adam'])
def test_adam_defect_fails(defect):
    cases = [c for c in E.adam_cases() if c[0] == 1027]
    fn = lambda p, g, m, v, s, eps, gs: E.adam_emul(p, g, m, v, s, eps=eps, grad_scale=gs, defect=defect)      # noqa: E731
    res = [_adam_run(*c, fn) for c in cases]
    new_fail = [r for r in res if r[0]]
    _report('adam', defect, len(new_fail), sum(r[1] for r in new_fail), len(cases))
    assert new_fail, 'the criterion does not see ' + defect


def test_adam_old_inputs_hide_the_defects():
    """the first-generation test's own inputs (zero state, steps 1-3, gradients of 0.1, grad_scale 1) and bounds: which defects pass there"""
    g0 = torch.Generator().manual_seed(1)
    n = 100003
    p0 = torch.randn(n, generator=g0); gr = torch.randn(n, generator=g0) * 0.1
    passed = []
    for defect in E.DEFECTS['adam']:
        p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
        pr, mr, vr = p0.clone(), torch.zeros(n), torch.zeros(n)
        for step in (1, 2, 3):
            p, m, v = E.adam_emul(p, gr, m, v, step, defect=defect)
            util.O.adam_step([pr], [gr], [mr], [vr], step, lr=1e-3)
        if bool(torch.isfinite(p).all()) and util.max_err(p, pr) < 1e-6 and util.max_err(v, vr) < 1e-8:
            passed.append(defect)
    print('adam, old inputs and bounds: pass', passed)
    assert 'one_minus_beta2_in_fp32' in passed and 'grad_scale_not_in_v' in passed


# ------------------------------------------------------------------------------------------------ loss
def _loss_run(V, n, gs, defect=None):
    c = E.loss_inputs(V, n)
    ref = E.loss_ref(c, gs)
    assert bool(torch.isfinite(ref['out']).all()) and all(bool(torch.isfinite(t).all()) for t in ref['d_prob'] + ref['d_vel'])
    out, dp, dv = E.loss_emul(c, gs, defect)
    return E.loss_check(out, dp, dv, ref), E.loss_old_passes(out, dp, dv, ref)


def test_loss_restatement_passes():
    for _, V, n, gs in E.LOSS_CASES:
        bad, _ = _loss_run(V, n, gs)
        assert not bad, (V, n, gs, bad)


@pytest.mark.parametrize('defect', E.DEFECTS['loss'])
def test_loss_defect_fails(defect):
    cases = [c for c in E.LOSS_CASES if c[2] < 2000]
    res = [_loss_run(V, n, gs, defect) for _, V, n, gs in cases]
    new_fail = [r for r in res if r[0]]
    _report('loss', defect, len(new_fail), sum(r[1] for r in new_fail), len(cases))
    assert new_fail, 'the criterion does not see ' + defect
    if defect == 'terms_swapped':
        assert len(new_fail) == len(cases) and all(r[1] for r in new_fail)       # the sorted comparison cannot see it, anywhere


def test_cpu_transcendentals_are_within_the_margin():
    """the restatement's own logf / log1pf / expf against fp64, in ulps of fp32 -- the measurement E.C_LOG and E.C_EXP leave room for"""
    g = torch.Generator().manual_seed(0)
    p = torch.rand(1 << 20, generator=g)
    x = -(torch.rand(1 << 20, generator=g) * 80)

    def ulps(f32v, f64v):
        a = f64v.abs()
        ulp = 2.0 ** (torch.floor(torch.log2(a.clamp_min(1e-300))) - 23)
        return float(((f32v.double() - f64v).abs() / ulp)[a > 0].max())
    e_log, e_log1p, e_exp = ulps(torch.log(p), torch.log(p.double())), ulps(torch.log1p(-p), torch.log1p(-p.double())), ulps(torch.exp(x), torch.exp(x.double()))
    print('CPU fp32 against fp64, worst ulp error: log %.3f, log1p %.3f, exp %.3f' % (e_log, e_log1p, e_exp))
    # 1 ulp = 2 U32; the criteria allow C / 2 ulp per call
    assert e_log <= E.C_LOG / 2 and e_log1p <= E.C_LOG / 2 and e_exp <= E.C_EXP / 2


# ------------------------------------------------------------------------------------------------ column sum
def _colsum_run(rows, n, pad, bf, beta, defect=None):
    c = E.colsum_inputs(rows, n, pad, bf)
    ref, bound = E.colsum_ref(c, beta)
    assert bool(torch.isfinite(ref).all())
    got = E.colsum_emul(c, beta, defect)
    return E.violations('colsum', got, ref, bound), E.colsum_old_passes(got, ref)


def test_colsum_restatement_passes():
    for case in E.COLSUM_CASES:
        bad, _ = _colsum_run(*case)
        assert not bad, (case, bad)


@pytest.mark.parametrize('defect', E.DEFECTS['colsum'])
def test_colsum_defect_fails(defect):
    res = [_colsum_run(*case, defect=defect) for case in E.COLSUM_CASES]
    new_fail = [r for r in res if r[0]]
    _report('colsum', defect, len(new_fail), sum(r[1] for r in new_fail), len(res))
    assert new_fail, 'the criterion does not see ' + defect


# ------------------------------------------------------------------------------------------------ time-embedding backward
def _te_run(shape, half, p, with_dym, defect=None):
    B, T, N, d = shape
    c = E.te_inputs(shape, half)
    mask = util.keep_mask_t(E.TE_DROP['seed'], E.TE_DROP['site'], (B * N, T, d), p) if p > 0 else None
    ref = E.te_bwd_ref(c, mask, p, half)
    assert bool(torch.isfinite(ref['dx']).all())
    dx, dym = E.te_bwd_emul(c, mask, p, half, defect)
    dym = dym if with_dym else None
    return E.te_bwd_check(dx, dym, ref), E.te_old_passes(dx, dym, ref, half)


def test_time_embed_bwd_restatement_passes():
    for case in E.TE_CASES:
        bad, _ = _te_run(*case)
        assert not bad, (case, bad)


@pytest.mark.parametrize('defect', E.DEFECTS['time_embed_bwd'])
def test_time_embed_bwd_defect_fails(defect):
    cases = [c for c in E.TE_CASES if c[0] == E.TE_SHAPES[0]]
    res = [_te_run(*c, defect=defect) for c in cases]
    new_fail = [r for r in res if r[0]]
    _report('time_embed_bwd', defect, len(new_fail), sum(r[1] for r in new_fail), len(cases))
    assert new_fail, 'the criterion does not see ' + defect
