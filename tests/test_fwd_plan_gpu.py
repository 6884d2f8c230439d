"""The x3 (and parity) forward plans held to fp64, launch by launch.

The backward plan's check (tests/test_bwd_plan_gpu.py) reads the forward's saved tensors from the device and trusts them: the bf16 FFN
hidden, the bf16 pre-LayerNorm sums, mean / rstd, lse, the q / k / v planes, ctx.  A forward that saves something subtly wrong -- statistics
of the bf16-rounded sum, a hidden saved in front of its dropout -- passes every backward link and shows only through the whole-model bands.
And nothing held what PlanBuilder.forward hands each kernel: out_scale = sqrt(d), the position table and add_mod = F on the folded embedding,
layer zero's shared query (q_seq_stride = 0) and x3_to_planes, res_mod = N on its broadcast residual, layer j's column block of the merged
cross K / V, the pre-dropout attention map of a cross attention that runs WITH dropout, the _fuse_attn_out_ffn peephole, o.C = 0 in the
inference plan, time_embed_fwd's site and scale, heads_split on ldc = NHp, which sites _patch reaches.

Per (configuration, precision, plan): one ordinary forward (the training plan: with dropout 0.1 and the fused loss) on a NaN-filled
workspace; then everything is NaN-filled again and the SAME plan is stepped one entry at a time through HfttEngine._run with the same
ws['seed'] and ws['p'] -- no second forward call, the step counter does not move.  Around every launch the spans its descriptor names are
copied to the host and the launch is held to the fp64 contract of its kind (tests/fwd_plan_emul.py, written from include/hftt_hip.h) on the
device's OWN inputs; the saved tensors per element, under the bounds derived there.  A failing link names itself: plan index, op, kernel,
output buffers.

Conditions (none is a measurement): every entry is checked or listed in EXEMPT with a reason; no launch reads an element that is still
NaN-filled; none overwrites an element an earlier launch of the plan wrote; after the last launch every buffer the plan names as an output is
fully written -- but for the padding columns of the logits, which stay NaN to the bit --; in the inference plan no saved buffer is touched and
the x1 buffers of the fused layers stay NaN to the bit; the nine outputs and every buffer are bit-identical to the ordinary run; the scalars the
link check takes from a descriptor are what the graph says (fwd_plan_emul.PlanRules); the d.* buffers heads_split_bwd reads are the ones the
loss launch wrote and the attention map's pointer is outs[4]; with dropout 0 the training and the inference plan give the same nine outputs
to the bit; the stepped plans contain every (op, kernel) pair of a paper-width forward with three decoder layers.

Configurations, inputs and the attention conditioning are tests/test_bwd_plan_gpu.py's (CONFIGS, _case, _engine): the training plan's
attentions sit inside the score range the fixed attention bands with dropout were calibrated on, asserted here as there.  The inference
plan runs at p = 0, where the attention bounds follow the launch's own largest |score|."""
import time

import pytest
import torch

import bwd_plan_emul as PE
import elementwise_emul as EE
import fwd_plan_emul as FE
import util
from test_bwd_plan_gpu import (CONFIGS, P_DROP, UNCONDITIONED, _case, _case_raw, _engine, _pairs, attention_links,
                               first_layers_are_outside_the_table)
from util import O

pytestmark = pytest.mark.gpu

# plan entries the link check leaves out, by op name, and why (none: every kind of ws['fwd'] and ws['fwd_inf'] has a contract)
EXEMPT = {}
# scratch first allocated by the ordinary run's own loss call, i.e. behind its NaN fill: compared where the stepped run wrote
LOSS_SCRATCH = ('loss_ws', 'loss_out')


def _bits(t):
    return t.reshape(-1).view(torch.int32 if t.element_size() == 4 else torch.int16)


def _nan_bits(t):
    return _bits(torch.full((1,), float('nan'), dtype=t.dtype)).item()


def _is_nan_filled(t):
    return _bits(t) == _nan_bits(t)


def _fill(ws):
    for k, t in ws['bufs'].items():
        if t.is_floating_point() and k != 'spec':
            t.fill_(float('nan'))
    for t in ws['outs']:
        t.fill_(float('nan'))


def _new_outs(eng, B, dev):
    T, N, V = eng.T, eng.N, eng.V
    shapes = [(B, T, N)] * 3 + [(B, T, N, V), (B, T, eng.Hd, N, eng.F)] + [(B, T, N)] * 3 + [(B, T, N, V)]
    return [torch.full(s, float('nan'), device=dev) for s in shapes]


def _saved_addresses(plan):
    s = set()
    for e in plan:
        for d in FE._descs(e):
            s |= {a for a in (getattr(d, 'pre_ln_out', 0), getattr(d, 'ln_mean', 0), getattr(d, 'ln_rstd', 0), getattr(d, 'h_out', 0) if hasattr(d, 'site_h') else 0) if a}
    return s


def _run_case(dev, name, precision, training, lines):
    cfg, B = CONFIGS[name]
    sd, x, labels, lm, factors, table, seed = _case(name)
    assert max(lm.values()) <= table
    model, eng = _engine(dev, name, precision)
    labels_d = tuple(t.to(dev).contiguous() for t in labels)
    tag = '%s/%s/%s' % (name, precision, 'training' if training else 'inference')
    with torch.cuda.device(eng.device):
        ws = eng.workspace(B)
        outs = _new_outs(eng, B, dev)
        ws['outs'] = outs
        _fill(ws)
        # ---- the ordinary run
        eng.forward(x, training=training, outputs=outs, save=training)
        if training:
            eng.loss(B, labels_d, weight_A=EE.LOSS_W[0], weight_B=EE.LOSS_W[1])
        torch.cuda.synchronize()
        assert ws['p'] == (P_DROP if training else 0.0) and (ws['seed'] == seed or not training) and ws['saved'] == (training or 'fwd_inf' not in ws)
        assert eng.step_counter == (1 if training else 0)
        plan = ws['fwd'] if ws['saved'] else ws['fwd_inf']
        inference = not ws['saved']
        assert ('fwd_inf' in ws) == bool(ws['strip'])
        ref_bufs = {k: t.clone() for k, t in ws['bufs'].items()}
        ref_outs = [t.clone() for t in outs]
        # ---- producer checks that need no launch
        assert ws['attn_out_descs'] and all(ad.probs == outs[4].data_ptr() for ad in ws['attn_out_descs'])
        # ---- reset, then the stepped run
        _fill(ws)
        eng._patch(ws, ws['p'], ws['seed'])
        stream = torch.cuda.current_stream(dev).cuda_stream
        spans = FE.engine_spans(eng, ws)
        rules = FE.PlanRules(eng, ws, plan, inference)
        wrong = rules.static()
        assert not wrong, '%s: %s' % (tag, '; '.join(wrong))
        tracked = dict(ws['bufs'])
        tracked.update(zip(util.OUT_NAMES, outs))
        written = {k: torch.zeros(t.numel(), dtype=torch.bool) for k, t in tracked.items()}
        for entry in plan:
            assert entry[2] in FE.CONTRACTS or entry[2] in EXEMPT, 'plan entry %s is neither checked nor exempt' % entry[2]

        def launch(i, entry):
            eng._run(ws, plan[i:i + 1], stream, outs=outs, seed=ws['seed'], p=ws['p'])
            torch.cuda.synchronize()
        failures, by_kind, lmaxes = [], {}, []
        t0 = time.time()
        for i, entry, rec, ins, outb, figs in FE.step_plan(eng, ws, plan, launch, spans):
            me = FE.describe(i, entry, outb)
            for k in ins:                                # ---- nothing a launch reads is still NaN-filled
                t = rec[k]
                assert not bool(torch.isnan(t.double() if t.dtype == torch.bfloat16 else t).any()), '%s reads NaN-filled elements of %s (%s)' % (me, ins[k][0], k)
            for out, (tname, off, rows, cols, ld) in outb.items():          # ---- written exactly once
                idx = (off + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]).reshape(-1)
                assert not bool(written[tname][idx].any()), '%s overwrites elements of %s an earlier launch wrote (%s)' % (me, tname, out)
                written[tname][idx] = True
            bad = FE.failures(figs)
            if bad:
                failures.append((me, bad))
            wrong = rules.check(i, entry, rec, ins, outb)
            assert not wrong, '%s: %s' % (me, '; '.join(wrong))
            ratio, fig = FE.worst(figs)
            k = by_kind.setdefault(entry[2], [0.0, '', 0])
            k[2] += 1
            if ratio >= k[0]:
                k[0], k[1] = ratio, 'plan[%d] %s %s' % (i, (entry[3] or {}).get('kernel', '-'), fig)
            if entry[2] == 'attn_fwd':
                lmaxes.append(FE.attn_lmax(rec))
        assert not rules.finish(), (tag, rules.finish())
        # ---- the loss launch between the two plans, on the device's own nine outputs
        b = ws['bufs']
        if training:
            d_names = ['d.%s_%s' % (n, s) for s in 'AB' for n in ('onset', 'offset', 'mpe')] + ['d.velocity_A', 'd.velocity_B']
            assert not any(bool(written[n].any()) for n in d_names) and all(bool(_is_nan_filled(b[n]).all()) for n in d_names)
            n_lab = B * eng.T * eng.N
            rec = dict(kind='loss', probs=[outs[k].cpu().reshape(-1) for k in (0, 1, 2, 5, 6, 7)], vel=[outs[3].cpu(), outs[8].cpu()], lo=labels[0].float(),
                       lf=labels[1].float(), lm=labels[2].float(), lv=labels[3].long(), n=n_lab, V=eng.V)
            eng.loss(B, labels_d, weight_A=EE.LOSS_W[0], weight_B=EE.LOSS_W[1])
            torch.cuda.synchronize()
            got = dict(out=b['loss_out'][:9].cpu(), d_prob=[b[n].cpu().reshape(-1) for n in d_names[:6]], d_vel=[b[n].cpu().reshape(n_lab, eng.V) for n in d_names[6:]])
            figs = FE.check(rec, got)
            if FE.failures(figs):
                failures.append(('%s: the loss launch' % tag, FE.failures(figs)))
            ratio, fig = FE.worst(figs)
            by_kind['loss'] = [ratio, 'hftt_loss %s' % fig, 1]
            # the d.* buffers heads_split_bwd will read are the ones this launch wrote
            for e in ws['bwd']:
                if e[2] == 'heads_split_bwd':
                    for k, v in PE.launch_io(e, eng, ws)[0].items():
                        if k.startswith('d_'):
                            tname = spans.where(v[0], v[1], v[2], v[3])[0]
                            assert tname in d_names and not bool(torch.isnan(b[tname]).any()), 'heads_split_bwd reads %s, which the loss launch did not write' % tname
        wall = time.time() - t0
        torch.cuda.synchronize()
        for kind, (ratio, at, n) in sorted(by_kind.items()):
            lines.append('FWDPLAN %-30s %-15s worst measured / bound %.3g at %s; %d launches' % (tag, kind, ratio, at, n))
        lines.append('FWDPLAN %-30s %d launches stepped and checked in %.1f s; largest |score| over the attention launches %.2f' % (tag, len(plan), wall, max(lmaxes)))
        assert not failures, '\n'.join('%s: %s' % f for f in failures)
        if training:
            assert max(lmaxes) <= table, (tag, lmaxes)
        # ---- every buffer the plan names as an output is fully written; the declared gap: the padding columns of the logits, untouched
        for tname, w in written.items():
            if not bool(w.any()):
                continue
            missing = ~w
            if tname.startswith('logits_'):
                gap = (torch.arange(w.numel()) % eng.NHp) >= eng.NH
                assert torch.equal(missing, gap), '%s: %s is written outside [S, NH] or not all of it' % (tag, tname)
                assert bool(_is_nan_filled(tracked[tname]).cpu()[gap].all()), '%s: the padding columns of %s were touched' % (tag, tname)
            else:
                assert not bool(missing.any()), '%s: %d elements of %s are never written' % (tag, int(missing.sum()), tname)
        # ---- the inference plan: no saved buffer touched, the x1 of a fused layer never written
        if inference:
            for addr in sorted(_saved_addresses(ws['fwd'])):
                tname = spans.find(addr)[0]
                assert not bool(written[tname].any()) and bool(_is_nan_filled(tracked[tname]).all()), '%s: the saved buffer %s was touched' % (tag, tname)
            fused = [FE._descs(e) for e in plan if len(FE._descs(e)) == 2]
            assert fused or eng.strip_small or eng.fuse_offn_opt == '0'
            for o, f in fused:
                tname = spans.find(f.x)[0]
                assert not o.C and bool(_is_nan_filled(tracked[tname]).all()), '%s: x1 buffer %s of a fused layer was written' % (tag, tname)
        # ---- stepping changes nothing
        for t, r, n in zip(outs, ref_outs, util.OUT_NAMES):
            assert torch.equal(_bits(t), _bits(r)), '%s: output %s of the stepped run differs from the ordinary run' % (tag, n)
        for k, r in ref_bufs.items():
            t = ws['bufs'][k]
            same = _bits(t) == _bits(r)
            if k in LOSS_SCRATCH:
                same = same | _is_nan_filled(t)
            assert bool(same.all()), '%s: buffer %s of the stepped run differs from the ordinary run' % (tag, k)
        assert eng.step_counter == (1 if training else 0)
    return by_kind


@pytest.mark.parametrize('plan', ['training', 'inference'])
@pytest.mark.parametrize('precision', ['x3', 'parity'])
@pytest.mark.parametrize('name', list(CONFIGS))
def test_forward_plan_link_by_link(dev, name, precision, plan):
    lines = []
    try:
        _run_case(dev, name, precision, plan == 'training', lines)
    finally:
        print('\n' + '\n'.join(lines))


@pytest.mark.parametrize('name,precision', UNCONDITIONED)
def test_forward_plan_attention_links_unconditioned(dev, name, precision):
    """test_bwd_plan_gpu.py's unconditioned run for the training forward plan: no conditioning of fc_q, the input at synth_spec's own scale,
    every attn_fwd launch (out, the attention map where the launch writes one, row maximum, 1 / sum) held on the device's own operands under
    the derived bound of tests/attn_peaked_emul.py; the other links are run and not judged."""
    cfg, B = CONFIGS[name]
    sd, x, labels, seed = _case_raw(name)
    model, eng = _engine(dev, name, precision, sd)
    lines = []
    try:
        with torch.cuda.device(eng.device):
            ws = eng.workspace(B)
            outs = _new_outs(eng, B, dev)
            ws['outs'] = outs
            _fill(ws)
            eng.forward(x, training=True, outputs=outs, save=True)
            torch.cuda.synchronize()
            assert ws['p'] == P_DROP and ws['seed'] == seed and ws['saved']
            _fill(ws)
            eng._patch(ws, ws['p'], ws['seed'])
            tag = '%s/%s/forward' % (name, precision)
            reached = attention_links(eng, ws, ws['fwd'], True, FE, tag, lines)
            first_layers_are_outside_the_table(eng, B, reached, True, tag, lines)
    finally:
        print('\n' + '\n'.join(lines))


@pytest.mark.parametrize('name', list(CONFIGS))
def test_training_and_inference_plans_agree_without_dropout(dev, name):
    """an eval forward through the training plan (save=True) and through the inference plan: the same nine outputs to the bit (x3: the
    mode that has an inference plan)"""
    cfg, B = CONFIGS[name]
    x = _case(name)[1]
    model, eng = _engine(dev, name, 'x3')
    a = [t.clone() for t in eng.forward(x, training=False, save=True)]
    ws = eng._ws[B]
    assert ws['saved'] and ws['p'] == 0.0
    b = eng.forward(x, training=False, save=False)
    torch.cuda.synchronize()
    assert ws['saved'] == ('fwd_inf' not in ws) and ('fwd_inf' in ws) == bool(ws['strip'])
    for n, s, t in zip(util.OUT_NAMES, a, b):
        assert torch.equal(_bits(s), _bits(t)), '%s: %s differs between the training and the inference plan' % (name, n)


def _plans(eng, B):
    ws = eng.workspace(B)
    return _pairs(ws['fwd']), _pairs(ws.get('fwd_inf', []))


def test_stepped_plans_reach_every_kernel_of_the_paper_forward(dev):
    """(op, kernel) pairs of the plans stepped above against a paper-width forward with three decoder layers, built and not run; both plans"""
    paper = O.HfttConfig(**dict(O.PAPER.as_dict(), dec_layer=3))
    model = util.build_model(paper, 5, dropout=P_DROP).to(dev)
    model.hftt_precision = 'x3'
    model.train()
    eng = model.hftt_engine()
    with torch.cuda.device(eng.device):
        want = _plans(eng, 1)
    assert want[1], 'the paper-width workspace has no inference plan'
    del model, eng
    have = (set(), set())
    for name, (cfg, B) in CONFIGS.items():
        m = util.build_model(cfg, 5, dropout=P_DROP).to(dev)
        m.hftt_precision = 'x3'
        m.train()
        e = m.hftt_engine()
        with torch.cuda.device(e.device):
            got = _plans(e, B)
        have[0].update(got[0]); have[1].update(got[1])
    for what, w, h in zip(('training', 'inference'), want, have):
        assert w <= h, 'no stepped configuration reaches %s of the %s plan' % (sorted(w - h), what)
