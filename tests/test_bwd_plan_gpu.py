"""The x3 (and parity) training backward held to fp64, launch by launch.

The kernel tests run the backward's kernels on operands of their own; the whole-model gradient checks allow 2e-2 .. 3e-2 on the first-layer
tensors and name a parameter, not a launch.  Nothing held what PlanBuilder.build_backward hands each kernel: out_scale = sqrt(d) on the
embedding product, the gate_scale written by HfttEngine._patch, beta = 1 on accumulating segments, the six-segment stacked K / V product,
K_out, HFTT_TN_DY_DROP in place of a masked copy, residual = the LayerNorm backward's dr on the dX launches, accumulate = 1 in
time_embed_bwd, which buffer the position tables' column sums read, the pruned plan of a frozen encoder.

Here one training forward with dropout 0.1 and the fused loss run as ever; then the backward plan is stepped ONE ENTRY AT A TIME through
HfttEngine._run (the same call the engine makes on the whole list).  Around every launch the spans its descriptor names are copied to the
host -- inputs, and the prior contents of every output -- and the launch is held to the fp64 contract of its kind (tests/bwd_plan_emul.py,
written from include/hftt_hip.h) on the device's OWN inputs, under the bound that kind's kernel test already carries.  Weight operands are
taken from flat_params through the layout's own table entries.  A failing link names itself: plan index, op, kernel, output buffer.

Conditions (none is a measurement): every entry is checked or listed in EXEMPT with a reason; flat_grads after the stepped run is
bit-identical to an ordinary backward of the same forward; on a NaN-filled flat_grads no launch accumulates into an element no launch has
written, none overwrites a written one, no parameter's element is NaN at the end, and with the encoder frozen everything below the border
stays NaN to the bit; every dropout site a backward descriptor names is a forward descriptor's, and no two forward launches share one; the
column sums of the position tables and of layer zero's query read what the launch the graph names produced; the scalars the link check
takes from a descriptor are what the graph says (bwd_plan_emul.PlanRules: sites against the forward plan, a gradient operand masked exactly
once, every dr added back once, gate_scale = 1 / keep, segments = whole parameters, out_scale = sqrt(d) on the embedding product alone);
the stepped plans contain every (op, kernel) pair of a paper-width three-decoder-layer backward.

Attention conditioning.  The attention bands with dropout are fixed numbers calibrated on randn scores: the largest |score| the ATTN_CASES of
tests/engine_layouts.py reach is 5.379 (bwd_plan_emul.attn_table_lmax, computed from that table).  The input is util.O.synth_spec(salt 13) x
INPUT_SCALE = 0.02.  The input scale alone cannot bring every attention inside: in the fp64 model the first encoder layer (sqrt(d) x the
token embedding + the position table) stays at 40 .. 48 at any scale and the first time layer (sqrt(d) x a LayerNorm output) at 1200 ..
1600, so bwd_plan_emul.condition scales the fc_q of an attention that is outside to 0.8 of the table's figure.  Resulting largest |score|
per configuration, fp64 model on the CPU (asserted below, and measured again on every attention launch's own device operands):
x3_small 4.82, x3_256 4.43, x3_256_long 4.51, x3_256_dec3 4.30, d128_ff256 4.58, x3_256_kt34 4.54.

What the conditioning leaves out is run by test_backward_plan_attention_links_unconditioned: no condition(), the input at synth_spec's own
scale (first encoder attention at 7,434 / 11,620, first time attention at 390 / 1,280), every attn_bwd launch under the derived bound of
tests/attn_peaked_emul.py instead of the calibrated bands.
"""
import time

import pytest
import torch

import attn_peaked_emul as AP
import bwd_plan_emul as PE
import util
from test_model_gpu import DROPOUT_CASES, OTHER_CONFIGS
from util import O

pytestmark = pytest.mark.gpu

P_DROP, MODEL_SEED, PERTURB_SEED, SPEC_SALT, LABEL_SALT = 0.1, 31, 32, 13, 14

# (configuration, batch).  The last one is the smallest shape that reaches the two attention-backward forms of the paper's backward the
# others do not: 72 notes = three key tiles (the note self attention), 100 frames = four (the time layers); one sequence set, so that both
# token counts stay multiples of the strip kernels' 32
CONFIGS = {k: (DROPOUT_CASES[k][1], 2) for k in ('x3_small', 'x3_256', 'x3_256_long', 'x3_256_dec3')}
CONFIGS['d128_ff256'] = (OTHER_CONFIGS['d128_ff256'], 2)
CONFIGS['x3_256_kt34'] = (O.HfttConfig(n_margin=4, n_frame=100, n_bin=32, n_note=72, cnn_channel=4, cnn_kernel=5, hid_dim=256, pf_dim=512, enc_layer=1,
                                       dec_layer=2, enc_head=4, dec_head=4, n_velocity=16), 1)

# plan entries the link check leaves out, by op name, and why (none: every kind of ws['bwd'] and ws['bwd_dec'] has a contract)
EXEMPT = {}

_CACHE = {}


def _case(name):
    """(state dict with the conditioned fc_q, input, labels, {attention: lmax}, table lmax) of a configuration, shared by its two modes"""
    if name not in _CACHE:
        cfg, B = CONFIGS[name]
        model = util.build_model(cfg, MODEL_SEED, dropout=P_DROP)
        util.perturb(model, PERTURB_SEED)
        sd = util.sd_cpu(model)
        x = O.synth_spec(B, cfg, salt=SPEC_SALT) * PE.INPUT_SCALE
        seed = (1234 * 1000003 + 1) & 0xFFFFFFFFFFFFFFFF            # HfttEngine: base seed 1234, first training step
        lm, factors, table = PE.condition(sd, x, cfg, seed, P_DROP)
        _CACHE[name] = (sd, x, O.synth_labels(B, cfg, salt=LABEL_SALT), lm, factors, table, seed)
    return _CACHE[name]


def _case_raw(name):
    """(state dict, input, labels, seed) of a configuration with NO conditioning: fc_q as initialised, the input at synth_spec's own scale"""
    if ('raw', name) not in _CACHE:
        cfg, B = CONFIGS[name]
        model = util.build_model(cfg, MODEL_SEED, dropout=P_DROP)
        util.perturb(model, PERTURB_SEED)
        _CACHE[('raw', name)] = (util.sd_cpu(model), O.synth_spec(B, cfg, salt=SPEC_SALT), O.synth_labels(B, cfg, salt=LABEL_SALT),
                                 (1234 * 1000003 + 1) & 0xFFFFFFFFFFFFFFFF)
    return _CACHE[('raw', name)]


def _engine(dev, name, precision, sd=None):
    cfg, B = CONFIGS[name]
    sd = _case(name)[0] if sd is None else sd
    model = util.build_model(cfg, MODEL_SEED, dropout=P_DROP)
    model.load_state_dict(sd)
    model = model.to(dev)
    model.hftt_precision = precision
    model.train()
    return model, model.hftt_engine()


def _pairs(plan):
    return {(name, (meta or {}).get('kernel', '')) for _, _, name, meta in plan}


def _step(eng, ws, plan, frozen, tag, lines):
    """the stepped run of one plan on a NaN-filled flat_grads, with every condition that is read off the launches"""
    dev = eng.device
    B = ws['B']
    nan_bits = torch.full((1,), float('nan')).view(torch.int32).item()
    # ---- the ordinary backward of the same forward
    eng.flat_grads.fill_(float('nan'))
    eng.backward(B, frozen_stages=frozen)
    torch.cuda.synchronize()
    g_ref = eng.flat_grads.clone()
    # ---- the stepped one
    eng.flat_grads.fill_(float('nan'))
    eng._patch(ws, ws['p'], ws['seed'])
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch(i, entry, rec, sp, outs):
        eng._run(ws, plan[i:i + 1], stream, outs=ws['outs'], seed=ws['seed'], p=ws['p'])
        torch.cuda.synchronize()
    touched = torch.zeros(eng.flat_grads.numel(), dtype=torch.bool)
    spans, rules = PE.engine_spans(eng, ws), PE.PlanRules(eng, ws)
    producer, failures, by_kind, lmaxes = {}, [], {}, []
    gp = {n: o for n, _, o, _ in eng._bound}
    dd = 'decoder_spec2midi.'
    t0 = time.time()
    with torch.cuda.device(dev):
        for entry in plan:
            assert entry[2] in PE.CONTRACTS or entry[2] in EXEMPT, 'plan entry %s is neither checked nor exempt' % entry[2]
        for i, entry, rec, where, figs in PE.step_plan(eng, ws, plan, launch):
            me = PE.describe(i, entry, where)
            bad = PE.failures(figs)
            if bad:
                failures.append((me, bad))
            wrong = rules.check(i, entry, where)                 # what the descriptor must carry from the graph
            assert not wrong, '%s: %s' % (me, '; '.join(wrong))
            ratio, fig = PE.worst(figs)
            k = by_kind.setdefault(entry[2], [0.0, '', 0])
            k[2] += 1
            if ratio >= k[0]:
                k[0], k[1] = ratio, 'plan[%d] %s %s' % (i, (entry[3] or {}).get('kernel', '-'), fig)
            if entry[2] == 'attn_bwd':
                lmaxes.append(PE.attn_lmax(rec))
            # ---- written exactly once
            acc = PE.accumulates(entry)
            for out, (tname, off, rows, cols, ld) in where.items():
                if tname != 'flat_grads':
                    continue
                idx = (off + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]).reshape(-1)
                if acc:
                    assert bool(touched[idx].all()), '%s: accumulates into elements of flat_grads that no launch has written (%s)' % (me, out)
                else:
                    assert not bool(touched[idx].any()), '%s: overwrites elements of flat_grads an earlier launch wrote (%s)' % (me, out)
                touched[idx] = True
            # ---- which buffer the column sums read
            if entry[2] == 'colsum':
                x_addr, rows, n, ld, out_addr = entry[1][:5]
                src = producer.get(spans.where(x_addr, rows, n, ld)[:2])
                oname, ooff = where['out'][:2]
                if oname == 'flat_grads' and ooff == gp[dd + 'pos_embedding_time.weight']:
                    want = ('time_embed_bwd', 'dym') if ws['p'] > 0 else ('gemm_nt', 'C')
                elif oname == 'flat_grads' and ooff == gp[dd + 'pos_embedding_freq.weight']:
                    want = ('ln_bwd', 'dr')                                   # the residual path: the undropped dr
                else:
                    assert oname == 'g.dq0', me
                    want = ('attn_bwd', 'dq')
                assert src is not None and src[1:] == want, '%s reads what %s wrote; the graph names %s' % (me, src, want)
            for out, w in where.items():
                producer[w[:2]] = (i, entry[2], out)
    wall = time.time() - t0
    torch.cuda.synchronize()
    assert not rules.finish(), (tag, rules.finish())
    for kind, (ratio, at, n) in sorted(by_kind.items()):
        lines.append('BWDPLAN %-26s %-18s worst measured / bound %.3g at %s; %d launches' % (tag, kind, ratio, at, n))
    lines.append('BWDPLAN %-26s %d launches stepped and checked in %.1f s; largest |score| over the attention launches %.2f' % (
        tag, len(plan), wall, max(lmaxes)))
    assert not failures, '\n'.join('%s: %s' % f for f in failures)
    # ---- stepping changes nothing
    g = eng.flat_grads
    assert torch.equal(g.view(torch.int32), g_ref.view(torch.int32)), '%s: the stepped backward and the ordinary one differ' % tag
    # ---- every parameter's element written; below the border of a frozen encoder nothing
    lo = eng.frozen_border(frozen)
    gc = g.cpu()
    assert bool((gc[:lo].view(torch.int32) == nan_bits).all()), '%s: an element below the frozen border was written' % tag
    for name, _, o, n in eng._bound:
        if o >= lo:
            assert bool(touched[o:o + n].all()) and not bool(torch.isnan(gc[o:o + n]).any()), '%s: %s is not written by the plan' % (tag, name)
        else:
            assert not bool(touched[o:o + n].any()), name
    assert max(lmaxes) <= _case(tag.split('/')[0])[5], (tag, lmaxes)
    return by_kind


@pytest.mark.parametrize('precision', ['x3', 'parity'])
@pytest.mark.parametrize('name', list(CONFIGS))
def test_backward_plan_link_by_link(dev, name, precision):
    cfg, B = CONFIGS[name]
    sd, x, labels, lm, factors, table, seed = _case(name)
    print('%s: fp64 model, largest |score| per attention %s (table %.3f); fc_q factors %s' % (
        name, ' '.join('%.2f' % v for v in lm.values()), table, {k: float('%.3g' % v) for k, v in factors.items()}))
    assert max(lm.values()) <= table
    model, eng = _engine(dev, name, precision)
    with torch.cuda.device(eng.device):
        eng.forward(x.to(dev), training=True, save=True)
        eng.loss(B, tuple(t.to(dev).contiguous() for t in labels))
    torch.cuda.synchronize()
    ws = eng._ws[B]
    assert ws['seed'] == seed and ws['p'] == P_DROP and ws['saved']
    lines = []
    for frozen in (0, 1):                        # (frozen_stages = 2 is a prefix of the full plan)
        plan, _ = eng.backward_plan(B, frozen)
        assert plan is ws['bwd' if frozen == 0 else 'bwd_dec']
        _step(eng, ws, plan, frozen, '%s/%s/%s' % (name, precision, 'full' if frozen == 0 else 'frozen_encoder'), lines)
    print('\n'.join(lines))
    # ---- dropout sites: a backward descriptor names only sites of this workspace's forward; no two forward launches share one
    fwd_sites = [PE.sites_of(e, True) for e in ws['fwd']]
    flat = [s for ss in fwd_sites for s in set(ss)]
    assert len(flat) == len(set(flat)), 'two forward launches share a dropout site: %s' % sorted(s for s in set(flat) if flat.count(s) > 1)
    assert set(flat) == set(range(1, eng._site + 1))
    for pname in ('bwd', 'bwd_dec'):
        for i, e in enumerate(ws[pname]):
            for s in PE.sites_of(e, False):
                assert s in set(flat), '%s[%d] %s names dropout site %d, which no forward launch of this workspace has' % (pname, i, e[2], s)


# (configuration, precision) of the unconditioned runs: the smallest configuration in both modes, and d = 256 with 256 keys (planes)
UNCONDITIONED = [('x3_small', 'x3'), ('x3_small', 'parity'), ('x3_256_long', 'x3')]


def attention_links(eng, ws, plan, forward, harness, tag, lines):
    """Steps `plan` one entry at a time and holds every attention launch, on the device's own operands, to the peaked-row criterion of
    tests/attn_peaked_emul.py (the derived element-wise bound AND e_dev <= 3 (e32 + e_x3) + 1e-6); the other links are run and not judged.
    harness: fwd_plan_emul or bwd_plan_emul (launch_io, make_record, engine_spans).  -> [(shape, largest |score|)] in launch order"""
    kind = 'attn_fwd' if forward else 'attn_bwd'
    stream = torch.cuda.current_stream(eng.device).cuda_stream
    sp = harness.engine_spans(eng, ws)
    reached, failures = [], []
    for i, entry in enumerate(plan):
        rec = None
        if entry[2] == kind:
            I, Oo = harness.launch_io(entry, eng, ws)
            rec = harness.make_record(entry, {k: sp.fetch(*v) for k, v in I.items()}, {}, eng, ws)
        eng._run(ws, plan[i:i + 1], stream, outs=ws['outs'], seed=ws['seed'], p=ws['p'])
        if rec is None:
            continue
        torch.cuda.synchronize()
        got = {k: sp.fetch(*v) for k, v in Oo.items()}
        figs, bad, lmax = AP.check_plan_launch(rec, got, forward)
        reached.append((rec['shape'], lmax))
        lines.append('PEAKED-PLAN %-28s plan[%d] %s %-36s %-22s planes %d drop %.2g largest |score| %-9.4g a: %s | b: %s' % (
            tag, i, kind, (entry[3] or {}).get('kernel', '-'), 'x'.join(map(str, rec['shape'])), rec['planes'], rec.get('drop_p', 0.0), lmax,
            ' '.join('%s %.3g' % (f, v[0]) for f, v in figs.items()), ' '.join('%s %.3g' % (f, v[1] / v[2]) for f, v in figs.items() if f != 'mx')))
        failures += ['plan[%d] %s %s: %s' % (i, kind, (entry[3] or {}).get('kernel', '-'), b) for b in bad]
    assert reached and not failures, '%s\n%s' % (tag, '\n'.join(failures))
    return reached


def first_layers_are_outside_the_table(eng, B, reached, forward, tag, lines):
    """the first encoder self attention [B T, H, F, F] and the first time attention [B N, H, T, T] of the plan (the last such launches of a
    backward plan) lie beyond the largest |score| the calibrated attention bands were made on"""
    table = PE.attn_table_lmax()
    enc = [l for s, l in reached if s[2] == s[3] == eng.F and s[0] == B * eng.T]
    tim = [l for s, l in reached if s[2] == s[3] == eng.T and s[0] == B * eng.N]
    assert enc and tim, reached
    first_enc, first_time = (enc[0], tim[0]) if forward else (enc[-1], tim[-1])
    lines.append('PEAKED-PLAN %-28s first encoder attention reaches %.4g, first time attention %.4g (table %.3f)' % (tag, first_enc, first_time, table))
    assert first_enc > table and first_time > table, (tag, first_enc, first_time, table)


@pytest.mark.parametrize('name,precision', UNCONDITIONED)
def test_backward_plan_attention_links_unconditioned(dev, name, precision):
    """bwd_plan_emul.condition NOT applied, the input at synth_spec's own scale: the first encoder and the first time attention run on the
    scores the calibrated bands were conditioned away from.  Every attn_bwd launch of the full plan is held teacher-forced under the derived
    bound of tests/attn_peaked_emul.py -- the plan's own sites and seeds, planes where the plan stores planes.  The other links are not
    judged here: the conditioned runs above hold them."""
    cfg, B = CONFIGS[name]
    sd, x, labels, seed = _case_raw(name)
    model, eng = _engine(dev, name, precision, sd)
    lines = []
    try:
        with torch.cuda.device(eng.device):
            eng.forward(x.to(dev), training=True, save=True)
            eng.loss(B, tuple(t.to(dev).contiguous() for t in labels))
            torch.cuda.synchronize()
            ws = eng._ws[B]
            assert ws['seed'] == seed and ws['p'] == P_DROP and ws['saved']
            plan, _ = eng.backward_plan(B, 0)
            eng._patch(ws, ws['p'], ws['seed'])
            tag = '%s/%s/backward' % (name, precision)
            reached = attention_links(eng, ws, plan, False, PE, tag, lines)
            first_layers_are_outside_the_table(eng, B, reached, False, tag, lines)
    finally:
        print('\n' + '\n'.join(lines))


def test_stepped_plans_reach_every_kernel_of_the_paper_backward(dev):
    """(op, kernel) pairs of the plans stepped above against a paper-width backward with three decoder layers, built and not run"""
    paper = O.HfttConfig(**dict(O.PAPER.as_dict(), dec_layer=3))
    model = util.build_model(paper, 5, dropout=P_DROP).to(dev)
    model.hftt_precision = 'x3'
    model.train()
    eng = model.hftt_engine()
    want = _pairs(eng.backward_plan(1, 0)[0]) | _pairs(eng.backward_plan(1, 1)[0])
    del model, eng
    have = set()
    for name, (cfg, B) in CONFIGS.items():
        m = util.build_model(cfg, 5, dropout=P_DROP).to(dev)
        m.hftt_precision = 'x3'
        m.train()
        e = m.hftt_engine()
        have |= _pairs(e.backward_plan(B, 0)[0]) | _pairs(e.backward_plan(B, 1)[0])
    assert want <= have, 'no stepped configuration reaches %s' % sorted(want - have)
