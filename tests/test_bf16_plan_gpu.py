"""The bf16 inference plan held to fp64, launch by launch.

tests/test_bf16_ulp_gpu.py holds each bf16 forward kernel at the ulp on synthetic operands; nothing held what the plan does BETWEEN them: which
tensors PlanBuilder declares as bf16, the folded embedding with out_scale = sqrt(d) and the position table, layer zero's query from the block GEMM
and its broadcast bf16 residual, the heads on ldc = NHp, time_embed's bf16 form, the no-save forms.  After an eval forward every intermediate of
the plan is still in the workspace, so each launch is checked TEACHER-FORCED: the fp64 model of that one launch (tests/bf16_plan_emul.py), fed the
device's own input buffers, against the device's output buffer under the criterion that kernel already carries (bf16_emul.py's constants;
fp32 results by the same unit count without the bf16 ulp; the attention links with the derived score term).  A defect shows at the launch that
made it.  tests/test_bf16_plan_emul_bound.py calibrates this on the CPU.

Then the free-running figure: each output against the fp64 free-running model, held to 3 x the float32 model's own error over eight inputs
(computed here from the model; no measured number is written into this file).

Paper-size runs are not repeated here: the three shapes reach the same kernel forms (asserted from the plans' kernel names)."""
import pytest
import torch

import bf16_plan_emul as PE
import util
from util import O, OUT_NAMES

pytestmark = pytest.mark.gpu

# launch outputs the link check leaves out, by buffer-name suffix, and why
EXEMPT = {s: 'saved for the backward only (the block family has no inference plan and runs the training one): no eval launch reads it; the bf16 '
             'backward is out of scope here' for s in ('.r1', '.r2', '.cr', '.m1', '.s1', '.m2', '.s2', '.cm', '.cs')}
_DESC_OUTPUTS = {'gemm_nt': ('C', 'pre_ln_out', 'ln_mean', 'ln_rstd'), 'strip_linear': ('C', 'pre_ln_out', 'ln_mean', 'ln_rstd'),
                 'ffn_fwd': ('y', 'h_out', 'pre_ln_out', 'ln_mean', 'ln_rstd'), 'attn_fwd': ('out', 'lse', 'probs')}


def _launch_outputs(plan, outs):
    """[(plan op, device address)] of everything the launches of `plan` write"""
    res = []
    for fn, args, name, _ in plan:
        if name in _DESC_OUTPUTS:
            assert len(args) == 1, name
            dsc = args[0]._obj
            res += [(name, getattr(dsc, f)) for f in _DESC_OUTPUTS[name] if getattr(dsc, f)]
        elif name == 'im2win':
            res.append((name, args[0]))
        elif name == 'time_embed_fwd':
            res.append((name, args[2]))
        elif name == 'heads_split':
            res += [(name, t.data_ptr()) for t in (outs[5:9] if args[1] else outs[0:4])]
        else:
            raise AssertionError('a launch kind the coverage walk does not know: %s' % name)
    return res


@pytest.mark.parametrize('fam', PE.FAMILIES)
def test_bf16_eval_plan_link_by_link(dev, fam):
    cfg, B = PE.configs()[fam]
    model = util.build_model(cfg, PE.MODEL_SEED)
    util.perturb(model, PE.PERTURB_SEED)
    sd = util.sd_cpu(model)
    x = O.synth_spec(B, cfg, salt=PE.SALT)
    model = model.to(dev).eval()
    model.hftt_precision = 'bf16'
    with torch.no_grad():
        outs = model(x.to(dev))
    torch.cuda.synchronize()
    eng = model.hftt_engine()
    ws = eng._ws[B]
    plan = ws['fwd'] if ws['saved'] else ws['fwd_inf']

    # ---- which kernels ran
    kernels = [(name, (m or {}).get('kernel', '')) for _, _, name, m in plan]
    attn = [k for n, k in kernels if n == 'attn_fwd']
    print(fam, sorted({k for _, k in kernels if k}))
    assert PE.family_of(cfg) == fam and eng.sb
    if fam == 'strip256':
        assert ws['saved'] is False and eng.bfs and not eng.strip_small
        assert attn[:cfg.enc_layer] == ['attn_fwd8_kernel'] * cfg.enc_layer and all(k.startswith('attn_fwd_kernel<') for k in attn[cfg.enc_layer:])
        assert any(k.startswith('strip_linear2_kernel<true') for _, k in kernels) and any(k.startswith('strip_linear2_kernel<false') for _, k in kernels)
        assert any(k.startswith('strip_mlp2_kernel<0') for _, k in kernels)
    elif fam == 'small64':
        assert ws['saved'] is False and eng.bfs and eng.strip_small
        assert any(k.startswith('bs_linear_kernel<') for _, k in kernels) and any(k == 'bs_mlp_kernel<0>' for _, k in kernels)
        assert all(k.startswith('attn_fwd_kernel<') for k in attn)
    else:
        assert ws['saved'] is True and not eng.strip and 'fwd_inf' not in ws
        assert all(k.startswith('gemm_nt') for n, k in kernels if n == 'gemm_nt') and not any(n in ('strip_linear', 'ffn_fwd') for n, _ in kernels)

    # ---- every named buffer, the prepared folded embedding and the outputs, copied
    bufs = {k: t.detach().cpu().clone() for k, t in ws['bufs'].items()}
    for n, t in zip(OUT_NAMES, outs):
        bufs[n] = t.detach().cpu().clone()
    d_pad = (eng.d + 63) // 64 * 64
    o = eng.Woff['embed']
    bufs['embed_w'] = eng.wbf[o:o + d_pad * eng.Kp].view(torch.bfloat16).view(d_pad, eng.Kp).cpu().clone()
    o = eng.Woff['embed_b']
    bufs['embed_b'] = eng.fprep[o:o + eng.d].cpu().clone()
    stream_dtype = torch.bfloat16 if fam != 'block' else torch.float32
    for n in ('x0', 'enc0.x1', 'enc0.x2', 'dec0.cx', 'y0'):
        assert bufs[n].dtype == stream_dtype, (n, bufs[n].dtype)
    for n in ('enc0.qkv', 'enc0.ctx', 'dec0.q0', 'dec0.ckv', 'dec0.cctx'):
        assert bufs[n].dtype == torch.bfloat16, (n, bufs[n].dtype)
    for n in ('enc0.lse', 'logits_f', 'logits_t'):
        assert bufs[n].dtype == torch.float32, (n, bufs[n].dtype)

    # ---- the teacher-forced link check
    m64 = PE.run(sd, x, cfg, fam, torch.float64, forced=bufs)
    report = []
    res = PE.check_all(bufs, m64.links, report)
    print('\n'.join(report))
    bf = [(st['identical'], n) for n, _, st in res if st['kind'] == 'bf']
    print('%s worst link: identical %.5f at %s; worst row %.4f; largest excess %.1f' % (
        fam, min(bf)[0], min(bf)[1], min(st['worst_row'] for _, _, st in res if st['kind'] == 'bf'),
        max(st['excess'] for _, _, st in res if st['kind'] == 'bf')))
    failures = [(n, b) for n, b, _ in res if b]
    assert not failures, failures

    # ---- coverage: every output address of every launch is a buffer the link check covered, or has a written reason
    spans = {k: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for k, t in ws['bufs'].items()}
    spans.update({n: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for n, t in zip(OUT_NAMES, outs)})
    written, unexplained = set(), []
    for op, addr in _launch_outputs(plan, outs):
        hit = [k for k, (lo, hi) in spans.items() if lo <= addr < hi]
        assert len(hit) == 1, (op, hex(addr), hit)
        written.add(hit[0])
        if hit[0] not in m64.links and not any(hit[0].endswith(s) for s in EXEMPT):
            unexplained.append((op, hit[0]))
    assert not unexplained, unexplained
    assert set(m64.links) - {'embed_w', 'embed_b'} <= written, sorted(set(m64.links) - written)     # (the two are written by prepare_weights)

    # ---- the free-running figure
    rows = PE.free_yardstick(sd, cfg, fam, B, PE.YARD_SALTS, lambda s: O.synth_spec(B, cfg, salt=s))
    bound = PE.free_bound(rows)
    err = PE.free_errors(bufs, PE.run(sd, x, cfg, fam, torch.float64))
    print('%s free-running, e = rms(out - m64) / rms(m64) and the mean signed error; yardstick: the float32 model over salts %s' % (fam, list(PE.YARD_SALTS)))
    for n in OUT_NAMES:
        print('  %-11s device e %.3e mean %+.3e   bound e %.3e mean %.3e   e32 per salt %s' % (
            n, err[n][0], err[n][1], bound[n][0], bound[n][1], ' '.join('%.2e' % r[n][0] for _, r in rows)))
    for n in OUT_NAMES:
        assert err[n][0] <= bound[n][0], (n, err[n][0], bound[n][0])
        assert abs(err[n][1]) <= bound[n][1], (n, err[n][1], bound[n][1])
