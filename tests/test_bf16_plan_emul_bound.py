"""CPU calibration of the bf16 plan's link check (tests/bf16_plan_emul.py; the device side is tests/test_bf16_plan_gpu.py).

(a) The float32 run of the model, taken as the device, passes every teacher-forced link at the three configurations the GPU test runs.
(b) Each planted defect fails, and fails FIRST at the link it was planted at (later links are fed the defective buffers and must still hold:
    that is what teacher forcing buys); a defect no criterion can see stays in the list as an expected-invisible case.
(c) The free-running figure is much blinder: which planted defects exceed 3 x the float32 model's own error against fp64 is reported."""
import pytest
import torch

import bf16_plan_emul as PE
import util
from util import O, OUT_NAMES

F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope='module')
def cases():
    """family -> (cfg, B, sd, x): the GPU test's model and input"""
    res = {}
    for fam, (cfg, B) in PE.configs().items():
        assert PE.family_of(cfg) == fam
        model = util.build_model(cfg, PE.MODEL_SEED)
        util.perturb(model, PE.PERTURB_SEED)
        res[fam] = (cfg, B, util.sd_cpu(model), O.synth_spec(B, cfg, salt=PE.SALT))
    return res


def _links(case, fam, defect=None):
    cfg, B, sd, x = case
    dev = PE.run(sd, x, cfg, fam, F32, defect=defect)                # the stand-in for the device, free-running
    m64 = PE.run(sd, x, cfg, fam, F64, forced=dev)                   # the model, every stage fed the stand-in's buffers
    report = []
    return PE.check_all(dev, m64.links, report), report


@pytest.mark.parametrize('fam', PE.FAMILIES)
def test_float32_model_passes_every_link(cases, fam):
    res, report = _links(cases[fam], fam)
    print('\n'.join(report))
    assert PE.first_failure(res) is None, [(n, b) for n, b, _ in res if b]
    names = [n for n, _, _ in res]
    for want in ('win', 'embed_w', 'x0', 'enc0.qkv', 'enc0.ctx', 'enc0.lse', 'enc0.x1', 'enc0.x2', 'dec0.q0', 'dec0.ckv', 'dec0.cctx', 'dec0.clse',
                 'dec0.cx', 'logits_f', 'y0', 'time0.x2', 'logits_t') + tuple(OUT_NAMES):
        assert want in names, want
    # the share of an attention link's bound that the score term makes up: all of it at the first layers (raw log-mel x sqrt(d)), little behind a LayerNorm
    share = {n: st['score_share'] for n, _, st in res if n.endswith('ctx')}
    print({k: round(v, 4) for k, v in share.items()})
    assert share['enc0.ctx'] > 0.9 and share['enc1.ctx'] < 0.5


@pytest.mark.parametrize('fam,defect', [(f, d) for d in PE.DEFECTS for f in PE.DEFECT_FAMILIES.get(d, PE.FAMILIES)])
def test_planted_defect_fails_first_at_its_own_link(cases, fam, defect):
    """(a family that has no such rounding point has no case: bf16_plan_emul.DEFECT_FAMILIES)"""
    res, report = _links(cases[fam], fam, defect)
    first = PE.first_failure(res)
    if defect in PE.DEFECTS_INVISIBLE:
        assert first is None, 'the defect %s has become visible at %s: take it out of DEFECTS_INVISIBLE' % (defect, first)
        return
    line = [r for r in report if r.startswith(PE.DEFECTS[defect] + ' ')]
    print('\n%-9s %-22s %s' % (fam, defect, '\n'.join(line)))
    assert first == PE.DEFECTS[defect], (defect, first, [(n, b) for n, b, _ in res if b])


def test_free_running_bound_is_blinder_than_the_links(cases):
    """the whole-plan figure (each output's rms error against the fp64 free-running model, held to 3 x the float32 model's) against the same
    planted defects: reported, and never sharper than the link check"""
    for fam in PE.FAMILIES:
        cfg, B, sd, x = cases[fam]
        rows = PE.free_yardstick(sd, cfg, fam, B, PE.YARD_SALTS, lambda s: O.synth_spec(B, cfg, salt=s))
        bound = PE.free_bound(rows)
        m64 = PE.run(sd, x, cfg, fam, F64)
        seen_free, seen_links = [], []
        for defect in PE.DEFECTS:
            if fam not in PE.DEFECT_FAMILIES.get(defect, PE.FAMILIES):
                continue
            err = PE.free_errors(PE.run(sd, x, cfg, fam, F32, defect=defect), m64)
            if any(err[n][0] > bound[n][0] or abs(err[n][1]) > bound[n][1] for n in OUT_NAMES):
                seen_free.append(defect)
            if defect not in PE.DEFECTS_INVISIBLE:
                seen_links.append(defect)
        print('%-9s free-running bound sees %d of %d planted defects %s; the links see %d' % (fam, len(seen_free), len(seen_links), seen_free, len(seen_links)))
        assert set(seen_free) <= set(seen_links)
