"""CPU calibration of the attention-dropout read-offs (tests/attn_drop_emul.py) that tests/test_attn_dropout_gpu.py runs on the kernels:
  * on a model kernel that applies the contract's mask, the three decoders return that mask exactly and every value inside its band, at
    every shape, with the store roundings of every mode (bf16, fp16 / bf16 pairs, fp32) and both head widths;
  * every planted defect is reported by a read-off at each of the new shapes where it changes anything;
  * which of the defects the one shape the suite had before (88 x 256, n = 4, H = 4; bands relative to the output's maximum) cannot see."""
import pytest
import torch

import attn_drop_emul as A
import util
from util import rel_err, max_err

N, H = A.N_SEQ, A.HEADS


def _id(s):
    return '%dx%d-%s' % s


def test_model_with_the_true_mask_is_the_fp64_reference():
    """ModelKernel without roundings against autograd through test_x3_gpu._attn_ref (the reference the GPU tests name), shared query included"""
    from test_x3_gpu import _attn_ref
    for Lq, Lk, layout in ((12, 15, 'cross'), (88, 70, 'shared'), (15, 15, 'self')):
        dh, p = 32, A.P_MAIN
        gen = torch.Generator().manual_seed(1)
        q, k, v, dO = A.random_operands(N, H, Lq, Lk, layout, dh, 'parity', gen)
        mask = A.true_mask(N, H, Lq, Lk, p)
        q64, k64, v64 = (t.double().clone().requires_grad_(True) for t in (q, k, v))
        o_ref, p_ref, _ = _attn_ref(q64.expand(N, Lq, H * dh), k64, v64, H, mask.double(), util.keep_scale(p))
        (o_ref * dO.double()).sum().backward()
        ref = A.reference(q, k, v, dO, H, mask, p)
        for name, want in (('out', o_ref), ('map', p_ref), ('dq', q64.grad), ('dk', k64.grad), ('dv', v64.grad)):
            assert rel_err(ref[name], want.detach()) < 1e-12, (layout, name)


@pytest.mark.parametrize('mode,dh', [('parity', 64), ('parity', 32), ('x3', 64), ('x3', 32), ('bf16', 64), ('bf16', 32)])
@pytest.mark.parametrize('shape', A.SHAPES, ids=_id)
def test_true_mask_is_decoded_exactly(shape, mode, dh):
    """store roundings of ks / Lk and of the two dS values do not move a decision or a value out of its band, with and without the map"""
    Lq, Lk, layout = shape
    for p in (A.P_MAIN, A.P_ALT):
        kern = A.ModelKernel(A.no_defect(N, H, Lq, Lk, p), p, H, mode)
        for want_probs in (False, True):
            res = A.read_offs(kern, N, H, Lq, Lk, layout, dh, p, want_probs)
            assert A.failures(res, A.true_mask(N, H, Lq, Lk, p), Lk, p, mode) == []
            if p != A.P_MAIN:
                break


def test_the_bands_are_tighter_than_a_scale_error():
    """a keep scale that is missing or applied twice is 10 % (p = 0.1) off: far outside the widest band, the bf16 ones"""
    for p in (A.P_MAIN, A.P_ALT):
        ks = util.keep_scale(p)
        for Lk in (15, 34, 70, 97, 129, 250, 255):
            assert A.kept_tol('bf16', Lk, p) < 2.0 ** -7 < 0.1 * min(ks - 1.0, 1.0 - 1.0 / ks)
        assert A.ds_tol('bf16') < 0.25 * (1.0 - 1.0 / ks)              # (a dS select without the scale decodes a kept element as 1 / ks)


def _changes(applied, truth):
    return applied['map_dropped'] or not applied['ds_scaled'] or any(not torch.equal(applied[x], truth) for x in ('fwd', 'dv', 'ds'))


@pytest.mark.parametrize('defect', sorted(A.DEFECTS))
def test_planted_defect_is_reported(defect):
    """at every new shape where the defect changes a decision, a scale or the map, a read-off says so; and it does at one shape at least"""
    p, dh, mode = A.P_MAIN, 64, 'x3'
    reported = 0
    for Lq, Lk, layout in A.SHAPES:
        truth = A.true_mask(N, H, Lq, Lk, p)
        applied = A.DEFECTS[defect](N, H, Lq, Lk, p)
        if not _changes(applied, truth):
            continue
        res = A.read_offs(A.ModelKernel(applied, p, H, mode), N, H, Lq, Lk, layout, dh, p, want_probs=True)
        bad = A.failures(res, truth, Lk, p, mode)
        print('%-36s %3d x %3d %-6s %s' % (defect, Lq, Lk, layout, '; '.join(bad)))
        assert bad, (defect, Lq, Lk, layout)
        reported += 1
    assert reported > 0


# what test_attention_shared_query_and_dropout (88 x 256, n = 4, H = 4, shared query; x3 bands 1e-4 / 3e-4 / 2e-5) holds of each defect
HIDDEN_AT_88X256 = {'quads_from_row_start', 'bwd_padded_row_stride'}


def test_what_the_88x256_case_can_and_cannot_see():
    """Two of the defects change nothing at 88 x 256 (Lk % 4 == 0, Lk == 32 KT): no test of that shape can see them, which is how they could
    hide.  The other six change decisions there, and the band comparison does see those."""
    n, Hh, Lq, Lk = A.OLD_CASE
    p, dh = A.P_MAIN, 64
    gen = torch.Generator().manual_seed(3)
    q, k, v, dO = A.random_operands(n, Hh, Lq, Lk, 'shared', dh, 'parity', gen)
    truth = A.true_mask(n, Hh, Lq, Lk, p)
    ref = A.reference(q, k, v, dO, Hh, truth, p)
    band = A.BANDS['x3']
    hidden = set()
    for name, f in sorted(A.DEFECTS.items()):
        applied = f(n, Hh, Lq, Lk, p)
        mk = A.ModelKernel(applied, p, Hh)
        out, st, pm = mk.fwd(q, k, v, True)
        dq, dk, dv = mk.bwd(st, dO)
        errs = dict(out=rel_err(out, ref['out']) / band['out'], map=max_err(pm, ref['map']) / band['map'],
                    dq=rel_err(dq.sum(0, keepdim=True), ref['dq']) / band['grad'], dk=rel_err(dk, ref['dk']) / band['grad'],
                    dv=rel_err(dv, ref['dv']) / band['grad'])
        seen = max(errs.values()) >= 1.0
        print('%-36s changes anything: %-5s  worst error / band: %s' % (name, _changes(applied, truth), ' '.join('%s %.3g' % kv for kv in errs.items())))
        assert seen == _changes(applied, truth), name            # (what differs at all is far outside the bands: nothing hides BETWEEN them here)
        if not seen:
            hidden.add(name)
    assert hidden == HIDDEN_AT_88X256
