"""The x3 and parity attention kernels on peaked softmax rows, against fp64 under the derived bound of tests/attn_peaked_emul.py.

Rows with two to four live keys an O(1) gap apart on scores of 5 .. 1e5 (the first encoder layer: 40 .. 48, the first time layer:
1,200 .. 1,600, raw log-mel: 1e5 -- DESIGN.md sections 2, 3), in two families (near-duplicate keys, solved ties on distinct keys), through
ops.attn_fwd / ops.attn_bwd in every form the engine launches: fp32 operands and f16-pair planes (npass 2), parity (npass 3), per-sequence
and shared query (q_seq_stride 0), with and without dropout 0.1 on the device generator, with and without the attention map.  The backward
runs teacher-forced on the device's own out and row statistics, its gradients inside a NaN arena.

Criterion: attn_peaked_emul.check -- (a) every element of out, map, row maximum, 1/sum, dq, dk, dv inside the derived bound, (b) per tensor
e_dev <= 3 (e32 + e_x3) + 1e-6.  The input conditions of the CPU test are asserted again here, from the same fp64 reference.  One line per
launch form is printed: the worst measured / bound per figure (profiles/attn_peaked_mi355x.txt keeps the table)."""
import pytest
import torch

import attn_peaked_emul as A

GUARD = 4096
GEOM_IDS = ['-'.join(map(str, g)) for g in A.GEOMS]
SHARED_GEOM = (2, 4, 88, 256, 64)
SITE, SEED = 7, 99


def _ops():
    from hftt_hip import ops
    return ops


def _kernels(geom, mode, planes, want_map, drop):
    """(forward, backward) kernel instantiation of a case by the launchers' dispatch, as plan.attn_meta mirrors it (the names the engine
    writes into its plans, held against kernel traces by tests/test_kernel_names_gpu.py)"""
    from hftt_hip import plan
    n, H, Lq, Lk, dh = geom
    dm = 0 if not drop > 0 else (1 if Lk % 4 == 0 else 2)
    npass = 2 if mode == 'x3' else 3
    return (plan.attn_meta(npass, False, n, H, Lq, Lk, H * dh, 0, planes, want_map, dm)['kernel'],
            plan.attn_meta(npass, True, n, H, Lq, Lk, H * dh, 0, planes, False, dm)['kernel'])


def _forms(geom):
    return [('x3', False), ('parity', False)] + ([('x3', True)] if geom[4] == 64 else [])


def _drop_of(gi, vi):
    return 0.1 if (gi + vi) % 2 else 0.0


def _settings(geom):
    gi = A.GEOMS.index(geom)
    return [(v_form, _drop_of(gi, vi), shared) for vi, v_form in enumerate(A.V_FORMS) for shared in ((False, True) if geom == SHARED_GEOM else (False,))]


def test_the_cases_reach_every_kernel_form():
    """by the launchers' dispatch: the forward on fp32 operands, the forward on planes, and the backward template forms of 96 and 128 keys
    (x3_attn_bwd_kernel<3, ...> / <4, ...>: DESIGN.md section 2, 100 frames x 72 notes), each with and without dropout; the 256-key and the
    dh = 32 forms as well"""
    fwd, bwd = set(), set()
    for geom in A.GEOMS:
        for v_form, drop, shared in _settings(geom):
            for mode, planes in _forms(geom):
                for want_map in (True, False):
                    f, b = _kernels(geom, mode, planes, want_map, drop)
                    fwd.add(f); bwd.add(b)
    for want in ('x3_attn_fwd_kernel<4, 64, 4, true>', 'x3_attn_fwd_kernel<4, 64, 4, false>', 'x3_attn_fwd_kernel<8, 64, 8, true>', 'x3_attn_fwd_kernel<2, 32, 4, false>',
                 'x3p_attn_fwd_kernel<4, 4, true, 0>', 'x3p_attn_fwd_kernel<4, 4, false, 1>', 'x3p_attn_fwd_kernel<3, 4, true, 2>', 'x3p_attn_fwd_kernel<8, 8, false, 0>',
                 'x3p_attn_fwd_kernel<8, 4, true, 1>', 'attn_fwd_kernel<4, 64, 3, false>'):
        assert want in fwd, (want, sorted(fwd))
    for want in ('x3_attn_bwd_kernel<3, 64, false, 0>', 'x3_attn_bwd_kernel<3, 64, false, 2>', 'x3_attn_bwd_kernel<3, 64, true, 0>', 'x3_attn_bwd_kernel<3, 64, true, 2>',
                 'x3_attn_bwd_kernel<4, 64, false, 0>', 'x3_attn_bwd_kernel<4, 64, false, 1>', 'x3_attn_bwd_kernel<4, 64, true, 0>', 'x3_attn_bwd_kernel<4, 64, true, 1>',
                 'x3_attn_bwd_kernel<8, 64, true, 0>', 'x3_attn_bwd_kernel<8, 64, true, 1>', 'x3_attn_bwd_kernel<2, 32, false, 0>', 'x3_attn_bwd_kernel<2, 32, false, 1>',
                 'attn_bwd_kernel<3, 64, 3, false>', 'attn_bwd_kernel<4, 64, 3, false>'):
        assert want in bwd, (want, sorted(bwd))


def _arena(dev, shape):
    numel = 1
    for s in shape:
        numel *= s
    flat = torch.full((numel + 2 * GUARD,), float('nan'), device=dev)
    return flat, flat[GUARD:GUARD + numel].view(shape)


def _guards_intact(flat):
    return bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())


def _launch(ops, dev, case, geom, mode, planes, drop):
    """-> {figure: device tensor} of one kernel form: the forward with the map, the forward without it (its out and row statistics under
    'out_nomap', 'mx_nomap', 'inv_nomap'), the backward on the first forward's out and statistics"""
    n, H, Lq, Lk, dh = geom
    d = H * dh
    shared = case.q.shape[0] == 1
    qd, kd, vd = case.q.to(dev).contiguous(), case.k.to(dev).contiguous(), case.v.to(dev).contiguous()
    if planes:
        qd, kd, vd = ops.to_planes(qd), ops.to_planes(kd), ops.to_planes(vd)
    if shared:
        qd = qd.expand(n, Lq, d)                                          # sequence stride 0
    kw = dict(npass=2 if mode == 'x3' else 3, drop_p=drop, drop_site=SITE, drop_seed=SEED)
    if planes:
        kw['planes'] = True
    out, lse, probs = ops.attn_fwd(qd, kd, vd, H, want_probs=True, **kw)
    out2, lse2 = ops.attn_fwd(qd, kd, vd, H, want_probs=False, **kw)
    arenas = [_arena(dev, (n, L, d)) for L in (Lq, Lk, Lk)]
    ops.attn_bwd(qd, kd, vd, out, lse, case.do.to(dev), H, grads_out=tuple(a[1] for a in arenas), **kw)
    torch.cuda.synchronize()
    assert all(_guards_intact(a[0]) for a in arenas), 'the arena around a gradient output was written'
    got = dict(out=out, map=probs, mx=lse[..., 0], inv=lse[..., 1], dq=arenas[0][1], dk=arenas[1][1], dv=arenas[2][1])
    nomap = dict(out=out2, mx=lse2[..., 0], inv=lse2[..., 1])
    return got, nomap


@pytest.mark.gpu
@pytest.mark.parametrize('geom', A.GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize('L', A.MAGS)
@pytest.mark.parametrize('family', A.FAMILIES)
def test_peaked_rows_forward_and_backward(dev, family, L, geom):
    ops = _ops()
    failures = []
    for v_form, drop, shared in _settings(geom):
        q, k, v, do = A.make(family, geom, L, v_form, shared)
        mag = A.magnitude(q, k, geom[1])
        tag = '%s L %g %s %s drop %g%s' % (family, L, '-'.join(map(str, geom)), v_form, drop, ' shared' if shared else '')
        assert 0.5 * L <= mag <= 5.0 * L, (tag, mag)
        mask, ks = A.dropout_mask(geom, drop, SITE, SEED) if drop > 0 else (None, 1.0)
        case = A.Case(q, k, v, do, geom[1], mask, ks)
        (case if drop == 0.0 else A.Case(q, k, v, do, geom[1])).assert_conditions(tag)          # the conditions are those of the undropped rows
        for mode, planes in _forms(geom):
            got, nomap = _launch(ops, dev, case, geom, mode, planes, drop)
            figs, bad = A.check(case, got, mode, planes)
            figs2, bad2 = A.check(case, nomap, mode, planes)
            form = '%s%s' % (mode, ' planes' if planes else '')
            kern = _kernels(geom, mode, planes, True, drop)
            print('PEAKED-GPU %-62s reached %-9.4g %-9s %-36s %-36s a: %s | no map: %s | b: %s' % (
                tag, mag, form, kern[0], kern[1], ' '.join('%s %.3g' % (f, figs[f][0]) for f in figs), ' '.join('%s %.3g' % (f, figs2[f][0]) for f in figs2),
                ' '.join('%s %.3g' % (f, figs[f][1] / figs[f][2]) for f in figs if f != 'mx')))
            failures += ['%s [%s]: %s' % (tag, form, b) for b in bad] + ['%s [%s, no map]: %s' % (tag, form, b) for b in bad2]
    assert not failures, '\n'.join(failures)
