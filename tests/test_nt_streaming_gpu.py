"""The A-stationary split-precision block GEMM (csrc/gemm_nt.hip gemm_nt_as3_kernel) against the kernel it replaces, and the embedding
backward's fused mask + column sum (hftt_dropout_bwd_colsum) against the two calls it replaces.

hftt_gemm_nt is called directly, once with HFTT_NT_STREAM=0 (gemm_nt_kernel: the dispatch before the form existed) and once with it on, on
the guarded planes of tests/engine_layouts.py: one guard row in front and behind, the gap columns [N, ldc) of C, NaN in the gaps of every
input.  Every output plane must be the same to the bit, the guards and gaps included; the result is also held to fp64 of the fp32 inputs under
the bound of tests/test_x3_gpu.py::test_gemm_nt_plain / _epilogues (TOL), and two launches of the new form must agree to the bit."""
import ctypes as C
import math
import os

import pytest
import torch

import engine_layouts as EL
import util                                   # noqa: F401
from util import keep_mask_t, keep_scale

pytestmark = pytest.mark.gpu

TOL = EL.TOL_X3                               # tests/test_x3_gpu.py TOL
SITE, SEED = 5, 77
BM = 64                                       # rows of one block of the A-stationary form (AS3_BM)

# (N, K, ldc, npass) and the epilogue of the launches the form was built for
CASES = {
    'embed': dict(N=256, K=96, ldc=256, npass=2, bias=1, add_mod=7, drop=0.1, out_scale=16.0),
    'heads': dict(N=131, K=256, ldc=192, npass=2, bias=1),
    'heads_dx': dict(N=256, K=192, ldc=256, npass=4),
    'gpos': dict(N=256, K=256, ldc=256, npass=4, res_mod=88),
    'k32': dict(N=256, K=32, ldc=256, npass=2),
}
MS = [1, 63, 64, 65, 88, 200, 'resident']


def _switch(on):
    os.environ['HFTT_NT_STREAM'] = '1' if on else '0'


@pytest.fixture(autouse=True)
def _restore_switch():
    old = os.environ.get('HFTT_NT_STREAM')
    yield
    if old is None:
        os.environ.pop('HFTT_NT_STREAM', None)
    else:
        os.environ['HFTT_NT_STREAM'] = old


def _build(dev, c, M):
    from hftt_hip import _capi, ops
    N, K, npass = c['N'], c['K'], c['npass']
    g = torch.Generator().manual_seed(M + N + K)
    rnd = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    A, W = rnd(M, K).to(dev), (rnd(N, K) / math.sqrt(K)).to(dev)
    t = dict(A=A, W=W, keep=[])
    d = _capi.GemmNtDesc()
    d.M, d.N, d.K, d.npass = M, N, K, npass
    pa, va = EL.in_plane(dev, A, ld=K + 8)
    d.A, d.lda = va.data_ptr(), K + 8
    t['keep'].append(pa)
    if c.get('bias'):
        t['bias'] = rnd(N).to(dev); d.bias = t['bias'].data_ptr()
    d.act, d.out_scale = 0, c.get('out_scale', 1.0)
    if c.get('add_mod'):
        t['table'] = rnd(c['add_mod'], N).to(dev)
        pt, vt = EL.in_plane(dev, t['table']); t['keep'].append(pt)
        d.add_table, d.add_mod = vt.data_ptr(), c['add_mod']
    if c.get('res_mod'):
        t['res_mod'] = rm = max(1, min(c['res_mod'], M - 1))            # below M wherever M has two rows
        t['res'] = rnd(rm, N).to(dev)
        pr, vr = EL.in_plane(dev, t['res'], ld=N + 8); t['keep'].append(pr)
        d.residual, d.ldr, d.res_mod = vr.data_ptr(), N + 8, rm
    d.drop_p, d.drop_site, d.drop_seed = c.get('drop', 0.0), SITE, SEED
    wp = ops.prepare_weight(W, npass)
    d.W, d.W_lo = wp.data_ptr(), wp[1].data_ptr()
    t['keep'].append(wp)
    return d, t


def _launch(dev, d, c, M):
    from hftt_hip import _capi
    plane, vc = EL.out_plane(dev, M, c['N'], ld=c['ldc'])
    d.C, d.ldc = vc.data_ptr(), c['ldc']
    _capi.check(_capi.lib().hftt_gemm_nt(C.byref(d), EL.stream(dev)), 'gemm_nt')
    torch.cuda.synchronize(dev)
    return plane, vc


def _ref(c, M, t, dev):
    lin = t['A'].double() @ t['W'].double().T
    if 'bias' in t:
        lin = lin + t['bias'].double()
    rows = torch.arange(M, device=dev)
    v = lin * c.get('out_scale', 1.0)
    if 'table' in t:
        v = v + t['table'].double()[rows % c['add_mod']]
    if c.get('drop'):
        v = v * keep_mask_t(SEED, SITE, (M, c['N']), c['drop']).to(dev).double() * keep_scale(c['drop'])
    if 'res' in t:
        v = v + t['res'].double()[rows % t['res_mod']]
    return v


@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('case', sorted(CASES))
def test_streaming_form_equals_the_block_kernel(dev, case, M):
    c = CASES[case]
    if M == 'resident':
        # one workgroup per CU: some workgroups take a second block, and the last block has one row
        M = BM * torch.cuda.get_device_properties(dev).multi_processor_count + BM + 1
    d, t = _build(dev, c, M)
    _switch(False)
    p_off, v_off = _launch(dev, d, c, M)
    _switch(True)
    p_on, v_on = _launch(dev, d, c, M)
    p_on2, _ = _launch(dev, d, c, M)
    for p in (p_off, p_on):
        assert p.guards_intact(), '%s: an element outside [M, N] was overwritten' % case
        assert p.written(), '%s: an element of [M, N] was not written' % case
    assert bool(torch.isfinite(v_on).all()), 'a value from an input gap reached the result'
    assert torch.equal(p_on.buf.view(torch.int32), p_off.buf.view(torch.int32)), 'switch on != switch off'
    assert torch.equal(p_on.buf.view(torch.int32), p_on2.buf.view(torch.int32)), 'two launches differ'
    err = EL.rel_err(v_on, _ref(c, M, t, dev))
    print('%-9s M=%-6d rel_err %.3e (bound %.1e)' % (case, M, err, TOL[c['npass']]))
    assert err < TOL[c['npass']]


# ------------------------------------------------------------------------------------------------ hftt_dropout_bwd_colsum
def _two_calls(L, st, buf, rows, n, ld, p, out, beta, ws, bf):
    from hftt_hip import _capi
    _capi.check(L.hftt_dropout_bwd(buf.data_ptr(), rows * ld, p, SITE, SEED, bf, st), 'dropout_bwd')
    _capi.check(L.hftt_colsum(buf.data_ptr(), rows, n, ld, out.data_ptr(), beta, ws.data_ptr(), bf, st), 'colsum')


@pytest.mark.parametrize('n', [4, 260, 4096])
@pytest.mark.parametrize('rows', [1, 15, 16, 17, 100])
def test_dropout_bwd_colsum_equals_the_two_calls(dev, rows, n):
    from hftt_hip import _capi
    L, st = _capi.lib(), EL.stream(dev)
    g = torch.Generator().manual_seed(rows * 7 + n)
    ws = torch.empty(L.hftt_colsum_ws_bytes(rows, n) // 4 + 16, device=dev)
    for ld in ([n, n + 12] if (rows, n) == (17, 260) else [n]):
        x = torch.randn(rows, ld, generator=g).to(dev)
        out0 = torch.randn(n, generator=g).to(dev)
        for bf in (0, 1):
            for p in (0.0, 0.1):
                for beta in (0.0, 1.0):
                    src = x.to(torch.bfloat16) if bf else x
                    a, b = src.clone(), src.clone()
                    oa, ob = out0.clone(), out0.clone()
                    _two_calls(L, st, a, rows, n, ld, p, oa, beta, ws, bf)
                    _capi.check(L.hftt_dropout_bwd_colsum(b.data_ptr(), rows, n, ld, p, SITE, SEED, ob.data_ptr(), beta, ws.data_ptr(), bf, st), 'dropout_bwd_colsum')
                    torch.cuda.synchronize(dev)
                    what = (rows, n, ld, bf, p, beta)
                    assert torch.equal(b[:, :n], a[:, :n]), ('masked buffer', what)
                    assert torch.equal(b[:, n:], src[:, n:]), ('the columns [n, ld) were touched', what)
                    assert torch.equal(ob.view(torch.int32), oa.view(torch.int32)), ('sums', what)
                    if p > 0 and rows * n >= 1024:
                        assert not torch.equal(b[:, :n], src[:, :n])        # (the mask was applied)
