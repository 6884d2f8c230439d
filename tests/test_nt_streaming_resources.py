"""The A-stationary split-precision block GEMM (csrc/gemm_nt.hip gemm_nt_as3_kernel) as the compiler built it, and the plan meta's name for it.

The kernel's comment lays it out for ONE workgroup of eight waves per CU -- two waves per SIMD, up to 256 VGPRs each -- and promises no
scratch: a spill would put a memory round trip into a loop whose whole purpose is to keep HBM busy."""
import os

import pytest

import hipcc_remarks
import util                                   # noqa: F401  (puts the package on sys.path)


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


def test_streaming_form_registers_and_occupancy():
    res = {k: v for k, v in hipcc_remarks.resources('gemm_nt.hip').items() if k.startswith('gemm_nt_as3_kernel<')}
    # fp16 / bf16 halves x K <= 128 / K <= 256 x weight tiles one / two k steps ahead
    assert sorted(res) == sorted('gemm_nt_as3_kernel<%d, %d, %s>' % (xe, nch, pf2) for xe in (2, 4) for nch in (4, 8) for pf2 in ('false', 'true'))
    for name, v in res.items():
        assert hipcc_remarks.get(v, 'ScratchSize') == 0, (name, v)
        assert hipcc_remarks.get(v, 'Occupancy') == 2, (name, v)
        assert hipcc_remarks.get(v, 'VGPRs') + hipcc_remarks.get(v, 'AGPRs') <= 256, (name, v)


def test_plan_meta_follows_the_switch():
    """nt_meta names the kernel hftt_gemm_nt resolves to (tests/test_kernel_names_gpu.py holds the names against a trace)"""
    from hftt_hip.plan import nt_meta
    shapes = [(2, 262144, 256, 96, dict(add_table=1, drop_site=3), '2, 4, false'), (2, 90112, 131, 256, {}, '2, 8, true'), (4, 90112, 256, 192, {}, '4, 8, true'),
              (2, 88, 256, 256, {}, '2, 8, true'), (4, 88, 256, 256, dict(residual=1), '4, 8, true')]
    for on in (True, False):
        _switch(on)
        for npass, M, N, K, epi, targs in shapes:
            kw = dict(add_table=0, gate=0, drop_site=0, residual=0)
            kw.update(epi)
            name = nt_meta(npass, False, M, N, K, False, False, False, False, ln=False, **kw)['kernel']
            assert name == ('gemm_nt_as3_kernel<%s>' % targs if on else 'gemm_nt_kernel<%d, %d, false>' % (64 if N == 131 else 256, npass))
    _switch(True)
    # what stays on the block kernel: the d = 64 plans, K > 256, fused LayerNorm, the gradient-rounding option
    assert nt_meta(2, False, 300, 64, 64, False, False, False, False, 0, 0, 0, 0, False)['kernel'] == 'gemm_nt_kernel<64, 2, false>'
    assert nt_meta(4, False, 300, 256, 512, False, False, False, False, 0, 0, 0, 0, False)['kernel'] == 'gemm_nt_kernel<256, 4, false>'
    assert nt_meta(2, False, 300, 256, 256, False, False, False, False, 0, 0, 0, 1, True)['kernel'] == 'gemm_nt_kernel<256, 2, true>'
    assert nt_meta(4, True, 300, 256, 192, False, False, False, False, 0, 0, 0, 0, False)['kernel'] == 'gemm_nt_kernel<256, 5, false>'
