"""Compile-time resource checks (hipcc cross-compiles without a GPU): the register allocation the launch plans rely on.

Round 5 found the <= 128-key attention backward forms at HALF their intended occupancy for three rounds: nothing bounded their registers, hipcc
spread them over 280-300 (accumulation registers as spill space), and one workgroup per CU ran where the LDS budget was laid out for two.  The
kernels were correct, so no parity test could see it; this one reads the compiler's own resource remarks."""
import re

import pytest

from hipcc_remarks import HIPCC, get as _get, resources as _resources


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_attention_backward_on_planes_registers_and_occupancy():
    res = _resources('x3_attn_pl.hip')
    seen = 0
    for name, v in res.items():
        m = re.match(r'x3_attn_bwd_kernel<(\d+), 64, true, (\d)>', name)
        if not m:
            continue
        seen += 1
        kt = int(m.group(1))
        assert _get(v, 'ScratchSize') == 0, (name, v)
        if kt in (3, 4):        # 96 / 128 keys: 63 / 76 KB of LDS = two workgroups per CU, i.e. two waves per SIMD: at most 256 registers in all
            assert _get(v, 'VGPRs') + _get(v, 'AGPRs') <= 256 and _get(v, 'Occupancy') >= 2, (name, v)
        if kt == 8:             # eight waves = two per SIMD
            assert _get(v, 'VGPRs') + _get(v, 'AGPRs') <= 256, (name, v)
    assert seen == 15           # KT 1, 2, 3, 4, 8 x three dropout forms
    # the forward on planes: its persistent grid is sized by LDS alone (launch_pf: three workgroups per CU at <= 96 keys, two at 128), so the
    # registers must allow that many waves per SIMD without scratch
    fwd = 0
    for name, v in res.items():
        m = re.match(r'x3p_attn_fwd_kernel<(\d+), (\d+), (true|false), (\d)>', name)
        if not m:
            continue
        fwd += 1
        kt, nw = int(m.group(1)), int(m.group(2))
        assert _get(v, 'ScratchSize') == 0, (name, v)
        need = 3 if kt <= 3 else (2 if kt <= 4 or nw == 8 else 1)
        assert _get(v, 'Occupancy') >= need, (name, v)
    assert fwd >= 24


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_x3_strip_registers_and_occupancy():
    """The split-precision strip kernels sit at the edge of the register file (the fused blocks at 256 + ~240 of 512), and their launchers size
    the persistent grids on two workgroups per CU for every output-tile-major form and every half-set (XR == 8) form.  Scratch is allowed only
    where it has been measured and accepted: the one-pass residual forms of the half-set kernel, 24 / 36 bytes per lane (x3_strip.hip, HFTT_XL_XR)."""
    res = _resources('x3_strip.hip')
    assert len(res) == 66
    n_kernels = half_set = fused = 0
    for name, v in res.items():
        scratch, occ = _get(v, 'ScratchSize'), _get(v, 'Occupancy')
        m = re.match(r'x3_linear_kernel<(\d), false, 1, ([23]), true, 8>', name)
        if m:       # (element type, K / 256): the parent values of the four forms that had scratch
            assert scratch <= {('4', '2'): 36, ('4', '3'): 24, ('2', '2'): 24, ('2', '3'): 36}[m.groups()], (name, v)
        else:
            assert scratch == 0, (name, v)
        if name.startswith('x3_linear_n_kernel<'):
            n_kernels += 1
            assert occ >= 2, (name, v)
        if re.match(r'x3_linear_kernel<.*, 8>$', name):
            half_set += 1
            assert occ >= 2, (name, v)
        if name.startswith(('x3_mlp_kernel<', 'x3_oln_mlp_kernel<')):
            fused += 1
            assert scratch == 0 and _get(v, 'VGPRs') + _get(v, 'AGPRs') <= 512, (name, v)
    assert (n_kernels, half_set, fused) == (18, 8, 6)


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_layernorm_backward_registers_and_occupancy():
    """The four LayerNorm backward forms are loaders around shared row helpers (ln_bwd.hip), and registers decide the bandwidth of the wide ones
    (the header comment of ln_bwd256_rows_kernel: R = 4 lost its occupancy to them).  A helper that keeps an array alive across the prefetch
    shows here and nowhere else: no scratch, and registers and occupancy no worse than each symbol had before the helpers."""
    # (VGPRs, Occupancy) of commit 7301703, where each kernel spelled its own arithmetic out (csrc/elementwise.hip)
    parent = {'ln_bwd_kernel<1>': (27, 8), 'ln_bwd_kernel<2>': (50, 8), 'ln_bwd_kernel<4>': (64, 8), 'ln_bwd64_kernel': (52, 8),
              'ln_bwd256_bf16_kernel': (166, 3), 'ln_bwd256_rows_kernel<2, true>': (104, 4)}
    res = {k: v for k, v in _resources('ln_bwd.hip').items() if k.startswith('ln_bwd') and k != 'ln_bwd_reduce_kernel'}
    assert sorted(res) == sorted(parent)
    for name, v in res.items():
        vgprs, occ = parent[name]
        assert _get(v, 'ScratchSize') == 0, (name, v)
        assert _get(v, 'VGPRs') <= vgprs and _get(v, 'Occupancy') >= occ, (name, v, parent[name])
