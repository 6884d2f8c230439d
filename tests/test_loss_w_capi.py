"""C ABI of the fused loss with class-balanced and focal criteria (hftt_loss_w, hftt_loss_w_ws_bytes): the exported symbols, the
descriptor's layout against the C compiler, the ABI version, every host-side refusal with its message (they run before the device guard and
the launch, so a box without a GPU tests them), and the compile-time resources of the new kernels.  No compute calls."""
import ctypes as C
import math
import os
import subprocess

import pytest

import hipcc_remarks
import util

HDR = os.path.join(util.ROOT, 'include', 'hftt_hip.h')


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location('hftt_build', os.path.join(util.ROOT, 'nylon-amt_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def lib():
    _build_module().build(verbose=False)
    from hftt_hip import _capi
    return _capi.lib()


def test_symbols_and_workspace_size(lib):
    from hftt_hip import _capi
    for name in ('hftt_loss_w', 'hftt_loss_w_ws_bytes'):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert 'loss_w.hip' in _build_module().SOURCES
    assert lib.hftt_loss_w_ws_bytes(8 * 128 * 88) == 256 * 2 * 4          # one pair of partials per pre-pass workgroup
    assert lib.hftt_abi_version() == _capi.ABI_VERSION == 8


def test_descriptor_layout_matches_the_c_compiler(lib, tmp_path):
    from hftt_hip import _capi
    cls, cname = _capi.LossWDesc, 'hftt_loss_w_desc'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {',
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname), 'printf("inner %zu\\n", sizeof(hftt_loss_desc));']
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for f in _capi.LossDesc._fields_:
        lines.append('printf("hftt_loss_desc.%s %%zu\\n", offsetof(hftt_loss_desc, %s));' % (f[0], f[0]))
    lines += ['printf("HFTT_ABI_VERSION %d\\n", HFTT_ABI_VERSION);', 'return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n') if l)
    assert int(got[cname]) == C.sizeof(cls)
    assert int(got['inner']) == C.sizeof(_capi.LossDesc) == cls.base.size == 208          # hftt_loss's descriptor, unchanged, comes first
    assert cls.base.offset == 0
    for f in cls._fields_:
        assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]
    for f in _capi.LossDesc._fields_:
        assert int(got['hftt_loss_desc.%s' % f[0]]) == getattr(_capi.LossDesc, f[0]).offset, f[0]
    assert int(got['HFTT_ABI_VERSION']) == 8 == lib.hftt_abi_version()                    # the symbols were added AT version 8


# non-null "device pointers": every case below is refused before anything dereferences them
PTR = [0x100000 + i * 0x10000 for i in range(40)]
N, V, NN = 264, 128, 88


def _desc(**kw):
    from hftt_hip import _capi
    a = dict(n=N, V=V, Nn=NN, prob=PTR[0:6], vel=PTR[6:8], labels=PTR[8:12], loss_out=PTR[12], ws=PTR[13], pos_weight=[None] * 6, gamma=[0.0] * 6,
             class_weight=[None, None], smoothing=[0.0, 0.0], ignore_index=[-100, -100], ws_w=PTR[14])
    a.update(kw)
    d = _capi.LossWDesc()
    b = d.base
    b.n, b.V = a['n'], a['V']
    for i in range(6):
        b.prob[i], b.d_prob[i] = a['prob'][i], PTR[20 + i]
        d.pos_weight[i], d.gamma[i] = a['pos_weight'][i], a['gamma'][i]
    for s in range(2):
        b.vel[s], b.d_vel[s] = a['vel'][s], PTR[30 + s]
        d.class_weight[s], d.smoothing[s], d.ignore_index[s] = a['class_weight'][s], a['smoothing'][s], a['ignore_index'][s]
    b.label_onset, b.label_offset, b.label_mpe, b.label_velocity = a['labels']
    b.weight_A, b.weight_B, b.grad_scale = 1.0, 1.0, 1.0
    b.loss_out, b.ws = a['loss_out'], a['ws']
    d.Nn, d.ws_w = a['Nn'], a['ws_w']
    return d


def _but(seq, i, v):
    seq = list(seq)
    seq[i] = v
    return seq


REJECTS = [
    # the base descriptor's checks, under this entry point's name
    ({'n': 0}, b'bad shape'), ({'V': 0}, b'bad shape'), ({'V': 257, 'n': 264}, b'bad shape'),
    ({'prob': _but(PTR[0:6], 4, None)}, b'null probability tensor 4'), ({'vel': [PTR[6], None]}, b'null operand'),
    ({'labels': _but(PTR[8:12], 3, None)}, b'null operand'), ({'loss_out': None}, b'null operand'), ({'ws': None}, b'null operand'),
    # its own
    ({'Nn': 0}, b'Nn=0 must be positive'), ({'Nn': -88}, b'Nn=-88 must be positive'),
    ({'Nn': 7}, b'n=264 must be a multiple of Nn=7'), ({'n': 265}, b'n=265 must be a multiple of Nn=88'),
    ({'gamma': _but([0.0] * 6, 2, 0.5)}, b'head 2: gamma=0.5 must be 0 or in [1, 4]'), ({'gamma': _but([0.0] * 6, 5, 4.5)}, b'head 5: gamma=4.5 must be 0 or in [1, 4]'),
    ({'gamma': _but([0.0] * 6, 0, -1.0)}, b'head 0: gamma=-1 must be 0 or in [1, 4]'), ({'gamma': _but([2.0] * 6, 3, math.nan)}, b'head 3: gamma=nan must be 0 or in [1, 4]'),
    ({'smoothing': [1.0, 0.0]}, b'side 0: smoothing=1 must be in [0, 1)'), ({'smoothing': [0.0, -0.125]}, b'side 1: smoothing=-0.125 must be in [0, 1)'),
    ({'smoothing': [math.nan, 0.0]}, b'side 0: smoothing=nan must be in [0, 1)'),
    # the pre-pass workspace: needed for class weights, or an ignore_index that a label can take
    ({'ws_w': None, 'class_weight': [PTR[15], None]}, b'the pre-pass workspace ws_w is null'),
    ({'ws_w': None, 'ignore_index': [-100, 0]}, b'the pre-pass workspace ws_w is null'),
    ({'ws_w': None, 'ignore_index': [127, -100]}, b'the pre-pass workspace ws_w is null'),
]


@pytest.mark.parametrize('kw,msg', REJECTS, ids=[m.decode().replace(' ', '_')[:40] + '-%d' % i for i, (_, m) in enumerate(REJECTS)])
def test_loss_w_rejects_before_any_launch(lib, kw, msg):
    d = _desc(**kw)
    assert lib.hftt_loss_w(C.byref(d), None) not in (0, 2, 3)         # (2 / 3: the launch path was reached)
    err = lib.hftt_last_error()
    assert err.startswith(b'loss_w: ') and msg in err, err


def test_null_descriptor_is_refused(lib):
    assert lib.hftt_loss_w(None, None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'loss_w: ') and b'null descriptor' in err


def test_hftt_loss_keeps_its_own_messages(lib):
    d = _desc(n=0).base
    assert lib.hftt_loss(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'loss: ') and b'bad shape' in err


def test_loss_spec_refuses_tables_of_another_shape():
    """LossSpec keeps its tables' shapes: fp32, contiguous, [Nn] resp. [V]"""
    import torch
    from hftt_hip import HfttError
    from hftt_hip.criteria import LossSpec
    with pytest.raises(HfttError, match='tables are contiguous fp32'):
        LossSpec(88, 128, [torch.ones(87)] + [None] * 5, [0.0] * 6, [None, None], [0.0, 0.0], [-100, -100])
    with pytest.raises(HfttError, match=r'smoothing=1 must be in \[0, 1\)'):
        LossSpec(88, 128, [None] * 6, [0.0] * 6, [None, None], [1.0, 0.0], [-100, -100])


def test_the_new_kernels_use_no_scratch():
    """loss_w.hip cross-compiled for gfx950 with the resource remarks: the per-lane head (pointers and gamma picked by lane out of the
    descriptor's arrays) and the per-side class-weight registers must not put an array into scratch memory"""
    res = hipcc_remarks.resources('loss_w.hip')
    print(res)
    # both forms of the main pass are compiled with and without the class-weight registers (the host picks)
    assert set(res) == {'loss_w_pre_kernel', 'loss_w_kernel<true>', 'loss_w_kernel<false>', 'loss_w_v4_kernel<true>', 'loss_w_v4_kernel<false>',
                        'loss_w_reduce_kernel'}, sorted(res)
    for name, v in res.items():
        assert hipcc_remarks.get(v, 'ScratchSize') == 0, (name, v)
        assert hipcc_remarks.get(v, 'Occupancy') >= 4, (name, v)          # a streaming kernel: latency is hidden by waves in flight
