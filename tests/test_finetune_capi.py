"""C ABI of the grouped optimizer step (hftt_adam_step_groups, hftt_grad_norm_groups): the exported symbols, the descriptor's layout against
the C compiler, every host-side refusal with its message (they run before the device guard and the launch, so a box without a GPU tests
them), and the compile-time resources of the two new kernels.  No compute calls."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest
import torch

import util

HDR = os.path.join(util.ROOT, 'include', 'hftt_hip.h')


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('hftt_build', os.path.join(util.ROOT, 'nylon-amt_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from hftt_hip import _capi
    return _capi.lib()


def test_descriptor_layout_matches_the_c_compiler(lib, tmp_path):
    from hftt_hip import _capi
    cls, cname = _capi.AdamGroupsDesc, 'hftt_adam_groups_desc'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {',
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines += ['printf("HFTT_ABI_VERSION %d\\n", HFTT_ABI_VERSION);', 'printf("HFTT_ADAM_MAX_GROUPS %d\\n", HFTT_ADAM_MAX_GROUPS);', 'return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n') if l)
    assert int(got[cname]) == C.sizeof(cls)
    for f in cls._fields_:
        assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]
    assert int(got['HFTT_ADAM_MAX_GROUPS']) == 8 == _capi.ADAM_MAX_GROUPS
    assert cls.lr.size == cls.weight_decay.size == 64 and cls.frozen.size == 32
    assert int(got['HFTT_ABI_VERSION']) == 8 == lib.hftt_abi_version() == _capi.ABI_VERSION          # the symbols were added AT version 8
    for name in ('hftt_adam_step_groups', 'hftt_grad_norm_groups'):
        assert name in _capi.SIGNATURES and hasattr(lib, name)


P = 0x1000          # a non-null, 16-byte aligned "device pointer": every case below is refused before anything dereferences it


def _desc(**kw):
    from hftt_hip import _capi
    a = dict(p=P, g=P, m=P, v=P, n=1024, quad_group=P, n_groups=2, step=1, lr=[1e-3, 1e-4], weight_decay=[0.01, 0.0], frozen=[0, 1], ctl=P)
    a.update(kw)
    d = _capi.AdamGroupsDesc()
    d.p, d.g, d.m, d.v, d.n, d.quad_group, d.n_groups, d.step = a['p'], a['g'], a['m'], a['v'], a['n'], a['quad_group'], a['n_groups'], a['step']
    d.beta1, d.beta2, d.eps, d.grad_scale = 0.9, 0.999, 1e-8, 1.0
    for i, (lr, wd, fr) in enumerate(zip(a['lr'], a['weight_decay'], a['frozen'])):
        d.lr[i], d.weight_decay[i], d.frozen[i] = lr, wd, fr
    d.ctl = a['ctl']
    return d


STEP_REJECTS = [({'p': None}, b'bad arguments'), ({'g': None}, b'bad arguments'), ({'m': None}, b'bad arguments'), ({'v': None}, b'bad arguments'),
                ({'n': 0}, b'bad arguments'), ({'step': 0}, b'bad arguments'),
                ({'p': P + 4}, b'buffers must be 16-byte aligned'), ({'v': P + 8}, b'buffers must be 16-byte aligned'),
                ({'n': 1022}, b'n=1022 must be a multiple of 4'), ({'n': 1025}, b'n=1025 must be a multiple of 4'),
                ({'n_groups': 0}, b'n_groups=0 must be in 1..8'), ({'n_groups': 9}, b'n_groups=9 must be in 1..8'),
                ({'quad_group': None}, b'the group map is null'),
                ({'ctl': P + 8}, b'ctl must be 16-byte aligned'),
                ({'weight_decay': [0.0, -0.01]}, b'group 1: weight_decay must be >= 0'), ({'weight_decay': [math.nan, 0.0]}, b'group 0: weight_decay must be >= 0'),
                ({'lr': [1e-3, 0.5], 'weight_decay': [0.0, 2.0]}, b'group 1: lr * weight_decay must be below 1'),
                ({'lr': [10.0, 1e-3], 'weight_decay': [0.5, 0.0]}, b'group 0: lr * weight_decay must be below 1')]


@pytest.mark.parametrize('kw,msg', STEP_REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in STEP_REJECTS])
def test_adam_step_groups_rejects_before_any_launch(lib, kw, msg):
    d = _desc(**kw)
    assert lib.hftt_adam_step_groups(C.byref(d), None) not in (0, 2, 3)         # (2 / 3: the launch path was reached)
    err = lib.hftt_last_error()
    assert err.startswith(b'adam_step_groups: ') and msg in err, err


def test_null_descriptor_is_refused(lib):
    assert lib.hftt_adam_step_groups(None, None) not in (0, 2, 3)
    assert b'null descriptor' in lib.hftt_last_error()


NORM_OK = dict(g=P, n=1024, quad_group=P, frozen_mask=2, grad_scale=1.0, max_norm=1.0, ws=P, ctl=P)
NORM_REJECTS = [({'g': None}, b'null operand'), ({'ws': None}, b'null operand'), ({'ctl': None}, b'null operand'),
                ({'n': 0}, b'n=0'), ({'n': 1023}, b'n=1023 must be a multiple of 4'), ({'quad_group': None}, b'the group map is null'),
                ({'frozen_mask': 256}, b'frozen_mask names a group beyond 8'),
                ({'g': P + 4}, b'16-byte aligned'), ({'ctl': P + 4}, b'16-byte aligned'),
                ({'grad_scale': math.inf}, b'grad_scale must be finite'), ({'max_norm': math.nan}, b'max_norm must be positive'),
                ({'max_norm': 0.0}, b'max_norm must be positive')]


@pytest.mark.parametrize('kw,msg', NORM_REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in NORM_REJECTS])
def test_grad_norm_groups_rejects_before_any_launch(lib, kw, msg):
    a = dict(NORM_OK, **kw)
    assert lib.hftt_grad_norm_groups(a['g'], a['n'], a['quad_group'], a['frozen_mask'], a['grad_scale'], a['max_norm'], a['ws'], a['ctl'], None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'grad_norm_groups: ') and msg in err, err


def test_python_entry_points_refuse_cpu_tensors(lib):
    from hftt_hip import HfttError, ops
    g, p, m, v = (torch.zeros(16) for _ in range(4))
    qmap = torch.zeros(4, dtype=torch.uint8)
    ctl, ws = torch.zeros(8, dtype=torch.int32), torch.zeros(2048, dtype=torch.float64)
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.grad_norm_groups(g, qmap, 0, ctl, ws)
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.adam_step_groups(p, g, m, v, 1, qmap, lr=[1e-3])


def test_the_new_kernels_use_no_scratch(tmp_path):
    """guard.hip cross-compiled for gfx950 with the resource remarks: the per-group constants are indexed dynamically, which must not put
    a register array into scratch memory"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('hftt_build', os.path.join(util.ROOT, 'nylon-amt_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src = os.path.join(mod.CSRC, 'guard.hip')
    r = subprocess.run([mod._hipcc()] + mod.FLAGS + ['-x', 'hip', '-c', src, '-o', str(tmp_path / 'guard.o'), '--cuda-device-only',
                                                      '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    scratch, name = {}, None
    for line in r.stderr.split('\n'):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
        m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', line)
        if m and name:
            scratch[name] = int(m.group(1))
    new = {k: v for k, v in scratch.items() if 'adam_groups_kernel' in k or 'grad_sqsum_groups_kernel' in k}
    print(scratch)
    assert len(new) == 2, scratch
    assert all(v == 0 for v in new.values()), new
