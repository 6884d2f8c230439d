"""C ABI of the Adam step that carries the averaged weights (hftt_adam_step_ema): the exported symbol, the descriptor's layout against the C
compiler, every host-side refusal with its message (they run before the device guard and the launch, so a box without a GPU tests them),
and the compile-time resources of the new kernel.  No compute calls."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest
import torch

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


def test_descriptor_layout_matches_the_c_compiler(lib, tmp_path):
    from hftt_hip import _capi
    cls, cname = _capi.AdamEmaDesc, 'hftt_adam_ema_desc'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {',
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname), 'printf("inner %zu\\n", sizeof(hftt_adam_groups_desc));']
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines += ['printf("HFTT_ABI_VERSION %d\\n", HFTT_ABI_VERSION);', 'return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n') if l)
    assert int(got[cname]) == C.sizeof(cls)
    assert int(got['inner']) == C.sizeof(_capi.AdamGroupsDesc) == cls.a.size          # the grouped step's descriptor, unchanged, comes first
    for f in cls._fields_:
        assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]
    assert cls.a.offset == 0
    assert int(got['HFTT_ABI_VERSION']) == 8 == lib.hftt_abi_version() == _capi.ABI_VERSION          # the symbol was added AT version 8
    assert 'hftt_adam_step_ema' in _capi.SIGNATURES and hasattr(lib, 'hftt_adam_step_ema')


# non-null, 16-byte aligned "device pointers", 64 KiB apart (n = 1024 elements are 4 KiB): every case below is refused before anything
# dereferences them
P, G, M_, V, MAP, CTL, EMA, EMC = (0x100000 + i * 0x10000 for i in range(8))
N = 1024


def _desc(**kw):
    from hftt_hip import _capi
    a = dict(p=P, g=G, m=M_, v=V, n=N, quad_group=MAP, n_groups=2, step=1, lr=[1e-3, 1e-4], weight_decay=[0.01, 0.0], frozen=[0, 1], ctl=CTL,
             ema=EMA, ema_c=EMC, ema_decay=0.9999)
    a.update(kw)
    d = _capi.AdamEmaDesc()
    g = d.a
    g.p, g.g, g.m, g.v, g.n, g.quad_group, g.n_groups, g.step = a['p'], a['g'], a['m'], a['v'], a['n'], a['quad_group'], a['n_groups'], a['step']
    g.beta1, g.beta2, g.eps, g.grad_scale = 0.9, 0.999, 1e-8, 1.0
    for i, (lr, wd, fr) in enumerate(zip(a['lr'], a['weight_decay'], a['frozen'])):
        g.lr[i], g.weight_decay[i], g.frozen[i] = lr, wd, fr
    g.ctl = a['ctl']
    d.ema, d.ema_c, d.ema_decay = a['ema'], a['ema_c'], a['ema_decay']
    return d


ONE = dict(n_groups=1, lr=[1e-3], weight_decay=[0.0], frozen=[0])          # one unfrozen group: the map may be left out
BYTES = 4 * N

REJECTS = [
    # what hftt_adam_step_groups refuses, under this entry point's name
    ({'p': None}, b'bad arguments'), ({'g': None}, b'bad arguments'), ({'m': None}, b'bad arguments'), ({'v': None}, b'bad arguments'),
    ({'n': 0}, b'bad arguments'), ({'step': 0}, b'bad arguments'),
    ({'p': P + 4}, b'buffers must be 16-byte aligned'), ({'v': V + 8}, b'buffers must be 16-byte aligned'),
    ({'n': 1022}, b'n=1022 must be a multiple of 4'), ({'n': 1025}, b'n=1025 must be a multiple of 4'),
    ({'n_groups': 0}, b'n_groups=0 must be in 1..8'), ({'n_groups': 9}, b'n_groups=9 must be in 1..8'),
    ({'quad_group': None}, b'the group map is null'),                                                       # two groups: the map is needed
    (dict(ONE, quad_group=None, frozen=[1]), b'the group map is null'),                                     # one group, but frozen
    ({'ctl': CTL + 8}, b'ctl must be 16-byte aligned'),
    ({'weight_decay': [0.0, -0.01]}, b'group 1: weight_decay must be >= 0'), ({'weight_decay': [math.nan, 0.0]}, b'group 0: weight_decay must be >= 0'),
    ({'lr': [1e-3, 0.5], 'weight_decay': [0.0, 2.0]}, b'group 1: lr * weight_decay must be below 1'),
    ({'lr': [10.0, 1e-3], 'weight_decay': [0.5, 0.0]}, b'group 0: lr * weight_decay must be below 1'),
    # the average's own
    ({'ema': None}, b'ema or ema_c is null'), ({'ema_c': None}, b'ema or ema_c is null'),
    ({'ema': EMA + 4}, b'ema and ema_c must be 16-byte aligned'), ({'ema_c': EMC + 8}, b'ema and ema_c must be 16-byte aligned'),
    ({'ema': P}, b'must not overlap p, g, m or v'), ({'ema': M_ + BYTES - 16}, b'must not overlap p, g, m or v'),
    ({'ema': V - BYTES + 16}, b'must not overlap p, g, m or v'), ({'ema': G}, b'must not overlap p, g, m or v'),
    ({'ema_c': P + 16}, b'must not overlap p, g, m or v'), ({'ema_c': M_}, b'must not overlap p, g, m or v'),
    ({'ema_c': V + BYTES - 16}, b'must not overlap p, g, m or v'),
    ({'ema_c': EMA + 16}, b'must not overlap each other'),
    ({'ema_decay': math.nan}, b'ema_decay=nan must be in [0, 1)'), ({'ema_decay': -0.1}, b'ema_decay=-0.1 must be in [0, 1)'),
    ({'ema_decay': 1.0}, b'ema_decay=1 must be in [0, 1)'), ({'ema_decay': 1.5}, b'ema_decay=1.5 must be in [0, 1)'),
]


@pytest.mark.parametrize('kw,msg', REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in REJECTS])
def test_adam_step_ema_rejects_before_any_launch(lib, kw, msg):
    d = _desc(**kw)
    assert lib.hftt_adam_step_ema(C.byref(d), None) not in (0, 2, 3)         # (2 / 3: the launch path was reached)
    err = lib.hftt_last_error()
    assert err.startswith(b'adam_step_ema: ') and msg in err, err


def test_null_descriptor_is_refused(lib):
    assert lib.hftt_adam_step_ema(None, None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'adam_step_ema: ') and b'null descriptor' in err


def test_the_grouped_step_keeps_its_own_messages(lib):
    """hftt_adam_step_groups shares the host checks: its messages still carry its name, and a null map is still refused there"""
    d = _desc(**dict(ONE, quad_group=None)).a
    assert lib.hftt_adam_step_groups(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'adam_step_groups: ') and b'the group map is null' in err


def test_python_entry_point_refuses_cpu_tensors(lib):
    from hftt_hip import HfttError, ops
    p, g, m, v, e, c = (torch.zeros(16) for _ in range(6))
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.adam_step_ema(p, g, m, v, e, c, 1, 0.9999, lr=[1e-3])


def test_the_new_kernel_uses_no_scratch(tmp_path):
    """guard.hip cross-compiled for gfx950 with the resource remarks: the per-group constants are indexed dynamically, which must not put
    a register array into scratch memory"""
    mod = _build_module()
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
    new = {k: v for k, v in scratch.items() if 'adam_ema_kernel' in k}
    print(scratch)
    assert len(new) == 1, scratch
    assert all(v == 0 for v in new.values()), new
