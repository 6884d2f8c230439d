"""One host launch path (csrc/hftt_launch.h): every kernel launch goes guard -> LDS attribute -> launch -> launch check through hftt_launch, and
the per-process device state (first device, CU count, per-kernel LDS attribute and resident-workgroup count) lives in hftt_launch.h and
capi.cpp alone.  The structure test keeps the next launcher from copying the plumbing again; the two-device GPU test holds the guard IN FRONT of the launch."""
import os
import re
import subprocess
import sys

import pytest

import util

CSRC = os.path.join(util.ROOT, 'nylon-amt_amd', 'csrc')


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(('.hip', '.h', '.cpp'))}


def test_launch_plumbing_lives_in_one_place():
    src = _sources()
    assert 'hftt_launch.h' in src and len(src) >= 20
    only_in = {'hipLaunchKernelGGL': {'hftt_launch.h'}, 'hipFuncSetAttribute': {'hftt_launch.h'},
               'hipOccupancyMaxActiveBlocksPerMultiprocessor': {'hftt_launch.h'}, 'hipGetDeviceProperties': {'capi.cpp'}}
    for call, allowed in only_in.items():
        users = {f for f, s in src.items() if call in s}
        assert users == allowed, (call, sorted(users))
    # no launch that bypasses the path in another spelling either
    assert not [f for f, s in src.items() if re.search(r'<<<|hipLaunchKernel\b|hipModuleLaunchKernel|hipExtLaunchKernel', s)]
    # the hand-kept copies this path replaced, and the per-launcher caches that went with them
    removed = re.compile(r'\b(n_cus|bs_cus|pl_n_cus|set_lds|bs_set_lds|HFTT_CHECK_LAUNCH)\b|static\s+\w+\s+(attr\w*|resident|n_cu)\b')
    for f, s in src.items():
        if f != 'hftt_launch.h':
            assert removed.search(s) is None, (f, removed.search(s).group(0))
    # every translation unit of the library that holds a kernel launches through the header
    for f, s in src.items():
        if '__global__' in s and f.endswith('.hip'):
            assert '#include "hftt_launch.h"' in s and 'hftt_launch<' in s, f
    # ... and the path itself checks the device before it touches the kernel
    body = src['hftt_launch.h']
    body = body[body.index('int hftt_launch('):]
    order = [body.index(k) for k in ('hftt_device_guard(', 'hftt_lds_attr<', 'hipLaunchKernelGGL(', 'hipGetLastError(')]
    assert order == sorted(order)


def test_strip_helpers_and_the_small_width_family_are_written_once():
    '''The strip kernels' device helpers (the dropout mask generator above all: forward and backward regenerate the same mask from it) have one
    definition each, and the small-width kernels one body (small_strip.h) that the two streams instantiate under their own symbol names.'''
    src = _sources()
    defs = {'drop16': r'\bvoid drop16\(', 'drop8': r'\bvoid drop8\(', 'pack2': r'\bunsigned pack2\(', 'lds16f': r'\bvoid lds16f\(',
            'wait_lgkm0': r'\bvoid wait_lgkm0\(', 'SLOT_BYTES': r'\bconstexpr int SLOT_BYTES\b'}
    for name, pat in defs.items():
        where = [f for f, s in src.items() for _ in re.findall(pat, s)]
        assert len(where) == 1, (name, where)
    for kernel in ('bs_linear_kernel', 'x3s_linear_kernel'):
        where = [f for f, s in src.items() for _ in re.findall(r'__global__ .*\bvoid %s\(' % kernel, s)]
        assert len(where) == 1, (kernel, where)
    small = [src[f] for f in ('small_strip.h', 'bs_strip.hip', 'x3_strip.hip')]
    assert 'x3s_strip.h' not in src
    # the block loop of the family (x3_strip.hip's d = 256 kernels launder their own hb: they are not this family's)
    marker = 'asm volatile("" : "+v"(hb))'
    assert src['small_strip.h'].count(marker) == 1 and src['bs_strip.hip'].count(marker) == 0
    tail = src['x3_strip.hip'][src['x3_strip.hip'].index('struct X3Stream'):]
    assert tail.count(marker) == 0 and all('#include "small_strip.h"' in s for s in small[1:])


def _code(text):
    return re.sub(r'//[^\n]*', '', text)


def _body(text, start):
    """the definition that `start` opens, up to the closing brace in column 0"""
    text = text[text.index(start):]
    return text[:text.index('\n}\n')]


def test_the_guard_test_op_is_a_single_launch_that_writes_its_sentinel():
    '''test_second_device_is_refused_before_anything_is_enqueued tells guard-before-launch from guard-after-launch only if the FIRST launch of
    the refused call writes the tensor that carries the sentinel: hftt_adam_step is one launch, and adam_kernel updates p, m, v in place -- in
    its quad loop and in its tail, through the one update (adam_update) that assigns all three.'''
    s = _sources()['guard.hip']
    body = _body(s, 'extern "C" int hftt_adam_step(')
    assert body.count('hftt_launch<') == 1 and 'hftt_launch<adam_kernel>' in body
    quad, tail = _body(s, 'void adam_kernel(').split('const long tail', 1)
    update = _body(s, 'void adam_update(')
    for x in 'pmv':
        assert re.search(r'float& %s\b' % x, update) and re.search(r'^\s*%s = ' % x, update, re.M), x        # the update writes its p, m, v ...
        # ... and both loops hand it theirs and store them back
        assert re.search(r'adam_update<true>\(pe\[e\], ge\[e\], me\[e\], ve\[e\],', quad) and re.search(r'reinterpret_cast<float4\*>\(%s\)\[i\] = %s;' % (x, x * 2), quad), x
        assert re.search(r'adam_update<false>\(pi, g\[i\], mi, vi,', tail) and re.search(r'\b%s\[i\] = %si;' % (x, x), tail), x


def test_layernorm_backward_and_adam_are_written_once():
    '''The LayerNorm backward output expression and the Adam denominator have one definition each across csrc/ (the four LayerNorm forms are
    loaders around ln_row_terms / ln_row_out, the three Adam kernels call adam_update), and no kernel of ln_bwd.hip spells the row arithmetic
    out again.'''
    src = {f: _code(t) for f, t in _sources().items()}
    assert 'elementwise.hip' not in src
    defs = {'LayerNorm output': r'=\s*(?:rstd|rs) \* (?:\(|__builtin_fmaf\()', 'Adam denominator': r'sqrtf\(\w+(?:\[\w+\])?\)[^;\n]*\beps\b'}
    for (name, pat), home in zip(defs.items(), ('ln_bwd.hip', 'guard.hip')):
        where = [f for f, t in src.items() for _ in re.findall(pat, t)]
        assert where == [home], (name, where)
    ln = src['ln_bwd.hip']
    kernels = ln.split('__global__')[1:]
    assert len(kernels) == 5          # four forms and the reduce
    for k in kernels:
        k = k[:k.index('\n}\n')]
        assert not re.search(r'\b(rstd|rs) \* |fmaf', k), k[:80]
        if 'ln_bwd_reduce_kernel' not in k:
            assert all(h in k for h in ('ln_row_terms<', 'ln_row_out<', 'ln_flush<')), k[:80]


_CHILD = r'''
import sys
sys.path[:0] = %r
import torch
from hftt_hip import HfttError, ops


def tensors(device):
    return [torch.full((1024,), f, device=device) for f in (-7.0, 1.0, 0.5, 0.25)]           # p, g, m, v


second = int(sys.argv[1])
p, g, m, v = tensors('cuda:0')
ops.adam_step(p, g, m, v, 1, lr=1.0)
torch.cuda.synchronize(0)
assert (p.cpu() != -7.0).all() and (m.cpu() != 0.5).all() and (v.cpu() != 0.25).all(), 'adam_step does not write p, m, v'
print('adam_step: one launch that writes p, m, v')
if second == 0:
    sys.exit(0)
with torch.cuda.device(second):
    p, g, m, v = tensors('cuda:%%d' %% second)
    torch.cuda.synchronize(second)
    try:
        ops.adam_step(p, g, m, v, 1, lr=1.0)
    except HfttError as e:
        assert 'rc=3' in str(e) and 'one process drives one device' in str(e), str(e)
    else:
        raise AssertionError('the launch from a second device was not refused')
    torch.cuda.synchronize(second)
    for t, f in ((p, -7.0), (m, 0.5), (v, 0.25)):
        assert torch.equal(t.cpu(), torch.full((1024,), f)), 'refused with status 3, but the kernel ran'
print('second-device launch refused before anything was enqueued')
'''


def _child(second):
    paths = [util.ROOT, os.path.join(util.ROOT, 'nylon-amt_amd')]
    r = subprocess.run([sys.executable, '-c', _CHILD % (paths,), str(second)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.gpu
def test_sentinel_op_overwrites_its_operands_on_the_first_device(dev):
    '''The half of the guard test that one device can run: in a fresh process, adam_step on device 0 overwrites every element of p, m and v
    (so an intact sentinel on the second device means that nothing ran there).'''
    assert 'adam_step: one launch that writes p, m, v' in _child(0)


@pytest.mark.gpu
def test_second_device_is_refused_before_anything_is_enqueued(dev):
    '''A fresh process (the guard's state is per process): adam_step on device 0, then the same call on device 1 with p, m, v pre-filled --
    status 3 and all three intact.  adam_step is ONE launch that updates them in place (the CPU test above), so with the guard behind the
    launch the kernel would have been enqueued and have overwritten them by the time status 3 came back.'''
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two visible devices')
    assert 'refused before anything was enqueued' in _child(1)
