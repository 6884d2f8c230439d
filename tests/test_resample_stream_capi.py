"""C ABI of the streaming resampler (hftt_resample_stream): the symbol at ABI 8, the descriptor layout against the C compiler, every host-side
rejection with its text (they run before the device guard and the launch, so a box without a GPU tests them), the loud failure of the Python
entry points without a device, the one copy of the FIR in csrc/, and the kernel's compile remarks.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

import hipcc_remarks
import util

HDR = os.path.join(util.ROOT, 'include', 'hftt_hip.h')
CSRC = os.path.join(util.ROOT, 'nylon-amt_amd', 'csrc')


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


def test_symbol_is_exported_and_bound_at_abi_8(lib):
    from hftt_hip import _capi
    src = open(HDR).read()
    assert re.search(r'\bhftt_resample_stream\s*\(', src)
    assert 'hftt_resample_stream' in _capi.SIGNATURES and hasattr(lib, 'hftt_resample_stream')
    assert lib.hftt_abi_version() == _capi.ABI_VERSION == 8
    assert int(re.search(r'#define HFTT_ABI_VERSION (\d+)', src).group(1)) == 8
    assert int(re.search(r'#define HFTT_RESAMPLE_STREAM_ROWS (\d+)', src).group(1)) == _capi.RESAMPLE_STREAM_ROWS
    mod = _build_module()
    assert 'resample_stream.hip' in mod.SOURCES and any(h.endswith('resample_fir.h') for h in mod.HEADERS)


def test_descriptor_layout_matches_the_c_compiler(lib, tmp_path):
    from hftt_hip import _capi
    cname, cls = 'hftt_resample_stream_desc', _capi.ResampleStreamDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {', 'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (f[0], cname, f[0]))
    lines += ['return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n') if l)
    assert int(got[cname]) == C.sizeof(cls)
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]


P = 0x1000          # a non-null "device pointer": every case below is refused before anything dereferences it


def _desc(**kw):
    from hftt_hip import _capi
    d = _capi.ResampleStreamDesc()
    d.wave = d.kernel = d.tab = d.store = P
    d.wave_len, d.store_len, d.max_count = 1000, 4096, 300
    d.S, d.up, d.down, d.width, d.taps, d.wave_i16 = 3, 160, 441, 17, 475, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REJECTS = [({'wave': None}, b'wave is null'), ({'kernel': None}, b'kernel is null'), ({'tab': None}, b'tab is null'), ({'store': None}, b'store is null'),
           ({'S': 0}, b'S=0'), ({'S': -1}, b'S=-1'), ({'S': 65536}, b'S=65536'),
           ({'taps': 474}, b'taps=474 must be 2 * width + down'), ({'width': 16}, b'taps=475 must be 2 * width + down'), ({'width': -1, 'taps': 439}, b'must be 2 * width + down'),
           ({'up': 0}, b'up=0'), ({'down': 0, 'taps': 34}, b'down=0'), ({'up': -160}, b'up=-160'),
           ({'max_count': -1}, b'max_count=-1'), ({'wave_i16': 2}, b'wave_i16=2'), ({'wave_i16': -1}, b'wave_i16=-1'),
           ({'wave_len': -1}, b'wave_len=-1'), ({'store_len': -5}, b'store_len=-5'),
           ({'up': 16000, 'down': 16001, 'width': 7, 'taps': 16015}, b'exceeds 64 KB of LDS')]


@pytest.mark.parametrize('kw,msg', REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in REJECTS])
def test_rejects_before_any_launch(lib, kw, msg):
    d = _desc(**kw)
    assert lib.hftt_resample_stream(C.byref(d), None) not in (0, 2, 3)
    assert msg in lib.hftt_last_error(), lib.hftt_last_error()


def test_rejects_a_null_descriptor_and_shares_the_window_rule_with_hftt_resample(lib):
    from hftt_hip import _capi, ops
    assert lib.hftt_resample_stream(None, None) != 0 and b'null descriptor' in lib.hftt_last_error()
    # the largest window that fits and the smallest that does not: the same verdict from both entry points and from the host's expression
    for up, down, width, fits in ((256, 8000, 192, True), (256, 8192, 0, True), (256, 8193, 0, False), (16000, 16001, 7, False), (160, 441, 17, True)):
        assert (ops.resample_stream_lds(up, down, width) <= 64 * 1024) == fits
        taps = 2 * width + down
        assert ((255 // up + 1) * down + taps) * 4 == ops.resample_stream_lds(up, down, width)
        r = _capi.ResampleDesc()
        r.wave = r.kernel = r.out = P
        r.n_in, r.n_out, r.up, r.down, r.width, r.taps = 10 * down, 1, up, down, width, taps
        if not fits:
            assert lib.hftt_resample(C.byref(r), None) not in (0, 2, 3) and b'exceeds 64 KB of LDS' in lib.hftt_last_error()
            assert lib.hftt_resample_stream(C.byref(_desc(up=up, down=down, width=width, taps=taps)), None) not in (0, 2, 3)
            assert b'exceeds 64 KB of LDS' in lib.hftt_last_error()


def test_plan_is_pure_host_arithmetic():
    from hftt_hip import ops
    up, down, width = 160, 441, 17
    assert ops.resample_stream_plan(0, 0, up, down, width, False) == (0, 0, 0)
    assert ops.resample_stream_plan(0, 0, up, down, width, True) == (0, 0, 0)
    assert ops.resample_stream_plan(width + down - 1, 0, up, down, width, False) == (0, 0, 0)
    assert ops.resample_stream_plan(width + down, 0, up, down, width, False) == (0, up, down - width)
    assert ops.resample_stream_plan(width + down, 0, up, down, width, True) == (0, -(-(width + down) * up // down), down - width)
    assert ops.resample_stream_plan(10 * down + width, 7 * up, up, down, width, False) == (7 * up, 3 * up, 10 * down - width)
    assert ops.resample_stream_plan(5, 5, 1, 1, 0, False) == (5, 0, 5) and ops.resample_stream_plan(9, 5, 1, 1, 0, False) == (5, 4, 9)
    assert ops.stream_frames_plan(1023, 0, False, 256, 2048) == (0, 0) and ops.stream_frames_plan(1024, 0, False, 256, 2048) == (0, 1)
    assert ops.stream_frames_plan(1024 + 255, 1, False, 256, 2048) == (1, 1) and ops.stream_frames_plan(1024 + 256, 1, False, 256, 2048) == (1, 2)
    assert ops.stream_frames_plan(0, 0, True, 256, 2048) == (0, 1) and ops.stream_frames_plan(512, 1, True, 256, 2048) == (1, 3)


def test_python_entry_points_fail_loudly_without_a_device(lib):
    from hftt_hip import HfttError, ops
    from model.amt import AMT
    with pytest.raises(HfttError, match='ROCm'):
        ops.ResampleStream(1, 44100, 16000, 'cpu')
    with pytest.raises(HfttError, match='ROCm'):
        ops.ResampleStream(2, 16000, 16000, 'cpu')
    with pytest.raises(HfttError, match='LDS'):
        ops.ResampleStream(1, 16001, 16000, 'cpu')
    with pytest.raises(HfttError):
        ops.ResampleStream(0, 44100, 16000, 'cpu')
    with pytest.raises(HfttError, match='ResampleStream'):
        ops.resample_stream(None, [None])
    with pytest.raises(HfttError, match='ResampleStream'):
        ops.stream_logmel(None, None)
    cfg = {'feature': {'sr': 16000, 'hop_sample': 256, 'mel_bins': 12, 'n_bins': 12, 'fft_bins': 2048, 'window_length': 2048, 'log_offset': 1e-8},
           'input': {'margin_b': 2, 'margin_f': 2, 'num_frame': 8, 'min_value': -18.5},
           'midi': {'note_min': 21, 'note_max': 28, 'num_note': 8, 'num_velocity': 4}}
    with pytest.raises(HfttError, match='ROCm'):
        AMT(cfg, None, device='cpu').open_stream(sr=44100)
    with pytest.raises(HfttError, match='rate 16001.*LDS'):
        AMT(cfg, None, device='cuda').open_stream(sr=16001)
    with pytest.raises(HfttError, match='sr=0'):
        AMT(cfg, None, device='cuda').open_stream(sr=0)


def test_one_copy_of_the_fir():
    """the window staging and the tap loop live in resample_fir.h alone; both kernels include it and hold no fmaf of their own"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ('logmel.hip', 'resample_stream.hip', 'resample_fir.h')}
    assert '__global__' not in src['resample_fir.h']
    assert len(re.findall(r'a0 = fmaf\(w\[t\], k\[t\], a0\)', src['resample_fir.h'])) == 2 and '(a0 + a1) + (a2 + a3)' in src['resample_fir.h']
    for f in ('logmel.hip', 'resample_stream.hip'):
        assert '#include "resample_fir.h"' in src[f] and 'fmaf' not in src[f], f
        assert len(re.findall(r'resample_stage\(', src[f])) == 1 and len(re.findall(r'resample_taps\(', src[f])) == 1, f
    assert 'asm' not in src['resample_stream.hip'] and '__builtin_amdgcn' not in src['resample_stream.hip']


def test_kernels_use_no_scratch():
    res = hipcc_remarks.resources('resample_stream.hip')
    names = {n for n in res if n.startswith('resample_stream_kernel')}
    assert len(names) == 2, sorted(res)                                       # fp32 and int16 input
    for name in sorted(names):
        v = res[name]
        assert hipcc_remarks.get(v, 'ScratchSize') == 0, (name, v)
        assert hipcc_remarks.get(v, 'VGPRs') <= 64, (name, v)                  # eight waves per SIMD stay possible: the tap loop is latency bound
        assert hipcc_remarks.get(v, 'LDS Size') == 0, (name, v)               # the window is dynamic LDS: (255 / up + 1) * down + taps floats
        print('%s: VGPRs %d, SGPRs %d, scratch 0, static LDS 0 B, occupancy %s' % (name, hipcc_remarks.get(v, 'VGPRs'), hipcc_remarks.get(v, 'SGPRs'), hipcc_remarks.get(v, 'Occupancy')))
    whole = hipcc_remarks.resources('logmel.hip')['resample_kernel']
    assert hipcc_remarks.get(whole, 'ScratchSize') == 0
