"""C ABI of the streaming note decoder (hftt_notes_stream_step, hftt_notes_stream_state_bytes): the symbols at ABI 8, the descriptor layout
against the C compiler, every host-side rejection with its text (they run before the device guard and the launch, so a box without a GPU
tests them), the state-size helper, the loud failure of the Python entry points without a device, and the step kernels' compile remarks.
No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hipcc_remarks
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


def test_symbols_are_exported_and_bound_at_abi_8(lib):
    from hftt_hip import _capi
    src = open(HDR).read()
    for name in ('hftt_notes_stream_step', 'hftt_notes_stream_state_bytes'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert lib.hftt_abi_version() == _capi.ABI_VERSION == 8
    assert int(re.search(r'#define HFTT_ABI_VERSION (\d+)', src).group(1)) == 8


def test_descriptor_layout_matches_the_c_compiler(lib, tmp_path):
    from hftt_hip import _capi
    cname, cls = 'hftt_notes_stream_desc', _capi.NotesStreamDesc
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
POINTERS = ('onset', 'offset', 'mpe', 'velocity', 'row_end', 'closed', 'state', 'out_pitch', 'out_velocity', 'out_onset', 'out_offset',
            'stream_notes', 'n_notes', 'overflow')


def _desc(lib, **kw):
    from hftt_hip import _capi
    d = _capi.NotesStreamDesc()
    d.S, d.N, d.H, d.note_min, d.cap, d.max_new, d.hop_sec = 3, 88, 512, 21, 100, 128, 0.016
    d.thred_onset = d.thred_offset = d.thred_mpe = 0.5
    for name in POINTERS:
        setattr(d, name, P)
    d.state_bytes = lib.hftt_notes_stream_state_bytes(3, 88)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REJECTS = [({name: None}, name.encode() if name.startswith('out_') or name in ('row_end', 'closed', 'stream_notes', 'n_notes', 'overflow') else
            (b'state is null' if name == 'state' else b'null ring')) for name in POINTERS] + [
    ({'S': 0}, b'S=0'), ({'S': -1}, b'S=-1'), ({'N': 0}, b'N=0'), ({'N': 129}, b'N=129'),
    ({'H': 3}, b'H=3'), ({'H': 0}, b'H=0'), ({'max_new': 513}, b'max_new=513'), ({'max_new': -1}, b'max_new=-1'),
    ({'mode_offset': 1}, b"'shorter'"), ({'mode_offset': 2}, b"'shorter'"), ({'mode_offset': -1}, b'mode_offset=-1'),
    ({'mode_velocity': 2}, b'mode_velocity=2'), ({'cap': -1}, b'cap=-1'), ({'state_bytes': 0}, b'state_bytes=0')]


@pytest.mark.parametrize('kw,msg', REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in REJECTS])
def test_rejects_before_any_launch(lib, kw, msg):
    d = _desc(lib, **kw)
    assert lib.hftt_notes_stream_step(C.byref(d), None) not in (0, 2, 3)
    assert msg in lib.hftt_last_error(), lib.hftt_last_error()


def test_rejects_a_state_one_byte_short_and_a_null_descriptor(lib):
    need = lib.hftt_notes_stream_state_bytes(3, 88)
    d = _desc(lib, state_bytes=need - 1)
    assert lib.hftt_notes_stream_step(C.byref(d), None) not in (0, 2, 3)
    assert b'state_bytes=%d below' % (need - 1) in lib.hftt_last_error(), lib.hftt_last_error()
    assert lib.hftt_notes_stream_step(None, None) != 0 and b'null descriptor' in lib.hftt_last_error()
    # no room asked for: no arrays needed.  The state is validated after the output-array rule, so a null state makes this a host-side
    # rejection whose text shows that the rule let cap = 0 through: nothing launches on the fake pointers, with or without a device
    d = _desc(lib, cap=0, out_pitch=None, out_onset=None, state=None)
    assert lib.hftt_notes_stream_step(C.byref(d), None) not in (0, 2, 3)
    assert b'state is null' in lib.hftt_last_error() and b'null output' not in lib.hftt_last_error(), lib.hftt_last_error()


def test_state_bytes_is_per_stream_and_pitch_not_per_row(lib):
    f = lib.hftt_notes_stream_state_bytes
    assert f(1, 1) == 68 and f(3, 88) == 68 * 3 * 88 and f(32, 128) == 68 * 32 * 128       # a 64-byte record and one count each
    assert f(1, 88) < f(2, 88) < f(2, 128)
    assert f(0, 88) == 0 and f(-1, 88) == 0 and f(1, 0) == 0 and f(1, 129) == 0 and f(1 << 20, 128) == 0


def test_python_entry_points_fail_loudly_without_a_device(lib):
    from hftt_hip import HfttError, ops
    from model.amt import AMT
    with pytest.raises(HfttError, match='ROCm'):
        ops.notes_stream_state(1, 8, 64, 'cpu')
    with pytest.raises(HfttError):
        ops.notes_stream_state(1, 8, 3, 'cpu')
    with pytest.raises(HfttError):
        ops.notes_stream_step(None, 0.016)
    cfg = {'feature': {'sr': 16000, 'hop_sample': 256, 'mel_bins': 12, 'n_bins': 12},
           'input': {'margin_b': 2, 'margin_f': 2, 'num_frame': 8, 'min_value': -18.5},
           'midi': {'note_min': 21, 'note_max': 28, 'num_note': 8, 'num_velocity': 4}}
    with pytest.raises(HfttError, match='ROCm'):
        AMT(cfg, None, device='cpu').open_stream()
    with pytest.raises(HfttError, match='world'):
        AMT(cfg, None, rank=0, world=2, device='cuda').open_stream()
    for mode in ('longer', 'offset'):
        with pytest.raises(HfttError, match="'shorter'"):
            AMT(cfg, None, device='cuda').open_stream(mode_offset=mode)
    with pytest.raises(HfttError, match='output'):
        AMT(cfg, None, device='cuda').open_stream(output='AB')
    with pytest.raises(HfttError, match='history'):
        AMT(cfg, None, device='cuda').open_stream(history=12)


def test_step_kernels_use_no_scratch():
    res = hipcc_remarks.resources('notes_stream.hip')
    names = {'notes_stream_count_kernel', 'notes_stream_offsets_kernel', 'notes_stream_emit_kernel'}
    assert names <= set(res), sorted(res)
    for name in names:
        assert hipcc_remarks.get(res[name], 'ScratchSize') == 0, (name, res[name])
        assert hipcc_remarks.get(res[name], 'VGPRs') <= 128, (name, res[name])      # two waves per workgroup stay resident side by side
