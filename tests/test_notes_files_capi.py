"""C ABI of the file-list entry points (hftt_clip_windows, hftt_notes_decode_seg, hftt_notes_seg_ws_bytes): descriptor layouts against the C
compiler, every host-side rejection (they run before the device guard and the launch, so a box without a GPU tests them), the workspace
helper, and the loud failure of the Python entry points without a device.  No compute calls."""
import ctypes as C
import os
import subprocess

import numpy as np
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


def test_descriptor_layouts_match_the_c_compiler(lib, tmp_path):
    from hftt_hip import _capi
    structs = {'hftt_clip_windows_desc': _capi.ClipWindowsDesc, 'hftt_notes_seg_desc': _capi.NotesSegDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines += ['printf("notes %zu\\n", sizeof(hftt_notes_desc));', 'printf("HFTT_NOTES_CHUNK %d\\n", HFTT_NOTES_CHUNK);',
              'printf("HFTT_ABI_VERSION %d\\n", HFTT_ABI_VERSION);', 'return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')
    got = dict(l.split() for l in out if l)
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])
    assert int(got['notes']) == C.sizeof(_capi.NotesDesc) == _capi.NotesSegDesc.n_seg.offset       # the one-file descriptor, embedded first
    assert int(got['HFTT_NOTES_CHUNK']) == _capi.NOTES_CHUNK
    assert int(got['HFTT_ABI_VERSION']) == 8 == lib.hftt_abi_version() == _capi.ABI_VERSION         # the new symbols were added AT version 8


P = 0x1000          # a non-null "device pointer": every case below is refused before anything dereferences it


def _clip(**kw):
    from hftt_hip import _capi
    d = _capi.ClipWindowsDesc()
    d.B, d.width, d.n_bins, d.n_files, d.R, d.fill = 4, 192, 256, 3, 1000, -18.0
    for name in ('feature', 'file_row0', 'win_file', 'win_start', 'out'):
        setattr(d, name, P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


CLIP_REJECTS = [({'feature': None}, b'feature'), ({'file_row0': None}, b'file_row0'), ({'win_file': None}, b'win_file'),
                ({'win_start': None}, b'win_start'), ({'out': None}, b'out'),
                ({'B': 0}, b'B=0'), ({'B': -1}, b'B=-1'), ({'width': 0}, b'width=0'), ({'n_bins': 0}, b'n_bins=0'), ({'n_bins': -3}, b'n_bins=-3'),
                ({'n_files': -1}, b'n_files=-1'), ({'R': -1}, b'R=-1'),
                ({'B': 1 << 15, 'n_bins': 256, 'width': 256}, b'2^31'), ({'B': (1 << 31) - 1, 'n_bins': (1 << 31) - 1, 'width': (1 << 31) - 1}, b'2^31')]


@pytest.mark.parametrize('kw,msg', CLIP_REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in CLIP_REJECTS])
def test_clip_windows_rejects_before_any_launch(lib, kw, msg):
    d = _clip(**kw)
    assert lib.hftt_clip_windows(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'clip_windows:') and msg in err, err


def test_clip_windows_null_descriptor(lib):
    assert lib.hftt_clip_windows(None, None) not in (0, 2, 3) and b'null descriptor' in lib.hftt_last_error()


def _seg(table=(0, 100, 100, 160), **kw):
    """a descriptor that passes every check; `table`: the host rows (None: a null pointer)"""
    from hftt_hip import _capi
    s = _capi.NotesSegDesc()
    d = s.notes
    d.F, d.N, d.note_min, d.cap, d.hop_sec = 160, 88, 21, 100, 0.016
    d.thred_onset = d.thred_offset = d.thred_mpe = 0.5
    for name in ('onset', 'offset', 'mpe', 'velocity', 'out_pitch', 'out_velocity', 'out_onset', 'out_offset', 'n_notes', 'ws'):
        setattr(d, name, P)
    d.ws_bytes = 1 << 30
    keep = None
    if table is not None:
        keep = (C.c_int32 * len(table))(*table)
        s.seg_row0_host = keep
        s.n_seg = len(table) - 1
    s.seg_row0, s.seg_notes = P, P
    for k, v in kw.items():
        if hasattr(d, k) and k not in ('n_seg', 'seg_row0', 'seg_notes'):
            setattr(d, k, v)
        else:
            setattr(s, k, v)
    return s, keep


def _refused(lib, s, msg):
    assert lib.hftt_notes_decode_seg(C.byref(s), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'notes_decode_seg:') and msg in err, err


# the one-file decode's own rejections (tests/test_notes_capi.py NOTES_REJECTS), through the segmented entry point
NOTES_REJECTS = [({'F': -1}, b'F=-1'), ({'N': 0}, b'N=0'), ({'N': 129}, b'N=129'), ({'cap': -1}, b'cap=-1'),
                 ({'mode_velocity': 2}, b'mode_velocity=2'), ({'mode_velocity': -1}, b'mode_velocity=-1'),
                 ({'mode_offset': 3}, b'mode_offset=3'), ({'mode_offset': -1}, b'mode_offset=-1'),
                 ({'n_notes': None}, b'n_notes'), ({'out_pitch': None}, b'out_pitch'), ({'out_velocity': None}, b'out_velocity'),
                 ({'out_onset': None}, b'out_onset'), ({'out_offset': None}, b'out_offset'),
                 ({'onset': None}, b'null roll'), ({'offset': None}, b'null roll'), ({'mpe': None}, b'null roll'), ({'velocity': None}, b'velocity'),
                 ({'ws': None}, b'ws is null'), ({'ws_bytes': 0}, b'ws_bytes=0'), ({'F': 1 << 40}, b'2^31')]
SEG_REJECTS = [({'n_seg': -1}, b'n_seg=-1'), ({'seg_notes': None}, b'seg_notes'), ({'seg_row0': None}, b'seg_row0'),
               ({'seg_row0_host': C.POINTER(C.c_int32)()}, b'seg_row0_host')]


@pytest.mark.parametrize('kw,msg', NOTES_REJECTS + SEG_REJECTS,
                         ids=['-'.join('%s=%s' % (n, v if isinstance(v, (int, type(None))) else 'NULL') for n, v in k.items()) for k, _ in NOTES_REJECTS + SEG_REJECTS])
def test_notes_decode_seg_rejects_before_any_launch(lib, kw, msg):
    s, keep = _seg(**kw)
    _refused(lib, s, msg)


@pytest.mark.parametrize('table,msg', [((1, 100, 160), b'seg_row0_host[0]=1'), ((-1, 100, 160), b'seg_row0_host[0]=-1'),
                                       ((0, 100, 99, 160), b'seg_row0_host[2]=99'), ((0, 161, 160), b'seg_row0_host[2]=160'),
                                       ((0, 100, 159), b'=159 must be F=160'), ((0, 100, 161), b'=161 must be F=160'), ((0,), b'seg_row0_host')],
                         ids=['first-1', 'first-neg', 'decreasing', 'decreasing-last', 'short', 'long', 'n_seg-0-with-rows'])
def test_notes_decode_seg_rejects_a_bad_row_table(lib, table, msg):
    s, keep = _seg(table=table)
    _refused(lib, s, msg)


def test_notes_decode_seg_null_descriptor_and_a_workspace_one_byte_short(lib):
    assert lib.hftt_notes_decode_seg(None, None) not in (0, 2, 3) and b'null descriptor' in lib.hftt_last_error()
    need = lib.hftt_notes_seg_ws_bytes(160, 88, 3)
    s, keep = _seg(ws_bytes=need - 1)
    _refused(lib, s, b'ws_bytes=%d below' % (need - 1))
    # n_seg == 0 needs no table: with F == 0 and null tables the first complaint is the workspace's
    s, keep = _seg(table=None, F=0, n_seg=0, seg_row0=None, ws_bytes=0)
    _refused(lib, s, b'ws_bytes=0 below')


def test_notes_seg_ws_bytes_is_monotone_and_zero_outside_the_domain(lib):
    from hftt_hip import _capi
    ch = _capi.NOTES_CHUNK
    Fs, Ns, Ss = (0, 1, ch - 1, ch, ch + 1, 2 * ch + 1, 3750, 225000), (1, 8, 88, 128), (0, 1, 2, 15, 16, 17, 360, 5000)
    v = np.array([[[lib.hftt_notes_seg_ws_bytes(F, N, S) for S in Ss] for N in Ns] for F in Fs], np.int64)
    assert (v > 0).all()
    assert (np.diff(v, axis=0) >= 0).all() and (np.diff(v, axis=1) >= 0).all() and (np.diff(v[1:], axis=1) > 0).all() and (np.diff(v, axis=2) > 0).all()
    assert v[-1, 2, 0] > v[-2, 2, 0] > v[1, 2, 0]
    # room for the chunks of ANY borders: n_seg segments add at most one partial chunk each to those of one file
    for F, N, S in ((160, 88, 3), (225000, 88, 360), (1, 1, 1)):
        assert lib.hftt_notes_seg_ws_bytes(F, N, S) >= lib.hftt_notes_ws_bytes(F, N) + 4 * (S + 1) + 4 * 9 * N * S
    assert lib.hftt_notes_seg_ws_bytes(225000, 88, 360) < 32 << 20          # per-chunk state: an hour in 360 files stays in megabytes
    for bad in ((-1, 88, 3), (10, 0, 3), (10, 129, 3), (10, 88, -1)):
        assert lib.hftt_notes_seg_ws_bytes(*bad) == 0, bad


def test_python_entry_points_refuse_cpu_tensors():
    from hftt_hip import HfttError, ops
    from model.amt import AMT
    z = torch.zeros(16, 8)
    with pytest.raises(HfttError):
        ops.notes_decode_seg(z, z, z, z.to(torch.int8), [0, 16], 0.016)
    with pytest.raises(HfttError):
        ops.clip_windows(torch.zeros(16, 12), [0, 16], [0], [0], 4, -18.0)
    cfg = {'feature': {'sr': 16000, 'hop_sample': 256, 'mel_bins': 12, 'n_bins': 12},
           'input': {'margin_b': 2, 'margin_f': 2, 'num_frame': 8, 'min_value': -18.5},
           'midi': {'note_min': 21, 'note_max': 28, 'num_note': 8, 'num_velocity': 4}}
    amt = AMT(cfg, None, device='cpu')
    with pytest.raises(HfttError):
        amt.transcript_notes_files([np.zeros((21, 12), np.float32)])
    with pytest.raises(HfttError):
        amt.transcript_notes_files([torch.zeros(21, 12)])
    with pytest.raises(HfttError, match='world'):
        AMT(cfg, None, rank=0, world=2, device='cuda').transcript_notes_files([np.zeros((21, 12), np.float32)])
    with pytest.raises(HfttError, match='output'):
        AMT(cfg, None, device='cuda').transcript_notes_files([np.zeros((21, 12), np.float32)], output='C')
