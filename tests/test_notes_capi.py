"""C ABI of the note decoder (hftt_stitch, hftt_notes_decode, hftt_notes_ws_bytes): descriptor layouts against the C compiler, every host-side
rejection (they run before the device guard and the launch, so a box without a GPU tests them), the workspace helper, and the loud failure
of the Python entry points on CPU tensors.  No compute calls."""
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
    structs = {'hftt_stitch_desc': _capi.StitchDesc, 'hftt_notes_desc': _capi.NotesDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines += ['printf("HFTT_STITCH_MAX_CLIPS %d\\n", HFTT_STITCH_MAX_CLIPS);', 'printf("HFTT_NOTES_CHUNK %d\\n", HFTT_NOTES_CHUNK);',
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
    assert int(got['HFTT_STITCH_MAX_CLIPS']) == _capi.STITCH_MAX_CLIPS and int(got['HFTT_NOTES_CHUNK']) == _capi.NOTES_CHUNK
    assert int(got['HFTT_ABI_VERSION']) == 8 == lib.hftt_abi_version()          # the new symbols were added AT version 8


P = 0x1000          # a non-null "device pointer": every case below is refused before anything dereferences it


def _stitch(rows=(0, 8, 16), **kw):
    from hftt_hip import _capi
    d = _capi.StitchDesc()
    d.b, d.T, d.N, d.V, d.src0, d.len, d.F = 3, 8, 8, 4, 0, 8, 24
    for name in ('onset', 'offset', 'mpe', 'velocity', 'roll_onset', 'roll_offset', 'roll_mpe', 'roll_velocity'):
        setattr(d, name, P)
    keep = (C.c_int32 * len(rows))(*rows)
    d.dst = keep
    for k, v in kw.items():
        setattr(d, k, v)
    return d, keep


def _notes(**kw):
    from hftt_hip import _capi
    d = _capi.NotesDesc()
    d.F, d.N, d.note_min, d.cap, d.hop_sec = 160, 88, 21, 100, 0.016
    d.thred_onset = d.thred_offset = d.thred_mpe = 0.5
    for name in ('onset', 'offset', 'mpe', 'velocity', 'out_pitch', 'out_velocity', 'out_onset', 'out_offset', 'n_notes', 'ws'):
        setattr(d, name, P)
    d.ws_bytes = 1 << 30
    for k, v in kw.items():
        setattr(d, k, v)
    return d


STITCH_REJECTS = [({'onset': None}, b'null operand'), ({'offset': None}, b'null operand'), ({'mpe': None}, b'null operand'),
                  ({'velocity': None}, b'velocity'), ({'roll_onset': None}, b'null roll'), ({'roll_offset': None}, b'null roll'),
                  ({'roll_mpe': None}, b'null roll'), ({'roll_velocity': None}, b'roll_velocity'),
                  ({'dst': C.POINTER(C.c_int32)()}, b'dst is null'),
                  ({'F': -1}, b'F=-1'), ({'N': 0}, b'N=0'), ({'N': 129}, b'N=129'), ({'V': 0}, b'V=0'), ({'V': 129}, b'V=129'),
                  ({'b': 0}, b'b=0'), ({'b': 65}, b'b=65'), ({'T': 0}, b'T=0'),
                  ({'len': 0}, b'len=0'), ({'len': 9}, b'len=9'), ({'src0': -1}, b'src0=-1'), ({'src0': 1}, b'src0=1'),
                  ({'len': 4, 'src0': 5}, b'src0=5')]


@pytest.mark.parametrize('kw,msg', STITCH_REJECTS, ids=['-'.join('%s=%s' % (n, v if isinstance(v, (int, type(None))) else 'NULL') for n, v in k.items()) for k, _ in STITCH_REJECTS])
def test_stitch_rejects_before_any_launch(lib, kw, msg):
    d, keep = _stitch(**kw)
    assert lib.hftt_stitch(C.byref(d), None) not in (0, 2, 3)
    assert msg in lib.hftt_last_error(), lib.hftt_last_error()


@pytest.mark.parametrize('dst,msg', [((0, 8, 17), b'dst[2]=17'), ((-1, 8, 16), b'dst[0]=-1'), ((0, 4, 16), b'overlap'), ((0, 16, 16), b'overlap')])
def test_stitch_rejects_rows_outside_the_rolls_and_two_writers(lib, dst, msg):
    d, keep = _stitch(rows=dst)
    assert lib.hftt_stitch(C.byref(d), None) not in (0, 2, 3)
    assert msg in lib.hftt_last_error(), lib.hftt_last_error()
    assert lib.hftt_stitch(None, None) != 0 and b'null descriptor' in lib.hftt_last_error()


NOTES_REJECTS = [({'F': -1}, b'F=-1'), ({'N': 0}, b'N=0'), ({'N': 129}, b'N=129'), ({'cap': -1}, b'cap=-1'),
                 ({'mode_velocity': 2}, b'mode_velocity=2'), ({'mode_velocity': -1}, b'mode_velocity=-1'),
                 ({'mode_offset': 3}, b'mode_offset=3'), ({'mode_offset': -1}, b'mode_offset=-1'),
                 ({'n_notes': None}, b'n_notes'), ({'out_pitch': None}, b'out_pitch'), ({'out_velocity': None}, b'out_velocity'),
                 ({'out_onset': None}, b'out_onset'), ({'out_offset': None}, b'out_offset'),
                 ({'onset': None}, b'null roll'), ({'offset': None}, b'null roll'), ({'mpe': None}, b'null roll'), ({'velocity': None}, b'velocity'),
                 ({'ws': None}, b'ws is null'), ({'ws_bytes': 0}, b'ws_bytes=0'), ({'F': 1 << 40}, b'2^31')]


@pytest.mark.parametrize('kw,msg', NOTES_REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in NOTES_REJECTS])
def test_notes_decode_rejects_before_any_launch(lib, kw, msg):
    d = _notes(**kw)
    assert lib.hftt_notes_decode(C.byref(d), None) not in (0, 2, 3)
    assert msg in lib.hftt_last_error(), lib.hftt_last_error()


def test_notes_decode_rejects_a_workspace_one_byte_short(lib):
    need = lib.hftt_notes_ws_bytes(160, 88)
    d = _notes(ws_bytes=need - 1)
    assert lib.hftt_notes_decode(C.byref(d), None) not in (0, 2, 3)
    assert b'ws_bytes=%d below' % (need - 1) in lib.hftt_last_error(), lib.hftt_last_error()
    assert lib.hftt_notes_decode(None, None) != 0 and b'null descriptor' in lib.hftt_last_error()


def test_notes_ws_bytes_is_positive_and_monotone(lib):
    from hftt_hip import _capi
    ch = _capi.NOTES_CHUNK
    prev = 0
    for F in (0, 1, ch - 1, ch, ch + 1, 2 * ch + 1, 3750, 225000):
        row = [lib.hftt_notes_ws_bytes(F, N) for N in (1, 8, 88, 128)]
        assert all(x > 0 for x in row) and row == sorted(row), (F, row)
        assert row[2] >= prev, F
        prev = row[2]
    assert lib.hftt_notes_ws_bytes(225000, 88) > lib.hftt_notes_ws_bytes(3750, 88) > lib.hftt_notes_ws_bytes(1, 88)
    assert lib.hftt_notes_ws_bytes(3750, 88) > lib.hftt_notes_ws_bytes(3750, 8)
    assert lib.hftt_notes_ws_bytes(225000, 88) < 16 << 20          # per-chunk state, not per-frame lists: an hour stays in megabytes
    assert lib.hftt_notes_ws_bytes(-1, 88) == 0 and lib.hftt_notes_ws_bytes(10, 0) == 0 and lib.hftt_notes_ws_bytes(10, 129) == 0


def test_python_entry_points_refuse_cpu_tensors():
    from hftt_hip import HfttError, ops
    from model.amt import AMT
    z = torch.zeros(16, 8)
    with pytest.raises(HfttError):
        ops.notes_decode(z, z, z, z.to(torch.int8), 0.016)
    with pytest.raises(HfttError):
        ops.stitch(torch.zeros(1, 8, 8), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, 4), (z, z, z, z.to(torch.int8)), [0])
    cfg = {'feature': {'sr': 16000, 'hop_sample': 256, 'mel_bins': 12, 'n_bins': 12},
           'input': {'margin_b': 2, 'margin_f': 2, 'num_frame': 8, 'min_value': -18.5},
           'midi': {'note_min': 21, 'note_max': 28, 'num_note': 8, 'num_velocity': 4}}
    amt = AMT(cfg, None, device='cpu')
    with pytest.raises(HfttError):
        amt.transcript_notes(np.zeros((21, 12), np.float32))
    with pytest.raises(HfttError):
        amt.transcript_notes(torch.zeros(21, 12))
    sharded = AMT(cfg, None, rank=0, world=2, device='cuda')
    with pytest.raises(HfttError, match='world'):
        sharded.transcript_notes(np.zeros((21, 12), np.float32))
