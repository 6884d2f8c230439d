"""C ABI and host half of the label renderer (hftt_labels_render, hftt_hip.ops.labels_table_host): descriptor layout against the C compiler, every
host-side refusal (they run before the device guard and the launch, so a box without a GPU tests them), and the note table: grouping in list
order, CSR bounds, the "no offset target" bit, file lengths, the reference's working domain.  No compute calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import util
from hipcc_remarks import get, resources

HDR = os.path.join(util.ROOT, 'include', 'hftt_hip.h')
CFG = {'feature': {'sr': 16000, 'hop_sample': 256}, 'midi': {'note_min': 21, 'num_note': 88}}


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
    from hftt_hip import _capi, ops
    structs = {'hftt_labels_desc': _capi.LabelsDesc, 'hftt_label_note': _capi.LabelNote}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines += ['printf("HFTT_LABELS_CHUNK %d\\n", HFTT_LABELS_CHUNK);', 'printf("HFTT_LABELS_TRAIN %d\\n", HFTT_LABELS_TRAIN);',
              'printf("HFTT_LABELS_STORE %d\\n", HFTT_LABELS_STORE);', 'printf("HFTT_ABI_VERSION %d\\n", HFTT_ABI_VERSION);', 'return 0; }']
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
    assert int(got['HFTT_LABELS_CHUNK']) == _capi.LABELS_CHUNK
    assert (int(got['HFTT_LABELS_TRAIN']), int(got['HFTT_LABELS_STORE'])) == (_capi.LABELS_TRAIN, _capi.LABELS_STORE)
    assert int(got['HFTT_ABI_VERSION']) == 8 == lib.hftt_abi_version()          # the symbol was added AT version 8
    # the numpy record that the table builder uploads is the C record
    assert ops.LABEL_NOTE.itemsize == int(got['hftt_label_note'])
    for name in ops.LABEL_NOTE.names:
        assert ops.LABEL_NOTE.fields[name][1] == int(got['hftt_label_note.' + name]), name


P = 0x1000          # a non-null "device pointer": every case below is refused before anything dereferences it
POINTERS = ('notes', 'row_ptr', 'file_nframe', 'win_file', 'win_start', 'onset', 'offset', 'mpe', 'velocity')


def _desc(**kw):
    from hftt_hip import _capi
    d = _capi.LabelsDesc()
    d.n_files, d.n_notes, d.B, d.len, d.N, d.tol, d.duration_tolerance, d.form = 2, 10, 8, 128, 88, 3, 0, 0
    d.hop_ms, d.fps = 16.0, 62.5
    for name in POINTERS:
        setattr(d, name, P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REJECTS = [({'notes': None}, b'notes is null'), ({'row_ptr': None}, b'row_ptr is null'), ({'file_nframe': None}, b'file_nframe is null'),
           ({'win_file': None}, b'win_file is null'), ({'win_start': None}, b'win_start is null'),
           ({'onset': None}, b'null output (onset'), ({'offset': None}, b'null output (onset / offset'), ({'mpe': None}, b'/ mpe'),
           ({'velocity': None}, b'/ velocity'),
           ({'B': 0}, b'B=0'), ({'B': -1}, b'B=-1'), ({'len': 0}, b'len=0'), ({'len': -5}, b'len=-5'), ({'N': 0}, b'N=0'), ({'N': 129}, b'N=129'),
           ({'tol': 0}, b'tol=0'), ({'tol': -1}, b'tol=-1'), ({'n_files': 0}, b'n_files=0'), ({'n_files': -1}, b'n_files=-1'),
           ({'n_notes': -1}, b'n_notes=-1'), ({'form': 2}, b'form=2'), ({'form': -1}, b'form=-1'),
           ({'duration_tolerance': 2}, b'duration_tolerance=2'), ({'hop_ms': 0.0}, b'hop_ms=0'), ({'fps': -1.0}, b'fps=-1'),
           ({'B': 1 << 17, 'len': 1 << 7, 'N': 128}, b'2^31'), ({'B': 190651, 'len': 128, 'N': 88}, b'2^31')]


@pytest.mark.parametrize('kw,msg', REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in REJECTS])
def test_labels_render_rejects_before_any_launch(lib, kw, msg):
    d = _desc(**kw)
    assert lib.hftt_labels_render(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'labels_render: ') and msg in err, err


def test_labels_render_rejects_a_null_descriptor(lib):
    assert lib.hftt_labels_render(None, None) not in (0, 2, 3) and b'null descriptor' in lib.hftt_last_error()


def _note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


def test_table_groups_by_file_and_pitch_in_list_order():
    '''a deliberately time-unsorted list: inside a (file, pitch) group the records keep the caller's order (it decides the velocity where
    onset triangles overlap), pitches ascend, files ascend, and the CSR index bounds every group'''
    from hftt_hip import ops
    f0 = [_note(60, 3.0, 3.5, 1), _note(40, 2.0, 2.5, 2), _note(60, 1.0, 1.5, 3), _note(108, 0.25, 9.0, 4), _note(60, 2.0, 2.25, 5), _note(21, 5.0, 5.5, 6)]
    f2 = [_note(60, 0.5, 0.75, 7), _note(60, 0.125, 0.25, 8)]
    t = ops.labels_table_host([f0, [], f2], CFG)
    N = 88
    assert t['N'] == N and t['hop_ms'] == 16.0 and t['fps'] == 62.5 and t['tol'] == 3
    assert t['notes'].dtype == ops.LABEL_NOTE and t['row_ptr'].dtype == np.int32 and t['file_nframe'].dtype == np.int32
    rp = t['row_ptr']
    assert rp.shape == (3 * N + 1,) and rp[0] == 0 and rp[-1] == len(t['notes']) == 8 and (np.diff(rp) >= 0).all()
    assert t['notes']['velocity'].tolist() == [6, 2, 1, 3, 5, 4, 7, 8]

    def group(file, pitch):
        g = file * N + pitch - 21
        return t['notes'][rp[g]:rp[g + 1]]
    assert group(0, 60)['onset_sec'].tolist() == [3.0, 1.0, 2.0] and group(0, 60)['velocity'].tolist() == [1, 3, 5]
    assert group(2, 60)['onset_sec'].tolist() == [0.5, 0.125] and group(2, 60)['offset_sec'].tolist() == [0.75, 0.25]
    assert len(group(0, 21)) == len(group(0, 40)) == len(group(0, 108)) == 1 and len(group(0, 61)) == 0
    assert int(np.diff(rp)[N:2 * N].sum()) == 0                                      # the empty file owns N empty groups
    assert t['file_nframe'].tolist() == [int(9.0 * 62.5 + 0.5) + 1, 1, int(0.75 * 62.5 + 0.5) + 1]
    assert not t['notes']['flags'].any()


def test_table_sets_the_no_offset_bit_for_an_exact_restrike_only():
    from hftt_hip import ops
    near = float(np.nextafter(0.5, 1.0))
    notes = [_note(60, 0.2, 0.5, 1),          # ends exactly where the next one starts: no offset target
             _note(60, 0.5, 0.9, 2),
             _note(61, 0.2, near, 3),         # one ulp late: keeps its target
             _note(61, 0.5, 0.9, 4),
             _note(62, 0.2, 0.5, 5),          # the onset at 0.5 belongs to ANOTHER pitch (and, below, another file)
             _note(63, 0.7, 0.7, 6),          # a zero-length note ends at its own onset
             _note(64, 1.0, 1.5, 7), _note(64, 0.5, 1.0, 8)]         # the restruck note comes LATER in the list
    other = [_note(62, 0.5, 0.9, 9)]
    t = ops.labels_table_host([notes, other], CFG)
    by_velocity = dict(zip(t['notes']['velocity'].tolist(), t['notes']['flags'].tolist()))
    assert by_velocity == {1: 1, 2: 0, 3: 0, 4: 0, 5: 0, 6: 1, 7: 0, 8: 1, 9: 0}
    # -0.0 == 0.0 as doubles
    t = ops.labels_table_host([[_note(60, 0.0, 0.5), _note(60, 0.0, -0.0 + 0.0)], [_note(60, -0.0, 0.0)]], CFG)
    assert t['notes']['flags'].tolist() == [0, 1, 1]


def test_table_file_lengths():
    from hftt_hip import ops
    from corpus.conv_note2label import note2label_arrays
    files = [[], [_note(30, 0.0, 0.0)], [_note(30, 1.0, 7.3), _note(90, 2.0, 30.999)], [_note(50, 0.0, 0.007)], [_note(50, 0.0, 0.009)]]
    for cfg in (CFG, {'feature': {'sr': 44100, 'hop_sample': 512}, 'midi': CFG['midi']}, {'feature': {'sr': 16000, 'hop_sample': 160}, 'midi': CFG['midi']}):
        t = ops.labels_table_host(files, cfg)
        assert t['file_nframe'].tolist() == [note2label_arrays(cfg, a)['mpe'].shape[0] for a in files]
        assert t['file_nframe'][0] == 1
    assert ops.labels_table_host(files, {'feature': {'sr': 44100, 'hop_sample': 512}, 'midi': CFG['midi']})['tol'] == 4


BAD_NOTES = [(_note(20, 0.1, 0.2), 'pitch'), (_note(109, 0.1, 0.2), 'pitch'), (_note(60.5, 0.1, 0.2), 'pitch'),
             (_note(60, -0.001, 0.2), 'onset'), (_note(60, 0.3, 0.2), 'onset'), (_note(60, float('nan'), 0.2), 'onset'),
             (_note(60, 0.1, float('nan')), 'onset'), (_note(60, 0.1, float('inf')), 'offset'), (_note(60, 0.1, 1e9), 'offset'),
             (_note(60, 0.1, 0.2, -1), 'velocity'), (_note(60, 0.1, 0.2, 128), 'velocity'), (_note(60, 0.1, 0.2, 1.5), 'velocity')]


@pytest.mark.parametrize('bad,what', BAD_NOTES, ids=['%s-%s-%s-%s' % tuple(b.values()) for b, _ in BAD_NOTES])
def test_table_refuses_notes_outside_the_reference_domain(bad, what):
    from hftt_hip import HfttError, ops
    good = _note(60, 0.1, 0.2)
    with pytest.raises(HfttError, match=r'file 1, note 1: .*%s' % what):
        ops.labels_table_host([[good], [good, bad, good]], CFG)


def test_table_refuses_a_grid_without_a_triangle_and_an_empty_corpus():
    from hftt_hip import HfttError, ops
    with pytest.raises(HfttError, match='tol=0'):
        ops.labels_table_host([[]], {'feature': {'sr': 16000, 'hop_sample': 3200}, 'midi': CFG['midi']})       # 200 ms hop
    with pytest.raises(HfttError, match='no files'):
        ops.labels_table_host([], CFG)
    with pytest.raises(HfttError, match='num_note'):
        ops.labels_table_host([[]], {'feature': CFG['feature'], 'midi': {'note_min': 0, 'num_note': 129}})


def test_python_entry_points_refuse_cpu_tensors():
    from hftt_hip import HfttError, ops
    from corpus.conv_note2label import note2label_device
    from corpus.make_dataset import assemble_note_store
    from training.dataset import NoteClipStore
    table = ops.labels_table([[_note(60, 0.1, 0.2)]], CFG, 'cpu')
    assert table.n_files == 1 and table.n_notes == 1 and table.notes.numel() == 24
    with pytest.raises(HfttError):
        ops.labels_render(table, torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 8)
    with pytest.raises(HfttError):
        note2label_device(CFG, [_note(60, 0.1, 0.2)], False, 'cpu')
    cfg = {'feature': {'sr': 16000, 'hop_sample': 256, 'mel_bins': 4, 'log_offset': 1e-8}, 'input': {'margin_b': 2, 'margin_f': 2, 'num_frame': 4},
           'midi': {'note_min': 21, 'num_note': 6}}
    store = NoteClipStore(assemble_note_store([np.zeros((9, 4), np.float32)], [[_note(22, 0.02, 0.05)]], cfg), cfg, 'cpu')
    assert len(store) == 9
    with pytest.raises(HfttError):
        store.batch([0, 1])


def test_render_kernel_needs_no_scratch_and_runs_at_full_occupancy():
    '''the compiler's own resource remarks (hipcc cross-compiles without a GPU): both output forms without a partner (labels.hip:
    labels_render_kernel<true> and <false>), no scratch, eight waves per SIMD'''
    res = resources('labels.hip')
    both = [res['labels_render_kernel<true>'], res['labels_render_kernel<false>']]
    assert [get(v, 'ScratchSize') for v in both] == [0, 0]
    assert [get(v, 'Occupancy') for v in both] == [8, 8]
    assert all(get(v, 'VGPRs') <= 64 for v in both)
