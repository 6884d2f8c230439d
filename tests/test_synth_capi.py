"""C ABI and host half of the clip synth (hftt_clip_synth; hftt_hip.ops.VoiceBank / clip_synth / synth_span; corpus.synth_audio's
synth_voice_bank / pluck_voice; corpus.make_dataset.assemble_synth_store; training.dataset.SynthClipStore): the symbol, the descriptor layout
against the C compiler, every host-side refusal by status and message (they run before the device guard and the launch, so a box without a
GPU tests them), the compile remarks of the kernel, and the Python side's argument checks.  No compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import util
from hipcc_remarks import get, resources

HDR = os.path.join(util.ROOT, 'include', 'hftt_hip.h')


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('hftt_build', os.path.join(util.ROOT, 'nylon-amt_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    assert 'clip_synth.hip' in mod.SOURCES
    from hftt_hip import _capi
    return _capi.lib()


def test_the_symbol_is_exported_and_bound_at_abi_8(lib):
    from hftt_hip import _capi
    assert 'hftt_clip_synth' in _capi.SIGNATURES and hasattr(lib, 'hftt_clip_synth')
    assert lib.hftt_clip_synth.argtypes[0] is C.POINTER(_capi.ClipSynthDesc)
    hdr = open(HDR).read()
    assert re.search(r'\bint hftt_clip_synth\(const hftt_clip_synth_desc\* d, void\* stream\);', hdr)
    assert re.search(r'#define HFTT_ABI_VERSION 8\b', hdr) and lib.hftt_abi_version() == 8 == _capi.ABI_VERSION
    assert re.search(r'#define HFTT_SYNTH_MAX_PARTIALS %d\b' % _capi.SYNTH_MAX_PARTIALS, hdr) and _capi.SYNTH_MAX_PARTIALS == 32
    assert re.search(r'#define HFTT_SYNTH_CHUNK %d\b' % _capi.SYNTH_CHUNK, hdr) and _capi.SYNTH_CHUNK == 256


def test_descriptor_layout_matches_the_c_compiler(lib, tmp_path):
    """the new struct, and the existing ones it stands beside: nothing moved"""
    from hftt_hip import _capi
    pairs = [('hftt_clip_synth_desc', _capi.ClipSynthDesc), ('hftt_clip_room_desc', _capi.ClipRoomDesc), ('hftt_labels_desc', _capi.LabelsDesc),
             ('hftt_label_note', _capi.LabelNote), ('hftt_clip_logmel_desc', _capi.ClipLogmelDesc)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines += ['printf("HFTT_ABI_VERSION %d\\n", HFTT_ABI_VERSION);', 'return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n') if l)
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])
    assert int(got['HFTT_ABI_VERSION']) == 8
    assert [int(got[k]) for k in ('hftt_clip_logmel_desc', 'hftt_label_note', 'hftt_clip_room_desc')] == [160, 24, 232]      # as before the synth


P = 0x1000          # a non-null "device pointer": every case below is refused before anything dereferences it
PTRS = ('notes', 'row_ptr', 'file_nsamp', 'win_file', 'win_start', 'inc', 'amp', 'dec', 'vel_gain', 'rel', 'attack', 'release', 'voice_index',
        'out', 'out_samp0', 'out_win_file', 'out_win_start')
SPAN = (4 + 192 - 1) * 256 + 1024
SPAN3 = (4 + 3 + 192 - 1) * 256 + 1024


def _desc(**kw):
    from hftt_hip import _capi
    d = _capi.ClipSynthDesc()
    d.n_files, d.n_notes, d.B, d.width, d.N = 3, 100, 8, 192, 88
    d.n_fft, d.hop, d.lead, d.sr, d.V, d.H, d.span = 2048, 256, 0, 16000.0, 4, 16, SPAN
    for name in PTRS:
        setattr(d, name, P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BANK = b'null voice bank (inc / amp / dec / vel_gain / rel / attack / release)'
OUT = b'null output (out / out_samp0 / out_win_file / out_win_start)'
CASES = [({'notes': None}, b'notes is null at n_notes=100'), ({'row_ptr': None}, b'row_ptr is null'), ({'file_nsamp': None}, b'file_nsamp is null'),
         ({'win_file': None}, b'null window table'), ({'win_start': None}, b'null window table'), ({'voice_index': None}, b'voice_index is null')] + \
        [({n: None}, BANK) for n in ('inc', 'amp', 'dec', 'vel_gain', 'rel', 'attack', 'release')] + \
        [({n: None}, OUT) for n in ('out', 'out_samp0', 'out_win_file', 'out_win_start')] + \
        [({'n_fft': 1024}, b'n_fft=1024 unsupported (2048 only)'), ({'B': 0}, b'B=0'), ({'B': 1 << 30}, b'B=1073741824'), ({'width': 0}, b'width=0'),
         ({'hop': 0}, b'hop=0'), ({'n_files': 0}, b'n_files=0'), ({'n_notes': -1}, b'n_notes=-1 is negative'), ({'V': 0}, b'V=0'),
         ({'N': 0}, b'N=0 outside 1..128'), ({'N': 129}, b'N=129 outside 1..128'), ({'H': 0}, b'H=0 outside 1..32'), ({'H': 33}, b'H=33 outside 1..32'),
         ({'V': 1 << 20, 'N': 128, 'H': 32}, b'exceeds 2^31 entries'), ({'lead': -1}, b'lead=-1 is negative'), ({'sr': 0.0}, b'sr=0 must be positive'),
         ({'sr': -16000.0}, b'sr=-16000 must be positive'), ({'sr': float('nan')}, b'must be positive'), ({'sr': float('inf')}, b'must be positive'),
         ({'span': SPAN - 1}, b'span=%d below the %d samples' % (SPAN - 1, SPAN)), ({'lead': 3}, b'span=%d below the %d samples' % (SPAN, SPAN3)),
         ({'B': (1 << 30) - 1, 'width': 1 << 20, 'span': 1 << 40}, b'2^31 workgroups'),
         ({'lead': (1 << 31) - 1, 'width': (1 << 31) - 1, 'hop': (1 << 31) - 1, 'span': 1 << 62}, b'span=%d below the' % (1 << 62))]


@pytest.mark.parametrize('kw,msg', CASES, ids=['-'.join('%s=%s' % kv for kv in kw.items()) for kw, _ in CASES])
def test_clip_synth_refuses_before_any_launch(lib, kw, msg):
    d = _desc(**kw)
    assert lib.hftt_clip_synth(C.byref(d), None) == 1
    err = lib.hftt_last_error()
    assert err.startswith(b'clip_synth: ') and msg in err, err


def test_a_null_descriptor_is_refused_and_a_table_without_notes_needs_no_records(lib):
    assert lib.hftt_clip_synth(None, None) == 1 and b'clip_synth: null descriptor' in lib.hftt_last_error()
    d = _desc(notes=None, n_notes=0, width=0)               # notes may be null at n_notes == 0: the call gets past it, to the next refusal
    assert lib.hftt_clip_synth(C.byref(d), None) == 1 and b'width=0' in lib.hftt_last_error()


def test_the_synth_kernel_needs_no_scratch_and_no_spill():
    """clip_synth.hip: one kernel; no scratch, no register spilled to memory, at least four waves per SIMD; the bank is read with scalar loads
    inside the partial loop (the survivor's fields go through readfirstlane)"""
    res = resources('clip_synth.hip')
    assert sorted(res) == ['clip_synth_kernel']
    v = res['clip_synth_kernel']
    assert get(v, 'ScratchSize') == 0 and get(v, 'VGPRs Spill') == 0 and get(v, 'Occupancy') >= 4, v
    print('clip_synth.hip: VGPRs %s, occupancy %s, LDS %s' % tuple(get(v, k) for k in ('VGPRs', 'Occupancy', 'LDS Size')))
    src = re.sub(r'//[^\n]*', '', open(os.path.join(util.ROOT, 'nylon-amt_amd', 'csrc', 'clip_synth.hip')).read())
    assert '#include "clip_synth_fn.h"' in src and 'synth_sin_turns(' in src and 'synth_exp2(' in src and '#include "block_scan.h"' in src
    assert not re.search(r'atomic|sinf\(|expf\(|exp2f\(|__sinf|__expf', src)        # the two functions come from the one header, nothing else


def _bank(V=2, N=5, H=3):
    return {'inc': np.full((V, N, H), 1 << 31, np.uint32), 'amp': np.ones((V, N, H), np.float32), 'dec': np.zeros((V, N, H), np.float32),
            'vel_gain': np.ones((V, 128), np.float32), 'rel': np.zeros(V, np.float32), 'attack': np.ones(V, np.int32), 'release': np.zeros(V, np.int32)}


def test_voice_bank_refusals():
    from hftt_hip import HfttError, ops
    vb = ops.VoiceBank(device='cpu', **_bank())
    assert (vb.V, vb.N, vb.H) == (2, 5, 3) and vb.inc.dtype == torch.int32 and int(vb.inc[0, 0, 0]) == -(1 << 31) and vb.amp.dtype == torch.float32
    assert vb.nbytes() == 3 * 2 * 5 * 3 * 4 + 2 * 128 * 4 + 3 * 2 * 4
    assert ops.VoiceBank(device='cpu', **dict(_bank(), inc=torch.full((2, 5, 3), (1 << 32) - 1, dtype=torch.int64))).inc[0, 0, 0] == -1

    def bad(match, **kw):
        with pytest.raises(HfttError, match=match):
            ops.VoiceBank(device='cpu', **dict(_bank(), **kw))
    bad('amp must be', amp=np.ones((2, 5), np.float32))
    bad('amp must be', **_bank(H=33))
    bad('amp must be', **_bank(N=129))
    bad('inc must have shape', inc=np.zeros((2, 5, 4), np.uint32))
    bad('vel_gain must have shape', vel_gain=np.ones((2, 127), np.float32))
    bad('rel must have shape', rel=np.zeros(3, np.float32))
    bad('attack must have shape', attack=np.ones(1, np.int32))
    bad('amp must be finite', amp=np.full((2, 5, 3), np.inf, np.float32))
    bad('dec must be finite', dec=np.full((2, 5, 3), np.nan, np.float32))
    bad('amp must be finite floating point', amp=np.ones((2, 5, 3), np.int32))
    bad('dec must not be negative', dec=np.full((2, 5, 3), -1e-3, np.float32))
    bad('rel must not be negative', rel=np.full(2, -1.0, np.float32))
    bad('inc must be integers', inc=np.ones((2, 5, 3), np.float32))
    bad('inc must be integers', inc=np.full((2, 5, 3), -1, np.int64))
    bad('inc must be integers', inc=np.full((2, 5, 3), 1 << 32, np.int64))
    bad('attack must be integers inside 1', attack=np.zeros(2, np.int32))
    bad('release must be integers inside 0', release=np.full(2, -1, np.int32))


def test_python_entry_points_refuse_cpu_tensors_and_wrong_arguments():
    import synth_emul as S
    from hftt_hip import HfttError, ops
    table = ops.LabelsTable(ops.labels_table_host([[S.note(22, 0.1, 0.2)], []], S.config(5)), 'cpu')
    vb = ops.VoiceBank(device='cpu', **_bank())
    nsamp = torch.tensor([4000, 0])
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.clip_synth(table, nsamp, vb, [0], [0], [0], 16, 256, 16000.0)
    with pytest.raises(HfttError, match='table must be an ops.LabelsTable'):
        ops.clip_synth(None, nsamp, vb, [0], [0], [0], 16, 256, 16000.0)
    with pytest.raises(HfttError, match='bank must be an ops.VoiceBank'):
        ops.clip_synth(table, nsamp, _bank(), [0], [0], [0], 16, 256, 16000.0)
    with pytest.raises(HfttError, match=r'the bank holds N=6 pitches, the note table N=5'):
        ops.clip_synth(table, nsamp, ops.VoiceBank(device='cpu', **_bank(N=6)), [0], [0], [0], 16, 256, 16000.0)
    with pytest.raises(HfttError, match=r'file_nsamp must be \[n_files=2\]'):
        ops.clip_synth(table, nsamp[:1], vb, [0], [0], [0], 16, 256, 16000.0)
    with pytest.raises(HfttError, match='must be \\[B\\]'):
        ops.clip_synth(table, nsamp, vb, [0, 1], [0], [0], 16, 256, 16000.0)
    assert ops.synth_span(192, 256) == SPAN == ops.room_span(192, 256) and ops.synth_span(192, 256, 3) == SPAN3 and ops.synth_span(16, 256, 3) == 3 * 2048 + 512


def test_synth_voice_bank_and_pluck_voice():
    from corpus import synth_audio as SA
    from hftt_hip import ops
    config = SA.default_config()
    a, b, c = SA.synth_voice_bank(5, config, seed=3), SA.synth_voice_bank(5, config, seed=3), SA.synth_voice_bank(5, config, seed=4)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a['amp'], c['amp'])
    assert a['inc'].dtype == np.uint32 and a['inc'].shape == a['amp'].shape == a['dec'].shape == (5, 88, 16) and a['vel_gain'].shape == (5, 128)
    ops.VoiceBank(device='cpu', **a)                        # it passes the bank's own checks
    f0 = 440.0 * 2.0 ** ((21 + np.arange(88) - 69) / 12.0)
    freq = a['inc'].astype(np.float64) / 2.0 ** 32 * 16000.0
    on = a['amp'] > 0
    # the fundamental within a few cents of the pitch (detune < 50 cents and a small inharmonicity), partials stretched upwards, Nyquist respected
    cents = 1200.0 * np.log2(freq[:, :, 0] / f0[None, :])
    assert (np.abs(cents) < 10.0).all() and (freq[on] < 8000.0).all() and not a['amp'][freq == 0].any() and (freq[~on] == 0).all()
    k = np.arange(1, 17)
    ratio = freq / (k[None, None, :] * f0[None, :, None])
    assert (ratio[on] > 0.99).all() and (ratio[on] < 1.06).all()
    assert (a['amp'] >= 0).all() and np.allclose(a['amp'].max(axis=2), a['amp'].max(axis=2)[:, :1]) and (a['amp'].max() <= 0.12 + 1e-6) and (a['amp'].max(axis=2) >= 0.03 - 1e-6).all()
    assert (a['dec'] > 0).all() and (np.diff(a['dec'], axis=2) > 0).all()              # higher partials decay faster
    assert (a['vel_gain'][:, 0] == 0).all() and np.allclose(a['vel_gain'][:, 127], 1.0) and (np.diff(a['vel_gain'], axis=1) > 0).all()
    assert (a['attack'] >= 1).all() and (a['release'] >= 1).all() and (a['rel'] > 0).all()
    for bad in (dict(n=0), dict(partials=0), dict(detune_cents=50.0)):
        with pytest.raises(ValueError):
            SA.synth_voice_bank(**dict(dict(n=2, config=config, seed=0), **bad))
    p = SA.pluck_voice(config)
    assert p['amp'].shape == (1, 88, 3) and p['release'][0] == 4800 and p['attack'][0] == 1 and p['rel'][0] == 0
    assert np.allclose(p['amp'][0, 0], [0.1, 0.05, 0.025]) and np.allclose(p['dec'] * 16000.0 / np.log2(np.e), 3.0) and np.allclose(p['vel_gain'][0, 64], 64 / 127.0)
    hi = p['inc'][0, 87].astype(np.float64) / 2.0 ** 32 * 16000.0                      # C8 = 4,186 Hz: its second and third partial lie above Nyquist
    assert abs(hi[0] - 4186.009) < 0.01 and hi[1] == 0 and hi[2] == 0 and p['amp'][0, 87].tolist() == [np.float32(0.1), 0.0, 0.0]
    ops.VoiceBank(device='cpu', **p)


def test_assemble_synth_store_and_a_file_without_notes():
    import synth_emul as S
    from corpus.make_dataset import assemble_synth_store, assemble_wave_store
    config = S.config(5)
    notes = [[S.note(22, 0.1, 0.5), S.note(25, 0.0, 0.2001)], [], [S.note(21, 0.0, 1.0)]]
    st = assemble_synth_store(notes, config, release_samples=300)
    assert st['file_nsamp'].dtype == np.int64 and st['file_nsamp'].tolist() == [8000 + 300, 300, 16000 + 300]
    assert st['table']['file_nframe'].tolist() == [int(0.5 * 62.5 + 0.5) + 1, 1, 63 + 1]
    nf = [max(1 + n // 256, f) for n, f in zip(st['file_nsamp'], st['table']['file_nframe'])]
    assert np.bincount(st['clip_file']).tolist() == nf and st['clip_frame'][:3].tolist() == [0, 1, 2] and st['clip_frame'][nf[0]] == 0
    # the clips are those of a wave store of files that long
    ws = assemble_wave_store([np.zeros(n, np.float32) for n in st['file_nsamp']], notes, config)
    assert np.array_equal(ws['clip_file'], st['clip_file']) and np.array_equal(ws['clip_frame'], st['clip_frame'])
    assert assemble_synth_store([[]], config)['file_nsamp'].tolist() == [0]
    with pytest.raises(ValueError):
        assemble_synth_store(notes, config, release_samples=-1)


def test_synth_clip_store_argument_errors():
    """everything SynthClipStore refuses in front of its first upload"""
    import synth_emul as S
    from corpus.make_dataset import assemble_synth_store
    from hftt_hip import HfttError, ops
    from training.dataset import SynthClipStore, WaveAugment
    config = S.config(5)
    store = assemble_synth_store([[S.note(22, 0.1, 0.5)]], config, 0)
    vb = ops.VoiceBank(device='cpu', **_bank())
    with pytest.raises(HfttError, match='bank must be an ops.VoiceBank'):
        SynthClipStore(store, config, 'cpu', _bank())
    with pytest.raises(HfttError, match='augment must be a WaveAugment'):
        SynthClipStore(store, config, 'cpu', vb, augment=object())
    for bad in (dict(pitch_semitones=(-1, 1)), dict(detune_cents=5.0), dict(shift=True), dict(mix_p=0.25)):
        with pytest.raises(HfttError, match='warps or mixes'):
            SynthClipStore(store, config, 'cpu', vb, augment=WaveAugment(**bad))
    with pytest.raises(HfttError, match='max_value'):
        SynthClipStore(store, dict(config, input=dict(config['input'], max_value=1.0)), 'cpu', vb)
    with pytest.raises(HfttError, match='the bank holds N=6 pitches, the config num_note=5'):
        SynthClipStore(store, config, 'cpu', ops.VoiceBank(device='cpu', **_bank(N=6)))
    with pytest.raises(HfttError, match='the bank lives on'):
        SynthClipStore(store, config, 'meta', vb)


def test_trainer_refuses_the_synth_store_next_to_another_store():
    tool = os.path.join(util.ROOT, 'tools', 'train_config5.py')
    cases = ((['--synth-store', '--wave-store'], 'exclusive'), (['--synth-store', '--note-store'], 'exclusive'), (['--synth-voices', '4'], 'they need --synth-store'),
             (['--synth-store', '--aug-mix-p', '0.5'], 'warps or mixes'))
    procs = [subprocess.Popen([sys.executable, tool] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for extra, _ in cases]
    for (extra, msg), p in zip(cases, procs):               # (side by side: each run is the interpreter's start-up and the parser)
        _, err = p.communicate(timeout=300)
        assert p.returncode == 2 and msg in err, (extra, err[-500:])
