"""C ABI and host half of the clip log-mel (hftt_clip_logmel, hftt_hip.ops.WaveTable, corpus.make_dataset.assemble_wave_store): the symbol, the
descriptor layout against the C compiler, every host-side refusal (they run before the device guard and the launch, so a box without a GPU tests
them), the kernel's compile remarks, and the wave store's clip list against the note store's.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

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
    from hftt_hip import _capi
    return _capi.lib()


def test_symbol_is_exported_and_bound_at_abi_8(lib):
    from hftt_hip import _capi
    assert 'hftt_clip_logmel' in _capi.SIGNATURES and hasattr(lib, 'hftt_clip_logmel')
    assert lib.hftt_clip_logmel.argtypes[0] is C.POINTER(_capi.ClipLogmelDesc)
    assert lib.hftt_abi_version() == 8 == _capi.ABI_VERSION
    assert re.search(r'\bint hftt_clip_logmel\(const hftt_clip_logmel_desc\* d, void\* stream\);', open(HDR).read())


def test_descriptor_layout_matches_the_c_compiler(lib, tmp_path):
    from hftt_hip import _capi
    cname, cls = 'hftt_clip_logmel_desc', _capi.ClipLogmelDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {',
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines += ['printf("HFTT_CLIP_LOGMEL_RUN %d\\n", HFTT_CLIP_LOGMEL_RUN);', 'printf("HFTT_CLIP_LOGMEL_MAX_MELS %d\\n", HFTT_CLIP_LOGMEL_MAX_MELS);',
              'printf("HFTT_ABI_VERSION %d\\n", HFTT_ABI_VERSION);', 'return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')
    got = dict(l.split() for l in out if l)
    assert int(got[cname]) == C.sizeof(cls)
    for f in cls._fields_:
        assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]
    assert int(got['HFTT_CLIP_LOGMEL_RUN']) == _capi.CLIP_LOGMEL_RUN and int(got['HFTT_CLIP_LOGMEL_MAX_MELS']) == _capi.CLIP_LOGMEL_MAX_MELS
    assert int(got['HFTT_ABI_VERSION']) == 8 == lib.hftt_abi_version()          # the symbol was added AT version 8


P = 0x1000          # a non-null "device pointer": every case below is refused before anything dereferences it
POINTERS = ('wave', 'file_samp0', 'win_file', 'win_start', 'window', 'twiddle', 'fb_start', 'fb_len', 'fb_off', 'fb_w', 'out')


def _desc(**kw):
    from hftt_hip import _capi
    d = _capi.ClipLogmelDesc()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.width = 100000, 1, 3, 8, 192
    d.n_fft, d.hop, d.n_mels, d.log_offset, d.fill = 2048, 256, 256, 1e-8, -18.420681
    for name in POINTERS:
        setattr(d, name, P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REJECTS = [({'wave': None}, b'wave is null'), ({'file_samp0': None}, b'file_samp0 is null'),
           ({'win_file': None}, b'null window table'), ({'win_start': None}, b'null window table'),
           ({'window': None}, b'null table (window'), ({'twiddle': None}, b'/ twiddle'), ({'fb_start': None}, b'/ fb_start'),
           ({'fb_len': None}, b'/ fb_len'), ({'fb_off': None}, b'/ fb_off'), ({'fb_w': None}, b'/ fb_w'), ({'out': None}, b'out is null'),
           ({'wave_i16': 2}, b'wave_i16=2'), ({'wave_i16': -1}, b'wave_i16=-1'),
           ({'n_fft': 1024}, b'n_fft=1024 unsupported (2048 only)'), ({'n_fft': 4096}, b'n_fft=4096'), ({'n_fft': 0}, b'n_fft=0'),
           ({'B': 0}, b'B=0'), ({'B': -1}, b'B=-1'), ({'width': 0}, b'width=0'), ({'width': -7}, b'width=-7'),
           ({'n_mels': 0}, b'n_mels=0'), ({'n_mels': 257}, b'n_mels=257 outside 1..256'), ({'hop': 0}, b'hop=0'), ({'hop': -256}, b'hop=-256'),
           ({'hop': 325}, b'hop=325'), ({'n_files': 0}, b'n_files=0'), ({'n_files': -1}, b'n_files=-1'), ({'total_samples': -1}, b'total_samples=-1'),
           ({'B': 1 << 30, 'width': 17}, b'2^31 workgroups')]


@pytest.mark.parametrize('kw,msg', REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in REJECTS])
def test_clip_logmel_rejects_before_any_launch(lib, kw, msg):
    d = _desc(**kw)
    assert lib.hftt_clip_logmel(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'clip_logmel: ') and msg in err, err


def test_clip_logmel_rejects_a_null_descriptor(lib):
    assert lib.hftt_clip_logmel(None, None) not in (0, 2, 3) and b'null descriptor' in lib.hftt_last_error()


def test_kernel_needs_no_scratch_and_stays_inside_64_kb_of_lds():
    '''the compiler's own resource remarks (hipcc cross-compiles without a GPU) for every kernel of clip_logmel.hip: no scratch, and the static
    LDS plus the staged samples of the largest hop the host admits (and of the paper's hop 256) within 65,536 bytes'''
    from hftt_hip import _capi
    res = resources('clip_logmel.hip')
    kernels = list(res)
    assert len(kernels) >= 1 and all('clip_logmel_kernel' in k for k in kernels), kernels
    assert [get(v, 'ScratchSize') for v in res.values()] == [0] * len(kernels)
    assert [get(v, 'VGPRs Spill') for v in res.values()] == [0] * len(kernels)
    lds = [get(v, 'LDS Size') for v in res.values()]
    staged = lambda hop: ((_capi.CLIP_LOGMEL_RUN - 1) * hop + 2048) * 4
    for static in lds:
        assert static + staged(256) <= 65536 and static + staged(324) <= 65536 < static + staged(325), (static, staged(324))
    print('clip_logmel.hip: %s, static LDS %s B + %d B staged at hop 256' % (kernels, lds, staged(256)))


def _note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


CFG = {'feature': {'sr': 16000, 'hop_sample': 256, 'mel_bins': 4, 'log_offset': 1e-8}, 'input': {'margin_b': 2, 'margin_f': 2, 'num_frame': 4},
       'midi': {'note_min': 21, 'num_note': 6}}


def test_assemble_wave_store_lists_the_clips_of_the_note_store():
    """three tiny files: one longer than its notes, one whose label track is longer than its audio, one without notes"""
    from corpus.make_dataset import assemble_note_store, assemble_wave_store
    rng = np.random.RandomState(3)
    waves = [rng.randn(1000).astype(np.float32) * 0.1, (rng.randn(300) * 3000).astype(np.int16), np.zeros(255, np.float32)]
    notes = [[_note(22, 0.01, 0.03)], [_note(23, 0.0, 0.09), _note(21, 0.02, 0.05)], []]
    ws = assemble_wave_store(waves, notes, CFG)
    assert ws['file_nsamp'].tolist() == [1000, 300, 255] and ws['file_nsamp'].dtype == np.int64
    assert all(w is v for w, v in zip(ws['waves'], waves))                       # the samples as given
    feats = [np.zeros((1 + len(w) // 256, 4), np.float32) for w in waves]        # what the front end makes of them: 1 + n // hop frames
    ns = assemble_note_store(feats, notes, CFG)
    nf = [max(1 + 1000 // 256, 3), max(1 + 300 // 256, int(0.09 * 62.5 + 0.5) + 1), 1]
    assert nf == [4, 7, 1]
    assert ws['clip_file'].tolist() == [0] * 4 + [1] * 7 + [2] and ws['clip_frame'].tolist() == list(range(4)) + list(range(7)) + [0]
    assert ws['clip_file'].dtype == ws['clip_frame'].dtype == np.int32 and len(ws['clip_file']) == len(ns['idx'])
    # the note store's idx is the same list in store rows: row = file_row0[file] + frame
    assert (ns['file_row0'][ws['clip_file']] + ws['clip_frame']).tolist() == ns['idx'].tolist()
    for k in ('notes', 'row_ptr', 'file_nframe'):
        assert np.array_equal(ws['table'][k], ns['table'][k]), k
    with pytest.raises(ValueError):
        assemble_wave_store(waves[:2], notes, CFG)


def test_wave_table_layout_and_dtypes():
    from hftt_hip import HfttError, ops
    waves = [np.array([0.5, -1.0, 1.0, 1e-5], np.float32), np.zeros(0, np.float32), np.array([-32768, 32767, 3], np.int16)]
    t = ops.WaveTable(waves, 'cpu', dtype='int16')
    assert t.wave.dtype == torch.int16 and t.wave.tolist() == [16384, -32768, 32767, 0, -32768, 32767, 3]
    assert t.file_samp0.dtype == torch.int64 and t.file_samp0.tolist() == [0, 4, 4, 7] and (t.n_files, t.total_samples) == (3, 7)
    assert t.nbytes() == 7 * 2 + 4 * 8
    f = ops.WaveTable(waves, 'cpu', dtype='float32')
    assert f.wave.dtype == torch.float32 and f.wave.tolist()[4:] == [-1.0, 32767 / 32768, 3 / 32768]
    for bad, what in (((waves, 'cpu', 'int8'), 'dtype'), (([], 'cpu'), 'no files'), (([np.zeros((2, 2), np.float32)], 'cpu'), '1-d'),
                      (([np.zeros(3, np.int32)], 'cpu'), 'int16 or floating')):
        with pytest.raises(HfttError, match=what):
            ops.WaveTable(*bad)


def test_python_entry_points_refuse_cpu_tensors_and_scaled_features():
    from hftt_hip import HfttError, ops
    from corpus.make_dataset import assemble_wave_store
    from training.dataset import WaveAugment, WaveClipStore
    cfg = {'feature': dict(CFG['feature'], fft_bins=2048), 'input': dict(CFG['input'], min_value=-18.420681), 'midi': CFG['midi']}
    store = assemble_wave_store([np.zeros(600, np.float32)], [[_note(22, 0.02, 0.05)]], cfg)
    with pytest.raises(HfttError):                      # no CPU fallback: the device tables are refused off the device
        WaveClipStore(store, cfg, 'cpu')
    with pytest.raises(HfttError, match='max_value'):
        WaveClipStore(store, {**cfg, 'input': dict(cfg['input'], max_value=6.0)}, 'cpu')
    with pytest.raises(HfttError, match='gain_db'):
        WaveAugment(gain_db=(3.0, -3.0))

    class Tables:                                       # an ops.LogMel that was never uploaded
        device = torch.device('cpu')
        n_fft, hop, n_mels, log_offset = 2048, 256, 4, 1e-8
        window = twiddle = fb_start = fb_len = fb_off = fb_w = torch.zeros(1)
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.clip_logmel(ops.WaveTable(store['waves'], 'cpu'), Tables, [0], [0], 8, -18.0)
