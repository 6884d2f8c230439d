"""C ABI and host half of the warp (hftt_wave_warp, hftt_clip_logmel_warp, hftt_labels_render_warp; hftt_hip.ops.Warp / WarpTable; the warp draws
of training.dataset.WaveAugment): the symbols, the descriptor layouts against the C compiler, every host-side refusal by message (they run
before the device guard and the launch, so a box without a GPU tests them), the compile remarks of the warped clip_logmel_kernel,
and the host tables.  No compute calls."""
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
ENTRIES = {'hftt_wave_warp': 'WaveWarpDesc', 'hftt_clip_logmel_warp': 'ClipLogmelWarpDesc', 'hftt_labels_render_warp': 'LabelsWarpDesc'}


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
    hdr = open(HDR).read()
    for name, cls in ENTRIES.items():
        assert name in _capi.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes[0] is C.POINTER(getattr(_capi, cls))
        cname = name + '_desc' if name != 'hftt_labels_render_warp' else 'hftt_labels_warp_desc'
        assert re.search(r'\bint %s\(const %s\* d, void\* stream\);' % (name, cname), hdr), name
    assert lib.hftt_abi_version() == 8 == _capi.ABI_VERSION


def test_descriptor_layouts_match_the_c_compiler(lib, tmp_path):
    from hftt_hip import _capi
    pairs = [('hftt_warp_args', _capi.WarpArgs), ('hftt_wave_warp_desc', _capi.WaveWarpDesc), ('hftt_clip_logmel_warp_desc', _capi.ClipLogmelWarpDesc),
             ('hftt_labels_warp_desc', _capi.LabelsWarpDesc), ('hftt_clip_logmel_desc', _capi.ClipLogmelDesc), ('hftt_labels_desc', _capi.LabelsDesc)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for m in ('HFTT_WARP_ZEROS', 'HFTT_WARP_TABLE_L', 'HFTT_WARP_TABLE_LEN', 'HFTT_WARP_STEP_MIN', 'HFTT_WARP_STEP_MAX', 'HFTT_ABI_VERSION'):
        lines.append('printf("%s %%d\\n", %s);' % (m, m))
    lines += ['printf("HFTT_WARP_DELAY_MAX %lld\\n", (long long)HFTT_WARP_DELAY_MAX);', 'return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n') if l)
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])
    assert (int(got['HFTT_WARP_ZEROS']), int(got['HFTT_WARP_TABLE_L']), int(got['HFTT_WARP_TABLE_LEN'])) == (_capi.WARP_ZEROS, _capi.WARP_TABLE_L, _capi.WARP_TABLE_LEN)
    assert (int(got['HFTT_WARP_STEP_MIN']), int(got['HFTT_WARP_STEP_MAX']), int(got['HFTT_WARP_DELAY_MAX'])) == (_capi.WARP_STEP_MIN, _capi.WARP_STEP_MAX, _capi.WARP_DELAY_MAX)
    assert int(got['HFTT_ABI_VERSION']) == 8 == lib.hftt_abi_version()          # the symbols were added AT version 8


P = 0x1000          # a non-null "device pointer": every case below is refused before anything dereferences it
WARP_PTRS = ('step_q24', 'delay_q24', 'cut', 'proto')


def _set(d, kw):
    for k, v in kw.items():
        tgt = d
        *path, leaf = k.split('.')
        for p in path:
            tgt = getattr(tgt, p)
        setattr(tgt, leaf, v)


def _warp_args(d):
    for name in WARP_PTRS:
        _set(d, {'warp.' + name: P})


def _wave_desc(**kw):
    from hftt_hip import _capi
    d = _capi.WaveWarpDesc()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.len = 100000, 1, 3, 8, 4096
    for name in ('wave', 'file_samp0', 'win_file', 'win_start', 'out'):
        setattr(d, name, P)
    _warp_args(d)
    _set(d, kw)
    return d


WAVE_REJECTS = [({'wave': None}, b'wave is null'), ({'file_samp0': None}, b'file_samp0 is null'), ({'win_file': None}, b'null window table'),
                ({'win_start': None}, b'null window table'), ({'out': None}, b'out is null')] + \
               [({'warp.' + n: None}, b'null warp table (step_q24 / delay_q24 / cut / proto)') for n in WARP_PTRS] + \
               [({'wave_i16': 2}, b'wave_i16=2'), ({'B': 0}, b'B=0'), ({'len': 0}, b'len=0'), ({'len': -3}, b'len=-3'), ({'n_files': 0}, b'n_files=0'),
                ({'total_samples': -1}, b'total_samples=-1 outside'), ({'total_samples': (1 << 38) + 1}, b'outside 0 .. 2^38'),
                ({'B': 1 << 30, 'len': 257}, b'2^31 workgroups')]


@pytest.mark.parametrize('kw,msg', WAVE_REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in WAVE_REJECTS])
def test_wave_warp_rejects_before_any_launch(lib, kw, msg):
    d = _wave_desc(**kw)
    assert lib.hftt_wave_warp(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'wave_warp: ') and msg in err, err


def _clip_desc(**kw):
    from hftt_hip import _capi
    d = _capi.ClipLogmelWarpDesc()
    b = d.base
    b.total_samples, b.wave_i16, b.n_files, b.B, b.width = 100000, 1, 3, 8, 192
    b.n_fft, b.hop, b.n_mels, b.log_offset, b.fill = 2048, 256, 256, 1e-8, -18.420681
    for name in ('wave', 'file_samp0', 'win_file', 'win_start', 'window', 'twiddle', 'fb_start', 'fb_len', 'fb_off', 'fb_w', 'out'):
        setattr(b, name, P)
    _warp_args(d)
    _set(d, kw)
    return d


CLIP_REJECTS = [({'base.wave': None}, b'wave is null'), ({'base.file_samp0': None}, b'file_samp0 is null'), ({'base.win_file': None}, b'null window table'),
                ({'base.win_start': None}, b'null window table'), ({'base.fb_start': None}, b'/ fb_start'), ({'base.out': None}, b'out is null'),
                ({'base.wave_i16': 2}, b'wave_i16=2'), ({'base.n_fft': 1024}, b'n_fft=1024 unsupported (2048 only)'), ({'base.B': 0}, b'B=0'),
                ({'base.width': 0}, b'width=0'), ({'base.n_mels': 257}, b'n_mels=257 outside 1..256'), ({'base.hop': 0}, b'hop=0'),
                ({'base.hop': 325}, b'hop=325'), ({'base.n_files': 0}, b'n_files=0'), ({'base.total_samples': -1}, b'total_samples=-1'),
                ({'base.B': 1 << 30, 'base.width': 17}, b'2^31 workgroups'), ({'base.total_samples': (1 << 38) + 1}, b'beyond 2^38')] + \
               [({'warp.' + n: None}, b'null warp table (step_q24 / delay_q24 / cut / proto)') for n in WARP_PTRS]


@pytest.mark.parametrize('kw,msg', CLIP_REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in CLIP_REJECTS])
def test_clip_logmel_warp_rejects_before_any_launch(lib, kw, msg):
    d = _clip_desc(**kw)
    assert lib.hftt_clip_logmel_warp(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'clip_logmel: ') and msg in err, err


def _labels_desc(**kw):
    from hftt_hip import _capi
    d = _capi.LabelsWarpDesc()
    b = d.base
    b.n_files, b.n_notes, b.B, b.len, b.N, b.tol, b.duration_tolerance, b.form = 3, 10, 4, 128, 88, 3, 0, 0
    b.hop_ms, b.fps = 16.0, 62.5
    for name in ('notes', 'row_ptr', 'win_file', 'win_start', 'onset', 'offset', 'mpe', 'velocity'):
        setattr(b, name, P)                 # (file_nframe stays NULL: the warped render does not read it)
    for name in ('shift', 't_delay', 't_scale', 'file_end_sec'):
        setattr(d, name, P)
    _set(d, kw)
    return d


LABELS_REJECTS = [({'base.n_files': 0}, b'n_files=0'), ({'base.n_notes': -1}, b'n_notes=-1'), ({'base.B': 0}, b'B=0'), ({'base.len': 0}, b'len=0'),
                  ({'base.N': 129}, b'N=129 outside 1..128'), ({'base.tol': 0}, b'tol=0'), ({'base.hop_ms': 0.0}, b'hop_ms=0'),
                  ({'base.duration_tolerance': 2}, b'duration_tolerance=2'), ({'base.form': 2}, b'form=2'), ({'base.notes': None}, b'notes is null'),
                  ({'base.row_ptr': None}, b'row_ptr is null'), ({'base.win_file': None}, b'win_file is null'), ({'base.win_start': None}, b'win_start is null'),
                  ({'base.onset': None}, b'null output'), ({'base.B': 1 << 20, 'base.len': 1 << 10, 'base.N': 88}, b'2^31 elements')] + \
                 [({n: None}, b'null warp table (shift / t_delay / t_scale / file_end_sec)') for n in ('shift', 't_delay', 't_scale', 'file_end_sec')]


@pytest.mark.parametrize('kw,msg', LABELS_REJECTS, ids=['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in LABELS_REJECTS])
def test_labels_render_warp_rejects_before_any_launch(lib, kw, msg):
    d = _labels_desc(**kw)
    assert lib.hftt_labels_render_warp(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'labels_render: ') and msg in err, err


def test_null_descriptors_and_the_unwarped_file_nframe(lib):
    from hftt_hip import _capi
    for name in ENTRIES:
        assert getattr(lib, name)(None, None) not in (0, 2, 3) and b'null descriptor' in lib.hftt_last_error()
    d = _labels_desc()                      # the unwarped entry point still needs file_nframe
    assert lib.hftt_labels_render(C.byref(d.base), None) not in (0, 2, 3) and b'file_nframe is null' in lib.hftt_last_error()


def test_both_instantiations_need_no_scratch_and_stay_inside_64_kb_of_lds():
    """the compiler's resource remarks for the unwarped and the warped staging loop (clip_logmel.hip: clip_logmel_kernel<2048, false> and
    <2048, true>): neither with scratch or spills, both with the static LDS that admits hop 324 and not 325"""
    from hftt_hip import _capi
    res = resources('clip_logmel.hip')
    both = [res['clip_logmel_kernel<2048, false>'], res['clip_logmel_kernel<2048, true>']]
    assert [get(v, 'ScratchSize') for v in both] == [0, 0]
    assert [get(v, 'VGPRs Spill') for v in both] == [0, 0]
    lds = [get(v, 'LDS Size') for v in both]
    staged = lambda hop: ((_capi.CLIP_LOGMEL_RUN - 1) * hop + 2048) * 4
    assert lds[0] == lds[1] and lds[0] + staged(324) <= 65536 < lds[0] + staged(325), lds
    print('clip_logmel.hip: unwarped / warped VGPRs %s' % [get(v, 'VGPRs') for v in both])


def _note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


CFG = {'feature': {'sr': 16000, 'hop_sample': 256}, 'midi': {'note_min': 21, 'num_note': 88}}


def test_labels_table_gains_the_warp_columns():
    from hftt_hip import ops
    t = ops.labels_table_host([[_note(30, 0.1, 0.5), _note(90, 0.0, 0.7), _note(60, 0.2, 0.3)], [], [_note(21, 0.0, 0.0), _note(108, 0.0, 0.25)]], CFG)
    assert t['file_end_sec'].dtype == np.float64 and t['file_end_sec'].tolist() == [0.7, 0.0, 0.25]
    assert t['pitch_min'].dtype == t['pitch_max'].dtype == np.int32
    assert t['pitch_min'].tolist() == [9, 87, 0] and t['pitch_max'].tolist() == [69, 0, 87] and t['sr'] == 16000
    tab = ops.LabelsTable(t, 'cpu')
    assert tab.file_end_sec.dtype == torch.float64 and tab.pitch_min.tolist() == [9, 87, 0]
    old = {k: v for k, v in t.items() if k not in ('file_end_sec', 'pitch_min', 'pitch_max', 'sr')}
    with pytest.raises(ops.HfttError, match='file_end_sec'):            # a host table from before the columns existed renders unwarped only
        ops.labels_render(ops.LabelsTable(old, 'cpu'), [0], [0], 8, warp=ops.Warp(torch.tensor([1 << 24]), torch.tensor([0])))


def test_warp_derives_cut_and_the_time_map_in_one_place():
    from hftt_hip import ops
    import warp_emul as W
    steps = [W.step_of(1.0), W.step_of(-1.7), 1 << 23, 1 << 25, 1 << 24]
    delays = [0, int(0.37 * W.ONE), 255 << 24, 7, (1 << 24) * 100]
    w = ops.Warp(torch.tensor(steps), torch.tensor(delays))
    assert w.step_q24.dtype == torch.int32 and w.delay_q24.dtype == torch.int64 and w.shift.dtype == torch.int32 and not bool(w.shift.any())
    assert w.cut().dtype == torch.float32 and w.cut().tolist() == [float(W.cut_of(s)) for s in steps]
    assert w.t_scale().dtype == torch.float64 and w.t_scale().tolist() == [W.t_scale_of(s) for s in steps]
    assert w.t_delay(16000).tolist() == [W.t_delay_of(d, 16000) for d in delays]
    with pytest.raises(ops.HfttError, match=r'must be \[B\]'):
        ops.Warp(torch.tensor(steps), torch.tensor(delays[:2]))
    with pytest.raises(ops.HfttError, match=r'must be \[B\]'):
        ops.Warp(torch.tensor(steps), torch.tensor(delays), shift=torch.zeros(3))


def test_python_entry_points_refuse_cpu_tensors_and_wrong_warps():
    from hftt_hip import HfttError, ops
    waves = ops.WaveTable([np.zeros(600, np.float32)], 'cpu', 'float32')
    w = ops.Warp(torch.tensor([1 << 24]), torch.tensor([0]))
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.wave_warp(waves, [0], [0], 16, w)
    with pytest.raises(HfttError, match='must be an ops.Warp'):
        ops.wave_warp(waves, [0], [0], 16, (1 << 24, 0))
    with pytest.raises(HfttError, match='holds 1 windows'):
        ops.wave_warp(waves, [0, 0], [0, 5], 16, w)
    with pytest.raises(HfttError, match=r'must be \[B\]'):
        ops.wave_warp(waves, [0], [0, 1], 16, w)

    class Tables:                                       # an ops.LogMel that was never uploaded
        device = torch.device('cpu')
        n_fft, hop, n_mels, log_offset = 2048, 256, 4, 1e-8
        window = twiddle = fb_start = fb_len = fb_off = fb_w = torch.zeros(1)
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.clip_logmel(waves, Tables, [0], [0], 8, -18.0, warp=w)
    with pytest.raises(HfttError, match='must be an ops.Warp'):
        ops.clip_logmel(waves, Tables, [0], [0], 8, -18.0, warp='yes')
    table = ops.labels_table([[_note(30, 0.1, 0.5)]], CFG, 'cpu')
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.labels_render(table, [0], [0], 8, warp=w)
    with pytest.raises(HfttError, match='must be an ops.Warp'):
        ops.labels_render(table, [0], [0], 8, warp=3)
    assert ops.WarpTable('cpu').proto.dtype == torch.float32 and ops.WarpTable('cpu').proto.numel() == 6 * 512 + 2


def test_wave_augment_arguments_and_defaults():
    from hftt_hip import HfttError
    from training.dataset import WaveAugment
    a = WaveAugment(gain_db=(-3.0, 3.0))
    assert not a.warps and a.pitch_semitones is None and (a.detune_cents, a.shift, a.p_warp) == (0.0, False, 1.0)
    assert not WaveAugment(pitch_semitones=(0, 0), detune_cents=0, shift=False).warps
    assert WaveAugment(pitch_semitones=(-2, 2)).warps and WaveAugment(detune_cents=20).warps and WaveAugment(shift=True).warps
    for kw, what in ((dict(pitch_semitones=(2, -2)), 'pitch_semitones'), (dict(pitch_semitones=(-0.5, 1)), 'pitch_semitones'),
                     (dict(pitch_semitones=(-12, 0)), 'pitch_semitones'), (dict(detune_cents=51), 'detune_cents'), (dict(detune_cents=-1), 'detune_cents'),
                     (dict(p_warp=1.5), 'p_warp')):
        with pytest.raises(HfttError, match=what):
            WaveAugment(**kw)
    # the warp draw on a CPU generator: reproducible, inside its ranges, clamped, and 3-tuple draws untouched by it
    a = WaveAugment(pitch_semitones=(-2, 2), detune_cents=20, shift=True, p_warp=0.5, seed=5)
    a.reset('cpu')
    lo, hi = torch.tensor([-2] * 32 + [0] * 32), torch.tensor([2] * 32 + [1] * 32)
    w = a.draw_warp(64, 256, lo, hi)
    assert len(a.draw(64)) == 3
    a.reset('cpu')
    w2 = a.draw_warp(64, 256, lo, hi)
    assert torch.equal(w.step_q24, w2.step_q24) and torch.equal(w.delay_q24, w2.delay_q24) and torch.equal(w.shift, w2.shift)
    assert bool(((w.shift >= lo) & (w.shift <= hi)).all()) and bool(((w.delay_q24 >= 0) & (w.delay_q24 < 256 << 24)).all())
    cents = 1200 * torch.log2(w.step_q24.double() / (1 << 24)) - 100 * w.shift
    assert bool((cents.abs() <= 20.0 + 1e-3).all())
    ident = (w.step_q24 == 1 << 24) & (w.delay_q24 == 0) & (w.shift == 0)
    assert 8 < int(ident.sum()) < 56                                   # p_warp = 0.5: some clips exactly unwarped, some not
    a0 = WaveAugment(pitch_semitones=(-2, 2), shift=True, p_warp=0.0)
    a0.reset('cpu')
    w0 = a0.draw_warp(16, 256)
    assert bool((w0.step_q24 == 1 << 24).all()) and not bool(w0.delay_q24.any()) and not bool(w0.shift.any())


def test_trainer_refuses_the_warp_options_without_the_wave_store():
    tool = os.path.join(util.ROOT, 'tools', 'train_config5.py')
    cases = (['--aug-pitch', '-2', '2'], ['--aug-detune-cents', '20'], ['--aug-shift'], ['--aug-warp-p', '0.5'])
    procs = [subprocess.Popen([sys.executable, tool] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for extra in cases]
    for extra, p in zip(cases, procs):                  # (side by side: each run is the interpreter's start-up and the parser)
        _, err = p.communicate(timeout=300)
        assert p.returncode == 2 and 'they need --wave-store' in err, (extra, err[-500:])
