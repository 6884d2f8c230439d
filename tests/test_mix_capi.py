"""C ABI and host half of clip mixing (hftt_clip_logmel_mix, hftt_clip_logmel_mix_warp, hftt_labels_render_mix; hftt_hip.ops.Mix /
audio_frames): the symbols, the descriptor layouts against the C compiler, every host-side refusal by message (they run before the device
guard and the launch, so a box without a GPU tests them), the compile remarks of the kernels with a partner, and the Python entry
points' argument checks.  No compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import util
from hipcc_remarks import CSRC, get, resources

HDR = os.path.join(util.ROOT, 'include', 'hftt_hip.h')
ENTRIES = {'hftt_clip_logmel_mix': ('ClipLogmelMixDesc', 'hftt_clip_logmel_mix_desc'), 'hftt_clip_logmel_mix_warp': ('ClipLogmelMixWarpDesc', 'hftt_clip_logmel_mix_warp_desc'),
           'hftt_labels_render_mix': ('LabelsMixDesc', 'hftt_labels_mix_desc')}


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
    for name, (cls, cname) in ENTRIES.items():
        assert name in _capi.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes[0] is C.POINTER(getattr(_capi, cls))
        assert re.search(r'\bint %s\(const %s\* d, void\* stream\);' % (name, cname), hdr), name
    assert lib.hftt_abi_version() == 8 == _capi.ABI_VERSION


def test_descriptor_layouts_match_the_c_compiler(lib, tmp_path):
    """the new structs, and the existing ones they embed: nothing moved"""
    from hftt_hip import _capi
    pairs = [('hftt_clip_mix_args', _capi.ClipMixArgs), ('hftt_clip_logmel_mix_desc', _capi.ClipLogmelMixDesc),
             ('hftt_clip_logmel_mix_warp_desc', _capi.ClipLogmelMixWarpDesc), ('hftt_labels_mix_desc', _capi.LabelsMixDesc),
             ('hftt_clip_logmel_desc', _capi.ClipLogmelDesc), ('hftt_labels_desc', _capi.LabelsDesc), ('hftt_warp_args', _capi.WarpArgs),
             ('hftt_clip_logmel_warp_desc', _capi.ClipLogmelWarpDesc), ('hftt_labels_warp_desc', _capi.LabelsWarpDesc)]
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
    assert int(got['HFTT_ABI_VERSION']) == 8 == lib.hftt_abi_version()          # the symbols were added AT version 8
    # the sizes the existing entry points were built against, from the header before clip mixing
    assert [int(got[k]) for k in ('hftt_clip_logmel_desc', 'hftt_labels_desc', 'hftt_warp_args', 'hftt_clip_logmel_warp_desc', 'hftt_labels_warp_desc')] == [160, 120, 32, 192, 152]


P = 0x1000          # a non-null "device pointer": every case below is refused before anything dereferences it
WARP_PTRS = ('step_q24', 'delay_q24', 'cut', 'proto')
MIX_PTRS = ('mix_file', 'mix_start', 'mix_gain')


def _set(d, kw):
    for k, v in kw.items():
        tgt = d
        *path, leaf = k.split('.')
        for p in path:
            tgt = getattr(tgt, p)
        setattr(tgt, leaf, v)


def _clip_desc(warp, **kw):
    from hftt_hip import _capi
    d = _capi.ClipLogmelMixWarpDesc() if warp else _capi.ClipLogmelMixDesc()
    b = d.base
    b.total_samples, b.wave_i16, b.n_files, b.B, b.width = 100000, 1, 3, 8, 192
    b.n_fft, b.hop, b.n_mels, b.log_offset, b.fill = 2048, 256, 256, 1e-8, -18.420681
    for name in ('wave', 'file_samp0', 'win_file', 'win_start', 'window', 'twiddle', 'fb_start', 'fb_len', 'fb_off', 'fb_w', 'out'):
        setattr(b, name, P)
    for name in MIX_PTRS:
        setattr(d.mix, name, P)
    if warp:
        for name in WARP_PTRS:
            setattr(d.warp, name, P)
            setattr(d.mix_warp, name, P)
    _set(d, kw)
    return d


BASE_REJECTS = [({'base.wave': None}, b'wave is null'), ({'base.file_samp0': None}, b'file_samp0 is null'), ({'base.win_file': None}, b'null window table'),
                ({'base.win_start': None}, b'null window table'), ({'base.fb_start': None}, b'/ fb_start'), ({'base.out': None}, b'out is null'),
                ({'base.wave_i16': 2}, b'wave_i16=2'), ({'base.n_fft': 1024}, b'n_fft=1024 unsupported (2048 only)'), ({'base.B': 0}, b'B=0'),
                ({'base.width': 0}, b'width=0'), ({'base.n_mels': 257}, b'n_mels=257 outside 1..256'), ({'base.hop': 0}, b'hop=0'),
                ({'base.hop': 325}, b'hop=325'), ({'base.n_files': 0}, b'n_files=0'), ({'base.total_samples': -1}, b'total_samples=-1'),
                ({'base.B': 1 << 30, 'base.width': 17}, b'2^31 workgroups')] + \
               [({'mix.' + n: None}, b'null partner table (mix_file / mix_start / mix_gain)') for n in MIX_PTRS]
WARP_REJECTS = BASE_REJECTS + [({'base.total_samples': (1 << 38) + 1}, b'beyond 2^38')] + \
               [({'warp.' + n: None}, b'null warp table (step_q24 / delay_q24 / cut / proto)') for n in WARP_PTRS] + \
               [({'mix_warp.' + n: None}, b'null partner warp table (step_q24 / delay_q24 / cut / proto)') for n in WARP_PTRS]
_ids = lambda rejects: ['-'.join('%s=%s' % kv for kv in k.items()) for k, _ in rejects]


@pytest.mark.parametrize('kw,msg', BASE_REJECTS, ids=_ids(BASE_REJECTS))
def test_clip_logmel_mix_rejects_before_any_launch(lib, kw, msg):
    d = _clip_desc(False, **kw)
    assert lib.hftt_clip_logmel_mix(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'clip_logmel: ') and msg in err, err


@pytest.mark.parametrize('kw,msg', WARP_REJECTS, ids=_ids(WARP_REJECTS))
def test_clip_logmel_mix_warp_rejects_before_any_launch(lib, kw, msg):
    d = _clip_desc(True, **kw)
    assert lib.hftt_clip_logmel_mix_warp(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'clip_logmel: ') and msg in err, err


LABEL_MAPS = (('shift', 't_delay', 't_scale'), ('mix_shift', 'mix_t_delay', 'mix_t_scale'))


def _labels_desc(maps=(True, True), **kw):
    from hftt_hip import _capi
    d = _capi.LabelsMixDesc()
    b = d.base
    b.n_files, b.n_notes, b.B, b.len, b.N, b.tol, b.duration_tolerance, b.form = 3, 10, 4, 128, 88, 3, 0, 0
    b.hop_ms, b.fps = 16.0, 62.5
    for name in ('notes', 'row_ptr', 'file_nframe', 'win_file', 'win_start', 'onset', 'offset', 'mpe', 'velocity'):
        setattr(b, name, P)
    for name in ('mix_file', 'mix_start', 'a_frames', 'file_end_sec'):
        setattr(d, name, P)
    for on, names in zip(maps, LABEL_MAPS):
        for name in names:
            setattr(d, name, P if on else None)
    _set(d, kw)
    return d


LABELS_REJECTS = [({'base.n_files': 0}, b'n_files=0'), ({'base.n_notes': -1}, b'n_notes=-1'), ({'base.B': 0}, b'B=0'), ({'base.len': 0}, b'len=0'),
                  ({'base.N': 129}, b'N=129 outside 1..128'), ({'base.tol': 0}, b'tol=0'), ({'base.hop_ms': 0.0}, b'hop_ms=0'),
                  ({'base.duration_tolerance': 2}, b'duration_tolerance=2'), ({'base.form': 2}, b'form=2'), ({'base.notes': None}, b'notes is null'),
                  ({'base.row_ptr': None}, b'row_ptr is null'), ({'base.win_file': None}, b'win_file is null'), ({'base.win_start': None}, b'win_start is null'),
                  ({'base.onset': None}, b'null output'), ({'base.B': 1 << 20, 'base.len': 1 << 10, 'base.N': 88}, b'2^31 elements'),
                  ({'mix_file': None}, b'null partner table (mix_file / mix_start)'), ({'mix_start': None}, b'null partner table (mix_file / mix_start)'),
                  ({'a_frames': None}, b'a_frames is null'), ({'file_end_sec': None}, b'null warp table (file_end_sec)')] + \
                 [({n: None}, b'null warp table (shift / t_delay / t_scale: all or none)') for n in LABEL_MAPS[0]] + \
                 [({n: None}, b'null partner warp table (mix_shift / mix_t_delay / mix_t_scale: all or none)') for n in LABEL_MAPS[1]]


@pytest.mark.parametrize('kw,msg', LABELS_REJECTS, ids=_ids(LABELS_REJECTS))
def test_labels_render_mix_rejects_before_any_launch(lib, kw, msg):
    d = _labels_desc(**kw)
    assert lib.hftt_labels_render_mix(C.byref(d), None) not in (0, 2, 3)
    err = lib.hftt_last_error()
    assert err.startswith(b'labels_render: ') and msg in err, err


def test_labels_render_mix_needs_file_nframe_exactly_when_a_source_has_no_map(lib):
    for maps in ((False, False), (True, False), (False, True)):
        d = _labels_desc(maps, **{'base.file_nframe': None})
        assert lib.hftt_labels_render_mix(C.byref(d), None) == 1 and b'file_nframe is null' in lib.hftt_last_error(), maps
    # without a map file_end_sec is not read; a remaining refusal shows that the call got past both checks
    d = _labels_desc((False, False), **{'file_end_sec': None, 'base.len': 0})
    assert lib.hftt_labels_render_mix(C.byref(d), None) == 1 and b'len=0' in lib.hftt_last_error()
    d = _labels_desc((True, True), **{'base.file_nframe': None, 'a_frames': None})
    assert lib.hftt_labels_render_mix(C.byref(d), None) == 1 and b'a_frames is null' in lib.hftt_last_error()


def test_null_descriptors(lib):
    for name in ENTRIES:
        assert getattr(lib, name)(None, None) not in (0, 2, 3) and b'null descriptor' in lib.hftt_last_error()


CLIP_KERNELS = ['clip_logmel_kernel<2048, false>', 'clip_logmel_kernel<2048, true>', 'clip_logmel_kernel<2048, false, clip_mix>', 'clip_logmel_kernel<2048, true, clip_mix>']
LABEL_KERNELS = ['labels_render_kernel<true>', 'labels_render_kernel<false>', 'labels_render_kernel<true, label_mix>', 'labels_render_kernel<false, label_mix>']


def test_the_mixed_clip_kernels_need_no_scratch_and_keep_the_static_lds():
    """clip_logmel.hip: exactly four kernels, clip_logmel_kernel unwarped and warped, without and with a partner; the two with a partner have
    no scratch, no register spilled to memory, and the static LDS of the two without: hop 324 is still admitted"""
    from hftt_hip import _capi
    res = resources('clip_logmel.hip')
    assert sorted(res) == sorted(CLIP_KERNELS)
    base, mix = [res[k] for k in CLIP_KERNELS[:2]], [res[k] for k in CLIP_KERNELS[2:]]
    assert [get(v, 'ScratchSize') for v in mix] == [0, 0] and [get(v, 'VGPRs Spill') for v in mix] == [0, 0]
    staged = lambda hop: ((_capi.CLIP_LOGMEL_RUN - 1) * hop + 2048) * 4
    lds = [get(v, 'LDS Size') for v in mix]
    assert len(set(get(v, 'LDS Size') for v in base)) == 1 and lds == [get(v, 'LDS Size') for v in base]
    assert lds[0] + staged(324) <= 65536 < lds[0] + staged(325)
    print('clip_logmel.hip with a partner: VGPRs %s, occupancy %s, SGPRs spilled to VGPR lanes %s, static LDS %s'
          % tuple([get(v, k) for v in mix] for k in ('VGPRs', 'Occupancy', 'SGPRs Spill', 'LDS Size')))


def test_the_mixed_label_kernels_need_no_scratch():
    """labels.hip: exactly four kernels, both output forms without and with a partner; the two with a partner have no scratch; registers and
    occupancy are printed"""
    res = resources('labels.hip')
    assert sorted(res) == sorted(LABEL_KERNELS)
    mix = [res[k] for k in LABEL_KERNELS[2:]]
    assert [get(v, 'ScratchSize') for v in mix] == [0, 0] and [get(v, 'VGPRs Spill') for v in mix] == [0, 0]
    print('labels.hip with a partner: VGPRs %s, occupancy %s, SGPRs spilled to VGPR lanes %s' % tuple([get(v, k) for v in mix] for k in ('VGPRs', 'Occupancy', 'SGPRs Spill')))


def test_the_shared_bodies_are_written_once():
    """the kernel templates, the refusals and the frame transform are written in one file each; no other file carries a second copy"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith(('.hip', '.h'))}
    for pat, home in ((r'__global__ .*\bvoid clip_logmel_kernel\(', 'clip_logmel.hip'), (r'__global__ .*\bvoid labels_render_kernel\(', 'labels.hip'),
                      (r'\bvoid label_walk\(', 'labels.hip'), (r'clip_logmel: n_fft=%d unsupported', 'clip_logmel.hip'), (r'labels_render: tol=%d', 'labels.hip'),
                      (r'dst\[j0 \+ 3 \* Ns\]', 'logmel_frame.h'), (r'xr \* xr \+ xi \* xi', 'logmel_frame.h'), (r'acc \+= fb_w\[off \+ j\] \* pw\[st \+ j\]', 'logmel_frame.h')):
        assert [f for f, s in src.items() for _ in re.findall(pat, s)] == [home], pat
    for f in ('clip_logmel.hip', 'logmel.hip'):
        assert '#include "logmel_frame.h"' in src[f] and '__global__' not in src['logmel_frame.h'], f


def _note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


CFG = {'feature': {'sr': 16000, 'hop_sample': 256}, 'midi': {'note_min': 21, 'num_note': 88}}


def test_python_entry_points_refuse_cpu_tensors_and_wrong_mixes():
    from hftt_hip import HfttError, ops
    waves = ops.WaveTable([np.zeros(600, np.float32), np.zeros(0, np.float32)], 'cpu', 'float32')
    m = ops.Mix(torch.tensor([1]), torch.tensor([0]), torch.tensor([0.5]))
    assert m.file.dtype == torch.int32 and m.start.dtype == torch.int32 and m.gain.dtype == torch.float32 and m.warp is None
    with pytest.raises(HfttError, match=r'must be \[B\]'):
        ops.Mix(torch.tensor([1, 0]), torch.tensor([0]), torch.tensor([0.5]))
    with pytest.raises(HfttError, match='must be an ops.Warp'):
        ops.Mix(torch.tensor([1]), torch.tensor([0]), torch.tensor([0.5]), warp=(1 << 24, 0))
    with pytest.raises(HfttError, match='the warp holds 2 windows'):
        ops.Mix(torch.tensor([1]), torch.tensor([0]), torch.tensor([0.5]), warp=ops.Warp(torch.tensor([1 << 24] * 2), torch.tensor([0, 0])))

    class Tables:                                       # an ops.LogMel that was never uploaded
        device = torch.device('cpu')
        n_fft, hop, n_mels, log_offset = 2048, 256, 4, 1e-8
        window = twiddle = fb_start = fb_len = fb_off = fb_w = torch.zeros(1)
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.clip_logmel(waves, Tables, [0], [0], 8, -18.0, mix=m)
    with pytest.raises(HfttError, match='must be an ops.Mix'):
        ops.clip_logmel(waves, Tables, [0], [0], 8, -18.0, mix=(1, 0, 0.5))
    table = ops.labels_table([[_note(30, 0.1, 0.5)], []], CFG, 'cpu')
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.labels_render(table, [0], [0], 8, mix=m, a_frames=[3])
    with pytest.raises(HfttError, match='must be an ops.Mix'):
        ops.labels_render(table, [0], [0], 8, mix='yes', a_frames=[3])
    with pytest.raises(HfttError, match='a mix needs a_frames'):
        ops.labels_render(table, [0], [0], 8, mix=m)
    old = {k: v for k, v in ops.labels_table_host([[_note(30, 0.1, 0.5)], []], CFG).items() if k not in ('file_end_sec', 'pitch_min', 'pitch_max', 'sr')}
    with pytest.raises(HfttError, match='file_end_sec'):                # a partner under a warp needs the table's warp columns
        ops.labels_render(ops.LabelsTable(old, 'cpu'), [0], [0], 8, a_frames=[3],
                          mix=ops.Mix(torch.tensor([1]), torch.tensor([0]), torch.tensor([0.5]), warp=ops.Warp(torch.tensor([1 << 24]), torch.tensor([0]))))


def test_audio_frames_is_the_kernels_frame_count():
    """1 + n' / hop per window on the host tensors (the arithmetic is integer: the device gives the same), 0 without a valid file or warp"""
    from hftt_hip import ops
    import warp_emul as W
    lens = [0, 1, 255, 256, 2304, 4219]
    waves = ops.WaveTable([np.zeros(n, np.float32) for n in lens], 'cpu', 'float32')
    files = [0, 1, 2, 3, 4, 5, -1, 6]
    assert ops.audio_frames(waves, 256, files).tolist() == [1 + n // 256 for n in lens] + [0, 0]
    steps = [W.step_of(1.0), 1 << 23, 1 << 25, 1 << 24, W.step_of(-1.7), (1 << 25) + 1, 1 << 24, 1 << 24]
    delays = [0, 7, 255 << 24, 512 << 24, int(0.37 * W.ONE), 0, 0, 0]
    got = ops.audio_frames(waves, 256, files, ops.Warp(torch.tensor(steps), torch.tensor(delays))).tolist()
    want = [1 + W.warp_len(lens[f], steps[b], delays[b]) // 256 for b, f in enumerate(files[:5])] + [0, 0, 0]
    assert got == want and got[3] == 4 and ops.audio_frames(waves, 256, files).dtype == torch.int64


def test_trainer_refuses_the_mix_options_without_the_wave_store():
    tool = os.path.join(util.ROOT, 'tools', 'train_config5.py')
    cases = (['--aug-mix-p', '0.5'], ['--aug-mix-gain-db', '-6', '0'])
    procs = [subprocess.Popen([sys.executable, tool] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for extra in cases]
    for extra, p in zip(cases, procs):                  # (side by side: each run is the interpreter's start-up and the parser)
        _, err = p.communicate(timeout=300)
        assert p.returncode == 2 and 'they need --wave-store' in err, (extra, err[-500:])
