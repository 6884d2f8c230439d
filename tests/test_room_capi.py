"""C ABI and host half of the room augmentation (hftt_clip_room; hftt_hip.ops.RoomBank / clip_room; WaveAugment's room_p; corpus.synth_audio's
synth_room_bank / align_ir): the symbol, the descriptor layout against the C compiler, every host-side refusal by status and message (they run
before the device guard and the launch, so a box without a GPU tests them), the compile remarks of the kernels, the one definition of the dry
sample, and the Python side's argument checks and draws.  No compute calls."""
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


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('hftt_build', os.path.join(util.ROOT, 'nylon-amt_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    assert 'clip_room.hip' in mod.SOURCES
    from hftt_hip import _capi
    return _capi.lib()


def test_the_symbol_is_exported_and_bound_at_abi_8(lib):
    from hftt_hip import _capi
    assert 'hftt_clip_room' in _capi.SIGNATURES and hasattr(lib, 'hftt_clip_room')
    assert lib.hftt_clip_room.argtypes[0] is C.POINTER(_capi.ClipRoomDesc)
    hdr = open(HDR).read()
    assert re.search(r'\bint hftt_clip_room\(const hftt_clip_room_desc\* d, void\* stream\);', hdr)
    assert re.search(r'#define HFTT_ABI_VERSION 8\b', hdr) and lib.hftt_abi_version() == 8 == _capi.ABI_VERSION
    assert re.search(r'#define HFTT_ROOM_MAX_TAPS %d\b' % _capi.ROOM_MAX_TAPS, hdr) and _capi.ROOM_MAX_TAPS == 8192


def test_descriptor_layout_matches_the_c_compiler(lib, tmp_path):
    """the new struct, and the existing ones it embeds or stands beside: nothing moved"""
    from hftt_hip import _capi
    pairs = [('hftt_clip_room_desc', _capi.ClipRoomDesc), ('hftt_clip_logmel_desc', _capi.ClipLogmelDesc), ('hftt_warp_args', _capi.WarpArgs),
             ('hftt_clip_mix_args', _capi.ClipMixArgs), ('hftt_clip_logmel_mix_warp_desc', _capi.ClipLogmelMixWarpDesc)]
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
    assert [int(got[k]) for k in ('hftt_clip_logmel_desc', 'hftt_warp_args', 'hftt_clip_mix_args')] == [160, 32, 24]      # as before the room


P = 0x1000          # a non-null "device pointer": every case below is refused before anything dereferences it
WARP_PTRS = ('step_q24', 'delay_q24', 'cut', 'proto')
MIX_PTRS = ('mix_file', 'mix_start', 'mix_gain')
SPAN = (4 + 192 - 1) * 256 + 1024


def _desc(warp=False, mix=False, **kw):
    from hftt_hip import _capi
    d = _capi.ClipRoomDesc()
    d.total_samples, d.wave_i16, d.n_files, d.B, d.width = 100000, 1, 3, 8, 192
    d.n_fft, d.hop, d.n_ir, d.L, d.span = 2048, 256, 4, 4096, SPAN
    for name in ('wave', 'file_samp0', 'win_file', 'win_start', 'ir', 'ir_taps', 'ir_index', 'out', 'out_samp0', 'out_win_file', 'out_win_start'):
        setattr(d, name, P)
    if warp:
        for name in WARP_PTRS:
            setattr(d.warp, name, P)
    if mix:
        for name in MIX_PTRS:
            setattr(d.mix, name, P)
    if warp and mix:
        for name in WARP_PTRS:
            setattr(d.mix_warp, name, P)
    for k, v in kw.items():
        tgt = d
        *path, leaf = k.split('.')
        for p in path:
            tgt = getattr(tgt, p)
        setattr(tgt, leaf, v)
    return d


OUT = b'null output (out / out_samp0 / out_win_file / out_win_start)'
BASE = [({'wave': None}, b'wave is null'), ({'file_samp0': None}, b'file_samp0 is null'), ({'win_file': None}, b'null window table'),
        ({'win_start': None}, b'null window table'), ({'ir': None}, b'null response table'), ({'ir_taps': None}, b'null response table'),
        ({'ir_index': None}, b'null response table'), ({'out': None}, OUT), ({'out_samp0': None}, OUT), ({'out_win_file': None}, OUT),
        ({'out_win_start': None}, OUT), ({'wave_i16': 2}, b'wave_i16=2'), ({'n_fft': 1024}, b'n_fft=1024 unsupported (2048 only)'),
        ({'B': 0}, b'B=0'), ({'B': 1 << 30}, b'B=1073741824'), ({'width': 0}, b'width=0'), ({'hop': 0}, b'hop=0'), ({'n_files': 0}, b'n_files=0'),
        ({'total_samples': -1}, b'total_samples=-1'), ({'n_ir': 0}, b'n_ir=0'), ({'L': 0}, b'L=0 outside 1..8192'), ({'L': 8193}, b'L=8193 outside 1..8192'),
        ({'span': SPAN - 1}, b'span=%d below the %d samples' % (SPAN - 1, SPAN)), ({'B': (1 << 30) - 1, 'width': 1 << 20, 'span': 1 << 40}, b'2^31 workgroups')]
WARP = [({'total_samples': (1 << 38) + 1}, b'beyond 2^38')] + [({'warp.' + n: None}, b'null warp table (step_q24 / delay_q24 / cut / proto: all or none)') for n in WARP_PTRS]
MIX = [({'mix.' + n: None}, b'null partner table (mix_file / mix_start / mix_gain: all or none)') for n in MIX_PTRS]
MIX_WARP = [({'mix_warp.' + n: None}, b'null partner warp table (step_q24 / delay_q24 / cut / proto)') for n in WARP_PTRS]
CASES = [((False, False), kw, msg) for kw, msg in BASE] + [((True, False), kw, msg) for kw, msg in BASE[:3] + WARP] + \
        [((False, True), kw, msg) for kw, msg in BASE[:3] + MIX] + [((True, True), kw, msg) for kw, msg in WARP + MIX_WARP] + \
        [((True, False), {'mix_warp.cut': P}, b'a partner warp table without both a warp and a partner'),
         ((False, True), {'mix_warp.proto': P}, b'a partner warp table without both a warp and a partner')]


@pytest.mark.parametrize('form,kw,msg', CASES, ids=['%s%s-%s' % ('warp' * f[0], 'mix' * f[1], '-'.join('%s=%s' % kv for kv in kw.items())) for f, kw, _ in CASES])
def test_clip_room_refuses_before_any_launch(lib, form, kw, msg):
    d = _desc(*form, **kw)
    assert lib.hftt_clip_room(C.byref(d), None) == 1
    err = lib.hftt_last_error()
    assert err.startswith(b'clip_room: ') and msg in err, err


def test_the_2_38_limit_holds_only_under_a_warp_and_a_null_descriptor_is_refused(lib):
    d = _desc(total_samples=(1 << 38) + 1, width=0)           # without a warp the call gets past it, to the next refusal
    assert lib.hftt_clip_room(C.byref(d), None) == 1 and b'width=0' in lib.hftt_last_error()
    assert lib.hftt_clip_room(None, None) == 1 and b'clip_room: null descriptor' in lib.hftt_last_error()


def test_the_room_kernels_need_no_scratch_and_no_spill():
    """clip_room.hip: one kernel in the four forms of the clip log-mel (unwarped / warped, without / with a partner); no scratch, no register
    spilled to memory, no static LDS (the staged span is dynamic: it follows the bank's L); registers and occupancy are printed"""
    res = resources('clip_room.hip')
    assert sorted(res) == sorted('clip_room_kernel<%s, %s>' % (w, m) for w in ('false', 'true') for m in ('false', 'true'))
    for k, v in res.items():
        assert get(v, 'ScratchSize') == 0 and get(v, 'VGPRs Spill') == 0 and get(v, 'LDS Size') == 0, (k, v)
    print('clip_room.hip: VGPRs %s, occupancy %s, SGPRs spilled to VGPR lanes %s' % tuple([get(v, k) for v in res.values()] for k in ('VGPRs', 'Occupancy', 'SGPRs Spill')))


def test_the_dry_sample_is_written_once_and_both_kernels_call_it():
    src = {f: re.sub(r'//[^\n]*', '', open(os.path.join(CSRC, f)).read()) for f in os.listdir(CSRC) if f.endswith(('.hip', '.h', '.cpp'))}
    for pat in (r'\bfloat clip_dry\(', r'\bclip_source clip_source_load\(', r'\bfloat warp_sample\('):
        assert [f for f, s in src.items() for _ in re.findall(pat, s)] == ['wave_warp.h' if 'warp_sample' in pat else 'clip_dry.h'], pat
    for f in ('clip_logmel.hip', 'clip_room.hip'):
        s = src[f]
        assert '#include "clip_dry.h"' in s and 'clip_dry<WARP, false>(' in s and 'clip_dry<WARP, true>(' in s, f
        # ... and neither spells the sample out again: no read of the corpus, no warped sample, no product with a gain outside the header
        assert not re.search(r'warp_sample\(|warp_source\(|\(const short\*\)|\* *gain\b|\* *gainB\b|1\.f / 32768', s), f
    assert '__global__' not in src['clip_dry.h']
    assert [f for f, s in src.items() for _ in re.findall(r'__global__ .*\bvoid clip_room_kernel\(', s)] == ['clip_room.hip']


def test_room_bank_and_wave_augment_refusals():
    from hftt_hip import HfttError, ops
    from training.dataset import WaveAugment
    bank = ops.RoomBank(np.ones((3, 5), np.float32), 'cpu', taps=[1, 5, 2])
    assert (bank.n_ir, bank.L) == (3, 5) and bank.ir.dtype == torch.float32 and bank.taps.dtype == torch.int32 and bank.taps.tolist() == [1, 5, 2]
    assert ops.RoomBank(np.ones((2, 7)), 'cpu').taps.tolist() == [7, 7]
    for bad in (np.ones(5, np.float32), np.ones((0, 5), np.float32), np.ones((2, 0), np.float32), np.ones((1, 8193), np.float32), np.ones((2, 3), np.int32),
                np.full((1, 4), np.nan, np.float32)):
        with pytest.raises(HfttError, match='RoomBank: ir must be'):
            ops.RoomBank(bad, 'cpu')
    for taps in ([0, 1, 1], [1, 6, 1], [1, 2], [1.0, 2.0, 3.0]):
        with pytest.raises(HfttError, match='RoomBank: taps must be integers'):
            ops.RoomBank(np.ones((3, 5), np.float32), 'cpu', taps=taps)
    for p in (-0.1, 1.5, float('nan')):
        with pytest.raises(HfttError, match='room_p=.* is no probability'):
            WaveAugment(room_p=p, room_bank=bank)
    with pytest.raises(HfttError, match='needs a room_bank'):
        WaveAugment(room_p=0.5)
    with pytest.raises(HfttError, match='room_bank must be an ops.RoomBank'):
        WaveAugment(room_p=0.5, room_bank=np.ones((3, 5), np.float32))
    assert WaveAugment().rooms is False and WaveAugment(room_bank=bank).rooms is False and WaveAugment(room_p=1.0, room_bank=bank).rooms is True


def test_python_entry_points_refuse_cpu_tensors_and_wrong_rooms():
    from hftt_hip import HfttError, ops
    waves = ops.WaveTable([np.zeros(600, np.float32), np.zeros(0, np.float32)], 'cpu', 'float32')
    bank = ops.RoomBank(np.ones((3, 5), np.float32), 'cpu')

    class Tables:                                       # an ops.LogMel that was never uploaded
        device = torch.device('cpu')
        n_fft, hop, n_mels, log_offset = 2048, 256, 4, 1e-8
        window = twiddle = fb_start = fb_len = fb_off = fb_w = torch.zeros(1)
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.clip_room(waves, [0], [0], 8, bank, [0], 256)
    with pytest.raises(HfttError, match='no CPU fallback'):
        ops.clip_logmel(waves, Tables, [0], [0], 8, -18.0, room=(bank, [0]))
    with pytest.raises(HfttError, match='bank must be an ops.RoomBank'):
        ops.clip_room(waves, [0], [0], 8, np.ones((3, 5)), [0], 256)
    for room in (bank, (bank,), (np.ones((3, 5)), [0])):
        with pytest.raises(HfttError, match=r'room must be \(an ops.RoomBank, ir_index\)'):
            ops.clip_logmel(waves, Tables, [0], [0], 8, -18.0, room=room)
    assert ops.room_span(192, 256) == SPAN and ops.room_span(20, 256) == 23 * 256 + 1024 and ops.room_span(1, 1000) == 2 * 1000 + 1024


def test_synth_room_bank():
    from corpus import synth_audio as SA
    ir, taps = SA.synth_room_bank(6, 16000, taps=4096, seed=3)
    ir2, taps2 = SA.synth_room_bank(6, 16000, taps=4096, seed=3)
    ir3, _ = SA.synth_room_bank(6, 16000, taps=4096, seed=4)
    assert ir.dtype == np.float32 and ir.shape == (6, 4096) and taps.dtype == np.int32 and taps.shape == (6,)
    assert np.array_equal(ir, ir2) and np.array_equal(taps, taps2) and not np.array_equal(ir, ir3)
    assert np.allclose(np.sqrt((ir.astype(np.float64) ** 2).sum(1)), 1.0, atol=1e-6)
    assert (np.abs(ir).argmax(1) == 0).all() and (ir[:, 0] > 0).all()
    assert ((taps >= 1) & (taps <= 4096)).all()
    for h, t in zip(ir, taps):
        assert not h[t:].any() and not h[1:16].any()         # nothing behind ir_taps; at least 1 ms of silence behind the direct path
        drr = 10 * np.log10(float(h[0]) ** 2 / float((h[1:].astype(np.float64) ** 2).sum()))
        assert -0.01 <= drr <= 12.01, drr
    # a short response: rt60 well inside the taps -> ir_taps in front of the end; a long one: ir_taps == taps
    _, short = SA.synth_room_bank(3, 16000, taps=8192, rt60=(0.1, 0.2), seed=1)
    _, long_ = SA.synth_room_bank(3, 16000, taps=1024, rt60=(0.5, 0.8), seed=1)
    assert (short < 8192).all() and (short >= 1600).all() and (long_ == 1024).all()
    assert SA.synth_room_bank(2, 16000, taps=1, seed=0)[0].tolist() == [[1.0], [1.0]]


def test_align_ir():
    from corpus import synth_audio as SA
    h = np.zeros(64)
    h[10], h[11], h[40], h[3] = -2.0, 0.5, 0.25, 0.1
    a = SA.align_ir(h)
    assert a.dtype == np.float32 and a.shape == (64,) and abs(float(np.sqrt((a.astype(np.float64) ** 2).sum())) - 1.0) < 1e-6
    assert int(np.abs(a).argmax()) == 0 and a[0] < 0 and a[1] > 0 and a[30] > 0 and not a[54:].any()
    assert np.allclose(a[:3], np.array([-2.0, 0.5, 0.0]) / np.sqrt(4.0 + 0.25 + 0.0625))
    for bad in (np.zeros(8), np.zeros((2, 4)) + 1, np.array([1.0, np.inf]), np.zeros(0)):
        with pytest.raises(ValueError):
            SA.align_ir(bad)


def test_draw_room_leaves_every_other_draw_of_a_seed_unchanged():
    """gain / noise / warp / mix draws of a seeded WaveAugment with room_p 0 and 0.5 on a CPU generator, in the order WaveClipStore.batch makes
    them: the room's two draws come last in a batch, so the batch that draws a room has every other draw of the seed unchanged; and with
    room_p == 0 no draw is made, so the seed reproduces every batch it gave before there was a room"""
    from hftt_hip import ops
    from training.dataset import WaveAugment
    bank = ops.RoomBank(np.ones((5, 4), np.float32), 'cpu')
    kw = dict(gain_db=(-6.0, 6.0), noise_dbfs=(-60.0, -40.0), seed=9, pitch_semitones=(-2, 2), detune_cents=20.0, shift=True, p_warp=0.7, mix_p=0.5)
    B = 16

    def batches(aug):
        aug.reset('cpu')
        out = []
        for _ in range(3):
            gain, noise, seed = aug.draw(B)
            w = aug.draw_warp(B, 256)
            on, partner, mgain = aug.draw_mix(B, 1000)
            pw = aug.draw_warp(B, 256)
            room = aug.draw_room(B)
            out.append(([gain, noise, torch.tensor(seed), w.step_q24, w.delay_q24, w.shift, on, partner, mgain, pw.step_q24, pw.delay_q24, pw.shift], room))
        return out
    off, on = batches(WaveAugment(**kw)), batches(WaveAugment(room_p=0.5, room_bank=bank, **kw))
    for k, ((a, ra), (b, rb)) in enumerate(zip(off, on)):
        assert ra is None and rb.dtype == torch.int32 and rb.shape == (B,) and int(rb.min()) >= -1 and int(rb.max()) < 5
        # (from the second batch on the stream has moved by the room draws in front: one generator serves all draws)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) == (k == 0), k
    again = batches(WaveAugment(room_bank=bank, **kw))
    assert all(torch.equal(x, y) for (a, _), (b, _) in zip(off, again) for x, y in zip(a, b)) and all(r is None for _, r in again)
    rooms = torch.cat([r for _, r in on])
    assert bool((rooms < 0).any()) and bool((rooms >= 0).any()) and torch.equal(rooms, torch.cat([r for _, r in batches(WaveAugment(room_p=0.5, room_bank=bank, **kw))]))


def test_trainer_refuses_the_room_options_without_the_wave_store_and_a_bank_next_to_synthesis_settings():
    tool = os.path.join(util.ROOT, 'tools', 'train_config5.py')
    cases = ((['--aug-room-p', '0.5'], 'they need --wave-store'), (['--aug-room-bank', 'bank.npz'], 'they need --wave-store'),
             (['--wave-store', '--aug-room-p', '0.5', '--aug-room-bank', 'bank.npz', '--aug-room-taps', '1024'], '--aug-room-bank supplies the responses'))
    procs = [subprocess.Popen([sys.executable, tool] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for extra, _ in cases]
    for (extra, msg), p in zip(cases, procs):           # (side by side: each run is the interpreter's start-up and the parser)
        _, err = p.communicate(timeout=300)
        assert p.returncode == 2 and msg in err, (extra, err[-500:])
