"""C ABI and host half of the played clip synth (hftt_clip_synth_parts; hftt_hip.ops.clip_synth's play / tune / part / nsamp, SynthPart, synth_nsamp,
synth_frames; training.dataset.SynthPlay and SynthClipStore's play; corpus.synth_audio.synth_voice_bank's headroom; the trainer's flags): the
symbol, the descriptor layout against the C compiler, every host-side refusal by status and message (they run before the device guard and the
launch, so a box without a GPU tests them), the compile remarks of the kernel, and the Python side's argument checks.  No compute calls."""
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
    assert 'clip_synth_parts.hip' in mod.SOURCES and 'clip_synth.hip' in mod.SOURCES
    from hftt_hip import _capi
    return _capi.lib()


def test_the_symbol_is_exported_and_the_abi_is_still_8(lib):
    from hftt_hip import _capi
    assert 'hftt_clip_synth_parts' in _capi.SIGNATURES and hasattr(lib, 'hftt_clip_synth_parts')
    assert lib.hftt_clip_synth_parts.argtypes[0] is C.POINTER(_capi.ClipSynthPartsDesc)
    hdr = open(HDR).read()
    assert re.search(r'\bint hftt_clip_synth_parts\(const hftt_clip_synth_parts_desc\* d, void\* stream\);', hdr)
    assert re.search(r'#define HFTT_ABI_VERSION 8\b', hdr) and lib.hftt_abi_version() == 8 == _capi.ABI_VERSION


def test_descriptor_layout_matches_the_c_compiler(lib, tmp_path):
    """the two new structs, and the one they embed: nothing moved"""
    from hftt_hip import _capi
    pairs = [('hftt_synth_play_args', _capi.SynthPlayArgs), ('hftt_clip_synth_parts_desc', _capi.ClipSynthPartsDesc), ('hftt_clip_synth_desc', _capi.ClipSynthDesc)]
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
    assert int(got['hftt_synth_play_args']) == 32 and int(got['hftt_clip_synth_parts_desc']) == int(got['hftt_clip_synth_desc']) + 8 + 32 + 4 * 8 + 8 + 32


P = 0x1000          # a non-null "device pointer": every case below is refused before anything dereferences it
BASE_PTRS = ('notes', 'row_ptr', 'win_file', 'win_start', 'inc', 'amp', 'dec', 'vel_gain', 'rel', 'attack', 'release', 'voice_index',
             'out', 'out_samp0', 'out_win_file', 'out_win_start')
PART_PTRS = ('part_file', 'part_start', 'part_voice', 'part_gain')
MAP_PTRS = ('shift', 't_delay', 't_scale')
SPAN = (4 + 192 - 1) * 256 + 1024
SPAN3 = (4 + 3 + 192 - 1) * 256 + 1024


def _desc(**kw):
    """a descriptor with everything given (both plays, the partner tables, part_nsamp) that only the changes in kw keep from the launch; base
    fields by their name, the others as 'play.shift', 'part_play.tune_q31', 'part_file', 'nsamp', ..."""
    from hftt_hip import _capi
    d = _capi.ClipSynthPartsDesc()
    b = d.base
    b.n_files, b.n_notes, b.B, b.width, b.N = 3, 100, 8, 192, 88
    b.n_fft, b.hop, b.lead, b.sr, b.V, b.H, b.span = 2048, 256, 0, 16000.0, 4, 16, SPAN
    for name in BASE_PTRS:
        setattr(b, name, P)
    b.file_nsamp = None                                      # not read here: null is allowed
    d.nsamp = d.part_nsamp = P
    for name in PART_PTRS:
        setattr(d, name, P)
    for play in (d.play, d.part_play):
        for name in MAP_PTRS + ('tune_q31',):
            setattr(play, name, P)
    for k, v in kw.items():
        obj, _, name = k.rpartition('.')
        setattr({'': d, 'play': d.play, 'part_play': d.part_play, 'base': d.base}[obj], name, v)
    return d


def _no_partner(**kw):
    return dict({n: None for n in PART_PTRS}, **kw)


BANK = b'null voice bank (inc / amp / dec / vel_gain / rel / attack / release)'
OUT = b'null output (out / out_samp0 / out_win_file / out_win_start)'
B_ = lambda **kw: {'base.' + k: v for k, v in kw.items()}
CASES = [(B_(notes=None), b'notes is null at n_notes=100'), (B_(row_ptr=None), b'row_ptr is null'), ({'nsamp': None}, b'nsamp is null'),
         (B_(win_file=None), b'null window table'), (B_(win_start=None), b'null window table'), (B_(voice_index=None), b'voice_index is null')] + \
        [(B_(**{n: None}), BANK) for n in ('inc', 'amp', 'dec', 'vel_gain', 'rel', 'attack', 'release')] + \
        [(B_(**{n: None}), OUT) for n in ('out', 'out_samp0', 'out_win_file', 'out_win_start')] + \
        [({'play.' + n: None}, b'null play table (shift / t_delay / t_scale: all or none)') for n in MAP_PTRS] + \
        [({'part_play.' + n: None}, b'null partner play table (part_play shift / t_delay / t_scale: all or none)') for n in MAP_PTRS] + \
        [({n: None}, b'null partner table (part_file / part_start / part_voice / part_gain: all or none)') for n in PART_PTRS] + \
        [(_no_partner(), b'part_nsamp given without partner tables'),
         (_no_partner(part_nsamp=None), b'part_play given without partner tables'),
         (_no_partner(part_nsamp=None, **{'part_play.' + n: None for n in MAP_PTRS}), b'part_play given without partner tables'),      # tune alone
         ({'part_nsamp': None}, b'part_nsamp is null with partner tables')] + \
        [(B_(n_fft=1024), b'n_fft=1024 unsupported (2048 only)'), (B_(B=0), b'B=0'), (B_(B=1 << 30), b'B=1073741824'), (B_(width=0), b'width=0'),
         (B_(hop=0), b'hop=0'), (B_(n_files=0), b'n_files=0'), (B_(n_notes=-1), b'n_notes=-1 is negative'), (B_(V=0), b'V=0'),
         (B_(N=0), b'N=0 outside 1..128'), (B_(N=129), b'N=129 outside 1..128'), (B_(H=0), b'H=0 outside 1..32'), (B_(H=33), b'H=33 outside 1..32'),
         (B_(V=1 << 20, N=128, H=32), b'exceeds 2^31 entries'), (B_(lead=-1), b'lead=-1 is negative'), (B_(sr=0.0), b'sr=0 must be positive'),
         (B_(sr=-16000.0), b'sr=-16000 must be positive'), (B_(sr=float('nan')), b'must be positive'), (B_(sr=float('inf')), b'must be positive'),
         (B_(span=SPAN - 1), b'span=%d below the %d samples' % (SPAN - 1, SPAN)), (B_(lead=3), b'span=%d below the %d samples' % (SPAN, SPAN3)),
         (B_(B=(1 << 30) - 1, width=1 << 20, span=1 << 40), b'2^31 workgroups'),
         (B_(lead=(1 << 31) - 1, width=(1 << 31) - 1, hop=(1 << 31) - 1, span=1 << 62), b'span=%d below the' % (1 << 62))]


@pytest.mark.parametrize('kw,msg', CASES, ids=['%d-' % i + '-'.join('%s=%s' % kv for kv in kw.items())[:60] for i, (kw, _) in enumerate(CASES)])
def test_clip_synth_parts_refuses_before_any_launch(lib, kw, msg):
    d = _desc(**kw)
    assert lib.hftt_clip_synth_parts(C.byref(d), None) == 1
    err = lib.hftt_last_error()
    assert err.startswith(b'clip_synth_parts: ') and msg in err, err


def test_a_null_descriptor_is_refused_and_file_nsamp_is_not_asked_for(lib):
    assert lib.hftt_clip_synth_parts(None, None) == 1 and b'clip_synth_parts: null descriptor' in lib.hftt_last_error()
    # base.file_nsamp null, notes null at n_notes == 0, no plays, no partner: the call gets past all of it, to the next refusal
    kw = _no_partner(part_nsamp=None, **{p + n: None for p in ('play.', 'part_play.') for n in MAP_PTRS + ('tune_q31',)})
    d = _desc(**dict(kw, **B_(notes=None, n_notes=0, width=0)))
    assert lib.hftt_clip_synth_parts(C.byref(d), None) == 1 and b'width=0' in lib.hftt_last_error()
    d = _desc(**B_(width=0))                                 # and with everything given
    assert lib.hftt_clip_synth_parts(C.byref(d), None) == 1 and b'width=0' in lib.hftt_last_error()


def test_the_parts_kernel_needs_no_scratch_and_no_spill():
    """clip_synth_parts.hip: one kernel; no scratch, no register spilled to memory, at least four waves per SIMD -- the condition its sibling is
    held to, for the same reason: four windows' tiles per SIMD hide the latency of the transcendental instructions"""
    res = resources('clip_synth_parts.hip')
    assert sorted(res) == ['clip_synth_parts_kernel']
    v = res['clip_synth_parts_kernel']
    assert get(v, 'ScratchSize') == 0 and get(v, 'VGPRs Spill') == 0 and get(v, 'Occupancy') >= 4, v
    print('clip_synth_parts.hip: VGPRs %s, occupancy %s, LDS %s' % tuple(get(v, k) for k in ('VGPRs', 'Occupancy', 'LDS Size')))
    src = re.sub(r'//[^\n]*', '', open(os.path.join(util.ROOT, 'nylon-amt_amd', 'csrc', 'clip_synth_parts.hip')).read())
    assert '#include "clip_synth_fn.h"' in src and 'synth_sin_turns(' in src and 'synth_exp2(' in src and '#include "block_scan.h"' in src
    assert not re.search(r'atomic|sinf\(|expf\(|exp2f\(|__sinf|__expf', src)        # the two functions come from the one header, nothing else
    assert len(re.findall(r'synth_sin_turns\(', src)) == 1                          # one walk for both parts, not one each


def _bank(V=2, N=5, H=3, inc=1 << 30):
    return {'inc': np.full((V, N, H), inc, np.uint32), 'amp': np.ones((V, N, H), np.float32), 'dec': np.zeros((V, N, H), np.float32),
            'vel_gain': np.ones((V, 128), np.float32), 'rel': np.zeros(V, np.float32), 'attack': np.ones(V, np.int32), 'release': np.zeros(V, np.int32)}


def test_synth_play_argument_errors():
    from hftt_hip import HfttError
    from training.dataset import SynthPlay
    p = SynthPlay(transpose=(-3, 4), tune_cents=20.0, tempo=(0.8, 1.25), shift=True, p_play=0.5, duet_p=0.25, duet_gain_db=(-9.0, -3.0))
    assert (p.transpose, p.tune_cents, p.tempo, p.shift, p.p_play, p.duet_p, p.duet_gain_db, p.duets) == ((-3, 4), 20.0, (0.8, 1.25), True, 0.5, 0.25, (-9.0, -3.0), True)
    assert not SynthPlay().duets and SynthPlay().tune_max() == 1 << 31 and p.tune_max() == int(round(2.0 ** (20.0 / 1200.0) * 2.0 ** 31))
    for bad, match in ((dict(transpose=(-12, 0)), 'transpose'), (dict(transpose=(2, 1)), 'transpose'), (dict(transpose=(0.5, 1)), 'transpose'), (dict(transpose=(1,)), 'transpose'),
                       (dict(tune_cents=50.5), 'tune_cents'), (dict(tune_cents=-1.0), 'tune_cents'), (dict(tempo=(0.4, 1.0)), 'tempo'), (dict(tempo=(1.0, 2.5)), 'tempo'),
                       (dict(tempo=(1.2, 1.1)), 'tempo'), (dict(p_play=1.5), 'p_play'), (dict(duet_p=-0.1), 'duet_p'), (dict(duet_gain_db=(0.0, -6.0)), 'duet_gain_db'),
                       (dict(duet_gain_db=None), 'duet_gain_db')):
        with pytest.raises(HfttError, match='SynthPlay: ' + match):
            SynthPlay(**bad)


def test_synth_part_and_the_ops_argument_errors():
    import synth_emul as S
    from hftt_hip import HfttError, ops
    with pytest.raises(HfttError, match='SynthPart: play must be an ops.Warp'):
        ops.SynthPart([0], [0], [0], [1.0], play=object())
    with pytest.raises(HfttError, match=r'SynthPart: file, start, voice, gain and tune must be \[B\], got shapes'):
        ops.SynthPart([0, 1], [0], [0, 0], [1.0, 1.0])
    with pytest.raises(HfttError, match=r'SynthPart: file, start, voice, gain and tune must be \[B\], got shapes'):
        ops.SynthPart([0, 1], [0, 0], [0, 0], [1.0, 1.0], tune=[1 << 31])
    with pytest.raises(HfttError, match='SynthPart: the play holds 1 windows'):
        ops.SynthPart([0, 1], [0, 0], [0, 0], [1.0, 1.0], play=ops.Warp([1 << 24], [0]))
    part = ops.SynthPart([0, -1], [3, 0], [1, 0], [0.5, 1.0], tune=[(1 << 32) - 1, 1 << 31])
    assert part.file.dtype == part.start.dtype == part.voice.dtype == part.tune.dtype == torch.int32 and part.gain.dtype == torch.float32
    assert part.tune.tolist() == [-1, -(1 << 31)]                                               # uint32 values carried as int32 bits, like inc
    assert ops.tune_q31(0.0) == 1 << 31 and ops.tune_q31([1200.0])[0] == 1 << 32 and ops.tune_q31(50.0) == int(round(2.0 ** (50 / 1200.0) * 2.0 ** 31))

    table = ops.LabelsTable(ops.labels_table_host([[S.note(22, 0.1, 0.2)], []], S.config(5)), 'cpu')
    vb = ops.VoiceBank(device='cpu', **_bank())
    nsamp = torch.tensor([4000, 300])
    play = ops.Warp([1 << 23, 1 << 24, 1 << 25], [0, 513 << 23, 0])
    # synth_nsamp: n + ceil(t'(end) sr) - ceil(end sr); tempo 0.5 doubles the 3,200 samples in front of the last offset; a delay of 256.5 samples
    # adds 257; 0 for a file outside the table; and synth_frames
    n = ops.synth_nsamp(table, nsamp, [0, 0, 2], play)
    assert n.dtype == torch.int64 and n.tolist() == [4000 + 3200, 4000 + 257, 0]
    assert ops.synth_nsamp(table, nsamp, [1, 0, -1]).tolist() == [300, 4000, 0]
    assert ops.synth_frames(torch.tensor([7200, 255, 0, -1]), 256).tolist() == [29, 1, 1, 0]
    with pytest.raises(HfttError, match='synth_nsamp: table must be an ops.LabelsTable'):
        ops.synth_nsamp(None, nsamp, [0])
    with pytest.raises(HfttError, match='synth_nsamp: play must be an ops.Warp'):
        ops.synth_nsamp(table, nsamp, [0], play=3)
    with pytest.raises(HfttError, match=r'synth_nsamp: file_nsamp must be \[n_files=2\], got shape \(1,\)'):
        ops.synth_nsamp(table, nsamp[:1], [0])
    with pytest.raises(HfttError, match=r'synth_nsamp: win_file must be \[B\], got shape \(1, 1\)'):
        ops.synth_nsamp(table, nsamp, [[0]])
    with pytest.raises(HfttError, match='synth_nsamp: the warp holds 3 windows'):
        ops.synth_nsamp(table, nsamp, [0], play)
    # clip_synth: the new arguments' types and shapes, and no CPU fallback for the new launch either
    args = (table, nsamp, vb, [0], [0], [0], 16, 256, 16000.0)
    for kw in (dict(play=ops.Warp([1 << 24], [0])), dict(tune=[1 << 31]), dict(part=ops.SynthPart([1], [0], [0], [1.0])), dict(nsamp=[4000])):
        with pytest.raises(HfttError, match='no CPU fallback'):
            ops.clip_synth(*args, **kw)


def test_the_store_checks_play_and_the_nyquist_headroom():
    import synth_emul as S
    from corpus import synth_audio as SA
    from corpus.make_dataset import assemble_synth_store
    from hftt_hip import HfttError, ops
    from training.dataset import SynthClipStore, SynthPlay, WaveAugment
    config = S.config(5)
    store = assemble_synth_store([[S.note(22, 0.1, 0.5)]], config, 0)
    vb = ops.VoiceBank(device='cpu', **_bank())
    with pytest.raises(HfttError, match='play must be a SynthPlay'):
        SynthClipStore(store, config, 'cpu', vb, play=WaveAugment())
    with pytest.raises(HfttError, match='warps or mixes'):                                       # the old refusal stands next to a play
        SynthClipStore(store, config, 'cpu', vb, augment=WaveAugment(mix_p=0.25), play=SynthPlay())
    # a partial 1 cent under Nyquist: 2 cents of tuning reach it, half a cent does not; a silent partial may lie anywhere
    near = int(round(2.0 ** 31 * 2.0 ** (-1.0 / 1200.0)))
    with pytest.raises(HfttError, match='headroom_cents >= 2'):
        SynthClipStore(store, config, 'cpu', ops.VoiceBank(device='cpu', **_bank(inc=near)), play=SynthPlay(tune_cents=2.0))
    for bank, play in ((_bank(inc=near), SynthPlay(tune_cents=0.5)), (dict(_bank(inc=near), amp=np.zeros((2, 5, 3), np.float32)), SynthPlay(tune_cents=50.0)),
                       (_bank(inc=near), SynthPlay(transpose=(-2, 2)))):
        with pytest.raises(HfttError, match='the bank lives on'):                                # past the headroom check, to the next refusal
            SynthClipStore(store, config, 'meta', ops.VoiceBank(device='cpu', **bank), play=play)
    # synth_voice_bank leaves the headroom it is asked for, and changes nothing at 0
    cfg = SA.default_config()
    a, b, c = SA.synth_voice_bank(3, cfg, seed=3), SA.synth_voice_bank(3, cfg, seed=3, headroom_cents=0.0), SA.synth_voice_bank(3, cfg, seed=3, headroom_cents=50.0)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    on_a, on_c = a['amp'] != 0, c['amp'] != 0
    assert on_c.sum() < on_a.sum() and not (on_c & ~on_a).any() and not c['inc'][~on_c].any()
    top = int(ops.tune_q31(50.0))
    assert ((a['inc'][on_a].astype(np.int64) * top) >> 31).max() >= 1 << 31 > ((c['inc'][on_c].astype(np.int64) * top) >> 31).max()
    with pytest.raises(ValueError):
        SA.synth_voice_bank(2, cfg, seed=0, headroom_cents=-1.0)


def test_the_trainer_refuses_the_play_flags_without_the_synth_store():
    tool = os.path.join(util.ROOT, 'tools', 'train_config5.py')
    need = 'they need --synth-store'
    cases = ((['--synth-transpose', '-2', '2'], need), (['--synth-tune-cents', '10'], need), (['--synth-tempo', '0.9', '1.1'], need), (['--synth-shift'], need),
             (['--synth-play-p', '0.5'], need), (['--synth-duet-p', '0.3'], need), (['--wave-store', '--synth-duet-gain-db', '-6', '0'], need),
             (['--synth-store', '--synth-tempo', '0.1', '1.0'], 'SynthPlay: tempo'), (['--synth-store', '--synth-duet-p', '0.5', '--aug-mix-p', '0.5'], 'warps or mixes'))
    procs = [subprocess.Popen([sys.executable, tool] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for extra, _ in cases]
    for (extra, msg), p in zip(cases, procs):               # (side by side: each run is the interpreter's start-up and the parser)
        _, err = p.communicate(timeout=300)
        assert p.returncode == 2 and msg in err, (extra, err[-500:])
