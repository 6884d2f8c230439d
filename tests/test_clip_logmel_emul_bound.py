"""The per-cell criterion of tests/clip_logmel_emul.py separates right from wrong, without a GPU.

On every scene of the GPU test (tests/test_clip_logmel_gpu.py reads the same files, widths and windows) the restatement of hftt_clip_logmel --
frontend_emul.logmel_emul per file, the window / fill mapping, the int16 conversion, gain and noise -- passes the criterion: the bound
hftt_logmel already carries around the fp64 reference of the (mixed) file's waveform in every valid cell, the fill's bits in every other.
Each planted defect fails it on at least one scene.  Each test prints what it found (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

import util  # noqa: F401  (puts the package on the path)
import frontend_emul as FE
import clip_logmel_emul as CE

PLAIN, I16, GAIN, MIXED = 'plain', 'int16', 'gain', 'gain+noise'
MODES = {PLAIN: {}, I16: {'wave_i16': True}, GAIN: {'gain': CE.GAIN}, MIXED: {'gain': CE.GAIN, 'noise_std': CE.NOISE_STD, 'seed': CE.SEED}}


@functools.lru_cache(maxsize=None)
def _tables():
    return FE.logmel_tables()


@functools.lru_cache(maxsize=None)
def _waves(i16):
    return tuple(CE.quantize_i16(w) for w in CE.scene_waves()) if i16 else CE.scene_waves()


@functools.lru_cache(maxsize=None)
def _expect(width, k, mode):
    kw = MODES[mode]
    return CE.clip_logmel_expect(_waves(kw.get('wave_i16', False)), _tables(), CE.SCENES[width][k], width, **kw)


def _emul(width, k, mode, defect=None):
    kw = MODES[mode]
    return CE.clip_logmel_emul(_waves(kw.get('wave_i16', False)), _tables(), CE.SCENES[width][k], width, CE.FILL, defect=defect, **kw)


def test_the_scenes_cover_what_they_claim():
    assert sorted(n for _, n in CE.FILES) == [1, 255, 256, 257, 1023, 2047, 2304, 4219]
    assert CE.FILES[CE.SILENT - 1][0] == 'constant' and CE.FILES[CE.SILENT][0] == 'zeros'
    assert float(CE.scene_waves()[CE.SILENT - 1].abs().max()) == 1.0
    nf = [CE.n_frames(n) for _, n in CE.FILES]
    used = set()
    for width in CE.WIDTHS:
        kinds = set()
        for scene in CE.SCENES[width]:
            assert len(scene) == 5
            files = [f for f, _ in scene]
            if files != sorted(files):
                kinds.add('unordered')
            for i, (f, s) in enumerate(scene):
                used.add(f)
                if s < 0:
                    kinds.add('negative')
                if s + width <= 0:
                    kinds.add('before')
                if s >= nf[f]:
                    kinds.add('behind')
                if s < nf[f] <= s + width - 1 or (width == 1 and s == nf[f] - 1):
                    kinds.add('last frame')
                if any(g == f and max(s, t) < min(s, t) + width and max(s, t) < nf[f] for g, t in scene[:i]):
                    kinds.add('overlap')
                if f == CE.SILENT and s <= 0 < s + width:
                    kinds.add('silent frame 0')
        assert kinds >= {'unordered', 'negative', 'before', 'behind', 'last frame', 'overlap'}, (width, kinds)
        assert width == 1 or 'silent frame 0' in kinds
    assert used == set(range(len(CE.FILES))) and CE.WIDTHS == (1, 21, 192) and 1 % 16 and 21 % 16          # a run shorter than, and one not a multiple of, a workgroup's 16 frames


def test_the_noise_term_has_the_stated_moments_and_the_hash_is_the_dropout_hash():
    idx = np.arange(1 << 16, dtype=np.uint64)
    h = CE.hash_u32(CE.SEED, 3, idx)
    # byte (i & 3) of hash(i >> 2) against a threshold is keep_mask: the same words
    for p in (0.1, 0.5):
        thr = int((1.0 - float(np.float32(p))) * 256.0 + 0.5)
        field = (CE.hash_u32(CE.SEED, 3, idx >> np.uint64(2)) >> (np.uint32(8) * (idx & np.uint64(3)).astype(np.uint32))) & np.uint32(0xFF)
        assert np.array_equal(field < thr, util.keep_mask(CE.SEED, 3, idx, p))
    nz = CE.noise_term(CE.SEED, 3, idx, 1.0).astype(np.float64)
    print('noise term at std 1: mean %.4f, std %.4f over %d samples; C = %r' % (nz.mean(), nz.std(), len(nz), CE.NOISE_C))
    assert abs(nz.mean()) < 0.02 and abs(nz.std() - 1.0) < 0.02
    assert float(CE.NOISE_C).hex() == '0x1.bb688c0000000p-8'
    assert len(set(h.tolist())) > 0.99 * len(h)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('width', CE.WIDTHS)
def test_restatement_passes(width, mode):
    worst = 0.0
    for k in range(len(CE.SCENES[width])):
        exp = _expect(width, k, mode)
        got = _emul(width, k, mode)
        bad = CE.clip_logmel_check(got, exp, CE.FILL)
        assert not bad, (width, k, mode, bad)
        worst = max(worst, CE.clip_logmel_ratio(got, exp))
    print('width %3d %-10s worst error / bound %.3f' % (width, mode, worst))


def test_the_silent_file_sits_on_the_floor_to_the_bit():
    floor = torch.log(torch.tensor(FE.f32(FE.LOG_OFFSET), dtype=torch.float32))
    for width in (21, 192):
        f, s = CE.SCENES[width][0][0]
        assert f == CE.SILENT
        got = _emul(width, 0, PLAIN)[0]
        v = _expect(width, 0, PLAIN)['valid'][0]
        assert int(v.sum()) == CE.n_frames(CE.FILES[CE.SILENT][1]) and bool((got[:, v] == floor).all())
        bleed = _emul(width, 0, PLAIN, defect='neighbour_samples_at_border')[0]
        assert not bool((bleed[:, v] == floor).all())


def test_gain_and_int16_are_the_premixed_waveform_to_the_bit():
    """what the GPU test's torch.equal checks rest on: mixing is a statement about the samples, so a run WITH gain / noise equals a run WITHOUT
    on the waveform mixed beforehand.  (Shown here for the restatement; the noise of a file depends on the window through noise_std.)"""
    t = _tables()
    width, k = 21, 0
    wins = CE.SCENES[width][k]
    got = _emul(width, k, MIXED)
    for b, (f, s) in enumerate(wins):
        pre = list(CE.scene_waves())
        pre[f] = CE.mix(pre[f], f, CE.GAIN[b], CE.NOISE_STD[b], CE.SEED)
        assert torch.equal(CE.clip_logmel_emul(pre, t, [wins[b]], width, CE.FILL)[0], got[b])
    q = _waves(True)
    assert torch.equal(_emul(width, k, I16), CE.clip_logmel_emul([CE.dequantize(w) for w in q], t, wins, width, CE.FILL))


# defect -> the modes it can show in
DEFECT_MODES = {'neighbour_samples_at_border': (PLAIN,), 'frame_off_by_one': (PLAIN,), 'fill_on_the_wrong_side': (PLAIN,), 'last_frame_outside': (PLAIN,),
                'win_file_ignored': (PLAIN,), 'noise_keyed_clip_local': (MIXED,), 'noise_keyed_frame_local': (MIXED,), 'gain_after_noise': (MIXED,),
                'int16_scale_32767': (I16,)}


@pytest.mark.parametrize('defect', CE.DEFECTS)
def test_defect_fails(defect):
    hits = []
    for mode in DEFECT_MODES[defect]:
        for width in (1, 21):                           # (192 adds fill columns only: every file is shorter than 21 frames)
            for k in range(len(CE.SCENES[width])):
                bad = CE.clip_logmel_check(_emul(width, k, mode, defect=defect), _expect(width, k, mode), CE.FILL)
                hits.append('%s/%d/%d:%s' % (mode, width, k, '+'.join(sorted({b[0] for b in bad})) or '-'))
    print('    %-30s %s' % (defect, '  '.join(hits)))
    assert any(not h.endswith(':-') for h in hits), 'no scene sees ' + defect
