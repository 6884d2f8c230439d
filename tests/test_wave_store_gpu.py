"""training.dataset.WaveClipStore (a waveform corpus resident on the device; a batch's log-mel windows and labels computed when it is gathered)
against NoteClipStore on the same corpus, whose features are ops.LogMel of the same fp32 waveforms: three short plucked-string files at the
training geometry (32 + 128 + 32 frames, 256 bins, 88 notes), n_slice 1 and 3.  Labels bit-equal; spec within the sum of the two kernels' bounds
around the fp64 reference (tests/frontend_emul.py), fill cells equal; the int16 store bit-equal to a float32 store of the dequantised samples; the
augmentations change the spec and nothing else, reproducibly; TrainStep consumes the loader's batches."""
import functools

import numpy as np
import pytest
import torch

import util
import frontend_emul as FE

pytestmark = pytest.mark.gpu
NAMES = ('spec', 'onset', 'offset', 'mpe', 'velocity')
SECONDS = (2.0, 1.3, 0.7)


def _note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


@functools.lru_cache(maxsize=None)
def _corpus():
    """(config, fp32 waves, note lists): the last note of file 0 ends behind its audio (the label track is longer than the features)"""
    from corpus import synth_audio as SA
    from corpus.make_dataset import finalize_config, prepare_config
    config = finalize_config(prepare_config(SA.default_config()))
    r = np.random.RandomState(7)
    notes = []
    for dur in SECONDS:
        t, a = 0.05, []
        while t < dur - 0.2:
            a.append(_note(int(r.randint(40, 89)), t, t + float(r.uniform(0.1, 0.5)), int(r.randint(40, 110))))
            t += float(r.uniform(0.05, 0.2))
        notes.append(a)
    notes[0].append(_note(50, 1.9, 2.3, 90))
    waves = [SA.pluck_wave(a, dur=dur) for a, dur in zip(notes, SECONDS)]
    assert max(float(w.abs().max()) for w in waves) < 1.0
    return config, waves, notes


@functools.lru_cache(maxsize=None)
def _bounds():
    """per file: up + down [frames, n_mels] of frontend_emul's criterion (|a - b| of two kernels that each meet it)"""
    t = FE.logmel_tables()
    out = []
    for w in _corpus()[1]:
        up, down = FE.logmel_bound(FE.logmel_ref(w, t))
        out.append(up + down)
    return out


@pytest.fixture(scope='module')
def stores(dev):
    from corpus.make_dataset import assemble_note_store, assemble_wave_store
    from hftt_hip import ops
    config, waves, notes = _corpus()
    lm = ops.LogMel(dev)
    feats = [lm(w.to(dev)).cpu().numpy() for w in waves]
    return {'note': assemble_note_store(feats, notes, config), 'wave': assemble_wave_store([w.numpy() for w in waves], notes, config)}


def _edge_ids(store, n_slice):
    """the first and the last clip of every file (n_slice 1), and clips in between"""
    f = store['clip_file'][:len(store['clip_file']) // n_slice * n_slice][::n_slice]
    first = [int(np.argmax(f == k)) for k in range(3)]
    last = [int(len(f) - 1 - np.argmax(f[::-1] == k)) for k in range(3)]
    return sorted(set(first + last + [len(f) // 3, len(f) // 2]))


@pytest.mark.parametrize('n_slice', [1, 3])
def test_wave_store_against_the_note_store(dev, stores, n_slice):
    from training.dataset import NoteClipStore, WaveClipStore
    config = _corpus()[0]
    old = NoteClipStore(stores['note'], config, dev, n_slice)
    new = WaveClipStore(stores['wave'], config, dev, n_slice, wave_dtype='float32')
    assert len(new) == len(old) and new.resident_bytes() > 0
    ids = _edge_ids(stores['wave'], n_slice)
    assert len(ids) == 8
    a, b = old.batch(ids), new.batch(ids)
    assert len(a) == len(b) == 5
    for name, x, y in zip(NAMES, a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, name
        if name != 'spec':
            assert torch.equal(x, y), name
    assert int(a[3].sum()) > 0
    cin = config['input']
    fill = torch.tensor(cin['min_value'], dtype=torch.float32)
    file, frame = new.clip_file[ids].tolist(), new.clip_frame[ids].tolist()
    sa, sb = a[0].cpu(), b[0].cpu()
    worst, differ, valid_cells, fill_cells = 0.0, 0, 0, 0
    for i, (f, c) in enumerate(zip(file, frame)):
        bound = _bounds()[f]
        fr = c - cin['margin_b'] + torch.arange(sa.shape[2])
        v = (fr >= 0) & (fr < bound.shape[0])
        assert bool((sb[i][:, ~v] == fill).all()) and bool((sa[i][:, ~v] == fill).all()), (i, 'fill')
        err = (sa[i][:, v].double() - sb[i][:, v].double()).abs()
        assert bool((err <= bound[fr[v]].T).all()), (i, f, c)
        worst = max(worst, float((err / bound[fr[v]].T).max()))
        differ += int((sa[i][:, v] != sb[i][:, v]).sum()); valid_cells += int(v.sum()) * sa.shape[1]; fill_cells += int((~v).sum()) * sa.shape[1]
    assert valid_cells > 0 and fill_cells > 0
    print('n_slice %d: |wave store - note store| / (up + down) worst %.3f; %d of %d valid cells differ bitwise' % (n_slice, worst, differ, valid_cells))
    if n_slice == 1:
        assert new.resident_bytes() < old.resident_bytes()
        for kw in ({}, {'shuffle': True, 'seed': 5}, {'rank': 1, 'world': 2, 'drop_last': True}):
            la, lb = old.loader(4, **kw), new.loader(4, **kw)
            assert len(la) == len(lb) and all(torch.equal(x, y) for x, y in zip(la.chunks, lb.chunks)), kw


def test_int16_store_is_the_float32_store_of_the_dequantised_samples(dev, stores):
    from training.dataset import WaveClipStore
    config, waves, _ = _corpus()
    q = [torch.round(w.double() * 32768.0).clamp(-32768, 32767).to(torch.int16) for w in waves]
    s16 = WaveClipStore(dict(stores['wave'], waves=[x.numpy() for x in q]), config, dev)
    s32 = WaveClipStore(dict(stores['wave'], waves=[(x.float() * (1.0 / 32768.0)).numpy() for x in q]), config, dev, wave_dtype='float32')
    auto = WaveClipStore(stores['wave'], config, dev)            # fp32 waves stored as int16: the same quantisation
    assert s16.waves.wave.dtype == torch.int16 and s32.waves.wave.dtype == torch.float32 and torch.equal(auto.waves.wave, s16.waves.wave)
    assert 2 * s16.waves.wave.numel() == s16.waves.wave.numel() * s16.waves.wave.element_size() and s16.resident_bytes() < s32.resident_bytes()
    ids = _edge_ids(stores['wave'], 1)
    for x, y in zip(s16.batch(ids), s32.batch(ids)):
        assert torch.equal(x, y)


def test_augmentation_changes_the_spec_only_and_is_reproducible(dev, stores):
    from training.dataset import WaveAugment, WaveClipStore
    config = _corpus()[0]
    ids = _edge_ids(stores['wave'], 1)
    plain = WaveClipStore(stores['wave'], config, dev).batch(ids)

    def two(seed):
        s = WaveClipStore(stores['wave'], config, dev, augment=WaveAugment(gain_db=(-6.0, 6.0), noise_dbfs=(-60.0, -40.0), seed=seed))
        return s.batch(ids), s.batch(ids)
    a1, a2 = two(3)
    b1, b2 = two(3)
    c1, _ = two(4)
    assert not torch.equal(a1[0], a2[0]) and not torch.equal(a1[0], plain[0]) and not torch.equal(a1[0], c1[0])
    assert torch.equal(a1[0], b1[0]) and torch.equal(a2[0], b2[0])
    assert bool(torch.isfinite(a1[0]).all())
    for k in range(1, 5):
        assert torch.equal(a1[k], plain[k]) and torch.equal(a2[k], plain[k]), NAMES[k]
    # gain alone at 0 dB is no change at all: 10^0 = 1
    unit = WaveClipStore(stores['wave'], config, dev, augment=WaveAugment(gain_db=(0.0, 0.0))).batch(ids)
    assert torch.equal(unit[0], plain[0])


def test_train_step_takes_the_wave_store_loader(dev):
    from corpus import synth_audio as SA
    from corpus.make_dataset import assemble_wave_store
    from hftt_hip.trainer import TrainStep
    from training.dataset import WaveAugment, WaveClipStore
    c = util.MINI
    config = {'feature': {'mel_bins': c.n_bin, 'n_bins': c.n_bin, 'fft_bins': 2048, 'window_length': 2048, 'log_offset': 1e-8, 'sr': 16000, 'hop_sample': 256},
              'input': {'margin_b': c.n_margin, 'margin_f': c.n_margin, 'num_frame': c.n_frame, 'min_value': -18.420681, 'max_value': 0.0},
              'midi': {'note_min': 21, 'num_note': c.n_note, 'num_velocity': c.n_velocity}}
    notes = [[_note(21 + (3 * i) % c.n_note, 0.05 + 0.06 * i, 0.2 + 0.06 * i, 1 + i % (c.n_velocity - 1)) for i in range(10)], [_note(25, 0.1, 0.3, 5)]]
    waves = [SA.pluck_wave(a, dur=d).numpy() for a, d in zip(notes, (0.9, 0.5))]
    store = WaveClipStore(assemble_wave_store(waves, notes, config), config, dev, augment=WaveAugment(gain_db=(-3.0, 3.0), noise_dbfs=(-60.0, -50.0), seed=1))
    model = util.build_model(c, 5).to(dev)
    model.hftt_precision = 'x3'
    model.train()
    before = [p.detach().clone() for p in model.parameters()]
    step = TrainStep(model, lr=1e-4)
    losses = []
    for i, batch in enumerate(store.loader(2, shuffle=True, seed=2)):
        if i == 3:
            break
        assert batch[0].shape == (2, c.n_bin, c.n_frame + 2 * c.n_margin)
        losses.append(step(batch[0], *batch[1:]).clone())
    assert len(losses) == 3 and all(l.shape == (9,) and bool(torch.isfinite(l).all()) for l in losses)
    assert any(not torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before))


def test_a_cpu_store_raises(stores):
    from hftt_hip import HfttError
    from training.dataset import WaveClipStore
    with pytest.raises(HfttError):
        WaveClipStore(stores['wave'], _corpus()[0], 'cpu')
