"""The device label renderer (csrc/labels.hip: hftt_labels_render; corpus.conv_note2label.note2label_device; training.dataset.NoteClipStore)
against the host function it restates: corpus.conv_note2label.note2label_arrays, which tests/golden/labels.npz pins to the reference's
note2label.  Everything is compared bit for bit (np.array_equal / torch.equal)."""
import numpy as np
import pytest
import torch

import util

pytestmark = pytest.mark.gpu

TRACKS = ('mpe', 'onset', 'offset', 'velocity')
DTYPES = {'mpe': np.bool_, 'onset': np.float32, 'offset': np.float32, 'velocity': np.int8}


def _cfg(sr=16000, hop=256, N=88, note_min=21):
    return {'feature': {'sr': sr, 'hop_sample': hop}, 'midi': {'note_min': note_min, 'num_note': N}}


def _note(pitch, onset, offset, velocity=64):
    return {'pitch': pitch, 'onset': onset, 'offset': offset, 'velocity': velocity}


def _same(dev, cfg, notes, flag=False):
    """note2label_device == note2label_arrays in dtype, shape and every element; returns the host arrays"""
    from corpus.conv_note2label import note2label_arrays, note2label_device
    host = note2label_arrays(cfg, notes, flag)
    got = note2label_device(cfg, notes, flag, dev)
    assert set(got) == set(TRACKS)
    for k in TRACKS:
        a = got[k].cpu().numpy()
        assert a.dtype == host[k].dtype == DTYPES[k] and a.shape == host[k].shape, (k, a.dtype, a.shape, host[k].shape)
        assert np.array_equal(a, host[k]), (k, int((a != host[k]).sum()), np.argwhere(a != host[k])[:5].tolist())
    return host


def _host_windows(cfg, files, flag, win_file, win_start, length):
    """the windows of a render request cut out of the host labels of whole files (zero outside a file)"""
    from corpus.conv_note2label import note2label_arrays
    labs = [note2label_arrays(cfg, a, flag) for a in files]
    out = {k: np.zeros((len(win_file), length, cfg['midi']['num_note']), DTYPES[k]) for k in TRACKS}
    for b, (fi, s) in enumerate(zip(win_file, win_start)):
        n = labs[fi]['mpe'].shape[0]
        lo, hi = max(s, 0), min(s + length, n)
        if lo < hi:
            for k in TRACKS:
                out[k][b, lo - s:hi - s] = labs[fi][k][lo:hi]
    return out


def _render_equals_host(dev, cfg, files, flag, win_file, win_start, length):
    from hftt_hip import ops
    table = ops.labels_table(files, cfg, dev)
    ref = _host_windows(cfg, files, flag, win_file, win_start, length)
    wf = torch.tensor(win_file, dtype=torch.int32, device=dev)
    ws = torch.tensor(win_start, dtype=torch.int32, device=dev)
    store = ops.labels_render(table, wf, ws, length, form='store', duration_tolerance=flag)
    train = ops.labels_render(table, wf, ws, length, form='train', duration_tolerance=flag)
    again = ops.labels_render(table, wf, ws, length, form='train', duration_tolerance=flag)
    for k, s, t, t2 in zip(('onset', 'offset', 'mpe', 'velocity'), store, train, again):
        assert s.dtype == {'onset': torch.float32, 'offset': torch.float32, 'mpe': torch.bool, 'velocity': torch.int8}[k]
        assert t.dtype == {'onset': torch.float32, 'offset': torch.float32, 'mpe': torch.float32, 'velocity': torch.int64}[k]
        a = s.cpu().numpy()
        assert a.shape == ref[k].shape and np.array_equal(a, ref[k]), (k, int((a != ref[k]).sum()), np.argwhere(a != ref[k])[:5].tolist())
        assert torch.equal(t, s.long() if k == 'velocity' else s.float()), k          # the train form is the store form, converted
        assert torch.equal(t, t2), k                                                 # and a launch repeats itself bit for bit
    return ref


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the reference pin
@pytest.mark.parametrize('case', [0, 1])
@pytest.mark.parametrize('flag', [False, True])
def test_reference_goldens(dev, case, flag):
    from corpus.conv_note2label import note2label_device
    g = util.golden('labels')
    notes = [_note(int(r[0]), float(r[1]), float(r[2]), int(r[3])) for r in g['c%d.notes' % case]]
    got = note2label_device(_cfg(), notes, flag, dev)
    for k in TRACKS:
        ref = g['c%d.%d.%s' % (case, int(flag), k)]
        a = got[k].cpu().numpy()
        assert a.dtype == ref.dtype and a.shape == ref.shape == ((463, 88), (860, 88))[case], (k, a.dtype, a.shape)
        assert np.array_equal(a, ref), (k, int((a != ref).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. adversarial cases against note2label_arrays
def test_list_order_decides_the_velocity_where_onsets_overlap(dev):
    a, b = _note(60, 1.000, 1.5, 40), _note(60, 1.040, 1.6, 90)
    ab, ba = _same(dev, _cfg(), [a, b]), _same(dev, _cfg(), [b, a])
    assert int((ab['velocity'] != ba['velocity']).sum()) == 2 and np.array_equal(ab['onset'], ba['onset'])


def test_a_velocity_of_zero_leaves_the_cell_open(dev):
    '''the rule in front of the onset frame tests the VALUE velocity == 0, not "written": the later note fills the frames the first left at 0'''
    a, b = _note(60, 1.000, 1.5, 0), _note(60, 1.040, 1.6, 90)
    zero = _same(dev, _cfg(), [a, b])
    one = _same(dev, _cfg(), [dict(a, velocity=1), b])
    p = 60 - 21
    assert set(zero['velocity'][:, p].tolist()) == {0, 90}
    assert ((zero['velocity'][:, p] == 90) & (one['velocity'][:, p] == 1)).any()        # a cell that a written 1 keeps and an open 0 loses


def test_exact_restrike_and_one_ulp_near_miss(dev):
    first, second = _note(60, 0.2, 0.5, 50), _note(60, 0.5, 0.9, 60)
    exact = _same(dev, _cfg(), [first, second])
    near = _same(dev, _cfg(), [dict(first, offset=float(np.nextafter(0.5, 1))), second])
    assert exact['offset'][:, 39].sum() == 1.75 and near['offset'][:, 39].sum() == 4.75
    _same(dev, _cfg(), [second, first])                           # the restruck note later in the list


@pytest.mark.parametrize('k', [10, 11, 100])
def test_half_frame_onset_holds_exactly_one_half(dev, k):
    '''an onset half way between two frames: frames k - 1 and k + 2 hold exactly 0.5 and carry the velocity (>= 0.5, not > 0.5)'''
    lab = _same(dev, _cfg(), [_note(21, (k + 0.5) * 0.016, (k + 20) * 0.016, 7)])
    assert lab['onset'][k - 1, 0] == 0.5 == lab['onset'][k + 2, 0]
    assert lab['velocity'][k - 1, 0] == 7 == lab['velocity'][k + 2, 0] and lab['velocity'][k - 2, 0] == 0 == lab['velocity'][k + 3, 0]


def test_triangles_are_clipped_to_the_file(dev):
    one = _same(dev, _cfg(), [_note(21, 0.0, 0.0, 5)], True)                               # a zero-length note at t = 0: one frame
    assert one['mpe'].shape == (1, 88) and one['onset'][0, 0] == 1.0 and one['velocity'][0, 0] == 5 and one['offset'][0, 0] == 0.0
    for flag in (False, True):
        last = _same(dev, _cfg(), [_note(30, 0.1, 1.0, 9), _note(40, 3.18, 3.2, 11), _note(40, 3.19, 3.2, 12)], flag)
        assert last['mpe'].shape[0] == 201 and last['offset'][200, 19] == 1.0 and last['mpe'][200, 19]
    # duration tolerance: the offset triangle of a 30 s note covers 376 frames of a 1,939-frame file, more than one 256-frame chunk
    long = _same(dev, _cfg(), [_note(30, 1.0, 31.0, 9)], True)
    assert long['offset'].shape[0] == 1939 and int((long['offset'][:, 9] > 0).sum()) == 376
    assert int((_same(dev, _cfg(), [_note(30, 1.0, 31.0, 9)], False)['offset'][:, 9] > 0).sum()) == 4      # 1935 .. 1938: the file ends there


@pytest.mark.parametrize('sr,hop,N,tol', [(16000, 160, 88, 5), (44100, 512, 88, 4), (16000, 256, 6, 3), (16000, 256, 128, 3)])
@pytest.mark.parametrize('flag', [False, True])
def test_other_grids(dev, sr, hop, N, tol, flag):
    from hftt_hip import ops
    cfg = _cfg(sr, hop, N, note_min=0 if N == 128 else 21)
    assert ops.labels_grid(cfg)[2] == tol
    r = np.random.RandomState(sr + hop + N)
    lo = cfg['midi']['note_min']
    notes = []
    for _ in range(120):
        on = float(r.uniform(0, 5.0))
        notes.append(_note(int(r.randint(lo, lo + N)), on, on + float(r.choice([0.0, 0.03, 0.3, 1.7])), int(r.randint(0, 128))))
    notes += [_note(lo, 1.0, 2.0, 3), _note(lo, 2.0, 2.5, 4), _note(lo + N - 1, 0.0, 7.0, 127)]      # a restrike; the last pitch up to the last frame
    lab = _same(dev, cfg, notes, flag)
    assert lab['mpe'][:, N - 1].all() and lab['velocity'].max() == 127


def test_one_pitch_with_more_notes_than_a_filter_chunk(dev):
    '''700 short notes of one pitch (the filter passes hold 256): the whole file, and a window in the middle of it'''
    r = np.random.RandomState(7)
    on = r.uniform(0.0, 20.0, 700)
    notes = [_note(64, float(t), float(t) + float(d), int(v)) for t, d, v in zip(on, r.uniform(0.0, 0.2, 700), r.randint(0, 128, 700))]
    notes += [_note(65, 3.0, 4.0, 1)]
    for flag in (False, True):
        _same(dev, _cfg(), notes, flag)
        _render_equals_host(dev, _cfg(), [notes], flag, [0, 0], [600, 601], 130)


def test_windows(dev):
    '''negative starts, windows that straddle the end of a file or lie wholly beyond it, a file and a pitch without notes, two files in one
    request in mixed order, a window longer than one chunk of frames'''
    cfg = _cfg(N=6)
    r = np.random.RandomState(3)
    f0 = [_note(int(r.choice([21, 22, 24, 26])), float(t), float(t) + float(d), int(v))
          for t, d, v in zip(r.uniform(0, 6.0, 60), r.uniform(0, 0.6, 60), r.randint(0, 128, 60))]
    f2 = [_note(26, 0.05, 0.4, 100), _note(21, 0.3, 4.9, 20), _note(21, 0.3, 0.31, 30)]
    files = [f0, [], f2]
    n0, n2 = (int(max(n['offset'] for n in a) * 62.5 + 0.5) + 1 for a in (f0, f2))
    win_file = [2, 0, 1, 0, 2, 0, 0, 1, 2, 0]
    win_start = [-3, -40, 0, n0 - 5, n2 - 1, n0, n0 + 1000, -7, 0, 100]
    for length in (8, 37, 300):
        for flag in (False, True):
            ref = _render_equals_host(dev, cfg, files, flag, win_file, win_start, length)
            assert not ref['mpe'][2].any() and not ref['onset'][6].any() and ref['mpe'][1].any() == (length > 40)
            assert not ref['mpe'][:, :, 23 - 21].any()                      # a pitch without notes
    assert ref['mpe'][0].any() and ref['mpe'][3].any() and ref['mpe'][9].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. store parity
MICRO_DS = {'feature': {'mel_bins': 16, 'n_bins': 16, 'log_offset': 1e-8, 'sr': 16000, 'hop_sample': 256},
            'input': {'margin_b': 4, 'margin_f': 4, 'num_frame': 8, 'min_value': -18.420681, 'max_value': 0.0},
            'midi': {'note_min': 21, 'num_note': 6, 'num_velocity': 8}}


def _random_notes(r, seconds, n, cm):
    out = []
    for _ in range(n):
        on = float(r.uniform(0, seconds))
        out.append(_note(int(r.randint(cm['note_min'], cm['note_min'] + cm['num_note'])), on, min(seconds, on + float(r.uniform(0, 0.4))),
                         int(r.randint(0, cm['num_velocity']))))
    return out


def _two_stores(dev, config, frames, seconds, n_notes, seed=11):
    from corpus.conv_note2label import note2label_arrays
    from corpus.make_dataset import assemble_note_store, assemble_store
    from training.dataset import DeviceClipStore, MyDataset, NoteClipStore
    r = np.random.RandomState(seed)
    notes = [_random_notes(r, s, n_notes, config['midi']) for s in seconds]
    feats = [r.randn(n, config['feature']['mel_bins']).astype(np.float32) for n in frames]
    dense = assemble_store(feats, [note2label_arrays(config, a) for a in notes], config)
    sparse = assemble_note_store(feats, notes, config)
    ds = MyDataset.from_arrays(dense['feature'], dense['label_onset'], dense['label_offset'], dense['label_mpe'], dense['label_velocity'],
                               dense['idx'], config, 1)
    return dense, sparse, DeviceClipStore(ds, dev), NoteClipStore(sparse, config, dev)


def test_note_store_equals_the_label_store(dev):
    '''two files at the MICRO_DS geometry: the labels of the first are longer than its features (0.8 s = 51 frames against 40), those of the
    second shorter (0.3 s = 20 frames against 33)'''
    dense, sparse, old, new = _two_stores(dev, MICRO_DS, frames=(40, 33), seconds=(0.8, 0.3), n_notes=25)
    assert sparse['table']['file_nframe'][0] > 40 and sparse['table']['file_nframe'][1] < 33
    assert np.array_equal(sparse['idx'], dense['idx']) and sparse['idx'].dtype == dense['idx'].dtype
    assert np.array_equal(sparse['feature'], dense['feature']) and sparse['feature'].dtype == dense['feature'].dtype
    assert sparse['file_row0'].tolist() == [4, 4 + int(sparse['table']['file_nframe'][0]) + 11]
    assert len(new) == len(old) == len(dense['idx'])
    seen = 0
    for i in range(0, len(old), 5):                                # batches of 5: the last one is partial
        ids = list(range(i, min(i + 5, len(old))))
        a, b = old.batch(ids), new.batch(ids)
        assert len(a) == len(b) == 5
        for name, x, y in zip(('spec', 'onset', 'offset', 'mpe', 'velocity'), a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (name, ids)
        seen += int(a[3].sum())
    assert seen > 0 and len(old) % 5 != 0
    assert new.resident_bytes() < sum(t.numel() * t.element_size() for t in (old.feature, old.label_onset, old.label_offset, old.label_mpe, old.label_velocity))
    for kw in ({}, {'shuffle': True, 'seed': 5}, {'rank': 1, 'world': 2}, {'rank': 2, 'world': 3, 'shuffle': True, 'seed': 9, 'drop_last': True},
               {'drop_last': True}):
        la, lb = old.loader(4, **kw), new.loader(4, **kw)
        assert len(la) == len(lb) and all(torch.equal(x, y) for x, y in zip(la.chunks, lb.chunks)), kw
    first = next(iter(new.loader(4, shuffle=True, seed=5)))
    for x, y in zip(first, old.batch(old.loader(4, shuffle=True, seed=5).chunks[0])):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the tuple is consumed unchanged
def test_train_step_takes_the_rendered_batch(dev):
    from hftt_hip.trainer import TrainStep
    c = util.MINI
    config = {'feature': {'mel_bins': c.n_bin, 'n_bins': c.n_bin, 'log_offset': 1e-8, 'sr': 16000, 'hop_sample': 256},
              'input': {'margin_b': c.n_margin, 'margin_f': c.n_margin, 'num_frame': c.n_frame, 'min_value': -18.420681, 'max_value': 0.0},
              'midi': {'note_min': 21, 'num_note': c.n_note, 'num_velocity': c.n_velocity}}
    _, _, old, new = _two_stores(dev, config, frames=(70,), seconds=(1.0,), n_notes=40)
    ids = [3, 20, 41, 55]
    losses = []
    for store in (old, new):
        model = util.build_model(c, 5).to(dev)
        model.hftt_precision = 'x3'
        model.train()
        batch = store.batch(ids)
        losses.append(TrainStep(model, lr=1e-4)(batch[0], *batch[1:]).clone())
    assert losses[0].shape == (9,) and torch.isfinite(losses[0]).all() and torch.equal(losses[0], losses[1])
