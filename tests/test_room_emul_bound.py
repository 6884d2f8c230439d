"""The room's emulator against itself (CPU): the pseudo-file tables of hftt_clip_room make a plain clip log-mel over the scratch rows see the
frames AND the fill columns of the whole wet file; and the worst-case bound the GPU test holds the kernel to is met by an fp32 numpy
convolution in forward and in reverse tap order -- it is no tighter than fp32 itself."""
import numpy as np
import pytest

import room_emul as R


def _wet_files(L=300, seed=5):
    r = np.random.RandomState(seed)
    h = (r.standard_normal(L) * np.exp(-np.arange(L) / 60.0)).astype(np.float32)
    return [R.wet_ref(w, h)[0] for w in R.corpus_waves()]


def _scratch(wet, n_prime, files, starts, width, hop=R.HOP):
    t = R.pseudo_tables(n_prime, starts, width, hop)
    span = R.span_of(width, hop)
    rows = np.full((len(files), span), np.nan)                # what the kernel does not write is never read
    for b, f in enumerate(files):
        if t['win_file'][b] >= 0:
            rows[b, :t['e'][b] - t['o'][b]] = wet[f][t['o'][b]:t['e'][b]]
    return rows.reshape(-1), t


def test_the_pseudo_files_show_the_whole_wet_file_for_the_six_windows():
    wet = _wet_files()
    files, starts = [f for f, _ in R.WINDOWS], [s for _, s in R.WINDOWS]
    n_prime = [R.LENS[f] if f >= 0 else -1 for f in files]
    rows, t = _scratch(wet, n_prime, files, starts, R.WIDTH)
    got = R.clip_frames(rows, t['samp0'], t['win_file'], t['win_start'])
    whole = np.concatenate(wet)
    samp0 = np.concatenate([[0], np.cumsum(R.LENS)])
    want = R.clip_frames(whole, samp0, files, starts)
    assert not np.isnan(got).any() and np.array_equal(got, want)
    # the windows are what they claim to be: frames and fill in the first two, all fill behind the end and without a file, one frame of the empty file
    fill = (want == R.FILL).all(axis=1)
    assert [int(f.sum()) for f in fill] == [3, 9, R.WIDTH, R.WIDTH - 3, R.WIDTH - 1, R.WIDTH]
    assert t['win_file'].tolist() == [0, 2, -1, 6, 8, -1] and t['win_start'].tolist() == [-3, 4, 4, 0, 0, 0]
    assert (np.diff(t['samp0']) >= 0).all() and t['samp0'][-1] == len(R.WINDOWS) * R.span_of()


@pytest.mark.parametrize('n', [0, 1, 255, 256, 1024, 1025, 2304])
def test_the_edges_of_the_mapping(n):
    """every window start around a file of n samples, o_b == n' and n' == 0 among them (n = 1024 at start 8, n = 0 at start 4 and 5)"""
    r = np.random.RandomState(n)
    wet = [r.uniform(-1, 1, n)]
    starts = list(range(-R.WIDTH - 1, n // R.HOP + 8))
    files = [0] * len(starts)
    rows, t = _scratch(wet, [n] * len(starts), files, starts, R.WIDTH)
    got = R.clip_frames(rows, t['samp0'], t['win_file'], t['win_start'])
    want = R.clip_frames(wet[0], [0, n], files, starts)
    assert not np.isnan(got).any() and np.array_equal(got, want)
    assert ((t['e'] - t['o']) <= R.span_of()).all()
    for b, s in enumerate(starts):                            # a shown frame never reads in front of o_b, unless o_b = 0
        assert t['o'][b] == 0 or (t['win_start'][b] * R.HOP - R.NFFT // 2 >= 0 and t['o'][b] % R.HOP == 0)


@pytest.mark.parametrize('L', [1, 5, 300, 2049, 4096])
def test_the_bound_is_no_tighter_than_fp32(L):
    r = np.random.RandomState(L)
    h = r.standard_normal(L).astype(np.float32)
    worst = 0.0
    for dry in R.corpus_waves()[:2]:
        ref, mag = R.wet_ref(dry, h)
        bound = R.wet_bound(mag, L)
        for reverse in (False, True):
            err = np.abs(R.wet_fp32(dry, h, reverse=reverse).astype(np.float64) - ref)
            assert (err <= bound).all(), (L, reverse, float((err / bound).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print('L = %d: largest fp32 error / bound %.3g' % (L, worst))
    assert L == 1 or worst > 0.0                               # (one tap, one product: exact against fp64 only by luck -- not asked)
