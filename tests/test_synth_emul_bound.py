"""What the GPU test of hftt_clip_synth (tests/test_synth_gpu.py) is worth, shown without a GPU on synth_emul.py's restatement of the header:
the fp32 rounding chain with correctly rounded S and E stays inside the bound on EVERY sample of the GPU test's inputs, and the test's criteria
reject the defects a kernel could have.  Which criterion rejects which defect:
  the bound against fp64      phase accumulated in fp32 (tau ~ 10 s), onset one sample late, release ignored, release decay from the onset,
                              velocity curve read at the pitch, a neighbouring file's record, a record dropped behind a full filter pass
  equal windows, bit for bit  a value that depends on the tile origin (a rotation recurrence anchored at the tile: two windows disagree wherever they meet)
  the cancelling pair         summation in time order (any order is inside a worst-case bound: the pair cancels to the bit only when its two
                              terms are adjacent, which table order makes them)"""
import numpy as np
import pytest

import synth_emul as S


def _worst(name, defect=None, only=None):
    """largest |fp32 emulation - fp64| / bound over the case's windows (only: window indices)"""
    table, bank, t, rows = S.reference(name)
    _, _, _, _, windows, _ = S.cases()[name]
    worst, seen = 0.0, 0
    for b, (f, _, v) in enumerate(windows):
        if rows[b] is None or (only is not None and b not in only):
            continue
        ref, bound, terms = rows[b]
        got = S.render32(table, bank, f, v, int(t['o'][b]), int(t['e'][b]), defect=defect)
        silent = terms == 0
        if defect is None:
            assert (got[silent] == 0).all() and not np.signbit(got[silent]).any()
        err = np.abs(got.astype(np.float64) - ref)
        live = ~silent
        if live.any():
            worst = max(worst, float((err[live] / bound[live]).max()))
        if silent.any() and float(err[silent].max()) > 0.0:
            worst = np.inf
        seen += len(got)
    assert seen > 0
    return worst


@pytest.mark.parametrize('name', sorted(S.cases()))
def test_the_fp32_chain_stays_inside_the_bound_on_every_sample_of_the_gpu_inputs(name):
    worst = _worst(name)
    print('%s: largest error / bound of the fp32 chain %.3g' % (name, worst))
    assert worst <= 1.0


# (defect, case, windows that show it): the crowd is window 2, the far window of file 3 is window 3, file 3's end window 4, file 1 is window 1
DEFECTS = [('phase_fp32', 'N5-H3-lead0', (3,)), ('onset_late', 'N5-H3-lead0', (1,)), ('no_release', 'N5-H3-lead0', (1,)),
           ('rel_from_onset', 'N5-H3-lead0', (1,)), ('vel_by_pitch', 'N5-H3-lead0', (1,)), ('leak', 'N5-H3-lead0', (1,)),
           ('drop_overflow', 'N5-H1-lead0', (2,))]


@pytest.mark.parametrize('defect,name,only', DEFECTS, ids=[d for d, _, _ in DEFECTS])
def test_the_bound_rejects(defect, name, only):
    clean, bad = _worst(name, None, only), _worst(name, defect, only)
    print('%s: largest error / bound %.3g clean, %.3g with the defect' % (defect, clean, bad))
    assert clean <= 1.0 < bad


def test_a_tile_anchored_recurrence_is_rejected_by_the_equality_of_overlapping_windows():
    table, bank, t, rows = S.reference('N5-H3-lead0')
    f, v = 1, 1
    a = S.render32(table, bank, f, v, 0, 5888, defect='tile_origin', origin=0)
    b = S.render32(table, bank, f, v, 1024, 5888, defect='tile_origin', origin=1024)          # the same samples from a window four frames later
    clean_a, clean_b = S.render32(table, bank, f, v, 0, 5888), S.render32(table, bank, f, v, 1024, 5888)
    assert np.array_equal(clean_a[1024:], clean_b) and not np.array_equal(a[1024:], b)


def test_summation_in_time_order_is_rejected_by_the_cancelling_pair():
    from hftt_hip.ops import labels_table_host
    bank, notes, nsamp = S.cancel_case()
    table = labels_table_host(notes, S.config(3))
    with_pair, alone = S.render32(table, bank, 0, 0, 0, nsamp[0]), S.render32(table, bank, 1, 0, 0, nsamp[1])
    assert np.array_equal(with_pair.view(np.int32), alone.view(np.int32)) and bool(alone.any())
    timed = S.render32(table, bank, 0, 0, 0, nsamp[0], defect='time_order')
    assert not np.array_equal(timed, alone)
    ref, bound, _ = S.render64(table, bank, 0, 0, 0, nsamp[0])
    assert (np.abs(timed.astype(np.float64) - ref) <= bound).all()                               # any order is inside a worst-case bound


def test_the_pseudo_file_tables_with_a_lead_of_zero_are_the_rooms():
    import room_emul as R
    n_prime, starts = [9000, 9000, 700, 0, -1, 9000], [-3, 25, 0, 0, 0, 40]
    a, b = S.pseudo_tables(n_prime, starts, width=20), R.pseudo_tables(n_prime, starts, width=20)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    c = S.pseudo_tables(n_prime, starts, width=20, lead=3)
    assert c['o'].tolist() == [0, (25 - 7) * 256, 0, 0, 0, (40 - 7) * 256] and c['win_start'].tolist() == [-3, 7, 0, 0, 0, 7]
    assert S.span_of(16) == 5888 == 2 * S.TILE + 1792 and S.span_of(16, 3) == 3 * S.TILE + 512
