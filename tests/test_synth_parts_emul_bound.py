"""What the GPU test of hftt_clip_synth_parts (tests/test_synth_parts_gpu.py) is worth, shown without a GPU on synth_parts_emul.py's restatement
of the header: the fp32 rounding chain with correctly rounded S and E stays inside the bound on EVERY sample of the GPU test's inputs, the time
map gives the bits the label walker of mix_emul.py forms, and the test's criteria reject the defects a kernel could have.  Which criterion
rejects which defect:
  the bound against fp64      sign of the partner offset flipped; partner cut at n'_A instead of n'_B; partner played with the primary's voice,
                              with the primary's release, with the primary's shift; time map applied to onsets only; tune shifted by 30 bits;
                              tune applied to the wrapped phase instead of inc; bank row p - k; rows outside the bank clamped instead of dropped
  the bits of t'              time map formed with one rounding (an fma): the labels' t' differ in the last place, and the host-prepared table
                              of the GPU test (times mapped in numpy, two roundings) no longer gives equal samples
  the cancelling duet         partner summed first (any order is inside a worst-case bound: the primary's record and the partner's first cancel
                              to the bit only when they are adjacent, which primary-first table order makes them)"""
import numpy as np
import pytest

import mix_emul as M
import synth_emul as S
import synth_parts_emul as P


def _worst(name, defect=None, only=None):
    """largest |fp32 emulation - fp64| / bound over the case's windows (only: window indices)"""
    table, bank, wins, t, rows = P.reference(name)
    worst, seen = 0.0, 0
    for b, (A, B) in enumerate(wins):
        if rows[b] is None or (only is not None and b not in only):
            continue
        ref, bound, terms = rows[b]
        got = P.render32_parts(table, bank, A, B, int(t['o'][b]), int(t['e'][b]), defect=defect)
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


@pytest.mark.parametrize('name', sorted(P.cases()))
def test_the_fp32_chain_stays_inside_the_bound_on_every_sample_of_the_gpu_inputs(name):
    worst = _worst(name)
    print('%s: largest error / bound of the fp32 chain %.3g' % (name, worst))
    assert worst <= 1.0


def test_the_inputs_hold_what_the_issue_asks_of_them():
    table, bank, wins, t, rows = P.reference('N5-H3')
    assert all(n >= 2 * S.TILE for n in P.FILE_NSAMP5[:4])                                       # files of at least two tiles
    # window 0: more than a filter pass of records sounds in one tile, the two parts together (and file 0 alone needs a second pass)
    A, B = wins[0]
    i = np.arange(S.TILE, 2 * S.TILE, dtype=np.int64)
    count = 0
    for recs, v, pos, n_part, _, _, v_rel, _ in P._parts(table, bank, A, B, i):
        rel = int(bank['release'][v_rel])
        count += sum(1 for on, D, _, _, _, _ in zip(*recs) if on < min(pos[-1] + 1, n_part) and on + D + rel > max(pos[0], 0))
    assert count > S.CHUNK and len(P.records_play(table, 0, P.IDENTITY)[0]) > S.CHUNK
    deltas = [B['start'] - A['start'] for A, B in wins[:3]]
    assert min(deltas) < 0 < max(deltas)                                                         # both signs of part_start - win_start
    # shifts +2 and -2 on files with all five pitches: notes leave the bank at both ends
    for (f, pl) in ((wins[0][0]['file'], wins[0][0]['play']), (wins[0][1]['file'], wins[0][1]['play'])):
        all_rows, kept = P.records_play(table, f, P.IDENTITY)[2], P.records_play(table, f, pl)[2]
        assert set(all_rows) == set(range(5)) and 0 < len(kept) < len(all_rows)
    assert wins[0][0]['play']['shift'] > 0 > wins[0][1]['play']['shift']
    A, B = wins[2]                                                                               # the partner ends inside the window: n'_B cuts it
    last = int(t['e'][2]) - 1 + (B['start'] - A['start']) * S.HOP
    assert B['nsamp'] < A['nsamp'] and last >= B['nsamp'] and max(on + D for on, D, _, _, _, _ in zip(*P.records_play(table, B['file'], B['play']))) > B['nsamp']


def test_records_play_forms_the_bits_of_t_that_the_label_walker_forms():
    """per output pitch and in list order, the walker's on_ms / off_ms are t' * 1000 of records_play's t', bit for bit -- and not with one rounding"""
    notes, N, _, _, _ = P.cases()['N5-H3']
    table, _, wins, _, _ = P.reference('N5-H3')
    config = S.config(N)
    differs = 0
    for A, B in wins[:2]:
        for part in (A, B):
            pl, f = part['play'], part['file']
            src = {'notes': notes[f], 'start': 0, 'shift': pl['shift'], 't_delay': pl['t_delay'], 't_scale': pl['t_scale']}
            per_pitch, _ = M.prepare(config, src)
            _, _, row, _, t_on, t_off = P.records_play(table, f, pl)
            bad = P.records_play(table, f, pl, defect='map_fma')
            for j in range(N):
                want = np.array([(x[2], x[3]) for x in per_pitch[j]], np.float64).reshape(-1, 2)
                got = np.stack([t_on[row == j] * 1000.0, t_off[row == j] * 1000.0], axis=1)
                assert np.array_equal(want.view(np.int64), got.view(np.int64)), (f, j)
            differs += int((bad[4] != t_on).sum() + (bad[5] != t_off).sum())
    assert differs > 0                                     # the one-rounding map is another function: the criterion sees it


# (defect, case, windows that show it)
DEFECTS = [('offset_sign', 'N5-H3', (0, 1)), ('cut_at_nA', 'N5-H3', (2,)), ('primary_voice', 'N5-H3', (0,)), ('primary_release', 'N5-H3', (0, 1, 2)),
           ('primary_shift', 'N5-H3', (0,)), ('map_onset_only', 'N5-H3', (0,)), ('tune_30', 'N5-H3', (0,)), ('tune_on_phase', 'N5-H1', (0,)),
           ('row_minus', 'N5-H3', (0,)), ('row_clamp', 'N5-H3', (0,))]


@pytest.mark.parametrize('defect,name,only', DEFECTS, ids=[d for d, _, _ in DEFECTS])
def test_the_bound_rejects(defect, name, only):
    clean, bad = _worst(name, None, only), _worst(name, defect, only)
    print('%s: largest error / bound %.3g clean, %.3g with the defect' % (defect, clean, bad))
    assert clean <= 1.0 < bad


def test_the_partner_summed_first_is_rejected_by_the_cancelling_duet():
    from hftt_hip.ops import labels_table_host
    bank, notes, nsamp = P.cancel_duet()
    table = labels_table_host(notes, S.config(3))
    A = {'file': 0, 'start': 0, 'voice': 0, 'play': P.IDENTITY, 'nsamp': nsamp[0]}
    B = {'file': 1, 'start': 0, 'voice': 1, 'play': P.IDENTITY, 'nsamp': nsamp[1], 'gain': 1.0}
    duet = P.render32_parts(table, bank, A, B, 0, nsamp[0])
    alone = S.render32(table, bank, 2, 1, 0, nsamp[2])
    assert np.array_equal(duet.view(np.int32), alone.view(np.int32)) and bool(alone.any())
    first = P.render32_parts(table, bank, A, B, 0, nsamp[0], defect='partner_first')
    assert not np.array_equal(first, alone)
    ref, bound, _ = P.render64_parts(table, bank, A, B, 0, nsamp[0])
    assert (np.abs(first.astype(np.float64) - ref) <= bound).all()                               # any order is inside a worst-case bound


def test_an_identity_play_is_synth_emul_itself():
    """render32_parts without a partner under the identity play == synth_emul.render32, bit for bit: the helper extends it, it is no second opinion"""
    table, bank, wins, t, _ = P.reference('N5-H3')
    for f, v in ((0, 2), (2, 0)):
        A = {'file': f, 'start': 0, 'voice': v, 'play': P.IDENTITY, 'nsamp': P.FILE_NSAMP5[f]}
        assert np.array_equal(P.render32_parts(table, bank, A, None, 2000, 6000).view(np.int32), S.render32(table, bank, f, v, 2000, 6000).view(np.int32))
        a, b = P.render64_parts(table, bank, A, None, 2000, 6000), S.render64(table, bank, f, v, 2000, 6000)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
