"""What the criterion of the streaming resampler resolves, on the CPU (no device): the carried-state model of tests/resample_stream_emul.py
against the whole-file model frontend_emul.resample_emul, for every rate of frontend_emul.RESAMPLE_RATES.

The criterion (criterion() below), per (rate, signal length, chunk size):
  * the concatenated outputs of all pushes and the close torch.equal resample_emul(whole signal);
  * promptness: every call produces exactly the count of ops.resample_stream_plan for the samples received so far;
  * the retained input never exceeds taps + down samples;
  * the frame schedule releases 1 + n_out // hop frames in total, and no frame in front of its last sample.
ops.resample_stream_plan itself is held against a brute force over all (n_in, n_done) up to 3 * down + taps: it may never release an output
that the prefix computes differently from the whole signal.  Each planted defect of the model must fail the criterion -- except the one listed
as unresolvable there, which is shown to be the same to the bit.
"""
import pytest
import torch

import frontend_emul as F
import resample_stream_emul as E

HOP, N_FFT = 16, 128          # the frame schedule is a function of (n_done, hop, n_fft): small ones, so that these short signals complete frames


def _signal(n, seed, i16=False):
    x = F.resample_noise(n, seed)
    return torch.round(x * 32768.0).clamp(-32768, 32767).to(torch.int16) if i16 else x


def _as_float(x):
    return x.float() * (1.0 / 32768.0) if x.dtype == torch.int16 else x


def criterion(sr, n, chunk, defect=None, i16=False):
    """the violations of one case, as strings (empty = pass)"""
    from hftt_hip import ops
    kern, up, down, width = F.resample_table(sr)
    taps = kern.shape[1]
    x = _signal(n, 7 * n + sr, i16)
    want = F.resample_emul(_as_float(x), kern, up, down, width)
    st = E.StreamEmul(kern, up, down, width, HOP, N_FFT, defect=defect)
    bad, outs, n_in = [], [], 0
    pieces = [x[i:i + chunk] for i in range(0, n, chunk)]
    for k, p in enumerate(pieces + [None]):
        closing = p is None
        n_in += 0 if closing else p.numel()
        _, count, _ = ops.resample_stream_plan(n_in, st.n_done, up, down, width, closing)
        out = st.close() if closing else st.push(p)
        outs.append(out)
        if out.numel() != count:
            bad.append('call %d: %d outputs, the plan says %d' % (k, out.numel(), count))
        if st.retained() > taps + down:
            bad.append('call %d: %d input samples retained (taps + down = %d)' % (k, st.retained(), taps + down))
    got = torch.cat(outs)
    if got.shape != want.shape or not torch.equal(got, want):
        bad.append('outputs differ from the whole-file model (%d vs %d samples)' % (got.numel(), want.numel()))
    frames, n_done = st.frame_log[-1]
    if frames != 1 + want.numel() // HOP:
        bad.append('%d frames in total, expected %d' % (frames, 1 + want.numel() // HOP))
    for k, (frames, n_done) in enumerate(st.frame_log[:-1]):
        if frames and (frames - 1) * HOP + N_FFT // 2 - 1 >= n_done:
            bad.append('call %d: frame %d released with %d samples' % (k, frames - 1, n_done))
    return bad


def _lengths(sr):
    kern, up, down, width = F.resample_table(sr)
    return F.resample_lengths(up, down, kern.shape[1]) + [3 * down + 2 * kern.shape[1] + 7]


@pytest.mark.parametrize('sr', F.RESAMPLE_RATES)
def test_every_chunking_gives_the_whole_file_model(sr):
    kern, up, down, width = F.resample_table(sr)
    for n in _lengths(sr):
        for chunk in sorted({1, 37, down, kern.shape[1], n}):
            assert criterion(sr, n, chunk) == [], (sr, n, chunk)


@pytest.mark.parametrize('sr', (44100, 8000))
def test_int16_chunks_are_converted_while_staged(sr):
    kern, up, down, width = F.resample_table(sr)
    n = 3 * down + 2 * kern.shape[1] + 7
    for chunk in (37, n):
        assert criterion(sr, n, chunk, i16=True) == [], (sr, chunk)


@pytest.mark.parametrize('sr', F.RESAMPLE_RATES)
def test_the_plan_never_releases_an_output_that_can_still_change(sr):
    from hftt_hip import ops
    kern, up, down, width = F.resample_table(sr)
    taps = kern.shape[1]
    top = 3 * down + taps
    x = F.resample_noise(top + taps + down, sr)
    first_diff = E.first_difference(x, kern, up, down, width, range(0, top + 1))
    tight = 0
    for n_in in range(top + 1):
        total = F.resample_n_out(n_in, up, down)
        for n_done in range(total + 1):
            first, count, keep = ops.resample_stream_plan(n_in, n_done, up, down, width, False)
            assert first == n_done and count >= 0
            assert n_done + count <= max(n_done, first_diff[n_in]), (n_in, n_done, count, first_diff[n_in])
            assert keep == min(n_in, max(0, ((n_done + count) // up) * down - width))
            f2, c2, _ = ops.resample_stream_plan(n_in, n_done, up, down, width, True)
            assert f2 == n_done and n_done + c2 == total
        tight += first_diff[n_in] - min(total, up * max(0, (n_in - width) // down))
    print('rate %d: the rule holds back %.1f outputs on average that already equal the whole signal\'s (trailing zeros of the table rows)' % (sr, tight / (top + 1)))


RESOLVED = [d for d in E.DEFECTS if d not in E.UNRESOLVABLE]


@pytest.mark.parametrize('defect', RESOLVED)
def test_each_planted_defect_fails_the_criterion(defect):
    hits = []
    for sr in (44100, 8000):
        kern, up, down, width = F.resample_table(sr)
        n = 3 * down + 2 * kern.shape[1] + 7
        for chunk in (37, down):
            if criterion(sr, n, chunk, defect=defect, i16=defect.startswith('i16')):
                hits.append((sr, chunk))
    assert {(44100, 37), (44100, 441)} <= set(hits), (defect, hits)       # (at 8000 -> 16000 the outermost taps of the rows are zero: a sample short there can go unseen)


def test_a_power_of_two_scale_behind_the_sum_is_the_same_to_the_bit():
    """the int16 scale applied after the sum: 2^-15 commutes with every fmaf and addition of the tap loop (nothing here is subnormal), so no
    criterion on the outputs can tell it from the kernel's order -- shown, not assumed"""
    for d in E.UNRESOLVABLE:
        kern, up, down, width = F.resample_table(44100)
        assert criterion(44100, 3 * down + 2 * kern.shape[1] + 7, 37, defect=d, i16=True) == []
