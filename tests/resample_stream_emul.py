"""The carried-state resampler, hftt_resample_stream (csrc/resample_stream.hip) with its host side (ops.resample_stream / ops.stream_logmel), as
a torch model on the host, statement for statement: push(chunk) / close() per stream.

The model keeps what the host keeps -- the counters and the input samples from ops.resample_stream_plan's retention index on --, stages each
call's window from that tail (zeros in front of sample 0 and, at a close, behind the last sample) and runs the accumulation of
frontend_emul.resample_emul on it: that function is imported, not restated.  It is handed a local signal whose sample 0 is a multiple of
`down` of the stream's timeline, so that a local output's phase o % up and window are the absolute ones; the local outputs in front of the
first one asked for are dropped.  The frame schedule of ops.stream_frames_plan rides along: frames_done after each call.

defect=<name> selects one deliberately wrong variant (tests/test_resample_stream_emul_bound.py shows that the criterion resolves each).
"""
import torch

from frontend_emul import resample_emul, resample_n_out

DEFECTS = ('phase_restarts_each_push', 'tail_one_short', 'count_ignores_width', 'close_drops_zero_tail', 'close_floor',
           'i16_scale_32767', 'i16_scale_after_sum')
# 'i16_scale_after_sum' -- the raw int16 values summed, the result scaled by 1 / 32768 -- is kept as a NEGATIVE control: 2^-15 is a power of
# two, so the scale commutes with every fmaf and every addition of the tap loop as long as nothing enters the subnormal range, and the result
# is the same to the bit.  No criterion on the outputs resolves it, and no kernel that did it would be wrong.  'i16_scale_32767' is the
# neighbouring mistake that does change the values.
UNRESOLVABLE = ('i16_scale_after_sum',)


def plan(n_in, n_done, up, down, width, closing, defect=None):
    """ops.resample_stream_plan, or one of its planted defects"""
    from hftt_hip import ops
    if defect == 'count_ignores_width' and not closing:
        total = resample_n_out(n_in, up, down)
        count = max(0, min(total, up * (n_in // down)) - n_done)
        return n_done, count, min(n_in, max(0, ((n_done + count) // up) * down - width))
    if defect == 'close_drops_zero_tail':
        closing = False
    if defect == 'close_floor' and closing:
        count = max(0, n_in * up // down - n_done)
        return n_done, count, n_in
    return ops.resample_stream_plan(n_in, n_done, up, down, width, closing)


def frames_plan(n_done, frames, closed, hop, n_fft):
    from hftt_hip import ops
    return ops.stream_frames_plan(n_done, frames, closed, hop, n_fft)


class StreamEmul:
    """one stream: kern fp32 [up, taps]; chunks fp32 or int16 (then converted while the window is staged, (float)s * (1 / 32768))"""

    def __init__(self, kern, up, down, width, hop=256, n_fft=2048, defect=None):
        assert defect is None or defect in DEFECTS
        self.kern, self.up, self.down, self.width, self.taps = kern, up, down, width, kern.shape[1]
        self.hop, self.n_fft, self.defect = hop, n_fft, defect
        self.n_in = self.n_done = self.in0 = self.frames = 0
        self.tail = None                       # input samples in0 .. n_in, in the dtype they came in
        self.closed = False
        self.frame_log = []                    # (frames released so far, n_done) after each call

    def retained(self):
        return 0 if self.tail is None else self.tail.numel()

    def _stage(self, a0):
        """fp32 samples a0 .. n_in of the stream's timeline: the tail where it has them, zeros elsewhere"""
        local = torch.zeros(self.n_in - a0)
        if self.tail is not None and self.tail.numel():
            lo = max(self.in0, a0)
            t = self.tail[lo - self.in0:]
            if t.dtype == torch.int16:
                if self.defect == 'i16_scale_after_sum':
                    t = t.float()
                else:
                    t = t.float() * (1.0 / (32767.0 if self.defect == 'i16_scale_32767' else 32768.0))
            local[lo - a0:] = t
        return local

    def _step(self, chunk, closing):
        assert not self.closed
        if chunk is not None and chunk.numel():
            self.tail = chunk.clone() if self.tail is None or self.tail.numel() == 0 else torch.cat([self.tail, chunk])
            self.n_in += chunk.numel()
        up, down, width = self.up, self.down, self.width
        first, count, keep = plan(self.n_in, self.n_done, up, down, width, closing, self.defect)
        out = torch.zeros(0)
        if count:
            f0, m = first // up, -(-width // down)
            a0 = (f0 - m) * down                                   # local sample 0: a multiple of down, at least `width` in front of the window
            j0 = first - (f0 - m) * up
            if self.defect == 'phase_restarts_each_push':          # the retained tail resampled as a file of its own: its first sample is "sample 0"
                a0, j0 = self.in0, 0                               # (a live stream releases whole frames, so first % up is 0: what restarts is the position inside the input frame)
            loc = resample_emul(self._stage(a0), self.kern, up, down, width)
            out = loc[j0:j0 + count]
            assert out.numel() == count or self.defect is not None, (out.numel(), count)
            out = torch.cat([out, torch.zeros(count - out.numel())])
            if self.defect == 'i16_scale_after_sum' and self.tail is not None and self.tail.dtype == torch.int16:
                out = out * (1.0 / 32768.0)
        self.n_done = first + count
        if self.defect == 'tail_one_short':
            keep = min(self.n_in, keep + 1)
        if self.tail is not None:
            self.tail = self.tail[keep - self.in0:]
        self.in0 = keep
        self.closed = closing
        _, self.frames = frames_plan(self.n_done, self.frames, closing, self.hop, self.n_fft)
        self.frame_log.append((self.frames, self.n_done))
        return out

    def push(self, chunk):
        return self._step(chunk, False)

    def close(self):
        return self._step(None, True)


def first_difference(x, kern, up, down, width, ns, batch=64):
    """Brute force for the plan: for every prefix length n of ns, the first output index at which resample_emul(x[:n]) differs from
    resample_emul(x) (n_out of the prefix when none does).  The prefixes of a batch are laid side by side in one signal, each starting at a
    multiple of `down` and followed by at least taps + down zeros -- the zeros every prefix sees beyond its end --, so one call of
    resample_emul computes them all; prefix outputs are then cut out at the matching multiple of `up`."""
    taps = kern.shape[1]
    whole = resample_emul(x, kern, up, down, width)
    res = {}
    ns = list(ns)
    for b in range(0, len(ns), batch):
        group, pos, parts, at = ns[b:b + batch], 0, [], []
        for n in group:
            at.append(pos)
            span = -(-(n + taps + down) // down) * down
            parts.append(torch.cat([x[:n], torch.zeros(span - n)]))
            pos += span
        out = resample_emul(torch.cat(parts), kern, up, down, width)
        for n, a in zip(group, at):
            n_out = resample_n_out(n, up, down)
            o0 = a // down * up
            diff = (out[o0:o0 + n_out] != whole[:n_out]).nonzero()
            res[n] = int(diff[0]) if diff.numel() else n_out
    return res
