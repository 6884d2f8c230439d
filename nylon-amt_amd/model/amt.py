"""Drop-in replacement of the reference's ``model/amt.py`` (class ``AMT``) on the MI355X HIP path.

Same surface as hftt_code/model/amt.py: ``AMT(config, model_path, batch_size=1, verbose_flag=False)``,
``wav2feature`` (:34), ``transcript`` (:66), ``transcript_stride`` (:121), ``mpe2note`` (:179), ``note2midi`` (:347).
Two additions: ``transcript_notes`` = ``mpe2note(*transcript(...))`` with the rolls and the decoding kept on the device (csrc/notes.hip).
and ``transcript_notes_files``, the same for a list of files in one pass (the file loop of evaluation/m_inference.py:77-165).
``open_stream`` returns a ``NoteStream``: the same notes for audio that arrives in pieces, each as soon as it is final (csrc/notes_stream.hip).
Differences in mechanism, not in results:
  * wav2feature runs the log-mel kernel of libhftt_hip.so (STFT + sparse mel + log on the GPU) instead of torchaudio;
  * transcript/transcript_stride gather ALL clip windows of a file and run them through the model in batches of
    ``batch_size`` clips (the reference stores batch_size and then runs clips one by one, amt.py:31,88);
  * note2midi writes a standard MIDI file directly (pretty_midi is not a dependency).
The model runs on the GPU only; there is no CPU fallback.
"""
import os
import pickle
import struct
import sys

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from hftt_hip._capi import HfttError   # noqa: E402


class AMT():
    def __init__(self, config, model_path, batch_size=1, verbose_flag=False, rank=None, world=None, device=None, gather='host'):
        """rank / world (default: those of torch.distributed when it is initialised, else 0 / 1): the clip batches of a file are dealt
        to the ranks round-robin and each rank runs its share on ITS GPU -- replicas only, NO collective on the data path (the reference
        runs one clip at a time on one device, amt.py:88).  gather='host' (default): every rank copies its own results to the host and
        rank 0 collects them by clip index through a host (gloo) channel, so RANK 0 returns the whole transcription (amt.py:104-113
        stitching order) and writes the files; the other ranks return arrays in which only their own clips are filled.  gather='all': the
        round-1..5 behaviour, an all_gather that leaves the whole result on every rank (only sensible for a few clips).  gather='none':
        no exchange at all (every rank keeps its shard; for callers that shard by FILE with hftt_hip.ddp.shard_indices)."""
        if gather not in ('host', 'all', 'none'):
            raise HfttError("gather must be 'host', 'all' or 'none'")
        self.gather = gather
        self._host_group = None
        if verbose_flag is True:
            print('torch version: ' + torch.__version__)
            print('torch cuda   : ' + str(torch.cuda.is_available()))
        if rank is None or world is None:
            from hftt_hip.ddp import rank_world
            rank, world = rank_world()
        self.rank, self.world = int(rank), int(world)
        if device is not None:
            self.device = device
        elif torch.cuda.is_available():
            self.device = 'cuda:%d' % int(os.environ.get('LOCAL_RANK', 0)) if self.world > 1 and 'LOCAL_RANK' in os.environ else 'cuda'
        else:
            self.device = 'cpu'      # the model itself will refuse to run there (no CPU fallback)

        self.config = config

        if model_path == None:   # noqa: E711  (kept as in the reference)
            self.model = None
        else:
            with open(model_path, 'rb') as f:
                self.model = pickle.load(f)
            self.model = self.model.to(self.device)
            self.model.eval()
            if hasattr(self.model, 'hftt_freeze_weights'):
                self.model.hftt_freeze_weights(True)           # a transcriber never changes its weights: operands are prepared once
            if verbose_flag is True:
                print(self.model)

        self.batch_size = max(1, int(batch_size))
        self._logmel = None

    # ------------------------------------------------------------------ front end (amt.py:34-63)
    def wav2feature(self, f_wav):
        wave, sr = _load_wav(f_wav)                       # [channels, n] float32 in [-1, 1)
        return self.wave2feature(torch.from_numpy(wave), sr)

    def wave2feature(self, wave, sr, on_device=False):
        """wave [channels, n] or [n] float tensor at sample rate sr -> log-mel [n_frames, n_mels] (CPU tensor like the reference;
        on_device=True: the device tensor as the kernel left it, for transcript_notes)."""
        from hftt_hip import ops
        fe = self.config['feature']
        if not str(self.device).startswith('cuda'):
            raise HfttError('wav2feature runs the HIP log-mel kernel: a ROCm device is required')
        wave = wave.float()
        wave_mono = wave.mean(dim=0) if wave.dim() == 2 else wave        # torch.mean(wave, dim=0), amt.py:56
        if sr != fe['sr']:
            wave_mono = ops.resample(wave_mono.to(self.device), sr, fe['sr'])      # Resample(sr, 16000), amt.py:57-58: hftt_resample (HIP)
        if self._logmel is None:
            if fe['fft_bins'] != fe['window_length']:
                raise HfttError('window_length must equal fft_bins')
            self._logmel = ops.LogMel(self.device, sr=fe['sr'], n_fft=fe['fft_bins'], hop=fe['hop_sample'], n_mels=fe['mel_bins'],
                                      log_offset=fe['log_offset'])
        feat = self._logmel(wave_mono.to(self.device))
        return feat if on_device else feat.cpu()

    # ------------------------------------------------------------------ clip windowing + batched inference
    def _run_windows(self, a_input, starts, mode, ablation_flag):
        """a_input [n_in, n_bins] float32 (numpy); one model call per batch of clip windows starting at `starts`."""
        if ablation_flag is True or mode != 'combination':
            raise HfttError("only mode='combination' without ablation is built (the 1-F-D-T model of model_spec2midi.py)")
        cin = self.config['input']
        width = cin['margin_b'] + cin['num_frame'] + cin['margin_f']
        x = torch.from_numpy(a_input).to(self.device)                          # the whole file's features: one host->device copy
        self.model.eval()
        batches = [starts[b0:b0 + self.batch_size] for b0 in range(0, len(starts), self.batch_size)]
        mine = list(range(self.rank, len(batches), self.world))                 # this rank's batches (round-robin)
        parts = [[] for _ in range(8)]
        for bi in mine:
            spec = torch.stack([x[i:i + width].T for i in batches[bi]], dim=0)  # [b, n_bins, width] (amt.py:89)
            with torch.no_grad():
                o = self.model(spec)
            sel = (o[0], o[1], o[2], o[3].argmax(3), o[5], o[6], o[7], o[8].argmax(3))   # velocity argmax (amt.py:107,113)
            for lst, t in zip(parts, sel):
                lst.append(t)                                                   # stays on the device: one copy back per file, not per batch
        return self._collect(parts, batches, mine)

    def _collect(self, parts, batches, mine):
        """per-rank device results -> 8 numpy arrays [n_clips, num_frame, num_note] in clip order (complete on rank 0; see __init__: gather)"""
        cin, cm = self.config['input'], self.config['midi']
        T, N = cin['num_frame'], cm['num_note']
        n_clips = sum(len(b) for b in batches)
        if self.world == 1:
            return [torch.cat(l, dim=0).to('cpu').numpy() for l in parts]
        import torch.distributed as dist
        if self.gather != 'all':
            # replicas only: each rank's results go to ITS host; rank 0 collects the shards by clip index over a host channel (gloo),
            # never over RCCL -- no device collective anywhere on the inference path
            my_clips = [i for bi in mine for i in range(bi * self.batch_size, bi * self.batch_size + len(batches[bi]))]
            local = [torch.cat(l, dim=0).to('cpu').numpy() if l else np.zeros((0, T, N), np.int64 if k % 4 == 3 else np.float32) for k, l in enumerate(parts)]
            shards = [(my_clips, local)]
            if self.gather == 'host':
                if dist.get_backend() == 'gloo':
                    grp = None
                else:
                    if self._host_group is None:
                        self._host_group = dist.new_group(backend='gloo')      # (collective over all ranks: every rank of the job runs the same AMT calls)
                    grp = self._host_group
                got = [None] * self.world if self.rank == 0 else None
                dist.gather_object((my_clips, local), got, dst=0, group=grp)
                if self.rank == 0:
                    shards = got
            res = []
            for k in range(8):
                full = np.zeros((n_clips, T, N), np.int64 if k % 4 == 3 else np.float32)
                for clips, arrs in shards:
                    if len(clips):
                        full[np.asarray(clips)] = arrs[k]
                res.append(full)
            return res
        gdev = 'cpu' if dist.get_backend() == 'gloo' else self.device          # gloo moves host memory; RCCL ('nccl') device memory
        per = -(-len(batches) // self.world) * self.batch_size                # clips per rank, padded: equal-sized all_gather
        res = []
        order = [i for r in range(self.world) for bi in range(r, len(batches), self.world) for i in range(bi * self.batch_size, bi * self.batch_size + len(batches[bi]))]
        counts = [sum(len(batches[bi]) for bi in range(r, len(batches), self.world)) for r in range(self.world)]
        for k, l in enumerate(parts):
            dt = torch.int64 if k % 4 == 3 else torch.float32
            local = torch.zeros(per, T, N, dtype=dt, device=gdev)
            if l:
                cat = torch.cat(l, dim=0)
                local[:cat.shape[0]] = cat
            gathered = [torch.empty_like(local) for _ in range(self.world)]
            dist.all_gather(gathered, local)
            flat = torch.cat([g[:c] for g, c in zip(gathered, counts)], dim=0)
            full = torch.empty(n_clips, T, N, dtype=dt, device=gdev)
            full[torch.tensor(order, device=gdev)] = flat
            res.append(full.to('cpu').numpy())
        return res

    def transcript(self, a_feature, mode='combination', ablation_flag=False):
        # a_feature: [num_frame, n_mels]
        a_feature = np.array(a_feature, dtype=np.float32)
        cin, cf, cm = self.config['input'], self.config['feature'], self.config['midi']
        T = cin['num_frame']
        n = a_feature.shape[0]
        a_tmp_b = np.full([cin['margin_b'], cf['n_bins']], cin['min_value'], dtype=np.float32)
        len_s = int(np.ceil(n / T) * T) - n
        a_tmp_f = np.full([len_s + cin['margin_f'], cf['n_bins']], cin['min_value'], dtype=np.float32)
        a_input = np.concatenate([a_tmp_b, a_feature, a_tmp_f], axis=0)
        starts = list(range(0, n, T))
        res = self._run_windows(a_input, starts, mode, ablation_flag)
        outs = []
        for k, r in enumerate(res):
            dt = np.int8 if k % 4 == 3 else np.float32
            full = np.zeros((n + len_s, cm['num_note']), dtype=dt)
            for c, i in enumerate(starts):
                full[i:i + T] = r[c]
            outs.append(full)
        return tuple(outs)

    def transcript_stride(self, a_feature, n_offset, mode='combination', ablation_flag=False):
        # a_feature: [num_frame, n_mels]
        a_feature = np.array(a_feature, dtype=np.float32)
        cin, cf, cm = self.config['input'], self.config['feature'], self.config['midi']
        half_frame = int(cin['num_frame'] / 2)
        n = a_feature.shape[0]
        a_tmp_b = np.full([cin['margin_b'] + n_offset, cf['n_bins']], cin['min_value'], dtype=np.float32)
        tmp_len = n + cin['margin_b'] + cin['margin_f'] + half_frame
        len_s = int(np.ceil(tmp_len / half_frame) * half_frame) - tmp_len
        a_tmp_f = np.full([len_s + cin['margin_f'] + (half_frame - n_offset), cf['n_bins']], cin['min_value'], dtype=np.float32)
        a_input = np.concatenate([a_tmp_b, a_feature, a_tmp_f], axis=0)
        starts = list(range(0, n, half_frame))
        res = self._run_windows(a_input, starts, mode, ablation_flag)
        outs = []
        for k, r in enumerate(res):
            dt = np.int8 if k % 4 == 3 else np.float32
            full = np.zeros((n + len_s, cm['num_note']), dtype=dt)
            for c, i in enumerate(starts):
                full[i:i + half_frame] = r[c][n_offset:n_offset + half_frame]
            outs.append(full)
        return tuple(outs)

    # ------------------------------------------------------------------ features -> notes without leaving the device
    def transcript_notes(self, a_feature, n_offset=None, output='B', thred_onset=0.5, thred_offset=0.5, thred_mpe=0.5,
                         mode_velocity='ignore_zero', mode_offset='shorter'):
        """The note list of ``mpe2note(*transcript(a_feature)[4:8], ...)`` (output='A': ``[0:4]``; with n_offset: of ``transcript_stride(a_feature,
        n_offset)``), bit for bit, with everything between the features and the compact note list on the device: padding with min_value and
        window slicing (torch as plumbing), one model call per batch, hftt_stitch per batch straight into the file-long rolls (velocity argmax
        included), hftt_notes_decode once, ONE small device->host copy, and the final stable (onset, pitch) sort (amt.py:343) on the host.
        a_feature [n_frames, n_bins]: a numpy array or a device tensor (``wave2feature(..., on_device=True)``).
        One process, one GPU: with world > 1 this raises HfttError -- sharded inference keeps transcript / transcript_stride + mpe2note.
        There is no CPU fallback."""
        from hftt_hip import ops
        if self.world > 1:
            raise HfttError('transcript_notes runs on one GPU (world = %d): sharded inference uses transcript / transcript_stride + mpe2note' % self.world)
        if output not in ('A', 'B'):
            raise HfttError("output must be 'A' (heads 0-3) or 'B' (heads 5-8)")
        if not str(self.device).startswith('cuda'):
            raise HfttError('transcript_notes decodes on the device: a ROCm device is required (there is no CPU fallback)')
        cin, cf, cm = self.config['input'], self.config['feature'], self.config['midi']
        T, N = cin['num_frame'], cm['num_note']
        if torch.is_tensor(a_feature):
            ops._need_cuda(a_feature)
            x = a_feature.to(device=self.device, dtype=torch.float32)
        else:
            x = torch.from_numpy(np.array(a_feature, dtype=np.float32)).to(self.device)
        n = x.shape[0]
        if n_offset is None:                                                    # transcript (amt.py:66-118)
            step, src0, front = T, 0, cin['margin_b']
            len_s = int(np.ceil(n / T) * T) - n
            back = len_s + cin['margin_f']
        else:                                                                   # transcript_stride (amt.py:121-176)
            step, src0, front = int(T / 2), int(n_offset), cin['margin_b'] + int(n_offset)
            tmp_len = n + cin['margin_b'] + cin['margin_f'] + step
            len_s = int(np.ceil(tmp_len / step) * step) - tmp_len
            back = len_s + cin['margin_f'] + (step - int(n_offset))
        F = n + len_s
        a_input = torch.full((front + n + back, cf['n_bins']), cin['min_value'], dtype=torch.float32, device=self.device)
        a_input[front:front + n] = x
        width = cin['margin_b'] + T + cin['margin_f']
        starts = list(range(0, n, step))
        rolls = tuple(torch.zeros(F, N, dtype=torch.int8 if k == 3 else torch.float32, device=self.device) for k in range(4))
        h0 = 0 if output == 'A' else 5
        self.model.eval()
        for b0 in range(0, len(starts), self.batch_size):
            batch = starts[b0:b0 + self.batch_size]
            spec = torch.stack([a_input[i:i + width].T for i in batch], dim=0)   # [b, n_bins, width] (amt.py:89)
            with torch.no_grad():
                o = self.model(spec)
            ops.stitch(o[h0], o[h0 + 1], o[h0 + 2], o[h0 + 3], rolls, batch, src0=src0, length=step)
        hop_sec = float(cf['hop_sample'] / cf['sr'])
        pitch, velocity, onset, offset = ops.notes_decode(*rolls, hop_sec, note_min=cm['note_min'], thred_onset=thred_onset, thred_offset=thred_offset,
                                                          thred_mpe=thred_mpe, mode_velocity=mode_velocity, mode_offset=mode_offset, host=True)
        pitch, velocity, onset, offset = pitch.numpy(), velocity.numpy(), onset.numpy(), offset.numpy()
        order = np.lexsort((pitch, onset))                                      # stable: by onset, then pitch, then the order of a_note (amt.py:343)
        return [{'pitch': int(pitch[i]), 'onset': float(onset[i]), 'offset': float(offset[i]), 'velocity': int(velocity[i])} for i in order]

    def transcript_notes_files(self, a_features, n_offset=None, output='B', thred_onset=0.5, thred_offset=0.5, thred_mpe=0.5,
                               mode_velocity='ignore_zero', mode_offset='shorter'):
        """``transcript_notes`` for a list of files in one pass (the file loop of evaluation/m_inference.py:77-165): one sorted note list per
        file; with output='AB' one ``(notes_A, notes_B)`` pair per file from a SINGLE model pass (both head sets, what m_inference.py writes).
        a_features: a sequence of [n_i, n_bins] arrays, numpy arrays and device tensors (``wave2feature(..., on_device=True)``) mixed freely.
        The features are concatenated on the device once and the clip table (file, start) of all files is built on the host with the
        arithmetic of transcript / transcript_stride and uploaded once.  Every ``batch_size`` clips -- ACROSS file borders, so only the last
        batch of the list is short -- are cut by hftt_clip_windows (padding with min_value per window: a window never shows a neighbouring
        file's frames), run through one model call and stitched into rolls that hold all files back to back.  One hftt_notes_decode_seg
        decodes every file on its own rows alone, one device->host copy fetches all lists, and the stable (onset, pitch) sort (amt.py:343) per
        file runs on the host.
        The result is that of ``[transcript_notes(f, ...) for f in a_features]``, bit for bit: the decode is exact per file, and the eval
        forward gives a clip the same outputs whatever else its batch holds (tests/test_notes_files_gpu.py holds both, and the packed call to
        the host path at equal batches).
        Memory: the whole list's features and rolls are resident at once, 1,024 + 13 * num_note bytes per frame at 256 bins (twice the 13 *
        num_note with 'AB'); a caller with more than the device holds splits the list.
        One process, one GPU (world > 1 raises HfttError); there is no CPU fallback.  An empty list gives []; a file of zero frames []."""
        from hftt_hip import ops
        if self.world > 1:
            raise HfttError('transcript_notes_files runs on one GPU (world = %d): sharded inference uses transcript / transcript_stride + mpe2note' % self.world)
        if output not in ('A', 'B', 'AB'):
            raise HfttError("output must be 'A' (heads 0-3), 'B' (heads 5-8) or 'AB' (both, one model pass)")
        if not str(self.device).startswith('cuda'):
            raise HfttError('transcript_notes_files decodes on the device: a ROCm device is required (there is no CPU fallback)')
        cin, cf, cm = self.config['input'], self.config['feature'], self.config['midi']
        T, N = cin['num_frame'], cm['num_note']
        n_files = len(a_features)
        if n_files == 0:
            return []
        # the features on the device, file after file: the host arrays travel as ONE block
        host_idx = [i for i, a in enumerate(a_features) if not torch.is_tensor(a)]
        host = [np.array(a_features[i], dtype=np.float32).reshape(-1, cf['n_bins']) for i in host_idx]
        pieces = [None] * n_files
        if host:
            block = torch.from_numpy(np.concatenate(host, axis=0)).to(self.device)
            r = 0
            for i, a in zip(host_idx, host):
                pieces[i] = block[r:r + a.shape[0]]
                r += a.shape[0]
        for i, a in enumerate(a_features):
            if torch.is_tensor(a):
                ops._need_cuda(a)
                pieces[i] = a.to(device=self.device, dtype=torch.float32).reshape(-1, cf['n_bins'])
        feature = block if len(host) == n_files else torch.cat(pieces, dim=0)
        lens = [int(p.shape[0]) for p in pieces]
        # the clip table of all files, file-major with ascending start (transcript amt.py:66-118, transcript_stride :121-176)
        if n_offset is None:
            step, src0, front = T, 0, cin['margin_b']
        else:
            step, src0, front = int(T / 2), int(n_offset), cin['margin_b'] + int(n_offset)
        file_row0, roll_row0, win_file, win_start, dst = [0], [0], [], [], []
        for f, n in enumerate(lens):
            if n_offset is None:
                len_s = int(np.ceil(n / T) * T) - n
            else:
                tmp_len = n + cin['margin_b'] + cin['margin_f'] + step
                len_s = int(np.ceil(tmp_len / step) * step) - tmp_len
            for i in range(0, n, step):
                win_file.append(f)
                win_start.append(i - front)                                     # a_input row i is the file's frame i - front
                dst.append(roll_row0[f] + i)
            file_row0.append(file_row0[f] + n)
            roll_row0.append(roll_row0[f] + (n + len_s if n else 0))
        F = roll_row0[n_files]
        sets = (0, 5) if output == 'AB' else ((0,) if output == 'A' else (5,))
        width = cin['margin_b'] + T + cin['margin_f']
        rolls = tuple(torch.zeros(len(sets) * F, N, dtype=torch.int8 if k == 3 else torch.float32, device=self.device) for k in range(4))
        if win_file:
            n_win = len(win_file)
            table = torch.tensor(file_row0 + win_file + win_start, dtype=torch.int32).to(self.device)   # file rows + the clip table: one upload
            rows, wf, ws = table[:n_files + 1], table[n_files + 1:n_files + 1 + n_win], table[n_files + 1 + n_win:]
            self.model.eval()
            for b0 in range(0, len(dst), self.batch_size):
                b1 = min(b0 + self.batch_size, len(dst))
                spec = ops.clip_windows(feature, rows, wf[b0:b1], ws[b0:b1], width, cin['min_value'])
                with torch.no_grad():
                    o = self.model(spec)
                for q, h0 in enumerate(sets):
                    ops.stitch(o[h0], o[h0 + 1], o[h0 + 2], o[h0 + 3], rolls, [q * F + x for x in dst[b0:b1]], src0=src0, length=step)
        seg_rows = [q * F + x for q in range(len(sets)) for x in roll_row0[:n_files]] + [len(sets) * F]
        hop_sec = float(cf['hop_sample'] / cf['sr'])
        pitch, velocity, onset, offset, seg_notes = (x.numpy() for x in ops.notes_decode_seg(
            *rolls, seg_rows, hop_sec, note_min=cm['note_min'], thred_onset=thred_onset, thred_offset=thred_offset, thred_mpe=thred_mpe,
            mode_velocity=mode_velocity, mode_offset=mode_offset, host=True))

        def notes_of(s):
            a, b = int(seg_notes[s]), int(seg_notes[s + 1])
            p, v, t0, t1 = pitch[a:b], velocity[a:b], onset[a:b], offset[a:b]
            order = np.lexsort((p, t0))                                         # stable: by onset, then pitch, then the order of a_note (amt.py:343)
            return [{'pitch': int(p[i]), 'onset': float(t0[i]), 'offset': float(t1[i]), 'velocity': int(v[i])} for i in order]
        if output == 'AB':
            return [(notes_of(f), notes_of(n_files + f)) for f in range(n_files)]
        return [notes_of(f) for f in range(n_files)]

    # ------------------------------------------------------------------ audio as it arrives -> notes as they become final
    def open_stream(self, n_streams=1, n_offset=None, output='B', thred_onset=0.5, thred_offset=0.5, thred_mpe=0.5,
                    mode_velocity='ignore_zero', history=None, mode_offset='shorter', sr=None):
        """A NoteStream: ``transcript_notes`` for audio that arrives in pieces, n_streams recordings side by side on this GPU.  See NoteStream
        for the contract.  sr: the rate of the samples that ``push_wave`` will bring, of every stream of the object (None: the feature rate);
        they are resampled on the device with their state carried forward (hftt_resample_stream).  A rate whose filter window does not fit
        the resampler's LDS is refused here.  One process, one GPU (world > 1 raises HfttError); mode_offset 'shorter' only; there is no CPU
        fallback."""
        return NoteStream(self, n_streams, n_offset, output, thred_onset, thred_offset, thred_mpe, mode_velocity, history, mode_offset, sr)

    # ------------------------------------------------------------------ posteriorgram -> notes (amt.py:179-344)
    def mpe2note(self, a_onset=None, a_offset=None, a_mpe=None, a_velocity=None, thred_onset=0.5, thred_offset=0.5, thred_mpe=0.5,
                 mode_velocity='ignore_zero', mode_offset='shorter'):
        hop_sec = float(self.config['feature']['hop_sample'] / self.config['feature']['sr'])
        a_onset = np.asarray(a_onset); a_offset = np.asarray(a_offset); a_mpe = np.asarray(a_mpe); a_velocity = np.asarray(a_velocity)
        a_note = []
        n_mpe = len(a_mpe)
        for j in range(self.config['midi']['num_note']):
            on_loc, on_time = _pick_peaks(a_onset[:, j], thred_onset, hop_sec)          # :193-223
            off_loc, off_time = _pick_peaks(a_offset[:, j], thred_offset, hop_sec)      # :224-253
            below = np.nonzero(a_mpe[:, j] < thred_mpe)[0]
            time_offset = 0.0
            for idx_on in range(len(on_loc)):
                loc_onset, time_onset = int(on_loc[idx_on]), float(on_time[idx_on])
                if idx_on + 1 < len(on_loc):                                            # :263-269
                    loc_next, time_next = int(on_loc[idx_on + 1]), float(on_time[idx_on + 1])
                else:
                    loc_next, time_next = n_mpe, (n_mpe - 1) * hop_sec
                loc_offset, flag_offset = loc_onset + 1, False                         # :272-281
                k = np.searchsorted(off_loc, loc_onset, side='right')
                if k < len(off_loc):
                    loc_offset, time_offset, flag_offset = int(off_loc[k]), float(off_time[k]), True
                if loc_offset > loc_next:                                               # :282-284
                    loc_offset, time_offset = loc_next, time_next
                loc_mpe, flag_mpe, time_mpe = loc_onset + 1, False, 0.0                 # :288-296 ("1 frame longer")
                kb = np.searchsorted(below, loc_onset + 1, side='left')
                if kb < len(below) and below[kb] < loc_next:
                    loc_mpe, flag_mpe = int(below[kb]), True
                    time_mpe = loc_mpe * hop_sec
                pitch_value = int(j + self.config['midi']['note_min'])
                velocity_value = int(a_velocity[loc_onset][j])
                if (not flag_offset) and (not flag_mpe):                                # :311-331
                    offset_value = float(time_next)
                elif flag_offset and (not flag_mpe):
                    offset_value = float(time_offset)
                elif (not flag_offset) and flag_mpe:
                    offset_value = float(time_mpe)
                elif mode_offset == 'offset':
                    offset_value = float(time_offset)
                elif mode_offset == 'longer':
                    offset_value = float(time_offset) if loc_offset >= loc_mpe else float(time_mpe)
                else:
                    offset_value = float(time_offset) if loc_offset <= loc_mpe else float(time_mpe)
                if mode_velocity != 'ignore_zero' or velocity_value > 0:                # :332-336
                    a_note.append({'pitch': pitch_value, 'onset': float(time_onset), 'offset': offset_value, 'velocity': velocity_value})
                if len(a_note) > 1 and a_note[-1]['pitch'] == a_note[-2]['pitch'] and a_note[-1]['onset'] < a_note[-2]['offset']:
                    a_note[-2]['offset'] = a_note[-1]['onset']                         # :338-341
        return sorted(sorted(a_note, key=lambda x: x['pitch']), key=lambda x: x['onset'])   # :343

    def note2midi(self, a_note, f_midi):
        """Single-track standard MIDI file, 220 ticks per beat at 120 bpm (pretty_midi's defaults), program 0."""
        ticks_per_sec = 220 * 2.0
        events = []
        for note in a_note:
            on, off = int(round(note['onset'] * ticks_per_sec)), int(round(note['offset'] * ticks_per_sec))
            events.append((on, 1, bytes([0x90, int(note['pitch']) & 0x7F, int(note['velocity']) & 0x7F])))
            events.append((max(off, on), 0, bytes([0x90, int(note['pitch']) & 0x7F, 0])))
        events.sort(key=lambda e: (e[0], e[1]))
        trk = bytearray()
        trk += b'\x00\xff\x51\x03' + (500000).to_bytes(3, 'big')          # tempo 120 bpm
        trk += b'\x00\xff\x58\x04\x04\x02\x18\x08'                         # 4/4
        trk += b'\x00\xc0\x00'                                             # program 0
        t = 0
        for tick, _, msg in events:
            trk += _vlq(tick - t) + msg
            t = tick
        trk += b'\x01\xff\x2f\x00'
        with open(f_midi, 'wb') as f:
            f.write(b'MThd' + struct.pack('>IHHH', 6, 0, 1, 220))
            f.write(b'MTrk' + struct.pack('>I', len(trk)) + bytes(trk))
        return


class NoteStream():
    """``AMT.open_stream``: push log-mel frames (``push``) or samples (``push_wave``) of n_streams recordings as they arrive and get back, per
    stream, the notes that no later audio can change; ``close`` ends streams and returns the rest.  The contract:

        sorted(all notes returned by push... + close, key=(onset, pitch)) == amt.transcript_notes(whole_feature, same arguments)

    bit for bit, for any chunking (with push_wave: whole_feature = ``wave2feature(wave, sr, on_device=True)``, sr the rate declared at
    ``open_stream(sr=)``: 44.1 or 48 kHz audio goes in as it comes from the sound card).  The wave side: ONE hftt_resample_stream launch per
    push_wave takes the new samples of all streams, behind each stream's carried tail of fewer than taps + down input samples, to the feature
    rate and into a per-stream slot of a resampled store (ops.ResampleStream); ONE hftt_clip_logmel launch over that store computes the frames
    that became complete, all streams at once; one batched copy slides the slots.  An output sample exists (width + down) / sr seconds
    after its instant -- 10.4 ms at 44.1 kHz, 0.5 ms at 48 kHz --, a frame n_fft / 2 samples later.  Then the frames join a
    per-stream tail; every clip whose look-ahead has arrived is cut from the tail (hftt_clip_windows, the tail as the "file", so the min_value
    padding shows only where transcript pads), the ready clips of ALL streams are packed into model calls of up to batch_size clips and
    stitched (hftt_stitch) into per-stream rings of `history` rows, and one hftt_notes_stream_step per round returns what became final with
    one device->host copy.  The decoder's state has a fixed size; nothing grows with the length of the recording.
    Latency: a roll row exists once the clip that holds it has run, i.e. once num_frame + margin_f frames behind the clip's start have
    arrived -- with n_offset = num_frame / 2, num_frame + margin_f - n_offset frames (96 frames, 1.5 s, at the default config); a note is
    final a few frames behind its offset peak, its mpe end or the next onset (include/hftt_hip.h: streaming notes).
    history: ring rows per stream, a multiple of the stitch length, default 4 * num_frame; a round delivers at most half of it, the other
    half holds what is undecided (an onset or offset plateau at or above its threshold that has not ended).  A stretch that outgrows it
    raises HfttError naming the stream and history=.
    Refused with HfttError: world > 1, a device that is not ROCm, mode_offset other than 'shorter' (under 'longer' / 'offset' a note may
    wait for an offset peak anywhere later in the file), a chunk for a closed stream, samples at another rate than the declared one, a
    declared rate whose filter window exceeds the resampler's LDS.  No CPU fallback."""

    def __init__(self, amt, n_streams, n_offset, output, thred_onset, thred_offset, thred_mpe, mode_velocity, history, mode_offset, sr=None):
        from hftt_hip import ops
        if amt.world > 1:
            raise HfttError('open_stream runs on one GPU (world = %d): sharded inference uses transcript / transcript_stride + mpe2note' % amt.world)
        if output not in ('A', 'B'):
            raise HfttError("output must be 'A' (heads 0-3) or 'B' (heads 5-8)")
        if mode_offset != 'shorter':
            raise HfttError("open_stream decodes mode_offset 'shorter' only (got %r): under 'longer' / 'offset' a note may wait for an offset peak "
                            "anywhere later in the file" % (mode_offset,))
        if mode_velocity not in ops.MODE_VELOCITY:
            raise HfttError('open_stream: mode_velocity %r unknown' % (mode_velocity,))
        if not str(amt.device).startswith('cuda'):
            raise HfttError('open_stream decodes on the device: a ROCm device is required (there is no CPU fallback)')
        self.amt, self.S = amt, int(n_streams)
        if self.S < 1:
            raise HfttError('open_stream: n_streams=%d must be positive' % self.S)
        fe = amt.config['feature']
        self.sr = int(fe['sr']) if sr is None else int(sr)
        if self.sr < 1:
            raise HfttError('open_stream: sr=%d must be a positive sample rate' % self.sr)
        if self.sr != int(fe['sr']):
            up, down, width = ops.resample_geometry(self.sr, fe['sr'])
            if ops.resample_stream_lds(up, down, width) > 64 * 1024:
                raise HfttError('open_stream: input rate %d -> feature rate %d: the filter window of one workgroup (down = %d, taps = %d) exceeds '
                                '64 KB of LDS' % (self.sr, fe['sr'], down, 2 * width + down))
        cin, cm = amt.config['input'], amt.config['midi']
        T = cin['num_frame']
        if n_offset is None:                                                    # transcript (amt.py:66-118)
            self.step, self.src0, self.front = T, 0, cin['margin_b']
        else:                                                                   # transcript_stride (amt.py:121-176)
            self.step, self.src0, self.front = int(T / 2), int(n_offset), cin['margin_b'] + int(n_offset)
            if not 0 <= self.src0 <= T - self.step:
                raise HfttError('open_stream: n_offset=%d outside 0..%d' % (self.src0, T - self.step))
        self.n_offset, self.h0 = n_offset, 0 if output == 'A' else 5
        self.width = cin['margin_b'] + T + cin['margin_f']
        H = 4 * T if history is None else int(history)
        if H < 2 * self.step or H % self.step:
            raise HfttError('open_stream: history=%d must be a multiple of the stitch length %d, at least twice it' % (H, self.step))
        self.per_round = max(1, H // 2 // self.step)                            # clips per stream and round: half the ring
        self.kw = dict(note_min=cm['note_min'], thred_onset=thred_onset, thred_offset=thred_offset, thred_mpe=thred_mpe, mode_velocity=mode_velocity)
        self.st = ops.notes_stream_state(self.S, cm['num_note'], H, amt.device)
        n_bins = amt.config['feature']['n_bins']
        self.tail = [torch.zeros(0, n_bins, dtype=torch.float32, device=amt.device) for _ in range(self.S)]
        self.tail0 = [0] * self.S                                               # the file frame of tail row 0
        self.n = [0] * self.S                                                   # frames received
        self.next = [0] * self.S                                                # start of the next clip
        self.closed = [False] * self.S
        self.rs = None                                                          # push_wave: the ops.ResampleStream of all streams, made at the first call
        self.is_wave = [False] * self.S                                         # the stream has been given samples

    # ------------------------------------------------------------------ the public calls
    def push(self, chunks):
        """chunks[s]: [n, n_bins] log-mel frames of stream s (numpy array or device tensor; None or n = 0: nothing) -> per stream the notes
        that became final, as the dicts of transcript_notes, sorted by (onset, pitch).  With n_streams == 1 a bare array goes in and a bare
        list comes out."""
        chunks, bare = self._per_stream(chunks)
        for s, a in enumerate(chunks):
            self._append(s, a)
        out = self._run([False] * self.S)
        return out[0] if bare else out

    def push_wave(self, chunks, sr=None):
        """chunks[s]: samples of stream s at the rate declared at open_stream (the feature rate by default): 1-d, or [channels, n] and then
        downmixed per sample as wave2feature does, ``wave.float().mean(dim=0)``; floating point in [-1, 1) or int16 (value s / 32768); any
        length; None: nothing.  sr: omitted, or the declared rate.  One hftt_resample_stream launch and one hftt_clip_logmel launch for all
        streams; a frame is computed once the resampled samples through t * hop + n_fft / 2 - 1 exist; then as push."""
        fe = self.amt.config['feature']
        if sr is not None and int(sr) != self.sr:
            raise HfttError('push_wave takes samples at the %s rate %d (got %d): the input rate of a stream object is declared at open_stream(sr=)'
                            % ('feature' if self.sr == int(fe['sr']) else 'declared', self.sr, sr))
        chunks, bare = self._per_stream(chunks)
        self._wave_round([self._wave_chunk(s, w) for s, w in enumerate(chunks)], [False] * self.S)
        out = self._run([False] * self.S)
        return out[0] if bare else out

    def close(self, which=None):
        """End the streams `which` (default: all that are open): pad as transcript / transcript_stride do, run the remaining clips, deliver
        the file's last rows and return the rest of the notes, per stream (a bare list with n_streams == 1)."""
        which = [s for s in range(self.S) if not self.closed[s]] if which is None else [int(s) for s in ([which] if np.isscalar(which) else which)]
        closing = [False] * self.S
        for s in which:
            if self.closed[s]:
                raise HfttError('close: stream %d is closed already' % s)
            closing[s] = True
        if any(closing[s] and self.is_wave[s] for s in range(self.S)):
            self._wave_round([None] * self.S, [closing[s] and self.is_wave[s] for s in range(self.S)])
        out = self._run(closing)
        return out[0] if self.S == 1 else out

    # ------------------------------------------------------------------ the parts
    def _per_stream(self, chunks):
        bare = self.S == 1 and not isinstance(chunks, (list, tuple))
        chunks = [chunks] if bare else list(chunks)
        if len(chunks) != self.S:
            raise HfttError('NoteStream: %d chunks for %d streams' % (len(chunks), self.S))
        return chunks, bare

    def _append(self, s, a):
        from hftt_hip import ops
        if a is None:
            return
        n_bins = self.tail[s].shape[1]
        if torch.is_tensor(a):
            ops._need_cuda(a)
            x = a.to(device=self.amt.device, dtype=torch.float32).reshape(-1, n_bins)
        else:
            x = torch.from_numpy(np.array(a, dtype=np.float32).reshape(-1, n_bins)).to(self.amt.device)
        if x.shape[0] == 0:
            return
        if self.closed[s]:
            raise HfttError('NoteStream: stream %d is closed' % s)
        self.tail[s] = torch.cat([self.tail[s], x], dim=0)
        self.n[s] += x.shape[0]

    def _wave_chunk(self, s, w):
        """one stream's chunk as ops.resample_stream takes it: 1-d, int16 or floating point; [channels, n] downmixed as wave2feature does"""
        if w is None:
            return None
        w = torch.as_tensor(w)
        if w.dtype != torch.int16 and not w.dtype.is_floating_point:
            raise HfttError('push_wave: stream %d: samples are int16 or floating point, got %s' % (s, w.dtype))
        if w.dim() == 2:
            w = (w.float() * (1.0 / 32768.0) if w.dtype == torch.int16 else w.float()).mean(dim=0)      # torch.mean(wave, dim=0), amt.py:56
        elif w.dim() != 1:
            raise HfttError('push_wave: stream %d: samples are 1-d (mono) or [channels, n], got shape %s' % (s, tuple(w.shape)))
        if w.numel() and self.closed[s]:
            raise HfttError('NoteStream: stream %d is closed' % s)
        self.is_wave[s] = True
        return w

    def _wave_round(self, chunks, closing):
        """the samples of all streams -> the frames they complete (closing[s]: all 1 + n / hop of the file, zeros to the right of the
        samples), appended to the feature tails: one ops.resample_stream, one ops.stream_logmel"""
        from hftt_hip import ops
        amt, fe = self.amt, self.amt.config['feature']
        hop, n_fft = fe['hop_sample'], fe['fft_bins']
        if amt._logmel is None:
            if fe['fft_bins'] != fe['window_length']:
                raise HfttError('window_length must equal fft_bins')
            amt._logmel = ops.LogMel(amt.device, sr=fe['sr'], n_fft=n_fft, hop=hop, n_mels=fe['mel_bins'], log_offset=fe['log_offset'])
        if self.rs is None:
            self.rs = ops.ResampleStream(self.S, self.sr, fe['sr'], amt.device, n_fft=n_fft, hop=hop)
        ops.resample_stream(self.rs, chunks, closing)
        for s, frames in enumerate(ops.stream_logmel(self.rs, amt._logmel)):
            self._append(s, frames)

    def _roll_rows(self, s):
        """F of transcript / transcript_stride for the n frames of stream s"""
        cin = self.amt.config['input']
        n, T = self.n[s], cin['num_frame']
        if self.n_offset is None:
            return int(np.ceil(n / T) * T)
        tmp_len = n + cin['margin_b'] + cin['margin_f'] + self.step
        return n + int(np.ceil(tmp_len / self.step) * self.step) - tmp_len

    def _run(self, closing):
        """rounds of: the ready clips of all streams (at most half a ring per stream) -> model -> stitch -> one decoder step"""
        from hftt_hip import ops
        amt, st, S, step = self.amt, self.st, self.S, self.step
        cin, cf = amt.config['input'], amt.config['feature']
        hop_sec = float(cf['hop_sample'] / cf['sr'])
        H = st.H
        notes = [[] for _ in range(S)]
        while True:
            clips, new_rows, close_now = [], [0] * S, [False] * S
            for s in range(S):
                if self.closed[s]:
                    continue
                F = self._roll_rows(s) if closing[s] else None
                k = 0
                while k < self.per_round:
                    i = self.next[s]
                    ready = i < self.n[s] if closing[s] else i - self.front + self.width <= self.n[s]
                    if not ready:
                        break
                    length = step if F is None else max(0, min(step, F - i))
                    clips.append((s, i, length))
                    new_rows[s] += length
                    self.next[s] = i + step
                    k += 1
                if closing[s] and self.next[s] >= self.n[s]:                     # its last clips are in this round: the rows up to F follow
                    close_now[s] = True
            if not clips and not any(close_now):
                break
            if clips:
                rows = [0]
                for s in range(S):
                    rows.append(rows[-1] + self.tail[s].shape[0])
                feature = torch.cat(self.tail, dim=0) if S > 1 else self.tail[0]
                if feature.shape[0] == 0:
                    feature = torch.zeros(1, feature.shape[1], dtype=torch.float32, device=amt.device)
                table = torch.tensor(rows + [s for s, _, _ in clips] + [i - self.front - self.tail0[s] for s, i, _ in clips], dtype=torch.int32).to(amt.device)
                nc = len(clips)
                frow, wf, ws = table[:S + 1], table[S + 1:S + 1 + nc], table[S + 1 + nc:]
                amt.model.eval()
                for b0 in range(0, nc, amt.batch_size):
                    b1 = min(b0 + amt.batch_size, nc)
                    spec = ops.clip_windows(feature.contiguous(), frow, wf[b0:b1], ws[b0:b1], self.width, cin['min_value'])
                    with torch.no_grad():
                        o = amt.model(spec)
                    for length in sorted({c[2] for c in clips[b0:b1]}):
                        sel = [q for q in range(b0, b1) if clips[q][2] == length]
                        if length == 0:
                            continue
                        idx = torch.tensor([q - b0 for q in sel], device=amt.device)
                        heads = [o[self.h0 + k] if len(sel) == b1 - b0 else o[self.h0 + k].index_select(0, idx) for k in range(4)]
                        ops.stitch(*heads, st.rings_flat, [clips[q][0] * H + clips[q][1] % H for q in sel], src0=self.src0, length=length)
            for s in range(S):
                if close_now[s]:                                                # rows that no clip covers are zero rows, as in transcript_notes
                    F, have = self._roll_rows(s), st.row_end[s] + new_rows[s]
                    for r in range(have, F):
                        for ring in st.rings_flat:
                            ring[s * H + r % H].zero_()
                    new_rows[s] += max(0, F - have)
                    self.closed[s] = True
                keep = max(self.tail0[s], min(self.next[s] - self.front, self.n[s]))
                if keep > self.tail0[s]:
                    self.tail[s] = self.tail[s][keep - self.tail0[s]:]
                    self.tail0[s] = keep
            st.deliver(new_rows, close_now)
            pitch, vel, t_on, t_off, heads, overflow = (x.numpy() for x in ops.notes_stream_step(st, hop_sec, host=True, **self.kw))
            for s in range(S):
                if overflow[s]:
                    raise HfttError('NoteStream: stream %d: an undecided stretch (a plateau at or above a threshold) outgrew the ring of %d rows: '
                                    'open the stream with a larger history=' % (s, H))
                a, b = int(heads[s]), int(heads[s + 1])
                notes[s] += [(float(t_on[q]), int(pitch[q]), float(t_off[q]), int(vel[q])) for q in range(a, b)]
        out = []
        for s in range(S):
            p = np.array([x[1] for x in notes[s]], np.int64)
            t = np.array([x[0] for x in notes[s]], np.float64)
            order = np.lexsort((p, t))                                          # by onset, then pitch (amt.py:343)
            out.append([{'pitch': notes[s][q][1], 'onset': notes[s][q][0], 'offset': notes[s][q][2], 'velocity': notes[s][q][3]} for q in order])
        return out


# ---------------------------------------------------------------------- helpers
def _pick_peaks(a, thred, hop_sec):
    """Local maxima >= thred of one pitch track with the reference's plateau rule (amt.py:195-223): a frame counts when
    the nearest DIFFERENT value on each side is smaller (or there is none); time refined from the two neighbours."""
    a = np.asarray(a, dtype=np.float32)
    n = len(a)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0)
    change = np.nonzero(a[1:] != a[:-1])[0] + 1
    run_start = np.concatenate([[0], change])
    run_id = np.zeros(n, np.int64)
    run_id[change] = 1
    run_id = np.cumsum(run_id)
    run_val = a[run_start]
    prev_val = np.concatenate([[-np.inf], run_val[:-1]])[run_id]
    next_val = np.concatenate([run_val[1:], [-np.inf]])[run_id]
    loc = np.nonzero((a >= thred) & (a > prev_val) & (a > next_val))[0]
    times = loc * hop_sec
    # Sub-frame refinement.  The reference mixes Python floats with numpy float32 scalars (amt.py:217-219); under NumPy 2
    # promotion rules (the build container, where the goldens were made) that arithmetic is carried out in float32, under
    # NumPy 1.x in float64 -- a <= 1e-6 s difference.  float32 is restated here so note order ties resolve identically.
    h2 = np.float32(hop_sec * 0.5)
    for q, i in enumerate(loc):
        if i == 0 or i == n - 1:
            continue
        l, c, r = a[i - 1], a[i], a[i + 1]
        if l > r:
            times[q] = float(np.float32(i * hop_sec) - (h2 * (l - r) / (c - r)))
        elif l < r:
            times[q] = float(np.float32(i * hop_sec) + (h2 * (r - l) / (c - l)))
    return loc, times


def _vlq(v):
    out = [v & 0x7F]
    v >>= 7
    while v:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    return bytes(reversed(out))


def _load_wav(path):
    """PCM / float WAV -> float32 [channels, n] scaled like torchaudio.load (integers / 2^(bits-1))."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.ndim == 1:
        data = data[:, None]
    if data.dtype == np.int16:
        x = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        x = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        x = (data.astype(np.float32) - 128.0) / 128.0
    else:
        x = data.astype(np.float32)
    return np.ascontiguousarray(x.T), int(sr)
