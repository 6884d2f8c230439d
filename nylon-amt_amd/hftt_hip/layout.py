"""Weight layout of the engine: pure offset arithmetic, no device, no library, no torch.

From the model dimensions, the precision mode, the option switches and the parameters' offsets / shapes in the flat buffer, `WeightLayout`
computes where every prepared operand lives: the matrix planes (bf16, fp32 or the x3 hi / lo pair -- the same element offsets), the fp32
vector plane, the strip-pack stream, and the table entries that tell the prepare kernels what to copy where (csrc/prep.hip:
prep entries; csrc/strip_gemm.hip, csrc/x3_strip.hip: strip-pack entries).  The engine allocates the tensors and uploads the tables.
"""
from collections import OrderedDict, namedtuple
from types import SimpleNamespace

# precision -> the descriptors' `npass` code (include/hftt_hip.h): 'x3' = split fp16 on forward products (2) and split bf16 on products with a
# gradient operand (4): three bf16-rate MFMA passes per product, fp32 tensors in HBM, outputs within 1e-3 of the reference (measured 1e-4)
PRECISION_NPASS = {'parity': 3, 'bf16': 1, 'x3': 2}

# option switches of an engine (HfttEngine.__init__ reads them from the environment):
# store_bf16 HFTT_BF16_STORE, strip HFTT_STRIP, planes HFTT_X3_PLANES, merge_ckv HFTT_X3_MERGE_CKV
Options = namedtuple('Options', 'store_bf16 strip planes merge_ckv', defaults=(True, True, True, True))


def _align(x, a):
    return (x + a - 1) // a * a


class _Flat:
    """Bump allocator over one flat tensor (element offsets, 16-byte aligned)."""

    def __init__(self):
        self.off = 0
        self.items = OrderedDict()
        self.sizes = {}

    def add(self, name, numel, align=8):
        self.off = _align(self.off, align)
        self.items[name] = self.off
        self.sizes[name] = numel
        self.off += numel
        return self.items[name]


def flat_offsets(named_numel):
    """offsets of the parameters in the flat fp32 buffer (reference state_dict order) and the buffer's length"""
    lay = _Flat()
    offs = [lay.add(n, k) for n, k in named_numel]
    return offs, _align(lay.off, 8)


def model_dims(cfg):
    """The shape symbols of the engine from the constructor arguments of the reference classes: T frames, F bins, N notes, V velocities,
    d hidden, p ffn, heads / layers of the encoder (e) and the decoder (d); Kp: the padded window width; NH: the packed head rows."""
    c = cfg
    n_proc = 2 * c['n_margin'] + 1
    NH = c['n_velocity'] + 3                     # packed head rows: velocity[0:V], onset, offset, mpe
    return SimpleNamespace(T=c['n_frame'], F=c['n_bin'], N=c['n_note'], V=c['n_velocity'], d=c['hid_dim'], p=c['pf_dim'],
                           He=c['enc_head'], Hd=c['dec_head'], Le=c['enc_layer'], Ld=c['dec_layer'], n_proc=n_proc, Kp=_align(n_proc, 32),
                           W=c['n_frame'] + 2 * c['n_margin'], nw=n_proc - (c['cnn_kernel'] - 1), NH=NH, NHp=_align(NH + 1, 64))


def precision_modes(d, p, npass, opts, fp32_hidden=False):
    """What a precision means at this width: which tensors are stored as bf16 and which kernel family runs."""
    m = SimpleNamespace(npass=npass, x3=npass == 2)
    # bf16 mode: tensors consumed only as MFMA operands (projections, attention context, FFN hidden and their gradients)
    # are STORED as bf16 -- identical numerics (they were rounded at load time anyway), half the traffic
    m.sb = npass == 1 and opts.store_bf16
    # the reference's default width (training/m_training.py:56-61: d = 64, ff = 128) in the x3 mode: the same launch sequence on the
    # small-width strip family (csrc/x3s_strip.h: every weight matrix of a launch resident in LDS, compact packs)
    # ... and, since round 5, in the bf16 mode (csrc/bs_strip.hip: the same launch sequence on the bf16 stream -- BASELINE config 2; the packs
    # are the x3 family's compact ones with bf16 halves, of which the bf16 kernels read the hi fragments)
    m.strip_small = opts.strip and (m.x3 or m.sb) and d == 64 and p == 128
    # strip kernels (csrc/strip_gemm.hip): bf16 mode at the paper's width.  Then the WHOLE activation stream between kernels is
    # bf16 (residual stream, pre-LayerNorm sums, hidden), fp32 lives only inside a kernel (accumulators, LayerNorm statistics).
    m.strip = (opts.strip and d == 256 and ((m.sb and p % 64 == 0) or (m.x3 and p == 512))) or m.strip_small
    # bfs: the bf16 activation / gradient STREAM of the bf16 strip plans.  The x3 strip plans run the same launch sequence on fp32 tensors.
    m.bfs = m.strip and m.sb
    # x3 strip plans: the STORED copy of the FFN hidden and its gradient dh are bf16.  fc_2 takes the hidden from registers at full width;
    # the stored copy is read as the ReLU / dropout gate and as ONE factor of the weight-gradient products (8 mantissa bits of one factor
    # leave dW's direction untouched: tests/test_paper_bf16_gpu.py), and these two tensors were 2 x 537 MB per layer at S_e.
    m.hh = m.strip and m.x3 and not fp32_hidden
    return m


def qkv_planes(modes, opts, d, H, Lq, Lk):
    """x3 strip plans: do the q / k / v projections of this attention hand their results over as f16-pair planes (written once by the
    projection's epilogue, staged by LDS-DMA in the attention forward: csrc/x3_attn_pl.hip)?  dh == 64 and one query block per wave."""
    if not (modes.x3 and modes.strip and opts.planes and d // H == 64):
        return False
    nqb = (Lq + 31) // 32
    return nqb <= (8 if Lk > 128 else 4)


# per-block matrix planes that only the general GEMM reads: with the strip plans most of them are never asked for (the strip packs
# replace them), and preparing all of them every step cost 80 us.  A plane is prepared once any launch plan has asked for it (Wp).
BLOCK_PLANES = ('.qkv', '.qkv_t', '.o', '.o_t', '.q', '.q_t', '.kv', '.kv_t', '.f1', '.f1_t', '.f2', '.f2_t')


class WeightLayout:
    """Woff: key -> element offset ('s.<key>': in the strip-pack stream; vectors: in the fp32 plane; else: in the matrix planes).
    prep / spack / spack_t: the table entries as tuples in the field order of PrepEntry / StripPackEntry (without PrepEntry's last field,
    which follows from `kind`); prep_keys / spack_keys / spack_t_keys: the region each entry writes into.
    n_w / n_f / n_s: elements of the matrix planes / the vector plane / the strip-pack stream; wl / fl / sl: their regions."""

    def __init__(self, dims, modes, opts, poff, pshape, merge_ckv_bwd_opt=True):
        D, d, p = dims, dims.d, dims.p
        x3, small = modes.x3, modes.strip_small
        wl, fl, sl = _Flat(), _Flat(), _Flat()
        W = {}
        prep, prep_keys = [], []
        spack, spack_keys, spack_t, spack_t_keys = [], [], [], []
        # x3 strip plans: the cross-attention K / V projections of ALL decoder layers (the same input: the encoder output, model_spec2midi.py:259,296)
        # as ONE launch with N = Ld * 2d instead of Ld launches that each re-read the encoder output
        self.merge_ckv = bool(modes.strip and x3 and not small and opts.merge_ckv and D.Ld in (2, 3) and qkv_planes(modes, opts, d, D.Hd, D.N, D.F))
        # ... and their backward (three layers): one weight-gradient product with six segments, the encoder-output gradient as two K = 768 halves
        self.merge_ckv_bwd = self.merge_ckv and D.Ld == 3 and merge_ckv_bwd_opt

        def put(key, entry):
            prep.append(entry)
            prep_keys.append(key)

        def mat(key, srcs, rows_each, cols, transposed, numel=None):
            """srcs: parameter names stacked along rows; returns plane offset of the [sum rows, cols] (or transposed) matrix."""
            rows = rows_each * len(srcs)
            if transposed:
                off = wl.add(key, numel or cols * _align(rows, 32), 64)
                for i, s in enumerate(srcs):
                    put(key, (poff[s], off + i * rows_each, rows_each, cols, cols, _align(rows, 32), 1))
            else:
                off = wl.add(key, numel or _align(rows, 64) * cols, 64)
                for i, s in enumerate(srcs):
                    put(key, (poff[s], off + i * rows_each * cols, rows_each, cols, cols, cols, 0))
            W[key] = off

        def mat2(key, srcs, rows_each, cols, numel=None, numel_t=None):
            """the matrix and its transpose (the backward's operand)"""
            mat(key, srcs, rows_each, cols, False, numel)
            mat(key + '_t', srcs, rows_each, cols, True, numel_t)

        def vec(key, srcs, n_each):
            off = fl.add(key, n_each * len(srcs), 8)
            for i, s in enumerate(srcs):
                put(key, (poff[s], off + i * n_each, 1, n_each, n_each, n_each, 2))
            W[key] = off

        def attn(pre, key, cross):
            """self attention: fc_q | fc_k | fc_v stacked; cross attention: fc_q alone (its input differs), fc_k | fc_v stacked"""
            if cross:
                mat2(key + '.q', [pre + 'fc_q.weight'], d, d)
            stacked, names = ('.kv', ['fc_k', 'fc_v']) if cross else ('.qkv', ['fc_q', 'fc_k', 'fc_v'])
            mat2(key + stacked, [pre + n + '.weight' for n in names], d, d)
            vec(key + stacked + '_b', [pre + n + '.bias' for n in names], d)
            mat2(key + '.o', [pre + 'fc_o.weight'], d, d)

        def ffn(pre, key):
            mat2(key + '.f1', [pre + 'fc_1.weight'], p, d)                                  # fc_1.weight [p, d]
            mat2(key + '.f2', [pre + 'fc_2.weight'], d, p, numel_t=_align(p, 64) * d)      # fc_2.weight [d, p]

        def heads(tag, key):
            """the four output heads of one decoder half as ONE [NHp, d] matrix: velocity rows [0, V), then onset, offset, mpe"""
            NHp, V = D.NHp, D.V
            rows = [('velocity', V, 0)] + [(nm, 1, V + i) for i, nm in enumerate(('onset', 'offset', 'mpe'))]
            src = lambda nm, what: poff['decoder_spec2midi.fc_%s_%s.%s' % (nm, tag, what)]
            W[key] = off = wl.add(key, NHp * d, 64)
            W[key + '_t'] = offt = wl.add(key + '_t', d * NHp, 64)
            W[key + '_b'] = ob = fl.add(key + '_b', NHp, 8)
            for nm, n, r0 in rows:
                put(key, (src(nm, 'weight'), off + r0 * d, n, d, d, d, 0))
            for nm, n, r0 in rows:
                put(key + '_t', (src(nm, 'weight'), offt + r0, n, d, d, NHp, 1))
            for nm, n, r0 in rows:
                put(key + '_b', (src(nm, 'bias'), ob + r0, 1, n, n, n, 2))

        def pack(key, parts, Ktot, Ntot, transpose=False, order=0, stride=1, offset=0, base=None, numel=None):
            """parts: (parameter name, n0, k0) blocks of the logical [Ntot, Ktot] matrix; returns the stream's element offset.
            x3: every fragment is a (hi, lo) pair -- twice the elements; slots come in pairs (stream position = offset + stride * (slot >> 1) +
            (slot & 1)), so a plain stream has stride 2 and the fused block's two matrices stride 4 with offsets 0 / 2; the transposed
            (backward) matrices are packed as bf16 halves by a table of their own, the others as fp16 halves.
            Small-width family (order 2, both precisions): compact packs, the (hi, lo) pair of (k chunk c, tile t) at pair index
            offset + c * NT + t (`offset`: pairs in front of this matrix, `numel`: pairs of the stream), 1024 int16 elements per pair."""
            if small:
                numel, order, stride = (numel or (Ktot // 16) * (Ntot // 32)) * 1024, 2, Ntot // 32
            elif x3:
                numel, stride, offset = 2 * (numel or Ntot * Ktot), 2 * stride, 2 * offset
            if base is None:
                base = sl.add(key, numel or Ntot * Ktot, 512)
                W['s.' + key] = base
            to_t = transpose and (x3 or small)
            for name, n0, k0 in parts:
                rows, cols = pshape[name]
                (spack_t if to_t else spack).append((poff[name], base, rows, cols, cols, 1 if transpose else 0, n0, k0, Ktot, order, stride, offset))
                (spack_t_keys if to_t else spack_keys).append(key)
            return base

        def strip_attn(pre, key, cross):
            wq, wk, wv, wo = (pre + n + '.weight' for n in ('fc_q', 'fc_k', 'fc_v', 'fc_o'))
            tm = 1 if x3 else 0                       # x3: the K == 256 linears without LayerNorm take the tile-major pack (csrc/x3_strip.hip)
            if cross:
                pack(key + '.q', [(wq, 0, 0)], d, d, order=tm)
                if not self.merge_ckv:               # (merged: one stream for all layers, 'dec.ca.kv_all' below)
                    pack(key + '.kv', [(wk, 0, 0), (wv, d, 0)], d, 2 * d, order=tm)
                pack(key + '.q_t', [(wq, 0, 0)], d, d, transpose=True, order=tm)
                if not self.merge_ckv_bwd:           # (merged backward: 'dec.ca.kv_all_t0/1' below)
                    pack(key + '.kv_t', [(wk, 0, 0), (wv, 0, d)], 2 * d, d, transpose=True)
            else:
                pack(key + '.qkv', [(wq, 0, 0), (wk, d, 0), (wv, 2 * d, 0)], d, 3 * d, order=tm)
                pack(key + '.qkv_t', [(wq, 0, 0), (wk, 0, d), (wv, 0, 2 * d)], 3 * d, d, transpose=True)
            if small:
                pack(key + '.o', [(wo, 0, 0)], d, d)
                pack(key + '.o_t', [(wo, 0, 0)], d, d, transpose=True)
            else:
                pack(key + '.o_t', [(wo, 0, 0)], d, d, transpose=True, order=tm)
                pack(key + '.o', [(wo, 0, 0)], d, d)  # LAST: the block's FFN stream follows it (hftt_attn_out_ffn_fwd reads the two as one)

        def strip_ffn(pre, key):
            w1, w2 = pre + 'fc_1.weight', pre + 'fc_2.weight'          # [p, d], [d, p]
            if small:
                n1, n2 = (d // 16) * (p // 32), (p // 16) * (d // 32)
                first, second = dict(numel=n1 + n2), dict(offset=n1)
            else:
                first, second = dict(order=1, stride=2, offset=0, numel=2 * d * p), dict(order=0, stride=2, offset=1)
            base = pack(key + '.ffn', [(w1, 0, 0)], d, p, **first)
            pack(key + '.ffn', [(w2, 0, 0)], p, d, base=base, **second)
            # dX half of the backward: first matrix fc_2.weight^T [p, d], second fc_1.weight^T [d, p]
            base = pack(key + '.ffn_t', [(w2, 0, 0)], d, p, transpose=True, **first)
            pack(key + '.ffn_t', [(w1, 0, 0)], p, d, transpose=True, base=base, **second)

        W['embed'] = wl.add('embed', _align(d, 64) * D.Kp, 64)
        W['embed_b'] = fl.add('embed_b', d, 8)
        blocks = []                                  # (prefix, key, has self attention, has cross attention)
        for i in range(D.Le):
            blocks.append((f'encoder_spec2midi.layers_freq.{i}.', f'enc{i}', True, False))
        blocks.append(('decoder_spec2midi.layer_zero_freq.', 'dec0', False, True))
        for i in range(D.Ld - 1):
            blocks.append((f'decoder_spec2midi.layers_freq.{i}.', f'dec{i + 1}', True, True))
        for i in range(D.Ld):
            blocks.append((f'decoder_spec2midi.layers_time.{i}.', f'time{i}', True, False))
        for pre, key, has_self, has_cross in blocks:
            if key == 'time0':
                heads('freq', 'heads_f')
            if has_self:
                attn(pre + 'self_attention.', key + '.sa', False)
            if has_cross:
                attn(pre + 'encoder_attention.', key + '.ca', True)
            ffn(pre + 'positionwise_feedforward.', key)
            if modes.strip:
                if has_self:
                    strip_attn(pre + 'self_attention.', key + '.sa', False)
                if has_cross:
                    strip_attn(pre + 'encoder_attention.', key + '.ca', True)
                strip_ffn(pre + 'positionwise_feedforward.', key)
                if x3 and not small:
                    # the joined forward launch (hftt_attn_out_ffn_fwd) takes ONE weight pointer: a block's fc_o pack (the hi / lo pairs of a
                    # [d, d] matrix: 2 * d * d int16 elements, 2 * 2 * d * d bytes) directly followed by its FFN pack
                    o = W['s.' + key + ('.ca.o' if has_cross else '.sa.o')]
                    assert W['s.' + key + '.ffn'] == o + 2 * d * d, 'strip packs of %s: .ffn does not follow .o' % key
        heads('time', 'heads_t')
        if self.merge_ckv:
            cross = [('decoder_spec2midi.layer_zero_freq.' if j == 0 else f'decoder_spec2midi.layers_freq.{j - 1}.') + 'encoder_attention.' for j in range(D.Ld)]
            parts = []
            for j, pre in enumerate(cross):
                parts += [(pre + 'fc_k.weight', 2 * j * d, 0), (pre + 'fc_v.weight', (2 * j + 1) * d, 0)]
            pack('dec.ca.kv_all', parts, d, D.Ld * 2 * d, order=1)
            if self.merge_ckv_bwd:                       # backward: dX of the stacked projection as two K = 768 halves of the [d, 6d] transposed matrix
                names = [pre + n + '.weight' for pre in cross for n in ('fc_k', 'fc_v')]
                for half in range(2):
                    pack('dec.ca.kv_all_t%d' % half, [(names[3 * half + i], 0, i * d) for i in range(3)], 3 * d, d, transpose=True)
            vec('dec.ca.kv_all_b', [pre + n + '.bias' for pre in cross for n in ('fc_k', 'fc_v')], d)
        if modes.bfs:                                # bf16 copy of the note position table: the (broadcast) residual of decoder layer zero
            W['dec_pos_bf'] = off = wl.add('dec_pos_bf', D.N * d, 64)
            put('dec_pos_bf', (poff['decoder_spec2midi.pos_embedding_freq.weight'], off, D.N, d, d, d, 0))

        self.Woff = W
        self.prep, self.prep_keys = prep, prep_keys
        self.spack, self.spack_keys, self.spack_t, self.spack_t_keys = spack, spack_keys, spack_t, spack_t_keys
        self.wl, self.fl, self.sl = wl, fl, sl
        self.n_w, self.n_f, self.n_s = _align(wl.off, 64), _align(fl.off, 8), _align(sl.off, 512)

    def prep_for(self, used):
        """the prep entries an engine needs once its plans have asked for the planes `used` (keys): every vector and whole-model matrix,
        and of the per-block planes only the used ones"""
        return [e for e, key in zip(self.prep, self.prep_keys) if e[6] == 2 or not key.endswith(BLOCK_PLANES) or key in used]
