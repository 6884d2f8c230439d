"""The weight layout (hftt_hip/layout.py) is pure arithmetic: its invariants are checked here without a GPU and without libhftt_hip.so,
from parameter shapes only, for the benchmark's two configurations and the test suite's MINI in every precision.  No recorded numbers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'nylon-amt_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from hftt_hip import layout as L   # noqa: E402


def _configs():
    import bench
    import util
    mini = {k: getattr(util.MINI, k) for k in bench.BenchCfg._fields}
    return {'paper': bench.CONFIGS['paper']._asdict(), 'tiny': bench.CONFIGS['tiny']._asdict(), 'mini': mini}


def _named_shapes(cfg):
    """parameter names and shapes in state_dict order, from the module classes (the values are not used)"""
    import torch
    from model.model_spec2midi import Encoder_SPEC2MIDI, Decoder_SPEC2MIDI, Model_SPEC2MIDI
    c = cfg
    enc = Encoder_SPEC2MIDI(c['n_margin'], c['n_frame'], c['n_bin'], c['cnn_channel'], c['cnn_kernel'], c['hid_dim'], c['enc_layer'], c['enc_head'],
                            c['pf_dim'], 0.0, 'cpu')
    dec = Decoder_SPEC2MIDI(c['n_frame'], c['n_bin'], c['n_note'], c['n_velocity'], c['hid_dim'], c['dec_layer'], c['dec_head'], c['pf_dim'], 0.0, 'cpu')
    return [(n, tuple(p.shape)) for n, p in Model_SPEC2MIDI(enc, dec).named_parameters()]


def _layout(cfg, precision, **kw):
    named = _named_shapes(cfg)
    numel = lambda s: int(__import__('math').prod(s))
    offs, total = L.flat_offsets((n, numel(s)) for n, s in named)
    poff = {n: o for (n, _), o in zip(named, offs)}
    pshape = dict(named)
    dims, opts = L.model_dims(cfg), L.Options()
    modes = L.precision_modes(dims.d, dims.p, L.PRECISION_NPASS[precision], opts)
    return dims, modes, L.WeightLayout(dims, modes, opts, poff, pshape, **kw), poff, {n: numel(s) for n, s in named}, total


CASES = [(c, p) for c in ('paper', 'tiny', 'mini') for p in ('parity', 'bf16', 'x3')]


def _check_regions(flat, total, align):
    spans = sorted((off, off + flat.sizes[k], k) for k, off in flat.items.items())
    for off, end, k in spans:
        assert off % align == 0 and end > off, k
    for (_, end, k), (off2, _, k2) in zip(spans, spans[1:]):
        assert end <= off2, (k, k2)
    assert not spans or spans[-1][1] <= total


@pytest.mark.parametrize('cname,precision', CASES)
def test_regions_do_not_overlap_and_are_aligned(cname, precision):
    dims, modes, lay, poff, pnumel, total = _layout(_configs()[cname], precision)
    _check_regions(lay.wl, lay.n_w, 64)
    _check_regions(lay.fl, lay.n_f, 8)
    _check_regions(lay.sl, lay.n_s, 512)
    # every key of the offset map names a region of its allocator, at that offset
    for key, off in lay.Woff.items():
        if key.startswith('s.'):
            assert lay.sl.items[key[2:]] == off
        else:
            assert (lay.wl.items.get(key), lay.fl.items.get(key)).count(off) >= 1, key
    assert modes.strip == bool(lay.spack) and (cname, precision, modes.strip) != ('paper', 'x3', False)


@pytest.mark.parametrize('cname,precision', CASES)
def test_prep_entries_stay_inside_their_region(cname, precision):
    dims, modes, lay, poff, pnumel, total = _layout(_configs()[cname], precision)
    assert len(lay.prep) == len(lay.prep_keys)
    by_off = {o: n for n, o in poff.items()}
    for (so, do, rows, cols, sld, dld, kind), key in zip(lay.prep, lay.prep_keys):
        flat = lay.fl if kind == 2 else lay.wl
        lo, hi = flat.items[key], flat.items[key] + flat.sizes[key]
        # csrc/prep.hip: kind 0 writes dst[r * dld + c], kind 1 (transposed) dst[c * dld + r], kind 2 a vector of `cols` elements
        last = {0: (rows - 1) * dld + cols, 1: (cols - 1) * dld + rows, 2: cols}[kind]
        assert lo <= do and do + last <= hi, (key, kind)
        assert sld >= cols and dld >= (rows if kind == 1 else cols)
        assert pnumel[by_off[so]] == rows * sld                     # the source is one whole parameter
    # what the engine prepares when no plan has asked for a per-block plane: everything else, still inside the table
    always = lay.prep_for(set())
    assert set(always) <= set(lay.prep) and all(e in always for e, k in zip(lay.prep, lay.prep_keys) if not k.endswith(L.BLOCK_PLANES))
    assert lay.prep_for(set(lay.prep_keys)) == lay.prep


@pytest.mark.parametrize('cname,precision', CASES)
def test_strip_pack_entries_tile_their_region(cname, precision):
    dims, modes, lay, poff, pnumel, total = _layout(_configs()[cname], precision)
    pair = 2 if (modes.x3 or modes.strip_small) else 1               # (hi, lo) fragments: twice the elements
    covered = {}
    for entries, keys in ((lay.spack, lay.spack_keys), (lay.spack_t, lay.spack_t_keys)):
        assert len(entries) == len(keys)
        for (so, base, rows, cols, sld, transpose, n0, k0, Ktot, order, stride, offset), key in zip(entries, keys):
            assert base == lay.sl.items[key] and base % 512 == 0, key
            assert sld == cols and k0 + (rows if transpose else cols) <= Ktot, key
            covered[key] = covered.get(key, 0) + rows * cols * pair
    assert covered == {k: lay.sl.sizes[k] for k in lay.sl.items}     # the blocks of a stream fill it exactly: no entry can reach past it
    if modes.x3 and not modes.strip_small:
        assert not set(lay.spack_keys) & set(lay.spack_t_keys)       # fp16 halves forward, bf16 halves backward: a stream has one table


@pytest.mark.parametrize('cname', ['paper', 'tiny', 'mini'])
def test_x3_ffn_pack_follows_the_out_projection_pack(cname):
    """hftt_attn_out_ffn_fwd reads a block's fc_o pack and its FFN pack through ONE pointer: the FFN stream starts where the hi / lo pairs
    of the [d, d] matrix end (2 * d * d int16 elements = 2 * 2 * d * d bytes)"""
    cfg = _configs()[cname]
    dims, modes, lay, *_ = _layout(cfg, 'x3')
    if not (modes.strip and not modes.strip_small):
        assert cname != 'paper'
        return
    d = dims.d
    blocks = [(f'enc{i}', 'sa') for i in range(dims.Le)] + [(f'dec{j}', 'ca') for j in range(dims.Ld)] + [(f'time{i}', 'sa') for i in range(dims.Ld)]
    for key, att in blocks:
        assert lay.Woff[f's.{key}.ffn'] == lay.Woff[f's.{key}.{att}.o'] + 2 * d * d, key
        assert 2 * (lay.Woff[f's.{key}.ffn'] - lay.Woff[f's.{key}.{att}.o']) == 2 * 2 * d * d


def test_merged_cross_kv_stream():
    cfg = _configs()['paper']
    for precision, pair in (('x3', 2), ('bf16', 1)):
        for ld in (1, 2, 3, 4):
            dims, modes, lay, *_ = _layout(dict(cfg, dec_layer=ld), precision)
            assert lay.merge_ckv == (precision == 'x3' and ld in (2, 3)) and lay.merge_ckv_bwd == (lay.merge_ckv and ld == 3)
            assert ('dec.ca.kv_all' in lay.sl.items) == lay.merge_ckv
            if lay.merge_ckv:
                assert lay.sl.sizes['dec.ca.kv_all'] == pair * ld * 2 * dims.d * dims.d
                assert lay.fl.sizes['dec.ca.kv_all_b'] == ld * 2 * dims.d
                assert not any(k.endswith('.ca.kv') for k in lay.sl.items)
            assert all(f'dec{j}.ca.kv_t' in lay.sl.items for j in range(ld)) == (not lay.merge_ckv_bwd)
    dims, modes, lay, *_ = _layout(cfg, 'x3', merge_ckv_bwd_opt=False)
    assert lay.merge_ckv and not lay.merge_ckv_bwd and 'dec.ca.kv_all_t0' not in lay.sl.items
