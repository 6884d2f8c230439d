"""The GEMM, strip, fused-FFN and attention kernels against fp64 IN THE LAYOUTS THE ENGINE LAUNCHES (hftt_hip/plan.py), with guard elements
round every output and NaN round every input (tests/engine_layouts.py: the arena, the case tables, the layout signature).

The other kernel tests go through hftt_hip/ops.py, whose wrappers hard-code ldc == N, one TN segment, beta = 0, K_out == K, res_mod = 0, fresh
contiguous outputs and no aliasing.  The plan builder launches none of the kernels below that way.  Held here, per case:

  * every element outside the documented footprint of an output (one guard row in front and behind, the gap columns [N, ld) of every row, the
    neighbouring column blocks that belong to nobody) keeps the sentinel to the bit; every element inside is written;
  * no NaN in a result: the gaps and guard rows of the inputs hold NaN, so a value from outside an operand's footprint that takes part in
    arithmetic shows;
  * the fp64 reference of the same operation from the rounded inputs the kernel reads, under the bound the kernel and mode already carry in
    the suite (no new tolerance: engine_layouts.py names the source of each);
  * the same launch on contiguous, non-aliased operands gives the same bits (every case here: no dispatcher predicate depends on a leading
    dimension or an alias at these shapes -- the all-bf16 attention form's stride-multiple-of-8 rule holds for both launches, the vector
    predicate of dispatch_nt_bf16 too).  For the TN GEMM the twin is the one-segment launch with K_out == K and beta = 0, whose rows and
    columns each segment must equal (beta = 1: prior + twin, one fp32 rounding); for the fused forward it is the inference form.

TN GEMM: three segments of the fused q / k / v gradient, two and six of the (stacked) cross-attention K / V, the three-segment small reduce
(N 192, K 64), the four head segments on N = NHp (three of one row, rows beyond NH in no segment), K_out = 65 of K = 96 (embedding fold),
caller-ordered destinations, beta = 1 on prior contents.  Block NT: ldc = NHp > N = NH (131 into 192), C == residual in place, add_table /
add_mod, res_mod below M under LayerNorm, the gate.  Strip linear: x at a column offset with ldx = 6d > K = 3d, C == residual in place,
res_mod = N_notes under LayerNorm, the stacked K / V planes at N = ldc = 1536, HFTT_SL_X_DROP; the d = 64 families at the same M.  Fused FFN
dX: residual, h_out, gate, dy masked on load (x3), and the all-bf16 forms.  fc_o + LayerNorm + FFN as one launch (hftt_attn_out_ffn_fwd) with
the broadcast residual, every saved tensor guarded, and the inference plan's form that writes y alone.  Attention forward + backward: q / k / v and dq / dk / dv interleaved in [n L, 3d]; K / V at
column block 1 of a three-layer stack (ldk = 6d) and dk / dv into the matching block of the [n Lk, 6d] gradient; the shared query with
sequence stride 0 and a per-sequence dq; dropout and the attention map.  Modes: x3 (npass 2 forward, 4 backward, planes and fp32 operands),
bf16 (all-bf16 flags), parity (npass 3), each where its plans contain the layout.

test_every_layout_the_plans_launch_has_a_case builds the engine at d 256 / ff 512 / three decoder layers and at d 64 in the three precision
modes and fails, printing the signature, for a launch whose layout signature no case of the tables has."""
import pytest
import torch

import util
from util import O
import engine_layouts as L

pytestmark = pytest.mark.gpu

FIGURES = {}          # case -> [(what, measured, bound)]: printed per case; gpu jobs collect them for the report


def _run(dev, build, launch, check, twin_equal, *key):
    ctx = build(dev, *key)
    launch(dev, ctx)
    torch.cuda.synchronize(dev)
    L.check_planes(ctx)
    check(ctx, FIGURES)
    tw = build(dev, *key, twin=True)
    launch(dev, tw)
    torch.cuda.synchronize(dev)
    L.check_planes(tw)
    twin_equal(ctx, tw)


@pytest.mark.parametrize('case,mode', [(c, m) for c, v in L.TN_CASES.items() for m in v['modes']])
def test_gemm_tn_segments(dev, case, mode):
    _run(dev, L.build_tn, L.launch_tn, L.check_tn, L.twin_equal_tn, case, mode)


@pytest.mark.parametrize('case,mode', [(c, m) for c, v in L.NT_CASES.items() for m in v['modes']])
def test_gemm_nt_layouts(dev, case, mode):
    _run(dev, L.build_nt, L.launch_nt, L.check_nt, L.twin_equal, case, mode)


@pytest.mark.parametrize('M', L.SL_MS)
@pytest.mark.parametrize('case,fam', [(c, f) for c, v in L.SL_CASES.items() for f in v['fams']])
def test_strip_linear_layouts(dev, case, fam, M):
    _run(dev, L.build_sl, L.launch_sl, L.check_sl, L.twin_equal, case, fam, M)


@pytest.mark.parametrize('M', L.SL_MS)
@pytest.mark.parametrize('case', list(L.FFN_CASES))
def test_fused_ffn_dx_layout(dev, case, M):
    _run(dev, L.build_ffn, L.launch_ffn, L.check_ffn, L.twin_equal, case, M)


@pytest.mark.parametrize('M', L.SL_MS)
@pytest.mark.parametrize('case', list(L.OFFN_CASES))
def test_attention_output_and_ffn_as_one_launch_layout(dev, case, M):
    """(its second launch is the inference plan's form, which writes y and the statistics only: the same bits)"""
    _run(dev, L.build_offn, L.launch_offn, L.check_offn, L.twin_equal_offn, case, M)


@pytest.mark.parametrize('case,mode', [(c, m) for c, v in L.ATTN_CASES.items() for m in v['modes']])
def test_attention_layouts(dev, case, mode):
    _run(dev, L.build_attn, L.launch_attn, L.check_attn, L.twin_equal, case, mode)


# ------------------------------------------------------------------------------------------------------------------ the coverage pin
_AXES = dict(n_margin=4, n_frame=16, n_bin=32, cnn_channel=4, cnn_kernel=5, n_note=8, n_velocity=16)
PIN_CONFIGS = {
    'd256': O.HfttConfig(hid_dim=256, pf_dim=512, enc_layer=1, dec_layer=3, enc_head=4, dec_head=4, **_AXES),      # strip plans, merged cross K / V
    'd64': O.HfttConfig(hid_dim=64, pf_dim=128, enc_layer=1, dec_layer=2, enc_head=2, dec_head=2, **_AXES),        # the small-width families
}


def plan_layouts(dev, cfg, precision):
    model = util.build_model(cfg, 5, dropout=0.1).to(dev)
    model.hftt_precision = precision
    model.train()
    return L.plan_signatures(model.hftt_engine().workspace(1))


@pytest.mark.parametrize('precision', ['x3', 'bf16', 'parity'])
@pytest.mark.parametrize('cfg', list(PIN_CONFIGS))
def test_every_layout_the_plans_launch_has_a_case(dev, cfg, precision):
    """walks ws['fwd'], ws['fwd_inf'] and ws['bwd'] (it launches nothing): a plan change that invents a layout has to bring its kernel test along"""
    have = L.table_signatures(dev)
    missing = {s: at for s, at in plan_layouts(dev, PIN_CONFIGS[cfg], precision).items() if not L.is_plain(s) and s not in have}
    for s, at in sorted(missing.items(), key=str):
        print('no case for %s   (first at %s)' % (s, at))
    assert not missing, '%d layouts of the %s / %s plans have no case in tests/engine_layouts.py' % (len(missing), cfg, precision)
