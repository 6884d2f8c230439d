"""x3 TN GEMMs (weight gradients, split bf16 operands: npass 4) at the shapes of the paper-size step: launch time (main + reduce kernels together)
and algorithmic TB/s.  usage: python tools/bench_tn_x3.py   (tools/ablate_tn.sh runs it on a build whose loader does not split; HFTT_LIB_PATH
picks another library, HFTT_TN_PIPE=0 the reference step schedule of this one).  The last rows are the masked form (HFTT_TN_DY_DROP, the
step's 128 x 256 and bf16-X launches) and the two small tiles of the d = 64 model."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'nylon-amt_amd'))
import torch
from hftt_hip import ops

dev = torch.device('cuda:0')
g = torch.Generator(device=dev).manual_seed(3)
FORMS = ((768, 256, False, False, None), (256, 256, False, False, None), (512, 256, False, False, None), (256, 512, False, True, None), (512, 256, True, False, None))
MASKED = ((256, 256, False, False, (0.1, 3, 77)), (256, 512, False, True, (0.1, 3, 77)))
SMALL = ((128, 128, False, False, None), (64, 64, False, False, None))
for M, forms in ((262144, FORMS + MASKED), (90112, FORMS + MASKED + SMALL)):
    for (N, K, ybf, xbf, drop) in forms:
        dY = torch.randn(M, N, generator=g, device=dev); X = torch.randn(M, K, generator=g, device=dev)
        if ybf: dY = dY.bfloat16()
        if xbf: X = X.bfloat16()
        dW, db = ops.gemm_tn(dY, X, npass=4, dy_drop=drop); torch.cuda.synchronize()
        t = []
        for _ in range(3):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5): dW, db = ops.gemm_tn(dY, X, npass=4, dy_drop=drop)
            e1.record(); torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / 5 * 1e3)
        us = min(t)
        nbytes = M * (N * dY.element_size() + K * X.element_size())
        print(f'M={M:7d} N={N} K={K} dY {"bf16" if ybf else "fp32"} X {"bf16" if xbf else "fp32"}{" masked" if drop else ""}: {us:7.1f} us  {nbytes / us / 1e6:5.2f} TB/s', flush=True)
