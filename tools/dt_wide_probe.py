"""Stand-alone A/B of the two 128-row forms of the f16x2 slab kernel (run from the repository root: python tools/dt_wide_probe.py):
the launches of the force backward that the eight-wave 128 x 256 form is routed to, and the ones it is not, each forced onto the
four-wave 128 x 128 tile and onto the eight-wave tile (gn_gemm_group_f16x2_form), operands hot (back to back) and cold (a 1.5 GB
copy in between).  profiles/dt_wide_ab.txt holds a run."""
import sys, os
sys.path.insert(0, os.getcwd())
import torch
from gotennet_amd import engine, _lib
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
r = lambda *s: torch.randn(*s, device=dev, generator=g)
E, Na, F = 54368, 2688, 256
ge, gp = r(E, 1536), r(E, F)
W17, W15, W12 = r(F, 1792) / 8, r(F, 1536) / 8, r(F, 1280) / 8
gt, C = r(E, F), torch.empty(E, F, device=dev)
gx, gv, Ws, Wv = r(Na, 1280), r(Na, 1280), r(F, 1280) / 8, r(F, 1280) / 8
gn, pre_n = torch.zeros(Na, 4 * F, device=dev), r(Na, 4 * F)
gq, Wqk, Rq, Dq = r(Na, 512), r(F, 512) / 8, r(Na, F), torch.empty(Na, F, device=dev)
riders = [dict(A=gx, lda=1280, W=Ws, C=gn, ldc=4 * F, rows=Na, nout=F, K=1280, c_off=2 * F, dgate=pre_n, g_off=2 * F),
          dict(A=gv, lda=1280, W=Wv, C=gn, ldc=4 * F, rows=Na, nout=F, K=1280, c_off=3 * F, dgate=pre_n, g_off=3 * F),
          dict(A=gq, lda=512, W=Wqk, C=Dq, ldc=F, rows=Na, nout=F, K=512, res=Rq)]
m1 = dict(A=r(Na, 512), lda=512, W=r(F, 512) / 8, C=torch.empty(Na, F, device=dev), ldc=F, rows=Na, nout=F, K=512, dgate=r(Na, F))
Xa, Xb, Wx = r(8064, 768), r(13440, 768), r(F, 768) / 8
cases = {
    "K=1536+256 two A (lda2) + riders": [dict(A=ge, lda=1536, A2=gp, lda2=F, a_seg=1536, W=W17, C=C, ldc=F, rows=E, nout=F, K=1792,
                                              res=gt)] + riders,
    "K=1024+256 two A (first layer) + riders": [dict(A=ge, lda=1536, A2=gp, lda2=F, a_seg=1024, W=W12, C=C, ldc=F, rows=E, nout=F,
                                                     K=1280, res=gt)] + riders,
    "K=1536 one A (last layer) + riders": [dict(A=ge, lda=1536, W=W15, C=C, ldc=F, rows=E, nout=F, K=1536)] + riders,
    "K=1792, no riders": [dict(A=ge, lda=1536, A2=gp, lda2=F, a_seg=1536, W=W17, C=C, ldc=F, rows=E, nout=F, K=1792, res=gt)],
    "gated K=256 + m1 rider": [dict(A=gp, lda=F, W=r(F, F) / 8, C=C, ldc=F, rows=E, nout=F, K=F, res=gt, gate=r(E, F), act=(0, F)), m1],
    "Xcat [8064 + 13440 x 256 x 768]": [dict(A=Xa, lda=768, W=Wx, C=torch.empty(8064, F, device=dev), ldc=F, rows=8064, nout=F, K=768),
                                        dict(A=Xb, lda=768, W=Wx, C=torch.empty(13440, F, device=dev), ldc=F, rows=13440, nout=F, K=768)],
}
big = torch.empty(384 * 1024 * 1024, device=dev)
big2 = torch.empty_like(big)


def timeit(probs, form, cold, n=12):
    ts = []
    for i in range(n + 3):
        if cold:
            big2.copy_(big)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); engine.gemm_group(probs, mode="f16x2", form=form); b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


print("# us per launch, median / min of 12; routed = what gn_gemm_group_f16x2 chooses")
for name, probs in cases.items():
    for label, form in (("routed", 0), ("4 waves 128x128", _lib.GEMM_FORM_BIG), ("8 waves 128x256", _lib.GEMM_FORM_BIG8)):
        h, c = timeit(probs, form, False), timeit(probs, form, True)
        print(f"{name:42s} {label:16s} hot {h[0]:7.1f} / {h[1]:7.1f}    cold {c[0]:7.1f} / {c[1]:7.1f}", flush=True)
