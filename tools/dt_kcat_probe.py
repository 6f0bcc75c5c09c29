"""Stand-alone timing of the input-gradient group of a layer (run from the repository root: python tools/dt_kcat_probe.py): K = 1536
as one product, K = 1792 from one A, K = 1536 + 256 from two tensors with leading dimensions of their own (lda2); operands hot (back to
back) and cold (a 1.5 GB copy in between).  profiles/dt_kcat_ab.txt holds a run."""
import sys, os
sys.path.insert(0, os.getcwd())
import torch
from gotennet_amd import engine, _lib
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
r = lambda *s: torch.randn(*s, device=dev, generator=g)
E, Na, F = 54368, 2688, 256
ge, ge2, gp = r(E, 1536), r(E, 1792), r(E, F)
W15, W17 = r(F, 1536) / 8, r(F, 1792) / 8
gt, C = r(E, F), torch.empty(E, F, device=dev)
gx, gv, Ws, Wv = r(Na, 1280), r(Na, 1280), r(F, 1280) / 8, r(F, 1280) / 8
gn, pre_n = torch.zeros(Na, 4 * F, device=dev), r(Na, 4 * F)
gq, Wqk, Rq, Dq = r(Na, 512), r(F, 512) / 8, r(Na, F), torch.empty(Na, F, device=dev)
riders = [dict(A=gx, lda=1280, W=Ws, C=gn, ldc=4 * F, rows=Na, nout=F, K=1280, c_off=2 * F, dgate=pre_n, g_off=2 * F),
          dict(A=gv, lda=1280, W=Wv, C=gn, ldc=4 * F, rows=Na, nout=F, K=1280, c_off=3 * F, dgate=pre_n, g_off=3 * F),
          dict(A=gq, lda=512, W=Wqk, C=Dq, ldc=F, rows=Na, nout=F, K=512, res=Rq)]
m1 = dict(A=r(Na, 512), lda=512, W=r(F, 512) / 8, C=torch.empty(Na, F, device=dev), ldc=F, rows=Na, nout=F, K=512, dgate=r(Na, F))
cases = {
    "K=1536 one A + riders": [dict(A=ge, lda=1536, W=W15, C=C, ldc=F, rows=E, nout=F, K=1536, res=gt)] + riders,
    "K=1792 one A + riders": [dict(A=ge2, lda=1792, W=W17, C=C, ldc=F, rows=E, nout=F, K=1792, res=gt)] + riders,
    "K=256 (Wt) + m1 rider": [dict(A=gp, lda=F, W=r(F, F) / 8, C=C, ldc=F, rows=E, nout=F, K=F, res=gt), m1],
    "m1 alone": [m1],
}
if _lib.ABI_VERSION >= 10:
    cases["K=1536+256 two A (lda2) + riders"] = [dict(A=ge, lda=1536, A2=gp, lda2=F, a_seg=1536, W=W17, C=C, ldc=F, rows=E,
                                                      nout=F, K=1792, res=gt)] + riders
big = torch.empty(384 * 1024 * 1024, device=dev)
big2 = torch.empty_like(big)
def timeit(probs, cold, n=12):
    ts = []
    for i in range(n + 3):
        if cold:
            big2.copy_(big)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); engine.gemm_group(probs, mode="f16x2"); b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]
print(f"# ABI {_lib.ABI_VERSION}; us per launch, median / min of 12")
for name, probs in cases.items():
    h, c = timeit(probs, False), timeit(probs, True)
    print(f"{name:36s} hot {h[0]:7.1f} / {h[1]:7.1f}    cold {c[0]:7.1f} / {c[1]:7.1f}", flush=True)
