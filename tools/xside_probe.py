"""Stand-alone timing of the two X-side projection groups of a layer with an edge update, f16x2, in every route they can take
(run from the repository root: python tools/xside_probe.py).  Sizes: rMD17 aspirin (21 atoms, lmax 2: 8 rows of X per atom) at
1, 32, 64, 96 and 128 molecules.

  forward   X_p = X W_vu^T, EQ = X W_vq^T, EK_l = X_l W_vk_l^T: the four-problem group, routed and on the two 128-row slab tiles
            (gn_gemm_group_f16x2_form);
  backward  gX1 = gX + [gXp | gEQ | gEK_l] W^T per degree block (a_seg, res, row maps): routed and on the two 128-row slab tiles.

Operands hot (back to back) and cold (a 1.5 GB copy in between); profiles/xside_ab.txt holds a run."""
import sys, os
sys.path.insert(0, os.getcwd())
import torch
from gotennet_amd import engine, _lib
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
r = lambda *s: torch.randn(*s, device=dev, generator=g)
F, D = 256, 8
FORMS = [("routed", 0), ("4 waves 128x128", _lib.GEMM_FORM_BIG), ("8 waves 128x256", _lib.GEMM_FORM_BIG8)]
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


def groups(n_mol):
    N = 21 * n_mol
    X, Xp, EQ, EK = r(N, D, F), torch.empty(N, D, F, device=dev), torch.empty(N, D, F, device=dev), torch.empty(N, D, F, device=dev)
    Wvu, Wvq, Wvk = r(F, F) / 8, r(F, F) / 8, [r(F, F) / 8, r(F, F) / 8]
    blocks = [(0, 3 * N, (3, D, 0)), (1, 5 * N, (5, D, 3))]
    out = {"fwd four problems": [dict(A=X, lda=F, W=Wvu, C=Xp, ldc=F, rows=N * D, nout=F, K=F),
                                 dict(A=X, lda=F, W=Wvq, C=EQ, ldc=F, rows=N * D, nout=F, K=F)] +
                                [dict(A=X, lda=F, W=Wvk[k], C=EK, ldc=F, rows=rows, nout=F, K=F, rowmap=rm) for k, rows, rm in blocks]}
    gXp, gEQ, gEK, gX, gX1 = r(N, D, F), r(N, D, F), r(N, D, F), r(N, D, F), torch.empty(N, D, F, device=dev)
    out["bwd X-cat K=768"] = [dict(A=gXp, A2=gEQ, A3=gEK, a_seg=F, lda=F, W=r(F, 3 * F) / 8, C=gX1, ldc=F, rows=rows, nout=F,
                                   K=3 * F, rowmap=rm, res=gX) for k, rows, rm in blocks]
    return out


print(f"# ABI {_lib.ABI_VERSION}; us per launch, median / min of 12; routed = what gn_gemm_group_f16x2 chooses")
for n_mol in (1, 32, 64, 96, 128):
    for name, probs in groups(n_mol).items():
        for label, form in FORMS:
            h, c = timeit(probs, form, False), timeit(probs, form, True)
            print(f"{n_mol:4d} mol  {name:22s} {label:16s} hot {h[0]:7.1f} / {h[1]:7.1f}    cold {c[0]:7.1f} / {c[1]:7.1f}", flush=True)
