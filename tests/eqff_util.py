"""Yardstick of the EQFF node chain (gn_eqff_fused_forward / _backward and the launch sequence they replace): inputs at the
kernel's edges, an fp64 restatement of the chain and of its input-gradient, and the per-atom bounds.

The chain (reference gotennet.py:716-748 after X_p = X W_vu^T), per atom:

    n = sqrt(sum_D X_p^2 + eps);  ctx = [h | n];  pre = ctx W0^T + b0;  [m1 | m2] = SiLU(pre) W1^T + b1
    h' = h + m1;  X' = X + m2 * X_p
  input-gradient, given g_h, g_X of (h', X'):
    g_m = [g_h | sum_D g_X X_p];  g_pre = (g_m W1) * SiLU'(pre);  g_ctx = g_pre W0
    g_Xp = g_X * m2 + (g_ctx[:, F:] / n) * X_p;  g_h1 = g_h + g_ctx[:, :F]

Bounds (u = 2^-24)
------------------
The products.  In the default ("f16x2") arithmetic the fused kernel gives ONE fp16 exponent to the operand tile of its 8
atoms (atoms 8 b .. 8 b + 7, all K columns).  DESIGN section 4's per-row formula, with the tile as the exponent group:

    max_n |C[a, n] - ref[a, n]|  <=  beta(K, d_a) * max_n |ref[a, n]|,   beta = 2 sqrt(K) * max(2^-23, 2^(d_a - 41))

  d_a = log2(largest finite operand magnitude of the tile / of atom a's own row); K = 2F for the first product, F for the
  second.  Atoms with d_a <= 18 -- every atom of a batch of molecules -- are also held to NEAR = 4e-6 of their own
  max-norm.  The "split" arithmetic (exact bf16 triples) is row-wise: 4e-6 of the own max-norm for every atom.
The forward is checked product by product against fp64 products of the kernel's OWN fp32 input to each (it writes ctx, pre
  and [m1 | m2]), so nothing needs propagating there: ctx[:, F:] within (D + 3) u relative (D fused multiply-adds, the
  add of eps, a square root of 1 ulp); h' is one fp32 add and X' one fused multiply-add of stored values.
The backward writes no intermediate, so the two product bounds are carried to the outputs here, in fp64, element-wise:
    E_gm[a, F:]  = (D + 1) u sum_D |g_X X_p|                                      the serial fused multiply-adds
    E_P[a, :]    = B1_a + E_gm[a] |W1|,     B1_a = beta(2F, d1_a) max_n |P[a, n]|   P = g_m W1
    E_v[a, :]    = E_P[a] * |SiLU'(pre[a])| + 8 u |v[a]|                            v = g_pre; SiLU' = s (1 + x (1 - s)), s from
                                                                                   v_exp_f32 + v_rcp_f32 (2 u each) and five
                                                                                   roundings, less than 8 u in all
    E_gctx[a, :] = B2_a + E_v[a] |W0|,      B2_a = beta(F, d2_a) max_n |(v W0)[a, n]|
    |g_h1 - ref| <= E_gctx[a, :F] + u |g_h1|
    |g_Xp - ref| <= E_gctx[a, F:] |X_p| / n + 3 u (|g_X m2| + |g_ctx[:, F:] X_p / n|)   (product, division, fused multiply-add)
  d1 is taken from the tile of g_m, d2 from the tile of v.  For the "split" arithmetic B1, B2 are 4e-6 of the max-norms.
"""
import math

import torch

EQ_ATOMS = 8                                      # atoms per workgroup = per exponent group (csrc/gn_eqff_fused.hip)
U32 = 2.0 ** -24
NEAR, NEAR_D = 4e-6, 18.0
SILU = torch.nn.functional.silu
#: (F, N, D): every F sees a ragged N (1, 7, 9, 17) and a ragged D (3, 15, 35); D = 80 once; both run in both arithmetics
SHAPES = [(128, 1, 3), (128, 7, 8), (128, 9, 15), (128, 17, 24), (128, 8, 35), (128, 9, 80),
          (256, 1, 35), (256, 7, 15), (256, 8, 24), (256, 9, 3), (256, 17, 8)]
ARITH = {"split": 1, "f16x2": 2}


def bias(b):
    return 0.0 if b is None else b.double()


def dsilu(x):
    s = torch.sigmoid(x)
    return s * (1.0 + x * (1.0 - s))


def make(F, N, D, seed=0, hostile=None):
    """fp32 CPU inputs.  ``hostile``: None; "spread" (N = 17: tile 0 = rows of h, X_p, g_h, g_X scaled by 10^dec with dec
    over -10 .. 0 and one all-zero atom, tile 1 = entirely zero, tile 2 = ordinary; eps = 1e-24 and no biases (None), so
    that neither n nor b0 hides the spread from either product); "nonfinite" (an Inf in atom 2's h and g_h, a NaN in atom 5's X_p and g_X)."""
    g = torch.Generator().manual_seed(4242 + 97 * seed + F + 7 * N + D)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(F=F, N=N, D=D, eps=1e-8, hostile=hostile, h=rn(N, F), X=rn(N, D, F), Xp=rn(N, D, F), gh=rn(N, F), gX=rn(N, D, F),
             W0=rn(F, 2 * F) / math.sqrt(2 * F), b0=rn(F) * 0.1, W1=rn(2 * F, F) / math.sqrt(F), b1=rn(2 * F) * 0.1)
    if hostile == "spread":
        assert N == 17
        d["eps"] = 1e-24
        d["b0"] = d["b1"] = None
        dec = torch.tensor([0.0, -10.0, -3.0, -6.0, 0.0, -9.0, -1.0, -10.0] + [0.0] * 9)
        scale = 10.0 ** dec
        scale[4] = 0.0                             # the all-zero atom
        scale[8:16] = 0.0                          # the all-zero tile
        for k in ("h", "gh"):
            d[k] = d[k] * scale[:, None]
        for k in ("Xp", "gX"):
            d[k] = d[k] * scale[:, None, None]
        d["dec"] = dec
    elif hostile == "nonfinite":
        assert N >= 8
        d["h"][2, F // 2 + 1] = d["gh"][2, 5] = float("inf")
        d["Xp"][5, D // 2, 3] = d["gX"][5, 0, F - 1] = float("nan")
        d["bad"] = [2, 5]
    return d


def forward_ref(d):
    """fp64 chain from the fp32 inputs -> dict(ctx, pre, mm, h1, X1)."""
    F = d["F"]
    h, X, Xp = d["h"].double(), d["X"].double(), d["Xp"].double()
    ctx = torch.cat([h, torch.sqrt((Xp ** 2).sum(1) + d["eps"])], 1)
    pre = ctx @ d["W0"].double().t() + bias(d["b0"])
    mm = SILU(pre) @ d["W1"].double().t() + bias(d["b1"])
    return dict(ctx=ctx, pre=pre, mm=mm, h1=h + mm[:, :F], X1=X + mm[:, None, F:] * Xp)


def backward_ref(d, mm, ctx, pre):
    """fp64 input-gradient from the fp32 inputs and the SAVED tensors given -> dict(gm, P, v, gctx, gXp, gh1)."""
    F = d["F"]
    gh, gX, Xp = d["gh"].double(), d["gX"].double(), d["Xp"].double()
    mm, ctx, pre = mm.double(), ctx.double(), pre.double()
    gm = torch.cat([gh, (gX * Xp).sum(1)], 1)
    P = gm @ d["W1"].double()
    v = P * dsilu(pre)
    gctx = v @ d["W0"].double()
    gXp = gX * mm[:, None, F:] + (gctx[:, F:] / ctx[:, F:])[:, None, :] * Xp
    return dict(gm=gm, P=P, v=v, gctx=gctx, gXp=gXp, gh1=gh + gctx[:, :F])


def backward_autograd(d):
    """g_Xp, g_h1 by autograd of sum(g_h h') + sum(g_X X') through the fp64 chain (X held fixed: X_p is the variable)."""
    F = d["F"]
    h, Xp = d["h"].double().requires_grad_(), d["Xp"].double().requires_grad_()
    ctx = torch.cat([h, torch.sqrt((Xp ** 2).sum(1) + d["eps"])], 1)
    mm = SILU(ctx @ d["W0"].double().t() + bias(d["b0"])) @ d["W1"].double().t() + bias(d["b1"])
    loss = (d["gh"].double() * (h + mm[:, :F])).sum() + (d["gX"].double() * (d["X"].double() + mm[:, None, F:] * Xp)).sum()
    g_h1, g_Xp = torch.autograd.grad(loss, (h, Xp))
    return g_Xp, g_h1


def tile_d(op):
    """d_a of the module docstring for an operand [N, K] (non-finite entries do not count, as in the kernel); 0 for an
    all-zero row (its product is exactly the bias)."""
    N = op.shape[0]
    mag = torch.where(torch.isfinite(op), op.abs(), torch.zeros_like(op)).double().amax(1)
    pad = torch.zeros(-(-N // EQ_ATOMS) * EQ_ATOMS, dtype=torch.float64)
    pad[:N] = mag
    tile = pad.view(-1, EQ_ATOMS).amax(1).repeat_interleave(EQ_ATOMS)[:N]
    d = torch.log2(tile / mag)
    return torch.where(mag == 0, torch.zeros_like(d), d)


def beta(K, d, arith):
    """Per-atom relative bound of one product."""
    if arith == "split":
        return torch.full_like(d, NEAR)
    return 2.0 * math.sqrt(K) * torch.maximum(torch.full_like(d, 2.0 ** -23), 2.0 ** (d - 41.0))


def product_check(C, op, W, b, arith):
    """C (kernel) against op W^T + b in fp64 of the kernel's own operand -> (per-atom error / max-norm, per-atom beta, d)."""
    ref = op.double() @ W.double().t() + bias(b)
    d = tile_d(op)
    e, big = (C.double() - ref).abs().amax(1), ref.abs().amax(1)
    err = torch.where(e == 0, torch.zeros_like(e), e / big)                # (an exactly-zero row of an all-zero operand: 0)
    return err, beta(op.shape[1], d, arith), d


def backward_bounds(d, r, mm, ctx, pre, arith):
    """(E_gXp [N,D,F], E_gh1 [N,F]) of the module docstring; r = backward_ref(d, mm, ctx, pre) on the same saved tensors."""
    F, D = d["F"], d["D"]
    gX, Xp = d["gX"].double(), d["Xp"].double()
    W1a, W0a = d["W1"].double().abs(), d["W0"].double().abs()
    n = ctx.double()[:, F:]
    E_gm = torch.cat([torch.zeros_like(r["gm"][:, :F]), (D + 1) * U32 * (gX * Xp).abs().sum(1)], 1)
    B1 = beta(2 * F, tile_d(r["gm"]), arith) * r["P"].abs().amax(1)
    E_P = B1[:, None] + E_gm @ W1a
    E_v = E_P * dsilu(pre.double()).abs() + 8 * U32 * r["v"].abs()
    B2 = beta(F, tile_d(r["v"]), arith) * r["gctx"].abs().amax(1)
    E_gctx = B2[:, None] + E_v @ W0a
    E_gh1 = E_gctx[:, :F] + U32 * r["gh1"].abs()
    tail = (r["gctx"][:, F:] / n)[:, None, :] * Xp
    E_gXp = (E_gctx[:, F:] / n)[:, None, :] * Xp.abs() + 3 * U32 * ((gX * mm.double()[:, None, F:]).abs() + tail.abs())
    return E_gXp, E_gh1


def emulate_f16x2(op):
    """CPU model of the tile arithmetic: the tile scaled by one power of two (|x| < 2^15), hi = fp16(x), lo = fp16(x - hi);
    returns hi + lo in fp64, rescaled.  What an operand keeps of itself under ONE exponent per 8-atom tile."""
    N = op.shape[0]
    out = torch.zeros_like(op, dtype=torch.float64)
    for b in range(0, N, EQ_ATOMS):
        t = op[b:b + EQ_ATOMS].double()
        m = float(t.abs().max())
        e = max(math.frexp(m)[1] - 15, -120) if m > 0 else -120            # |x| < 2^(e + 15)
        s = t * 2.0 ** -e
        hi = s.half().double()
        lo = (s - hi).half().double()
        out[b:b + EQ_ATOMS] = (hi + lo) * 2.0 ** e
    return out
