"""Yardstick of the attention-weight kernels (gn_attn_softmax / gn_attn_softmax_dropout, csrc/gn_gata.hip): hand-built CSR
graphs at the kernels' own edges, an fp64 restatement of the header's formula, and an a-priori, per-element error bound.

The operation (include/gotennet_hip.h, "K6 GATA message / softmax / aggregate"), for target i with incoming edges e (source j):

    s[e,h] = sum_{c in head h} q[i,c] k[j,c] act(t_attn[e,c])          head h = channels [h F/H, (h+1) F/H)
    a[e,h] = exp(s[e,h] - max_e s) / (sum_e exp(s - max) + 1e-16) * nrm[e],   nrm = 1/sqrt(F)  or  sqrt(outdeg[j])/sqrt(F)

The bound (u = 2^-24, the unit round-off of fp32; every constant below is counted off the kernel's arithmetic, none is
fitted to a measured error)
--------------------------------------------------------------------------------------------------------------------
Score.  A lane forms four terms (q k) act(t) -- two multiplies, (1 + u)^2 -- of an activation with relative error
eps_act, and adds them serially (at most four roundings on any term, counting the accumulate of the term itself); the
lph = (F/4)/H lanes of a head are then summed by log2(lph) exchange steps, one rounding each.  To first order

    |s^ - s| <= delta_s = u * ( (2 + 4 + log2(lph) + c_act) * sum_c |q k act(t)|  +  c_arg * sum_c |q k act(t)| |t| )

  SiLU(x) = x * rcp(1 + exp2(fl(-log2e x))): the argument carries the rounding of the constant (0.22 u) and of the product
  (u), i.e. a relative error of at most 2 u |x| on the exponential (the c_arg term; damped by exp/(1+exp) <= 1, which is
  dropped); v_exp_f32 and v_rcp_f32 are 1 ulp = 2 u each, the add and the final product u each: c_act = 6, c_arg = 2.
  tanh (library tanhf, 2 ulp): c_act = 4, c_arg = 0.  Identity: 0, 0.
Soft-max.  Numerator and denominator carry the SAME computed maximum, so it cancels; with the computed scores the weight
  is exp(s^_e) / sum_j exp(s^_j): relative error <= expm1(2 max_segment delta_s).
  The argument of the exponential, fl(log2e * fl(s^ - max)), carries three roundings (subtraction u, constant 0.22 u,
  product u): relative 2.25 u |s - max| on the numerator, and the soft-max-weighted mean of the same on the denominator.
  The sum: a lane adds its share serially -- ceil(deg H / 64) terms in the wave form (strip index = lane + 64 n), ceil(deg
  / 64) in the workgroup form -- and the lanes are combined in at most 6 exchange steps; all terms are positive, so the
  relative error is at most (ceil(deg H / 64) + 6) u in either form.
  The rest, c_misc: exp of the numerator 2 u, exp in the denominator 2 u, + 1e-16 u, v_rcp_f32 2 u, sqrt 2 u, the rounded
  constant 1/sqrt(F) u, three products 3 u: 13 u; taken as 16 u to cover the second-order terms.
  Underflow: a result below the smallest normal may be flushed, 2^-126 on the exponential (times 1/sum <= 1, times nrm) and
  on the final product: an absolute floor of 2^-126 (nrm + 1).

    |a^ - a| <= a * ( expm1(2 max_seg delta_s) + u (2.25 (|s - max| + mean_seg |s - max|) + ceil(deg H / 64) + 6 + 16) )
                + 2^-126 (nrm + 1)
"""
import functools
import math

import torch

ACT_SILU, ACT_TANH, ACT_NONE = 0, 3, 11           # GN_ACT_* of include/gotennet_hip.h
ACT_FN = {ACT_SILU: torch.nn.functional.silu, ACT_TANH: torch.tanh, ACT_NONE: lambda x: x}
C_ACT = {ACT_SILU: (6.0, 2.0), ACT_TANH: (4.0, 0.0), ACT_NONE: (0.0, 0.0)}      # (c_act, c_arg) of the docstring
U32 = 2.0 ** -24
W_STRIP, WG_CAP = 512, 2048                       # ATTN_W_STRIP, ATTN_CAP of csrc/gn_gata.hip
N_TARGETS = 42                                    # around 40, no multiple of the four targets of a wave-form workgroup
Q_SCALE = {"ordinary": 1.0, "saturating": 8.0, "degenerate": 0.0}
#: (F, activation): every instantiation the two entry points launch
FORMS = [(256, ACT_SILU), (64, ACT_SILU), (16, ACT_SILU), (64, ACT_TANH), (64, ACT_NONE),
         (512, ACT_SILU), (512, ACT_TANH), (1024, ACT_SILU), (1024, ACT_TANH)]
LAYOUTS = [("engine", True), ("compact", False), ("engine", False), ("compact", True)]      # (layout, with outdeg)


def heads(F: int):
    """Every H the entry points accept at width F: a power of two dividing F/4 with at most 64 lanes per head."""
    return [H for H in (1, 2, 4, 8, 16, 32, 64, 128, 256) if (F // 4) % H == 0 and (F // 4) // H <= 64]


def kernel_form(F: int, act: int, dropout: bool = False) -> str:
    """The kernel the launcher picks (gn_attn_softmax / _dropout: `F <= 256`, `act == SiLU`, `F == 256`)."""
    if F <= 256:
        name = "wave_f256" if (F == 256 and act == ACT_SILU and not dropout) else ("wave_silu" if act == ACT_SILU else "wave_generic")
    else:
        name = "workgroup_silu" if act == ACT_SILU else "workgroup_generic"
    return ("drop_" if dropout else "") + name


def strip_form(F: int, H: int, deg: int) -> str:
    """Where a target's scores live: the kernel's `deg * H <= ATTN_W_STRIP` / `<= ATTN_CAP` choice."""
    if F <= 256 and deg == 0:
        return "none"                              # the wave returns before either body
    return "lds" if deg * H <= (W_STRIP if F <= 256 else WG_CAP) else "global"


def degrees(F: int, H: int, seed: int = 0):
    """Per-target in-degrees: 0, 1, 2, 63, 64, 65 and both sides of every strip threshold; a degree-0 target on either
    side of the longest one inside the first group of four consecutive targets; 65 on the last (partial) group."""
    edge = [512 // H, 512 // H + 1] + ([2048 // H, 2048 // H + 1] if F > 256 else [])
    longest = max(edge + [65])
    special = [1, 2, 63, 64] + edge + [65]
    special.remove(longest)
    second = max(special)
    special.remove(second)
    g = torch.Generator().manual_seed(1000 + seed)
    last = 65 if 65 in special else special[-1]
    special.remove(last)
    fill = torch.randint(3, 13, (N_TARGETS - 5 - len(special),), generator=g).tolist()
    rest = special + fill
    rest = [rest[i] for i in torch.randperm(len(rest), generator=g).tolist()]
    degs = [0, longest, 0, second] + rest + [last]
    assert len(degs) == N_TARGETS and N_TARGETS % 4
    return degs


def cases(F: int, act: int):
    """The input sets of one (F, activation): every accepted H x the three score regimes, the (layout, outdeg) pairs in
    rotation so that every pair meets every regime and every strip form."""
    out = []
    for hi, H in enumerate(heads(F)):
        for ri, regime in enumerate(Q_SCALE):
            layout, with_outdeg = LAYOUTS[(hi + ri) % 4]
            out.append(dict(F=F, act=act, H=H, regime=regime, layout=layout, outdeg=with_outdeg, seed=hi))
    return out


def case_id(c) -> str:
    return f"F{c['F']}-act{c['act']}-H{c['H']}-{c['regime']}-{c['layout']}-{'outdeg' if c['outdeg'] else 'plain'}"


def build(c, degs=None):
    """CPU tensors of one case.  q | k share rows of 4F floats (k at column F) and t_attn sits in rows of 3F floats in the
    "engine" layout (engine._gata_forward); the compact layout has q, k [N, F] and t_attn [E, F] of their own."""
    F, H = c["F"], c["H"]
    degs = degrees(F, H, c["seed"]) if degs is None else list(degs)
    N = len(degs)
    g = torch.Generator().manual_seed(77 + 13 * c["seed"] + F)
    rowptr = torch.zeros(N + 1, dtype=torch.int32)
    rowptr[1:] = torch.tensor(degs, dtype=torch.int64).cumsum(0).to(torch.int32)
    E = int(rowptr[-1])
    src = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)
    rn = lambda *s: torch.randn(*s, generator=g)
    if c["layout"] == "engine":
        qk, te = rn(N, 4 * F), rn(E, 3 * F)
        q, k, t, ldqk, ldt = qk[:, :F], qk[:, F:2 * F], te[:, :F], 4 * F, 3 * F
        q.mul_(Q_SCALE[c["regime"]])
        bufs = dict(qk=qk, te=te)
    else:
        q, k, t, ldqk, ldt = rn(N, F) * Q_SCALE[c["regime"]], rn(N, F), rn(E, F), F, F
        bufs = dict(q=q, k=k, te=t)
    outdeg = torch.bincount(src.long(), minlength=N).to(torch.int32) if c["outdeg"] else None
    return dict(case=c, F=F, H=H, act=c["act"], N=N, E=E, degs=degs, rowptr=rowptr, src=src, outdeg=outdeg,
                q=q, k=k, t=t, ldqk=ldqk, ldt=ldt, bufs=bufs)


def _segments(d):
    return torch.repeat_interleave(torch.arange(d["N"]), torch.tensor(d["degs"]))


def _softmax(s, seg, N, nrm):
    mx = torch.full((N, s.shape[1]), -math.inf, dtype=s.dtype).scatter_reduce(0, seg[:, None].expand_as(s), s, "amax")
    ex = torch.exp(s - mx[seg])
    den = torch.zeros((N, s.shape[1]), dtype=s.dtype).index_add_(0, seg, ex) + 1e-16
    return ex / den[seg] * nrm[:, None], mx


def _norm(d, dtype):
    if d["outdeg"] is None:
        return torch.full((d["E"],), 1.0, dtype=dtype) / math.sqrt(d["F"])
    return torch.sqrt(d["outdeg"][d["src"].long()].to(dtype)) / math.sqrt(d["F"])


def reference(d, shift=None, remove=None):
    """fp64, from the fp32 inputs -> dict(a [E,H], s, sabs = sum |q k act(t)|, sabs_t = sum |q k act(t)| |t|, seg).
    ``shift`` = (e, h, x): raw score (e, h) moved by x; ``remove`` = e: edge e taken out of its segment (its own row of
    `a` is then zero) -- the two perturbations a meaningful bound must reject."""
    F, H, E = d["F"], d["H"], d["E"]
    seg = _segments(d)
    t64 = d["t"].double()
    prod = d["q"].double()[seg] * d["k"].double()[d["src"].long()] * ACT_FN[d["act"]](t64)
    s = prod.view(E, H, F // H).sum(2)
    sabs = prod.abs().view(E, H, F // H).sum(2)
    sabs_t = (prod.abs() * t64.abs()).view(E, H, F // H).sum(2)
    if shift is not None:
        s = s.clone()
        s[shift[0], shift[1]] += shift[2]
    nrm = _norm(d, torch.float64)
    if remove is None:
        a, mx = _softmax(s, seg, d["N"], nrm)
    else:
        keep = torch.ones(E, dtype=torch.bool)
        keep[remove] = False
        a = torch.zeros_like(s)
        a[keep], mx = _softmax(s[keep], seg[keep], d["N"], nrm[keep])
    return dict(a=a, s=s, sabs=sabs, sabs_t=sabs_t, seg=seg, mx=mx, nrm=nrm)


def bound(d, r):
    """The per-element absolute bound of the module docstring, [E, H] fp64."""
    F, H, N = d["F"], d["H"], d["N"]
    seg = r["seg"]
    c_act, c_arg = C_ACT[d["act"]]
    lph = (F // 4) // H
    delta = U32 * ((6.0 + math.log2(lph) + c_act) * r["sabs"] + c_arg * r["sabs_t"])
    dmax = torch.zeros((N, H), dtype=torch.float64).scatter_reduce(0, seg[:, None].expand_as(delta), delta, "amax")
    dist = (r["s"] - r["mx"][seg]).abs()
    w = r["a"] / r["nrm"][:, None]                                     # the plain soft-max weights
    mean_dist = torch.zeros((N, H), dtype=torch.float64).index_add_(0, seg, w * dist)
    deg = torch.tensor(d["degs"], dtype=torch.float64)
    serial = torch.ceil(deg * H / 64.0)[seg][:, None]
    rel = torch.expm1(2.0 * dmax[seg]) + U32 * (2.25 * (dist + mean_dist[seg]) + serial + 6.0 + 16.0)
    return r["a"] * rel + 2.0 ** -126 * (r["nrm"][:, None] + 1.0)


def restate_fp32(d):
    """The formula in plain fp32 torch (no kernel): what the CPU test holds to the bound."""
    F, H, E = d["F"], d["H"], d["E"]
    seg = _segments(d)
    prod = d["q"][seg] * d["k"][d["src"].long()] * ACT_FN[d["act"]](d["t"])
    s = prod.view(E, H, F // H).sum(2)
    return _softmax(s, seg, d["N"], _norm(d, torch.float32))[0]


def worst_ratio(a, r, bnd, rows=None):
    """max |a - ref| / bound over the rows given (all by default); a non-finite `a` counts as infinite."""
    err = (a.double() - r["a"]).abs() / bnd
    err = torch.where(torch.isfinite(a.double()), err, torch.full_like(err, math.inf))
    if rows is not None:
        err = err[rows]
    return float(err.max()) if err.numel() else 0.0


@functools.lru_cache(maxsize=4)
def built(F, act, H, regime, layout, with_outdeg, seed):
    """build + reference + bound of a case, shared (read-only) by the tests that use the same one."""
    d = build(dict(F=F, act=act, H=H, regime=regime, layout=layout, outdeg=with_outdeg, seed=seed))
    r = reference(d)
    return d, r, bound(d, r)


def built_case(c):
    return built(c["F"], c["act"], c["H"], c["regime"], c["layout"], c["outdeg"], c["seed"])
