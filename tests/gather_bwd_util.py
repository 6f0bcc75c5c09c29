"""Yardstick of the backward gather entry points, gn_message_backward / gn_message_backward_dropout and gn_htr_backward
(csrc/gn_backward.hip, gn_highl.hip, gn_options.hip): the hand-built graphs of tests/gather_util.py and their transposes,
the by-source (CSC) view built on the CPU, an fp64 restatement of the header's K10 contract, an a-priori per-element error
bound for every output tensor, the case table and the launchers' routing restated in Python.

The operations (include/gotennet_hip.h, K10), for edge e with target i and source j; o, dblk, tblk as in gather_util:

    g_o[e,0] = g_h1[i];  g_o[e,dblk(l)] += sum_{m in l} rl[e,m] g_X1[i,m];  g_o[e,tblk(l)] += sum_{m in l} X_in[j,m] g_X1[i,m]
    g_tf[e,b] = g_o x_j cut           g_cut[e] = sum_{b,c} g_o tf x_j         g_a[e,h] = sum_{(b,c) in head h} g_o v_j
    g_rl[e,m] = sum_c g_X1[i,m,c] o[e,dblk(l(m)),c]
    g_x[j,b] = sum_{e: src = j} g_o tf cut      g_v[j,b] = sum_{e: src = j} a g_o
    g_X_out[j,m] = g_X1[j,m] + sum_{e: src = j} g_X1[i,m] o[e,tblk(l(m))]
    g_s[e,h] = a g_a - (a_soft / nrm_e) sum_{e' -> i} a g_a,    nrm_e = sqrt(outdeg[j]) / sqrt(F)  or  1 / sqrt(F)
    g_q[i] = sum_e g_s[e,hq(c)] k_j act(pta)    g_k[j] = sum_{e: src = j} g_s q_i act(pta)    g_pta[e] = g_s q_i k_j act'(pta)
  mean: the upstream of every message of target i is g / deg(i); max: it goes to the arg-max edge, evenly among exact ties.
  TWO head maps: the message's a uses head (b F + c) / (M F / H) of the flattened value vector, the scores use c / (F / H).
  HTR, per block B (a degree; all D rows when joint), pa = EQ_i . r, pb = EK_j . r, c = 2 - r . r (0 with norej):
    gw = g_t_out act(pre_t) gate'(w_raw)   (g_t_out itself with GN_HTR_DIRECT)        g_pre_t = g_t_out w act'(pre_t)
    gEQ[i,m] = sum_e gw (EK_m - c r_m pb)    gEK[j,m] = sum_{e: src = j} gw (EQ_m - c r_m pa)
    g_rl[e,m] = sum_f gw ( -c (EQ_m pb + pa EK_m) + 2 r_m pa pb )     (the last term only with the rejection)

The bounds (u = 2^-24; the library is built with -ffp-contract=off, so every rounding is one the source spells; every
constant is counted off the kernels' arithmetic, none is fitted to a measured error).  Each is
    u * (sum over the terms of  constant * un-cancelled magnitude)  +  u |result|  +  2^-126.
--------------------------------------------------------------------------------------------------------------------
ns = slots(F); lps = F / 4 lanes per slot, w = min(lps, 64) lanes per butterfly; chain(d) = ceil(d / ns) + ns + 1: a slot adds
its share serially, the ns slot partials are added in slot order, one more for the second order (gather_util, K6).  By
target d is the in-degree, BY SOURCE the out-degree.
g_o.  Block 0 is a load.  A gate block is an fma chain over the n_b rows it serves (n_b = 2 l + 1 with its own gate, D with
  a shared one): c_go = n_b on Go = sum |rl g_X1| (sum |X_j g_X1|).  mean: 1.0f / deg (u), one product (u), taken as + 3;
  max: the routed rows are g / count, one division (taken as 3 u), + 3.  Block 0: 0 (+ 3).
g_tf = (g_o x) cut: two products:                     (c_go + 3) Go |x| cut
g_cut: g_o tf x two products, hsum4 two adds, the M blocks serially, log2(w) butterfly steps, one more:
                                                       (c_go + 5 + M + log2 w) on sum Go |tf x|
       (F > 256: F / 256 partial slices, the degree groups: G slices; the test adds the slices in fp64 and holds the sum --
        fewer roundings than counted)
g_a: g_o v one product, hsum4 two, M staged partials serially (the groups: their blocks, then the G slices in slice order),
     log2(lps) butterfly steps, one more:             c_ga = c_go + 4 + M + G + log2 lps   on  Ga = sum_{head} Go |v|
g_rl: o = fma(a, v, (tf x) cut) three roundings, the product, hsum4 two, log2(w), one more (mean / max: + 3 on g_X1):
                                                       (7 + log2 w [+ 3]) on sum_c |g_X1| (|tf x cut| + |a v|)
g_x: tf cut one product, the fma:  (c_go + 2 + chain(outdeg)) on sum Go |tf| cut;   g_v: the fma: (c_go + 1 + chain(outdeg))
g_X_out: o three roundings, the fma: (4 + chain(outdeg) [+ 3]) on sum |g_X1| (|tf x cut| + |a v|); the residual add is the u |result|
g_s: dot = sum a g_a: one product, a lane adds ceil(deg / 64) terms, six butterfly steps; nrm = sqrtf(outdeg) * inv_sqrt_f:
     sqrtf 2 u, the rounded constant u, the product u; the division 3 u; the product with dot and the subtraction 2 u:
       E_s = (c_ga + 2) |a| Ga + (|a_soft| / nrm) ( sum_e' c_ga |a| Ga + (ceil(deg / 64) + 6 + 1 + 9) sum_e' |a| Ga )
g_q, g_k: act(pta) relative (c_act + c_arg |pta|) u (attn_util.C_ACT), k act one product, the fma:
       sum_e E_s |k act| + (c_act + c_arg |pta| + 2 + chain) sum_e |g_s k act|        (g_k: q for k, chain(outdeg))
g_pta = ((q k) g_s) act'(pta): three products:  E_s |q k act'| + |g_s q k| E_act' + 3 |g_s q k act'|
  act' SiLU = s (1 + x (1 - s)), s = sigmoid_fast(x) relative e_s = (5 + 2 |x|) u (argument 2 |x|, v_exp_f32 2, the add 1,
  v_rcp_f32 2); 1 - s: u + e_s s; x (1 - s): u; 1 + .: u; the product u:
       E_act' = s [ (6 + 2 |x|) (|1 + x (1 - s)| + |x| s) + 3 |x| (1 - s) + 2 ]        (absolute: act' has a zero at x = -1.278)
  tanh: 1 - t t, tanhf 2 ulp: E_act' = 9 t^2 + 2.   sigmoid gate s (1 - s), s relative 8 u (gather_util.GATE_EPS):
       E_gate' = 9 s (1 - s) + s + 8 s^2.
HTR.  gw: act relative (c_act + c_arg |pre_t|), one product; with a gate gate' absolute E_gate' and one more product:
       E_gw = |g_t| ( |act gate'| (c_act + c_arg |pre_t| + 2) + |act| E_gate' );   DIRECT: 0.
  n = rows of the block (+ lmax when joint: the general kernel adds the per-degree partial dots); pa, pb, r . r are n-term fma
  chains, c = 2 - r . r one more rounding: |c^ - c| <= (n + 1) u (2 + rr), |c| <= 2 + rr; A_q = sum |r EQ|, A_k = sum |r EK|.
  gEQ:  T = |EK_m| + (2 + rr) |r_m| A_k:   E_gw T + |gw| (2 n + 6 + chain(deg)) T         (gEK: EQ, A_q, chain(outdeg))
  g_rl: T = (2 + rr) (|EQ_m| A_k + A_q |EK_m|) + 2 |r_m| A_q A_k:   sum_f E_gw T + |gw| (3 n + 12 + log2 w) T
  g_pre_t = (g_t w) act'(pre_t):   |g_t w| E_act' + 2 |g_t w act'|
  Underflow: gw (and g_t w) is a product of up to three factors; behind a saturated gate it falls below the smallest normal
  and may be flushed: 2^-126 on gw times the magnitude T it multiplies, summed like the terms (added to the 2^-126 floor).
Which bound a form is held to: every message-backward form (pair, merged, degree groups, degree-sliced) and every HTR form
(the tuned by-target / by-source kernels, which factor gw out of the per-row terms, the general and the degree-sliced kernels)
is held to the ONE bound above; the counts take the longer of the orders where they differ (M staged partials against the
groups' NB + G, the merged kernels' fma(g_o, tf cut) against the sliced kernels' same expression).
"""
import functools
import math

import torch

from tests import attn_util as A
from tests import gather_util as U
from tests.gather_util import FLOOR, MAX, MEAN, SLICED, U32, Shape, slots

HTR_DIRECT = 16
GS_CAP = 2048                                      # gn_backward.hip: deg * H <= GS_CAP keeps the head gradients in LDS
BASE_KINDS = ("ragged", "ragged9", "hub", "single", "empty")
KINDS = BASE_KINDS + ("ragged_T", "hub_T")
PAD_COLS = U.PAD_COLS


# ------------------------------------------------------------------------------------------------ graphs
def transpose(gr):
    """The same edge set with source and target swapped, re-sorted (stably) into CSR -> (graph, emap: old edge id of every
    new edge).  The in-degrees of `gr` become the out-degrees."""
    N = gr["N"]
    new_tgt, new_src = gr["src"].long(), gr["seg"]
    emap = torch.sort(new_tgt, stable=True)[1]
    degs = torch.bincount(new_tgt, minlength=N).tolist()
    rowptr = torch.zeros(N + 1, dtype=torch.int32)
    rowptr[1:] = torch.tensor(degs, dtype=torch.int64).cumsum(0).to(torch.int32)
    out = dict(gr, kind=gr["kind"] + "_T", degs=degs, rowptr=rowptr, src=new_src[emap].to(torch.int32).contiguous(),
               seg=new_tgt[emap].contiguous())
    return out, emap


def csc_view(d):
    """colptr, perm, tgt_by_src of a CSR graph: a stable sort of the edges by source (NOT gn_build_csc)."""
    src = d["src"].long()
    perm = torch.sort(src, stable=True)[1]
    outdeg = torch.bincount(src, minlength=d["N"])
    colptr = torch.zeros(d["N"] + 1, dtype=torch.int32)
    colptr[1:] = outdeg.cumsum(0).to(torch.int32)
    return dict(colptr=colptr, perm=perm.to(torch.int32).contiguous(), tgt_by_src=d["seg"][perm].to(torch.int32).contiguous(),
                outdeg=outdeg.to(torch.int32))


def check_csc(d):
    """The invariants every by-source kernel indexes with; asserted before any launch."""
    N, E = d["N"], d["E"]
    rp, cp, perm, src = d["rowptr"].long(), d["colptr"].long(), d["perm"].long(), d["src"].long()
    assert rp.numel() == N + 1 and int(rp[0]) == 0 and int(rp[-1]) == E and bool((rp[1:] >= rp[:-1]).all())
    assert cp.numel() == N + 1 and int(cp[0]) == 0 and int(cp[-1]) == E and bool((cp[1:] >= cp[:-1]).all())
    assert perm.numel() == E and torch.equal(torch.sort(perm)[0], torch.arange(E))
    assert E == 0 or (0 <= int(src.min()) and int(src.max()) < N)
    col = torch.repeat_interleave(torch.arange(N), cp[1:] - cp[:-1])
    assert torch.equal(src[perm], col)                                   # src[perm[pp]] == j for pp in column j
    dst = d["seg"]                                                       # the target of CSR edge e
    assert torch.equal(torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1]), dst)
    assert torch.equal(d["tgt_by_src"].long(), dst[perm])
    assert torch.equal(d["outdeg"].long(), cp[1:] - cp[:-1])


def promised_out_degrees(kind, ns):
    """Out-degrees a transposed kind places deliberately (the in-degrees of its base kind)."""
    if kind == "ragged_T":
        return {0, 1, ns, ns + 1, 2 * ns + 1, 63, 64, 65}
    if kind == "hub_T":
        return {3, 301}
    return set()


def _regraph(d, kind):
    """`d` (built on the base kind) moved to the transposed graph: edge tensors follow the edge map."""
    gr, emap = transpose(d)
    out = dict(d)
    out.update({k: gr[k] for k in ("kind", "degs", "rowptr", "src", "seg")})
    for key in U.EDGE_KEYS:
        if d.get(key) is not None:
            out[key] = d[key][emap].contiguous()
    assert out["kind"] == kind
    return out


def _plant_ties(d, keys=("tbuf", "a", "cut", "rl")):
    """aggr = max: the first two edges of every target with two or more carry the same message (as build_k6 does)."""
    for i, deg in enumerate(d["degs"]):
        e0 = int(d["rowptr"][i])
        if deg >= 2:
            d["src"][e0 + 1] = d["src"][e0]
            for key in keys:
                d[key][e0 + 1] = d[key][e0]


# ------------------------------------------------------------------------------------------------ routing
def bwd_head_ok(F, H):
    return H > 0 and (H & (H - 1)) == 0 and (F // 4) % H == 0 and (F // 4) // H <= 64


def msg_groups(lmax, sd, st, flags=0, act=A.ACT_SILU):
    """gn_message_backward_groups."""
    if U.use_highl(lmax, flags) or act != A.ACT_SILU:
        return 1
    return lmax - 1 if (lmax >= 3 and sd and st) else 1


def kernel_form(entry, F, lmax, sep_dir=True, sep_tensor=True, first=False, ga=True, H=8, flags=0, act=A.ACT_SILU, mode=0):
    """The kernels the launcher picks: message_backward / message_backward_launch / gn_launch_msg_bwd, gn_htr_backward /
    htr_backward_launch, gn_use_highl and gn_message_backward_groups.  entry = "msg_bwd" | "htr_bwd"."""
    tf = lambda b: "T" if b else "F"
    highl = U.use_highl(lmax, flags)
    if entry == "msg_bwd":
        if highl or F > 256 or act != A.ACT_SILU:
            assert not first                       # refused: GN_ERR_BAD_ARG
            return f"hl_msg_bwd({U.aggr_of(flags)})"
        if not first and msg_groups(lmax, sep_dir, sep_tensor) > 1:
            assert ga                              # refused without the workspace
            if H > 8:                              # the group kernels carry eight head sums
                return "hl_msg_bwd(add)"
            return f"groups<{lmax},{256 if F == 256 else 0}>+attn+gk"
        if lmax == 1:
            sep_dir = sep_tensor = False
        fc = 256 if F == 256 and ((sep_dir and sep_tensor) or lmax == 1) else 0
        head = f"{lmax},{tf(sep_dir)},{tf(sep_tensor)}"
        if ga:
            return f"merged{'_first' if first else ''}<{head},{fc}>+attn+gk"
        return f"pair_first<{head},{fc}>" if first else f"pair<{head},0>"      # the general pair: run-time width at every F
    assert entry == "htr_bwd"
    if highl or F > 256 or (not mode and act != A.ACT_SILU):
        return "hl_htr_bwd"
    if mode:
        return f"htr_general<{lmax}>"
    fc = 256 if F == 256 else 0
    return {1: "htr_tgt+src<1,%d>", 2: "htr_tgt+src<2,%d>", 3: "htr_tgt+srcgroup<3,%d>", 4: "htr_tgt×2+srcgroup<4,%d>"}[lmax] % fc


# ------------------------------------------------------------------------------------------------ message backward: cases
def mb_case(F, lmax, sd=True, st=True, H=8, first=False, ga=True, flags=0, act=A.ACT_SILU, drop=False, outdeg=False):
    assert bwd_head_ok(F, H) and U.head_ok(Shape(lmax, sd, st).M, F, H)
    return dict(F=F, lmax=lmax, sd=bool(sd), st=bool(st), H=H, first=first, ga=ga, flags=flags, act=act, drop=drop, outdeg=outdeg)


def mb_id(c):
    fl = "".join(n for b, n in ((SLICED, "-sliced"), (MEAN, "-mean"), (MAX, "-max")) if c["flags"] & b)
    return (f"F{c['F']}-l{c['lmax']}-{'T' if c['sd'] else 'F'}{'T' if c['st'] else 'F'}-H{c['H']}{'-first' if c['first'] else ''}"
            f"{'' if c['ga'] else '-noga'}{fl}{'' if c['act'] == A.ACT_SILU else '-act%d' % c['act']}{'-drop' if c['drop'] else ''}"
            f"{'-outdeg' if c['outdeg'] else ''}")


def mb_form(c):
    return kernel_form("msg_bwd", c["F"], c["lmax"], c["sd"], c["st"], c["first"], c["ga"], c["H"], c["flags"], c["act"])


def mb_allows_both(c):
    """Whether the entry point takes this case with ga_parts given AND withheld (the tuned, ungrouped forms)."""
    return mb_form(c).startswith(("merged", "pair"))


def _mb_cases():
    out, T, Fa = [], True, False
    add = lambda *a, **k: out.append(mb_case(*a, **k))
    for first in (Fa, T):                                                   # lmax 1
        for ga in (T, Fa):
            add(64, 1, T, T, 8, first, ga, outdeg=first)
    n = 0
    for lmax in (2, 3, 4):                                                  # every (sep_dir, sep_tensor) pair, both X_in forms
        for sd in (T, Fa):
            for st in (T, Fa):
                for first in (Fa, T):
                    for ga in (T, Fa):
                        if not ga and not first and lmax >= 3 and sd and st:
                            continue                                        # the degree groups need the workspace
                        add(64, lmax, sd, st, 8, first, ga, outdeg=bool(n % 3 == 0))
                    n += 1
    for lmax in (1, 2, 3, 4):                                               # the compile-time-width forms
        for first in (Fa, T):
            add(256, lmax, T, T, 8, first, T)
    for lmax in (1, 2, 3, 4):
        add(256, lmax, T, T, 8, T, Fa)
    add(256, 3, T, Fa, 8, Fa, T); add(256, 2, T, T, 8, Fa, Fa)
    add(16, 2, T, T, 4, Fa, T); add(16, 3, T, T, 4, Fa, T); add(16, 4, Fa, T, 2, T, Fa); add(16, 1, T, T, 1, Fa, Fa)      # ns = 64
    add(64, 2, T, T, 1, Fa, T); add(64, 2, T, T, 16, Fa, T); add(64, 2, T, Fa, 16, Fa, Fa, outdeg=T)                      # head counts
    add(64, 3, T, T, 1, Fa, T); add(64, 3, T, T, 16, Fa, T); add(64, 4, T, T, 16, Fa, T); add(64, 4, T, T, 16, T, T)
    add(128, 2, T, T, 32, Fa, T); add(128, 2, T, T, 32, Fa, Fa); add(128, 3, T, T, 32, Fa, T)     # deg 64 / 65 astride deg * H = 2048
    add(64, 2, T, T, 8, flags=SLICED); add(64, 4, T, T, 8, flags=SLICED, outdeg=T); add(64, 4, Fa, T, 16, flags=SLICED)
    add(32, 5, T, T, 8); add(32, 8, T, T, 8, outdeg=T); add(32, 8, T, Fa, 1)
    add(512, 2, T, T, 8); add(1024, 2, T, T, 8, outdeg=T)
    add(64, 2, T, T, 8, act=A.ACT_TANH); add(64, 3, T, T, 8, act=A.ACT_TANH)
    add(64, 2, T, T, 8, flags=MEAN); add(32, 5, T, T, 8, flags=MEAN, outdeg=T)
    add(64, 3, T, T, 8, flags=MAX); add(32, 5, Fa, T, 4, flags=MAX)
    add(64, 2, T, T, 8, drop=T); add(64, 3, T, T, 8, drop=T, outdeg=T); add(64, 2, T, Fa, 8, Fa, Fa, drop=T, outdeg=T)    # dropout
    add(64, 2, T, T, 8, flags=SLICED, drop=T, outdeg=T); add(64, 3, T, T, 8, T, T, drop=T)
    return out


MB_CASES = _mb_cases()
BIG = lambda c: c["F"] >= 512 or c["lmax"] >= 8      # kept on `ragged` and `hub_T` only


def mb_kinds(c, first_of_group=False):
    kinds = ("ragged", "hub_T") if BIG(c) else ("ragged", "hub", "ragged_T", "hub_T")
    return kinds + (("ragged9", "single") if first_of_group and not BIG(c) else ())


def build_mb(c, kind, seed=0):
    """CPU tensors of one message-backward case on one graph: the forward tensors of gather_util.build_k6 (same seeds), eproj =
    (t_attn pre-activation | t_filter), qk rows of 2 F + 8 floats (q | k | NaN), the upstream gradients, a_soft and the CSC view."""
    base = kind[:-2] if kind.endswith("_T") else kind
    kc = dict(F=c["F"], lmax=c["lmax"], sd=c["sd"], st=c["st"], H=c["H"], first=c["first"], flags=c["flags"] & ~MAX)
    d = U.build_k6(kc, base, seed)
    d["case"], d["lmax_arg"], d["aggr"] = c, c["lmax"] | c["flags"], U.aggr_of(c["flags"])
    if base != kind:
        d = _regraph(d, kind)
    if c["flags"] & MAX and d["E"]:
        _plant_ties(d)
    F, H, S, N, E = d["F"], d["H"], d["S"], d["N"], d["E"]
    g = torch.Generator().manual_seed(20011 + 31 * seed + F + 7 * c["lmax"] + H + 3 * len(kind))
    rn = lambda *s: torch.randn(*s, generator=g)
    d["eproj"] = d["tbuf"].clone()
    d["eproj"][:, :F] = rn(E, F)
    if c["flags"] & MAX and E:                      # (the tied pairs share their score as well)
        _plant_ties(d, ("eproj",))
    d["lde"], d["ldqk"], d["ldn"] = d["ldt"], 2 * F + PAD_COLS, 2 * F + PAD_COLS
    d["qk"] = torch.full((N, d["ldqk"]), math.nan)
    d["qk"][:, :2 * F] = rn(N, 2 * F)
    d["g_h1"], d["g_X1"] = rn(N, F), rn(N, S.D, F)
    d.update(csc_view(d))
    d["use_outdeg"] = c["outdeg"]
    d["a_soft"] = None
    if c["drop"]:                                   # a = a dropped copy of a_soft: a third of the entries zero, the rest scaled
        d["a_soft"] = d["a"]
        keep = torch.rand(E, H, generator=g) >= 1.0 / 3.0
        d["a"] = torch.where(keep, d["a_soft"] * 1.5, torch.zeros(()))
    d["G"] = 1 if c["first"] else msg_groups(c["lmax"], c["sd"], c["st"], c["flags"], c["act"])
    d["form"] = mb_form(c)
    return d


def _clean_blocks(d):
    """x, v, tf [., M, F] in fp64; the zero-X_in form's unread (NaN) tensor-gate blocks as zeros."""
    x, v, tf = (t.double() for t in U._blocks(d))
    if d["X_in"] is None:
        lo = 1 + d["S"].ND
        x, v, tf = x.clone(), v.clone(), tf.clone()
        x[:, lo:], v[:, lo:], tf[:, lo:] = 0.0, 0.0, 0.0
    return x, v, tf


def _act64(t, act):
    """act, act', |error of act| / (u |act|), |error of act'| / u  (module docstring)."""
    if act == A.ACT_SILU:
        s = torch.sigmoid(t)
        f, df = t * s, s * (1.0 + t * (1.0 - s))
        e_df = s * ((6.0 + 2.0 * t.abs()) * ((1.0 + t * (1.0 - s)).abs() + t.abs() * s) + 3.0 * t.abs() * (1.0 - s) + 2.0)
        return f, df, 6.0 + 2.0 * t.abs(), e_df
    if act == A.ACT_TANH:
        th = torch.tanh(t)
        return th, 1.0 - th * th, torch.full_like(t, 4.0), 9.0 * th * th + 2.0
    raise KeyError(act)


def _fwd_messages(d, x, v, tf, a, hidx, fp32=False):
    """The per-edge messages [E, 1 + D, F] (for the arg-max routing): in fp64, or in the kernels' own fp32 arithmetic
    (hl_max_route_kernel: fma(a, v, (tf x) cut), fma(X_j, o_t, o_d rl))."""
    S, E, F = d["S"], d["E"], d["F"]
    src = d["src"].long()
    bd, bt = torch.tensor([S.dblk(l) for l in S.l_of]), torch.tensor([S.tblk(l) for l in S.l_of])
    ah = a[:, hidx.reshape(-1)].view(E, S.M, F)
    if fp32:
        o = U.fma32(ah.float(), v.float()[src], (tf.float() * x.float()[src]) * d["cut"].view(-1, 1, 1))
        mX = U.fma32(d["X_in"][src], o[:, bt], o[:, bd] * d["rl"][:, :, None])
    else:
        o = tf * x[src] * d["cut"].double().view(-1, 1, 1) + ah * v[src]
        mX = d["rl"].double()[:, :, None] * o[:, bd] + d["X_in"].double()[src] * o[:, bt]
    return torch.cat([o[:, :1], mX], 1)


def max_route(msg, seg, N, ties_first=False):
    """[E, 1 + D, F] weights: 1 / (number of arg-max edges) on the arg-max edges of every output element, 0 elsewhere."""
    mx = torch.full((N,) + tuple(msg.shape[1:]), -math.inf, dtype=msg.dtype).scatter_reduce(
        0, seg.view(-1, 1, 1).expand_as(msg), msg, "amax", include_self=True)
    hit = (msg == mx[seg]).double()
    if ties_first:                                  # mutation: the whole gradient to the first arg-max edge
        first = torch.zeros_like(hit)
        seen = torch.zeros((N,) + tuple(msg.shape[1:]), dtype=torch.bool)
        for e in range(msg.shape[0]):
            i = int(seg[e])
            take = (hit[e] > 0) & ~seen[i]
            first[e] = take.double()
            seen[i] |= take
        return first
    cnt = torch.zeros((N,) + tuple(msg.shape[1:]), dtype=torch.float64).index_add_(0, seg, hit)
    return hit / cnt[seg].clamp_min(1.0)


def _seg_sum(t, idx, N):
    return torch.zeros((N,) + tuple(t.shape[1:]), dtype=t.dtype).index_add_(0, idx, t)


MB_OUTPUTS = ("g_tf", "g_pta", "g_cut", "g_rl", "g_s", "g_q", "g_k", "g_x", "g_v", "g_X_out")


def ref_mb(d, mut=None, route32=True):
    """fp64 restatement of the message backward from the fp32 inputs -> dict(output -> fp64 tensor, "b:" + output -> its bound).
    `route32`: under aggr = max the arg-max is a discrete decision the kernel takes on ITS fp32 messages; the restatement
    takes the same decision from the same arithmetic (fma32), everything else is fp64.  `mut` names one of the mutations a
    meaningful bound must reject."""
    S, F, H, N, E, ns = d["S"], d["F"], d["H"], d["N"], d["E"], d["ns"]
    M, D, act, aggr, G = S.M, S.D, d["case"]["act"], d["aggr"], d["G"]
    src, seg = d["src"].long(), d["seg"]
    x, v, tf = _clean_blocks(d)
    first = d["X_in"] is None
    Xin = torch.zeros(N, D, F, dtype=torch.float64) if first else d["X_in"].double()
    a = d["a"].double()
    a_soft = a if (d["a_soft"] is None or mut == "soft_is_a") else d["a_soft"].double()
    cut, rl = d["cut"].double(), d["rl"].double()
    gh, gX = d["g_h1"].double(), d["g_X1"].double()
    q, k, pta = d["qk"][:, :F].double(), d["qk"][:, F:2 * F].double(), d["eproj"][:, :F].double()
    hidx = U.head_index(S, F, H)                                          # the message's head map [M, F]
    hq = torch.arange(F) // (F // H)                                      # the scores' head map [F]
    if mut == "msg_map_for_scores":
        hq = hidx[0]
    if mut == "score_map_for_msg":
        hidx = hq.view(1, F).expand(M, F)
    dblk = {l: S.dblk(l) for l in range(1, S.lmax + 1)}
    tblk = {l: S.tblk(l) for l in range(1, S.lmax + 1)}
    if mut == "swap_blocks":
        dblk[S.lmax], tblk[S.lmax] = tblk[S.lmax], dblk[S.lmax]
    bd, bt = torch.tensor([dblk[l] for l in S.l_of]), torch.tensor([tblk[l] for l in S.l_of])
    if mut == "shift_rl":                           # the rows of the last degree rotated by one
        col = list(range(D))
        lo = S.lmax * S.lmax - 1
        col[lo:] = col[lo + 1:] + [lo]
        rl = rl[:, col]
    indeg = torch.tensor(d["degs"], dtype=torch.float64)
    outdeg = d["outdeg"].double()
    # upstream gradient of every per-edge message [E, 1 + D, F] and its rounding allowance (in u, relative)
    gm = torch.cat([gh[:, None], gX], 1)[seg]
    c_up = 0.0
    if aggr == "mean":
        gm, c_up = gm / indeg.clamp_min(1.0)[seg].view(-1, 1, 1), 3.0
    elif aggr == "max":
        msg = _fwd_messages(d, x, v, tf, a, U.head_index(S, F, H), fp32=route32)
        gm, c_up = gm * max_route(msg.double(), seg, N, ties_first=(mut == "ties_first")), 3.0
    gm0, gmX = gm[:, 0], gm[:, 1:]
    xj, vj, Xj = x[src], v[src], Xin[src]
    ah = a[:, hidx.reshape(-1)].view(E, M, F)
    sp, av = tf * xj * cut.view(-1, 1, 1), ah * vj
    o, oa = sp + av, sp.abs() + av.abs()
    # g_o and its magnitude; c_go per block
    go = torch.zeros(E, M, F, dtype=torch.float64)
    Go = torch.zeros(E, M, F, dtype=torch.float64)
    go[:, 0], Go[:, 0] = gm0, gm0.abs()
    go.index_add_(1, bd, rl[:, :, None] * gmX)
    Go.index_add_(1, bd, (rl[:, :, None] * gmX).abs())
    go.index_add_(1, bt, Xj * gmX)
    Go.index_add_(1, bt, (Xj * gmX).abs())
    n_b = torch.zeros(M)
    n_b.index_add_(0, bd, torch.ones(D))
    n_b2 = torch.zeros(M)
    n_b2.index_add_(0, bt, torch.ones(D))
    c_go = (torch.maximum(n_b, n_b2).double() + c_up).view(1, M, 1)
    lps = F // 4
    lw, llps = math.log2(min(lps, 64)), math.log2(lps)
    chain_in = (torch.ceil(indeg / ns) + ns + 1.0)
    chain_out = (torch.ceil(outdeg / ns) + ns + 1.0)
    R, Bd = {}, {}
    fin = lambda name, val, e_u: (R.__setitem__(name, val), Bd.__setitem__(name, U32 * (e_u + val.abs()) + FLOOR))
    # ---- per-edge outputs of the gates
    cut_tf = cut.clone()
    if mut == "drop_cut" and E:
        cut_tf[E // 2] = 1.0
    fin("g_tf", go * xj * cut_tf.view(-1, 1, 1), (c_go + 3.0) * Go * xj.abs() * cut.view(-1, 1, 1))
    fin("g_cut", (go * tf * xj).sum((1, 2)), ((c_go + 5.0 + M + lw) * Go * (tf * xj).abs()).sum((1, 2)))
    hflat = hidx.reshape(-1)
    g_a = torch.zeros(E, H, dtype=torch.float64).index_add_(1, hflat, (go * vj).reshape(E, M * F))
    c_ga = c_go + 4.0 + M + G + llps
    Ga = torch.zeros(E, H, dtype=torch.float64).index_add_(1, hflat, (Go * vj.abs()).reshape(E, M * F))
    E_ga = torch.zeros(E, H, dtype=torch.float64).index_add_(1, hflat, (c_ga * Go * vj.abs()).reshape(E, M * F))
    fin("g_rl", (gmX * o[:, bd]).sum(2), (7.0 + lw + c_up) * (gmX.abs() * oa[:, bd]).sum(2))
    # ---- by-source sums
    keep = torch.ones(E, dtype=torch.bool)
    if mut == "hub_loses_edge":
        jmax = int(outdeg.argmax())
        keep[int(d["perm"][int(d["colptr"][jmax + 1]) - 1])] = False
    co = chain_out.view(-1, 1, 1)
    fin("g_x", _seg_sum((go * tf * cut.view(-1, 1, 1))[keep], src[keep], N),
        _seg_sum((c_go + 2.0) * Go * tf.abs() * cut.view(-1, 1, 1), src, N) + co * _seg_sum(Go * tf.abs() * cut.view(-1, 1, 1), src, N))
    fin("g_v", _seg_sum(ah * go, src, N), _seg_sum((c_go + 1.0) * ah.abs() * Go, src, N) + co * _seg_sum(ah.abs() * Go, src, N))
    if not first:
        part = gmX * o[:, bt]
        if mut == "self_loop_once":                 # the self-loop's source-side term left out (counted once, as the residual)
            part = part * (src != seg).double().view(-1, 1, 1)
        TX = _seg_sum(gmX.abs() * oa[:, bt], src, N)
        fin("g_X_out", gX + _seg_sum(part, src, N), (4.0 + c_up + co) * TX)
    # ---- softmax backward
    nrm_deg = outdeg[seg] if mut == "nrm_of_target" else outdeg[src]
    nrm = (torch.sqrt(nrm_deg) if d["use_outdeg"] else torch.ones(E, dtype=torch.float64)) / math.sqrt(F)
    dot = _seg_sum(a * g_a, seg, N)
    pref = a_soft / nrm[:, None]
    g_s = a * g_a - pref * dot[seg]
    serial = torch.ceil(indeg / 64.0)[seg].view(-1, 1)
    E_s = (E_ga + 2.0 * Ga) * a.abs() + pref.abs() * (_seg_sum(E_ga * a.abs(), seg, N)[seg]
                                                      + (serial + 16.0) * _seg_sum(a.abs() * Ga, seg, N)[seg])
    fin("g_s", g_s, E_s)
    E_s = E_s + g_s.abs()                           # the rounding of g_s itself, carried into what reads it
    # ---- scores backward
    f, df, e_f, e_df = _act64(pta, act)
    gsc, Esc = g_s[:, hq], E_s[:, hq]
    qi, kj = q[seg], k[src]
    tq = (gsc * kj * f).abs()
    fin("g_q", _seg_sum(gsc * kj * f, seg, N), _seg_sum(Esc * (kj * f).abs() + (e_f + 2.0) * tq, seg, N) + chain_in.view(-1, 1) * _seg_sum(tq, seg, N))
    tk = (gsc * qi * f).abs()
    fin("g_k", _seg_sum(gsc * qi * f, src, N), _seg_sum(Esc * (qi * f).abs() + (e_f + 2.0) * tk, src, N) + chain_out.view(-1, 1) * _seg_sum(tk, src, N))
    fin("g_pta", gsc * qi * kj * df, Esc * (qi * kj * df).abs() + (gsc * qi * kj).abs() * e_df + 3.0 * (gsc * qi * kj * df).abs())
    R.update({"b:" + kname: b for kname, b in Bd.items()})
    R["g_a"] = g_a
    return R


# ------------------------------------------------------------------------------------------------ HTR backward
def hb_case(F, lmax, mode=0, flags=0, act=A.ACT_SILU):
    return dict(F=F, lmax=lmax, mode=mode, flags=flags, act=act)


def hb_id(c):
    return (f"F{c['F']}-l{c['lmax']}-mode{c['mode']}{'-sliced' if c['flags'] & SLICED else ''}"
            f"{'' if c['act'] == A.ACT_SILU else '-act%d' % c['act']}")


def hb_form(c):
    return kernel_form("htr_bwd", c["F"], c["lmax"], flags=c["flags"], act=c["act"], mode=c["mode"])


def _hb_cases():
    J, NR, DIR = U.HTR_JOINT, U.HTR_NOREJ, HTR_DIRECT
    out = [hb_case(F, lmax) for F in (64, 256) for lmax in (1, 2, 3, 4)]
    out += [hb_case(16, 2), hb_case(16, 3), hb_case(16, 4)]
    out += [hb_case(64, 2, J), hb_case(64, 3, J), hb_case(64, 2, NR), hb_case(64, 4, NR | J)]
    out += [hb_case(64, 2, 1 << 2), hb_case(64, 2, 2 << 2), hb_case(64, 2, 3 << 2), hb_case(64, 3, J | (1 << 2)), hb_case(64, 1, NR | (3 << 2))]
    out += [hb_case(64, 2, DIR), hb_case(64, 3, DIR | J), hb_case(64, 2, DIR | (2 << 2)), hb_case(32, 5, DIR | NR)]
    out += [hb_case(64, 2, flags=SLICED), hb_case(64, 4, flags=SLICED), hb_case(64, 4, J | (2 << 2), SLICED), hb_case(32, 5), hb_case(32, 8),
            hb_case(32, 8, J), hb_case(512, 2), hb_case(512, 2, 3 << 2)]
    out += [hb_case(64, 2, act=A.ACT_TANH), hb_case(64, 3, 1 << 2, act=A.ACT_TANH)]
    return out


HB_CASES = _hb_cases()
HB_OUTPUTS = ("gEQ", "gEK", "g_rl", "g_pre_t")


def build_hb(c, kind, seed=0):
    """CPU tensors of one HTR-backward case: EQ, EK, rl of gather_util.build_k7, the upstream g_t_out, pre_t, and the SAVED w and
    w_raw (the fp64 forward restatement rounded once: inputs, not recomputed)."""
    base = kind[:-2] if kind.endswith("_T") else kind
    d = U.build_k7(dict(F=c["F"], lmax=c["lmax"], mode=c["mode"] & 15, w_raw=True, flags=c["flags"]), base, seed)
    if base != kind:
        d = _regraph(d, kind)
    d["case"], d["mode"], d["form"], d["act"] = c, c["mode"], hb_form(c), c["act"]
    E, F = d["E"], d["F"]
    g = torch.Generator().manual_seed(8803 + 31 * seed + F + 7 * c["lmax"] + 3 * len(kind))
    d["g_t_out"], d["pre_t"] = torch.randn(E, F, generator=g), torch.randn(E, F, generator=g) * 1.5
    fw = U.ref_k7(d, mode=c["mode"] & 15)
    d["w"], d["w_raw"] = fw["w"].float(), fw["w_raw"].float()
    d.update(csc_view(d))
    d["ns"] = slots(F)
    return d


def _gate64(wr, kind):
    """gate'(w_raw) and |its error| / u."""
    if kind == 0:
        return torch.ones_like(wr), torch.zeros_like(wr)
    if kind == 1:
        s = torch.sigmoid(wr)
        return s * (1.0 - s), 9.0 * s * (1.0 - s) + s + 8.0 * s * s
    if kind == 2:
        th = torch.tanh(wr)
        return 1.0 - th * th, 9.0 * th * th + 2.0
    _, df, _, e_df = _act64(wr, A.ACT_SILU)
    return df, e_df


def ref_hb(d, mut=None):
    """fp64 restatement of the HTR backward -> dict(output -> tensor, "b:" + output -> bound); g_pre_t is absent with DIRECT."""
    S, F, N, E, ns, mode = d["S"], d["F"], d["N"], d["E"], d["ns"], d["mode"]
    joint, rej, gate, direct = bool(mode & U.HTR_JOINT), not (mode & U.HTR_NOREJ), (mode >> 2) & 3, bool(mode & HTR_DIRECT)
    src, seg = d["src"].long(), d["seg"]
    EQ, EK, r = d["EQ"].double(), d["EK"].double(), d["rl"].double()
    qi, kj = EQ[seg], EK[src]
    gt = d["g_t_out"].double()
    R, Bd = {}, {}
    # fl: gw is a product of up to three factors and a saturated gate takes it below the smallest normal, where it may be
    # flushed: 2^-126 on gw, times the magnitude it multiplies
    fin = lambda name, val, e_u, fl=0.0: (R.__setitem__(name, val), Bd.__setitem__(name, U32 * (e_u + val.abs()) + FLOOR * (1.0 + fl)))
    if direct:
        gw, E_gw = gt, torch.zeros_like(gt)
    else:
        pt = d["pre_t"].double()
        f, df, e_f, e_df = _act64(pt, d["act"])
        dg, e_dg = _gate64(d["w_raw"].double(), gate)
        gw = gt * f * dg
        E_gw = gt.abs() * ((f * dg).abs() * (e_f + 2.0) + f.abs() * e_dg)
        w = d["w"].double()
        if mut == "act_for_dact":
            df = f
        fin("g_pre_t", gt * w * df, (gt * w).abs() * e_df + 2.0 * (gt * w * df).abs(), df.abs())
    indeg, outdeg = torch.tensor(d["degs"], dtype=torch.float64), d["outdeg"].double()
    chain_in = (torch.ceil(indeg / ns) + ns + 1.0).view(-1, 1, 1)
    chain_out = (torch.ceil(outdeg / ns) + ns + 1.0).view(-1, 1, 1)
    lw = math.log2(min(F // 4, 64))
    gq_e, gk_e = torch.zeros(E, S.D, F, dtype=torch.float64), torch.zeros(E, S.D, F, dtype=torch.float64)
    Tq, Tk = torch.zeros_like(gq_e), torch.zeros_like(gq_e)
    g_rl, T_rl, F_rl = (torch.zeros(E, S.D, dtype=torch.float64) for _ in range(3))
    n_max = 0
    for lo, hi in U._k7_blocks(S, joint):
        n = hi - lo + (S.lmax if joint else 0)
        n_max = max(n_max, n)
        qb, kb, rb = qi[:, lo:hi], kj[:, lo:hi], r[:, lo:hi, None]
        pa, pb, rr = (qb * rb).sum(1, keepdim=True), (kb * rb).sum(1, keepdim=True), (rb * rb).sum(1, keepdim=True)
        Aq, Ak = (qb * rb).abs().sum(1, keepdim=True), (kb * rb).abs().sum(1, keepdim=True)
        c = (2.0 - rr) if rej else torch.zeros_like(rr)
        ck = (torch.ones_like(rr) if mut == "rr_factor_one" else c) if rej else c
        cm = (2.0 + rr) if rej else torch.zeros_like(rr)
        gq_e[:, lo:hi] = gw[:, None] * (kb - c * rb * pb)
        gk_e[:, lo:hi] = gw[:, None] * (qb - ck * rb * pa)
        Tq[:, lo:hi] = kb.abs() + cm * rb.abs() * Ak
        Tk[:, lo:hi] = qb.abs() + cm * rb.abs() * Aq
        t = -c * (qb * pb + pa * kb) + (2.0 * rb * pa * pb if rej else 0.0)
        Tm = cm * (qb.abs() * Ak + Aq * kb.abs()) + (2.0 * rb.abs() * Aq * Ak if rej else 0.0)
        g_rl[:, lo:hi] = (gw[:, None] * t).sum(2)
        T_rl[:, lo:hi] = (E_gw[:, None] * Tm + gw.abs()[:, None] * (3.0 * n + 12.0 + lw) * Tm).sum(2)
        F_rl[:, lo:hi] = Tm.sum(2)
    cn = 2.0 * n_max + 6.0
    fin("gEQ", _seg_sum(gq_e, seg, N), _seg_sum(E_gw[:, None] * Tq + cn * gw.abs()[:, None] * Tq, seg, N)
        + chain_in * _seg_sum(gw.abs()[:, None] * Tq, seg, N), _seg_sum(Tq, seg, N))
    fin("gEK", _seg_sum(gk_e, src, N), _seg_sum(E_gw[:, None] * Tk + cn * gw.abs()[:, None] * Tk, src, N)
        + chain_out * _seg_sum(gw.abs()[:, None] * Tk, src, N), _seg_sum(Tk, src, N))
    fin("g_rl", g_rl, T_rl, F_rl)
    R.update({"b:" + kname: b for kname, b in Bd.items()})
    return R


# ------------------------------------------------------------------------------------------------ fp32 emulations
def _slot_sum32(terms, idx, order, ptr, ns):
    """Node sums in the kernels' order, fp32: entry `ptr[n] + slot + t ns` of `order` goes to slot `slot` serially, the slot
    partials are added in slot order.  terms [E, ...] fp32 -> [N, ...] fp32."""
    N = ptr.numel() - 1
    ptr = ptr.long()
    acc = torch.zeros((N, ns) + tuple(terms.shape[1:]))
    maxdeg = int((ptr[1:] - ptr[:-1]).max()) if N else 0
    for t in range((maxdeg + ns - 1) // ns):
        pos = ptr[:-1, None] + t * ns + torch.arange(ns)[None]
        nv, sv = (pos < ptr[1:, None]).nonzero(as_tuple=True)
        if nv.numel():
            acc[nv, sv] = acc[nv, sv] + terms[order[pos[nv, sv]]]
    s = acc[:, 0]
    for kk in range(1, ns):
        s = s + acc[:, kk]
    return s


def _act32(t, act):
    if act == A.ACT_SILU:
        s = torch.sigmoid(t)
        return t * s, s * (1.0 + t * (1.0 - s))
    th = torch.tanh(t)
    return th, 1.0 - th * th


def group_blocks(lmax):
    """The value blocks of the degree groups {scalar,1,2}, {3}, {4} (sep_dir and sep_tensor: block l = direction gate,
    lmax + l = tensor gate of degree l)."""
    return [[0, 1, 2, lmax + 1, lmax + 2]] + [[l, lmax + l] for l in range(3, lmax + 1)]


def mb_fp32(d):
    """The message backward in fp32 in the kernels' own order (the by-target / by-source pair, the merged and the degree-sliced
    kernels: fma chains over the rows of a gate, fma(a, v, (tf x) cut), slot-strided serial node sums by CSR row and by CSC
    column, slot partials in slot order; the degree-group forms: the head sums of each group's blocks, then the G slices added
    in slice order, as attn_bwd_body does).  Channel and head sums use torch's fp32 sums (a pairwise tree, as the butterflies are)."""
    S, F, H, N, E, ns = d["S"], d["F"], d["H"], d["N"], d["E"], d["ns"]
    M, D, act, aggr = S.M, S.D, d["case"]["act"], d["aggr"]
    src, seg = d["src"].long(), d["seg"]
    x64, v64, tf64 = _clean_blocks(d)
    x, v, tf = x64.float(), v64.float(), tf64.float()
    first = d["X_in"] is None
    Xin = torch.zeros(N, D, F) if first else d["X_in"]
    a, cut, rl = d["a"], d["cut"], d["rl"]
    a_soft = a if d["a_soft"] is None else d["a_soft"]
    hidx, hq = U.head_index(S, F, H), torch.arange(F) // (F // H)
    indeg = torch.tensor(d["degs"])
    gm = torch.cat([d["g_h1"][:, None], d["g_X1"]], 1)[seg]
    inv = torch.ones(E)
    if aggr == "mean":
        inv = (1.0 / indeg.clamp_min(1).float())[seg]
    elif aggr == "max":
        msg = _fwd_messages(d, x64, v64, tf64, a.double(), hidx, fp32=True)
        hit = max_route(msg.double(), seg, N)
        cnt = torch.round(1.0 / hit.clamp_min(1e-30)).float()
        gm = torch.where(hit > 0, gm / cnt, torch.zeros(()))
    xj, vj, Xj = x[src], v[src], Xin[src]
    ah = a[:, hidx.reshape(-1)].view(E, M, F)
    o = U.fma32(ah, vj, (tf * xj) * cut.view(-1, 1, 1))
    go = torch.zeros(E, M, F)
    go[:, 0] = gm[:, 0] * inv.view(-1, 1)
    for m, l in enumerate(S.l_of):                  # rows ascending: the fma chains of the gates
        go[:, S.dblk(l)] = U.fma32(rl[:, m, None], gm[:, 1 + m], go[:, S.dblk(l)])
    got = torch.zeros(E, M, F)
    for m, l in enumerate(S.l_of):
        got[:, S.tblk(l)] = U.fma32(gm[:, 1 + m], Xj[:, m], got[:, S.tblk(l)])
    go = go + got                                   # (a block is a direction gate or a tensor gate: one of the two is zero)
    go[:, 1:] = go[:, 1:] * inv.view(-1, 1, 1)
    bd, bt = torch.tensor([S.dblk(l) for l in S.l_of]), torch.tensor([S.tblk(l) for l in S.l_of])
    out = {}
    out["g_tf"] = (go * xj) * cut.view(-1, 1, 1)
    out["g_cut"] = ((go * tf) * xj).sum((1, 2))
    if d["form"].startswith("groups"):
        g_a = torch.zeros(E, H)
        for blocks in group_blocks(S.lmax):
            g_a = g_a + torch.zeros(E, H).index_add_(1, hidx[blocks].reshape(-1), (go * vj)[:, blocks].reshape(E, len(blocks) * F))
    else:
        g_a = torch.zeros(E, H).index_add_(1, hidx.reshape(-1), (go * vj).reshape(E, M * F))
    out["g_rl"] = ((gm[:, 1:] * o[:, bd]).sum(2)) * inv.view(-1, 1)
    order_t, order_s = torch.arange(E), d["perm"].long()
    # fma chains of the node sums are emulated as product-then-add (one rounding more than the kernels' fma)
    out["g_x"] = _slot_sum32(go * (tf * cut.view(-1, 1, 1)), src, order_s, d["colptr"], ns)
    out["g_v"] = _slot_sum32(ah * go, src, order_s, d["colptr"], ns)
    if not first:
        out["g_X_out"] = d["g_X1"] + _slot_sum32(gm[:, 1:] * (o[:, bt] * inv.view(-1, 1, 1)), src, order_s, d["colptr"], ns)
    nrm = (torch.sqrt(d["outdeg"].float()[src]) if d["use_outdeg"] else torch.ones(E)) * torch.tensor(1.0 / math.sqrt(F)).float()
    dot = torch.zeros(N, H).index_add_(0, seg, a * g_a)
    g_s = a * g_a - (a_soft / nrm[:, None]) * dot[seg]
    out["g_s"] = g_s
    f, df = _act32(d["eproj"][:, :F], act)
    q, k = d["qk"][:, :F], d["qk"][:, F:2 * F]
    gsc = g_s[:, hq]
    out["g_q"] = _slot_sum32(gsc * (k[src] * f), seg, order_t, d["rowptr"], ns)
    out["g_k"] = _slot_sum32(gsc * (q[seg] * f), src, order_s, d["colptr"], ns)
    out["g_pta"] = ((q[seg] * k[src]) * gsc) * df
    return out


def hb_fp32(d, order="general"):
    """The HTR backward in fp32 in the kernels' own order: fma chains pa, pb, r . r rows ascending, slot-strided node sums, and
    per row either the general / degree-sliced kernels' expressions (gw (ek + pb (-c r)); gw ((eq pb + pa ek)(-c) + pa pb 2 r))
    or, order = "tuned", those of the register-tiled kernels, which factor gw out of the per-row terms (u = gw pb (-c),
    v = gw pa (-c), s2 = gw (pa pb) 2: fma(r, u, gw ek); fma(gw, eq + pa (-c r)); fma(r, s2, fma(v, ek, u eq)))."""
    S, F, N, E, ns, mode = d["S"], d["F"], d["N"], d["E"], d["ns"], d["mode"]
    joint, rej, gate, direct = bool(mode & U.HTR_JOINT), not (mode & U.HTR_NOREJ), (mode >> 2) & 3, bool(mode & HTR_DIRECT)
    src, seg = d["src"].long(), d["seg"]
    qi, kj, r = d["EQ"][seg], d["EK"][src], d["rl"]
    out = {}
    gw = d["g_t_out"]
    if not direct:
        f, df = _act32(d["pre_t"], d["act"])
        out["g_pre_t"] = (gw * d["w"]) * df
        gw = gw * f
        if gate:
            wr = d["w_raw"]
            s, th = torch.sigmoid(wr), torch.tanh(wr)
            gw = gw * {1: s * (1.0 - s), 2: 1.0 - th * th, 3: _act32(wr, A.ACT_SILU)[1]}[gate]
    gq_e, gk_e, g_rl = torch.zeros(E, S.D, F), torch.zeros(E, S.D, F), torch.zeros(E, S.D)
    for lo, hi in U._k7_blocks(S, joint):
        z = torch.zeros(E, F)
        pa, pb, rr = z, z, torch.zeros(E, 1)
        for m in range(lo, hi):
            pa, pb = U.fma32(r[:, m, None], qi[:, m], pa), U.fma32(r[:, m, None], kj[:, m], pb)
            rr = U.fma32(r[:, m, None], r[:, m, None], rr)
        c = (2.0 - rr) if rej else torch.zeros(E, 1)
        for m in range(lo, hi):
            rm = r[:, m, None]
            if order == "tuned":
                assert rej and not direct
                u, v, s2 = (gw * pb) * (-c), (gw * pa) * (-c), (gw * (pa * pb)) * 2.0
                gq_e[:, m] = U.fma32(rm.expand(E, F).contiguous(), u, gw * kj[:, m])
                gk_e[:, m] = gw * (qi[:, m] + pa * (-c * rm))
                t4 = U.fma32(rm.expand(E, F).contiguous(), s2, U.fma32(v, kj[:, m], u * qi[:, m]))
            else:
                gq_e[:, m] = gw * (kj[:, m] + pb * (-c * rm))
                gk_e[:, m] = gw * (qi[:, m] + pa * (-c * rm))
                t4 = gw * ((qi[:, m] * pb + pa * kj[:, m]) * (-c) + (pa * pb) * (2.0 * rm if rej else 0.0 * rm))
            g_rl[:, m] = t4.sum(1)
    out["gEQ"] = _slot_sum32(gq_e, seg, torch.arange(E), d["rowptr"], ns)
    out["gEK"] = _slot_sum32(gk_e, src, d["perm"].long(), d["colptr"], ns)
    out["g_rl"] = g_rl
    return out


# ------------------------------------------------------------------------------------------------ shared, read-only
def ratios(got, ref, names, masks=None):
    """{output: worst |got - ref| / bound}."""
    return {n: U.worst_ratio(got[n], ref[n], ref["b:" + n], None if masks is None else masks.get(n)) for n in names if n in ref}


@functools.lru_cache(maxsize=8)
def _built_mb(key, kind):
    d = build_mb(dict(key), kind)
    check_csc(d)
    return d, ref_mb(d)


def built_mb(c, kind):
    return _built_mb(tuple(sorted(c.items())), kind)


@functools.lru_cache(maxsize=8)
def _built_hb(key, kind):
    d = build_hb(dict(key), kind)
    check_csc(d)
    return d, ref_hb(d)


def built_hb(c, kind):
    return _built_hb(tuple(sorted(c.items())), kind)


def relabel_bwd(d, perm):
    """gather_util.relabel plus the backward's node / edge tensors -> (dict, emap).  The by-source view is CARRIED, not re-sorted:
    every source keeps its own out-edge order (as every target keeps its in-edge order), so that sums by source keep their bits."""
    d2, emap = U.relabel(d, perm)
    for key in ("qk", "g_h1", "g_X1"):
        if d.get(key) is not None:
            d2[key] = d[key][perm].contiguous()
    for key in ("eproj", "a_soft", "g_t_out", "pre_t", "w", "w_raw"):
        if d.get(key) is not None:
            d2[key] = d[key][emap].contiguous()
    inv_e = torch.empty(d["E"], dtype=torch.long)
    inv_e[emap] = torch.arange(d["E"])
    cp, old = d["colptr"].long(), d["perm"].long()
    cols = [inv_e[old[int(cp[j]):int(cp[j + 1])]] for j in perm.tolist()]
    newperm = torch.cat(cols + [torch.zeros(0, dtype=torch.long)])
    outdeg = d["outdeg"][perm].contiguous()
    colptr = torch.zeros(d["N"] + 1, dtype=torch.int32)
    colptr[1:] = outdeg.long().cumsum(0).to(torch.int32)
    d2.update(colptr=colptr, perm=newperm.to(torch.int32).contiguous(), outdeg=outdeg,
              tgt_by_src=d2["seg"][newperm].to(torch.int32).contiguous())
    return d2, emap
