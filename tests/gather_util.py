"""Yardstick of the two forward gather entry points, gn_message_aggregate (K6) and gn_htr_edge (K7) (csrc/gn_gata.hip,
gn_options.hip, gn_highl.hip): hand-built CSR graphs at the kernels' own edges, an fp64 restatement of the header's
formulas, an a-priori per-element error bound, the case table and the launchers' routing restated in Python.

The operations (include/gotennet_hip.h, "K6 GATA message / softmax / aggregate" and "K7 HTR edge weights"), for target i
with incoming edges e (source j), M F-wide blocks of the value vector (0 scalar | ND direction gates | NT tensor gates):

    o[e,b,c]   = t_filter[e,b,c] x[j,b,c] cut[e] + a[e, (b F + c) / (M F / H)] v[j,b,c]
    h_out[i]   = h_in[i] + aggr_e o[e,0,:]
    X_out[i,m] = X_in[i,m] + aggr_e ( rl[e,m] o[e,dblk(l(m))] + X_in[j,m] o[e,tblk(l(m))] )
    dblk(l) = sep_dir ? l : 1,   tblk(l) = 1 + ND + (sep_tensor ? l - 1 : 0);   aggr = sum | mean | max (0 without edges)
    w[e,f]     = g( sum_blocks sum_m P(EQ[i])_m P(EK[j])_m ),  P(a) = a - (a . rl_B) rl_B per block B (a degree; all D rows when
                 joint; the identity with norej),  g = identity | sigmoid | tanh | SiLU;  w_raw = the sum before g.

The bounds (u = 2^-24, the unit round-off of fp32; the library is built with -ffp-contract=off, so every rounding below is
one the source spells; every constant is counted off the kernels' arithmetic, none is fitted to a measured error)
--------------------------------------------------------------------------------------------------------------------
K6.  T_e = the un-cancelled magnitude of edge e's contribution to one output element:
       row 0:  |tf x cut| + |a v|                                        (block 0)
       row m:  |rl_m| (|tf x cut| + |a v|)[dblk] + |X_j,m| (|tf x cut| + |a v|)[tblk]
  One term: (tf x) cut is two roundings, fma(a, v, .) a third; o_d rl a fourth; fma(X_j, o_t, .) a fifth: c_term = 5.
  The sum: a slot adds its share serially, edge e0 + slot + n ns, so a term meets at most ceil(deg / ns) roundings
  (ns = 256 / (F / 4) slots, at least 1); the slot partials are added in slot order, at most ns more; one more covers the
  second-order terms.  The residual add rounds the result once.

    add:   |out^ - out| <= u (5 + ceil(deg / ns) + ns + 1) sum_e T_e + u |residual + sum| + 2^-126
    mean:  the factor 1.0f / (float)deg is a correctly rounded division (u) and one product (u); taken as 4 u:
           |out^ - out| <= u (5 + ceil(deg / ns) + ns + 1 + 4) sum_e T_e / deg + u |residual + mean| + 2^-126
    max:   no sum, only the term error remains, |max_e c^_e - max_e c_e| <= max_e |c^_e - c_e|:
           |out^ - out| <= u (5 + 1) max_e T_e + u |residual + max| + 2^-126
  (2^-126: a result below the smallest normal may be flushed; added once.  The zero-X_in form has no residual add on X; the
  term stays, the bound is the same for both forms.)
K7, per block B of n rows (n = 2 l + 1, or D when joint; nb blocks; D rows in all), with A_q = sum_m |r_m EQ_m|,
  A_k = sum_m |r_m EK_m|, rr = r . r (NOT 1: the reference's degree >= 3 harmonics have r . r in 2.5 .. 7, self-loops 0):
  literal (htr_edge_kernel, lmax <= 2):  pq = sum r EQ is an n-term fma chain (n u A_q); a_m = EQ_m + pq (-r_m) is a product
    and an add:  |a^_m - P(EQ)_m| <= u (|EQ_m| + (n + 3) |r_m| A_q), one more for the second order; the D products
    a_m b_m are accumulated by one fma chain (D roundings, + 1):
      |w^ - w| <= u sum_B [ (D + 1) sum_m |P(EQ)_m| |P(EK)_m|
                            + sum_m ( (|EQ_m| + (n + 4) |r_m| A_q) |P(EK)_m| + |P(EQ)_m| (|EK_m| + (n + 4) |r_m| A_k) ) ]
  closed (lmax 3, lmax 4 "all rows first", every `mode` kernel, the degree-sliced kernel):
    w_B = EQ.EK - (2 - rr) (EQ.r) (EK.r).  EQ.EK: n-term fma chain (n u sum |EQ||EK|).  The product term: pq, pk, rr are
    n-term chains (3 n u), 2 - rr one rounding, two products (2 u): (3 n + 3) u (2 + rr) A_q A_k, using |2 - rr| <= 2 + rr.
    The difference rounds once and the block results are added serially (nb roundings) on the un-cancelled magnitude:
      |w^ - w| <= u sum_B [ (n + 1 + nb) sum_m |EQ_m| |EK_m| + (3 n + 4 + nb) (2 + rr) A_q A_k ]      (norej: first term only)
  gate g on w^ (gn_highl.h gate1):  |g(w^) - g(w)| <= sup|g'| |w^ - w| + eps_g |g(w)|, with
    sigmoid = 1 / (1 + expf(-w)): expf 2 ulp (4 u), the add u, the division <= 3 u: eps_g = 8 u, sup|g'| = 1/4;
    tanh (library tanhf, 2 ulp): eps_g = 4 u, sup|g'| = 1;
    SiLU = w * sigmoid_fast(w) (v_exp_f32 / v_rcp_f32; the figures tests/attn_util.py carries for the same function):
    eps_g = (6 + 2 |w|) u, sup|g'| = 1.1.
  2^-126 is added once, as for K6.
"""
import functools
import math

import torch

U32 = 2.0 ** -24
FLOOR = 2.0 ** -126
SLICED, MEAN, MAX = 0x100, 0x200, 0x400            # GN_LMAX_SLICED / _MEAN / _MAX of include/gotennet_hip.h
HTR_JOINT, HTR_NOREJ = 1, 2                        # GN_HTR_JOINT / _NOREJ; the gate kind sits in bits 2..3
GATE_NAMES = {0: "none", 1: "sigmoid", 2: "tanh", 3: "silu"}
PAD_COLS = 8                                       # NaN columns past M F in the x / v rows (ldxv = M F + 8)


# ------------------------------------------------------------------------------------------------ shapes and routing
class Shape:
    """Block layout of the value vector for (lmax, sep_dir, sep_tensor) (gotennet.py:197-203)."""

    def __init__(self, lmax, sd, st):
        self.lmax, self.sd, self.st = lmax, bool(sd), bool(st)
        self.D = (lmax + 1) ** 2 - 1
        self.ND, self.NT = (lmax if sd else 1), (lmax if st else 1)
        self.M = 1 + self.ND + self.NT
        self.l_of = [l for l in range(1, lmax + 1) for _ in range(2 * l + 1)]      # degree of row m

    def dblk(self, l):
        return l if self.sd else 1

    def tblk(self, l):
        return 1 + self.ND + (l - 1 if self.st else 0)


def slots(F):
    return max(1, 256 // (F // 4))


def head_ok(M, F, H):
    return H > 0 and (M * F) % H == 0 and ((M * F) // H) % 4 == 0


def aggr_of(flags):
    return "mean" if flags & MEAN else ("max" if flags & MAX else "add")


def use_highl(lmax, flags):
    """gn_use_highl (csrc/gn_highl.hip)."""
    return lmax > 4 or (flags & (SLICED | MEAN | MAX)) != 0


def kernel_form(entry, F, lmax, sep_dir=True, sep_tensor=True, first=False, sliced=False, aggr="add", mode=0):
    """The kernel(s) the launcher picks: the switch of gn_message_aggregate, the routing of gn_htr_edge (csrc/gn_gata.hip)
    and gn_use_highl.  entry = "msg" | "htr"."""
    tf = lambda b: "T" if b else "F"
    highl = lmax > 4 or sliced or aggr != "add"
    if entry == "msg":
        if highl:
            assert not first                       # refused: GN_ERR_BAD_ARG
            return f"hl_msg<{lmax}>({aggr})"
        if lmax == 1:
            sep_dir = sep_tensor = False           # lmax = 1: the flags are no-ops, one instantiation
        fc = 256 if F == 256 and ((sep_dir and sep_tensor) or lmax == 1) else 0
        head = f"{lmax},{tf(sep_dir)},{tf(sep_tensor)}"
        if lmax <= 2 or first:
            return f"mono<{head},{'first' if first else 'full'},{fc}>"
        rest = f"group34<{head},3..4,{fc}>" if lmax == 4 else f"group<{head},3..3,{fc}>"      # GN_K6_MERGE34 = 1
        return f"group<{head},1..2,scalar,{fc}>+{rest}"
    assert entry == "htr"
    if highl:
        return "hl_htr"
    if mode:
        return f"htr_general<{lmax}>"
    fc = 256 if F == 256 else 0
    return {1: "htr_literal<1,%d>", 2: "htr_literal<2,%d>", 3: "htr_closed<3,%d>", 4: "htr_closed_all<4,%d>"}[lmax] % fc


def htr_arith(form):
    """Which of the two K7 bounds / restatements a kernel form is held to."""
    return "literal" if form.startswith("htr_literal") else "closed"


# ------------------------------------------------------------------------------------------------ graphs
def graph_degrees(kind, ns):
    """In-degrees of the hand-built graphs (hub: the hub's index is 7; its edge 150 is the self-loop)."""
    if kind == "ragged":                           # N = 11: a degree-0 target first, last and between the two longest
        return [0, 2 * ns + 1, 0, 65, 1, max(ns - 1, 0), ns, ns + 1, 63, 64, 0]
    if kind == "ragged9":
        return [0, 2 * ns + 1, 0, 65, 1, ns, ns + 1, 64, 0]
    if kind == "single":                           # N = 1: every edge is a self-loop
        return [ns + 1]
    if kind == "hub":
        return [3] * 7 + [301] + [3] * 13
    if kind == "empty":
        return [0] * 5
    raise KeyError(kind)


HUB, HUB_SELF = 7, 150


def make_graph(kind, ns, seed=0):
    degs = graph_degrees(kind, ns)
    N = len(degs)
    assert N <= 330 and sum(degs) <= 4000 and (N % 8 or kind == "empty")
    g = torch.Generator().manual_seed(4242 + 17 * seed + ns)
    rowptr = torch.zeros(N + 1, dtype=torch.int32)
    rowptr[1:] = torch.tensor(degs, dtype=torch.int64).cumsum(0).to(torch.int32)
    E = int(rowptr[-1])
    src = torch.randint(0, N, (E,), generator=g, dtype=torch.int32)       # with repeats: rows are shared
    if kind == "hub":
        src[int(rowptr[HUB]) + HUB_SELF] = HUB
    seg = torch.repeat_interleave(torch.arange(N), torch.tensor(degs, dtype=torch.int64))
    return dict(kind=kind, degs=degs, N=N, E=E, rowptr=rowptr, src=src, seg=seg)


def _rl(g, gr, S):
    """Per degree block a random direction times a block norm in [0.5, 2.7] (r . r != 1); zero rows on self-loops."""
    E = gr["E"]
    rl = torch.zeros(E, S.D)
    for l in range(1, S.lmax + 1):
        lo, n = l * l - 1, 2 * l + 1
        d = torch.randn(E, n, generator=g)
        d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-6)
        rl[:, lo:lo + n] = d * (0.5 + 2.2 * torch.rand(E, 1, generator=g))
    rl[gr["src"].long() == gr["seg"]] = 0.0
    return rl


# ------------------------------------------------------------------------------------------------ K6 inputs
def k6_case(F, lmax, sd, st, hk, first=False, flags=0):
    S = Shape(lmax, sd, st)
    if hk == "one":
        H = 1
    elif hk == "max":
        H = S.M * F // 4                           # the largest H with (M F / H) % 4 == 0
    else:                                          # the default-like H = 8 (4 where 8 is refused)
        H = 8 if head_ok(S.M, F, 8) else 4
    assert head_ok(S.M, F, H)
    return dict(F=F, lmax=lmax, sd=bool(sd), st=bool(st), H=H, first=first, flags=flags)


def k6_id(c):
    fl = "".join(n for b, n in ((SLICED, "-sliced"), (MEAN, "-mean"), (MAX, "-max")) if c["flags"] & b)
    return f"F{c['F']}-l{c['lmax']}-{'T' if c['sd'] else 'F'}{'T' if c['st'] else 'F'}-H{c['H']}{'-first' if c['first'] else ''}{fl}"


def k6_form(c):
    return kernel_form("msg", c["F"], c["lmax"], c["sd"], c["st"], c["first"], bool(c["flags"] & SLICED), aggr_of(c["flags"]))


def _k6_cases():
    out, T, Fa = [], True, False
    add = lambda *a, **k: out.append(k6_case(*a, **k))
    for F, hk in ((16, "max"), (64, "def"), (256, "def")):                 # lmax 1 (M = 3)
        for first in (Fa, T):
            add(F, 1, T, T, hk, first)
    add(64, 1, Fa, T, "one")
    rot, n = ("one", "max", "def"), 0
    for lmax in (2, 3, 4):                                                  # every (sep_dir, sep_tensor) pair, both X_in forms
        for sd in (T, Fa):
            for st in (T, Fa):
                for first in (Fa, T):
                    add(64, lmax, sd, st, "def" if (sd and st) else rot[n % 3], first)
                    n += 1
    add(64, 2, T, T, "one"); add(64, 2, T, T, "max"); add(64, 4, T, T, "max")
    add(16, 2, T, T, "def"); add(16, 3, Fa, T, "max"); add(16, 4, T, Fa, "one"); add(16, 4, T, T, "def", True)   # ns = 64
    for lmax in (2, 3, 4):                                                  # the compile-time-width forms
        for first in (Fa, T):
            add(256, lmax, T, T, "def", first)
    add(256, 3, T, Fa, "def")
    add(512, 2, T, T, "def"); add(512, 2, T, T, "def", True); add(1024, 2, T, T, "def")
    for lmax, sd, st, hk in ((2, T, T, "def"), (2, T, Fa, "one"), (4, T, T, "def"), (4, Fa, T, "max")):
        add(64, lmax, sd, st, hk, flags=SLICED)
    add(32, 5, T, T, "def"); add(32, 5, Fa, T, "max"); add(32, 8, T, T, "def"); add(32, 8, T, Fa, "one")
    add(64, 2, T, T, "def", flags=MEAN); add(32, 5, T, T, "def", flags=MEAN); add(32, 8, Fa, Fa, "one", flags=MEAN)
    add(64, 3, T, T, "def", flags=MAX); add(32, 8, T, T, "def", flags=MAX)
    return out


K6_CASES = _k6_cases()


def head_index(S, F, H, per_head=None):
    """[M, F] long: the attention head of channel c of block b, (b F + c) / (M F / H)."""
    per_head = (S.M * F) // H if per_head is None else per_head
    return (torch.arange(S.M * F) // per_head).clamp_max(H - 1).view(S.M, F)


def build_k6(c, kind, seed=0):
    """CPU tensors of one case on one graph.  x / v sit in rows of ldxv = M F + 8 floats and t_filter at column F of rows of
    ldt = (1 + M) F floats (the t_attn block first, as the engine lays eproj out); every float outside the blocks is NaN."""
    F, H, S = c["F"], c["H"], Shape(c["lmax"], c["sd"], c["st"])
    gr = make_graph(kind, slots(F), seed)
    N, E, M, D = gr["N"], gr["E"], S.M, S.D
    g = torch.Generator().manual_seed(991 + 31 * seed + F + 7 * c["lmax"] + H)
    rn = lambda *s: torch.randn(*s, generator=g)
    ldxv, ldt = M * F + PAD_COLS, (1 + M) * F
    xbuf, vbuf, tbuf = torch.full((N, ldxv), math.nan), torch.full((N, ldxv), math.nan), torch.full((E, ldt), math.nan)
    xbuf[:, :M * F], vbuf[:, :M * F], tbuf[:, F:] = rn(N, M * F), rn(N, M * F), rn(E, M * F)
    a = rn(E, H) * 0.5                              # signed: it carries `norm`
    cut = torch.rand(E, generator=g)
    cut[::7] = 0.0
    rl = _rl(g, gr, S)
    if c["flags"] & MAX and E:                      # exact ties: the first two edges of every target with two or more
        for i, deg in enumerate(gr["degs"]):
            e0 = int(gr["rowptr"][i])
            if deg >= 2:
                gr["src"][e0 + 1] = gr["src"][e0]
                tbuf[e0 + 1], a[e0 + 1], cut[e0 + 1], rl[e0 + 1] = tbuf[e0], a[e0], cut[e0], rl[e0]
    h_in, X_in = rn(N, F), (None if c["first"] else rn(N, D, F))
    if c["first"]:                                  # the zero-X_in form must not read the tensor-gate blocks
        lo = (1 + S.ND) * F
        xbuf[:, lo:], vbuf[:, lo:], tbuf[:, F + lo:] = math.nan, math.nan, math.nan
    d = dict(gr, case=c, S=S, F=F, H=H, xbuf=xbuf, vbuf=vbuf, tbuf=tbuf, ldxv=ldxv, ldt=ldt, a=a, cut=cut, rl=rl,
             h_in=h_in, X_in=X_in, lmax_arg=c["lmax"] | c["flags"], aggr=aggr_of(c["flags"]), ns=slots(F))
    return d


def _blocks(d):
    S, F, N, E = d["S"], d["F"], d["N"], d["E"]
    x = d["xbuf"][:, :S.M * F].reshape(N, S.M, F)
    v = d["vbuf"][:, :S.M * F].reshape(N, S.M, F)
    tf = d["tbuf"][:, F:].reshape(E, S.M, F)
    return x, v, tf


def _aggregate(msg, seg, N, aggr, deg):
    out = torch.zeros((N,) + tuple(msg.shape[1:]), dtype=msg.dtype)
    if aggr == "max":
        return out.scatter_reduce(0, seg.view(-1, 1, 1).expand_as(msg), msg, "amax", include_self=False)
    out.index_add_(0, seg, msg)
    return out / deg.clamp_min(1).to(msg.dtype).view(-1, 1, 1) if aggr == "mean" else out


def ref_k6(d, hidx=None, dblk=None, tblk=None, rlcol=None, cut=None, keep=None):
    """fp64, from the fp32 inputs -> dict(out [N, 1 + D, F] (row 0 = h_out), T = sum_e T_e (max_e T_e under max)).
    The keyword arguments are the mutations a meaningful bound must reject: another head map, other gate blocks per degree,
    other rl columns, another cut, edges taken out."""
    S, F, H, N, E = d["S"], d["F"], d["H"], d["N"], d["E"]
    src, seg = d["src"].long(), d["seg"]
    x, v, tf = (t.double() for t in _blocks(d))
    hidx = head_index(S, F, H) if hidx is None else hidx
    cut = (d["cut"] if cut is None else cut).double()
    sp = tf * x[src] * cut.view(-1, 1, 1)
    av = d["a"].double()[:, hidx.reshape(-1)].view(E, S.M, F) * v[src]
    o, oa = sp + av, sp.abs() + av.abs()
    bd = torch.tensor([(S.dblk(l) if dblk is None else dblk[l]) for l in S.l_of])
    bt = torch.tensor([(S.tblk(l) if tblk is None else tblk[l]) for l in S.l_of])
    rl = d["rl"].double()
    rl = rl if rlcol is None else rl[:, rlcol]
    mX, TX = rl[:, :, None] * o[:, bd], rl.abs()[:, :, None] * oa[:, bd]
    if d["X_in"] is not None:
        Xj = d["X_in"].double()[src]
        mX, TX = mX + Xj * o[:, bt], TX + Xj.abs() * oa[:, bt]
    msg, T = torch.cat([o[:, :1], mX], 1), torch.cat([oa[:, :1], TX], 1)
    if keep is not None:
        msg, T, seg = msg[keep], T[keep], seg[keep]
    deg = torch.bincount(seg, minlength=N)
    res = torch.cat([d["h_in"].double()[:, None], torch.zeros(N, S.D, F, dtype=torch.float64) if d["X_in"] is None
                     else d["X_in"].double()], 1)
    out = res + _aggregate(msg, seg, N, d["aggr"], deg)
    Tagg = _aggregate(T, seg, N, "max" if d["aggr"] == "max" else "add", deg)
    return dict(out=out, T=Tagg, deg=deg)


def bound_k6(d, r):
    """The per-element absolute bound of the module docstring, [N, 1 + D, F] fp64."""
    ns, deg = d["ns"], r["deg"].double().view(-1, 1, 1)
    if d["aggr"] == "max":
        first = 6.0 * r["T"]
    elif d["aggr"] == "mean":
        first = (5.0 + torch.ceil(deg / ns) + ns + 1.0 + 4.0) * r["T"] / deg.clamp_min(1.0)
    else:
        first = (5.0 + torch.ceil(deg / ns) + ns + 1.0) * r["T"]
    return U32 * (first + r["out"].abs()) + FLOOR


def fma32(a, b, c):
    """fmaf on fp32 tensors: the product is exact in fp64, the sum rounds once there and once more to fp32."""
    return (a.double() * b.double() + c.double()).float()


def k6_fp32(d):
    """The kernels' arithmetic in fp32 in their own order: slot-strided serial sums (edge e0 + slot + n ns), the slot
    partials in slot order, then the residual.  -> [N, 1 + D, F] fp32."""
    S, F, H, N, E, ns = d["S"], d["F"], d["H"], d["N"], d["E"], d["ns"]
    src = d["src"].long()
    x, v, tf = _blocks(d)
    hidx = head_index(S, F, H)
    sp = (tf * x[src]) * d["cut"].view(-1, 1, 1)
    o = fma32(d["a"][:, hidx.reshape(-1)].view(E, S.M, F), v[src], sp)
    bd, bt = torch.tensor([S.dblk(l) for l in S.l_of]), torch.tensor([S.tblk(l) for l in S.l_of])
    mX = o[:, bd] * d["rl"][:, :, None]
    if d["X_in"] is not None:
        mX = fma32(d["X_in"][src], o[:, bt], mX)
    msg = torch.cat([o[:, :1], mX], 1)
    mx = d["aggr"] == "max"
    acc = torch.full((N, ns, 1 + S.D, F), -math.inf if mx else 0.0)
    rp = d["rowptr"].long()
    for t in range((max(d["degs"]) + ns - 1) // ns):
        e = rp[:-1, None] + t * ns + torch.arange(ns)[None]
        iv, sv = (e < rp[1:, None]).nonzero(as_tuple=True)
        if iv.numel():
            term = msg[e[iv, sv]]
            acc[iv, sv] = torch.maximum(acc[iv, sv], term) if mx else acc[iv, sv] + term
    s = acc[:, 0]
    for k in range(1, ns):
        s = torch.maximum(s, acc[:, k]) if mx else s + acc[:, k]
    deg = torch.tensor(d["degs"])
    if mx:
        s[deg == 0] = 0.0
    if d["aggr"] == "mean":
        s = s * (1.0 / deg.clamp_min(1).float()).view(-1, 1, 1)
    if d["X_in"] is None:
        return torch.cat([(d["h_in"] + s[:, 0])[:, None], s[:, 1:]], 1)
    return torch.cat([d["h_in"][:, None], d["X_in"]], 1) + s


# ------------------------------------------------------------------------------------------------ K7 inputs
def k7_case(F, lmax, mode=0, w_raw=False, flags=0):
    return dict(F=F, lmax=lmax, mode=mode, w_raw=w_raw, flags=flags)


def k7_id(c):
    return f"F{c['F']}-l{c['lmax']}-mode{c['mode']}{'-raw' if c['w_raw'] else ''}{'-sliced' if c['flags'] & SLICED else ''}"


def k7_form(c):
    return kernel_form("htr", c["F"], c["lmax"], sliced=bool(c["flags"] & SLICED), mode=c["mode"])


def _k7_cases():
    out = [k7_case(F, lmax) for F in (64, 256) for lmax in (1, 2, 3, 4)]
    out += [k7_case(16, 2), k7_case(16, 3), k7_case(1024, 1)]
    for lmax in (2, 3):                                                     # every non-zero mode, w_raw NULL and given
        for mode in range(1, 16):
            for raw in (False, True):
                out.append(k7_case(64, lmax, mode, raw))
    out += [k7_case(64, 1, HTR_JOINT | (3 << 2), True), k7_case(64, 4, HTR_JOINT | (1 << 2), True), k7_case(16, 4, HTR_NOREJ)]
    out += [k7_case(64, 2, flags=SLICED), k7_case(64, 4, flags=SLICED), k7_case(32, 5), k7_case(32, 8),
            k7_case(64, 4, HTR_JOINT | (2 << 2), True, SLICED), k7_case(32, 5, HTR_NOREJ | (3 << 2), True), k7_case(32, 8, HTR_JOINT)]
    return out


K7_CASES = _k7_cases()


def build_k7(c, kind, seed=0):
    F, lmax = c["F"], c["lmax"]
    S = Shape(lmax, True, True)
    gr = make_graph(kind, slots(F), seed)
    g = torch.Generator().manual_seed(577 + 31 * seed + F + 7 * lmax)
    EQ, EK = torch.randn(gr["N"], S.D, F, generator=g), torch.randn(gr["N"], S.D, F, generator=g)
    return dict(gr, case=c, S=S, F=F, EQ=EQ, EK=EK, rl=_rl(g, gr, S), lmax_arg=lmax | c["flags"], mode=c["mode"],
                form=k7_form(c))


def _k7_blocks(S, joint):
    return [(0, S.D)] if joint else [(l * l - 1, (l + 1) * (l + 1) - 1) for l in range(1, S.lmax + 1)]


def _gate64(w, kind):
    return {0: lambda t: t, 1: torch.sigmoid, 2: torch.tanh, 3: torch.nn.functional.silu}[kind](w)


def ref_k7(d, mode=None, rr_one_l3=False, rej_q_only=False, gate_raw=False):
    """fp64 -> dict(w_raw, w [E, F], b_lit, b_cl: the two bracketed sums of the module docstring).  ``mode`` overrides the
    case's; the other keyword arguments are mutations: r . r taken as 1 at degree 3, the rejection applied to EQ only,
    w_raw returned gated."""
    S, F = d["S"], d["F"]
    mode = d["mode"] if mode is None else mode
    joint, rej, gate = bool(mode & HTR_JOINT), not (mode & HTR_NOREJ), (mode >> 2) & 3
    q, k, r = d["EQ"].double()[d["seg"]], d["EK"].double()[d["src"].long()], d["rl"].double()
    blocks = _k7_blocks(S, joint)
    nb, w = len(blocks), 0.0
    b_lit, b_cl = 0.0, 0.0
    for lo, hi in blocks:
        n = hi - lo
        qb, kb, rb = q[:, lo:hi], k[:, lo:hi], r[:, lo:hi, None]
        pq, pk, rr = (qb * rb).sum(1), (kb * rb).sum(1), (rb * rb).sum(1)
        Aq, Ak = (qb * rb).abs().sum(1), (kb * rb).abs().sum(1)
        if rr_one_l3 and lo == 8 and not joint:
            wb = (qb * kb).sum(1) - (2.0 - 1.0) * pq * pk
            Pq, Pk = qb, kb
        else:
            Pq = qb - pq[:, None] * rb if rej else qb
            Pk = kb - pk[:, None] * rb if (rej and not rej_q_only) else kb
            wb = (Pq * Pk).sum(1)
        w = w + wb
        b_lit = b_lit + (S.D + 1.0) * (Pq * Pk).abs().sum(1) + (
            (qb.abs() + (n + 4.0) * rb.abs() * Aq[:, None]) * Pk.abs() + Pq.abs() * (kb.abs() + (n + 4.0) * rb.abs() * Ak[:, None])).sum(1)
        b_cl = b_cl + (n + 1.0 + nb) * (qb * kb).abs().sum(1) + (rej * (3.0 * n + 4.0 + nb)) * (2.0 + rr) * Aq * Ak
    return dict(w_raw=_gate64(w, gate) if gate_raw else w, w=_gate64(w, gate), b_lit=b_lit, b_cl=b_cl, gate=gate)


GATE_EPS = {0: (1.0, 0.0, 0.0), 1: (0.25, 8.0, 0.0), 2: (1.0, 4.0, 0.0), 3: (1.1, 6.0, 2.0)}    # sup|g'|, eps_g, its |w| part


def bound_k7(d, r, arith=None):
    """(bound of w_raw, bound of w), [E, F] fp64, for the arithmetic form the case's kernel uses."""
    arith = htr_arith(d["form"]) if arith is None else arith
    raw = U32 * (r["b_lit"] if arith == "literal" else r["b_cl"])
    sup, eps, eps_w = GATE_EPS[r["gate"]]
    gated = sup * raw + U32 * (eps + eps_w * r["w_raw"].abs()) * r["w"].abs()
    return raw + FLOOR, gated + FLOOR


def _gate32(w, kind):
    return {0: lambda t: t, 1: torch.sigmoid, 2: torch.tanh, 3: torch.nn.functional.silu}[kind](w)


def k7_fp32(d, arith=None):
    """The kernels' arithmetic in fp32 in their own order -> (w_raw, w) fp32: the literal two-rejection form of
    htr_edge_kernel at lmax <= 2, or the closed form, block by block, rows ascending."""
    S, F, mode = d["S"], d["F"], d["mode"]
    arith = htr_arith(d["form"]) if arith is None else arith
    joint, rej, gate = bool(mode & HTR_JOINT), not (mode & HTR_NOREJ), (mode >> 2) & 3
    q, k, r = d["EQ"][d["seg"]], d["EK"][d["src"].long()], d["rl"]
    w = torch.zeros(d["E"], F)
    for lo, hi in _k7_blocks(S, joint):
        z = torch.zeros(d["E"], F)
        pq, pk, ab, rr = z, z, z, torch.zeros(d["E"], 1)
        if arith == "literal":
            for m in range(lo, hi):
                pq, pk = fma32(r[:, m, None], q[:, m], pq), fma32(-r[:, m, None], k[:, m], pk)
            for m in range(lo, hi):
                w = fma32(q[:, m] + pq * (-r[:, m, None]), k[:, m] + pk * r[:, m, None], w)
        else:
            for m in range(lo, hi):
                ab, pq, pk = fma32(q[:, m], k[:, m], ab), fma32(r[:, m, None], q[:, m], pq), fma32(r[:, m, None], k[:, m], pk)
                rr = fma32(r[:, m, None], r[:, m, None], rr)
            w = w + (ab - (pq * pk) * (2.0 - rr) if rej else ab)
    return w, _gate32(w, gate)


# ------------------------------------------------------------------------------------------------ shared, read-only
def worst_ratio(got, ref, bnd, mask=None):
    """max |got - ref| / bound over the elements of `mask` (all by default); a non-finite `got` counts as infinite."""
    err = (got.double() - ref).abs() / bnd
    err = torch.where(torch.isfinite(got.double()), err, torch.full_like(err, math.inf))
    if mask is not None:
        err = err[mask]
    return float(err.max()) if err.numel() else 0.0


@functools.lru_cache(maxsize=8)
def _built_k6(key, kind):
    c = dict(key)
    d = build_k6(c, kind)
    r = ref_k6(d)
    return d, r, bound_k6(d, r)


def built_k6(c, kind):
    """build + reference + bound of a case on a graph, shared (read-only) by the tests that use the same one."""
    return _built_k6(tuple(sorted(c.items())), kind)


@functools.lru_cache(maxsize=8)
def _built_k7(key, kind):
    d = build_k7(dict(key), kind)
    r = ref_k7(d)
    return d, r, bound_k7(d, r)


def built_k7(c, kind):
    return _built_k7(tuple(sorted(c.items())), kind)


NODE_KEYS = ("xbuf", "vbuf", "h_in", "X_in", "EQ", "EK")
EDGE_KEYS = ("tbuf", "a", "cut", "rl")


def relabel(d, perm):
    """The same graph with atom k of the new numbering = atom perm[k] of the old: every target keeps its own edge order,
    `src` is renumbered.  -> (new dict, emap: old edge id of every new edge)."""
    N, rp = d["N"], d["rowptr"].long()
    inv = torch.empty(N, dtype=torch.long)
    inv[perm] = torch.arange(N)
    emap = torch.cat([torch.arange(int(rp[i]), int(rp[i + 1])) for i in perm.tolist()] + [torch.zeros(0, dtype=torch.long)])
    degs = [d["degs"][i] for i in perm.tolist()]
    d2 = dict(d, degs=degs)
    d2["rowptr"] = torch.zeros(N + 1, dtype=torch.int32)
    d2["rowptr"][1:] = torch.tensor(degs, dtype=torch.int64).cumsum(0).to(torch.int32)
    d2["src"] = inv[d["src"].long()[emap]].to(torch.int32).contiguous()
    d2["seg"] = torch.repeat_interleave(torch.arange(N), torch.tensor(degs, dtype=torch.int64))
    for key in NODE_KEYS:
        if d.get(key) is not None:
            d2[key] = d[key][perm].contiguous()
    for key in EDGE_KEYS:
        if d.get(key) is not None:
            d2[key] = d[key][emap].contiguous()
    return d2, emap
