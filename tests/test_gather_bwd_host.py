"""CPU: the yardstick of tests/gather_bwd_util.py proved before any kernel is held to it.  The explicit fp64 restatements
of the message and HTR backward equal torch's fp64 autograd of the forward restatements (gather_util.ref_k6 composed with the
fp64 softmax of attn_util; gather_util.ref_k7); an fp32 emulation in the kernels' operation order stays within the a-priori
bound for every case and graph; the mutations a meaningful bound must reject are rejected; the transposed graphs put the
out-degrees on the slot tails; the case table reaches every form the routing can return."""
import math

import pytest
import torch

from tests import attn_util as A
from tests import gather_bwd_util as B
from tests import gather_util as U

#: restatement against autograd: the a-priori bound with u = 2^-53 in place of 2^-24 (the same counted constants on the same
#: un-cancelled magnitudes), times 8: autograd adds a node's terms one after the other (up to 301 roundings on the hub, against the
#: ceil(deg / ns) + ns + 1 the bound counts) and differentiates the soft-max through its maximum and its + 1e-16
#: (+ 2^-149: where a saturated gate leaves values below 1e-50 the subtraction of the bound's 2^-126 floor is not exact)
AUTOGRAD_SLACK = 8.0 * 2.0 ** -29


def _close64(got, ref, bnd):
    return float(((got - ref).abs() / ((bnd - U.FLOOR).clamp_min(0.0) * AUTOGRAD_SLACK + 2.0 ** -149)).max()) if ref.numel() else 0.0


# ------------------------------------------------------------------------------------------------ graphs
@pytest.mark.parametrize("ns", [1, 4, 16, 64])
def test_transposed_graphs_put_out_degrees_on_the_slot_tails(ns):
    for kind in ("ragged", "hub"):
        gr = U.make_graph(kind, ns)
        gt, emap = B.transpose(gr)
        assert torch.equal(torch.sort(emap)[0], torch.arange(gr["E"]))
        gt.update(B.csc_view(gt))
        B.check_csc(gt)
        out = gt["outdeg"].tolist()
        assert out == gr["degs"]                                           # the in-degrees became the out-degrees
        assert B.promised_out_degrees(kind + "_T", ns) <= set(out)
        assert {0, 1, ns, ns + 1} <= set(out) or kind == "hub"
        # the same edge set
        pairs = sorted(zip(gr["src"].tolist(), gr["seg"].tolist()))
        assert pairs == sorted(zip(gt["seg"].tolist(), gt["src"].tolist()))
    gt, _ = B.transpose(U.make_graph("hub", ns))
    gt.update(B.csc_view(gt))
    assert int(gt["outdeg"][U.HUB]) == 301 and max(gt["outdeg"].tolist()) > 256
    col = gt["perm"][int(gt["colptr"][U.HUB]):int(gt["colptr"][U.HUB + 1])].long()
    assert int((gt["seg"][col] == U.HUB).sum()) >= 1                       # one of the hub's out-edges is the self-loop


def test_csc_invariants_are_checked():
    d = B.build_mb(B.mb_case(64, 2), "ragged_T")
    B.check_csc(d)
    bad = dict(d, perm=d["perm"].flip(0).contiguous())
    with pytest.raises(AssertionError):
        B.check_csc(bad)
    bad = dict(d, tgt_by_src=d["tgt_by_src"].roll(1))
    with pytest.raises(AssertionError):
        B.check_csc(bad)


# ------------------------------------------------------------------------------------------------ restatement = autograd
AUTO_MB = [B.mb_case(16, 2, True, True, 2, outdeg=True), B.mb_case(16, 3, False, True, 4), B.mb_case(16, 2, True, False, 1, first=True),
           B.mb_case(16, 2, True, True, 4, flags=U.MEAN, outdeg=True), B.mb_case(16, 3, True, True, 2, flags=U.MAX),
           B.mb_case(16, 2, True, True, 4, drop=True, outdeg=True), B.mb_case(16, 2, True, True, 4, act=A.ACT_TANH)]


def _autograd_mb(d):
    """fp64 autograd of ref_k6 o softmax on the inputs of `d` -> (dict of gradients, d with a / a_soft = the exact softmax)."""
    S, F, H, N, E = d["S"], d["F"], d["H"], d["N"], d["E"]
    leaf = lambda t: t.double().clone().requires_grad_(True)
    L = {k: leaf(d[k]) for k in ("xbuf", "vbuf", "tbuf", "cut", "rl", "h_in")}
    q, k, t = leaf(d["qk"][:, :F]), leaf(d["qk"][:, F:2 * F]), leaf(d["eproj"][:, :F])
    X_in = None if d["X_in"] is None else leaf(d["X_in"])
    att = A.reference(dict(F=F, H=H, N=N, E=E, act=d["case"]["act"], degs=d["degs"], src=d["src"], q=q, k=k, t=t,
                           outdeg=d["outdeg"] if d["use_outdeg"] else None))
    mask = None
    if d["a_soft"] is not None:
        mask = torch.where(d["a"] != 0, torch.full((), 1.5, dtype=torch.float64), torch.zeros((), dtype=torch.float64))
    a = att["a"] if mask is None else att["a"] * mask
    out = U.ref_k6(dict(d, a=a, X_in=X_in, **L))["out"]
    loss = (out[:, 0] * d["g_h1"].double()).sum() + (out[:, 1:] * d["g_X1"].double()).sum()
    wrt = [L["tbuf"], L["xbuf"], L["vbuf"], L["cut"], L["rl"], q, k, t, att["s"]] + ([] if X_in is None else [X_in])
    g = torch.autograd.grad(loss, wrt, allow_unused=True)
    MF = S.M * F
    got = dict(g_tf=g[0][:, F:].reshape(E, S.M, F), g_x=g[1][:, :MF].reshape(N, S.M, F), g_v=g[2][:, :MF].reshape(N, S.M, F),
               g_cut=g[3], g_rl=g[4], g_q=g[5], g_k=g[6], g_pta=g[7], g_s=g[8])
    if X_in is not None:
        got["g_X_out"] = g[9]
    d2 = dict(d, a=a.detach(), a_soft=None if mask is None else att["a"].detach())
    return got, d2


@pytest.mark.parametrize("c", AUTO_MB, ids=B.mb_id)
def test_message_backward_restatement_equals_autograd(c):
    for kind in B.KINDS:
        if kind == "empty":
            continue
        d = B.build_mb(c, kind)
        for key in ("xbuf", "vbuf", "tbuf", "eproj", "qk"):                # autograd multiplies the unread NaN columns by zero
            d[key] = torch.nan_to_num(d[key], nan=0.25)
        got, d2 = _autograd_mb(d)
        ref = B.ref_mb(d2, route32=False)
        for name, gv in got.items():
            assert _close64(gv, ref[name], ref["b:" + name]) <= 1.0, (B.mb_id(c), kind, name)
        assert kind != "hub" or int((d["src"].long() == d["seg"]).sum()) >= 1          # the self-loop was among them


AUTO_HB = [B.hb_case(16, 2), B.hb_case(16, 3, U.HTR_JOINT | (1 << 2)), B.hb_case(16, 2, U.HTR_NOREJ | (2 << 2)), B.hb_case(16, 4, 3 << 2),
           B.hb_case(16, 2, B.HTR_DIRECT), B.hb_case(16, 3, act=A.ACT_TANH)]


@pytest.mark.parametrize("c", AUTO_HB, ids=B.hb_id)
def test_htr_backward_restatement_equals_autograd(c):
    for kind in B.KINDS:
        if kind == "empty":
            continue
        d = B.build_hb(c, kind)
        leaf = lambda t: t.double().clone().requires_grad_(True)
        EQ, EK, rl, pt = leaf(d["EQ"]), leaf(d["EK"]), leaf(d["rl"]), leaf(d["pre_t"])
        fw = U.ref_k7(dict(d, EQ=EQ, EK=EK, rl=rl), mode=c["mode"] & 15)
        direct = bool(c["mode"] & B.HTR_DIRECT)
        # DIRECT: g_t_out is dL/dw of the UNGATED sum; otherwise t' = act(pre_t) gate(w_raw)
        out = fw["w_raw"] if direct else B._act64(pt, c["act"])[0] * fw["w"]
        g = torch.autograd.grad((out * d["g_t_out"].double()).sum(), [EQ, EK, rl] + ([] if direct else [pt]), allow_unused=True)
        g = [torch.zeros_like(t) if gv is None else gv for gv, t in zip(g, (EQ, EK, rl, pt))]       # (norej: w does not read rl)
        d2 = dict(d, w=fw["w"].detach(), w_raw=fw["w_raw"].detach())
        ref = B.ref_hb(d2)
        got = dict(gEQ=g[0], gEK=g[1], g_rl=g[2], **({} if direct else {"g_pre_t": g[3]}))
        assert ("g_pre_t" in ref) == (not direct)
        for name, gv in got.items():
            assert _close64(gv, ref[name], ref["b:" + name]) <= 1.0, (B.hb_id(c), kind, name)


# ------------------------------------------------------------------------------------------------ fp32 emulation within the bound
MB_GROUPS = sorted({(c["F"], c["lmax"]) for c in B.MB_CASES})
HB_GROUPS = sorted({(c["F"], c["lmax"]) for c in B.HB_CASES})


@pytest.mark.parametrize("F,lmax", MB_GROUPS, ids=lambda v: str(v))
def test_message_backward_fp32_emulation_within_bound(F, lmax):
    """The proof that the constants were counted: the kernels' arithmetic, emulated in fp32 in their order, meets the bound."""
    seen = set()
    for c in [c for c in B.MB_CASES if (c["F"], c["lmax"]) == (F, lmax)]:
        key = tuple(sorted(dict(c, ga=True).items()))                      # (merged and pair: one emulation, one bound)
        if key in seen:
            continue
        seen.add(key)
        assert B.mb_form(c).startswith("groups") == (B.msg_groups(c["lmax"], c["sd"], c["st"], c["flags"], c["act"]) > 1
                                                     and not c["first"] and c["H"] <= 8 and c["F"] <= 256)
        for kind in B.mb_kinds(c):
            d, ref = B.built_mb(c, kind)
            rs = B.ratios(B.mb_fp32(d), ref, B.MB_OUTPUTS)
            assert max(rs.values()) <= 1.0, (B.mb_id(c), kind, rs)
            assert max(rs.values()) > 1e-3, (B.mb_id(c), kind, rs)         # ... and the bound is not vacuous


@pytest.mark.parametrize("F,lmax", HB_GROUPS, ids=lambda v: str(v))
def test_htr_backward_fp32_emulation_within_bound(F, lmax):
    for c in [c for c in B.HB_CASES if (c["F"], c["lmax"]) == (F, lmax)]:
        for kind in B.mb_kinds(c):
            d, ref = B.built_hb(c, kind)
            order = "tuned" if d["form"].startswith("htr_tgt") else "general"       # the register-tiled kernels factor gw out
            rs = B.ratios(B.hb_fp32(d, order), ref, B.HB_OUTPUTS)
            assert max(rs.values()) <= 1.0, (B.hb_id(c), kind, rs)
            assert max(rs.values()) > 1e-3, (B.hb_id(c), kind, rs)


# ------------------------------------------------------------------------------------------------ mutations
def _rejected(ref, mut, names):
    return {n: U.worst_ratio(mut[n], ref[n], ref["b:" + n]) for n in names if n in ref}


MUTATIONS = [
    ("msg_map_for_scores", B.mb_case(64, 2), "ragged", ("g_q", "g_k", "g_pta")),
    ("score_map_for_msg", B.mb_case(64, 2), "ragged", ("g_s", "g_v", "g_rl")),
    ("swap_blocks", B.mb_case(64, 3), "ragged", ("g_tf", "g_rl", "g_X_out")),
    ("shift_rl", B.mb_case(64, 2, True, False), "ragged", ("g_tf", "g_x")),
    ("drop_cut", B.mb_case(64, 2), "ragged", ("g_tf",)),
    ("hub_loses_edge", B.mb_case(64, 2), "hub_T", ("g_x",)),
    ("soft_is_a", B.mb_case(64, 2, drop=True), "ragged", ("g_s",)),
    ("nrm_of_target", B.mb_case(64, 2, outdeg=True), "ragged_T", ("g_s",)),
    ("self_loop_once", B.mb_case(64, 2), "hub", ("g_X_out",)),
    ("ties_first", B.mb_case(64, 3, flags=U.MAX), "ragged", ("g_tf", "g_rl", "g_cut")),
]


@pytest.mark.parametrize("mut,c,kind,names", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_message_backward_bound_rejects_mutation(mut, c, kind, names):
    d, ref = B.built_mb(c, kind)
    rs = _rejected(ref, B.ref_mb(d, mut=mut), B.MB_OUTPUTS)
    for n in names:
        assert rs[n] > 1.0, (mut, n, rs)


def test_ties_are_planted_and_shared_evenly():
    d, ref = B.built_mb(B.mb_case(64, 3, flags=U.MAX), "ragged_T")
    i = d["degs"].index(max(d["degs"]))
    e0 = int(d["rowptr"][i])
    assert int(d["src"][e0]) == int(d["src"][e0 + 1]) and torch.equal(d["eproj"][e0], d["eproj"][e0 + 1])
    assert torch.equal(ref["g_tf"][e0], ref["g_tf"][e0 + 1])               # the two arg-max edges got the same half


@pytest.mark.parametrize("mut,c,name", [("rr_factor_one", B.hb_case(64, 3), "gEK"), ("act_for_dact", B.hb_case(64, 2), "g_pre_t")],
                         ids=["rr_factor_one", "act_for_dact"])
def test_htr_backward_bound_rejects_mutation(mut, c, name):
    d, ref = B.built_hb(c, "ragged_T")
    rs = _rejected(ref, B.ref_hb(d, mut=mut), B.HB_OUTPUTS)
    assert rs[name] > 1.0, (mut, rs)
    assert all(v == 0.0 for n, v in rs.items() if n != name)              # ... and nothing else moved


# ------------------------------------------------------------------------------------------------ routing
def test_kernel_form_on_calls_read_off_the_launchers():
    kf = B.kernel_form
    assert kf("msg_bwd", 256, 2) == "merged<2,T,T,256>+attn+gk"                       # GN_MSGB_CASE(2, true, true, FC), ga_parts given
    assert kf("msg_bwd", 256, 2, True, False) == "merged<2,T,F,0>+attn+gk"            # GN_MSGB_CASE(2, true, false, 0)
    assert kf("msg_bwd", 256, 2, ga=False) == "pair<2,T,T,0>"                         # msg_bwd_target_kernel<L, SD, ST>: run-time width
    assert kf("msg_bwd", 256, 4, first=True, ga=False) == "pair_first<4,T,T,256>"
    assert kf("msg_bwd", 64, 1, True, False, first=True) == "merged_first<1,F,F,0>+attn+gk"
    assert kf("msg_bwd", 64, 3) == "groups<3,0>+attn+gk" and kf("msg_bwd", 256, 4) == "groups<4,256>+attn+gk"
    assert kf("msg_bwd", 64, 3, H=16) == "hl_msg_bwd(add)"                            # the group kernels carry eight head sums
    assert kf("msg_bwd", 64, 3, first=True, H=16) == "merged_first<3,T,T,0>+attn+gk"
    assert kf("msg_bwd", 64, 3, False, True) == "merged<3,F,T,0>+attn+gk"
    assert kf("msg_bwd", 512, 2) == kf("msg_bwd", 32, 5) == kf("msg_bwd", 64, 2, flags=U.SLICED) == "hl_msg_bwd(add)"
    assert kf("msg_bwd", 64, 2, act=A.ACT_TANH) == "hl_msg_bwd(add)" and kf("msg_bwd", 64, 2, flags=U.MEAN) == "hl_msg_bwd(mean)"
    assert kf("htr_bwd", 64, 2) == "htr_tgt+src<2,0>" and kf("htr_bwd", 256, 3) == "htr_tgt+srcgroup<3,256>"
    assert kf("htr_bwd", 256, 4) == "htr_tgt×2+srcgroup<4,256>" and kf("htr_bwd", 64, 4, mode=B.HTR_DIRECT) == "htr_general<4>"
    assert kf("htr_bwd", 64, 2, act=A.ACT_TANH) == "hl_htr_bwd" and kf("htr_bwd", 64, 2, act=A.ACT_TANH, mode=4) == "htr_general<2>"
    assert kf("htr_bwd", 512, 1) == kf("htr_bwd", 32, 6, mode=3) == kf("htr_bwd", 64, 3, flags=U.SLICED) == "hl_htr_bwd"
    assert B.msg_groups(3, True, True) == 2 and B.msg_groups(4, True, True) == 3 and B.msg_groups(4, True, False) == 1
    assert B.msg_groups(4, True, True, U.SLICED) == 1 and B.msg_groups(3, True, True, act=A.ACT_TANH) == 1


def test_case_table_reaches_every_form():
    forms = set()
    for F in (16, 32, 64, 128, 256, 512, 1024):
        for lmax in range(1, 9):
            for sd in (True, False):
                for st in (True, False):
                    for flags in (0, U.SLICED, U.MEAN, U.MAX):
                        for act in (A.ACT_SILU, A.ACT_TANH):
                            for first in (False, True):
                                for ga in (True, False):
                                    for H in (1, 8, 16):
                                        if not B.bwd_head_ok(F, H):
                                            continue
                                        if first and (lmax > 4 or flags or act != A.ACT_SILU or F > 256):
                                            continue                       # refused
                                        if flags & U.MAX and not ga:
                                            continue                       # refused
                                        if not ga and not first and not flags and act == A.ACT_SILU and F <= 256 and B.msg_groups(lmax, sd, st) > 1:
                                            continue                       # refused: the degree groups need the workspace
                                        forms.add(B.kernel_form("msg_bwd", F, lmax, sd, st, first, ga, H, flags, act))
    assert forms == {B.mb_form(c) for c in B.MB_CASES}
    forms = {B.kernel_form("htr_bwd", F, lmax, flags=fl, act=act, mode=mode) for F in (16, 64, 256, 512) for lmax in range(1, 9)
             for fl in (0, U.SLICED) for act in (A.ACT_SILU, A.ACT_TANH) for mode in (0, 1, 2, 4, 16, 17)}
    assert forms == {B.hb_form(c) for c in B.HB_CASES}
    # the degree-64 target of `ragged` sits on deg * H == GS_CAP and the degree-65 target past it at H = 32
    assert any(c["H"] == 32 and c["F"] == 128 for c in B.MB_CASES) and 64 * 32 == B.GS_CAP
    for c in B.MB_CASES:
        if B.mb_allows_both(c):
            assert dict(c, ga=not c["ga"]) in B.MB_CASES or c["H"] != 8 or c["F"] != 64 or c["drop"] or c["lmax"] == 1, B.mb_id(c)
