"""GPU: gn_message_backward, gn_message_backward_dropout and gn_htr_backward called directly, every kernel form the launchers
can select, against the fp64 restatement and the a-priori per-element bounds of tests/gather_bwd_util.py (proved on the CPU by
tests/test_gather_bwd_host.py).  Each case prints the kernel form it selects and the worst error / bound per output tensor;
the last test prints the worst per form."""
import math

import pytest
import torch

from tests import attn_util as A
from tests import gather_bwd_util as B
from tests import gather_util as U

pytestmark = pytest.mark.gpu

PAD_ROWS = 8                                       # sentinel rows past the last row of every output array
SENTINEL = 12345.678
WORST = {}                                         # kernel form -> {output: worst error / bound seen by this module}
#: whether two routes to the same gradients give the same BITS, per output (measured on MI355X, then pinned: an observation,
#: not a requirement chosen in advance).  Both sides always meet the bound.
SAME_BITS = {
    # ga_parts given / withheld: the single-read kernel and the by-target / by-source pair round alike, output for output
    "merged_vs_pair": {k: True for k in B.MB_OUTPUTS},
    # the degree-sliced kernels against the tuned ones: the per-source sums agree; the head sums are staged in another order
    # (g_s and what reads it), g_rl leaves another butterfly; HTR: the tuned kernels factor gw out of the per-row terms
    "sliced_vs_tuned": {"g_tf": True, "g_pta": False, "g_rl": False, "g_s": False, "g_q": False, "g_k": False, "g_x": True,
                        "g_v": True, "g_X_out": True, "htr:gEQ": False, "htr:gEK": False, "htr:g_rl": False, "htr:g_pre_t": True},
    # the dropout entry with a_soft == a is the plain entry
    "dropout_vs_plain": {k: True for k in B.MB_OUTPUTS},
}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _padded(rows, cols, dev="cuda"):
    """[rows + PAD_ROWS, cols]: NaN inside (a skipped element fails its bound), the sentinel past the end."""
    t = torch.full((rows + PAD_ROWS, cols), SENTINEL, device=dev)
    t[:rows] = math.nan
    return t


def _f32(*ts):
    for t in ts:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())


def _i32(*ts):
    for t in ts:
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch_mb(d, expect_rc=0, null_gX=False, **over):
    """The ONE place message-backward inputs reach the library.  Everything the kernels index with is asserted here, before any
    launch: a wrong argument would be a device fault, not a failing test.  Launches twice (the second into fresh arrays): same
    bits; sentinel rows and pad columns keep their value.  -> dict of CPU tensors.  ``expect_rc`` != 0: a refusal -- returns
    after the ONE call, having checked that nothing was written; ``over`` overrides arguments for those."""
    from gotennet_amd import _lib
    lib = _lib.load()
    c, S, F, H, N, E = d["case"], d["S"], d["F"], d["H"], d["N"], d["E"]
    M, D, MF = S.M, S.D, S.M * d["F"]
    B.check_csc(d)
    _f32(d["xbuf"], d["vbuf"], d["eproj"], d["a"], d["a_soft"], d["qk"], d["X_in"], d["rl"], d["cut"], d["g_h1"], d["g_X1"])
    _i32(d["rowptr"], d["src"], d["tgt_by_src"], d["colptr"], d["perm"], d["outdeg"])
    for ld in (d["ldxv"], d["lde"], d["ldqk"], d["ldn"]):
        assert ld % 4 == 0
    # a row is read at [row * ld, row * ld + width): the last one ends inside its buffer
    assert d["ldxv"] >= MF and (N - 1) * d["ldxv"] + MF <= d["xbuf"].numel() and d["xbuf"].numel() == d["vbuf"].numel()
    assert d["lde"] >= (1 + M) * F and (E == 0 or (E - 1) * d["lde"] + (1 + M) * F <= d["eproj"].numel())
    assert d["ldqk"] >= 2 * F and (N - 1) * d["ldqk"] + 2 * F <= d["qk"].numel() and d["ldn"] >= 2 * F
    assert d["a"].numel() == E * H and d["rl"].numel() == E * D and d["cut"].numel() == E and (d["a_soft"] is None or d["a_soft"].numel() == E * H)
    assert d["g_h1"].numel() == N * F and d["g_X1"].numel() == N * D * F and (d["X_in"] is None or d["X_in"].numel() == N * D * F)
    assert d["outdeg"].numel() == N
    flags = d["lmax_arg"] & ~0xff
    if expect_rc == 0 or not over:
        assert B.bwd_head_ok(F, H) and F in (16, 32, 64, 128, 256, 512, 1024) and (d["lmax_arg"] & 0xff) == S.lmax
        assert d["X_in"] is not None or not (U.use_highl(S.lmax, flags) or F > 256 or c["act"] != A.ACT_SILU)
        assert c["ga"] or (not (flags & U.MAX) and (c["first"] or B.msg_groups(S.lmax, S.sd, S.st, flags, c["act"]) == 1))
    wide = max(1, F // 256)                                                  # partial slices of g_rl / g_cut at F > 256
    Gapi = B.msg_groups(S.lmax, S.sd, S.st, flags, c["act"])                 # what the caller sizes g_cut / ga_parts for
    ncut = max(wide, Gapi)
    ga_len = E * (1 + D) * F if flags & U.MAX else Gapi * E * H
    names = ("xbuf", "vbuf", "eproj", "a", "qk", "rl", "cut", "g_h1", "g_X1", "rowptr", "src", "tgt_by_src", "colptr", "perm")
    dev = {k: d[k].cuda() for k in names}
    X_in = None if d["X_in"] is None else d["X_in"].cuda()
    a_soft = None if d["a_soft"] is None else d["a_soft"].cuda()
    outdeg = d["outdeg"].cuda() if d["use_outdeg"] else None
    st = torch.cuda.current_stream().cuda_stream
    o = lambda key, default: over.get(key, default)
    res = []
    for _ in range(2):
        g_eproj, g_s = _padded(E, d["lde"]), _padded(E, H)
        g_nproj, g_x, g_v = _padded(N, d["ldn"]), _padded(N, d["ldxv"]), _padded(N, d["ldxv"])
        g_X_out = None if null_gX else _padded(N, D * F)
        g_rl, g_cut = _padded(wide * E * D, 1), _padded(ncut * E, 1)
        ga = _padded(ga_len, 1) if (c["ga"] or over.get("force_ga")) and not over.get("no_ga") else None
        args = [dev["xbuf"].data_ptr(), dev["vbuf"].data_ptr(), o("ldxv", d["ldxv"]), dev["eproj"].data_ptr(), o("lde", d["lde"]),
                dev["a"].data_ptr()]
        dropout = d["a_soft"] is not None or over.get("dropout_entry")
        if dropout:
            args.append(_ptr(a_soft))
        args += [dev["qk"].data_ptr(), o("ldqk", d["ldqk"]), None if over.get("null_X") else _ptr(X_in), dev["rl"].data_ptr(),
                 dev["cut"].data_ptr(), _ptr(outdeg), dev["g_h1"].data_ptr(), dev["g_X1"].data_ptr(), dev["rowptr"].data_ptr(),
                 dev["src"].data_ptr(), dev["tgt_by_src"].data_ptr(), dev["colptr"].data_ptr(), dev["perm"].data_ptr(),
                 g_eproj.data_ptr(), g_s.data_ptr(), g_nproj.data_ptr(), o("ldn", d["ldn"]), g_x.data_ptr(), g_v.data_ptr(),
                 dev["g_X1"].data_ptr() if over.get("alias_gX") else _ptr(g_X_out), g_rl.data_ptr(), g_cut.data_ptr(), _ptr(ga), E,
                 N, F, o("H", H), o("lmax_arg", d["lmax_arg"]), int(S.sd), int(S.st), o("act", c["act"]), st]
        rc = (lib.gn_message_backward_dropout if dropout else lib.gn_message_backward)(*args)
        torch.cuda.synchronize()
        assert rc == expect_rc, rc
        outs = dict(g_eproj=g_eproj, g_s=g_s, g_nproj=g_nproj, g_x=g_x, g_v=g_v, g_rl=g_rl, g_cut=g_cut)
        if g_X_out is not None:
            outs["g_X_out"] = g_X_out
        rows = dict(g_eproj=E, g_s=E, g_nproj=N, g_x=N, g_v=N, g_X_out=N, g_rl=wide * E * D, g_cut=ncut * E)
        for name, t in outs.items():
            assert bool((t[rows[name]:] == SENTINEL).all()), f"{name}: a row past the end was written"
            assert not expect_rc or bool(torch.isnan(t[:rows[name]]).all()), f"{name}: written by a refused call"
        if expect_rc:
            return None
        assert ga is None or bool((ga[ga_len:] == SENTINEL).all())
        for t, width in ((g_nproj, 2 * F), (g_x, MF), (g_v, MF)):
            assert bool(torch.isnan(t[:N, width:]).all()), "a pad column was written"
        res.append({k: t[:rows[k]].cpu() for k, t in outs.items()})
    for k in res[0]:
        assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), f"{k}: two launches differ"
    r = res[0]
    nw = 1 if c["first"] else ncut                                          # the zero-X_in form writes ONE g_cut slice
    out = dict(g_tf=r["g_eproj"][:, F:].reshape(E, M, F), g_pta=r["g_eproj"][:, :F], g_s=r["g_s"], g_q=r["g_nproj"][:, :F],
               g_k=r["g_nproj"][:, F:2 * F], g_x=r["g_x"][:, :MF].reshape(N, M, F), g_v=r["g_v"][:, :MF].reshape(N, M, F),
               g_rl=r["g_rl"].view(wide, E, D).double().sum(0), g_cut=r["g_cut"].view(ncut, E)[:nw].double().sum(0),
               cut_slices=r["g_cut"].view(ncut, E), rl_slices=r["g_rl"].view(wide, E, D))
    if "g_X_out" in r:
        out["g_X_out"] = r["g_X_out"].view(N, D, F)
    return out


def _launch_hb(d, expect_rc=0, **over):
    """The ONE place HTR-backward inputs reach the library; same rules as _launch_mb.  -> dict(gEQ, gEK, g_rl [, g_pre_t])."""
    from gotennet_amd import _lib
    lib = _lib.load()
    c, S, F, N, E = d["case"], d["S"], d["F"], d["N"], d["E"]
    D, mode = S.D, d["mode"]
    direct, gate = bool(mode & B.HTR_DIRECT), (mode >> 2) & 3
    B.check_csc(d)
    _f32(d["g_t_out"], d["pre_t"], d["w"], d["w_raw"], d["EQ"], d["EK"], d["rl"])
    _i32(d["rowptr"], d["src"], d["tgt_by_src"], d["colptr"], d["perm"])
    assert d["EQ"].numel() == N * D * F and d["EK"].numel() == N * D * F and d["rl"].numel() == E * D
    for k in ("g_t_out", "pre_t", "w", "w_raw"):
        assert d[k].numel() == E * F
    if expect_rc == 0:
        assert not over and 0 <= mode <= 31 and F in (16, 32, 64, 128, 256, 512, 1024)
        assert (d["lmax_arg"] & 0xff) == S.lmax and not (d["lmax_arg"] & ~(0xff | U.SLICED))
    wide = max(1, F // 256)
    dev = {k: d[k].cuda() for k in ("EQ", "EK", "rl", "rowptr", "src", "tgt_by_src", "colptr", "perm")}
    for k in ("g_t_out", "pre_t", "w", "w_raw"):                            # (one NaN row past E: never read, and never a NULL pointer at E = 0)
        dev[k] = torch.cat([d[k], torch.full((1, F), math.nan)]).cuda()
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for _ in range(2):
        gEQ, gEK, g_rl = _padded(N, D * F), _padded(N, D * F), _padded(wide * E * D, 1)
        g_pre_t = None if direct else _padded(E, F)
        rc = lib.gn_htr_backward(
            dev["g_t_out"].data_ptr(), None if direct else dev["pre_t"].data_ptr(), None if direct else dev["w"].data_ptr(),
            dev["w_raw"].data_ptr() if (gate and not direct) else None, dev["EQ"].data_ptr(), dev["EK"].data_ptr(), dev["rl"].data_ptr(),
            dev["rowptr"].data_ptr(), dev["src"].data_ptr(), dev["tgt_by_src"].data_ptr(), dev["colptr"].data_ptr(), dev["perm"].data_ptr(),
            N, F, over.get("lmax_arg", d["lmax_arg"]), over.get("mode", mode), gEQ.data_ptr(), gEK.data_ptr(), g_rl.data_ptr(),
            _ptr(g_pre_t), over.get("act", c["act"]), st)
        torch.cuda.synchronize()
        assert rc == expect_rc, rc
        outs = dict(gEQ=gEQ, gEK=gEK, g_rl=g_rl, **({} if direct else {"g_pre_t": g_pre_t}))
        rows = dict(gEQ=N, gEK=N, g_rl=wide * E * D, g_pre_t=E)
        for name, t in outs.items():
            assert bool((t[rows[name]:] == SENTINEL).all()), f"{name}: a row past the end was written"
            assert not expect_rc or bool(torch.isnan(t[:rows[name]]).all()), f"{name}: written by a refused call"
        if expect_rc:
            return None
        res.append({k: t[:rows[k]].cpu() for k, t in outs.items()})
    for k in res[0]:
        assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), f"{k}: two launches differ"
    r = res[0]
    out = dict(gEQ=r["gEQ"].view(N, D, F), gEK=r["gEK"].view(N, D, F), g_rl=r["g_rl"].view(wide, E, D).double().sum(0))
    if not direct:
        out["g_pre_t"] = r["g_pre_t"]
    return out


def _note(form, rs):
    w = WORST.setdefault(form, {})
    for k, v in rs.items():
        w[k] = max(w.get(k, 0.0), v)


def _first_masks(d):
    """The zero-X_in form leaves the tensor-gate columns of g_eproj unwritten: they are not held to the bound."""
    if d["X_in"] is not None:
        return None
    m = torch.ones(d["E"], d["S"].M, d["F"], dtype=torch.bool)
    m[:, 1 + d["S"].ND:] = False
    return {"g_tf": m}


def _mb_ratios(d, ref, out, masks=None):
    fm = _first_masks(d)
    if fm is not None:
        masks = dict(masks or {})
        masks["g_tf"] = fm["g_tf"] if "g_tf" not in masks else (fm["g_tf"] & masks["g_tf"])
    return B.ratios(out, ref, B.MB_OUTPUTS, masks)


def _fmt(rs):
    return " ".join(f"{k}={v:.3f}" for k, v in rs.items())


# ------------------------------------------------------------------------------------------------ error / bound
MB_GROUPS = sorted({(c["F"], c["lmax"]) for c in B.MB_CASES})
HB_GROUPS = sorted({(c["F"], c["lmax"]) for c in B.HB_CASES})


@pytest.mark.parametrize("F,lmax", MB_GROUPS, ids=lambda v: str(v))
def test_message_backward_error_within_bound(F, lmax):
    """Every case of the table at this (F, lmax) on `ragged`, `hub` and their transposes (out-degrees 0, 1, ns - 1, ns, ns + 1,
    2 ns + 1, 63, 64, 65; a source with 301 out-edges, one the self-loop); the first case also at N = 9 and N = 1."""
    for n, c in enumerate([c for c in B.MB_CASES if (c["F"], c["lmax"]) == (F, lmax)]):
        for kind in B.mb_kinds(c, n == 0):
            d, ref = B.built_mb(c, kind)
            rs = _mb_ratios(d, ref, _launch_mb(d))
            print(f"{B.mb_id(c)} {kind}: kernel {d['form']}, E={d['E']}: {_fmt(rs)}")
            assert max(rs.values()) <= 1.0, (B.mb_id(c), kind, rs)
            _note(d["form"], rs)


@pytest.mark.parametrize("F,lmax", HB_GROUPS, ids=lambda v: str(v))
def test_htr_backward_error_within_bound(F, lmax):
    for n, c in enumerate([c for c in B.HB_CASES if (c["F"], c["lmax"]) == (F, lmax)]):
        for kind in B.mb_kinds(c, n == 0):
            d, ref = B.built_hb(c, kind)
            rs = B.ratios(_launch_hb(d), ref, B.HB_OUTPUTS)
            print(f"{B.hb_id(c)} {kind}: kernel {d['form']}, E={d['E']}: {_fmt(rs)}")
            assert max(rs.values()) <= 1.0, (B.hb_id(c), kind, rs)
            _note(d["form"], rs)


# ------------------------------------------------------------------------------------------------ isolated nodes, E = 0
ISOLATED = [B.mb_case(64, 2), B.mb_case(64, 2, ga=False), B.mb_case(64, 3), B.mb_case(256, 4, first=True), B.mb_case(64, 3, H=16),
            B.mb_case(32, 5), B.mb_case(512, 2), B.mb_case(64, 2, flags=U.MEAN)]


@pytest.mark.parametrize("c", ISOLATED, ids=B.mb_id)
def test_message_backward_nodes_without_edges(c):
    """Nodes without in-edges: g_q exactly zero; without out-edges: g_x, g_v, g_k exactly zero and g_X_out = g_X1 bit for bit.
    E = 0, N = 5: the launch still runs and writes the same."""
    from gotennet_amd._lib import GN_ERR_BAD_ARG as BAD
    for kind in ("ragged_T", "ragged", "empty"):
        d = B.build_mb(c, kind)
        if kind == "empty" and not c["first"] and B.msg_groups(c["lmax"], c["sd"], c["st"], c["flags"], c["act"]) > 1 and c["F"] <= 256:
            # E is the stride of the degree groups' slices: E = 0 is refused for the grouped shapes
            _launch_mb(d, expect_rc=BAD)
            continue
        out = _launch_mb(d)
        no_in, no_out = torch.tensor(d["degs"]) == 0, d["outdeg"] == 0
        assert int(no_out.sum()) >= (3 if kind == "ragged_T" else (5 if kind == "empty" else 0))
        assert int(no_in.sum()) >= (3 if kind == "ragged" else (5 if kind == "empty" else 0))
        zero = lambda t: bool((_bits(t) == 0).all())
        assert zero(out["g_q"][no_in])
        assert zero(out["g_x"][no_out]) and zero(out["g_v"][no_out]) and zero(out["g_k"][no_out])
        if "g_X_out" in out and d["X_in"] is not None:
            assert torch.equal(_bits(out["g_X_out"][no_out]), _bits(d["g_X1"][no_out]))


def test_htr_backward_nodes_without_edges():
    for c in (B.hb_case(64, 2), B.hb_case(256, 4), B.hb_case(64, 3, U.HTR_JOINT | 4), B.hb_case(32, 5)):
        for kind in ("ragged_T", "ragged", "empty"):
            d = B.build_hb(c, kind)
            out = _launch_hb(d)
            assert bool((_bits(out["gEQ"][torch.tensor(d["degs"]) == 0]) == 0).all())
            assert bool((_bits(out["gEK"][d["outdeg"] == 0]) == 0).all())


# ------------------------------------------------------------------------------------------------ the zero-X_in form
@pytest.mark.parametrize("F,lmax,sd,st,ga", [(64, 1, True, True, True), (64, 2, True, True, False), (64, 3, True, True, True),
                                             (64, 3, True, True, False), (64, 4, True, True, True), (64, 4, False, True, False),
                                             (256, 4, True, True, True), (16, 3, True, False, True)])
def test_zero_x_in_form_keeps_its_promises(F, lmax, sd, st, ga):
    """X_in = NULL with NaN in the tensor-gate blocks of eproj / x / v: finite outputs; the tensor-gate columns of g_eproj keep
    their pre-launch fill; those blocks of g_x / g_v are exactly zero; g_X_out may be NULL; ONE g_cut slice is written; and
    against a general-form call with a zero X_in tensor ("same gradients, summation order aside") both meet the bound."""
    c = B.mb_case(F, lmax, sd, st, 8 if F >= 64 else 4, first=True, ga=ga)
    for kind in ("ragged", "hub_T"):
        d, ref = B.built_mb(c, kind)
        S, lo = d["S"], (1 + d["S"].ND) * F
        assert bool(torch.isnan(d["xbuf"][:, lo:]).all()) and bool(torch.isnan(d["eproj"][:, F + lo:]).all())
        out = _launch_mb(d, null_gX=True)
        tg = slice(1 + S.ND, S.M)
        assert bool(torch.isnan(out["g_tf"][:, tg]).all())                  # not written
        for k in ("g_pta", "g_s", "g_q", "g_k", "g_x", "g_v", "g_rl", "g_cut"):
            assert bool(torch.isfinite(out[k]).all()), k
        assert bool(torch.isfinite(out["g_tf"][:, :1 + S.ND]).all())
        assert bool((_bits(out["g_x"][:, tg]) == 0).all()) and bool((_bits(out["g_v"][:, tg]) == 0).all())
        assert bool(torch.isnan(out["cut_slices"][1:]).all()) and out["cut_slices"].shape[0] == B.msg_groups(lmax, sd, st)
        rs = _mb_ratios(d, ref, out)
        assert max(rs.values()) <= 1.0, rs
        # the general form on a zero X_in tensor and finite tensor-gate blocks
        g = torch.Generator().manual_seed(3)
        c0 = dict(c, first=False, ga=True)
        d0 = dict(d, case=c0, X_in=torch.zeros(d["N"], S.D, F), G=B.msg_groups(lmax, sd, st), form=B.mb_form(c0))
        for key, col in (("xbuf", lo), ("vbuf", lo), ("eproj", F + lo)):
            d0[key] = d[key].clone()
            d0[key][:, col:col + S.NT * F] = torch.randn(d[key].shape[0], S.NT * F, generator=g)
        out0 = _launch_mb(d0)
        rs0 = _mb_ratios(d0, B.ref_mb(d0), out0)
        assert max(rs0.values()) <= 1.0, rs0
        for k in ("g_pta", "g_s", "g_q", "g_k", "g_rl"):                    # ... and the two agree within the sum of the bounds
            assert bool(((out[k].double() - out0[k].double()).abs() <= 2.0 * ref["b:" + k]).all()), k


# ------------------------------------------------------------------------------------------------ two routes, same gradients
def _same(x, y, names):
    return {k: torch.equal(_bits(x[k]), _bits(y[k])) for k in names if k in x and k in y}


def _pin(key, same):
    print(f"same bits [{key}]: {same}")
    assert same == SAME_BITS[key], (key, same)


def test_merged_against_pair():
    """ga_parts given (the single-read kernel, then attention backward and g_k) and withheld (the by-target / by-source pair)."""
    agg = {}
    for c in (B.mb_case(64, 2), B.mb_case(256, 2), B.mb_case(64, 3, False, True), B.mb_case(64, 4, first=True), B.mb_case(64, 1)):
        for kind in ("ragged", "hub_T"):
            d, ref = B.built_mb(c, kind)
            cp = dict(c, ga=False)
            dp = dict(d, case=cp, form=B.mb_form(cp))
            x, y = _launch_mb(d), _launch_mb(dp)
            rx, ry = _mb_ratios(d, ref, x), _mb_ratios(dp, ref, y)
            assert max(rx.values()) <= 1.0 and max(ry.values()) <= 1.0, (B.mb_id(c), kind, rx, ry)
            for k, v in _same(x, y, B.MB_OUTPUTS).items():
                agg[k] = agg.get(k, True) and v
    _pin("merged_vs_pair", agg)


def test_sliced_against_tuned():
    agg = {}
    for c in (B.mb_case(64, 2), B.mb_case(64, 2, ga=False), B.mb_case(64, 4), B.mb_case(64, 3, True, False), B.mb_case(256, 3)):
        for kind in ("ragged", "hub_T"):
            d, ref = B.built_mb(c, kind)
            cs = dict(c, flags=U.SLICED)
            ds = dict(d, case=cs, form=B.mb_form(cs), lmax_arg=c["lmax"] | U.SLICED)
            x, y = _launch_mb(d), _launch_mb(ds)
            rx, ry = _mb_ratios(d, ref, x), _mb_ratios(ds, ref, y)
            assert max(rx.values()) <= 1.0 and max(ry.values()) <= 1.0, (B.mb_id(c), kind, rx, ry)
            for k, v in _same(x, y, [n for n in B.MB_OUTPUTS if n != "g_cut"]).items():     # (the groups deliver g_cut in G slices)
                agg[k] = agg.get(k, True) and v
    hagg = {}
    for c in (B.hb_case(64, 2), B.hb_case(256, 4), B.hb_case(64, 3, U.HTR_JOINT | 4)):
        for kind in ("ragged", "hub_T"):
            d, ref = B.built_hb(c, kind)
            cs = dict(c, flags=U.SLICED)
            ds = dict(d, case=cs, form=B.hb_form(cs), lmax_arg=c["lmax"] | U.SLICED)
            x, y = _launch_hb(d), _launch_hb(ds)
            assert max(B.ratios(x, ref, B.HB_OUTPUTS).values()) <= 1.0 and max(B.ratios(y, ref, B.HB_OUTPUTS).values()) <= 1.0
            for k, v in _same(x, y, B.HB_OUTPUTS).items():
                hagg[k] = hagg.get(k, True) and v
    _pin("sliced_vs_tuned", dict(agg, **{"htr:" + k: v for k, v in hagg.items()}))


def test_dropout_entry_with_undropped_weights_against_the_plain_entry():
    agg = {}
    for c in (B.mb_case(64, 2, outdeg=True), B.mb_case(64, 3), B.mb_case(64, 2, flags=U.SLICED)):
        for kind in ("ragged", "hub_T"):
            d, ref = B.built_mb(c, kind)
            dd = dict(d, a_soft=d["a"])
            x, y = _launch_mb(d), _launch_mb(dd)
            assert max(_mb_ratios(d, ref, x).values()) <= 1.0 and max(_mb_ratios(dd, ref, y).values()) <= 1.0
            for k, v in _same(x, y, B.MB_OUTPUTS).items():
                agg[k] = agg.get(k, True) and v
    _pin("dropout_vs_plain", agg)


# ------------------------------------------------------------------------------------------------ relabelling
def _perm(N):
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    assert not torch.equal(perm, torch.arange(N))
    return perm


NODE_OUT, EDGE_OUT = ("g_q", "g_k", "g_x", "g_v", "g_X_out", "gEQ", "gEK"), ("g_tf", "g_pta", "g_s", "g_rl", "g_cut", "g_pre_t")


@pytest.mark.parametrize("c", [B.mb_case(64, 2), B.mb_case(64, 2, ga=False), B.mb_case(256, 4), B.mb_case(64, 3, first=True),
                               B.mb_case(32, 5, flags=U.MEAN), B.mb_case(64, 3, flags=U.MAX)], ids=B.mb_id)
def test_message_backward_relabelled_atoms(c):
    """Another numbering of the atoms (every target keeps its own edge order; the by-source order follows the stable sort):
    node-sized outputs are permuted bit for bit, edge-sized ones follow the edge map."""
    for kind in ("ragged", "hub_T"):
        d, ref = B.built_mb(c, kind)
        perm = _perm(d["N"])
        d2, emap = B.relabel_bwd(d, perm)
        x, y = _launch_mb(d), _launch_mb(d2)
        for k in NODE_OUT:
            if k in x:
                assert torch.equal(_bits(y[k]), _bits(x[k][perm])), (B.mb_id(c), kind, k)
        for k in EDGE_OUT:
            if k in x:
                assert torch.equal(_bits(y[k]), _bits(x[k][emap])), (B.mb_id(c), kind, k)


@pytest.mark.parametrize("c", [B.hb_case(64, 2), B.hb_case(256, 4), B.hb_case(64, 3, U.HTR_JOINT | 8), B.hb_case(32, 8)], ids=B.hb_id)
def test_htr_backward_relabelled_atoms(c):
    for kind in ("ragged", "hub_T"):
        d, ref = B.built_hb(c, kind)
        perm = _perm(d["N"])
        d2, emap = B.relabel_bwd(d, perm)
        x, y = _launch_hb(d), _launch_hb(d2)
        for k in NODE_OUT:
            if k in x:
                assert torch.equal(_bits(y[k]), _bits(x[k][perm])), (B.hb_id(c), kind, k)
        for k in EDGE_OUT:
            if k in x:
                assert torch.equal(_bits(y[k]), _bits(x[k][emap])), (B.hb_id(c), kind, k)


# ------------------------------------------------------------------------------------------------ confinement
@pytest.mark.parametrize("c", [B.mb_case(64, 2), B.mb_case(64, 2, ga=False), B.mb_case(64, 3), B.mb_case(256, 4, True, True),
                               B.mb_case(64, 3, True, False), B.mb_case(32, 5)], ids=B.mb_id)
def test_message_backward_nan_stays_where_it_belongs(c):
    """One NaN in g_X1[i, m, ch]: exactly the outputs the restatement says depend on it are non-finite (the mask is the fp64
    restatement run on the same NaN, not written by hand); everything else still meets the bound."""
    d, ref = B.built_mb(c, "ragged")
    i, m, ch = d["degs"].index(64), d["S"].D - 2, d["F"] // 2 + 1
    gX = d["g_X1"].clone()
    gX[i, m, ch] = math.nan
    dn = dict(d, g_X1=gX)
    want = B.ref_mb(dn)
    out = _launch_mb(dn)
    masks = {}
    for k in B.MB_OUTPUTS:
        bad = ~torch.isfinite(want[k])
        got_bad = ~torch.isfinite(out[k])
        assert torch.equal(got_bad, bad), (B.mb_id(c), k, int(got_bad.sum()), int(bad.sum()))
        masks[k] = ~bad
    assert sum(int((~mk).sum()) for mk in masks.values()) > 0
    e = int(d["rowptr"][i])
    assert not bool(torch.isfinite(out["g_rl"][e, m])) and bool(torch.isfinite(out["g_rl"][e, m - 1]))
    rs = _mb_ratios(d, ref, out, masks)
    assert max(rs.values()) <= 1.0, rs


@pytest.mark.parametrize("c", [B.hb_case(64, 2), B.hb_case(256, 4), B.hb_case(64, 3, U.HTR_JOINT | 4), B.hb_case(32, 5)], ids=B.hb_id)
def test_htr_backward_nan_stays_where_it_belongs(c):
    d, ref = B.built_hb(c, "ragged")
    e, ch = int(d["rowptr"][d["degs"].index(64)]) + 5, d["F"] // 2 + 1
    gt = d["g_t_out"].clone()
    gt[e, ch] = math.nan
    dn = dict(d, g_t_out=gt)
    want, out = B.ref_hb(dn), _launch_hb(dn)
    masks = {}
    for k in B.HB_OUTPUTS:
        bad = ~torch.isfinite(want[k])
        assert bool(bad.any()) and torch.equal(~torch.isfinite(out[k]), bad), (B.hb_id(c), k)
        masks[k] = ~bad
    assert max(B.ratios(out, ref, B.HB_OUTPUTS, masks).values()) <= 1.0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_before_any_launch():
    from gotennet_amd._lib import GN_ERR_BAD_ARG as BAD
    d = B.build_mb(B.mb_case(64, 2), "ragged9")
    _launch_mb(d, expect_rc=BAD, alias_gX=True)                             # g_X_out == g_X1
    for ld in ("ldxv", "lde", "ldqk", "ldn"):
        _launch_mb(d, expect_rc=BAD, **{ld: d[ld] + 2})                     # rows not 16-byte aligned
    _launch_mb(d, expect_rc=BAD, H=3)                                       # not a power of two
    _launch_mb(d, expect_rc=BAD, H=32)                                      # (F / 4) % H != 0
    _launch_mb(d, expect_rc=BAD, lmax_arg=0)
    _launch_mb(d, expect_rc=BAD, lmax_arg=9)
    _launch_mb(d, expect_rc=BAD, lmax_arg=2 | 0x800)                        # a stray bit
    _launch_mb(d, expect_rc=BAD, lmax_arg=2 | U.MEAN | U.MAX)
    _launch_mb(d, expect_rc=BAD, lmax_arg=2 | U.MAX, no_ga=True)            # max without its workspace
    _launch_mb(d, expect_rc=BAD, lmax_arg=2 | U.MAX, null_X=True)           # ... without X_in
    _launch_mb(d, expect_rc=BAD, lmax_arg=2 | U.SLICED, null_X=True)        # the zero-X_in form: register-tiled SiLU kernels only
    _launch_mb(d, expect_rc=BAD, act=A.ACT_TANH, null_X=True)
    _launch_mb(d, expect_rc=BAD, act=12)
    _launch_mb(d, expect_rc=BAD, dropout_entry=True)                        # the dropout entry with NULL a_soft
    d5 = B.build_mb(B.mb_case(512, 2), "ragged9")
    _launch_mb(d5, expect_rc=BAD, null_X=True)                              # zero-X_in at F = 512
    d3 = B.build_mb(B.mb_case(64, 3), "ragged9")
    _launch_mb(d3, expect_rc=BAD, no_ga=True)                               # the degree groups without ga_parts
    h = B.build_hb(B.hb_case(64, 2), "ragged9")
    _launch_hb(h, expect_rc=BAD, mode=32)
    _launch_hb(h, expect_rc=BAD, act=12)
    _launch_hb(h, expect_rc=BAD, act=-1)
    _launch_hb(h, expect_rc=BAD, lmax_arg=0)
    _launch_hb(h, expect_rc=BAD, lmax_arg=9)
    _launch_hb(h, expect_rc=BAD, lmax_arg=2 | U.MEAN)                       # a stray bit in lmax


# ------------------------------------------------------------------------------------------------ the table
def test_worst_ratio_per_kernel_form():
    """Runs last: the worst error / bound of every kernel form and output over this module's cases (DESIGN section 2 quotes it).
    Run on its own it launches one case per form that the session has not seen yet."""
    for c in B.MB_CASES:
        if B.mb_form(c) not in WORST:
            d, ref = B.built_mb(c, "ragged")
            _note(d["form"], _mb_ratios(d, ref, _launch_mb(d)))
    for c in B.HB_CASES:
        if B.hb_form(c) not in WORST:
            d, ref = B.built_hb(c, "ragged")
            _note(d["form"], B.ratios(_launch_hb(d), ref, B.HB_OUTPUTS))
    for form, rs in sorted(WORST.items()):
        print(f"== {form}: {_fmt(rs)}")
    for title, fam in (("message", [rs for rs in WORST.values() if "g_tf" in rs]), ("HTR", [rs for rs in WORST.values() if "gEQ" in rs])):
        names = sorted({k for rs in fam for k in rs})
        print(f"== smallest worst ratio per output, {title}: " + " ".join(f"{k}={min(rs[k] for rs in fam if k in rs):.3f}" for k in names))
    assert max(max(rs.values()) for rs in WORST.values()) <= 1.0
    assert set(WORST) == {B.mb_form(c) for c in B.MB_CASES} | {B.hb_form(c) for c in B.HB_CASES}
