"""CPU: the yardstick of tests/test_hip_gather_forward.py (tests/gather_util.py) proved without a GPU -- the vectorised fp64
reference equals a per-edge, per-row loop; an fp32 restatement in the kernels' own summation order stays inside the bound
on every input set the GPU module launches, no element left out; ten ways a kernel could be subtly wrong leave the bound;
the case table reaches every kernel the two launchers can select."""
import pytest
import torch

from tests import gather_util as U

GRAPHS = ("ragged", "hub")


# ------------------------------------------------------------------------------------------------ naive loops
def _naive_k6(d):
    S, F, H, N = d["S"], d["F"], d["H"], d["N"]
    M, D = S.M, S.D
    per_head = (M * F) // H
    x = d["xbuf"].double()
    v = d["vbuf"].double()
    out = torch.zeros(N, 1 + D, F, dtype=torch.float64)
    for i in range(N):
        best = None
        e0, e1 = int(d["rowptr"][i]), int(d["rowptr"][i + 1])
        for e in range(e0, e1):
            j = int(d["src"][e])
            o = []
            for b in range(M):
                head = (b * F + torch.arange(F)) // per_head
                tf = d["tbuf"][e, F + b * F:F + (b + 1) * F].double()
                o.append(tf * x[j, b * F:(b + 1) * F] * float(d["cut"][e]) + d["a"][e].double()[head] * v[j, b * F:(b + 1) * F])
            msg = [o[0]]
            for m in range(D):
                l = next(l for l in range(1, S.lmax + 1) if m < (l + 1) ** 2 - 1)
                bd = l if S.sd else 1
                bt = 1 + S.ND + (l - 1 if S.st else 0)
                t = float(d["rl"][e, m]) * o[bd]
                if d["X_in"] is not None:
                    t = t + d["X_in"][j, m].double() * o[bt]
                msg.append(t)
            msg = torch.stack(msg)
            if d["aggr"] == "max":
                best = msg if best is None else torch.maximum(best, msg)
            else:
                out[i] += msg
        if d["aggr"] == "max" and best is not None:
            out[i] = best
        if d["aggr"] == "mean" and e1 > e0:
            out[i] /= e1 - e0
        out[i, 0] += d["h_in"][i].double()
        if d["X_in"] is not None:
            out[i, 1:] += d["X_in"][i].double()
    return out


def _naive_k7(d):
    S, F, mode = d["S"], d["F"], d["mode"]
    joint, rej, gate = bool(mode & 1), not (mode & 2), (mode >> 2) & 3
    w = torch.zeros(d["E"], F, dtype=torch.float64)
    for e in range(d["E"]):
        q, k, r = d["EQ"][int(d["seg"][e])].double(), d["EK"][int(d["src"][e])].double(), d["rl"][e].double()
        blocks = [list(range(S.D))] if joint else [list(range(l * l - 1, (l + 1) ** 2 - 1)) for l in range(1, S.lmax + 1)]
        for rows in blocks:
            if rej:
                dq, dk = sum(q[m] * r[m] for m in rows), sum(k[m] * r[m] for m in rows)
            for m in rows:
                pq = q[m] - dq * r[m] if rej else q[m]
                pk = k[m] - dk * r[m] if rej else k[m]
                w[e] += pq * pk
    return w, U._gate64(w, gate)


@pytest.mark.parametrize("c,kind", [(U.k6_case(16, 2, True, True, "def"), "ragged9"),
                                    (U.k6_case(64, 3, False, True, "max"), "ragged9"),
                                    (U.k6_case(32, 5, True, False, "one", flags=U.MEAN), "ragged9"),
                                    (U.k6_case(64, 2, True, True, "def", True, 0), "single"),
                                    (U.k6_case(64, 3, True, True, "def", flags=U.MAX), "ragged9")], ids=lambda v: v if isinstance(v, str) else U.k6_id(v))
def test_k6_reference_equals_a_per_edge_loop(c, kind):
    d = U.build_k6(c, kind)
    r = U.ref_k6(d)
    naive = _naive_k6(d)
    assert float((r["out"] - naive).abs().max()) <= 1e-13 * max(1.0, float(naive.abs().max()))


@pytest.mark.parametrize("c", [U.k7_case(64, 2), U.k7_case(16, 3, U.HTR_JOINT | (1 << 2)), U.k7_case(16, 3, U.HTR_NOREJ | (3 << 2))],
                         ids=U.k7_id)
def test_k7_reference_equals_a_per_edge_loop(c):
    d = U.build_k7(c, "ragged9")
    r = U.ref_k7(d)
    w_raw, w = _naive_k7(d)
    scale = max(1.0, float(w_raw.abs().max()))
    assert float((r["w_raw"] - w_raw).abs().max()) <= 1e-13 * scale and float((r["w"] - w).abs().max()) <= 1e-13 * scale


# ------------------------------------------------------------------------------------------------ fp32 in the kernels' order
def test_k6_fp32_in_kernel_order_is_within_the_bound():
    worst = {}
    for c in U.K6_CASES:
        for kind in GRAPHS:
            d, r, bnd = U.built_k6(c, kind)
            ratio = U.worst_ratio(U.k6_fp32(d), r["out"], bnd)          # every element of h_out and X_out
            assert ratio <= 1.0, (U.k6_id(c), kind, ratio)
            worst[U.k6_form(c)] = max(worst.get(U.k6_form(c), 0.0), ratio)
    for form, ratio in sorted(worst.items()):
        print(f"{form}: fp32 restatement, worst error / bound = {ratio:.3f}")


def test_k7_fp32_in_kernel_order_is_within_the_bound():
    worst = {}
    for c in U.K7_CASES:
        for kind in GRAPHS:
            d, r, (b_raw, b_w) = U.built_k7(c, kind)
            w_raw, w = U.k7_fp32(d)
            ratio = max(U.worst_ratio(w_raw, r["w_raw"], b_raw), U.worst_ratio(w, r["w"], b_w))
            assert ratio <= 1.0, (U.k7_id(c), kind, ratio)
            worst[d["form"]] = max(worst.get(d["form"], 0.0), ratio)
    for form, ratio in sorted(worst.items()):
        print(f"{form}: fp32 restatement, worst error / bound = {ratio:.3f}")


def test_empty_and_tiny_graphs_build_and_meet_the_bound():
    for kind in ("empty", "single", "ragged9"):
        for c in (U.k6_case(64, 2, True, True, "def"), U.k6_case(64, 3, True, True, "def", True), U.k6_case(64, 3, True, True, "def", flags=U.MAX)):
            d, r, bnd = U.built_k6(c, kind)
            assert U.worst_ratio(U.k6_fp32(d), r["out"], bnd) <= 1.0
        d, r, (b_raw, _) = U.built_k7(U.k7_case(64, 3), kind)
        assert U.worst_ratio(U.k7_fp32(d)[0], r["w_raw"], b_raw) <= 1.0


# ------------------------------------------------------------------------------------------------ mutations
def _leaves_k6(c, kind, rows=None, **mut):
    d, r, bnd = U.built_k6(c, kind)
    assert U.worst_ratio(r["out"], r["out"], bnd) == 0.0
    m = U.ref_k6(d, **mut)
    mask = None
    if rows is not None:
        mask = torch.zeros_like(bnd, dtype=torch.bool)
        mask[rows] = True
    return U.worst_ratio(m["out"], r["out"], bnd, mask) > 1.0, d


DEFAULT_L2 = U.k6_case(64, 2, True, True, "def")


def test_mutation_hub_loses_its_last_edge():
    for c in (DEFAULT_L2, U.k6_case(256, 4, True, True, "def"), U.k6_case(1024, 2, True, True, "def"), U.k6_case(16, 4, True, False, "one")):
        d = U.built_k6(c, "hub")[0]
        keep = torch.ones(d["E"], dtype=torch.bool)
        keep[int(d["rowptr"][U.HUB + 1]) - 1] = False
        assert _leaves_k6(c, "hub", rows=U.HUB, keep=keep)[0], U.k6_id(c)


def test_mutation_head_index_with_per_head_rounded_to_a_block():
    for c in (DEFAULT_L2, U.k6_case(64, 4, True, True, "def")):       # M = 5 / 9, H = 8: per_head = 40 / 72
        S = U.Shape(c["lmax"], True, True)
        per_head = (S.M * 64) // c["H"]
        assert per_head % 64
        rounded = 64 * max(1, round(per_head / 64))
        assert _leaves_k6(c, "ragged", hidx=U.head_index(S, 64, c["H"], rounded))[0]


def test_mutation_direction_and_tensor_blocks_swapped_at_degree_2():
    S = U.Shape(2, True, True)
    dblk, tblk = {1: S.dblk(1), 2: S.tblk(2)}, {1: S.tblk(1), 2: S.dblk(2)}
    assert _leaves_k6(DEFAULT_L2, "ragged", dblk=dblk, tblk=tblk)[0]


def test_mutation_degree_3_uses_block_2_with_sep_dir_off():
    for lmax in (3, 4):
        c = U.k6_case(64, lmax, False, True, "def")
        assert _leaves_k6(c, "ragged", dblk={l: (2 if l == 3 else 1) for l in range(1, lmax + 1)})[0]


def test_mutation_rl_column_shifted_inside_degree_3():
    c = U.k6_case(64, 4, True, True, "def")
    col = torch.arange(24)
    col[8:15] += 1
    assert _leaves_k6(c, "ragged", rlcol=col)[0]
    c = U.k6_case(64, 3, True, True, "def", True)
    col = torch.arange(15)
    col[8:15] = 8 + (torch.arange(7) + 1) % 7
    assert _leaves_k6(c, "hub", rlcol=col)[0]


def test_mutation_cut_dropped_on_one_edge():
    d = U.built_k6(DEFAULT_L2, "ragged")[0]
    i = d["degs"].index(64)
    e = next(e for e in range(int(d["rowptr"][i]), int(d["rowptr"][i + 1])) if float(d["cut"][e]) == 0.0)
    cut = d["cut"].clone()
    cut[e] = 1.0
    assert _leaves_k6(DEFAULT_L2, "ragged", rows=i, cut=cut)[0]
    d = U.built_k6(DEFAULT_L2, "hub")[0]
    e = int(d["rowptr"][U.HUB]) + 1
    assert 0.0 < float(d["cut"][e]) < 0.95
    cut = d["cut"].clone()
    cut[e] = 1.0
    assert _leaves_k6(DEFAULT_L2, "hub", rows=U.HUB, cut=cut)[0]


@pytest.mark.parametrize("kind", GRAPHS)
def test_mutations_of_the_htr_weights(kind):
    # r . r taken as 1 at degree 3: both closed forms and the sliced kernel
    for c in (U.k7_case(64, 3), U.k7_case(256, 4), U.k7_case(32, 5)):
        d, r, (b_raw, _) = U.built_k7(c, kind)
        assert U.worst_ratio(U.ref_k7(d, rr_one_l3=True)["w_raw"], r["w_raw"], b_raw) > 1.0, U.k7_id(c)
    # the rejection applied to EQ only
    for c in (U.k7_case(64, 2), U.k7_case(64, 3)):
        d, r, (b_raw, _) = U.built_k7(c, kind)
        assert U.worst_ratio(U.ref_k7(d, rej_q_only=True)["w_raw"], r["w_raw"], b_raw) > 1.0, U.k7_id(c)
    # joint treated as per-degree
    c = U.k7_case(64, 2, U.HTR_JOINT, True)
    d, r, (b_raw, _) = U.built_k7(c, kind)
    assert U.worst_ratio(U.ref_k7(d, mode=0)["w_raw"], r["w_raw"], b_raw) > 1.0
    # w_raw returned gated
    for gate in (1, 2, 3):
        c = U.k7_case(64, 3, U.HTR_NOREJ | (gate << 2), True)
        d, r, (b_raw, b_w) = U.built_k7(c, kind)
        assert U.worst_ratio(U.ref_k7(d, gate_raw=True)["w_raw"], r["w_raw"], b_raw) > 1.0
        assert U.worst_ratio(r["w_raw"], r["w"], b_w) > 1.0          # ... and w returned un-gated


def test_rr_is_not_one_and_zero_on_self_loops():
    d = U.built_k7(U.k7_case(64, 3), "hub")[0]
    rr = (d["rl"][:, 8:15] ** 2).sum(1)
    loops = d["src"].long() == d["seg"]
    assert bool(loops[int(d["rowptr"][U.HUB]) + U.HUB_SELF]) and bool((rr[loops] == 0).all())
    assert float(rr[~loops].min()) < 0.5 and float(rr[~loops].max()) > 4.0


# ------------------------------------------------------------------------------------------------ graphs and coverage
def test_graphs_sit_on_the_slot_tails():
    for F in (16, 32, 64, 256, 512, 1024):
        ns = U.slots(F)
        assert ns == max(1, 256 // (F // 4))
        gr = U.make_graph("ragged", ns)
        assert {0, 1, max(ns - 1, 0), ns, ns + 1, 2 * ns + 1, 63, 64, 65} <= set(gr["degs"])
        degs = gr["degs"]
        assert degs[0] == 0 and degs[-1] == 0 and degs[2] == 0 and degs[1] == 2 * ns + 1 and degs[3] == 65
        assert gr["N"] % 8 and gr["E"] <= 4000 and int(gr["src"].max()) < gr["N"] and gr["src"].dtype == torch.int32
        assert gr["src"].unique().numel() < gr["E"]                      # rows are shared
        hub = U.make_graph("hub", ns)
        assert hub["degs"][U.HUB] == 301 and int(hub["src"][int(hub["rowptr"][U.HUB]) + U.HUB_SELF]) == U.HUB
        assert U.make_graph("single", ns)["N"] == 1 and U.make_graph("ragged9", ns)["N"] == 9
        assert U.make_graph("empty", ns)["E"] == 0 and U.make_graph("empty", ns)["N"] == 5


def test_case_table_reaches_every_kernel_form():
    tf = ("T", "F")
    pairs = [(a, b) for a in tf for b in tf]
    # gn_message_aggregate's switch (csrc/gn_gata.hip): lmax 1 one instantiation, lmax 2..4 the four flag pairs, each with the
    # zero-X_in form; F = 256 instantiations for lmax 1 and the default pair; lmax >= 3 with X_in: degree groups
    want = {f"mono<1,F,F,{x},{fc}>" for x in ("full", "first") for fc in (0, 256)}
    for lmax in (2, 3, 4):
        for a, b in pairs:
            for fc in ((0, 256) if (a, b) == ("T", "T") else (0,)):
                want.add(f"mono<{lmax},{a},{b},first,{fc}>")
                if lmax == 2:
                    want.add(f"mono<2,{a},{b},full,{fc}>")
                elif lmax == 3:
                    want.add(f"group<3,{a},{b},1..2,scalar,{fc}>+group<3,{a},{b},3..3,{fc}>")
                else:
                    want.add(f"group<4,{a},{b},1..2,scalar,{fc}>+group34<4,{a},{b},3..4,{fc}>")
    got = {U.k6_form(c) for c in U.K6_CASES}
    assert {f for f in got if not f.startswith("hl_")} == want
    # gn_highl.hip: hl_msg_fwd_kernel<L, AGGR>, L = 0..8 (a call launches 0..lmax), AGGR = add | mean | max
    hl = set()
    for c in U.K6_CASES:
        if U.k6_form(c).startswith("hl_"):
            assert U.use_highl(c["lmax"], c["flags"])
            hl |= {(L, U.aggr_of(c["flags"])) for L in range(c["lmax"] + 1)}
    assert hl == {(L, ag) for L in range(9) for ag in ("add", "mean", "max")}
    assert {(c["lmax"], U.aggr_of(c["flags"])) for c in U.K6_CASES if c["flags"]} >= {(2, "add"), (4, "add"), (2, "mean"), (5, "mean"), (3, "max")}
    # gn_htr_edge: htr_edge_kernel<1..4, 0 | 256>, htr_edge_general_kernel<1..4> (gn_options.hip), hl_htr_edge_kernel
    want7 = {f"htr_literal<{l},{fc}>" for l in (1, 2) for fc in (0, 256)} | {f"htr_closed<3,{fc}>" for fc in (0, 256)} | {
        f"htr_closed_all<4,{fc}>" for fc in (0, 256)} | {f"htr_general<{l}>" for l in (1, 2, 3, 4)} | {"hl_htr"}
    assert {U.k7_form(c) for c in U.K7_CASES} == want7
    for lmax in (2, 3):
        assert {(c["mode"], c["w_raw"]) for c in U.K7_CASES if c["lmax"] == lmax and c["mode"] and not c["flags"]} == {
            (m, raw) for m in range(1, 16) for raw in (False, True)}
    assert {c["lmax"] for c in U.K7_CASES if U.k7_form(c) == "hl_htr"} == {2, 4, 5, 8}
    # the widths: every slot count, the compile-time width, and H = 1 / straddling / largest
    assert {c["F"] for c in U.K6_CASES} == {16, 32, 64, 256, 512, 1024}
    for c in U.K6_CASES:
        assert U.head_ok(U.Shape(c["lmax"], c["sd"], c["st"]).M, c["F"], c["H"])
    assert any(c["H"] == 1 for c in U.K6_CASES) and any(c["H"] == U.Shape(c["lmax"], c["sd"], c["st"]).M * c["F"] // 4 for c in U.K6_CASES)
    assert any(c["H"] == 8 and c["lmax"] == 2 and c["sd"] and c["st"] for c in U.K6_CASES)            # per_head = 5 F / 8
    assert any(c["H"] == 8 and c["lmax"] == 4 and c["sd"] and c["st"] for c in U.K6_CASES)            # per_head = 9 F / 8


def test_routing_restatement_on_a_few_known_calls():
    assert U.kernel_form("msg", 256, 2) == "mono<2,T,T,full,256>"
    assert U.kernel_form("msg", 256, 2, first=True) == "mono<2,T,T,first,256>"
    assert U.kernel_form("msg", 256, 2, sep_tensor=False) == "mono<2,T,F,full,0>"
    assert U.kernel_form("msg", 128, 4, True, False) == "group<4,T,F,1..2,scalar,0>+group34<4,T,F,3..4,0>"
    assert U.kernel_form("msg", 128, 4, True, False, first=True) == "mono<4,T,F,first,0>"
    assert U.kernel_form("msg", 64, 5) == "hl_msg<5>(add)" and U.kernel_form("msg", 64, 2, aggr="max") == "hl_msg<2>(max)"
    assert U.kernel_form("htr", 256, 2) == "htr_literal<2,256>" and U.kernel_form("htr", 64, 3) == "htr_closed<3,0>"
    assert U.kernel_form("htr", 64, 4) == "htr_closed_all<4,0>" and U.kernel_form("htr", 64, 4, mode=2) == "htr_general<4>"
    assert U.kernel_form("htr", 64, 4, sliced=True, mode=2) == "hl_htr" and U.kernel_form("htr", 64, 6) == "hl_htr"
