"""CPU: the yardstick of tests/norm_util.py proved on the host.  Every closed form equals torch's fp64 forward and autograd, the
fp32 emulation stays inside the a-priori bound on every case (worst ratio printed), the conditions on the inputs hold from the
reference alone, every listed mutation of the emulation is rejected, and the entry points refuse bad arguments before a launch."""
import math

import pytest
import torch

from oracle import gotennet_oracle as orc
from tests import norm_util as U

R = U.ratio
WORST = {}
PTR = 64                                           # a non-NULL address no refused call may touch
LN_IDS = [U.ln_id(n) for n in range(len(U.LN_CASES))]
PG_IDS = [U.pg_case(n)["id"] for n in range(len(U.PG_CASES))]
TN_IDS = [U.tn_id(n) for n in range(len(U.TN_CASES))]
HEAD_IDS = [U.head_id(n) for n in range(len(U.HEAD_CASES))]
CLOSED = 1e-6                                      # closed form against restatement: fp64 rounding, in units of the fp32 bound


def _note(rs):
    for k, v in rs.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= 1.0, (k, v)


def _show(tag, rs):
    print(f"{tag}: " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))


# ------------------------------------------------------------------------------------------------ case tables
def test_tables_hold_every_listed_shape():
    assert {c[0] for c in U.LN_CASES} == set(U.LN_F) == {1, 4, 48, 63, 64, 65, 96, 200, 256, 1024}
    assert {c[1] for c in U.LN_CASES} == set(U.LN_N) == {1, 3, 4, 5, 9} and {c[2] for c in U.LN_CASES} == set(U.KINDS)
    rows = {k for n in range(len(U.LN_CASES)) for k in U.row_kinds(n)}
    assert rows == {"rand", "const0", "const1", "const1000", "mean1e4", "zerograd"}
    for n in range(len(U.LN_CASES)):
        c = U.ln_case(n)
        assert c["eps"] == 1e-5 and (c["F"] < 4 or (bool((c["gamma"] == 0).any()) and bool((c["gamma"] < 0).any())))
    assert {c[0] for c in U.PG_CASES} == set(U.PG_N) == {0, 1, 63, 64, 65, 130}
    assert {c[1] for c in U.PG_CASES} == set(U.PG_C) == {1, 48, 255, 256, 257, 300}
    acts = {c[2] for c in U.PG_CASES}
    assert {U.NONE, U.SILU} < acts and len(acts - {U.NONE, U.SILU}) >= 2 and {c[3] for c in U.PG_CASES} == {True, False}
    assert {c[0] for c in U.TN_CASES} == set(range(1, 9)) and {c[1] for c in U.TN_CASES} == set(U.TN_F) == {1, 4, 63, 64, 65, 200, 256}
    assert {c[2] for c in U.TN_CASES} == set(U.TN_N) == {1, 2, 3, 5} and any((c[0] * c[2]) % 4 for c in U.TN_CASES)
    plans = {k for n in range(len(U.TN_CASES)) for k in U.tn_case(n)["plan"].values()}
    assert plans == set(U.BLOCK_PLAN)
    assert U.tie_channels(256, 3) == [3, 70, 133] and U.tie_channels(65, 2) == [3, 64]       # other lanes, other 64-strides
    assert set(U.GATE_N) == {0, 4, 1020, 1024, 1028, 4100}
    assert {c[0] for c in U.HEAD_CASES} == set(U.HEAD_HD) == {1, 32, 63, 64, 65, 200} and {c[2] for c in U.HEAD_CASES} >= set(U.KINDS)
    assert set(U.MOL_SIZES) == {0, 1, 15, 16, 17, 64, 65, 70}
    assert any(1030 in c[1] and c[0] == 32 for c in U.HEAD_CASES)
    assert {c[3] for c in U.HEAD_CASES} == {True, False} and {c[4] for c in U.HEAD_CASES} == {True, False}
    x = U.sweep_points()
    assert x.numel() % 4 == 0 and x.numel() >= (1 << 16)
    for v in (0.0, U.MIN_NORMAL, 1e-6, 19.99, 20.0, 20.01, 88.0, 100.0, math.inf):
        assert bool((x == U.f32c(v)).any()) and bool((x == -U.f32c(v)).any()), v


def test_tensor_norm_ties_are_exact_and_gaps_wide():
    """In every block the two largest and the two smallest clamped norms are bit-equal or at least 1e-4 apart (relative), in
    fp64 and in the fp32 emulation alike; every tie block really ties."""
    for n in range(len(U.TN_CASES)):
        c = U.tn_case(n)
        assert all(g == 0.0 or g >= 1e-4 for g in U.tn_norm_gaps(c)), c["id"]
        if c["F"] < 4:
            continue
        for (a, l), kind in c["plan"].items():
            cnt, off = 2 * l + 1, l * l - 1
            for dt in (torch.float32, torch.float64):
                s = c["X"][a, off:off + cnt].to(dt).pow(2).sum(0).sqrt().clamp(min=U.f32c(c["eps"]))
                if kind in ("tie_max2", "tie_max3", "tie_both"):
                    assert int((s == s.max()).sum()) == min(3 if kind == "tie_max3" else 2, len(U.tie_channels(c["F"], 3)))
                if kind in ("tie_min2", "tie_min3", "tie_both", "zero_and_tiny"):
                    assert int((s == s.min()).sum()) >= 2
                if kind == "all_equal":
                    assert float(s.max() - s.min()) == 0.0
                if kind == "eps_channel":
                    raw = c["X"][a, off:off + cnt].to(dt).pow(2).sum(0).sqrt()
                    assert float(raw[c["F"] // 2]) == U.f32c(c["eps"])


# ------------------------------------------------------------------------------------------------ activations and gates
@pytest.mark.parametrize("k", U.KINDS, ids=U.ACT_NAMES)
def test_activation_closed_form_emulation_and_bound(k):
    """Over the whole sweep: the closed form and its derivative are torch's fp64 function and autograd; the emulation is inside
    the bound; at +-Inf all three agree on NaN / the signed limit."""
    x = U.sweep_points()
    fin = torch.isfinite(x)
    rv, rd = U.ref_value_and_slope(U.REF_ACT[k], x)
    rs = {}
    for name, tr, ref in (("act", U.act, rv), ("dact", U.dact, rd)):
        b = U.bound_of(tr(U.RE, U.RE.load(x), k)).expand_as(ref)
        f64, f32 = tr(U.F64, U.F64.load(x), k).v.expand_as(ref), tr(U.F32, U.F32.load(x), k).v.expand_as(ref)
        assert R(f64[fin], ref[fin], b[fin]) < CLOSED, name
        assert U.same_class(f64[~fin], ref[~fin]) and U.same_class(f32[~fin], ref[~fin]), name
        rs[f"{U.ACT_NAMES[k]}.{name}"] = R(f32[fin], ref[fin], b[fin])
    _show(U.ACT_NAMES[k], rs)
    _note(rs)


@pytest.mark.parametrize("kind", range(4))
def test_gate_closed_form_emulation_and_bound(kind):
    x = U.sweep_points()
    fin = torch.isfinite(x)
    rv, rd = U.ref_value_and_slope(U.REF_GATE[kind], x)
    rs = {}
    for name, tr, ref in (("gate", U.gate, rv), ("dgate", U.dgate, rd)):
        b = U.bound_of(tr(U.RE, U.RE.load(x), kind)).expand_as(ref)
        f64, f32 = tr(U.F64, U.F64.load(x), kind).v.expand_as(ref), tr(U.F32, U.F32.load(x), kind).v.expand_as(ref)
        assert R(f64[fin], ref[fin], b[fin]) < CLOSED, name
        rs[f"{name}{kind}"] = R(f32[fin], ref[fin], b[fin])
    _show(f"gate {kind}", rs)
    _note(rs)


def test_kinks_on_direct_inputs():
    """relu'(0) = 0, leaky'(0) = 0.01, ELU'(0) = 1, SELU'(0) = lambda alpha; one smallest normal to either side takes the
    side's slope -- torch's autograd and the closed form alike."""
    x = torch.tensor([0.0, U.MIN_NORMAL, -U.MIN_NORMAL])
    want = {U.RELU: (0.0, 1.0, 0.0), U.LEAKY: (0.01, 1.0, 0.01), U.ELU: (1.0, 1.0, 1.0),
            U.SELU: (U.SELU_L * U.SELU_A, U.SELU_L, U.SELU_L * U.SELU_A)}
    for k, w in want.items():
        _, rd = U.ref_value_and_slope(U.REF_ACT[k], x)
        d = U.dact(U.F64, U.F64.load(x), k).v.expand_as(rd)
        assert torch.allclose(rd, torch.tensor(w, dtype=torch.float64), rtol=1e-15, atol=0), k
        assert torch.allclose(d, rd, rtol=1e-15, atol=0), k
    assert all(v in U.SPECIAL for v in (0.0, U.MIN_NORMAL, -U.MIN_NORMAL))
    for n in range(len(U.HEAD_CASES)):
        assert U.head_case(n)["pre1"].view(-1)[:3].tolist() == [0.0, U.MIN_NORMAL, -U.MIN_NORMAL][:U.head_case(n)["pre1"].numel()]


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_outputs(ar, c, mut=None):
    k = c["act"]
    return dict(y=U.ln_forward(ar, c, None, mut).v, ya=U.ln_forward(ar, c, k, mut).v, gx=U.ln_backward(ar, c, None, mut).v,
                gxa=U.ln_backward(ar, c, k, mut).v)


@pytest.mark.parametrize("n", range(len(U.LN_CASES)), ids=LN_IDS)
def test_layernorm_closed_form_emulation_and_conditions(n):
    c, ex = U.ln_case(n), U.ln_expected(n)
    f64, f32 = _ln_outputs(U.F64, c), _ln_outputs(U.F32, c)
    for key in f64:
        assert R(f64[key], *ex[key]) < CLOSED, key
    rs = {f"ln.{key}": R(f32[key], *ex[key]) for key in f32}
    _show(c["id"], rs)
    _note(rs)
    if c["act"] in U.KINKED:                                                 # the side of the kink is certain on every element
        m = U.ln_margin(c, c["act"])
        print(f"{c['id']}: min |v| / bound(v) = {m:.1f}")
        assert m >= U.MARGIN
    for r, kind in enumerate(c["kinds"]):
        if kind == "zerograd":                                               # an all-zero gradient row: exactly zero, in all three
            assert float(ex["gx"][0][r].abs().max()) == 0.0 and float(f32["gx"][r].abs().max()) == 0.0
            assert float(f32["gxa"][r].abs().max()) == 0.0
        if kind.startswith("const"):                                         # a constant row is bounded, not exempt: y = beta
            assert torch.equal(ex["y"][0][r], c["beta"].double()) and bool(torch.isfinite(ex["y"][1][r]).all())


@pytest.mark.parametrize("n", range(len(U.PG_CASES)), ids=PG_IDS)
def test_param_grad_closed_form_and_emulation(n):
    c = U.pg_case(n)
    ref, b = U.pg_reference(c), [U.bound_of(t) for t in U.pg_transcript(U.RE, c)]
    f64, f32 = U.pg_transcript(U.F64, c), U.pg_transcript(U.F32, c)
    for i in range(2):
        assert R(f64[i].v, ref[i], b[i]) < CLOSED
    if c["N"] == 0:
        assert float(f32[0].v.abs().max()) == 0.0 and float(f32[1].v.abs().max()) == 0.0 and float(ref[0].abs().max()) == 0.0
    rs = {"pg.dgamma": R(f32[0].v, ref[0], b[0]), "pg.dbeta": R(f32[1].v, ref[1], b[1])}
    _show(c["id"], rs)
    _note(rs)


# ------------------------------------------------------------------------------------------------ TensorLayerNorm
@pytest.mark.parametrize("n", range(len(U.TN_CASES)), ids=TN_IDS)
def test_tensor_norm_closed_form_emulation_and_routing(n):
    c, ex = U.tn_case(n), U.tn_expected(n)
    y64, (g64, _, _) = U.tn_transcript(U.F64, c), U.tn_transcript(U.F64, c, True)
    y32, (g32, amx, amn) = U.tn_transcript(U.F32, c), U.tn_transcript(U.F32, c, True)
    assert R(y64.v, *ex["Y"]) < CLOSED and R(g64.v, *ex["gX"]) < CLOSED
    assert torch.equal(amx, ex["amx"]) and torch.equal(amn, ex["amn"])       # fp32 and fp64 route to the same channels
    rs = {"tn.Y": R(y32.v, *ex["Y"]), "tn.gX": R(g32.v, *ex["gX"])}
    _show(c["id"], rs)
    _note(rs)
    for (a, l), kind in c["plan"].items():
        off, cnt = l * l - 1, 2 * l + 1
        if kind == "all_equal" or c["F"] == 1:                               # the flat block: delta := 1, output and gradient zero
            for t in (ex["Y"][0], ex["gX"][0], y32.v, g32.v):
                assert float(t[a, off:off + cnt].abs().max()) == 0.0, kind


# ------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("n", range(len(U.HEAD_CASES)), ids=HEAD_IDS)
def test_head_closed_form_and_emulation(n):
    c = U.head_case(n)
    for mean in (0, 1):
        ex = U.head_expected(n, mean)
        f64, f32 = U.head_transcript(U.F64, c, mean), U.head_transcript(U.F32, c, mean)
        for key in ex:
            assert R(f64[key].v.expand_as(ex[key][0]), *ex[key]) < CLOSED, key
        rs = {f"head.{key}": R(f32[key].v.expand_as(ex[key][0]), *ex[key]) for key in ex}
        _show(f"{c['id']} mean={mean}", rs)
        _note(rs)
        empty = [b for b, s in enumerate(c["sizes"]) if s == 0]
        for b in empty:                                                      # the empty molecule: mol_shift alone, under both modes
            assert float(ex["energy"][0][b]) == c["mol_shift"] and float(f32["energy"].v[b]) == c["mol_shift"]


@pytest.mark.parametrize("n", [0, 4, 7])
def test_head_restatement_is_the_oracle(n):
    """atomwise_energy (Atomwise: standardised per atom) and atomwise_v3 (the mean added after the aggregation) with the
    hidden layer an identity: the same numbers as the restatement."""
    c = U.head_case(n)
    Hd, k = c["Hd"], c["act"]
    batch = torch.repeat_interleave(torch.arange(c["n_mol"]), torch.tensor(c["sizes"]))
    head = {"out_net.1.out_net.0.weight": torch.eye(Hd, dtype=torch.float64), "out_net.1.out_net.0.bias": torch.zeros(Hd, dtype=torch.float64),
            "out_net.1.out_net.1.weight": c["W2"].double()[None, :], "out_net.1.out_net.1.bias": torch.tensor([c["b2"]], dtype=torch.float64)}
    if c["use_ref"]:
        head["atomref.weight"] = c["atomref"].double()[:, None]
    name = {"ssp": "softplus", "leaky": "leakyrelu"}.get(U.ACT_NAMES[k], U.ACT_NAMES[k])
    for mean in (0, 1):
        agg = "mean" if mean else "sum"
        std = dict(head, **{"standardize.stddev": torch.tensor(c["scale"], dtype=torch.float64),
                            "standardize.mean": torch.tensor(c["shift"], dtype=torch.float64)})
        e = orc.atomwise_energy(std, c["pre1"].double(), batch, c["n_mol"], name, c["z"].long(), agg)[:, 0]
        ref = U.head_reference(c, mean)
        assert torch.allclose(e + c["mol_shift"], ref["energy"], rtol=1e-13, atol=1e-13)
        e3, _ = orc.atomwise_v3(head, c["pre1"].double(), batch, c["n_mol"], c["mol_shift"], c["scale"], name, c["z"].long(), agg)
        assert torch.allclose(e3[:, 0] + c["shift"] * (1.0 if mean else torch.tensor(c["sizes"], dtype=torch.float64)) * (torch.tensor(c["sizes"]) > 0),
                              ref["energy"], rtol=1e-13, atol=1e-13)


# ------------------------------------------------------------------------------------------------ mutations
def _worst_ln(mut):
    worst = (0.0, "")
    for n in range(len(U.LN_CASES)):
        c, ex = U.ln_case(n), U.ln_expected(n)
        got = _ln_outputs(U.F32, c, mut)
        worst = max(worst, (max(R(got[key], *ex[key]) for key in got), c["id"]))
    return worst


def _worst_pg(mut):
    worst = (0.0, "")
    for n in range(len(U.PG_CASES)):
        c = U.pg_case(n)
        ref, b, got = U.pg_reference(c), U.pg_transcript(U.RE, c), U.pg_transcript(U.F32, c, mut)
        worst = max(worst, (max(R(got[i].v, ref[i], U.bound_of(b[i])) for i in range(2)), c["id"]))
    return worst


def _worst_tn(mut):
    worst = (0.0, "")
    for n in range(len(U.TN_CASES)):
        c, ex = U.tn_case(n), U.tn_expected(n)
        r = max(R(U.tn_transcript(U.F32, c, False, mut).v, *ex["Y"]), R(U.tn_transcript(U.F32, c, True, mut)[0].v, *ex["gX"]))
        worst = max(worst, (r, c["id"]))
    return worst


def _worst_act(mut):
    """Through the edge-gate window with g = wg = 1, as the GPU sweep runs it."""
    x = U.sweep_points()
    x = x[torch.isfinite(x)]
    one = torch.ones_like(x)
    worst = (0.0, "")
    for k in U.KINDS:
        rv, rd = U.ref_value_and_slope(U.REF_ACT[k], x)
        bp, bw = U.edge_gate_bwd(U.RE, one, x, one, k)
        gp, gw = U.edge_gate_bwd(U.F32, one, x, one, k, mut)
        r = max(R(gp.v, rd, U.bound_of(bp)), R(gw.v, rv, U.bound_of(bw)))
        worst = max(worst, (r, U.ACT_NAMES[k]))
    return worst


def _worst_gate(mut):
    x = U.sweep_points()
    x = x[torch.isfinite(x)]
    worst = (0.0, "")
    for kind in range(4):
        rv, rd = U.ref_value_and_slope(U.REF_GATE[kind], x)
        r = max(R(U.gate(U.F32, U.F32.load(x), kind, mut).v, rv, U.bound_of(U.gate(U.RE, U.RE.load(x), kind))),
                R(U.dgate(U.F32, U.F32.load(x), kind, mut).v.expand_as(rd), rd, U.bound_of(U.dgate(U.RE, U.RE.load(x), kind)).expand_as(rd)))
        worst = max(worst, (r, f"kind {kind}"))
    return worst


def _worst_head(mut):
    worst = (0.0, "")
    for n in range(len(U.HEAD_CASES)):
        c = U.head_case(n)
        for mean in (0, 1):
            ex, got = U.head_expected(n, mean), U.head_transcript(U.F32, c, mean, mut)
            r = max(R(got[key].v.expand_as(ex[key][0]), *ex[key]) for key in ex)
            worst = max(worst, (r, f"{c['id']} mean={mean}"))
    return worst


_WORST_OF = dict(ln=_worst_ln, pg=_worst_pg, tn=_worst_tn, act=_worst_act, gate=_worst_gate, head=_worst_head)


@pytest.mark.parametrize("mut", sorted(U.MUTATIONS))
def test_mutation_is_rejected(mut):
    """Each mutated emulation breaches the bound on at least one case of its family."""
    worst, where = _WORST_OF[U.MUTATIONS[mut]](mut)
    print(f"{mut}: worst error / bound {worst:.3g} on {where}")
    assert worst > 1.0, mut


def test_softplus_threshold_is_seen_at_100():
    x = torch.tensor([100.0])
    got = U.act(U.F32, U.F32.load(x), U.SOFTPLUS, "softplus_no_threshold").v
    assert not bool(torch.isfinite(got).all()) and float(U.act(U.F32, U.F32.load(x), U.SOFTPLUS).v) == 100.0


def test_mutation_list_is_complete():
    need = {"ln": 6, "pg": 1, "tn": 6, "act": 7, "gate": 1, "head": 5}
    for fam, cnt in need.items():
        assert sum(1 for v in U.MUTATIONS.values() if v == fam) >= cnt, fam


# ------------------------------------------------------------------------------------------------ ABI refusals (no device needed)
def test_entry_points_refuse_before_any_launch():
    from gotennet_amd import _lib
    lib = _lib.load()
    bad = _lib.GN_ERR_BAD_ARG
    P = PTR
    for N, F in ((-1, 8), (4, 0), (4, -3)):
        assert lib.gn_layernorm(P, P, P, 1e-5, N, F, P, None) == bad
        assert lib.gn_layernorm_backward(P, P, 1e-5, P, N, F, P, None) == bad
        assert lib.gn_layernorm_silu(P, P, P, 1e-5, N, F, P, 0, None) == bad
        assert lib.gn_layernorm_silu_backward(P, P, P, 1e-5, P, N, F, P, 0, None) == bad
        assert lib.gn_layernorm_param_grad(P, P, P, 1e-5, P, N, F, 0, P, P, P, None) == bad
        assert lib.gn_tensor_norm(P, P, 1e-12, N, F, 2, P, None) == bad
        assert lib.gn_tensor_norm_backward(P, P, P, 1e-12, N, F, 2, P, None) == bad
    for act in (-1, 12, 99):
        assert lib.gn_layernorm_silu(P, P, P, 1e-5, 4, 8, P, act, None) == bad
        assert lib.gn_layernorm_silu_backward(P, P, P, 1e-5, P, 4, 8, P, act, None) == bad
        assert lib.gn_layernorm_param_grad(P, P, P, 1e-5, P, 4, 8, act, P, P, P, None) == bad
        assert lib.gn_head_energy(P, P, 0.0, 1.0, 0.0, 0.0, None, P, P, 2, 8, P, P, 0, None, act, None) == bad
        assert lib.gn_head_grad(P, P, 1.0, None, 4, 8, P, act, None) == bad
    for act in (-2, 12):
        assert lib.gn_edge_gate_backward(P, P, act, P, 8, P, P, None) == bad
    for k in U.KINDS:                                                        # an activation needs beta
        if k != U.NONE:
            assert lib.gn_layernorm_param_grad(P, P, None, 1e-5, P, 4, 8, k, P, P, P, None) == bad
    for lmax in (0, -1, 9):
        assert lib.gn_tensor_norm(P, P, 1e-12, 4, 8, lmax, P, None) == bad
        assert lib.gn_tensor_norm_backward(P, P, P, 1e-12, 4, 8, lmax, P, None) == bad
    for kind in (-1, 4):
        assert lib.gn_gate(P, kind, 8, P, None) == bad and lib.gn_gate_backward(P, P, kind, 8, P, None) == bad
    for n in (1, 2, 3, 1023, -4):
        assert lib.gn_gate(P, 1, n, P, None) == bad and lib.gn_gate_backward(P, P, 1, n, P, None) == bad
        assert lib.gn_edge_gate_backward(P, P, 0, P, n, P, P, None) == bad
    for Hd in (0, -1):
        assert lib.gn_head_energy(P, P, 0.0, 1.0, 0.0, 0.0, None, P, P, 2, Hd, P, P, 0, None, 0, None) == bad
        assert lib.gn_head_grad(P, P, 1.0, None, 4, Hd, P, 0, None) == bad
    assert lib.gn_head_energy(P, P, 0.0, 1.0, 0.0, 0.0, None, P, P, -1, 8, P, P, 0, None, 0, None) == bad
    assert lib.gn_head_grad(P, P, 1.0, None, -1, 8, P, 0, None) == bad
    for N in (0, 1, 63, 64, 65, 130, 1000):
        for C in (1, 48, 300):
            assert lib.gn_layernorm_param_grad_workspace(N, C) == U.pg_workspace(N, C) == 2 * ((N + 63) // 64) * C


def test_worst_ratios():
    print("worst emulation / bound: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
