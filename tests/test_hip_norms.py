"""GPU: gn_layernorm, gn_layernorm_silu, gn_layernorm_backward, gn_layernorm_silu_backward, gn_layernorm_param_grad (with
gn_layernorm_param_grad_workspace), gn_tensor_norm, gn_tensor_norm_backward, gn_head_energy and gn_head_grad called directly,
against the fp64 restatement and the a-priori per-element bounds of tests/norm_util.py (proved on the CPU by
tests/test_norm_host.py).  Every output lies between sentinel guard rows, every launch runs twice (same bits), each case prints
its worst error / bound per output; the last test prints the worst per entry point."""
import math

import pytest
import torch

from tests import norm_util as U
from tests.norm_gpu import SENTINEL, Out
from tests.norm_gpu import bits as _bits, dev as _dev, launch as _launch, lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu

WORST = {}
R = U.ratio
LN_CASES, PG_CASES, TN_CASES, HEAD_CASES = (range(len(t)) for t in (U.LN_CASES, U.PG_CASES, U.TN_CASES, U.HEAD_CASES))
LN_IDS = [U.ln_id(n) for n in LN_CASES]
PG_IDS = [U.pg_case(n)["id"] for n in PG_CASES]
TN_IDS = [U.tn_id(n) for n in TN_CASES]
HEAD_IDS = [U.head_id(n) for n in HEAD_CASES]


def _note(entry, rs, tag):
    print(f"{tag}: " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))
    for k, v in rs.items():
        WORST[entry + "." + k] = max(WORST.get(entry + "." + k, 0.0), v)
    assert all(v <= 1.0 for v in rs.values()), (tag, rs)


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_run(c, x=None):
    """All four LayerNorm entry points on case c (the backwards on the forward's own input).  -> dict(y, ya, gx, gxa)."""
    lib, st = _lib(), _stream()
    N, F, k = c["N"], c["F"], c["act"]
    d = {key: _dev(c[key]) for key in ("gamma", "beta", "g")}
    d["x"] = _dev(c["x"] if x is None else x)
    p = {key: t.data_ptr() for key, t in d.items()}
    eps = c["eps"]
    out = _launch(lambda o: lib.gn_layernorm(p["x"], p["gamma"], p["beta"], eps, N, F, o["y"], st), dict(y=(N, F)))
    out.update(_launch(lambda o: lib.gn_layernorm_silu(p["x"], p["gamma"], p["beta"], eps, N, F, o["ya"], k, st), dict(ya=(N, F))))
    out.update(_launch(lambda o: lib.gn_layernorm_backward(p["x"], p["gamma"], eps, p["g"], N, F, o["gx"], st), dict(gx=(N, F))))
    out.update(_launch(lambda o: lib.gn_layernorm_silu_backward(p["x"], p["gamma"], p["beta"], eps, p["g"], N, F, o["gxa"], k, st),
                       dict(gxa=(N, F))))
    return out


ENTRY = dict(y="gn_layernorm", ya="gn_layernorm_silu", gx="gn_layernorm_backward", gxa="gn_layernorm_silu_backward")


@pytest.mark.parametrize("n", LN_CASES, ids=LN_IDS)
def test_layernorm_within_bound(n):
    c, ex = U.ln_case(n), U.ln_expected(n)
    out = _ln_run(c)
    for key, entry in ENTRY.items():
        _note(entry, {key: R(out[key], *ex[key])}, c["id"])
    for r, kind in enumerate(c["kinds"]):
        if kind == "zerograd":
            assert float(out["gx"][r].abs().max()) == 0.0 and float(out["gxa"][r].abs().max()) == 0.0
    if c["act"] == U.NONE:                                                   # the identity kind is the bare form, bit for bit
        assert torch.equal(_bits(out["ya"]), _bits(out["y"])) and torch.equal(_bits(out["gxa"]), _bits(out["gx"]))


def test_layernorm_non_finite_stays_in_its_row():
    n = LN_IDS.index("F64-N9-silu-r0")
    c = U.ln_case(n)
    clean = _ln_run(c)
    x = c["x"].clone()
    x[2, 5], x[6, 63] = math.nan, math.inf
    dirty = _ln_run(c, x)
    keep = torch.tensor([r not in (2, 6) for r in range(c["N"])])
    for key in clean:
        assert torch.equal(_bits(dirty[key][keep]), _bits(clean[key][keep])), key
        assert bool(torch.isnan(dirty[key][~keep]).all()), key


def test_layernorm_silu_pair_replays_in_a_graph():
    lib = _lib()
    c = U.ln_case(LN_IDS.index("F256-N4-silu-r5"))
    N, F, k, eps = c["N"], c["F"], c["act"], c["eps"]
    eager = _ln_run(c)
    d = {key: _dev(c[key]) for key in ("x", "gamma", "beta", "g")}
    p = {key: t.data_ptr() for key, t in d.items()}
    ya, gxa = Out(N, F), Out(N, F)

    def body():
        st = _stream()
        assert lib.gn_layernorm_silu(p["x"], p["gamma"], p["beta"], eps, N, F, ya.ptr(), k, st) == 0
        assert lib.gn_layernorm_silu_backward(p["x"], p["gamma"], p["beta"], eps, p["g"], N, F, gxa.ptr(), k, st) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    ya.inner().fill_(math.nan)
    gxa.inner().fill_(math.nan)
    graph.replay()
    torch.cuda.synchronize()
    ya.check("ya")
    gxa.check("gxa")
    assert torch.equal(_bits(ya.inner().cpu()), _bits(eager["ya"])) and torch.equal(_bits(gxa.inner().cpu()), _bits(eager["gxa"]))


def test_layernorm_zero_rows_touch_nothing():
    lib, st = _lib(), _stream()
    d = _dev(torch.randn(4 * 8))
    p = d.data_ptr()
    o = Out(4, 8, fill=SENTINEL)
    assert lib.gn_layernorm(p, p, p, 1e-5, 0, 8, o.ptr(), st) == 0 and lib.gn_layernorm_silu(p, p, p, 1e-5, 0, 8, o.ptr(), 0, st) == 0
    assert lib.gn_layernorm_backward(p, p, 1e-5, p, 0, 8, o.ptr(), st) == 0
    assert lib.gn_layernorm_silu_backward(p, p, p, 1e-5, p, 0, 8, o.ptr(), 0, st) == 0
    assert lib.gn_tensor_norm(p, p, 1e-12, 0, 8, 2, o.ptr(), st) == 0 and lib.gn_tensor_norm_backward(p, p, p, 1e-12, 0, 8, 2, o.ptr(), st) == 0
    assert lib.gn_head_energy(p, p, 0.0, 1.0, 0.0, 0.0, None, p, p, 0, 8, o.ptr(), o.ptr(), 0, o.ptr(), 0, st) == 0
    assert lib.gn_head_grad(p, p, 1.0, None, 0, 8, o.ptr(), 0, st) == 0
    torch.cuda.synchronize()
    assert bool((o.t == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ LayerNorm parameter gradients
@pytest.mark.parametrize("n", PG_CASES, ids=PG_IDS)
def test_layernorm_param_grad_within_bound(n):
    lib, st = _lib(), _stream()
    c = U.pg_case(n)
    N, C, k = c["N"], c["C"], c["act"]
    ref, b = U.pg_reference(c), [U.bound_of(t) for t in U.pg_transcript(U.RE, c)]
    d = {key: _dev(c[key]) for key in ("x", "gamma", "beta", "g")}
    p = {key: t.data_ptr() for key, t in d.items()}
    words = int(lib.gn_layernorm_param_grad_workspace(N, C))
    assert words == U.pg_workspace(N, C)
    specs = dict(work=(words, 1), dgamma=(C, 1))
    if not c["no_dbeta"]:
        specs["dbeta"] = (C, 1)
    out = _launch(lambda o: lib.gn_layernorm_param_grad(p["x"], p["gamma"], None if c["no_beta"] else p["beta"], c["eps"], p["g"], N, C,
                                                        k, o["work"], o["dgamma"], o.get("dbeta"), st), specs)
    assert bool(torch.isfinite(out["work"]).all()), "a workspace word was left unwritten"
    rs = {"dgamma": R(out["dgamma"][:, 0], ref[0], b[0])}
    if not c["no_dbeta"]:
        rs["dbeta"] = R(out["dbeta"][:, 0], ref[1], b[1])
    _note("gn_layernorm_param_grad", rs, c["id"])
    if N == 0:                                                               # no rows: exact zeros
        assert float(out["dgamma"].abs().max()) == 0.0 and (c["no_dbeta"] or float(out["dbeta"].abs().max()) == 0.0)


# ------------------------------------------------------------------------------------------------ TensorLayerNorm
def _tn_run(c, X=None):
    lib, st = _lib(), _stream()
    N, F, lmax, D = c["N"], c["F"], c["lmax"], c["D"]
    d = dict(X=_dev(c["X"] if X is None else X), w=_dev(c["w"]), g=_dev(c["g"]))
    p = {key: t.data_ptr() for key, t in d.items()}
    out = _launch(lambda o: lib.gn_tensor_norm(p["X"], p["w"], c["eps"], N, F, lmax, o["Y"], st), dict(Y=(N * D, F)))
    out.update(_launch(lambda o: lib.gn_tensor_norm_backward(p["X"], p["w"], p["g"], c["eps"], N, F, lmax, o["gX"], st),
                       dict(gX=(N * D, F))))
    return {key: t.view(N, D, F) for key, t in out.items()}


@pytest.mark.parametrize("n", TN_CASES, ids=TN_IDS)
def test_tensor_norm_within_bound_and_routing(n):
    c, ex = U.tn_case(n), U.tn_expected(n)
    out = _tn_run(c)
    _note("gn_tensor_norm", {"Y": R(out["Y"], *ex["Y"])}, c["id"])
    _note("gn_tensor_norm_backward", {"gX": R(out["gX"], *ex["gX"])}, c["id"])
    other = U.tn_transcript(U.F64, c, True, "last_extremal")[0].v          # the same gradient routed to the LAST extremal channel
    bound = ex["gX"][1]
    for (a, l), kind in c["plan"].items():
        off, cnt = l * l - 1, 2 * l + 1
        blk = slice(off, off + cnt)
        if kind == "all_equal" or c["F"] == 1:
            assert float(out["Y"][a, blk].abs().max()) == 0.0 and float(out["gX"][a, blk].abs().max()) == 0.0, "flat block"
        elif kind in U.TIE_KINDS and c["F"] >= 4:                            # first index, as torch.max / torch.min route
            assert R(out["gX"][a, blk], ex["gX"][0][a, blk], bound[a, blk]) <= 1.0
            assert R(out["gX"][a, blk], other[a, blk], bound[a, blk]) > 1.0, (kind, a, l)


def test_tensor_norm_non_finite_stays_in_its_block():
    c = U.tn_case(TN_IDS.index("l3-F200-N5"))
    clean = _tn_run(c)
    X = c["X"].clone()
    X[1, 4, 7], X[3, 10, 150] = math.nan, math.inf                           # (atom 1, degree 2) and (atom 3, degree 3)
    dirty = _tn_run(c, X)
    keep = torch.ones(c["N"], c["D"], dtype=torch.bool)
    keep[1, 3:8], keep[3, 8:15] = False, False
    for key in clean:
        assert torch.equal(_bits(dirty[key][keep]), _bits(clean[key][keep])), key


# ------------------------------------------------------------------------------------------------ energy head
def _head_run(c, mean, pre1=None, graph=False):
    lib = _lib()
    A, Hd, k, n_mol = c["A"], c["Hd"], c["act"], c["n_mol"]
    d = {key: _dev(c[key]) for key in ("W2", "atomref", "z", "mol_ptr")}
    d["pre1"] = _dev(c["pre1"] if pre1 is None else pre1)
    p = {key: t.data_ptr() for key, t in d.items()}
    ref_p = p["atomref"] if c["use_ref"] else None

    def call(o):
        st = _stream()
        rc = lib.gn_head_energy(p["pre1"], p["W2"], c["b2"], c["scale"], c["shift"], c["mol_shift"], ref_p, p["z"], p["mol_ptr"],
                                n_mol, Hd, o["y"], o["energy"], mean, o.get("atom_scale"), k, st)
        return rc or lib.gn_head_grad(p["pre1"], p["W2"], c["scale"], o.get("atom_scale"), A, Hd, o["g_pre1"], k, st)

    specs = dict(y=(A, 1), energy=(n_mol, 1), g_pre1=(A, Hd))
    if c["use_asc"]:
        specs["atom_scale"] = (A, 1)
    if not graph:
        out = _launch(call, specs)
        return {key: (t[:, 0] if key != "g_pre1" else t) for key, t in out.items()}
    outs = {key: Out(r, cc) for key, (r, cc) in specs.items()}
    ptrs = {key: o.ptr() for key, o in outs.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call(ptrs) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert call(ptrs) == 0
    for o in outs.values():
        o.inner().fill_(math.nan)
    g.replay()
    torch.cuda.synchronize()
    for key, o in outs.items():
        o.check(key)
    return {key: (o.inner().cpu()[:, 0] if key != "g_pre1" else o.inner().cpu()) for key, o in outs.items()}


@pytest.mark.parametrize("n", HEAD_CASES, ids=HEAD_IDS)
def test_head_within_bound(n):
    c = U.head_case(n)
    for mean in (0, 1):
        ex, out = U.head_expected(n, mean), _head_run(c, mean)
        _note("gn_head_energy", {key: R(out[key], *ex[key]) for key in out if key != "g_pre1"}, f"{c['id']} mean={mean}")
        _note("gn_head_grad", {"g_pre1": R(out["g_pre1"], *ex["g_pre1"])}, f"{c['id']} mean={mean}")
        for b, size in enumerate(c["sizes"]):
            if size == 0:
                assert float(out["energy"][b]) == c["mol_shift"], "the empty molecule"
        if c["use_asc"]:                                                     # 1 / n is one correctly rounded division; `sum`: exactly 1
            want = (1.0 / torch.tensor(c["sizes"], dtype=torch.float32))[torch.repeat_interleave(
                torch.arange(c["n_mol"]), torch.tensor(c["sizes"]))] if mean else torch.ones(c["A"])
            assert torch.equal(_bits(out["atom_scale"]), _bits(want))


def test_head_replays_in_a_graph():
    c = U.head_case(HEAD_IDS.index("Hd32-A1033-silu-atomref-ascale"))
    eager, replay = _head_run(c, 1), _head_run(c, 1, graph=True)
    for key in eager:
        assert torch.equal(_bits(eager[key]), _bits(replay[key])), key


def test_head_non_finite_stays_in_its_molecule():
    n = HEAD_IDS.index("Hd65-A248-sigmoid-atomref-ascale")
    c = U.head_case(n)
    ptr = c["mol_ptr"].tolist()
    pre1 = c["pre1"].clone()
    a_nan, a_inf = ptr[3] + 2, ptr[6] + 40                                   # an atom of molecule 3 and one of molecule 6
    pre1[a_nan, 5], pre1[a_inf, 60] = math.nan, -math.inf
    for mean in (0, 1):
        clean, dirty = _head_run(c, mean), _head_run(c, mean, pre1)
        atoms = torch.ones(c["A"], dtype=torch.bool)
        atoms[a_nan], atoms[a_inf] = False, False
        mols = torch.ones(c["n_mol"], dtype=torch.bool)
        mols[3], mols[6] = False, False
        assert torch.equal(_bits(dirty["y"][atoms]), _bits(clean["y"][atoms]))
        assert torch.equal(_bits(dirty["energy"][mols]), _bits(clean["energy"][mols])) and bool(torch.isnan(dirty["energy"][3]))
        assert torch.equal(_bits(dirty["atom_scale"]), _bits(clean["atom_scale"]))
        elem = torch.ones(c["A"], c["Hd"], dtype=torch.bool)
        elem[a_nan, 5], elem[a_inf, 60] = False, False
        assert torch.equal(_bits(dirty["g_pre1"][elem]), _bits(clean["g_pre1"][elem]))


def test_worst_ratios_per_entry_point():
    print("worst error / bound: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())))
    assert WORST and all(v <= 1.0 for v in WORST.values())
