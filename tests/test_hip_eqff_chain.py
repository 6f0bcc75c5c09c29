"""GPU: the EQFF node chain called directly, in BOTH of its forms on the same inputs -- the fused kernels
(gn_eqff_fused_forward / _backward) and the launch sequence they replace (gn_eqff_context -> gemm -> gemm -> gn_eqff_update;
gn_eqff_backward_a -> gemm -> gemm -> gn_eqff_backward_b) -- against the fp64 restatement and the per-atom bounds of
tests/eqff_util.py (proved on the CPU by tests/test_eqff_chain_host.py).  The forward is checked product by product
against fp64 products of the kernel's own fp32 input to each; the backward against the bounds carried to its outputs.
Each case prints the worst error / bound per stage."""
import pytest
import torch

from tests import eqff_util as U

pytestmark = pytest.mark.gpu

PAD = 8                                            # sentinel rows past N in every array a kernel writes
SENTINEL = 12345.678
_FLOAT_KEYS = ("h", "X", "Xp", "gh", "gX", "W0", "b0", "W1", "b1")


def _gpu(d):
    """Device copies + the transposed weights; every tensor a kernel reads is fp32 and contiguous, of the size N, D, F imply."""
    F, N, D = d["F"], d["N"], d["D"]
    g = {k: (None if d[k] is None else d[k].cuda().contiguous()) for k in _FLOAT_KEYS}
    g["W1T"], g["W0T"] = g["W1"].t().contiguous(), g["W0"].t().contiguous()
    want = dict(h=(N, F), X=(N, D, F), Xp=(N, D, F), gh=(N, F), gX=(N, D, F), W0=(F, 2 * F), b0=(F,), W1=(2 * F, F),
                b1=(2 * F,), W1T=(F, 2 * F), W0T=(2 * F, F))
    for k, shape in want.items():
        if g[k] is not None:
            assert g[k].dtype == torch.float32 and g[k].is_contiguous() and tuple(g[k].shape) == shape, k
    assert N >= 1 and D >= 1 and F in (128, 256)
    return g


def _padded(t, N):
    """A copy of t's first N rows followed by PAD sentinel rows (t = None: NaN rows, so that a skipped element shows)."""
    out = torch.full((N + PAD,) + tuple(t.shape[1:]), SENTINEL, device="cuda")
    out[:N] = t[:N]
    return out


def _fresh(N, *tail):
    out = torch.full((N + PAD,) + tail, SENTINEL, device="cuda")
    out[:N] = float("nan")
    return out


def _take(bufs, N):
    for k, b in bufs.items():
        assert bool((b[N:] == SENTINEL).all()), f"{k}: a row past N was written"
    return {k: b[:N].cpu() for k, b in bufs.items()}


def _same_bits(a, b):
    """Bit equality; a non-finite element must be non-finite in both (its payload is not a value)."""
    fa, fb = torch.isfinite(a), torch.isfinite(b)
    return bool((fa == fb).all()) and torch.equal(a[fa].view(torch.int32), b[fb].view(torch.int32))


def _planes(g, arith):
    from gotennet_amd import engine, _lib
    lib = _lib.load()
    sizer = lib.gn_split_bf16x3_size if arith == "split" else lib.gn_split_f16x2_size
    out = {}
    for k in ("W0", "W1", "W1T", "W0T"):
        out[k] = engine.split_weight(g[k], arith)
        assert out[k].numel() == sizer(g[k].shape[0], g[k].shape[1]) and out[k].is_contiguous()
    return out


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _forward(d, g, arith, form="fused", save=True):
    """h', X' and the kept tensors of one forward, on the CPU.  form: "fused" (save = False: the ctx_out = mm_out = NULL
    inference form) or "sequence".  Two launches: same bits.  Every written array carries PAD sentinel rows."""
    from gotennet_amd import engine, _lib
    F, N, D = d["F"], d["N"], d["D"]
    p = _planes(g, arith)
    ptr = lambda t: None if t is None else t.data_ptr()
    outs = []
    for _ in range(2):
        b = dict(h=_padded(g["h"], N), X=_padded(g["X"], N), pre=_fresh(N, F))
        if save or form == "sequence":
            b.update(ctx=_fresh(N, 2 * F), mm=_fresh(N, 2 * F))
        if form == "fused":
            rc = _lib.load().gn_eqff_fused_forward(
                ptr(g["Xp"]), ptr(p["W0"]), ptr(g["b0"]), ptr(p["W1"]), ptr(g["b1"]), float(d["eps"]), N, F, D, ptr(b["h"]),
                ptr(b["X"]), ptr(b.get("ctx")), ptr(b["pre"]), ptr(b.get("mm")), U.ARITH[arith], _stream())
            assert rc == 0, rc
        else:                                       # as engine._eqff_htr_forward sequences it
            b["g1act"] = _fresh(N, F)
            _lib.call("gn_eqff_context", ptr(b["h"]), ptr(g["Xp"]), float(d["eps"]), N, F, D, ptr(b["ctx"]), _stream())
            engine.gemm(b["ctx"], 2 * F, g["W0"], g["b0"], b["g1act"], F, N, F, 2 * F, act=(0, F), pre_out=b["pre"], mode=arith)
            engine.gemm(b["g1act"], F, g["W1"], g["b1"], b["mm"], 2 * F, N, 2 * F, F, mode=arith)
            _lib.call("gn_eqff_update", ptr(b["mm"]), ptr(g["Xp"]), N, F, D, ptr(b["h"]), ptr(b["X"]), _stream())
        torch.cuda.synchronize()
        outs.append(_take(b, N))
    for k in outs[0]:
        assert _same_bits(outs[0][k], outs[1][k]), f"{form} forward, {k}: two launches differ"
    return outs[0]


def _backward(d, g, arith, saved, form="fused", gX_null=False):
    """g_Xp, g_h1 of one backward on the saved tensors given (CPU, from a forward), on the CPU."""
    from gotennet_amd import engine, _lib
    F, N, D = d["F"], d["N"], d["D"]
    p = _planes(g, arith)
    mm, ctx, pre = (saved[k].cuda().contiguous() for k in ("mm", "ctx", "pre"))
    assert tuple(mm.shape) == (N, 2 * F) and tuple(ctx.shape) == (N, 2 * F) and tuple(pre.shape) == (N, F)
    ptr = lambda t: None if t is None else t.data_ptr()
    gX = None if gX_null else g["gX"]
    outs = []
    for _ in range(2):
        b = dict(gXp=_fresh(N, D, F), gh1=_fresh(N, F))
        if form == "fused":
            rc = _lib.load().gn_eqff_fused_backward(
                ptr(g["gh"]), ptr(gX), ptr(mm), ptr(g["Xp"]), ptr(ctx), ptr(pre), ptr(p["W1T"]), ptr(p["W0T"]), N, F, D,
                ptr(b["gXp"]), ptr(b["gh1"]), U.ARITH[arith], _stream())
            assert rc == 0, rc
        else:                                       # as engine._eqff_htr_backward sequences it
            b.update(gm=_fresh(N, 2 * F), g_g1=_fresh(N, F), g_ctx=_fresh(N, 2 * F))
            _lib.call("gn_eqff_backward_a", ptr(g["gh"]), ptr(gX), ptr(mm), ptr(g["Xp"]), N, F, D, ptr(b["gm"]), ptr(b["gXp"]),
                      _stream())
            engine.gemm(b["gm"], 2 * F, g["W1T"], None, b["g_g1"], F, N, F, 2 * F, dgate=pre, mode=arith)
            engine.gemm(b["g_g1"], F, g["W0T"], None, b["g_ctx"], 2 * F, N, 2 * F, F, mode=arith)
            _lib.call("gn_eqff_backward_b", ptr(b["g_ctx"]), ptr(ctx), ptr(g["Xp"]), ptr(g["gh"]), N, F, D, ptr(b["gXp"]),
                      ptr(b["gh1"]), _stream())
        torch.cuda.synchronize()
        outs.append(_take(b, N))
    for k in outs[0]:
        assert _same_bits(outs[0][k], outs[1][k]), f"{form} backward, {k}: two launches differ"
    return outs[0]


def _good(d):
    ok = torch.ones(d["N"], dtype=torch.bool)
    ok[d.get("bad", [])] = False
    return ok


def _check_forward(d, o, arith, what):
    """The stage-wise checks of one forward's outputs (fused or sequence); -> the per-stage worst error / bound."""
    F, N, D = d["F"], d["N"], d["D"]
    ok = _good(d)
    r = U.forward_ref(d)
    ratios = {}
    assert torch.equal(o["ctx"][:, :F].view(torch.int32), d["h"].view(torch.int32))
    n_err = ((o["ctx"][:, F:].double() - r["ctx"][:, F:]).abs() / r["ctx"][:, F:])[ok]
    ratios["n"] = float(n_err.max() / ((D + 3) * U.U32))
    hidden = U.SILU(o["pre"].double())
    stages = (("pre", o["pre"], o["ctx"], d["W0"], d["b0"]), ("mm", o["mm"], hidden, d["W1"], d["b1"]))
    stat = {}
    for name, C, op, W, b in stages:
        err, bet, dd = U.product_check(C, op, W, b, arith)
        near = ok & (dd <= U.NEAR_D)
        ratios[name] = float((err / bet)[ok].max())
        ratios[name + "_near"] = float(err[near].max() / U.NEAR)
        stat[name] = (err, dd, near)
    h1 = d["h"] + o["mm"][:, :F]                     # one fp32 add of stored values: the same bits
    assert _same_bits(o["h"][ok], h1[ok]), f"{what}: h' is not h + m1"
    X1 = d["X"].double() + o["mm"][:, None, F:].double() * d["Xp"].double()
    x_err = (o["X"].double() - X1).abs()[ok]
    ratios["X"] = float((x_err / (U.U32 * X1.abs()[ok] + 2.0 ** -149)).max())     # one fused multiply-add
    print(f"{what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)
    return stat


def _check_backward(d, o, saved, arith, what):
    ok = _good(d)
    r = U.backward_ref(d, saved["mm"], saved["ctx"], saved["pre"])
    E_gXp, E_gh1 = U.backward_bounds(d, r, saved["mm"], saved["ctx"], saved["pre"], arith)
    ratios = {}
    for name, C, ref, bnd in (("gXp", o["gXp"], r["gXp"], E_gXp), ("gh1", o["gh1"], r["gh1"], E_gh1)):
        err, bnd = (C.double() - ref).abs()[ok], bnd[ok]
        assert bool(torch.isfinite(C[ok]).all()), f"{what}: {name} is non-finite outside the poisoned atoms"
        assert bool((err <= bnd).all()), (what, name, float((err[bnd > 0] / bnd[bnd > 0]).max()))
        ratios[name] = float((err[bnd > 0] / bnd[bnd > 0]).max()) if bool((bnd > 0).any()) else 0.0
    print(f"{what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("arith", ["f16x2", "split"])
@pytest.mark.parametrize("F,N,D", U.SHAPES)
def test_eqff_chain_both_forms_against_fp64(F, N, D, arith):
    """N in {1, 7, 8, 9, 17} (clamped loads, skipped stores of the last 8-atom tile) x D in {3, 8, 15, 24, 35, 80} (the
    clamped last trip of the 8-row loop): fused and sequence, forward and backward; "split": the two forms' bits agree."""
    d = U.make(F, N, D)
    g = _gpu(d)
    fwd = {form: _forward(d, g, arith, form) for form in ("fused", "sequence")}
    for form, o in fwd.items():
        _check_forward(d, o, arith, f"F{F} N{N} D{D} {arith} {form} forward")
    lean = _forward(d, g, arith, "fused", save=False)                  # ctx_out = mm_out = NULL
    assert _same_bits(lean["h"], fwd["fused"]["h"]) and _same_bits(lean["X"], fwd["fused"]["X"])
    saved = fwd["fused"]
    bwd = {form: _backward(d, g, arith, saved, form) for form in ("fused", "sequence")}
    for form, o in bwd.items():
        _check_backward(d, o, saved, arith, f"F{F} N{N} D{D} {arith} {form} backward")
    if arith == "split":
        for k in ("h", "X", "ctx", "pre", "mm"):
            assert _same_bits(fwd["fused"][k], fwd["sequence"][k]), k
        for k in ("gXp", "gh1"):
            assert _same_bits(bwd["fused"][k], bwd["sequence"][k]), k


@pytest.mark.parametrize("arith", ["f16x2", "split"])
@pytest.mark.parametrize("F", [128, 256])
def test_eqff_chain_hostile_operands(F, arith):
    """One tile spread over ten decades with an all-zero atom, one tile entirely zero, one ordinary (N = 17); and an Inf / a
    NaN in two atoms of a tile.  Per-atom bounds for everyone else; exact zeros where the operand is zero."""
    d = U.make(F, 17, 8, hostile="spread")
    g = _gpu(d)
    fwd = {form: _forward(d, g, arith, form) for form in ("fused", "sequence")}
    stat = {form: _check_forward(d, o, arith, f"F{F} spread {arith} {form} forward") for form, o in fwd.items()}
    saved = fwd["fused"]
    bwd = {form: _backward(d, g, arith, saved, form) for form in ("fused", "sequence")}
    for form, o in bwd.items():
        _check_backward(d, o, saved, arith, f"F{F} spread {arith} {form} backward")
    zero = [4] + list(range(8, 16))                  # m * X_p and both gradients of an all-zero atom: exact
    for form in fwd:
        assert torch.equal(fwd[form]["X"][zero].view(torch.int32), d["X"][zero].view(torch.int32))
        assert bool((bwd[form]["gXp"][zero] == 0).all())
    if arith == "f16x2":                             # not vacuous: the atoms the bound loosens are the atoms that need it
        for name in ("pre", "mm"):
            err, dd, near = stat["fused"][name]
            assert bool((dd > 28).any()) and float(err[dd > 28].max()) > float(err[near].max()), name
    else:
        for k in ("h", "X", "ctx", "pre", "mm"):
            assert _same_bits(fwd["fused"][k], fwd["sequence"][k]), k
        for k in ("gXp", "gh1"):
            assert _same_bits(bwd["fused"][k], bwd["sequence"][k]), k

    d = U.make(F, 9, 8, hostile="nonfinite")
    g = _gpu(d)
    fwd = {form: _forward(d, g, arith, form) for form in ("fused", "sequence")}
    for form, o in fwd.items():
        _check_forward(d, o, arith, f"F{F} nonfinite {arith} {form} forward")
        for k in ("h", "X", "pre", "mm"):
            rows = torch.isfinite(o[k]).flatten(1).all(1)
            assert rows.tolist() == _good(d).tolist(), f"{form} {k}: non-finite rows {(~rows).nonzero().flatten().tolist()}"
    saved = fwd["fused"]
    bwd = {form: _backward(d, g, arith, saved, form) for form in ("fused", "sequence")}
    for form, o in bwd.items():
        _check_backward(d, o, saved, arith, f"F{F} nonfinite {arith} {form} backward")
        for k in ("gXp", "gh1"):
            rows = torch.isfinite(o[k]).flatten(1).all(1)
            assert rows.tolist() == _good(d).tolist(), f"{form} {k}: non-finite rows {(~rows).nonzero().flatten().tolist()}"
    if arith == "split":
        for k in ("h", "X", "ctx", "pre", "mm"):
            assert _same_bits(fwd["fused"][k], fwd["sequence"][k]), k
        for k in ("gXp", "gh1"):
            assert _same_bits(bwd["fused"][k], bwd["sequence"][k]), k


@pytest.mark.parametrize("F,N,D", [(128, 17, 24), (256, 9, 3)])
def test_eqff_chain_split_is_row_wise(F, N, D):
    """ "split" arithmetic: permuting the atoms permutes the outputs bit for bit (another tile, another row of the tile)."""
    d = U.make(F, N, D)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3))
    d2 = dict(d, **{k: d[k][perm].contiguous() for k in ("h", "X", "Xp", "gh", "gX")})
    o1, o2 = _forward(d, _gpu(d), "split"), _forward(d2, _gpu(d2), "split")
    for k in ("h", "X", "ctx", "pre", "mm"):
        assert _same_bits(o1[k][perm], o2[k]), k
    b1, b2 = _backward(d, _gpu(d), "split", o1), _backward(d2, _gpu(d2), "split", o2)
    for k in ("gXp", "gh1"):
        assert _same_bits(b1[k][perm], b2[k]), k


def test_eqff_backward_a_null_gx_is_a_zero_gx():
    """gn_eqff_backward_a with g_X = NULL (an energy head that reads h only) against a zero g_X: the same bits."""
    d = U.make(128, 9, 15)
    g = _gpu(d)
    saved = _forward(d, g, "split")
    null = _backward(d, g, "split", saved, "sequence", gX_null=True)
    g["gX"] = torch.zeros_like(g["gX"])
    zero = _backward(dict(d, gX=torch.zeros_like(d["gX"])), g, "split", saved, "sequence")
    for k in ("gm", "g_g1", "g_ctx", "gXp", "gh1"):
        assert _same_bits(null[k], zero[k]), k
    fused = _backward(dict(d, gX=torch.zeros_like(d["gX"])), g, "split", saved, "fused")
    assert _same_bits(fused["gXp"], zero["gXp"]) and _same_bits(fused["gh1"], zero["gh1"])


def test_eqff_fused_refusals_return_before_any_launch():
    from gotennet_amd import _lib
    lib = _lib.load()
    d = U.make(128, 9, 8)
    g = _gpu(d)
    p = _planes(g, "f16x2")
    saved = _forward(d, g, "f16x2")
    mm, ctx, pre = (saved[k].cuda() for k in ("mm", "ctx", "pre"))
    N, F, D = d["N"], d["F"], d["D"]
    gXp, gh1, h, X = _fresh(N, D, F), _fresh(N, F), _padded(g["h"], N), _padded(g["X"], N)
    st = _stream()
    bwd = lambda F_, arith, out: lib.gn_eqff_fused_backward(
        g["gh"].data_ptr(), g["gX"].data_ptr(), mm.data_ptr(), g["Xp"].data_ptr(), ctx.data_ptr(), pre.data_ptr(),
        p["W1T"].data_ptr(), p["W0T"].data_ptr(), N, F_, D, out, gh1.data_ptr(), arith, st)
    fwd = lambda F_, arith: lib.gn_eqff_fused_forward(
        g["Xp"].data_ptr(), p["W0"].data_ptr(), g["b0"].data_ptr(), p["W1"].data_ptr(), g["b1"].data_ptr(), 1e-8, N, F_, D,
        h.data_ptr(), X.data_ptr(), None, None, None, arith, st)
    assert bwd(F, 2, g["gX"].data_ptr()) == _lib.GN_ERR_BAD_ARG            # g_Xp == g_X
    assert bwd(64, 2, gXp.data_ptr()) == _lib.GN_ERR_BAD_ARG and bwd(F, 3, gXp.data_ptr()) == _lib.GN_ERR_BAD_ARG
    assert bwd(F, 0, gXp.data_ptr()) == _lib.GN_ERR_BAD_ARG
    assert fwd(64, 2) == _lib.GN_ERR_BAD_ARG and fwd(512, 1) == _lib.GN_ERR_BAD_ARG and fwd(F, 3) == _lib.GN_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(gXp[:N]).all()) and bool(torch.isnan(gh1[:N]).all())          # nothing was launched
    assert torch.equal(h[:N], g["h"]) and torch.equal(X[:N], g["X"]) and torch.equal(g["gX"].cpu(), d["gX"])
    assert not lib.gn_eqff_fused_supported(64, 0, 2) and not lib.gn_eqff_fused_supported(128, 3, 2)
    assert lib.gn_eqff_fused_supported(128, 0, 1) and lib.gn_eqff_fused_supported(256, 0, 2)
