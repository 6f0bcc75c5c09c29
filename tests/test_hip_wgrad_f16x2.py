"""GPU: the f16x2 weight-gradient kernel (``wgrad_mode = "f16x2"``, gn_weight_grad_group_mode) against fp64 torch on
small and edge shapes, its exponent paths and store bounds, the routing of the modules' backward, and the parameter
gradients of the models and the QM9 read-outs against the fp64 oracle with that arithmetic."""
import pytest
import torch

from tests.test_hip_param_grads import _check, _energy_loss, _err, _gpu_modules, _launches, _oracle
from tests.test_hip_qm9_training import _compare, _kat_head, _kat_inputs, _kat_loss, _kat_oracle
from tests.test_qm9_training_host import HEADS, qm9_grad_kat

pytestmark = pytest.mark.gpu

TOL = 1e-4
MODE = "f16x2"
DEV = "cuda"


def _run(probs, mode=MODE, chunk=16):
    from gotennet_amd import engine
    for i0 in range(0, len(probs), chunk):
        engine.weight_grad_group(probs[i0:i0 + chunk], mode=mode)


def _assert_close(q, rw, rb, what):
    ew = _err(q["dW"], rw)
    print(f"{what}: dW {ew:.3e}")
    assert bool(torch.isfinite(q["dW"]).all()), (what, "dW not finite")
    assert ew <= 1e-5, (what, "dW", ew)
    if rb is not None:
        eb = _err(q["db"], rb)
        print(f"{what}: db {eb:.3e}")
        assert bool(torch.isfinite(q["db"]).all()), (what, "db not finite")
        assert eb <= 1e-5, (what, "db", eb)


# ---------------------------------------------------------------------------------------------------- 1. kernel
def test_kernel_matches_fp64_on_small_shapes():
    torch.manual_seed(0)
    probs, refs = [], []
    shapes = [(r, n, k) for r in (0, 1, 15, 16, 17, 31, 33, 513, 2049) for n in (1, 3, 33, 96) for k in (20, 32, 257)]
    shapes.append((54373, 33, 257))                  # several row splits
    for i, (rows, nout, K) in enumerate(shapes):
        y_off, a_off = i % 3, (i * 5) % 7
        dY = torch.randn(max(rows, 1), nout + y_off + 2, device=DEV)
        A = torch.randn(max(rows, 1), K + a_off + 1, device=DEV)
        dW = torch.full((nout, K), float("nan"), device=DEV)
        db = torch.full((nout,), float("nan"), device=DEV)
        probs.append(dict(dY=dY, ldy=dY.shape[1], y_off=y_off, A=A, lda=A.shape[1], a_off=a_off, dW=dW, db=db,
                          rows=rows, nout=nout, K=K))
        yr, ar = dY[:rows, y_off:y_off + nout].double(), A[:rows, a_off:a_off + K].double()
        refs.append((yr.t() @ ar, yr.sum(0)))
    # a degree row map over X [N, D, F]: the rows of degree l = 2 (5 of D = 8)
    N, D, F = 1000, 8, 64
    gEK, X = torch.randn(N, D, F, device=DEV), torch.randn(N, D, F, device=DEV)
    dWk = torch.full((F, F), float("nan"), device=DEV)
    probs.append(dict(dY=gEK, ldy=F, A=X, lda=F, dW=dWk, rows=N * 5, nout=F, K=F, rowmap=(5, D, 3)))
    refs.append((gEK[:, 3:8].reshape(-1, F).double().t() @ X[:, 3:8].reshape(-1, F).double(), None))
    _run(probs)
    first = [(q["dW"].clone(), None if q.get("db") is None else q["db"].clone()) for q in probs]
    for q in probs:
        q["dW"].fill_(float("nan"))
        if q.get("db") is not None:
            q["db"].fill_(float("nan"))
    _run(probs)
    for q, (rw, rb), (w1, b1) in zip(probs, refs, first):
        what = (q["rows"], q["nout"], q["K"])
        _assert_close(q, rw, rb, what)
        assert torch.equal(q["dW"], w1), what                    # bit-reproducible
        if rb is not None:
            assert torch.equal(q["db"], b1), what


# ---------------------------------------------------------------------------------------------------- 2. exponents
def _exponent_case(kind):
    g = torch.Generator().manual_seed(5)
    rows, n = 96, 64
    dY, A = torch.randn(rows, n, generator=g), torch.randn(rows, n, generator=g)
    two = lambda e: 2.0 ** e
    if kind == "grow":                               # the exponent grows at the second stage: the accumulator is rescaled
        dY[:32] *= two(-30); A[:32] *= two(-30); dY[32:] *= two(10); A[32:] *= two(10)
    elif kind == "shrink":
        dY[:64] *= two(10); A[:64] *= two(10); dY[64:] *= two(-30); A[64:] *= two(-30)
    elif kind == "zero_stage":
        dY[32:64] = 0.0; A[32:64] = 0.0
    elif kind == "row_scales":
        s = torch.ldexp(torch.ones(rows), torch.randint(-20, 21, (rows,), generator=g))[:, None]
        dY, A = dY * s, A * s
    elif kind == "col_scales":
        dY = dY * torch.ldexp(torch.ones(n), torch.randint(-12, 13, (n,), generator=g))
        A = A * torch.ldexp(torch.ones(n), torch.randint(-12, 13, (n,), generator=g))
    return dY.to(DEV), A.to(DEV)


@pytest.mark.parametrize("kind", ["grow", "shrink", "zero_stage", "row_scales", "col_scales"])
def test_exponent_paths(kind):
    dY, A = _exponent_case(kind)
    rows, n = dY.shape
    q = dict(dY=dY, ldy=n, A=A, lda=n, dW=torch.full((n, n), float("nan"), device=DEV),
             db=torch.full((n,), float("nan"), device=DEV), rows=rows, nout=n, K=n)
    _run([q])
    _assert_close(q, dY.double().t() @ A.double(), dY.double().sum(0), kind)


def test_zero_blocks_give_exact_zeros():
    g = torch.Generator().manual_seed(6)
    rows, n = 96, 64
    dY, A = torch.randn(rows, n, generator=g).to(DEV), torch.randn(rows, n, generator=g).to(DEV)
    dY[:, 32:] = 0.0                                 # an all-zero 32-column block of dY
    q = dict(dY=dY, ldy=n, A=A, lda=n, dW=torch.full((n, n), float("nan"), device=DEV),
             db=torch.full((n,), float("nan"), device=DEV), rows=rows, nout=n, K=n)
    _run([q])
    assert torch.equal(q["dW"][32:], torch.zeros(32, n, device=DEV)) and torch.equal(q["db"][32:], torch.zeros(32, device=DEV))
    _assert_close(q, dY.double().t() @ A.double(), dY.double().sum(0), "zero dY block")
    q["A"] = torch.zeros(rows, n, device=DEV)        # an all-zero A
    q["dW"].fill_(float("nan"))
    _run([q])
    assert torch.equal(q["dW"], torch.zeros(n, n, device=DEV))


# ---------------------------------------------------------------------------------------------------- 3. bounds
def test_only_the_addressed_block_is_written():
    torch.manual_seed(2)
    rows, nout, K, w_row, total = 300, 33, 257, 7, 50
    dY, A = torch.randn(rows, nout, device=DEV), torch.randn(rows, K, device=DEV)
    sentinel = -12345.0
    dW = torch.full((total, K + 5), sentinel, device=DEV)
    db = torch.full((total,), sentinel, device=DEV)
    _run([dict(dY=dY, ldy=nout, A=A, lda=K, dW=dW, w_row=w_row, db=db, b_row=w_row, rows=rows, nout=nout, K=K)])
    ref = dY.double().t() @ A.double()
    assert _err(dW[w_row:w_row + nout, :K], ref) <= 1e-5
    assert _err(db[w_row:w_row + nout], dY.double().sum(0)) <= 1e-5
    keep = torch.ones_like(dW, dtype=torch.bool)
    keep[w_row:w_row + nout, :K] = False
    assert bool((dW[keep] == sentinel).all())
    keepb = torch.ones_like(db, dtype=torch.bool)
    keepb[w_row:w_row + nout] = False
    assert bool((db[keepb] == sentinel).all())


# ---------------------------------------------------------------------------------------------------- 4. routing
def _backward_calls_and_grads(mode, set_attr=True):
    o = _oracle("l2_sep_f32")
    net, head = _gpu_modules(o)
    if set_attr:
        net.wgrad_mode = head.wgrad_mode = mode
    loss = _energy_loss(net, head, o)
    calls = _launches(loss.backward)
    grads = {n: p.grad.clone() for n, p in net.named_parameters()}
    grads.update({"head." + n: p.grad.clone() for n, p in head.named_parameters()})
    return calls, grads


def test_backward_routes_by_wgrad_mode():
    calls, _ = _backward_calls_and_grads(MODE)
    assert "gn_weight_grad_group_mode" in calls and "gn_weight_grad_group" not in calls
    base_calls, base = _backward_calls_and_grads(None, set_attr=False)     # modules that never had the attribute set
    assert "gn_weight_grad_group" in base_calls and "gn_weight_grad_group_mode" not in base_calls
    for mode in (None, "f32"):
        calls, grads = _backward_calls_and_grads(mode)
        assert calls == base_calls, mode
        for n in base:
            assert torch.equal(grads[n], base[n]), (mode, n)


def test_head_alone_routes_by_wgrad_mode():
    import types
    from gotennet_amd.outputs import Atomwise
    torch.manual_seed(4)
    N, F = 21, 32
    batch, z = torch.arange(3).repeat_interleave(7).cuda(), torch.randint(1, 9, (N,)).cuda()
    head = Atomwise(n_in=F, n_hidden=16, activation="silu").cuda().eval()
    head.parameter_grads = True
    h = torch.randn(N, F, device=DEV)
    out = {}
    for mode in ("unset", None, "f32", MODE):
        if mode != "unset":
            head.wgrad_mode = mode
        head.zero_grad(set_to_none=True)
        inp = types.SimpleNamespace(z=z, batch=batch, pos=None, representation=h.clone().requires_grad_(True))
        loss = head(inp)["y"].sum()
        calls = _launches(loss.backward)
        new, old = "gn_weight_grad_group_mode" in calls, "gn_weight_grad_group" in calls
        assert (new, old) == ((True, False) if mode == MODE else (False, True)), mode
        out[mode] = [p.grad.clone() for p in head.parameters()]
    for mode in (None, "f32"):
        for a, b in zip(out[mode], out["unset"]):
            assert torch.equal(a, b), mode
    for a, b in zip(out[MODE], out["unset"]):
        assert _err(a, b) <= 1e-5


# ---------------------------------------------------------------------------------------------------- 5. parity
PARITY = ["l2_sep_f32", "l4_sep_f32", "l2_mixed_f64ch", "l7_mixed_jointhtr_gated", "opt_layernorm_tln", "opt_aggr_max_l3"]


@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("name", PARITY)
def test_parameter_gradients_match_oracle_in_f16x2(name):
    """Both losses of test_hip_param_grads, every parameter <= 1e-4 of its own maximum against fp64 autograd, exact zeros
    where the oracle's are."""
    o = _oracle(name)
    net, head = _gpu_modules(o)
    net.wgrad_mode = head.wgrad_mode = MODE
    loss = _energy_loss(net, head, o)
    calls = _launches(loss.backward)
    assert "gn_weight_grad_group_mode" in calls and "gn_weight_grad_group" not in calls
    got = {n: p.grad for n, p in net.named_parameters()}
    got.update({"head." + n: p.grad for n, p in head.named_parameters()})
    _check(got, o["energy"], "energy")
    net.zero_grad(set_to_none=True)
    t = o["t"]
    h, X = net(t["z"].cuda(), t["edge_index"].cuda(), t["edge_diff"].cuda(), t["edge_vec"].cuda())
    ((o["wh"].float().cuda() * h).sum() + (o["wX"].float().cuda() * X).sum()).backward()
    _check({n: p.grad for n, p in net.named_parameters()}, o["hx"], "h,X")


# ---------------------------------------------------------------------------------------------------- 6. QM9 read-outs
@pytest.mark.parametrize("tag", HEADS)
def test_qm9_readout_gradients_match_oracle_in_f16x2(tag, gemm_mode):
    t, sd, cot, _ = qm9_grad_kat()
    head = _kat_head(tag, sd)
    head.wgrad_mode = MODE
    inp, h, X = _kat_inputs(t)
    loss, _ = _kat_loss(head, inp, cot[tag])
    calls = _launches(loss.backward)
    assert "gn_weight_grad_group_mode" in calls and "gn_weight_grad_group" not in calls
    _compare(tag, head, h, X, _kat_oracle(tag), f"kat[{gemm_mode}, wgrad f16x2]")


@pytest.mark.parametrize("sact", [None, "silu"])
def test_standalone_block_matches_oracle_in_f16x2(sact):
    """The block of test_standalone_block_matches_oracle (no size but n_vin and n_hidden a multiple of 4)."""
    from gotennet_amd.outputs import GatedEquivariantBlock
    from oracle import gotennet_oracle as orc
    torch.manual_seed(13)
    N = 7
    blk = GatedEquivariantBlock(24, 20, 5, 3, 12, sactivation=sact)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.uniform_(-0.3, 0.3)
    sd64 = {k: v.double().requires_grad_(True) for k, v in blk.state_dict().items()}
    s64 = torch.randn(N, 24, dtype=torch.float64, requires_grad=True)
    v64 = torch.randn(N, 3, 20, dtype=torch.float64, requires_grad=True)
    so, vo = orc.gated_equivariant_block(sd64, "", s64, v64, "silu", sact)
    g = torch.Generator().manual_seed(2)
    cs, cv = torch.randn(so.shape, generator=g, dtype=torch.float64), torch.randn(vo.shape, generator=g, dtype=torch.float64)
    names = [n for n, _ in blk.named_parameters()]
    ref = torch.autograd.grad((cs * so).sum() + (cv * vo).sum(), [s64, v64] + [sd64[n] for n in names])
    blk = blk.cuda().eval()
    blk.parameter_grads, blk.wgrad_mode = True, MODE
    s = s64.detach().float().cuda().requires_grad_(True)
    v = v64.detach().float().cuda().requires_grad_(True)
    s_out, v_out = blk(s, v)
    loss = (cs.float().cuda() * s_out).sum() + (cv.float().cuda() * v_out).sum()
    calls = _launches(loss.backward)
    assert "gn_weight_grad_group_mode" in calls and "gn_weight_grad_group" not in calls
    got = [s.grad, v.grad] + [p.grad for p in blk.parameters()]
    for n, gv, r in zip(["scalars", "vectors"] + names, got, ref):
        assert gv.shape == r.shape, n
        e = _err(gv, r)
        print(f"block[sact={sact}, wgrad f16x2] {n}: {e:.3e}")
        assert e <= TOL, (n, e)
