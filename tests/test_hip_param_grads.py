"""GPU: parameter gradients (``parameter_grads``) against the fp64 oracle's autograd, the weight-gradient kernel against
fp64 torch, and the training semantics (accumulation, freezing, reproducibility, refusals, SGD steps)."""
import types

import pytest
import torch

from tests.golden_util import load_case, seeded_modules
from tests.test_hip_parity import _net_from_case
from tests.test_param_grads_host import ACCEPTED, FULL

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _err(a, b):
    """max-norm relative error of one parameter tensor against its own largest value."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    m = float(b.abs().max())
    return float((a - b).abs().max()) / m if m > 0 else float(a.abs().max())


def _head(cfg, head_sd):
    from gotennet_amd.outputs import Atomwise
    head = Atomwise(n_in=cfg["n_atom_basis"], n_hidden=cfg.get("head_hidden", 16), property="property", activation="silu")
    head.load_state_dict(head_sd, strict=True)
    return head.cuda().eval()


_ORACLE = {}


def _oracle(name):
    """fp64 autograd gradients of both losses w.r.t. every state_dict parameter (and the head's), cached per fixture."""
    if name in _ORACLE:
        return _ORACLE[name]
    from oracle import gotennet_oracle as orc
    cfg, sd, head_sd, t = load_case(name)
    net = _net_from_case(cfg, sd).cpu() if not cfg.get("seeded") else seeded_modules(cfg)[0]
    pnames = [n for n, _ in net.named_parameters()]
    sd64 = {k: (v.double().requires_grad_(k in pnames) if v.is_floating_point() else v) for k, v in sd.items()}
    hnames = [k for k in head_sd if k.startswith("out_net.")]             # (standardize.* are buffers)
    hd64 = {k: v.double().requires_grad_(k in hnames) for k, v in head_sd.items()}
    n_mol, N = int(t["batch"].max()) + 1, t["z"].shape[0]
    h, X = orc.gotennet_forward(sd64, cfg, t["z"], t["edge_index"], t["edge_diff"].double(), t["edge_vec"].double())
    g = torch.Generator().manual_seed(7)
    c = torch.randn(n_mol, 1, generator=g, dtype=torch.float64)
    wh = torch.randn(h.shape, generator=g, dtype=torch.float64)
    wX = torch.randn(X.shape, generator=g, dtype=torch.float64)
    e = orc.atomwise_energy(hd64, h, t["batch"], n_mol, "silu", z=t["z"])
    pp = [sd64[n] for n in pnames] + [hd64[k] for k in hnames]
    g1 = torch.autograd.grad((c * e).sum(), pp, retain_graph=True, allow_unused=True)
    g2 = torch.autograd.grad((wh * h).sum() + (wX * X).sum(), [sd64[n] for n in pnames], allow_unused=True)
    z0 = lambda gr, p: torch.zeros_like(p) if gr is None else gr
    out = dict(cfg=cfg, sd=sd, head_sd=head_sd, t=t, n_mol=n_mol, c=c, wh=wh, wX=wX,
               energy={n: z0(gr, p) for n, gr, p in zip(pnames + ["head." + k for k in hnames], g1, pp)},
               hx={n: z0(gr, sd64[n]) for n, gr in zip(pnames, g2)})
    _ORACLE[name] = out
    return out


def _gpu_modules(o):
    cfg = o["cfg"]
    if cfg.get("seeded"):
        net, _ = seeded_modules(cfg)
        net = net.cuda().eval()
    else:
        net = _net_from_case(cfg, o["sd"])
    head = _head(cfg, o["head_sd"])
    net.parameter_grads = head.parameter_grads = True
    return net, head


def _energy_loss(net, head, o, edges=None):
    t = o["t"]
    ei, ed, ev = edges or (t["edge_index"], t["edge_diff"], t["edge_vec"])
    h, X = net(t["z"].cuda(), ei.cuda(), ed.cuda(), ev.cuda())
    inp = types.SimpleNamespace(z=t["z"].cuda(), batch=t["batch"].cuda(), pos=None, representation=h)
    e = head(inp)["property"]
    return (o["c"].float().cuda() * e).sum()


def _grads(modules):
    return {f"{i}.{n}": (None if p.grad is None else p.grad.clone()) for i, m in enumerate(modules)
            for n, p in m.named_parameters()}


def _check(got, ref, what):
    for n, r in ref.items():
        gv = got[n]
        assert gv is not None, (what, n)
        zero = r == 0
        assert torch.equal(gv.detach().cpu()[zero], torch.zeros_like(gv.cpu()[zero])), (what, n, "exact zeros")
        e = _err(gv, r)
        assert e <= TOL, (what, n, e)


def _run_both_losses(name):
    o = _oracle(name)
    net, head = _gpu_modules(o)
    _energy_loss(net, head, o).backward()
    got = {n: p.grad for n, p in net.named_parameters()}
    got.update({"head." + n: p.grad for n, p in head.named_parameters()})
    _check(got, o["energy"], "energy")
    net.zero_grad(set_to_none=True)
    t = o["t"]
    h, X = net(t["z"].cuda(), t["edge_index"].cuda(), t["edge_diff"].cuda(), t["edge_vec"].cuda())
    ((o["wh"].float().cuda() * h).sum() + (o["wX"].float().cuda() * X).sum()).backward()
    _check({n: p.grad for n, p in net.named_parameters()}, o["hx"], "h,X")


# ---------------------------------------------------------------------------------------------------- kernel
def test_weight_grad_kernel_matches_fp64():
    from gotennet_amd import engine
    torch.manual_seed(0)
    dev = "cuda"
    probs, refs = [], []
    shapes = [(r, n, k) for r in (0, 1, 31, 33, 54373) for n in (1, 3, 33, 1536) for k in (20, 32, 257)]
    for i, (rows, nout, K) in enumerate(shapes):
        y_off, a_off = i % 3, (i * 5) % 7
        dY = torch.randn(max(rows, 1), nout + y_off + 2, device=dev)
        A = torch.randn(max(rows, 1), K + a_off + 1, device=dev)
        dW = torch.full((nout, K), float("nan"), device=dev)
        db = torch.full((nout,), float("nan"), device=dev)
        probs.append(dict(dY=dY, ldy=dY.shape[1], y_off=y_off, A=A, lda=A.shape[1], a_off=a_off, dW=dW, db=db,
                          rows=rows, nout=nout, K=K))
        yr, ar = dY[:rows, y_off:y_off + nout].double(), A[:rows, a_off:a_off + K].double()
        refs.append((yr.t() @ ar, yr.sum(0)))
    # a degree row map over X [N, D, F]: the rows of degree l = 2 (5 of D = 8)
    N, D, F = 1000, 8, 64
    gEK, X = torch.randn(N, D, F, device=dev), torch.randn(N, D, F, device=dev)
    dWk = torch.empty(F, F, device=dev)
    probs.append(dict(dY=gEK, ldy=F, A=X, lda=F, dW=dWk, rows=N * 5, nout=F, K=F, rowmap=(5, D, 3)))
    refs.append((gEK[:, 3:8].reshape(-1, F).double().t() @ X[:, 3:8].reshape(-1, F).double(), None))
    for i0 in range(0, len(probs), 16):
        engine.weight_grad_group(probs[i0:i0 + 16])
    first = [(q["dW"].clone(), None if q.get("db") is None else q["db"].clone()) for q in probs]
    for i0 in range(0, len(probs), 16):
        engine.weight_grad_group(probs[i0:i0 + 16])
    for q, (rw, rb), (w1, b1) in zip(probs, refs, first):
        assert _err(q["dW"], rw) <= 1e-5, (q["rows"], q["nout"], q["K"])
        assert torch.equal(q["dW"], w1)                          # bit-reproducible
        if rb is not None:
            assert _err(q["db"], rb) <= 1e-5, (q["rows"], q["nout"], q["K"])
            assert torch.equal(q["db"], b1)


# ---------------------------------------------------------------------------------------------------- parity
@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("name", ACCEPTED)
def test_fixture_parameter_gradients_match_oracle(name):
    _run_both_losses(name)


@pytest.mark.parametrize("name", FULL)
def test_full_size_parameter_gradients_match_oracle(name):
    _run_both_losses(name)


# ---------------------------------------------------------------------------------------------------- call paths
def test_unsorted_edges_give_the_same_gradients():
    cfg, sd, _, t = load_case("l2_sep_shuffled_noloop")
    net = _net_from_case(cfg, sd)
    net.parameter_grads = True
    order = torch.sort(t["edge_index"][1], stable=True).indices
    g = torch.Generator().manual_seed(3)
    wh = torch.randn(t["z"].shape[0], cfg["n_atom_basis"], generator=g).cuda()
    out = []
    for ei, ed, ev in ((t["edge_index"], t["edge_diff"], t["edge_vec"]),
                       (t["edge_index"][:, order], t["edge_diff"][order], t["edge_vec"][order])):
        net.zero_grad(set_to_none=True)
        h, X = net(t["z"].cuda(), ei.cuda(), ed.cuda(), ev.cuda())
        ((h * wh).sum() + X.sum()).backward()
        out.append(_grads([net]))
    for n in out[0]:
        assert torch.equal(out[0][n], out[1][n]), n


def test_wrapper_position_paths_give_identical_gradients():
    import gotennet_amd
    from gotennet_amd.outputs import Atomwise
    o = _oracle("l2_sep_f32")
    cfg, t = o["cfg"], o["t"]
    net = gotennet_amd.GotenNetWrapper(
        n_atom_basis=cfg["n_atom_basis"], n_interactions=cfg["n_interactions"], n_rbf=cfg["n_rbf"],
        cutoff_fn=gotennet_amd.CosineCutoff(cfg["cutoff"]), max_z=cfg["max_z"], num_heads=cfg["num_heads"],
        scale_edge=cfg["scale_edge"], lmax=cfg["lmax"], sep_dir=cfg["sep_dir"], sep_tensor=cfg["sep_tensor"])
    net.load_state_dict(o["sd"], strict=True)
    net = net.cuda().eval()
    out = []
    for forces in (False, True):
        head = Atomwise(n_in=cfg["n_atom_basis"], n_hidden=cfg.get("head_hidden", 16), property="property",
                        activation="silu", derivative="forces" if forces else None)
        head.load_state_dict(o["head_sd"], strict=True)
        head = head.cuda().eval()
        net.parameter_grads = head.parameter_grads = True
        net.zero_grad(set_to_none=True)
        pos = t["pos"].cuda().requires_grad_(forces)
        inp = types.SimpleNamespace(z=t["z"].cuda(), pos=pos, batch=t["batch"].cuda())
        inp.representation, inp.vector_representation = net(inp)
        box = []
        calls = _launches(lambda: box.append(head(inp)))
        res = box[0]
        if forces:                                 # logged forces: the input-gradient backward alone, the usual forces
            assert "gn_weight_grad_group" not in calls and "gn_message_backward" in calls
            assert _err(res["forces"], t["forces"]) <= TOL
        (o["c"].float().cuda() * res["property"]).sum().backward()
        out.append(_grads([net, head]))
    for n in out[0]:
        assert torch.equal(out[0][n], out[1][n]), n
    _check({k.split(".", 1)[1] if k.startswith("0.") else "head." + k.split(".", 1)[1]: v for k, v in out[0].items()},
           o["energy"], "wrapper")


def _launches(fn, calls=None):
    """The library entry points ``fn()`` calls, appended to ``calls`` (the per-launch timer hook, recording names only)."""
    from gotennet_amd import _lib
    calls = [] if calls is None else calls
    old = _lib.TIMER
    _lib.TIMER = types.SimpleNamespace(want=lambda name, args: calls.append(name), events=[])
    try:
        fn()
    finally:
        _lib.TIMER = old
    return calls


# (Atomwise kwargs, oracle) over the head branches: aggregation sum / mean / None, n_out > 1 with per-output
# standardisation, no hidden layer, two hidden layers; AtomwiseV3 with aggregation sum and None
HEADS = {
    "sum_2layers": dict(n_hidden=16),
    "mean": dict(n_hidden=16, aggregation_mode="mean", mean=torch.tensor([0.4]), stddev=torch.tensor([1.3])),
    "none": dict(n_hidden=16, aggregation_mode=None),
    "nout3": dict(n_out=3, n_hidden=16, mean=torch.tensor([0.1, -0.2, 0.3]), stddev=torch.tensor([1.5, 0.7, 2.0])),
    "nout3_mean": dict(n_out=3, n_hidden=16, aggregation_mode="mean"),
    "1layer": dict(n_layers=1),
    "3layers": dict(n_layers=3, n_hidden=[24, 8]),
    "v3_sum": dict(v3=True, n_hidden=16, mean=0.3, stddev=1.7),
    "v3_none": dict(v3=True, n_hidden=16, aggregation_mode=None, mean=-0.2, stddev=0.9),
}


@pytest.mark.parametrize("kind", list(HEADS))
def test_head_parameter_gradients_match_oracle(kind):
    """Every branch of the head's parameter gradients (and its dL/dh) against fp64 autograd through the oracle's heads."""
    from gotennet_amd.outputs import Atomwise, AtomwiseV3
    from oracle import gotennet_oracle as orc
    kw = dict(HEADS[kind])
    v3 = kw.pop("v3", False)
    torch.manual_seed(11)
    F, n_mol, per = 32, 3, 7
    N = n_mol * per
    batch, z = torch.arange(n_mol).repeat_interleave(per), torch.randint(1, 9, (N,))
    head = (AtomwiseV3 if v3 else Atomwise)(n_in=F, activation="silu", **kw)
    with torch.no_grad():
        for p in head.parameters():
            if p.dim() == 1:
                p.uniform_(-0.3, 0.3)
            else:
                p.mul_(1.5)
    hsd = {k: v.double().requires_grad_(k.startswith("out_net.")) for k, v in head.state_dict().items()}
    names = [n for n, _ in head.named_parameters()]
    h64 = torch.randn(N, F, dtype=torch.float64, requires_grad=True)
    agg = kw.get("aggregation_mode", "sum")
    if v3:
        y_ref, _ = orc.atomwise_v3(hsd, h64, batch, n_mol, kw["mean"], kw["stddev"], "silu", z=z, aggregation=agg)
    elif agg is None:
        y_ref = orc.atomwise_contributions(hsd, h64, z, "silu")
    else:
        y_ref = orc.atomwise_energy(hsd, h64, batch, n_mol, "silu", z=z, aggregation=agg)
    c = torch.randn(y_ref.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    ref = torch.autograd.grad((c * y_ref).sum(), [h64] + [hsd[n] for n in names])
    head = head.cuda().eval()
    head.parameter_grads = True
    h = h64.detach().float().cuda().requires_grad_(True)
    y = head(types.SimpleNamespace(z=z.cuda(), batch=batch.cuda(), pos=None, representation=h))["y"]
    assert y.shape == y_ref.shape
    (c.float().cuda() * y).sum().backward()
    assert _err(h.grad, ref[0]) <= TOL, "dL/dh"
    for (n, p), r in zip(head.named_parameters(), ref[1:]):
        assert _err(p.grad, r) <= TOL, n


# ---------------------------------------------------------------------------------------------------- semantics
def test_freezing_accumulation_and_reproducibility():
    o = _oracle("l2_sep_f32")
    net, head = _gpu_modules(o)
    _energy_loss(net, head, o).backward()
    base = _grads([net, head])
    net.zero_grad(set_to_none=True)
    head.zero_grad(set_to_none=True)
    _energy_loss(net, head, o).backward()
    again = _grads([net, head])
    for n in base:
        assert torch.equal(base[n], again[n]), n                 # bit-reproducible
    net.zero_grad(set_to_none=True)
    head.zero_grad(set_to_none=True)
    loss = _energy_loss(net, head, o)
    loss.backward(retain_graph=True)
    loss.backward()
    for n, v in _grads([net, head]).items():
        assert torch.equal(v, 2 * base[n]), n                    # autograd accumulates
    net.zero_grad(set_to_none=True)
    head.zero_grad(set_to_none=True)
    net.A_na.requires_grad_(False)
    net.gata_list[0].requires_grad_(False)
    _energy_loss(net, head, o).backward()
    frozen = {id(p) for p in [net.A_na.weight, *net.gata_list[0].parameters()]}
    for i, mod in enumerate([net, head]):
        for n, p in mod.named_parameters():
            if id(p) in frozen:
                assert p.grad is None, n
            else:
                assert torch.equal(p.grad, base[f"{i}.{n}"]), n
    net.requires_grad_(True)


def test_second_order_and_unsupported_configurations_are_refused():
    import gotennet_amd
    from gotennet_amd.outputs import Atomwise
    o = _oracle("l2_sep_f32")
    cfg, t = o["cfg"], o["t"]
    net = gotennet_amd.GotenNetWrapper(
        n_atom_basis=cfg["n_atom_basis"], n_interactions=cfg["n_interactions"], n_rbf=cfg["n_rbf"],
        cutoff_fn=gotennet_amd.CosineCutoff(cfg["cutoff"]), max_z=cfg["max_z"], num_heads=cfg["num_heads"],
        scale_edge=cfg["scale_edge"], lmax=cfg["lmax"], sep_dir=cfg["sep_dir"], sep_tensor=cfg["sep_tensor"]).cuda().eval()
    head = Atomwise(n_in=cfg["n_atom_basis"], n_hidden=16, activation="silu").cuda().eval()
    net.parameter_grads = head.parameter_grads = True
    pos = t["pos"].cuda().requires_grad_(True)
    inp = types.SimpleNamespace(z=t["z"].cuda(), pos=pos, batch=t["batch"].cuda())
    inp.representation, _ = net(inp)
    e = head(inp)["y"]
    with pytest.raises(NotImplementedError, match="second-order"):
        torch.autograd.grad(e.sum(), pos, create_graph=True)
    # composed edge update: refused before any launch (the library is never entered)
    ccfg, csd, _, ct = load_case("opt_mlpa_linw_postln")
    cnet = _net_from_case(ccfg, csd)
    cnet.parameter_grads = True
    from gotennet_amd import _lib
    calls = []
    old = _lib.TIMER
    _lib.TIMER = types.SimpleNamespace(want=lambda name, args: calls.append(name), events=[])
    try:
        with pytest.raises(NotImplementedError, match="composed edge updates"):
            cnet(ct["z"].cuda(), ct["edge_index"].cuda(), ct["edge_diff"].cuda(), ct["edge_vec"].cuda())
    finally:
        _lib.TIMER = old
    assert calls == []
    # ... and through the wrapper without a position gradient: refused before the radius graph is built
    wnet = gotennet_amd.GotenNetWrapper(
        n_atom_basis=ccfg["n_atom_basis"], n_interactions=ccfg["n_interactions"], n_rbf=ccfg["n_rbf"],
        cutoff_fn=gotennet_amd.CosineCutoff(ccfg["cutoff"]), max_z=ccfg["max_z"], num_heads=ccfg["num_heads"],
        lmax=ccfg["lmax"], edge_updates=ccfg["edge_updates"], sep_htr=ccfg.get("sep_htr", True)).cuda().eval()
    wnet.parameter_grads = True
    winp = types.SimpleNamespace(z=ct["z"].cuda(), pos=ct["pos"].cuda(), batch=ct["batch"].cuda())
    calls = []
    with pytest.raises(NotImplementedError, match="composed edge updates"):
        _launches(lambda: wnet(winp), calls)
    assert calls == []


# ---------------------------------------------------------------------------------------------------- training
def test_three_sgd_steps_match_the_oracle():
    from oracle import gotennet_oracle as orc
    o = _oracle("l2_sep_f32")
    cfg, t = o["cfg"], o["t"]
    net, head = _gpu_modules(o)
    target = torch.randn(o["n_mol"], 1, generator=torch.Generator().manual_seed(5))
    lr = 1e-3
    params = list(net.parameters()) + list(head.parameters())
    p0 = [p.detach().clone() for p in params]
    opt = torch.optim.SGD(params, lr=lr)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        h, X = net(t["z"].cuda(), t["edge_index"].cuda(), t["edge_diff"].cuda(), t["edge_vec"].cuda())
        e = head(types.SimpleNamespace(z=t["z"].cuda(), batch=t["batch"].cuda(), pos=None, representation=h))["property"]
        loss = ((e - target.cuda()) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[2] < losses[0]
    # the same three steps in fp64 on the oracle
    pnames = [n for n, _ in net.named_parameters()]
    sd = {k: v.double() for k, v in o["sd"].items() if v.is_floating_point()}
    sd.update({k: v for k, v in o["sd"].items() if not v.is_floating_point()})
    hd = {k: v.double() for k, v in o["head_sd"].items()}
    leaves = [sd[n] for n in pnames] + [hd[k] for k, _ in head.named_parameters()]
    start = [v.clone() for v in leaves]
    for _ in range(3):
        for v in leaves:
            v.requires_grad_(True)
        h, _ = orc.gotennet_forward(sd, cfg, t["z"], t["edge_index"], t["edge_diff"].double(), t["edge_vec"].double())
        e = orc.atomwise_energy(hd, h, t["batch"], o["n_mol"], "silu", z=t["z"])
        gr = torch.autograd.grad(((e - target.double()) ** 2).mean(), leaves, allow_unused=True)
        with torch.no_grad():
            for v, gv in zip(leaves, gr):
                if gv is not None:
                    v -= lr * gv
        for v in leaves:
            v.detach_()
    # (the fp32 parameters round each update: that rounding, 2^-24 of |p| per step, is allowed on top)
    for (n, p), a, v, s in zip(list(net.named_parameters()) + list(head.named_parameters()), p0, leaves, start):
        ref = v - s
        got = (p.detach() - a).double().cpu()
        err = float((got - ref).abs().max())
        assert err <= TOL * float(ref.abs().max()) + 3 * 2.0 ** -24 * float(s.abs().max()), (n, err)
