"""GPU: training the QM9 vector read-outs (``Dipole``, ``ElectronicSpatialExtentV2``, ``GatedEquivariantBlock`` with
``parameter_grads``) against the fp64 oracle's autograd: the reference KAT in all three arithmetics, degenerate points
(zero vector norms, a zero molecular dipole), a stand-alone block, the three QM9 heads on the representation in one
loss, the training semantics and three SGD steps."""
import types

import pytest
import torch

from tests.test_hip_param_grads import TOL, _err, _launches
from tests.test_qm9_training_host import HEADS, oracle_grads, qm9_grad_kat

pytestmark = pytest.mark.gpu


def _kat_head(tag, sd, mean=0.3):
    import gotennet_amd.outputs as out
    if tag == "dip_task":
        m = out.Dipole(n_in=64, predict_magnitude=True, property="property", mean=torch.tensor(mean), stddev=torch.tensor(1.7))
    elif tag == "dip_vec":
        m = out.Dipole(n_in=64, n_hidden=32, property="dipole")
    else:
        m = out.ElectronicSpatialExtentV2(n_in=64, property="property", contributions="contrib")
    m.load_state_dict(sd[tag], strict=True)
    m = m.cuda().eval()
    m.parameter_grads = True
    return m


def _kat_inputs(t, h=None, X=None, pos=None, grad=True):
    h = (t["h"] if h is None else h).cuda().requires_grad_(grad)
    X = (t["X"] if X is None else X).cuda().requires_grad_(grad)        # passed whole: the head takes the X[:, :3] view
    inp = types.SimpleNamespace(z=t["z"].cuda(), batch=t["batch"].cuda(), pos=(t["pos"] if pos is None else pos).cuda(),
                                representation=h, vector_representation=X)
    return inp, h, X


def _kat_loss(head, inp, cot):
    res = head(inp)
    return sum((c.float().cuda() * res[o]).sum() for o, c in cot.items()), res


def _compare(tag, head, h, X, ref, what):
    """Every gradient finite and within TOL of the fp64 autograd's; dL/dX exact zeros in rows 3 and above."""
    got = {"h": h.grad, "X": X.grad if X.grad is not None else torch.zeros_like(X)}
    got.update({n: p.grad for n, p in head.named_parameters()})
    assert sorted(got) == sorted(ref)
    assert torch.equal(got["X"][:, 3:], torch.zeros_like(got["X"][:, 3:])), (what, tag, "dL/dX[:, 3:]")
    for n, r in ref.items():
        assert got[n] is not None, (what, tag, n)
        assert bool(torch.isfinite(got[n]).all()), (what, tag, n, "not finite")
        e = _err(got[n], r)
        print(f"{what} {tag} {n}: {e:.3e}")
        assert e <= TOL, (what, tag, n, e)


_KAT_ORACLE = {}


def _kat_oracle(tag):
    if tag not in _KAT_ORACLE:
        t, sd, cot, _ = qm9_grad_kat()
        _KAT_ORACLE[tag] = oracle_grads(tag, t, sd[tag], cot[tag])
    return _KAT_ORACLE[tag]


# ---------------------------------------------------------------------------------------------------- 1. KAT
@pytest.mark.parametrize("tag", HEADS)
def test_kat_gradients_match_oracle(tag, gemm_mode):
    """N = 24 (molecules of 9, 1 and 14 atoms), F = 64, D = 8: dL/dh, dL/dX and every parameter.  Covers the
    n_vout = n_sout = 1 padding of the second block, n_hidden != n_in (dip_vec) and a one-atom molecule."""
    t, sd, cot, _ = qm9_grad_kat()
    head = _kat_head(tag, sd)
    inp, h, X = _kat_inputs(t)
    loss, res = _kat_loss(head, inp, cot[tag])
    assert all(res[o].grad_fn is not None for o in cot[tag])
    loss.backward()
    _compare(tag, head, h, X, _kat_oracle(tag), f"kat[{gemm_mode}]")


# ---------------------------------------------------------------------------------------------------- 2. degenerate points
@pytest.mark.parametrize("tag", HEADS)
def test_zero_norm_points_have_finite_matching_gradients(tag):
    """One atom with X[:, :3] = 0 (every ||V_f|| of the first block is 0 there: torch.norm's subgradient 0); for the
    magnitude head also the one-atom molecule with X = 0, pos = 0 and mean = 0, whose dipole is exactly 0."""
    t, sd, cot, _ = qm9_grad_kat()
    X, pos, mean = t["X"].clone(), t["pos"].clone(), 0.3
    X[4, :3] = 0.0
    if tag == "dip_task":
        X[9], pos[9], mean = 0.0, 0.0, 0.0               # atom 9 is the whole of molecule 1
    head = _kat_head(tag, sd, mean=mean)
    inp, h, Xg = _kat_inputs(t, X=X, pos=pos)
    loss, res = _kat_loss(head, inp, cot[tag])
    if tag == "dip_task":
        assert float(res["property"][1].detach()) == 0.0
    loss.backward()
    _compare(tag, head, h, Xg, oracle_grads(tag, t, sd[tag], cot[tag], X=X, pos=pos, mean=mean), "degenerate")


# ---------------------------------------------------------------------------------------------------- 3. stand-alone block
@pytest.mark.parametrize("sact", [None, "silu"])
def test_standalone_block_matches_oracle(sact):
    """No size but n_vin and n_hidden a multiple of 4: pads of 1 (V / W halves), 1 (ctx) and 0 (x)."""
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
    blk.parameter_grads = True
    s = s64.detach().float().cuda().requires_grad_(True)
    v = v64.detach().float().cuda().requires_grad_(True)
    s_out, v_out = blk(s, v)
    assert s_out.shape == so.shape and v_out.shape == vo.shape
    assert _err(s_out, so) <= TOL and _err(v_out, vo) <= TOL
    ((cs.float().cuda() * s_out).sum() + (cv.float().cuda() * v_out).sum()).backward()
    got = [s.grad, v.grad] + [p.grad for p in blk.parameters()]
    for n, gv, r in zip(["scalars", "vectors"] + names, got, ref):
        assert gv.shape == r.shape, n
        e = _err(gv, r)
        print(f"block[sact={sact}] {n}: {e:.3e}")
        assert e <= TOL, (n, e)


# ---------------------------------------------------------------------------------------------------- 4. / 6. end to end
_KW = dict(n_atom_basis=32, n_interactions=2, n_rbf=8, num_heads=8, scale_edge=False, lmax=2, sep_dir=True, sep_tensor=True)


def _qm9_model():
    """The model of test_qm9_heads_on_the_representation_match_oracle (F = 32, L = 2, lmax = 2, 2 x 9 atoms) with the three
    heads of the QM9 task -> (modules on the host, their fp64 state dicts, the batch)."""
    import gotennet_amd
    import gotennet_amd.outputs as out
    from tests.test_hip_parity import _synthetic
    torch.manual_seed(7)
    net = gotennet_amd.GotenNetWrapper(cutoff_fn=gotennet_amd.CosineCutoff(5.0), **_KW)
    heads = dict(mu=out.Dipole(n_in=32, predict_magnitude=True, property="mu"),
                 r2=out.ElectronicSpatialExtentV2(n_in=32, property="r2"),
                 u0=out.Atomwise(n_in=32, n_hidden=16, property="u0", activation="silu"))
    with torch.no_grad():
        for m in heads.values():
            for p in m.parameters():
                if p.dim() == 1:
                    p.uniform_(-0.3, 0.3)
    mods = dict(net=net, **heads)
    sds = {k: {n: v.clone().double() for n, v in m.state_dict().items()} for k, m in mods.items()}
    pos, batch, z = _synthetic(2, 9, 3.0, seed=3)
    return mods, sds, (pos, batch, z.clamp(max=9))


def _param_names(mods):
    return {k: [n for n, _ in m.named_parameters()] for k, m in mods.items()}


def _oracle_qm9(sds, data, edges=None, which=("mu", "r2", "u0")):
    """The oracle's read-outs from fp64 state dicts (``edges``: a fixed radius graph)."""
    from oracle import gotennet_oracle as orc
    pos, batch, z = data
    ei, w, vec = edges or orc.distance(pos.double(), batch, 5.0)
    h, X = orc.gotennet_forward(sds["net"], orc.default_config(**_KW), z, ei, w, vec)
    out = {}
    if "mu" in which:
        out["mu"], _ = orc.dipole(sds["mu"], h, X, pos.double(), batch, 2, "silu", predict_magnitude=True)
    if "r2" in which:
        out["r2"], _ = orc.electronic_spatial_extent(sds["r2"], h, pos.double(), z, batch, 2, "softplus")
    if "u0" in which:
        out["u0"] = orc.atomwise_energy(sds["u0"], h, batch, 2, "silu", z=z)
    return out


def _gpu_qm9(mods, data):
    pos, batch, z = data
    for m in mods.values():
        m.cuda().eval()
        m.parameter_grads = True
    inp = types.SimpleNamespace(z=z.cuda(), pos=pos.cuda(), batch=batch.cuda())

    def run(which=("mu", "r2", "u0")):
        inp.representation, inp.vector_representation = mods["net"](inp)
        return {k: mods[k](inp)[k] for k in which}
    return run


def test_three_heads_in_one_loss_match_oracle():
    mods, sds, data = _qm9_model()
    names = _param_names(mods)
    for k, sd in sds.items():
        for n in names[k]:
            sd[n].requires_grad_(True)
    g = torch.Generator().manual_seed(9)
    cot = {k: torch.randn(2, 1, generator=g, dtype=torch.float64) for k in ("mu", "r2", "u0")}
    out64 = _oracle_qm9(sds, data)
    leaves = [(k, n) for k in mods for n in names[k]]
    gr = torch.autograd.grad(sum((cot[k] * out64[k]).sum() for k in cot), [sds[k][n] for k, n in leaves], allow_unused=True)
    ref = {kn: (torch.zeros_like(sds[kn[0]][kn[1]]) if v is None else v) for kn, v in zip(leaves, gr)}
    run = _gpu_qm9(mods, data)
    counts = {}
    for which in (("mu", "r2", "u0"), ("mu",)):
        for m in mods.values():
            m.zero_grad(set_to_none=True)
        out = run(which)
        loss = sum((cot[k].float().cuda() * out[k]).sum() for k in which)
        calls = _launches(loss.backward)
        counts[which] = calls.count("gn_message_backward")
        if len(which) == 3:
            for k in which:
                assert _err(out[k], out64[k]) <= TOL, k
            for (k, n), r in ref.items():
                gv = dict(mods[k].named_parameters())[n].grad
                assert gv is not None or not r.any(), (k, n)
                e = _err(torch.zeros_like(r) if gv is None else gv, r)
                print(f"end-to-end {k}.{n}: {e:.3e}")
                assert e <= TOL, (k, n, e)
            for name in ("gn_geb_gate_backward", "gn_geb_context_backward", "gn_dipole_reduce_backward",
                         "gn_ese_reduce_backward"):
                assert name in calls, name
    # the representation's backward ran once for the three heads: as many message backwards as for one head
    assert counts[("mu", "r2", "u0")] == counts[("mu",)] > 0


def test_three_sgd_steps_on_mu_and_r2_match_the_oracle():
    mods, sds, data = _qm9_model()
    del mods["u0"], sds["u0"]
    names = _param_names(mods)
    target = {k: torch.randn(2, 1, generator=torch.Generator().manual_seed(5 + i)) for i, k in enumerate(("mu", "r2"))}
    # the dipole is taken about the origin and the second molecule sits 20 A away: gradients reach 3e4, and the fp64 oracle
    # alone diverges at 1e-5; at 1e-6 its loss falls 4186 -> 1852 -> 840 and the median parameter moves by 1 % in 3 steps
    lr = 1e-6
    run = _gpu_qm9(mods, data)
    params = [p for m in mods.values() for p in m.parameters()]
    p0 = [p.detach().clone() for p in params]
    opt = torch.optim.SGD(params, lr=lr)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = run(("mu", "r2"))
        loss = sum(((out[k] - target[k].cuda()) ** 2).mean() for k in target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", losses)
    assert losses[2] < losses[0]
    # the same three steps in fp64 on the oracle (fixed edge list: the radius graph does not change with the weights)
    from oracle import gotennet_oracle as orc
    edges = orc.distance(data[0].double(), data[1], 5.0)
    leaves = [sds[k][n] for k in mods for n in names[k]]
    start = [v.clone() for v in leaves]
    for _ in range(3):
        for v in leaves:
            v.requires_grad_(True)
        out = _oracle_qm9(sds, data, edges, which=("mu", "r2"))
        gr = torch.autograd.grad(sum(((out[k] - target[k].double()) ** 2).mean() for k in target), leaves, allow_unused=True)
        with torch.no_grad():
            for v, gv in zip(leaves, gr):
                if gv is not None:
                    v -= lr * gv
        for v in leaves:
            v.detach_()
    # the bound of test_three_sgd_steps_match_the_oracle (the fp32 parameters round each update: 2^-24 of |p| per step)
    labels = [f"{k}.{n}" for k in mods for n in names[k]]
    for n, p, a, v, s in zip(labels, params, p0, leaves, start):
        ref = v - s
        got = (p.detach() - a).double().cpu()
        err = float((got - ref).abs().max())
        assert err <= TOL * float(ref.abs().max()) + 3 * 2.0 ** -24 * float(s.abs().max()), (n, err)


# ---------------------------------------------------------------------------------------------------- 5. semantics
def _kat_grads(head, t, cot, freeze=None, twice=False):
    head.zero_grad(set_to_none=True)
    inp, h, X = _kat_inputs(t)
    loss, _ = _kat_loss(head, inp, cot)
    if twice:
        loss.backward(retain_graph=True)
    loss.backward()
    out = {"h": h.grad, "X": X.grad}
    out.update({n: p.grad for n, p in head.named_parameters()})
    return out


@pytest.mark.parametrize("tag", ["dip_task", "ese"])
def test_reproducible_accumulating_and_freezable(tag):
    t, sd, cot, _ = qm9_grad_kat()
    head = _kat_head(tag, sd)
    base = _kat_grads(head, t, cot[tag])
    again = _kat_grads(head, t, cot[tag])
    for n in base:
        if base[n] is None:                              # (ESE does not read X)
            assert again[n] is None and n == "X" and tag == "ese"
            continue
        assert torch.equal(base[n], again[n]), n         # bit-reproducible
    twice = _kat_grads(head, t, cot[tag], twice=True)
    for n in base:
        if base[n] is not None:
            assert torch.equal(twice[n], 2 * base[n]), n  # autograd accumulates
    frozen = (head.equivariant_layers[0].mix_vectors if tag == "dip_task" else head.out_net[1].out_net[0]).weight
    frozen.requires_grad_(False)
    part = _kat_grads(head, t, cot[tag])
    for n, p in head.named_parameters():
        if p is frozen:
            assert part[n] is None, n
        else:
            assert torch.equal(part[n], base[n]), n
    assert torch.equal(part["h"], base["h"])


@pytest.mark.parametrize("tag", HEADS)
def test_default_path_is_unchanged(tag):
    """``parameter_grads = False``: today's launches, today's bits, no grad_fn -- whatever requires grad."""
    t, sd, cot, _ = qm9_grad_kat()
    head = _kat_head(tag, sd)
    inp, _, _ = _kat_inputs(t)
    with torch.no_grad():                                # grad mode off: the default path
        head(inp)                                        # (the first call also packs the weights)
        want_calls = _launches(lambda: head(inp))
        want = head(inp)
    head.parameter_grads = False
    assert head.parameter_grads is False
    box = []
    calls = _launches(lambda: box.append(head(inp)))
    assert calls == want_calls
    assert not any(c.endswith("_backward") for c in calls)
    for k, v in want.items():
        assert torch.equal(box[0][k], v), k
        assert box[0][k].grad_fn is None and not box[0][k].requires_grad, k
    # the trainable path computes the same outputs and keeps ``contributions`` detached
    head.parameter_grads = True
    res = head(inp)
    for o in cot[tag]:
        assert res[o].grad_fn is not None and _err(res[o], want[o]) <= 1e-6, o
    if tag == "ese":
        assert res["contrib"].grad_fn is None and torch.equal(res["contrib"], want["contrib"])


@pytest.mark.parametrize("tag", HEADS)
def test_refusals_come_before_any_launch(tag):
    t, sd, cot, _ = qm9_grad_kat()
    head = _kat_head(tag, sd)
    # positions are data in this mode
    inp, _, _ = _kat_inputs(t)
    inp.pos = inp.pos.clone().requires_grad_(True)
    calls = []
    with pytest.raises(NotImplementedError, match="pos"):
        _launches(lambda: head(inp), calls)
    assert calls == []
    # ... but not on the default path, where they are detached as before
    head.parameter_grads = False
    head(inp)
    head.parameter_grads = True
    # a backward that would need its own derivative
    inp, h, _ = _kat_inputs(t)
    loss, _ = _kat_loss(head, inp, cot[tag])
    calls = []
    with pytest.raises(NotImplementedError, match="second-order"):
        _launches(lambda: torch.autograd.grad(loss, h, create_graph=True), calls)
    assert calls == []
