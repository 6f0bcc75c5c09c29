"""GPU: attention dropout in training mode -- the mask kernel against the numpy restatement of its definition, and the
forward, the forces and the parameter gradients against the fp64 oracle with the SAME masks applied to its segment
softmax (the oracle has no dropout: ``dropout_util.patch_oracle_softmax``).  Every fixture's edge list is target-sorted,
so the caller's edge order is the internal order the mask is defined on."""
import types

import numpy as np
import pytest
import torch

from tests import test_hip_param_grads as tpg
from tests.dropout_util import mask_reference, patch_oracle_softmax
from tests.golden_util import load_case, rel_err
from tests.test_hip_parity import _net_from_case, _synthetic

pytestmark = pytest.mark.gpu

TOL = 1e-4
SEED = 20240
FIXTURES = ["l1_nosep_scale_f32", "l2_sep_f32", "l3_sep_scale_f32", "l4_sep_f32", "l5_sep_f32", "opt_act_ssp",
            "opt_aggr_mean_l2", "opt_aggr_max_l3"]
WIDE = "wide512"


# ---------------------------------------------------------------------------------------------------- helpers
def _set_dropout(net, p, train=True):
    net.attn_dropout = p
    for g in net.gata_list:
        g.dropout = p
    return net.train(train)


_WIDE = {}


def _wide_case():
    """One seeded F = 512 model (the workgroup-per-target softmax kernel, the wide-slot backward), built as
    test_forces_match_oracle_wide builds its model: -> (cfg, sd, head_sd, t) like a fixture."""
    if not _WIDE:
        import gotennet_amd
        from gotennet_amd.outputs import Atomwise
        from oracle import gotennet_oracle as orc
        F, L, lmax = 512, 2, 2
        torch.manual_seed(F + lmax)
        net = gotennet_amd.GotenNet(n_atom_basis=F, n_interactions=L, n_rbf=32, cutoff_fn=gotennet_amd.CosineCutoff(5.0),
                                    num_heads=8, scale_edge=False, lmax=lmax, sep_dir=True, sep_tensor=True)
        head = Atomwise(n_in=F, n_hidden=16, property="property", activation="silu")
        with torch.no_grad():
            for m in (net, head):
                for n, p in m.named_parameters():
                    if p.dim() == 1:
                        p.uniform_(-0.05, 0.05) if "norm.weight" not in n else p.uniform_(0.9, 1.1)
        cfg = orc.default_config(n_atom_basis=F, n_interactions=L, n_rbf=32, num_heads=8, scale_edge=False, lmax=lmax,
                                 sep_dir=True, sep_tensor=True)
        cfg.update(max_z=100, n_mol=3)
        pos, batch, z = _synthetic(3, 14, 4.0, seed=F)
        ei, w, vec = orc.distance(pos, batch, 5.0, 32)
        _WIDE["case"] = (cfg, {k: v.clone() for k, v in net.state_dict().items()},
                         {k: v.clone() for k, v in head.state_dict().items()},
                         dict(z=z, pos=pos, batch=batch, edge_index=ei, edge_diff=w, edge_vec=vec))
    return _WIDE["case"]


def _case(name):
    cfg, sd, head_sd, t = _wide_case() if name == WIDE else load_case(name)
    tgt = t["edge_index"][1]
    assert bool((tgt[1:] >= tgt[:-1]).all()), "fixture edge list is not target-sorted"
    return cfg, sd, head_sd, t


def _masks(net, E, p):
    from gotennet_amd import attention_dropout_mask
    return [attention_dropout_mask(net.last_dropout_key, li, E, net.num_heads, p).cpu() for li in range(net.n_interactions)]


def _d64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _edges_from_pos(pos, ei):
    """edge_vec = pos[j] - pos[i] and its length (0 on self-loops, whose norm autograd never sees), as orc.distance."""
    vec = pos[ei[0]] - pos[ei[1]]
    loop = (ei[0] == ei[1])
    safe = torch.where(loop.unsqueeze(1), torch.ones_like(vec), vec)
    return torch.where(loop, torch.zeros_like(vec[:, 0]), torch.norm(safe, dim=-1)), vec


_REF = {}


def _oracle_forward(monkeypatch, name, key, masks):
    """(h, X) of the masked fp64 oracle on the fixture's own edge arrays; computed once per (fixture, key)."""
    from oracle import gotennet_oracle as orc
    ck = ("fwd", name, key)
    if ck not in _REF:
        cfg, sd, _, t = _case(name)
        count = patch_oracle_softmax(monkeypatch, masks)
        with torch.no_grad():
            _REF[ck] = orc.gotennet_forward(_d64(sd), cfg, t["z"], t["edge_index"], t["edge_diff"].double(),
                                            t["edge_vec"].double())
        assert count[0] == cfg["n_interactions"]                  # one softmax call per interaction
    return _REF[ck]


def _oracle_forces(monkeypatch, name, key, masks):
    """(energy, -dE/dpos) of the masked fp64 oracle with the fixture's edge LIST and geometry from ``pos``."""
    from oracle import gotennet_oracle as orc
    ck = ("forces", name, key)
    if ck not in _REF:
        cfg, sd, head_sd, t = _case(name)
        count = patch_oracle_softmax(monkeypatch, masks)
        pos = t["pos"].double().requires_grad_(True)
        w, vec = _edges_from_pos(pos, t["edge_index"])
        h, _ = orc.gotennet_forward(_d64(sd), cfg, t["z"], t["edge_index"], w, vec)
        n_mol = int(t["batch"].max()) + 1
        e = orc.atomwise_energy(_d64(head_sd), h, t["batch"], n_mol, "silu", z=t["z"])
        (g,) = torch.autograd.grad(e.sum(), pos)
        assert count[0] == cfg["n_interactions"]
        _REF[ck] = (e.detach(), -g)
    return _REF[ck]


def _key_of(net):
    return tuple(int(v) for v in net.last_dropout_key.cpu())


def _gpu_forces(net, head, t):
    pos = t["pos"].cuda().requires_grad_(True)
    ei = t["edge_index"].cuda()
    w, vec = _edges_from_pos(pos, ei)
    h, _ = net(t["z"].cuda(), ei, w, vec)
    e = head(types.SimpleNamespace(z=t["z"].cuda(), batch=t["batch"].cuda(), pos=None, representation=h))["property"]
    (g,) = torch.autograd.grad(e.sum(), pos)
    return e.detach(), -g


def _modules(name, p, train=True):
    cfg, sd, head_sd, t = _case(name)
    net = _net_from_case(cfg, sd).requires_grad_(False)           # (forces only: no parameter wants a gradient)
    return cfg, t, _set_dropout(net, p, train), tpg._head(cfg, head_sd).requires_grad_(False)


# ---------------------------------------------------------------------------------------------------- 1. mask kernel
@pytest.mark.parametrize("seed", [1234, -7, (0x5EED1234 << 32) | 0x0BADF00D])
def test_mask_kernel_matches_numpy(seed):
    """Bit-exact against the numpy restatement of the definition; a key with a non-zero high half (and a negative one,
    whose high half is all ones) included; two layers differ."""
    from gotennet_amd import attention_dropout_mask
    key = torch.tensor([seed, 99], dtype=torch.int64).cuda()       # (the reserved second value is ignored)
    for E in (0, 1, 77):
        for H in (1, 4, 8):
            for p in (0.0, 0.1, 0.5, 1.0):
                got = [attention_dropout_mask(key, layer, E, H, p).cpu().numpy() for layer in (0, 3)]
                for layer, g in zip((0, 3), got):
                    ref = mask_reference(seed, layer, E, H, p)
                    assert g.shape == (E, H) and g.dtype == np.float32
                    assert np.array_equal(g.view(np.uint32), ref.view(np.uint32)), (E, H, p, layer)
                if E == 77 and 0 < p < 1:
                    assert not np.array_equal(got[0], got[1])
    # a different reserved value: the same mask
    key2 = torch.tensor([seed, 0], dtype=torch.int64).cuda()
    assert torch.equal(attention_dropout_mask(key, 1, 77, 8, 0.5), attention_dropout_mask(key2, 1, 77, 8, 0.5))


# ---------------------------------------------------------------------------------------------------- 2. forward
@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", FIXTURES + [WIDE])
def test_forward_matches_masked_oracle(monkeypatch, name, p):
    cfg, t, net, _ = _modules(name, p)
    torch.manual_seed(SEED)
    with torch.no_grad():
        h, X = net(t["z"].cuda(), t["edge_index"].cuda(), t["edge_diff"].cuda(), t["edge_vec"].cuda())
    masks = _masks(net, t["edge_index"].shape[1], p)
    assert all(0 < float((m == 0).float().mean()) < 1 for m in masks)          # something was dropped, something kept
    h_ref, X_ref = _oracle_forward(monkeypatch, name, (p,) + _key_of(net), masks)
    eh, eX = rel_err(h.cpu(), h_ref), rel_err(X.cpu(), X_ref)
    print(f"{name} p={p}: h {eh:.2e} X {eX:.2e}")
    assert eh < TOL and eX < TOL


# ---------------------------------------------------------------------------------------------------- 3. forces
@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("name", FIXTURES + [WIDE])
def test_forces_match_masked_oracle(monkeypatch, name):
    p = 0.1
    cfg, t, net, head = _modules(name, p)
    torch.manual_seed(SEED)
    e, f = _gpu_forces(net, head, t)
    masks = _masks(net, t["edge_index"].shape[1], p)
    e_ref, f_ref = _oracle_forces(monkeypatch, name, (p,) + _key_of(net), masks)
    ee, ef = rel_err(e.cpu(), e_ref), rel_err(f.cpu(), f_ref)
    print(f"{name}: energy {ee:.2e} forces {ef:.2e}")
    assert ee < TOL and ef < TOL


@pytest.mark.parametrize("name", ["l2_sep_f32", "l1_nosep_scale_f32"])
def test_forces_pair_form(monkeypatch, name):
    """The by-target / by-source kernel pair (no head-sum workspace): the softmax backward's site in msg_bwd_target_body."""
    from gotennet_amd import engine
    monkeypatch.setattr(engine, "MSG_BWD_PAIR", True)
    p = 0.1
    cfg, t, net, head = _modules(name, p)
    box = []
    torch.manual_seed(SEED)
    calls = tpg._launches(lambda: box.append(_gpu_forces(net, head, t)))
    assert "gn_message_backward_dropout" in calls and "gn_message_backward" not in calls
    e, f = box[0]
    masks = _masks(net, t["edge_index"].shape[1], p)
    e_ref, f_ref = _oracle_forces(monkeypatch, name, (p,) + _key_of(net), masks)
    assert rel_err(e.cpu(), e_ref) < TOL and rel_err(f.cpu(), f_ref) < TOL


# ---------------------------------------------------------------------------------------------------- 4. parameter gradients
def _pre(name):
    """What the GPU run of both losses needs of ``tpg._oracle``'s result, without running the oracle: the fixture and the
    loss weights, drawn as that function draws them."""
    cfg, sd, head_sd, t = _case(name)
    n_mol, N = int(t["batch"].max()) + 1, t["z"].shape[0]
    g = torch.Generator().manual_seed(7)
    D = (cfg["lmax"] + 1) ** 2 - 1
    c = torch.randn(n_mol, 1, generator=g, dtype=torch.float64)
    wh = torch.randn((N, cfg["n_atom_basis"]), generator=g, dtype=torch.float64)
    wX = torch.randn((N, D, cfg["n_atom_basis"]), generator=g, dtype=torch.float64)
    return dict(cfg=cfg, sd=sd, head_sd=head_sd, t=t, n_mol=n_mol, c=c, wh=wh, wX=wX)


@pytest.mark.parametrize("name", ["l2_sep_f32", "l3_sep_scale_f32", "l5_sep_f32", "opt_act_ssp"])
def test_parameter_gradients_match_masked_oracle(monkeypatch, name):
    p = 0.1
    o = _pre(name)
    t = o["t"]
    net, head = tpg._gpu_modules(o)
    _set_dropout(net, p)
    torch.manual_seed(SEED)
    tpg._energy_loss(net, head, o).backward()
    key = _key_of(net)
    got = {n: q.grad for n, q in net.named_parameters()}
    got.update({"head." + n: q.grad for n, q in head.named_parameters()})
    net.zero_grad(set_to_none=True)
    torch.manual_seed(SEED)                                       # the same key, hence the same masks, for the second loss
    h, X = net(t["z"].cuda(), t["edge_index"].cuda(), t["edge_diff"].cuda(), t["edge_vec"].cuda())
    ((o["wh"].float().cuda() * h).sum() + (o["wX"].float().cuda() * X).sum()).backward()
    assert _key_of(net) == key
    got_hx = {n: q.grad for n, q in net.named_parameters()}
    # the masked oracle through that file's own helper, in a cache of its own (its unmasked results stay untouched)
    monkeypatch.setattr(tpg, "_ORACLE", {})
    count = patch_oracle_softmax(monkeypatch, _masks(net, t["edge_index"].shape[1], p))
    ref = tpg._oracle(name)
    assert count[0] == o["cfg"]["n_interactions"]
    assert torch.equal(ref["c"], o["c"]) and torch.equal(ref["wh"], o["wh"]) and torch.equal(ref["wX"], o["wX"])
    tpg._check(got, ref["energy"], "energy")
    tpg._check(got_hx, ref["hx"], "h,X")


# ---------------------------------------------------------------------------------------------------- 5. strip overflow
def _hub_case(F, lmax=2):
    """A hand-made graph: target 0 with in-degree 300 (300 * 8 heads exceeds the wave strip's 512 floats, the softmax
    workgroup kernel's 2048 and the backward's GS_CAP = 2048), four ordinary atoms, one atom without incoming edges."""
    import gotennet_amd
    from gotennet_amd.outputs import Atomwise
    from oracle import gotennet_oracle as orc
    n_sph = 295
    k = torch.arange(n_sph, dtype=torch.float64) + 0.5
    phi, th = torch.acos(1 - 2 * k / n_sph), np.pi * (1 + 5 ** 0.5) * k
    sphere = 3.0 * torch.stack([torch.cos(th) * torch.sin(phi), torch.sin(th) * torch.sin(phi), torch.cos(phi)], 1)
    extra = torch.tensor([[0.9, 0.1, 0.0], [0.0, 1.1, 0.2], [0.3, 0.0, 1.2], [-1.0, -0.5, 0.3], [0.5, 0.6, -1.0]],
                         dtype=torch.float64)
    pos = torch.cat([torch.zeros(1, 3, dtype=torch.float64), sphere, extra]).float()
    N = pos.shape[0]                                             # 301: hub, 295 on a sphere, ordinary 296..299, lone 300
    edges = [(j, 0) for j in range(1, N)]                        # every atom -> hub: in-degree 300
    edges += [(0, j) for j in range(1, 21)] + [(0, j) for j in range(296, 300)]
    edges += [(a, b) for a in range(296, 300) for b in range(296, 300) if a != b]
    edges += [(300, 296), (300, 297)]                            # atom 300 sends, nothing arrives at it
    ei = torch.tensor(edges, dtype=torch.int64).t().contiguous()
    ei = ei[:, torch.sort(ei[1], stable=True).indices].contiguous()
    assert int((ei[1] == 0).sum()) == 300 and int((ei[1] == 300).sum()) == 0
    torch.manual_seed(F + 1)
    kw = dict(n_atom_basis=F, n_interactions=2, n_rbf=16, num_heads=8, scale_edge=True, lmax=lmax, sep_dir=True, sep_tensor=True)
    net = gotennet_amd.GotenNet(cutoff_fn=gotennet_amd.CosineCutoff(5.0), **kw)
    head = Atomwise(n_in=F, n_hidden=16, property="property", activation="silu")
    with torch.no_grad():
        for m in (net, head):
            for n, q in m.named_parameters():
                if q.dim() == 1:
                    q.uniform_(-0.05, 0.05) if "norm.weight" not in n else q.uniform_(0.9, 1.1)
    z = torch.randint(1, 9, (N,), generator=torch.Generator().manual_seed(3))
    return (orc.default_config(**kw), {k_: v.clone() for k_, v in net.state_dict().items()},
            {k_: v.clone() for k_, v in head.state_dict().items()}, z, pos, ei, net, head)


@pytest.mark.parametrize("F", [32, 512])          # one wave per target / one workgroup per target (and the wide-slot backward)
def test_hub_target_beyond_the_strips(monkeypatch, F):
    from oracle import gotennet_oracle as orc
    p = 0.1
    cfg, sd, head_sd, z, pos, ei, net, head = _hub_case(F)
    net = _set_dropout(net.cuda().requires_grad_(False), p)
    head = head.cuda().eval().requires_grad_(False)
    t = dict(z=z, pos=pos, batch=torch.zeros(z.shape[0], dtype=torch.int64), edge_index=ei)
    torch.manual_seed(SEED)
    with torch.no_grad():
        w, vec = _edges_from_pos(pos.cuda(), ei.cuda())
        h, X = net(z.cuda(), ei.cuda(), w, vec)
    key = _key_of(net)
    torch.manual_seed(SEED)
    e, f = _gpu_forces(net, head, t)
    assert _key_of(net) == key
    masks = _masks(net, ei.shape[1], p)
    count = patch_oracle_softmax(monkeypatch, masks)
    p64 = pos.double().requires_grad_(True)
    w64, vec64 = _edges_from_pos(p64, ei)
    h_ref, X_ref = orc.gotennet_forward(_d64(sd), cfg, z, ei, w64, vec64)
    e_ref = orc.atomwise_energy(_d64(head_sd), h_ref, t["batch"], 1, "silu", z=z)
    (g_ref,) = torch.autograd.grad(e_ref.sum(), p64)
    assert count[0] == 2
    errs = (rel_err(h.cpu(), h_ref.detach()), rel_err(X.cpu(), X_ref.detach()), rel_err(e.cpu(), e_ref.detach()),
            rel_err(f.cpu(), -g_ref))
    print(f"hub F={F}: h {errs[0]:.2e} X {errs[1]:.2e} energy {errs[2]:.2e} forces {errs[3]:.2e}")
    assert max(errs) < TOL


@pytest.mark.parametrize("lmax,pair", [(2, True), (3, False)])
def test_hub_target_head_gradients_in_global_memory(monkeypatch, lmax, pair):
    """Eval mode, no dropout: the hub's 300 * 8 head gradients exceed GS_CAP = 2048, so the softmax / scores backward of
    that target works on the global g_s rows instead of LDS -- in the by-target kernel of the by-target / by-source pair
    (lmax 2, no head-sum workspace) and in attn_bwd_kernel over the two head-sum slices of the degree groups (lmax 3)."""
    from gotennet_amd import engine
    from oracle import gotennet_oracle as orc
    monkeypatch.setattr(engine, "MSG_BWD_PAIR", pair)
    cfg, sd, head_sd, z, pos, ei, net, head = _hub_case(32, lmax)
    net = _set_dropout(net.cuda().requires_grad_(False), 0.0, train=False)
    head = head.cuda().eval().requires_grad_(False)
    t = dict(z=z, pos=pos, batch=torch.zeros(z.shape[0], dtype=torch.int64), edge_index=ei)
    e, f = _gpu_forces(net, head, t)
    p64 = pos.double().requires_grad_(True)
    w64, vec64 = _edges_from_pos(p64, ei)
    h_ref, _ = orc.gotennet_forward(_d64(sd), cfg, z, ei, w64, vec64)
    e_ref = orc.atomwise_energy(_d64(head_sd), h_ref, t["batch"], 1, "silu", z=z)
    (g_ref,) = torch.autograd.grad(e_ref.sum(), p64)
    ee, ef = rel_err(e.cpu(), e_ref.detach()), rel_err(f.cpu(), -g_ref)
    print(f"hub lmax={lmax} pair={pair}: energy {ee:.2e} forces {ef:.2e}")
    assert ee < TOL and ef < TOL


# ---------------------------------------------------------------------------------------------------- 6. unchanged paths
def _hx_forces(net, head, t):
    with torch.no_grad():
        h, X = net(t["z"].cuda(), t["edge_index"].cuda(), t["edge_diff"].cuda(), t["edge_vec"].cuda())
    return (h, X) + _gpu_forces(net, head, t)


def test_paths_without_dropout_keep_their_bits():
    from gotennet_amd.pipeline import EnergyForces
    name = "l2_sep_f32"
    cfg, t, net0, head = _modules(name, 0.0, train=False)
    base = _hx_forces(net0, head, t)
    assert net0.last_dropout_key is None
    for a, b in zip(base, _hx_forces(net0.train(), head, t)):                  # train() with attn_dropout = 0
        assert torch.equal(a, b)
    assert net0.last_dropout_key is None
    _, _, net1, _ = _modules(name, 0.1, train=False)                           # eval() with attn_dropout = 0.1
    for a, b in zip(base, _hx_forces(net1, head, t)):
        assert torch.equal(a, b)
    assert net1.last_dropout_key is None
    # EnergyForces is an inference tool: it never drops, whatever the module's mode
    from tests.test_hip_forces import _head_from_case
    hf = _head_from_case(cfg, load_case(name)[2])
    args = [t[k].cuda() for k in ("z", "edge_index", "edge_diff", "edge_vec", "batch")] + [int(t["batch"].max()) + 1]
    e0, f0 = EnergyForces(net1, hf)(*args)
    e1, f1 = EnergyForces(net1.train(), hf)(*args)
    assert torch.equal(e0, e1) and torch.equal(f0, f1)
    assert net1.last_dropout_key is None


# ---------------------------------------------------------------------------------------------------- 7. reproducibility
def test_seeded_runs_repeat_and_unseeded_runs_differ(monkeypatch):
    name, p = "l2_sep_f32", 0.1
    o = _pre(name)
    t = o["t"]
    net, head = tpg._gpu_modules(o)
    _set_dropout(net, p)
    args = (t["z"].cuda(), t["edge_index"].cuda(), t["edge_diff"].cuda(), t["edge_vec"].cuda())
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        head.zero_grad(set_to_none=True)
        torch.manual_seed(SEED)
        with torch.no_grad():
            h, X = net(*args)
        torch.manual_seed(SEED)
        tpg._energy_loss(net, head, o).backward()
        runs.append((h, X, _key_of(net), tpg._grads([net, head])))
    assert runs[0][2] == runs[1][2]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for n, v in runs[0][3].items():
        assert v is not None and torch.equal(v, runs[1][3][n]), n
    # no reseeding: another key, another mask, another result
    with torch.no_grad():
        h2, _ = net(*args)
        k2 = _key_of(net)
        h3, _ = net(*args)
    assert k2 != _key_of(net) and k2[0] != runs[0][2][0]
    assert not torch.equal(h2, h3)
    # a generator of the module's own takes over from the default one
    net.dropout_generator = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():
        h4, _ = net(*args)
        net.dropout_generator.manual_seed(5)
        h5, _ = net(*args)
    assert torch.equal(h4, h5)
    net.dropout_generator = None
    # p = 1 drops every attention weight: the oracle with an all-zero mask
    _set_dropout(net, 1.0)
    with torch.no_grad():
        h1, X1 = net(*args)
    E, H = t["edge_index"].shape[1], net.num_heads
    for m in _masks(net, E, 1.0):
        assert float(m.abs().max()) == 0.0
    h_ref, X_ref = _oracle_forward(monkeypatch, name, ("p1",), [torch.zeros(E, H)] * net.n_interactions)
    assert rel_err(h1.cpu(), h_ref) < TOL and rel_err(X1.cpu(), X_ref) < TOL


# ---------------------------------------------------------------------------------------------------- 8. stand-alone GATA
@pytest.mark.parametrize("name", ["l2_sep_f32", "l3_sep_scale_f32"])
def test_standalone_gata_layer_drops_as_layer_0(monkeypatch, name):
    from gotennet_amd import attention_dropout_mask
    from oracle import gotennet_oracle as orc
    p = 0.1
    cfg, sd, _, t = _case(name)
    net = _set_dropout(_net_from_case(cfg, sd), p)
    ei, ed = t["edge_index"], t["edge_diff"]
    N, E = t["z"].shape[0], ei.shape[1]
    _, _, tr = orc.gotennet_forward(sd, cfg, t["z"], ei, ed, t["edge_vec"], return_trace=True)
    rl = tr["rl"]
    n_edges = torch.zeros(N).index_add_(0, ei[0], torch.ones(E))[ei[0]]
    h_in, X_in, t_in = tr["layers"][0]                            # inputs of layer 1
    gata = net.gata_list[1]
    assert gata.training and gata.dropout == p
    torch.manual_seed(SEED)
    h1, X1, _ = gata(ei.cuda(), h_in.unsqueeze(1).cuda(), X_in.cuda(), rl.cuda(), t_in.cuda(), ed.cuda(),
                     n_edges.unsqueeze(1).cuda())
    mask = attention_dropout_mask(gata.last_dropout_key, 0, E, cfg["num_heads"], p).cpu()
    assert 0 < float((mask == 0).float().mean()) < 1
    count = patch_oracle_softmax(monkeypatch, [mask])
    pfx = "gata_list.1."
    d = _d64(sd)
    hn, Xn = orc.gata_input_norms(d, cfg, pfx, h_in.double(), X_in.double())
    h_ref, X_ref = orc.gata_message_aggregate(d, cfg, pfx, ei, hn, Xn, rl.double(), t_in.double(), ed.double(), n_edges.double())
    assert count[0] == 1
    assert rel_err(h1.squeeze(1).cpu(), h_ref) < TOL and rel_err(X1.cpu(), X_ref) < TOL
