"""GPU: the hand-written force backward checked STAGE BY STAGE against fp64 autograd of the oracle.

``engine.backward(..., trace=)`` records the adjoints (gradients of the loss w.r.t. each intermediate state) at every stage
boundary: each layer's output (h, X, t), its message stage's output (what EQFF and HTR read), its normalised inputs, and the
init (h0, t0, phi, the initial X, the edge inputs).  Each is compared with the same adjoint of the fp64 restatement in
tests/oracle_adjoints.py (pinned to the oracle by tests/test_oracle_adjoints.py), for two losses: (a) the Atomwise energy
(the force path, dL/dX = None at the last layer) and (b) sum(wh * h) + sum(wX * X).  Errors are max-norm relative per
molecule -- X-like tensors per molecule AND degree block, t / phi / edge inputs over the molecule's edges -- so an error in a
block or a stage that contributes little to the forces is not diluted.  Adjoints that are zero in truth (dL/dt of the last
layer's output; dL/dX of it under the energy loss) must be exactly zero; dL/dX_in of a layer run in the zero-X_in form is
never computed and is skipped.  The configurations cross the switches that select different backward kernels.  The
saving forward's per-layer (h, X, t) must equal the inference forward's bit for bit, and a traced backward is
bit-reproducible and returns the untraced backward's bits.

Bounds: every checkpoint is held to TOL = 1e-4 per molecule and degree block, the project's contract, and to FLOOR.  Worst
errors measured on MI355X over the three arithmetics and both losses (the module prints each (configuration, arithmetic,
loss, checkpoint) with ``-s``): 5.4e-6 outside the steerable-norm configurations (dL/d edge_diff; edge_vec 4.5e-6, t 4.6e-6,
phi 3.4e-6, X blocks 3.3e-6, h 1.2e-6), 1.9e-5 with TensorLayerNorm (X blocks of layer 0: its max-min norm amplifies rounding in the backward).
FLOOR is 2e-5, and 5e-5 where the model has a steerable norm.
"""
import pytest
import torch

from tests.oracle_adjoints import KIND, check_adjoint, groups, oracle_adjoints, seeded_model

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_mode")]

TOL = 1e-4
FLOOR, FLOOR_STEERABLE_NORM = 2e-5, 5e-5


def _base(**kw):
    hp = dict(n_atom_basis=64, n_interactions=2, n_rbf=16, lmax=2, num_heads=8, scale_edge=False, sep_dir=True,
              sep_tensor=True)
    hp.update(kw)
    return hp


#: name -> (constructor arguments, system, module attributes, engine switches)
#: system: ("mols", n_mol, n_atoms, box) random molecules 20 A apart; ("cap", n, box, cap) one dense molecule whose capped
#: radius graph is asymmetric; ("cluster", n, box) one molecule whose every atom sees every other one
F128 = _base(n_atom_basis=128, n_interactions=3)
MOLS = ("mols", 3, 14, 4.0)
CONFIGS = {
    "f128_lmax2_fused": (F128, MOLS, dict(fuse_eqff=True), {}),
    "f128_lmax2_unfused": (F128, MOLS, dict(fuse_eqff=False), {}),
    "f128_lmax2_msg_pair": (F128, MOLS, dict(fuse_eqff=True), dict(MSG_BWD_PAIR=True)),
    "f128_lmax2_general_first": (F128, MOLS, dict(fuse_eqff=False), dict(ZERO_X_FIRST=False)),
    "f256_lmax3": (_base(n_atom_basis=256, lmax=3), ("mols", 2, 14, 4.0), {}, {}),
    "f64_lmax4": (_base(lmax=4, n_interactions=3), MOLS, {}, {}),
    "f128_lmax4": (_base(n_atom_basis=128, lmax=4), ("mols", 2, 16, 4.0), {}, {}),
    "f64_lmax4_sliced": (_base(lmax=4), MOLS, dict(sliced_kernels=True), {}),
    "f64_lmax5": (_base(lmax=5), MOLS, {}, {}),
    "f32_lmax8": (_base(n_atom_basis=32, lmax=8, num_heads=4), ("mols", 2, 12, 3.5), {}, {}),
    "nosep_scale": (_base(sep_dir=False, sep_tensor=False, scale_edge=True), MOLS, {}, {}),
    "aggr_mean": (_base(aggr="mean", lmax=3), MOLS, {}, {}),
    "aggr_max": (_base(aggr="max", lmax=3), MOLS, {}, {}),
    "composed_joint_evec16": (_base(edge_updates="gated_linw_ln", sep_htr=False, evec_dim=16), MOLS, {}, {}),
    "composed_mlp_evec16": (_base(edge_updates="mlpa_linwa_postln", evec_dim=16, emlp_dim=48, edge_ln="layer",
                                  n_interactions=3), MOLS, {}, {}),
    "norms_f64": (_base(layernorm="layer", steerable_norm="tensor", n_interactions=3), MOLS, {}, {}),
    "norms_f192_embedded": (_base(n_atom_basis=192, layernorm="layer", steerable_norm="tensor"), MOLS, {}, {}),
    "layernorm_only_lmax3": (_base(layernorm="layer", lmax=3), MOLS, {}, {}),
    "gelu": (_base(activation="gelu", lmax=3), MOLS, {}, {}),
    "f512_h8": (_base(n_atom_basis=512), ("mols", 2, 12, 4.0), {}, {}),
    "f1024_h16": (_base(n_atom_basis=1024, num_heads=16), ("mols", 2, 12, 4.0), {}, {}),
    "capped_asymmetric": (_base(scale_edge=True), ("cap", 60, 6.0, 8), {}, {}),
    "complete_cluster": (_base(scale_edge=True), ("cluster", 110, 2.5), {}, {}),
}

_ORACLE = {}
#: worst error of each (config, arithmetic, loss, checkpoint) met in this process
WORST = {}


def _system(name):
    kind, *a = CONFIGS[name][1]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if kind == "mols":
        n_mol, n_at, box = a
        pos = torch.cat([torch.rand((n_at, 3), generator=g) * box + 20.0 * b for b in range(n_mol)])
        cap = 32
    else:
        n_at, box = a[0], a[1]
        n_mol, pos = 1, torch.rand((n_at, 3), generator=g) * box
        cap = a[2] if kind == "cap" else n_at + 8
    batch = torch.arange(n_mol).repeat_interleave(n_at)
    z = torch.randint(1, 9, (n_mol * n_at,), generator=g)
    return pos, batch, z, n_mol, cap


def _upstream(cfg, N, seed):
    D = (cfg["lmax"] + 1) ** 2 - 1
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, cfg["n_atom_basis"]), generator=g), torch.randn((N, D, cfg["n_atom_basis"]), generator=g)


def _oracle(name, net, head, cfg, pos, batch, z, n_mol, cap):
    """fp64 adjoints of the configuration: computed once, shared by the three arithmetics."""
    if name not in _ORACLE:
        import os
        old = torch.get_num_threads()
        torch.set_num_threads(min(8, os.cpu_count() or 1))
        try:
            up = _upstream(cfg, pos.shape[0], 77)
            o = oracle_adjoints(net.state_dict(), cfg, head.state_dict(), z, pos, batch, n_mol, cap, up)
        finally:
            torch.set_num_threads(old)
        o["upstream"] = up
        _ORACLE[name] = o
    return _ORACLE[name]


def _by_key(trace):
    out = {}
    for d in trace:
        key = (d["stage"], d["layer"])
        assert key not in out, key
        out[key] = {k: v for k, v in d.items() if k not in ("stage", "layer")}
    return out


def _equal_traces(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            if isinstance(x[k], torch.Tensor):
                assert torch.equal(x[k], y[k]), (x["stage"], x["layer"], k)
            else:
                assert x[k] == y[k]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_backward_adjoints_match_oracle(name):
    from gotennet_amd import engine
    from gotennet_amd.graph import distance
    from gotennet_amd.outputs import molecule_ptr
    hp, _, attrs, switches = CONFIGS[name]
    mode = engine.GEMM_MODE
    try:
        net, head, cfg = seeded_model(hp, seed=sum(map(ord, name)) % 1000)
        for k, v in attrs.items():
            setattr(net, k, v)
        engine.check_backward_supported(net.config())
    except NotImplementedError as exc:                   # a combination the constructor or the backward refuses
        pytest.skip(f"{name}: {exc}")
    pos, batch, z, n_mol, cap = _system(name)
    o = _oracle(name, net, head, cfg, pos, batch, z, n_mol, cap)
    old = {k: getattr(engine, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(engine, k, v)
        net, head = net.cuda().eval(), head.cuda().eval()
        ecfg, pw = net.config(), net.packed_weights()
        ei, ed, ev = distance(pos.cuda(), batch.cuda(), 5.0, cap)
        assert torch.equal(ei.cpu(), o["edge_index"])                         # CSR order = the oracle's edge order
        N, L, lmax = pos.shape[0], hp["n_interactions"], hp["lmax"]
        z32 = z.cuda().to(torch.int32)
        g = engine.Graph(ecfg, pw, N, ei, ed, ev)
        if "sliced_kernels" in attrs:
            assert ecfg.sliced
        # the saving forward (pre_out / ctx / pre_g1 / mm copies, the saving fused EQFF variant) computes the same bits
        tr_inf, tr_sav = [], []
        h_i, X_i, _ = engine.forward(ecfg, pw, z32, g, trace=tr_inf)
        h, X, tape = engine.forward(ecfg, pw, z32, g, save=True, trace=tr_sav)
        assert torch.equal(h, h_i) and torch.equal(X, X_i)
        for li, (a, b) in enumerate(zip(tr_inf, tr_sav)):
            for k, u, v in zip("hXt", a, b):
                assert torch.equal(u, v), (li, k)
        # loss (a): the Atomwise energy through the head kernels; loss (b): the general upstream gradient
        mol_ptr = molecule_ptr(batch.cuda(), n_mol)
        _, _, pre1 = head.energy_raw(h, z32, mol_ptr, n_mol, mode=ecfg.gemm_mode)
        gh = head.grad_h_raw(pre1, ecfg.F_model or ecfg.F, mode=ecfg.gemm_mode)
        wh, wX = (u.cuda() for u in o["upstream"])
        runs = {}
        for loss, (uh, uX) in (("a", (gh, None)), ("b", (wh, wX))):
            tr, tr2 = [], []
            gv, gd = engine.backward(ecfg, pw, z32, g, tape, uh, uX, trace=tr)
            gv0, gd0 = engine.backward(ecfg, pw, z32, g, tape, uh, uX)
            engine.backward(ecfg, pw, z32, g, tape, uh, uX, trace=tr2)
            torch.cuda.synchronize()
            assert torch.equal(gv, gv0) and torch.equal(gd, gd0), loss        # the trace changes no bit
            _equal_traces(tr, tr2)                                             # bit-reproducible
            runs[loss] = _by_key([{k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in d.items()} for d in tr])
    finally:
        for k, v in old.items():
            setattr(engine, k, v)

    grp = groups(batch, o["edge_index"])
    floor = FLOOR_STEERABLE_NORM if hp.get("steerable_norm") else FLOOR
    failures = []
    for loss, got in runs.items():
        ref = o["adj_" + loss]
        assert set(got) == set(ref), (sorted(got), sorted(ref))
        for key in ref:
            for what, r in ref[key].items():
                v = got[key][what]
                if v is None:                                 # never computed: dL/dX_in of a zero-X_in layer
                    assert what == "X" and engine.zero_X_in(ecfg, 0) and (key == ("init", -1) or key[1] == 0), (key, what)
                    continue
                assert v.shape == r.shape, (key, what, v.shape, r.shape)
                assert torch.isfinite(v).all(), (key, what)
                ok, err = check_adjoint(v, r, KIND[what], grp, lmax, TOL)
                tag = f"{key[0]}{'' if key[1] < 0 else key[1]}.{what}"
                wk = (name, mode, loss, tag)
                WORST[wk] = max(WORST.get(wk, 0.0), err)
                print(f"adjoint worst {name} {mode} loss-{loss} {tag}: "
                      f"{'exact 0' if not bool(r.ne(0).any()) else f'{err:.2e}'}")
                if not ok or err >= floor:
                    failures.append((loss, tag, err))
    assert not failures, failures
