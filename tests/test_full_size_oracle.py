"""GPU: the full-size batches (BASELINE C2 at lmax 2 and at the north-star lmax 4, C3, C5) checked MOLECULE BY MOLECULE
against the fp64 oracle (oracle/gotennet_oracle.py, pinned to the reference by tests/test_oracle_golden.py).

Molecules do not interact, so the oracle run on one molecule alone is exactly what the batched HIP path must return for that
molecule -- first, middle and last molecules included (the last ones sit in the ragged last tile of every launch).  Every
error is measured against the molecule's OWN largest value (and X per degree block): an error confined to one molecule or
to one degree block is not diluted by the largest value in the batch.  These sizes reach the paths small systems never
take: the un-fused EQFF chain (> engine.EQFF_FUSED_MAX_ATOMS atoms), the 128 x 128 GEMM tile, the slab kernel, E ~ 54 k edge
launches.  The oracle runs once per configuration and molecule (cached in tests/golden_util.py), not once per arithmetic.

Bounds: TOL = 1e-4 per molecule is the project's contract; FLOOR = 2e-5 per molecule is the fp64-truth bound that
tests/test_hip_forces.py::test_fused_pipeline_matches_golden holds the small systems to.  Worst per-molecule errors measured
on MI355X over all configurations and the three arithmetics (the module prints them with ``-s``): h 1.2e-6, X per degree
block 2.0e-6, forces 4.4e-6, position gradients of the general upstream gradient 3.9e-6, energy 1.5e-6 of the molecule's
atomic-energy mass.  Energy against |E| itself reaches 2.0e-5 (a molecule whose atomic energies cancel to 1/30 of their
mass): that measure is held to TOL only."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests.golden_util import (GOLDEN_DIR, degree_blocks, group_rel_err, molecule_rows, oracle_molecule, rel_err,
                               seeded_modules)

pytestmark = pytest.mark.gpu

TOL = 1e-4
FLOOR = 2e-5


def _fixture_cfg(name, **over):
    zf = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    cfg = json.loads(bytes(zf["cfg"]).decode())
    cfg.update(over)
    return cfg


def _selected(B, n_random, seed):
    """First, middle and last molecules, plus ``n_random`` drawn with a seeded generator."""
    fixed = sorted({0, 1, 2, B // 2 - 1, B // 2, B - 3, B - 2, B - 1})
    g = torch.Generator().manual_seed(seed)
    rest = [m for m in torch.randperm(B, generator=g).tolist() if m not in fixed][:n_random]
    return sorted(fixed + rest)


# name -> (model + inputs config, molecules checked, forces / gradients checked)
CONFIGS = {
    "c2_lmax2": (_fixture_cfg("c2_full_forward_seeded"), _selected(128, 8, 11), True),
    "c2_lmax4": (_fixture_cfg("c2_model_lmax4_1mol_seeded", workload="rmd17_aspirin", batch_seed=0, n_mol=128),
                 _selected(128, 8, 12), True),
    "c3": (_fixture_cfg("c3_ac_ala3_2mol_seeded", n_mol=64), sorted({0, 31, 32, 63} | {5, 17, 44, 58}), True),
    # forward and energy only: fp64 autograd through 370 atoms at a 32-neighbour cap is too large for a test
    "c5": (_fixture_cfg("c5_nanotube_1mol_seeded", n_mol=8), [0, 7], False),
}
GRAD_MOLECULES = 8          # the general-upstream-gradient check: the first 8 of a configuration's selected molecules

#: worst per-molecule error of each (configuration, arithmetic, quantity) met in this process (printed with ``-s``)
WORST = {}


def _inputs(cfg):
    from gotennet_amd import synthetic
    return synthetic.make_batch(cfg["workload"], cfg["n_mol"], seed=cfg["batch_seed"])


def _modules(cfg):
    """The seeded model (tests/golden_util.seeded_fill: non-zero biases, norm weights other than 1) on the CPU."""
    net, head = seeded_modules(cfg)
    for m in (net, head):
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                assert bool((p != 0).any()), n                              # every bias epilogue sees non-zero values
            if n.endswith("norm.weight"):
                assert bool((p != 1).all()), n
    return net, head


def _upstream(cfg, N):
    """Per-atom weights of h and of X: the upstream gradient dL/dh, dL/dX of a loss sum(wh * h) + sum(wX * X)."""
    D = (cfg["lmax"] + 1) ** 2 - 1
    g = torch.Generator().manual_seed(2024 + cfg["lmax"])
    return (torch.randn((N, cfg["n_atom_basis"]), generator=g), torch.randn((N, D, cfg["n_atom_basis"]), generator=g))


def _record(name, mode, what, err):
    key = (name, mode, what)
    WORST[key] = max(WORST.get(key, 0.0), err)
    print(f"per-molecule worst {name} {mode} {what}: {WORST[key]:.3e}")


def _check(name, mode, got, ref, what, floor=True):
    """One molecule's quantity against its oracle value: the hard contract and (``floor``) the fp64-truth floor."""
    err = rel_err(got, ref) if not isinstance(ref, list) else max(group_rel_err(got, ref[0], ref[1]))
    _record(name, mode, what, err)
    assert err < TOL, (name, mode, what, err)
    assert not floor or err < FLOOR, (name, mode, what, err)
    return err


def check_molecules(name, mode, cfg, sd, hsd, pos, batch, z, mols, h=None, X=None, e=None, f=None, forces=True):
    """Per selected molecule: h, X per degree block, energy, forces -- each against that molecule's fp64 oracle."""
    for m in mols:
        o = oracle_molecule(cfg, sd, hsd, pos, batch, z, m, forces=forces)
        rows = molecule_rows(batch, m)
        if h is not None:
            _check(name, mode, h[rows], o["h"], "h")
            _check(name, mode, X[rows], [o["X"], degree_blocks(cfg["lmax"])], "X(per degree block)")
        # energy: a sum of atomic energies that partly cancel, so its rounding scales with the molecule's atomic-energy mass
        # sum |E_i|, not with |E| (up to 30x smaller for these molecules): the contract holds |dE| / |E|, the floor
        # |dE| / sum |E_i|
        _check(name, mode, e[m].double(), o["energy"][0], "energy |dE|/|E|", floor=False)
        err_mass = float((e[m].double() - o["energy"][0]).abs().max()) / float(o["energy_mass"])
        _record(name, mode, "energy |dE|/sum|E_i|", err_mass)
        assert err_mass < FLOOR, (name, mode, m, err_mass)
        if forces:
            _check(name, mode, f[rows], o["forces"], "forces")


def _run_full(cfg, net, head, fuse_eqff=None):
    from gotennet_amd.graph import distance
    from gotennet_amd.pipeline import EnergyForces
    pos, batch, z = _inputs(cfg)
    net, head = net.cuda().eval(), head.cuda().eval()
    net.fuse_eqff = fuse_eqff
    ei, ed, ev = distance(pos.cuda(), batch.cuda(), cfg["cutoff"], 32)
    h, X = net(z.cuda(), ei, ed, ev)
    e, f = EnergyForces(net, head)(z.cuda(), ei, ed, ev, batch.cuda(), cfg["n_mol"])
    torch.cuda.synchronize()
    return (pos, batch, z), [v.cpu() for v in (h, X, e, f)], ei.shape[1]


def _check_upstream(name, mode, cfg, net, sd, hsd, mols, fuse_eqff=None):
    """GotenNetWrapper's position path (_RepresentationPosFn) with a general upstream gradient: d sum(wh * h) / d pos and
    d sum(wX * X) / d pos from ONE forward (retain_graph: the second backward reads the same tape), per atom against the
    oracle's autograd through orc.distance.  The caller's gradient tensors must come back bit-unchanged."""
    import gotennet_amd
    pos, batch, z = _inputs(cfg)
    hp = {k: cfg[k] for k in ("n_atom_basis", "n_interactions", "n_rbf", "lmax", "num_heads", "scale_edge", "sep_dir",
                              "sep_tensor", "max_z")}
    wrap = gotennet_amd.GotenNetWrapper(cutoff_fn=gotennet_amd.CosineCutoff(cfg["cutoff"]), max_num_neighbors=32, **hp)
    wrap.load_state_dict(net.state_dict(), strict=True)
    wrap = wrap.cuda().eval()
    wrap.fuse_eqff = fuse_eqff
    wh, wX = _upstream(cfg, pos.shape[0])
    wh_c, wX_c = wh.cuda(), wX.cuda()
    wh_0, wX_0 = wh_c.clone(), wX_c.clone()
    p = pos.cuda().requires_grad_(True)
    h, X = wrap(types.SimpleNamespace(z=z.cuda(), pos=p, batch=batch.cuda()))
    (gp_h,) = torch.autograd.grad((h,), p, grad_outputs=(wh_c,), retain_graph=True)
    (gp_X,) = torch.autograd.grad((X,), p, grad_outputs=(wX_c,))
    torch.cuda.synchronize()
    assert torch.equal(wh_c, wh_0) and torch.equal(wX_c, wX_0)           # caller gradients are read-only
    gp_h, gp_X = gp_h.cpu(), gp_X.cpu()
    assert torch.isfinite(gp_h).all() and torch.isfinite(gp_X).all()
    for m in mols:
        o = oracle_molecule(cfg, sd, hsd, pos, batch, z, m, upstream=(wh, wX))
        rows = molecule_rows(batch, m)
        _check(name, mode, gp_h[rows], o["pos_grad_h"], "d(wh.h)/dpos")
        _check(name, mode, gp_X[rows], o["pos_grad_X"], "d(wX.X)/dpos")


@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("name", list(CONFIGS))
def test_full_size_matches_oracle_per_molecule(name):
    from gotennet_amd import engine
    cfg, mols, forces = CONFIGS[name]
    net, head = _modules(cfg)
    sd, hsd = net.state_dict(), head.state_dict()
    (pos, batch, z), (h, X, e, f), E = _run_full(cfg, net, head)
    N = pos.shape[0]
    assert N > engine.EQFF_FUSED_MAX_ATOMS and not engine.eqff_fused_ok(net.config(), N)     # the un-fused EQFF chain
    assert E > 50_000
    assert torch.isfinite(h).all() and torch.isfinite(X).all() and torch.isfinite(e).all() and torch.isfinite(f).all()
    check_molecules(name, engine.GEMM_MODE, cfg, sd, hsd, pos, batch, z, mols, h, X, e, f, forces=forces)


@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("name", ["c2_lmax2", "c2_lmax4"])
def test_full_size_upstream_gradient_per_atom(name):
    from gotennet_amd import engine
    cfg, mols, _ = CONFIGS[name]
    net, head = _modules(cfg)
    _check_upstream(name, engine.GEMM_MODE, cfg, net, net.state_dict(), head.state_dict(), mols[:GRAD_MOLECULES])


@pytest.mark.parametrize("mode", ["split", "f16x2"])
def test_full_size_fused_eqff_matches_oracle_per_molecule(mode):
    """fuse_eqff = True at 2688 atoms (the auto switch keeps the fused EQFF kernels to 1024 atoms or fewer; a caller may
    force them): forward, energy, forces and the general upstream gradient per molecule.  The fused kernels exist in the
    two plane arithmetics only."""
    from gotennet_amd import engine
    name = "c2_lmax2"
    cfg, mols, _ = CONFIGS[name]
    net, head = _modules(cfg)
    sd, hsd = net.state_dict(), head.state_dict()
    old, engine.GEMM_MODE = engine.GEMM_MODE, mode
    try:
        (pos, batch, z), (h, X, e, f), _ = _run_full(cfg, net, head, fuse_eqff=True)
        assert engine.eqff_fused_ok(net.config(), pos.shape[0])
        check_molecules(name + "_fused", mode, cfg, sd, hsd, pos, batch, z, mols, h, X, e, f)
        _check_upstream(name + "_fused", mode, cfg, net, sd, hsd, mols[:GRAD_MOLECULES], fuse_eqff=True)
    finally:
        engine.GEMM_MODE = old
