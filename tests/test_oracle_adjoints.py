"""CPU: the fp64 restatement with intermediates (tests/oracle_adjoints.py) that the GPU adjoint checks compare against, and
the sensitivity of their comparison.  No GPU needed."""
import pytest
import torch

from oracle import gotennet_oracle as orc
from tests.golden_util import rel_err
from tests.oracle_adjoints import adjoint_error, check_adjoint, forward_with_intermediates, groups, oracle_adjoints, seeded_model

TOL = 1e-4

PIN_CASES = {
    "lmax2_sep": dict(n_atom_basis=32, n_interactions=3, n_rbf=8, lmax=2, num_heads=4, scale_edge=False, sep_dir=True,
                      sep_tensor=True),
    "lmax3_norms_composed_mean": dict(n_atom_basis=32, n_interactions=2, n_rbf=8, lmax=3, num_heads=4, scale_edge=True,
                                      sep_dir=False, sep_tensor=False, sep_htr=False, layernorm="layer",
                                      steerable_norm="tensor", edge_updates="gated_mlp_linw_ln", evec_dim=16,
                                      emlp_dim=24, edge_ln="layer", aggr="mean", activation="gelu"),
    "lmax5_max": dict(n_atom_basis=16, n_interactions=2, n_rbf=8, lmax=5, num_heads=4, scale_edge=False, sep_dir=True,
                      sep_tensor=True, aggr="max"),
}


def _system(seed, n_mol=2, n_atoms=9, box=3.5):
    g = torch.Generator().manual_seed(seed)
    pos = torch.cat([torch.rand((n_atoms, 3), generator=g) * box + 20.0 * b for b in range(n_mol)])
    batch = torch.arange(n_mol).repeat_interleave(n_atoms)
    z = torch.randint(1, 9, (n_mol * n_atoms,), generator=g)
    return pos, batch, z


@pytest.mark.parametrize("name", list(PIN_CASES))
def test_restatement_matches_oracle(name):
    """The restated loop computes what orc.gotennet_forward computes, bit for bit, and its position gradient is
    orc.energy_and_forces's forces; its adjoints of the edge inputs give the same forces through the chain rule."""
    net, head, cfg = seeded_model(PIN_CASES[name], seed=7)
    sd = {k: v.double() if v.is_floating_point() else v for k, v in net.state_dict().items()}
    hsd = {k: v.double() for k, v in head.state_dict().items()}
    pos, batch, z = _system(3)
    pos = pos.double()
    ei, w, vec = orc.distance(pos, batch, 5.0)
    with torch.no_grad():
        h_ref, X_ref = orc.gotennet_forward(sd, cfg, z, ei, w, vec)
        h, X, _ = forward_with_intermediates(sd, cfg, z, ei, w, vec)
    assert torch.equal(h, h_ref) and torch.equal(X, X_ref)
    _, f_ref, _ = orc.energy_and_forces(sd, cfg, hsd, z, pos, batch, 2)
    N, D, F = X.shape
    g = torch.Generator().manual_seed(1)
    upstream = (torch.randn((N, F), generator=g), torch.randn((N, D, F), generator=g))
    o = oracle_adjoints(sd, cfg, hsd, z, pos, batch, 2, 32, upstream)
    assert torch.equal(o["h"], h_ref) and torch.equal(o["X"], X_ref)
    assert torch.allclose(o["forces"], f_ref, rtol=0, atol=1e-12 * float(f_ref.abs().max()))
    # dL/dpos from the edge-input adjoints: edge_vec = pos[src] - pos[dst], edge_diff = |edge_vec| (non-self edges)
    init = o["adj_a"][("init", -1)]
    src, dst = ei
    mask = src != dst
    gv = init["vec"].clone()
    gv[mask] += init["diff"][mask, None] * vec[mask] / w[mask, None]
    gv[~mask] = 0
    gpos = torch.zeros_like(pos).index_add_(0, src, gv).index_add_(0, dst, -gv)
    assert rel_err(-gpos, f_ref) < 1e-10
    # the last layer's output t and (energy loss) X adjoints are zero in truth; the general loss has dL/dX = wX there
    last = o["adj_a"][("layer", cfg["n_interactions"] - 1)]
    assert not last["t"].any() and not last["X"].any()
    assert torch.equal(o["adj_b"][("layer", cfg["n_interactions"] - 1)]["X"], upstream[1].double())


def test_checker_sees_one_block_of_one_molecule():
    """A 1e-3 relative error in one degree block of one molecule: the per-molecule, per-block check fails it although the
    whole-tensor max-norm error stays under TOL (the block is small against the largest value in the batch)."""
    lmax, F, n_mol, n_at = 3, 16, 3, 10
    D = (lmax + 1) ** 2 - 1
    g = torch.Generator().manual_seed(0)
    ref = torch.randn((n_mol * n_at, D, F), generator=g, dtype=torch.float64)
    ref[n_at:2 * n_at, 3:8] *= 1e-2                             # molecule 1, l = 2: a block of small adjoints
    got = ref.clone()
    got[n_at:2 * n_at, 3:8] *= 1 + 1e-3
    batch = torch.arange(n_mol).repeat_interleave(n_at)
    ei = torch.stack([torch.arange(n_mol * n_at), torch.arange(n_mol * n_at)])
    grp = groups(batch, ei)
    assert rel_err(got, ref) < TOL                              # the whole-tensor check passes it
    ok, err = check_adjoint(got, ref, "block", grp, lmax, TOL)
    assert not ok and err > 0.9e-3
    assert adjoint_error(got, ref, "atom", grp, lmax) < TOL     # per molecule without the blocks: still diluted
    ok, _ = check_adjoint(ref.clone(), ref, "block", grp, lmax, TOL)
    assert ok
    # zero in truth: exactly zero passes, anything else fails
    zero = torch.zeros_like(ref)
    assert check_adjoint(zero.float(), zero, "block", grp, lmax, TOL)[0]
    tiny = zero.clone()
    tiny[0, 0, 0] = 1e-30
    assert not check_adjoint(tiny, zero, "block", grp, lmax, TOL)[0]
