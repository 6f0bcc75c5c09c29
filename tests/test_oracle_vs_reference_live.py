"""CPU: the oracle against the reference's fp64 forward on seeded cases (tests/golden/kat_oracle_fp64.npz, written by
tools/make_golden.py from the live reference).  The fixture carries inputs and (h, X) only: the weights are rebuilt here
with golden_util.seeded_fill, which fills the reference's modules and the mirror modules identically."""
import os

import numpy as np
import pytest
import torch

from tests.golden_util import GOLDEN_DIR, seeded_fill


@pytest.mark.parametrize("lmax,sep,scale", [(1, False, True), (2, True, False), (3, True, True), (4, True, False)])
def test_oracle_matches_live_reference_fp64(lmax, sep, scale):
    import gotennet_amd
    from oracle import gotennet_oracle as orc
    k = np.load(os.path.join(GOLDEN_DIR, "kat_oracle_fp64.npz"))
    t = {n.split("/", 1)[1]: torch.from_numpy(k[n]) for n in k.files if n.startswith(f"l{lmax}/")}
    hp = dict(n_atom_basis=32, n_interactions=3, n_rbf=8, lmax=lmax, num_heads=4, scale_edge=scale,
              sep_dir=sep, sep_tensor=sep, max_z=12)
    net = gotennet_amd.GotenNet(cutoff_fn=gotennet_amd.CosineCutoff(5.0), **hp)      # parameter holders only (CPU)
    seeded_fill(net, 100 + lmax)
    sd = {n: (v.double() if v.is_floating_point() else v) for n, v in net.state_dict().items()}
    cfg = orc.default_config(cutoff=5.0, **{n: v for n, v in hp.items() if n != "max_z"})
    ei, w, vec = orc.distance(t["pos"], t["batch"], 5.0)
    assert torch.equal(ei, t["edge_index"])
    h, X = orc.gotennet_forward(sd, cfg, t["z"], ei, w, vec)
    h_ref, X_ref = t["h"], t["X"]
    assert float((h - h_ref).abs().max() / h_ref.abs().max()) < 1e-12
    assert float((X - X_ref).abs().max() / X_ref.abs().max()) < 1e-12
