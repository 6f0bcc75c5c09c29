"""Multi-image periodic neighbour lists, host side (no GPU): the brute-force yardstick of tests/pbc_multi_util.py against
the minimum-image one, the conditions the narrow test systems must meet, the replica identity in the fp64 oracle, and the
relaxed cell check."""
import inspect
import os
import re

import pytest
import torch

from tests import pbc_multi_util as MU
from tests import pbc_util as U

NARROW = ["n1", "n2", "r2", "n3", "n4", "n5"]


@pytest.mark.parametrize("name", ["a", "b", "c", "e"])
def test_brute_force_equals_the_minimum_image_one_on_wide_cells(name):
    s = U.system(name)
    ref = U.brute_force(s["pos"], s["batch"], s["cell"])
    bf = MU.brute_force(s["pos"], s["batch"], s["cell"])
    assert torch.equal(bf["edge_index"], ref["edge_index"]) and torch.equal(bf["edge_shift"], ref["edge_shift"])
    assert abs(bf["gap"] - ref["gap"]) < 1e-12 and not bf["border"]


@pytest.mark.parametrize("name", NARROW)
def test_narrow_systems_meet_their_input_conditions(name):
    """Gap to the cutoff, a complete enumeration, no image outside the range the relaxed check hands the kernel, and the cap
    of 32 bites neither in the cell nor (asserted by ``replica_oracle`` users: here directly) in the replica."""
    from gotennet_amd import graph
    s = MU.system(name)
    R = graph.image_ranges(s["cell"], MU.CUTOFF)
    bf = MU.brute_force(s["pos"], s["batch"], s["cell"], ranges=R)
    MU.assert_input(bf, 32)
    assert bool((bf["t_max"] <= R.long()).all()), (bf["t_max"].tolist(), R.tolist())
    assert int(bf["cand"].min()) >= 0
    # ordering: target-major, sources ascending, shifts ascending lexicographically
    ei, sh = bf["edge_index"], bf["edge_shift"] + 50
    key = ((ei[1] * 1000 + ei[0]) * 100 + sh[:, 0]) * 10000 + sh[:, 1] * 100 + sh[:, 2]
    assert bool((key[1:] > key[:-1]).all())
    loops = (ei[0] == ei[1]) & (bf["edge_shift"] == 0).all(1)
    assert int(loops.sum()) == s["pos"].shape[0] and not bool(bf["edge_diff"][loops].any())
    assert bool((bf["edge_diff"][~loops] > 0.9).all())            # self-images included: real edges at a real distance
    rep, owner, count = MU.replicate(s)
    rbf = U.brute_force(rep["pos"], rep["batch"], rep["cell"])    # (asserts one image per pair: the replica is minimum-image)
    U.assert_gap(rbf)
    assert max(int(h.sum(1).max()) for h in rbf["hits"]) <= 32
    # the replica's list is the cell's, copy by copy: same degrees, same number of edges per copy
    assert rbf["edge_index"].shape[1] == int((bf["degree"] * count[s["batch"]].long()).sum())


def test_narrow_systems_are_what_they_are_named_for():
    def self_images(name):
        s = MU.system(name)
        bf = MU.brute_force(s["pos"], s["batch"], s["cell"])
        return bf, int(((bf["edge_index"][0] == bf["edge_index"][1]) & (bf["edge_shift"] != 0).any(1)).sum())
    bf, n = self_images("n1")                                     # several images of a pair, no self-image
    pair = bf["edge_index"][1] * 100 + bf["edge_index"][0]
    assert n == 0 and bf["edge_index"].shape[1] == 48 and int(torch.bincount(pair).max()) >= 2
    assert self_images("n2")[1] == 12
    bf, n = self_images("n3")
    assert n == 18 and bf["edge_index"].shape[1] == 19 and abs(bf["gap"] - (2.9 * 3 ** 0.5 - 5.0)) < 1e-6
    bf, n = self_images("r2")
    assert n == bf["edge_index"].shape[1] - 1 and int(bf["t_max"].max()) == 2
    a, b = MU.system("n1"), MU.system("n5")                       # n5: n1 moved by lattice vectors, same list, other shifts
    fa, fb = (MU.brute_force(s["pos"], s["batch"], s["cell"]) for s in (a, b))
    assert torch.equal(fa["edge_index"], fb["edge_index"]) and not torch.equal(fa["edge_shift"], fb["edge_shift"])
    assert float((fa["edge_vec"] - fb["edge_vec"]).abs().max()) < 1e-5


def test_cap_cases():
    """Statements about the inputs of the capped list tests.  n2 / CAP_N2_SPLITS_PAIR: the cap falls between two images of
    one (target, source) pair.  n1 / CAP_N1_SECOND_TRIP and r2 / CAP_R2_SECOND_TRIP: some target reaches the cap on a
    candidate beyond its first 64, i.e. in a later trip of the wave.  (n2 has 2 x 27 = 54 candidates per target: no second
    trip there.)"""
    from gotennet_amd import graph

    def hits_of(name):
        s = MU.system(name)
        R = graph.image_ranges(s["cell"], MU.CUTOFF)
        bf = MU.brute_force(s["pos"], s["batch"], s["cell"], max_num_neighbors=10 ** 6, ranges=R)
        return [(bf["edge_index"][0][bf["edge_index"][1] == i], bf["cand"][bf["edge_index"][1] == i])
                for i in range(s["pos"].shape[0])]
    cap = MU.CAP_N2_SPLITS_PAIR
    assert any(len(src) > cap and src[cap - 1] == src[cap] for src, _ in hits_of("n2"))
    for name, cap in (("n1", MU.CAP_N1_SECOND_TRIP), ("r2", MU.CAP_R2_SECOND_TRIP)):
        assert any(len(src) > cap and int(cand[cap - 1]) >= 64 for src, cand in hits_of(name)), name
        assert any(int(cand[0]) < 64 for _, cand in hits_of(name))     # (and hits in the first trip as well)


@pytest.mark.parametrize("name", ["n1", "n2", "n3"])
def test_replica_identity_fp64(name):
    """Translation symmetry in the oracle: on n1 (no self-images, so the oracle's index rule for self-loops is the right one)
    the multi-image list of the cell gives the replica's energy / count, forces and stress to 1e-10; on every system the
    replica's forces tile (asserted inside ``replica_oracle``)."""
    s = MU.system(name)
    _, _, sd, hsd, cfg = U.make_model(32, 2, 2, seed=1)
    o = MU.replica_oracle(sd, cfg, hsd, s)
    bf = MU.brute_force(s["pos"], s["batch"], s["cell"])
    assert o["n_edges"] == bf["edge_index"].shape[1] * int(o["count"][0])
    if name != "n1":
        return
    c = U.oracle_efs(sd, cfg, hsd, s, bf["edge_index"], bf["edge_shift"])
    assert float((c["energy"] - o["energy"]).abs().max()) < 1e-10 * float(c["forces"].abs().max())
    assert float((c["forces"] - o["forces"]).abs().max()) < 1e-10 * float(o["forces"].abs().max())
    assert float(((c["stress"] - o["stress"]).abs() / o["scale"].reshape(-1, 1, 1)).max()) < 1e-10


def test_image_ranges_values_and_refusals():
    from gotennet_amd import graph
    cells = torch.tensor([U.CUBE, MU.N1_CELL, MU.N2_CELL, MU.R2_CELL, MU.N3_CELL])
    R = graph.image_ranges(cells, 5.0)
    assert R.dtype == torch.int32 and tuple(R.shape) == (5, 3)
    # floor(5 / w + 1/2 + 1/64): 10.5 -> 0.99;  7.06 / 6.33 / 8.10 -> 1.2 / 1.3 / 1.1;  3.79 / 4.17 / 3.60 -> 1.8 / 1.7 / 1.9;
    # 2.4 / 2.9 / 3.3 -> 2.6 / 2.2 / 2.03;  2.9 -> 2.2
    assert R.tolist() == [[0, 0, 0], [1, 1, 1], [1, 1, 1], [2, 2, 2], [2, 2, 2]]
    assert graph.image_ranges(torch.eye(3) * 10.0, 5.0).tolist() == [[1, 1, 1]]          # exactly 2 * cutoff: 1/2 + 1/2 = 1
    assert graph.image_ranges(torch.eye(3) * 10.4, 5.0).tolist() == [[0, 0, 0]]          # 0.981 + 0.016 < 1
    assert graph.image_ranges(torch.diag(torch.tensor([20.0, 5.0, 1.7])), 5.0).tolist() == [[0, 1, 3]]
    assert graph.image_ranges(torch.eye(3) * 2.0, 6.0).tolist() == [[3, 3, 3]]           # cutoff / 3: the narrowest cell accepted
    for bad in (torch.eye(3) * 1.6, torch.diag(torch.tensor([12.0, 12.0, 1.0])), torch.zeros((3, 3)),
                torch.eye(3) * float("nan"), torch.eye(3) * float("inf"),
                torch.stack([torch.eye(3) * 12.0, torch.eye(3) * 1.6])):
        with pytest.raises(ValueError, match="cutoff / 3"):
            graph.image_ranges(bad, 5.0)
    with pytest.raises(ValueError):
        graph.image_ranges(torch.eye(4), 5.0)
    # a sheared cell: every lattice vector is long, the perpendicular width decides
    skewed = torch.tensor([[10.5, 0.0, 0.0], [10.5, 10.5, 0.0], [0.0, 0.0, 10.5]])     # widths 7.42, 10.5, 10.5
    assert graph.image_ranges(skewed, 5.0).tolist() == [[1, 0, 0]]


def test_resolve_images_and_check_volume():
    from gotennet_amd import graph
    wide, narrow = torch.tensor(U.CUBE), torch.tensor(MU.N2_CELL)
    assert graph.resolve_images(wide, 5.0, "minimum") is None and graph.resolve_images(wide, 5.0, "auto") is None
    assert graph.resolve_images(wide, 5.0, "all").tolist() == [[0, 0, 0]]
    assert graph.resolve_images(torch.stack([wide, narrow]), 5.0, "auto").tolist() == [[0, 0, 0], [1, 1, 1]]
    with pytest.raises(ValueError, match="2 \\* cutoff"):          # today's message
        graph.resolve_images(narrow, 5.0, "minimum")
    with pytest.raises(ValueError):
        graph.resolve_images(wide, 5.0, "some")
    graph.check_volume(narrow * 1.01)
    for bad in (torch.zeros((3, 3)), torch.eye(3) * float("nan"), torch.tensor([[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]])):
        with pytest.raises(ValueError, match="volume"):
            graph.check_volume(bad)


def test_interfaces_and_declarations(repo_root):
    import gotennet_amd
    from gotennet_amd import _lib, engine, graph, pipeline
    header = open(os.path.join(repo_root, "include", "gotennet_hip.h")).read()
    for name in ("gn_radius_count_pbc_images", "gn_radius_fill_pbc_images", "gn_edge_geometry_images", "gn_node_init_images",
                 "gn_node_init_backward_images", "gn_edge_geometry_backward_images", "gn_embedding_grad_images"):
        assert name in _lib.SIGNATURES, name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/gotennet_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert inspect.signature(graph.distance_pbc).parameters["images"].default == "minimum"
    assert inspect.signature(gotennet_amd.GotenNet.forward).parameters["self_images"].default is False
    assert inspect.signature(engine.Graph.__init__).parameters["self_images"].default is False
    assert inspect.signature(pipeline.CapturedStep.__init__).parameters["images"].default == "minimum"
