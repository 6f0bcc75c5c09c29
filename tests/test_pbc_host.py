"""Periodic boundary conditions, host side (no GPU): the cell check, the brute-force yardstick against an independent
enumeration, the virial identity the stress kernel relies on (fp64 oracle), and the C ABI declarations."""
import os
import re

import pytest
import torch

from tests import pbc_util as U


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_check_cell_accepts_the_test_cells(name):
    from gotennet_amd import graph
    s = U.system(name)
    w = graph.check_cell(s["cell"], U.CUTOFF)
    assert w.dtype == torch.float64 and tuple(w.shape) == (s["n_mol"], 3) and bool((w >= 2 * U.CUTOFF).all())
    graph.check_cell(s["cell"].float(), U.CUTOFF)                 # fp32 input, still judged in fp64
    graph.check_cell(s["cell"][0], U.CUTOFF)                      # a [3, 3] cell


def test_cell_widths_values():
    from gotennet_amd import graph
    w = graph.cell_widths(torch.tensor([U.ORTHO, U.TRICLINIC, U.LEFT_HANDED]))
    assert torch.allclose(w[0], torch.tensor([10.2, 10.8, 11.5], dtype=torch.float64), atol=1e-12)
    # triclinic: a x b = (0, 0, 115.5) -> the c width is |c_z| = 12; V = 10.5 * 11 * 12
    assert abs(float(w[1, 2]) - 12.0) < 1e-12
    a, b, c = (torch.tensor(v, dtype=torch.float64) for v in U.TRICLINIC)
    assert abs(float(w[1, 0]) - 1386.0 / float(torch.linalg.cross(b, c).norm())) < 1e-12
    assert torch.allclose(w[2], w[1][[1, 0, 2]], atol=1e-12)      # the left-handed cell: rows swapped, same widths


def test_check_cell_refuses_small_and_skewed_cells():
    from gotennet_amd import graph
    with pytest.raises(ValueError, match="2 \\* cutoff"):
        graph.check_cell(torch.eye(3) * 9.9, 5.0)
    # every lattice vector is longer than 10, but the shear leaves a perpendicular width of 10.5 / sqrt(2) = 7.4
    skewed = torch.tensor([[10.5, 0.0, 0.0], [10.5, 10.5, 0.0], [0.0, 0.0, 10.5]])
    assert float(skewed.norm(dim=1).min()) > 10.0
    with pytest.raises(ValueError, match="2 \\* cutoff"):
        graph.check_cell(skewed, 5.0)
    # one bad box among good ones, and a singular cell
    with pytest.raises(ValueError, match="cell 1"):
        graph.check_cell(torch.stack([torch.eye(3) * 12.0, skewed]), 5.0)
    with pytest.raises(ValueError):
        graph.check_cell(torch.zeros((3, 3)), 5.0)
    with pytest.raises(ValueError):
        graph.check_cell(torch.eye(4), 5.0)


@pytest.mark.parametrize("name", ["a", "e"])
def test_brute_force_agrees_with_27_image_enumeration(name):
    """Wrapped systems: every pair is within one cell, so the 27 nearest images hold every hit."""
    s = U.system(name)
    bf = U.brute_force(s["pos"], s["batch"], s["cell"], U.CUTOFF, max_num_neighbors=10 ** 6)
    U.assert_gap(bf)
    got = {(int(j), int(i)) + tuple(int(x) for x in sh) for j, i, sh in zip(bf["edge_index"][0], bf["edge_index"][1], bf["edge_shift"])}
    assert len(got) == bf["edge_index"].shape[1]
    assert got == U.enumerate_27(s["pos"], s["batch"], s["cell"], U.CUTOFF)
    # target-major, sources ascending; the self-loop with shift 0 and distance 0
    key = bf["edge_index"][1] * 10 ** 6 + bf["edge_index"][0]
    assert bool((key[1:] > key[:-1]).all())
    loops = bf["edge_index"][0] == bf["edge_index"][1]
    assert int(loops.sum()) == s["pos"].shape[0] and not bool(bf["edge_shift"][loops].any()) and not bool(bf["edge_diff"][loops].any())


def test_unwrapped_system_has_the_wrapped_graph():
    """(b) is (a) moved by lattice vectors: same edges, same edge vectors, other shifts."""
    a, b = U.system("a"), U.system("b")
    fa, fb = (U.brute_force(s["pos"], s["batch"], s["cell"]) for s in (a, b))
    U.assert_gap(fb)
    assert torch.equal(fa["edge_index"], fb["edge_index"]) and not torch.equal(fa["edge_shift"], fb["edge_shift"])
    # (both systems are rounded to fp32 after the move: two coordinates of up to 40 A, half an ulp = 1.9e-6 each)
    assert float((fa["edge_vec"] - fb["edge_vec"]).abs().max()) < 1e-5
    assert int(fb["edge_shift"].abs().max()) > 2                   # beyond what an enumeration of the raw positions would cover


def test_cap_systems():
    """(c): 70 atoms, so a target's scan takes two 64-lane trips; cap 64 never bites, cap 16 bites in the first trip and
    ``U.CAP_SECOND_TRIP`` inside the second one for some targets (a statement about the input)."""
    s = U.system("c")
    bf = U.brute_force(s["pos"], s["batch"], s["cell"], U.CUTOFF, 64)
    U.assert_gap(bf)
    hits = bf["hits"][0]
    total, first = hits.sum(1), hits[:, :64].sum(1)
    assert int(total.max()) < 64 and int(total.min()) > 16
    assert int(((first < U.CAP_SECOND_TRIP) & (total > U.CAP_SECOND_TRIP)).sum()) >= 5
    for cap in (16, U.CAP_SECOND_TRIP):
        e = U.brute_force(s["pos"], s["batch"], s["cell"], U.CUTOFF, cap)["edge_index"]
        assert int(torch.bincount(e[1]).max()) == cap


@pytest.mark.parametrize("name,lmax", [("a", 2), ("c", 2), ("e", 3)])
def test_virial_identity_fp64(name, lmax):
    """sum_e r_e (x) dE/dr_e equals autograd's dE/d(eps) through a strain of positions and cell: the identity gn_virial
    relies on.  1e-10 relative to the un-cancelled sum (measured ~1e-15); for lmax = 2 the antisymmetric part vanishes (rotation invariance)."""
    s = U.system(name)
    _, _, sd, hsd, cfg = U.make_model(32, 2, lmax, seed=1)
    bf = U.brute_force(s["pos"], s["batch"], s["cell"])
    o = U.oracle_efs(sd, cfg, hsd, s, bf["edge_index"], bf["edge_shift"])
    scale = o["scale"].reshape(-1, 1, 1)
    assert float(o["scale"].min()) > 0
    assert float(((o["virial"] - o["stress"]).abs() / scale).max()) < 1e-10
    if lmax == 2:      # (the lmax = 3 model's stress has a 1e-2 antisymmetric part in the oracle itself: it is returned as computed)
        assert float(((o["stress"] - o["stress"].transpose(1, 2)).abs() / scale).max()) < 1e-10
    assert float(o["forces"].sum(0).abs().max()) < 1e-10 * float(o["forces"].abs().max()) * s["pos"].shape[0]


def test_new_symbols_declared_in_header_and_signatures(repo_root):
    from gotennet_amd import _lib
    header = open(os.path.join(repo_root, "include", "gotennet_hip.h")).read()
    for name in ("gn_cell_prepare", "gn_radius_count_pbc", "gn_radius_fill_pbc", "gn_edge_vectors_pbc", "gn_virial"):
        assert name in _lib.SIGNATURES, name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/gotennet_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.ABI_VERSION == 11 and "#define GN_ABI_VERSION 11" in header      # additive entries: the ABI number stays


def test_host_interfaces_exist():
    import inspect
    import gotennet_amd
    from gotennet_amd import engine, graph, pipeline
    assert gotennet_amd.GotenNetWrapper.periodic is False
    assert "cell" in inspect.signature(pipeline.EnergyForces.__call__).parameters
    p = inspect.signature(pipeline.CapturedStep.__init__).parameters
    assert p["cell"].default is None and p["edge_shift"].default is None
    assert "cell" in inspect.signature(engine.Graph.set_positions).parameters and callable(engine.virial)
    with pytest.raises(gotennet_amd._lib.GotenNetHipError):       # no CPU fallback
        graph.distance_pbc(torch.zeros((2, 3)), torch.zeros(2, dtype=torch.long), torch.eye(3) * 12, 5.0)
