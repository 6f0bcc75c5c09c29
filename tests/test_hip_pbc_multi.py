"""GPU: periodic cells narrower than twice the cutoff -- the multi-image radius graph against the brute force of
tests/pbc_multi_util.py, and energies, forces, stress and parameter gradients on lists with self-images against the fp64
oracle on a replica of the cell (translation symmetry: the oracle itself cannot run a list with self-images)."""
import functools
import types

import pytest
import torch

from tests import pbc_multi_util as MU
from tests import pbc_util as U
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's bound: energies, forces, parameter gradients (max-norm relative)


def _dev(s):
    return dict(pos=s["pos"].float().cuda(), batch=s["batch"].cuda(), z=s["z"].cuda(), cell=s["cell"].float().cuda())


def _gpu_model(F=32, L=2, lmax=2, seed=1):
    net, head, sd, hsd, cfg = U.make_model(F, L, lmax, seed)
    return net.cuda().eval(), head.cuda().eval(), sd, hsd, cfg


@functools.lru_cache(maxsize=None)
def _reference(name, lmax, params=False):
    """The replica oracle of one system, computed once and shared (read-only)."""
    _, _, sd, hsd, cfg = U.make_model(32, 2, lmax, seed=1)
    return MU.replica_oracle(sd, cfg, hsd, MU.system(name), params=params)


def _launches(fn):
    """The library entry points ``fn()`` calls (the per-launch timer hook, recording names only)."""
    from gotennet_amd import _lib
    calls, old = [], _lib.TIMER
    _lib.TIMER = types.SimpleNamespace(want=lambda name, args: calls.append(name), events=[])
    try:
        fn()
    finally:
        _lib.TIMER = old
    return calls


def _inputs(d, requires_grad=False):
    return types.SimpleNamespace(z=d["z"], pos=d["pos"].clone().requires_grad_(requires_grad), batch=d["batch"], cell=d["cell"])


# ------------------------------------------------------------------------------------------------------------ 1. lists
LIST_CASES = [("n1", 32, "all"), ("n1", 32, "auto"), ("n2", 32, "all"), ("r2", 32, "all"), ("n3", 32, "auto"),
              ("n4", 32, "auto"), ("n4", 32, "all"), ("n5", 32, "all"),
              ("n2", MU.CAP_N2_SPLITS_PAIR, "all"), ("n1", MU.CAP_N1_SECOND_TRIP, "all"), ("r2", MU.CAP_R2_SECOND_TRIP, "all")]


@pytest.mark.parametrize("name,cap,images", LIST_CASES)
def test_distance_pbc_multi_matches_brute_force(name, cap, images):
    from gotennet_amd import engine, graph
    s, d = MU.system(name), _dev(MU.system(name))
    bf = MU.brute_force(s["pos"], s["batch"], s["cell"], MU.CUTOFF, cap)
    MU.assert_input(bf)
    calls = _launches(lambda: d.update(out=graph.distance_pbc(d["pos"], d["batch"], d["cell"], MU.CUTOFF, cap, images=images)))
    ei, ed, ev, sh = d["out"]
    torch.cuda.synchronize()
    assert "gn_radius_count_pbc_images" in calls and "gn_radius_fill_pbc_images" in calls and "gn_radius_fill_pbc" not in calls
    assert ei.dtype == torch.int64 and sh.dtype == torch.int32 and tuple(sh.shape) == (ei.shape[1], 3)
    assert torch.equal(ei.cpu(), bf["edge_index"])
    assert torch.equal(sh.cpu().long(), bf["edge_shift"])
    # the bounds of tests/test_hip_pbc.py for the same quantities
    assert float((ev.cpu().double() - bf["edge_vec"]).abs().max()) <= 1e-5
    assert float((ed.cpu().double() - bf["edge_diff"]).abs().max()) <= 2e-5
    same = ei[0] == ei[1]
    loops = same & (sh == 0).all(1)
    assert int(loops.sum()) == int(((bf["edge_index"][0] == bf["edge_index"][1]) & (bf["edge_shift"] == 0).all(1)).sum())
    assert not bool(ed[loops].any()) and not bool(ev[loops].any())              # exactly 0 on the self-loop ...
    assert bool((ed[~loops] > 0).all())                                          # ... and only there: self-images included
    if name in ("n2", "r2", "n3", "n4"):
        assert int((same & ~loops).sum()) > 0
    # the fixed-list kernel on that list: the fill's bits, self-images included
    net = _gpu_model()[0]
    g = engine.Graph(net.config(), net.packed_weights(), d["pos"].shape[0], ei, self_images=True)
    g.set_periodic(sh, d["batch"], d["cell"])
    g.set_positions(d["pos"])
    torch.cuda.synchronize()
    assert torch.equal(g.edge_vec, ev) and torch.equal(g.edge_diff, ed)
    if s["n_mol"] == 1:                              # a broadcast [3, 3] cell is the same graph
        out2 = graph.distance_pbc(d["pos"], d["batch"], d["cell"][0], MU.CUTOFF, cap, images=images)
        assert all(torch.equal(x, y) for x, y in zip(out2, (ei, ed, ev, sh)))


@pytest.mark.parametrize("name,cap", [("a", 32), ("b", 32), ("c", 32), ("c", U.CAP_SECOND_TRIP)])
def test_all_images_on_wide_cells_is_the_minimum_image_list_bitwise(name, cap):
    from gotennet_amd import graph
    d = _dev(U.system(name))
    ref = graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, cap)
    torch.cuda.synchronize()
    got = graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, cap, images="all")
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, ref))
    # "auto" on wide cells IS the default path: the same launches, the same bits
    base = _launches(lambda: graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, cap))
    auto = _launches(lambda: d.update(out=graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, cap, images="auto")))
    assert auto == base and all(torch.equal(x, y) for x, y in zip(d["out"], ref))


# ------------------------------------------------------------------------------------------ 2. energy, forces, stress
def _check_stress(stress, o, what):
    """As tests/test_hip_pbc.py: max |s_hip - s_ref| <= 1e-4 (1/V) sum_e |r_e| |dE/dr_e| per box, the un-cancelled virial."""
    err = (stress.double().cpu() - o["stress"]).abs().flatten(1).max(1).values
    print(f"{what}: stress err / un-cancelled sum = {(err / o['scale']).tolist()}")
    assert bool((err <= TOL * o["scale"]).all()), (what, (err / o["scale"]).tolist())


def _check_forces(f, o, n_atoms, what):
    """Max-norm relative 1e-4 as tests/test_hip_pbc.py.  A one-atom cell's force vanishes by symmetry (the reference is 0 up
    to fp64 rounding), so there the 1e-4 is carried to the un-cancelled sum of the atom's edge gradients, as for the stress."""
    err = float((f.double().cpu() - o["forces"]).abs().max())
    scale = float(o["forces"].abs().max()) if n_atoms > 1 else o["force_scale"]
    print(f"{what}: forces err / scale = {err / scale:.2e} (scale {scale:.3e})")
    assert err < TOL * scale, (what, err / scale)


@pytest.mark.parametrize("name,lmax", [("n1", 2), ("n2", 2), ("r2", 2), ("n4", 2), ("n2", 3)])
def test_energy_forces_stress_match_replica_oracle(name, lmax, gemm_mode):
    from gotennet_amd import graph
    from gotennet_amd.pipeline import EnergyForces
    o = _reference(name, lmax)
    s, d = MU.system(name), _dev(MU.system(name))
    bf = MU.brute_force(s["pos"], s["batch"], s["cell"])
    MU.assert_input(bf, 32)
    net, head, *_ = _gpu_model(32, 2, lmax)
    ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], MU.CUTOFF, 32, images="auto")
    assert torch.equal(ei.cpu(), bf["edge_index"]) and torch.equal(sh.cpu().long(), bf["edge_shift"])
    ef = EnergyForces(net, head, check_edges=False)
    e, f, stress = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"])
    torch.cuda.synchronize()
    what = f"{name} lmax {lmax} {gemm_mode}"
    print(f"{what}: energy rel err {rel_err(e.cpu(), o['energy']):.2e} (energy {o['energy'].flatten().tolist()})")
    assert rel_err(e.cpu(), o["energy"]) < TOL
    _check_forces(f, o, s["pos"].shape[0], what)
    _check_stress(stress, o, what)
    e2, f2, s2 = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"])
    assert torch.equal(e, e2) and torch.equal(f, f2) and torch.equal(stress, s2)
    if name == "n1":            # no self-images: the two self-loop rules pick the same edges, so the plain call gives the same bits
        e0, f0 = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"])
        assert torch.equal(e, e0) and torch.equal(f, f0)


# ------------------------------------------------------------------------------------------------ 3. parameter gradients
def test_parameter_gradients_match_replica_oracle(gemm_mode):
    s, d = MU.system("n2"), _dev(MU.system("n2"))
    ref = _reference("n2", 2, params=True)["param_grads"]
    net, head, *_ = _gpu_model()
    net.periodic = "all"
    net.parameter_grads = head.parameter_grads = True
    inp = _inputs(d)
    inp.representation, inp.vector_representation = net(inp)
    head.derivative = None
    head(inp)["property"].sum().backward()
    grads = {n: p.grad.clone() for n, p in net.named_parameters()}
    grads.update({"head." + n: p.grad.clone() for n, p in head.named_parameters()})
    worst = 0.0
    for n, g in grads.items():
        r = ref[n]
        m = float(r.abs().max())
        err = float((g.double().cpu() - r).abs().max()) / m if m > 0 else float(g.abs().max())
        worst = max(worst, err)
        assert err <= TOL, (n, err)
    print(f"n2 parameter gradients {gemm_mode}: worst rel err {worst:.2e} over {len(grads)} tensors")


# ------------------------------------------------------------------------------------- 4. captured step and the wrapper
def test_captured_step_on_a_list_with_self_images(gemm_mode):
    from gotennet_amd import engine, graph
    from gotennet_amd.pipeline import CapturedStep, EnergyForces
    s, d = MU.system("n2"), _dev(MU.system("n2"))
    net, head, *_ = _gpu_model()
    ef = EnergyForces(net, head, check_edges=False)
    ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], MU.CUTOFF, 32, images="all")
    step = CapturedStep(ef, d["z"], ei, d["batch"], s["n_mol"], cell=d["cell"], edge_shift=sh, images="all")
    torch.cuda.synchronize()

    def eager(pos, cell):                            # the same FIXED list at this geometry
        g = engine.Graph(net.config(), net.packed_weights(), pos.shape[0], ei, self_images=True)
        g.set_periodic(sh, d["batch"], cell)
        g.set_positions(pos)
        return ef(d["z"], ei, g.edge_diff, g.edge_vec, d["batch"], s["n_mol"], cell=cell)

    gen = torch.Generator().manual_seed(9)
    move = (torch.rand(s["pos"].shape, generator=gen, dtype=torch.float64) * 2 - 1) * 0.02
    pos, cell = ((s["pos"] + move) * 1.01).float().cuda(), (s["cell"] * 1.01).float().cuda()
    for p, c in ((d["pos"], None), (pos, cell), (d["pos"], d["cell"])):
        got = [t.clone() for t in (step(p) if c is None else step(p, cell=c))]
        torch.cuda.synchronize()
        want = eager(p, d["cell"] if c is None else c)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(got, want))
    e0, f0, s0 = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"])
    assert all(torch.equal(x, y) for x, y in zip(got, (e0, f0, s0)))


def test_wrapper_on_a_narrow_cell(gemm_mode):
    from gotennet_amd import graph
    from gotennet_amd.pipeline import EnergyForces
    s, d = MU.system("n2"), _dev(MU.system("n2"))
    net, head, *_ = _gpu_model()
    ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], MU.CUTOFF, 32, images="all")
    e_ref, f_ref, _ = EnergyForces(net, head, check_edges=False)(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"])
    for mode in ("all", "auto"):
        net.periodic = mode
        inp = _inputs(d, requires_grad=True)
        inp.representation, inp.vector_representation = net(inp)
        out = head(inp)
        assert rel_err(out["property"].detach().cpu(), e_ref.cpu()) < TOL
        assert rel_err(out["forces"].detach().cpu(), f_ref.cpu()) < TOL
        with torch.no_grad():                        # the no-grad route builds the same graph
            h, X = net(_inputs(d))
        assert rel_err(h, inp.representation.detach()) < 1e-5


# ------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_before_any_launch():
    from gotennet_amd import graph
    from gotennet_amd.pipeline import CapturedStep, EnergyForces
    s, d = MU.system("n2"), _dev(MU.system("n2"))
    net, head, *_ = _gpu_model()
    ef = EnergyForces(net, head, check_edges=False)
    ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], MU.CUTOFF, 32, images="all")
    step = CapturedStep(ef, d["z"], ei, d["batch"], s["n_mol"], cell=d["cell"], edge_shift=sh, images="all")
    torch.cuda.synchronize()
    tiny = torch.eye(3, device="cuda").unsqueeze(0) * 1.6          # width < cutoff / 3
    nan = d["cell"].clone()
    nan[0, 1, 1] = float("nan")
    flat = d["cell"].clone()
    flat[0, 2] = flat[0, 1]                                        # zero volume
    pnet = _gpu_model()[0]

    def wrapper(cell, mode):
        def run():
            pnet.periodic = mode
            inp = _inputs(d)
            inp.cell = cell
            pnet(inp)
        return run

    def dist(cell, **kw):
        return lambda: graph.distance_pbc(d["pos"], d["batch"], cell, MU.CUTOFF, 32, **kw)

    cases = [(dist(tiny, images="all"), "cutoff / 3"), (dist(tiny, images="auto"), "cutoff / 3"),
             (dist(nan, images="all"), "cutoff / 3"), (dist(nan, images="auto"), "cutoff / 3"),
             (dist(d["cell"], images="minimum"), "2 \\* cutoff"), (dist(d["cell"]), "2 \\* cutoff"),
             (dist(d["cell"], images="some"), "images"),
             (wrapper(tiny, "all"), "cutoff / 3"), (wrapper(nan, "auto"), "cutoff / 3"), (wrapper(d["cell"], True), "2 \\* cutoff"),
             (lambda: CapturedStep(ef, d["z"], ei, d["batch"], s["n_mol"], cell=tiny, edge_shift=sh, images="all"), "cutoff / 3"),
             (lambda: CapturedStep(ef, d["z"], ei, d["batch"], s["n_mol"], cell=d["cell"], edge_shift=sh), "2 \\* cutoff"),
             (lambda: step(d["pos"], cell=flat), "volume"), (lambda: step(d["pos"], cell=nan), "volume")]
    for k, (fn, msg) in enumerate(cases):
        def refused():
            with pytest.raises(ValueError, match=msg):
                fn()
        assert _launches(refused) == [], k
    e1, f1, s1 = (t.clone() for t in step(d["pos"]))               # the refused cells never reached the recorded buffers
    e0, f0, s0 = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"])
    torch.cuda.synchronize()
    assert torch.equal(e1, e0) and torch.equal(f1, f0) and torch.equal(s1, s0)


def test_forward_keeps_the_index_rule_unless_asked():
    """``GotenNet.forward`` without ``self_images=True`` is what it was: the entry points that tell a self-loop by index, so
    on a list with self-images it drops them from NodeInit.  With the flag the *_images entry points run; on a list without
    self-images (n1) the two give the same bits."""
    import gotennet_amd
    from gotennet_amd import graph
    net = _gpu_model()[0]
    fwd = functools.partial(gotennet_amd.GotenNet.forward, net)
    out = {}
    for name in ("n2", "n1"):
        d = _dev(MU.system(name))
        ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], MU.CUTOFF, 32, images="all")
        with torch.no_grad():
            plain = _launches(lambda: out.update(plain=fwd(d["z"], ei, ed, ev, _sorted=True)))
            flagged = _launches(lambda: out.update(flagged=fwd(d["z"], ei, ed, ev, _sorted=True, self_images=True)))
        torch.cuda.synchronize()
        assert "gn_node_init" in plain and "gn_edge_geometry" in plain and not any(c.endswith("_images") for c in plain)
        assert "gn_node_init_images" in flagged and "gn_edge_geometry_images" in flagged
        assert "gn_node_init" not in flagged and "gn_edge_geometry" not in flagged
        same = torch.equal(out["plain"][0], out["flagged"][0]) and torch.equal(out["plain"][1], out["flagged"][1])
        assert same == (name == "n1"), name
