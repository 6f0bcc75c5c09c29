"""GPU: periodic boundary conditions -- the minimum-image radius graph, the fixed-list edge vectors, the virial kernel, the
periodic captured step and the wrapper's opt-in route, against the fp64 yardstick of tests/pbc_util.py."""
import functools
import types

import pytest
import torch

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
def _reference(name, lmax, cap=32, scale=1.0):
    """The yardstick of one system, computed once and shared (read-only): the brute-force list and the oracle on it.
    ``scale``: positions and cell scaled alike, evaluated on the UNSCALED system's list (the captured step's fixed list)."""
    s = U.system(name)
    bf = U.brute_force(s["pos"], s["batch"], s["cell"], U.CUTOFF, cap)
    U.assert_gap(bf)
    _, _, sd, hsd, cfg = U.make_model(32, 2, lmax, seed=1)
    pos, cell = (s["pos"] * scale).float().double(), (s["cell"] * scale).float().double()
    return bf, U.oracle_efs(sd, cfg, hsd, s, bf["edge_index"], bf["edge_shift"], pos=pos, cell=cell)


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


def _check_stress(stress, o, what):
    """max |s_hip - s_ref| <= 1e-4 (1/V) sum_e |r_e| |dE/dr_e| per box: the project's 1e-4 carried to the un-cancelled sum
    (the virial cancels three- to ten-fold on these inputs; a bound relative to max |s| would test the cancellation)."""
    err = (stress.double().cpu() - o["stress"]).abs().flatten(1).max(1).values
    big = o["stress"].abs().flatten(1).max(1).values
    for m in range(err.shape[0]):
        print(f"{what} box {m}: stress err / un-cancelled sum = {float(err[m] / o['scale'][m]):.2e}, "
              f"err / max|stress| = {float(err[m] / big[m]):.2e} (cancellation {float(o['scale'][m] / big[m]):.1f}x)")
    assert bool((err <= TOL * o["scale"]).all()), (what, (err / o["scale"]).tolist())


# ---------------------------------------------------------------------------------------------------- 1. the radius graph
GRAPH_CASES = [("a", 32), ("b", 32), ("d", 32), ("e", 32)] + [("c", cap) for cap in U.CAPS_C]


@pytest.mark.parametrize("name,cap", GRAPH_CASES)
def test_distance_pbc_matches_brute_force(name, cap):
    from gotennet_amd import engine, graph
    s, d = U.system(name), _dev(U.system(name))
    bf = U.brute_force(s["pos"], s["batch"], s["cell"], U.CUTOFF, cap)
    U.assert_gap(bf)
    ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, cap)
    torch.cuda.synchronize()
    assert ei.dtype == torch.int64 and sh.dtype == torch.int32 and tuple(sh.shape) == (ei.shape[1], 3)
    assert torch.equal(ei.cpu(), bf["edge_index"])
    assert torch.equal(sh.cpu().long(), bf["edge_shift"])
    assert float((ev.cpu().double() - bf["edge_vec"]).abs().max()) <= 1e-5
    # |v| from three components each within 6e-6 (a fp32 subtraction and three fmaf on magnitudes up to 60 A)
    assert float((ed.cpu().double() - bf["edge_diff"]).abs().max()) <= 2e-5
    loops = ei[0] == ei[1]
    # (a cap that bites drops the self-loop of a target whose first `cap` sources all come before it: the list decides)
    assert int(loops.sum()) == (s["pos"].shape[0] if cap >= 32 else int((bf["edge_index"][0] == bf["edge_index"][1]).sum()))
    assert not bool(ed[loops].any()) and not bool(ev[loops].any())
    # the fixed-list kernel on that list: the fill's bits
    net = _gpu_model()[0]
    g = engine.Graph(net.config(), net.packed_weights(), d["pos"].shape[0], ei)
    g.set_periodic(sh, d["batch"], d["cell"])
    g.set_positions(d["pos"])
    torch.cuda.synchronize()
    assert torch.equal(g.edge_vec, ev) and torch.equal(g.edge_diff, ed)
    # a broadcast [3, 3] cell is the same graph
    if s["n_mol"] == 1:
        ei2, ed2, ev2, sh2 = graph.distance_pbc(d["pos"], d["batch"], d["cell"][0], U.CUTOFF, cap)
        assert torch.equal(ei2, ei) and torch.equal(sh2, sh) and torch.equal(ev2, ev) and torch.equal(ed2, ed)


# ------------------------------------------------------------------------------------------ 2. energy, forces, stress
@pytest.mark.parametrize("name,lmax", [("a", 2), ("c", 2), ("a", 3)])
def test_energy_forces_stress_match_oracle(name, lmax, gemm_mode):
    from gotennet_amd import graph
    from gotennet_amd.pipeline import EnergyForces
    bf, o = _reference(name, lmax)
    s, d = U.system(name), _dev(U.system(name))
    net, head, *_ = _gpu_model(32, 2, lmax)
    ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, 32)
    assert torch.equal(ei.cpu(), bf["edge_index"])
    ef = EnergyForces(net, head, check_edges=False)
    e, f, stress = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"])
    e0, f0 = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"])
    torch.cuda.synchronize()
    assert torch.equal(e, e0) and torch.equal(f, f0)               # the cell adds the stress, nothing else
    assert tuple(stress.shape) == (s["n_mol"], 3, 3)
    print(f"{name} lmax {lmax} {gemm_mode}: energy rel err {rel_err(e.cpu(), o['energy']):.2e}, "
          f"forces rel err {rel_err(f.cpu(), o['forces']):.2e}")
    assert rel_err(e.cpu(), o["energy"]) < TOL
    assert rel_err(f.cpu(), o["forces"]) < TOL
    _check_stress(stress, o, f"{name} lmax {lmax} {gemm_mode}")
    e2, f2, stress2 = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"])
    assert torch.equal(stress, stress2)
    e3, f3, s3 = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"], forces=False)
    assert torch.equal(e3, e) and f3 is None and s3 is None


# -------------------------------------------------------------------------------------------------- 3. gn_virial alone
def test_virial_kernel_alone():
    """The oracle's edge gradients cast to fp32, with an EMPTY box put between the two boxes of system (a).  Reference: the
    same fp32 numbers summed in fp64.  Bound per box: (n_edges + 2) 2^-24 sum |r| |g| / V, the worst case of any fp32
    summation order (n_edges - 1 additions, the products, the division)."""
    from gotennet_amd._lib import call, ptr
    bf, o = _reference("a", 2)
    s = U.system("a")
    ev, gv, gd = o["edge_vec"].float(), o["g_vec"].float(), o["g_diff"].float()
    n0 = int((s["batch"] == 0).sum())
    mol_ptr = torch.tensor([0, n0, n0, s["pos"].shape[0]], dtype=torch.int32)
    deg = torch.bincount(bf["edge_index"][1], minlength=s["pos"].shape[0])
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).to(torch.int32)
    vol = torch.tensor([float(o["volume"][0]), 1.0, float(o["volume"][1])], dtype=torch.float32)
    r, nrm = ev.double(), ev.double().norm(dim=1, keepdim=True)
    g = gv.double() + torch.where(nrm > 0, gd.double().unsqueeze(1) * r / nrm.clamp_min(1e-300), torch.zeros_like(r))
    box = torch.tensor([0, 2])[s["batch"][bf["edge_index"][1]]]
    ref = torch.zeros((3, 3, 3), dtype=torch.float64).index_add_(0, box, r.unsqueeze(2) * g.unsqueeze(1)) / vol.double().reshape(3, 1, 1)
    mass = torch.zeros(3, dtype=torch.float64).index_add_(0, box, r.norm(dim=1) * g.norm(dim=1)) / vol.double()
    n_edges = torch.bincount(box, minlength=3)
    outs = []
    dv = [t.cuda() for t in (gv, gd, ev, rowptr, mol_ptr, vol)]
    for _ in range(2):
        out = torch.full((3, 3, 3), float("nan"), dtype=torch.float32, device="cuda")
        call("gn_virial", *[ptr(t) for t in dv[:5]], 3, ptr(dv[5]), ptr(out), torch.cuda.current_stream().cuda_stream)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0][1].cpu(), torch.zeros(3, 3))        # the empty box
    err = (outs[0].double().cpu() - ref).abs().flatten(1).max(1).values
    bound = (n_edges + 2).double() * 2.0 ** -24 * mass
    print("gn_virial: err", err.tolist(), "bound", bound.tolist())
    assert bool((err[[0, 2]] <= bound[[0, 2]]).all()) and float(mass[[0, 2]].min()) > 0


# ------------------------------------------------------------------------------------------------ 4. the captured step
def _perturbed(s, k):
    """Position set k of system ``s``: small moves (fp32-representable).  Asserts that the edge list stays the brute-force
    list of the unperturbed system, away from the cutoff."""
    g = torch.Generator().manual_seed(40 + k)
    pos = (s["pos"] + 0.001 * k * torch.randn(s["pos"].shape, generator=g, dtype=torch.float64)).float().double()
    bf0 = U.brute_force(s["pos"], s["batch"], s["cell"])
    bf = U.brute_force(pos, s["batch"], s["cell"])
    U.assert_gap(bf)
    assert torch.equal(bf["edge_index"], bf0["edge_index"]) and torch.equal(bf["edge_shift"], bf0["edge_shift"])
    return pos


def test_captured_step_with_cell(gemm_mode):
    from gotennet_amd import graph
    from gotennet_amd.pipeline import CapturedStep, EnergyForces
    s, d = U.system("a"), _dev(U.system("a"))
    net, head, *_ = _gpu_model()
    ef = EnergyForces(net, head, check_edges=False)
    ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, 32)
    step = CapturedStep(ef, d["z"], ei, d["batch"], s["n_mol"], cell=d["cell"], edge_shift=sh)
    torch.cuda.synchronize()
    for k in (1, 2, 3):
        p = _perturbed(s, k).float().cuda()
        e_g, f_g, s_g = (t.clone() for t in step(p))
        torch.cuda.synchronize()
        ei_k, ed_k, ev_k, sh_k = graph.distance_pbc(p, d["batch"], d["cell"], U.CUTOFF, 32)
        assert torch.equal(ei_k, ei) and torch.equal(sh_k, sh)
        e_e, f_e, s_e = ef(d["z"], ei_k, ed_k, ev_k, d["batch"], s["n_mol"], cell=d["cell"])
        torch.cuda.synchronize()
        assert torch.equal(e_g, e_e) and torch.equal(f_g, f_e) and torch.equal(s_g, s_e), k
    # a barostat's move: cell and positions scaled by 1.01.  The recorded list is FIXED (pairs that cross the cutoff keep
    # their edge, with a zero cutoff weight; pairs that enter it are not seen), so the oracle runs on the same fixed list.
    _, o = _reference("a", 2, 32, 1.01)
    pos, cell = (s["pos"] * 1.01).float().cuda(), (s["cell"] * 1.01).float().cuda()
    e, f, stress = (t.clone() for t in step(pos, cell=cell))
    torch.cuda.synchronize()
    print(f"captured, cell x 1.01, {gemm_mode}: energy rel err {rel_err(e.cpu(), o['energy']):.2e}, "
          f"forces rel err {rel_err(f.cpu(), o['forces']):.2e}")
    assert rel_err(e.cpu(), o["energy"]) < TOL and rel_err(f.cpu(), o["forces"]) < TOL
    _check_stress(stress, o, f"captured x 1.01 {gemm_mode}")
    # the recorded graph follows the cell buffer: back to the first cell, the first result
    e1, f1, s1 = (t.clone() for t in step(d["pos"], cell=d["cell"]))
    torch.cuda.synchronize()
    e_e, f_e, s_e = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"])
    torch.cuda.synchronize()
    assert torch.equal(e1, e_e) and torch.equal(f1, f_e) and torch.equal(s1, s_e)


def test_periodic_calls_leave_the_replay_counter_alone():
    """EnergyForces(replay=True): calls with ``cell`` run eagerly, record nothing and do not bring the recording of the
    plain path forward -- it still takes ``replay_after`` plain calls on the topology."""
    from gotennet_amd import graph
    from gotennet_amd.pipeline import EnergyForces
    s, d = U.system("a"), _dev(U.system("a"))
    net, head, *_ = _gpu_model()
    ef = EnergyForces(net, head, check_edges=False, replay=True, replay_after=2)
    ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, 32)
    outs = [ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"]) for _ in range(4)]
    torch.cuda.synchronize()
    assert ef._graph_state is None and all(torch.equal(o[2], outs[0][2]) for o in outs)
    e1, f1 = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"])
    assert ef._graph_state is None                                 # the first plain repeat of this topology: still eager
    e2, f2 = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"])
    torch.cuda.synchronize()
    assert ef._graph_state is not None                             # the second: recorded and replayed
    assert torch.equal(e1, e2) and torch.equal(f1, f2) and torch.equal(f1, outs[0][1])
    e3, f3, s3 = ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=d["cell"])      # eager again, the record stays
    torch.cuda.synchronize()
    assert ef._graph_state is not None and torch.equal(s3, outs[0][2]) and torch.equal(f3, f1)


# --------------------------------------------------------------------------------------------------------- 5. the wrapper
def _inputs(d, requires_grad=False, cell=True):
    pos = d["pos"].clone().requires_grad_(requires_grad)
    inp = types.SimpleNamespace(z=d["z"], pos=pos, batch=d["batch"])
    if cell:
        inp.cell = d["cell"]
    return inp


def test_wrapper_periodic_forces(gemm_mode):
    from gotennet_amd import graph
    from gotennet_amd.pipeline import EnergyForces
    s, d = U.system("a"), _dev(U.system("a"))
    net, head, *_ = _gpu_model()
    ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, 32)
    e_ref, f_ref = EnergyForces(net, head, check_edges=False)(d["z"], ei, ed, ev, d["batch"], s["n_mol"])
    net.periodic = True
    inp = _inputs(d, requires_grad=True)
    inp.representation, inp.vector_representation = net(inp)
    out = head(inp)
    assert rel_err(out["property"].detach().cpu(), e_ref.cpu()) < TOL
    assert rel_err(out["forces"].detach().cpu(), f_ref.cpu()) < TOL
    with torch.no_grad():                                          # the no-grad route builds the same graph
        h, X = net(_inputs(d))
    assert rel_err(h, inp.representation.detach()) < 1e-5
    # periodic = False: an inputs.cell is ignored, today's isolated-molecule result
    net.periodic = False
    with torch.no_grad():
        h0, X0 = net(_inputs(d))
        h1, X1 = net(_inputs(d, cell=False))
    assert torch.equal(h0, h1) and torch.equal(X0, X1) and not torch.equal(h0, h)


def test_wrapper_periodic_parameter_gradients(gemm_mode):
    s, d = U.system("a"), _dev(U.system("a"))
    bf = U.brute_force(s["pos"], s["batch"], s["cell"])
    net, head, sd, hsd, cfg = _gpu_model()
    ref = U.oracle_efs(sd, cfg, hsd, s, bf["edge_index"], bf["edge_shift"], params=True)["param_grads"]
    net.periodic = True
    net.parameter_grads = head.parameter_grads = True
    got = []
    for forces in (False, True):                                   # parameter_grads alone, and with pos.requires_grad
        net.zero_grad(set_to_none=True), head.zero_grad(set_to_none=True)
        inp = _inputs(d, requires_grad=forces)
        inp.representation, inp.vector_representation = net(inp)
        head.derivative = "forces" if forces else None             # (logged forces need a pos that requires grad)
        head(inp)["property"].sum().backward()
        grads = {n: p.grad.clone() for n, p in net.named_parameters()}
        grads.update({"head." + n: p.grad.clone() for n, p in head.named_parameters()})
        got.append(grads)
    worst = 0.0
    for n, g in got[0].items():
        assert torch.equal(g, got[1][n]), n
        r = ref[n]
        m = float(r.abs().max())
        err = float((g.double().cpu() - r).abs().max()) / m if m > 0 else float(g.abs().max())
        worst = max(worst, err)
        assert err <= TOL, (n, err)
    print(f"periodic parameter gradients {gemm_mode}: worst rel err {worst:.2e} over {len(got[0])} tensors")


# ------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_before_any_launch():
    from gotennet_amd import graph
    from gotennet_amd.pipeline import CapturedStep, EnergyForces
    s, d = U.system("a"), _dev(U.system("a"))
    net, head, *_ = _gpu_model()
    ef = EnergyForces(net, head, check_edges=False)
    ei, ed, ev, sh = graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, 32)
    small = d["cell"].clone()
    small[1] = torch.eye(3, device="cuda") * 9.9
    grad_cell = d["cell"].clone().requires_grad_(True)
    pnet = _gpu_model()[0]
    pnet.periodic = True

    def wrapper(cell, requires_grad):
        inp = _inputs(d, requires_grad=requires_grad)
        inp.cell = cell
        return lambda: pnet(inp)

    cases = [
        lambda: graph.distance_pbc(d["pos"], d["batch"], small, U.CUTOFF, 32),
        lambda: graph.distance_pbc(d["pos"], d["batch"], grad_cell, U.CUTOFF, 32),
        wrapper(small, False), wrapper(small, True), wrapper(grad_cell, False), wrapper(grad_cell, True),
        lambda: ef(d["z"], ei, ed, ev, d["batch"], s["n_mol"], cell=grad_cell),
        lambda: CapturedStep(ef, d["z"], ei, d["batch"], s["n_mol"], edge_shift=sh),
        lambda: CapturedStep(ef, d["z"], ei, d["batch"], s["n_mol"], cell=d["cell"]),
        lambda: CapturedStep(ef, d["z"], ei, d["batch"], s["n_mol"], cell=small, edge_shift=sh),
    ]
    for k, fn in enumerate(cases):
        def refused():
            with pytest.raises(ValueError):
                fn()
        assert _launches(refused) == [], k
