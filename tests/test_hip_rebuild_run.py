"""GPU: the neighbour list rebuilt inside the step.  ``pipeline.RebuiltStep`` is held bit for bit to the eager step on the
host-built padded list (the same kernels on the same inputs) and to ``EnergyForces`` on the unpadded list (bit for bit in the
"f32" and "split" arithmetics, whose rows do not depend on what else is in the batch; 1e-4 relative in "f16x2");
``MDRun`` / ``Relax`` with ``rebuild="device"``: recorded equals eager after every step, and in "f32" / "split" both are the
``rebuild="host"`` trajectory."""
import functools

import pytest
import torch

from tests import fire_util as FU
from tests import md_util as MU
from tests import pbc_multi_util as PM
from tests import pbc_util as U
from tests import rebuild_util as RU

pytestmark = pytest.mark.gpu

DT, FORCE_SCALE, STEPS = 0.2, 0.05, 24                                 # tests/test_hip_md_run.py's set-up
THERMOSTAT = dict(kT=0.02, gamma=0.5, key=(77, 5))
F16X2_BOUND = 1e-4                                                     # the project's relative bound of the f16x2 arithmetic


@functools.lru_cache(maxsize=None)
def _model():
    net, head, *_ = U.make_model(32, 2, 2, seed=1)
    return net.cuda().eval(), head.cuda().eval()


def _ef():
    from gotennet_amd.pipeline import EnergyForces
    return EnergyForces(*_model(), check_edges=False)


# ------------------------------------------------------------------------------------------------ RebuiltStep
SYSTEMS = ("molecules", "a", "n1")


@functools.lru_cache(maxsize=None)
def _system(name):
    """-> dict(z, batch, n_mol, cell or None, images, positions: three sets, the second a displacement of the first)."""
    if name == "molecules":
        s = MU.md_molecules()
        moved = s["pos"].clone()
        moved[6, 0] += 0.3                                             # 4.88 -> 5.18 from the other end: the pair leaves the list
        moved[1] += torch.tensor([0.05, -0.1, 0.02])
        return dict(z=s["z"], batch=s["batch"], n_mol=3, cell=None, images="minimum", positions=(s["pos"], moved, s["pos"]))
    images = "all" if name == "n1" else "minimum"
    s = (PM if images == "all" else U).system(name)
    pos = s["pos"].float()
    moved = pos + 0.3 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(4))
    return dict(z=s["z"], batch=s["batch"], n_mol=s["n_mol"], cell=s["cell"].float(), images=images, positions=(pos, moved, pos))


def _host_list(s, pos):
    from gotennet_amd import graph
    batch = s["batch"].cuda()
    if s["cell"] is None:
        return graph.distance(pos, batch, U.CUTOFF, 32) + (None,)
    return graph.distance_pbc(pos, batch, s["cell"].cuda(), U.CUTOFF, 32, n_mol=s["n_mol"], images=s["images"])


def _rebuilt_outputs(name, mode):
    """One ``RebuiltStep`` replayed on the three position sets -> (list of (energy, forces[, stress]) on the CPU, edge counts)."""
    from gotennet_amd.pipeline import RebuiltStep
    s = _system(name)
    step = RebuiltStep(_ef(), s["z"].cuda(), s["batch"].cuda(), s["n_mol"], cell=None if s["cell"] is None else s["cell"].cuda(),
                       images=s["images"])
    outs, counts = [], []
    for pos in s["positions"]:
        out = step(pos.cuda())
        torch.cuda.synchronize()
        outs.append([t.cpu().clone() for t in out])
        counts.append(int(step.edge_count.item()))
    assert step.state.tolist() == [0]
    assert step.edge_index.shape == (2, step.capacity) and (step.edge_shift is None) == (s["cell"] is None)
    return outs, counts, step.layout


@functools.lru_cache(maxsize=None)
def _cached_rebuilt(name, mode):
    return _rebuilt_outputs(name, mode)


@pytest.mark.parametrize("name", SYSTEMS)
def test_rebuilt_step_is_the_eager_step_on_the_padded_list(gemm_mode, name):
    s = _system(name)
    outs, counts, lay = _cached_rebuilt(name, gemm_mode)
    ef = _ef()
    z_pad, batch_pad = lay.pad_z(s["z"].cuda()), lay.batch
    cell_pad = None if s["cell"] is None else torch.cat([s["cell"].reshape(-1, 3, 3), torch.eye(3).unsqueeze(0)]).cuda()
    for k, pos in enumerate(s["positions"]):
        ei, ed, ev, sh = _host_list(s, pos.cuda())
        assert counts[k] == ei.shape[1]
        pei, pev, ped, _ = RU.padded_list(lay.N, lay.n_pad, lay.edge_capacity, ei, ev, ed, sh)
        want = ef(z_pad, pei, ped, pev, batch_pad, s["n_mol"] + 1, cell=cell_pad)
        torch.cuda.synchronize()
        want = [want[0][:s["n_mol"]], want[1][:lay.N]] + ([want[2][:s["n_mol"]]] if cell_pad is not None else [])
        assert len(want) == len(outs[k])
        for what, a, b in zip(("energy", "forces", "stress"), outs[k], want):
            assert torch.equal(a, b.cpu()), f"{name} {gemm_mode}, positions {k}: {what} differs by {float((a - b.cpu()).abs().max()):.3e}"
    if name == "molecules":
        assert counts[1] < counts[0] == counts[2]                      # the list did change between the replays
    for a, b in zip(outs[0], outs[2]):
        assert torch.equal(a, b)                                       # and the replay on the first positions is reproduced


@pytest.mark.parametrize("name", SYSTEMS)
def test_rebuilt_step_against_the_unpadded_step(gemm_mode, name):
    """f32 and split: bit for bit (their rows do not depend on what else is in the batch).  f16x2: 1e-4 relative; measured on
    MI355X: worst relative difference 0 on all three systems, i.e. bit identity there too."""
    s = _system(name)
    outs, _, lay = _cached_rebuilt(name, gemm_mode)
    ef = _ef()
    worst = 0.0
    for k, pos in enumerate(s["positions"]):
        ei, ed, ev, sh = _host_list(s, pos.cuda())
        want = ef(s["z"].cuda(), ei, ed, ev, s["batch"].cuda(), s["n_mol"], cell=None if s["cell"] is None else s["cell"].cuda())
        torch.cuda.synchronize()
        for what, a, b in zip(("energy", "forces", "stress"), outs[k], want):
            b = b.cpu()
            rel = float((a.double() - b.double()).abs().max() / b.double().abs().max())
            worst = max(worst, rel)
            print(f"padded vs unpadded, {name} {gemm_mode}, positions {k}: {what} relative difference {rel:.3e}, "
                  f"equal bits: {torch.equal(a, b)}")
    print(f"padded vs unpadded, {name} {gemm_mode}: worst relative difference {worst:.3e}")
    if gemm_mode == "f16x2":
        assert worst <= F16X2_BOUND
    else:
        assert worst == 0.0


# ------------------------------------------------------------------------------------------------ MD
def _md(s, captured, rebuild, **kw):
    from gotennet_amd.md import MDRun
    kw.setdefault("log_len", 256)
    return MDRun(_ef(), s["z"].cuda(), s["pos"].float().cuda(), s["batch"].cuda(), s["n_mol"], dt=DT, force_scale=FORCE_SCALE,
                 vel=s["vel"].float().cuda(), captured=captured, rebuild=rebuild, **kw)


def _md_snapshot(md):
    torch.cuda.synchronize()
    out = [md.pos.cpu(), md.vel.cpu(), md.potential_energy.cpu(), md.kinetic_energy.cpu()]
    return out + ([md.stress.cpu()] if md._cell is not None else [])


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: entry {k} differs, max |difference| {float((x.double() - y.double()).abs().max()):.3e}"


@functools.lru_cache(maxsize=None)
def _md_eager(mode, thermostat, rebuild):
    """The eager trajectory of the three molecules in the current arithmetic (``mode`` is the cache key), computed once ->
    (per-step snapshots, energy log, rebuilds, edge counts seen).  Read-only."""
    md = _md(MU.md_molecules(), False, rebuild, thermostat=THERMOSTAT if thermostat else None)
    traj, counts = [], []
    for _ in range(STEPS):
        md.run(1)
        traj.append(_md_snapshot(md))
        counts.append(md.edge_count)
    return traj, md.energy_log().cpu(), md.rebuilds, counts


@pytest.mark.parametrize("thermostat", [False, True], ids=["nve", "langevin"])
def test_md_device_captured_equals_device_eager(gemm_mode, thermostat):
    ref, ref_log, ref_rebuilds, counts = _md_eager(gemm_mode, thermostat, "device")
    th = THERMOSTAT if thermostat else None
    md = _md(MU.md_molecules(), True, "device", thermostat=th, check_every=1)
    for k in range(STEPS):
        md.run(1)
        _same(_md_snapshot(md), ref[k], f"{gemm_mode}, step {k + 1}")
        assert md.edge_count == counts[k]
    assert md.step == STEPS and md.rebuilds == 0 == ref_rebuilds           # nothing is re-recorded
    assert len(set(counts)) > 1, "the list never changed: the input does not test the rebuild"
    assert torch.equal(md.energy_log().cpu(), ref_log)
    md8 = _md(MU.md_molecules(), True, "device", thermostat=th, check_every=8).run(STEPS)
    _same(_md_snapshot(md8), ref[-1], f"{gemm_mode}, check_every=8")
    assert md8.step == STEPS and md8.rebuilds == 0 and torch.equal(md8.energy_log().cpu(), ref_log)


@pytest.mark.parametrize("mode", ["f32", "split"])
@pytest.mark.parametrize("thermostat", [False, True], ids=["nve", "langevin"])
def test_md_device_mode_is_the_host_mode_trajectory(mode, thermostat):
    from gotennet_amd import engine
    old = engine.GEMM_MODE
    engine.GEMM_MODE = mode
    try:
        dev, dev_log, _, _ = _md_eager(mode, thermostat, "device")
        host, host_log, host_rebuilds, host_counts = _md_eager(mode, thermostat, "host")
    finally:
        engine.GEMM_MODE = old
    assert host_rebuilds >= 1, "test input: the host-mode list never changed"
    for k in range(STEPS):
        _same(dev[k], host[k], f"{mode}, step {k + 1}")
    assert torch.equal(dev_log, host_log)


def _periodic(name, images):
    s = dict((PM if images == "all" else U).system(name))
    s["vel"] = 0.05 * torch.randn(s["pos"].shape, generator=torch.Generator().manual_seed(9))
    return s


@pytest.mark.parametrize("name,images", [("a", "minimum"), ("n1", "all")])
def test_periodic_md_device_captured_equals_device_eager(gemm_mode, name, images):
    s = _periodic(name, images)
    kw = dict(cell=s["cell"].float().cuda(), images=images)
    eager, md = _md(s, False, "device", **kw), _md(s, True, "device", **kw)
    host = _md(s, False, "host", **kw) if gemm_mode == "f32" else None
    for k in range(12):
        eager.run(1), md.run(1)
        a, b = _md_snapshot(md), _md_snapshot(eager)
        assert len(a) == 5                                             # stress included
        _same(a, b, f"{name} {gemm_mode}, step {k + 1}")
        assert md.edge_count == eager.edge_count
        if host is not None:
            host.run(1)
            _same(a, _md_snapshot(host), f"{name} f32 against host mode, step {k + 1}")
            assert md.edge_count == host.edge_count
    assert md.step == eager.step == 12 and md.rebuilds == eager.rebuilds == 0
    assert torch.equal(md.cell.cpu(), s["cell"].float().reshape(-1, 3, 3)) and md.cell.shape == (s["n_mol"], 3, 3)
    if host is not None:
        print(f"periodic {name} ({images}): host-mode rebuilds {host.rebuilds} of 12 steps")


def test_device_mode_replays_advance_one_step_each(gemm_mode):
    """The counterpart of ``test_a_stale_replay_advances_nothing``: across a list change every replay completes a step."""
    ref, _, _, counts = _md_eager(gemm_mode, False, "device")
    md = _md(MU.md_molecules(), True, "device")
    md.run(1)                                                          # (the first replay of the graph, synchronised)
    seen = [md.edge_count]
    for k in range(2, 14):
        md._step.graph.replay()
        assert md._state.tolist() == [0, k]                            # (a host read: a synchronisation per replay)
        seen.append(int(md._step.edge_count.item()))
    assert seen == counts[:13] and len(set(seen)) > 1
    _same(_md_snapshot(md), ref[12], "after 13 replays")


# ------------------------------------------------------------------------------------------------ Relax
def _relax(captured, rebuild, **kw):
    from gotennet_amd import Relax
    s = MU.md_molecules()
    kw.setdefault("log_len", 256)
    return Relax(_ef(), s["z"].cuda(), s["pos"].float().cuda(), s["batch"].cuda(), s["n_mol"], fmax=FU.REF_FMAX, captured=captured,
                 rebuild=rebuild, **kw)


def _relax_snapshot(rx):
    torch.cuda.synchronize()
    out = [rx.pos, rx.vel, rx.potential_energy, rx.forces, rx._dt, rx._alpha, rx._n_pos, rx.status, rx.converged_at, rx._coef]
    return [t.cpu().clone() for t in out]


def test_relax_device_captured_equals_device_eager(gemm_mode):
    eager, rx = _relax(False, "device"), _relax(True, "device")
    host = _relax(False, "host") if gemm_mode == "f32" else None
    _same(_relax_snapshot(rx), _relax_snapshot(eager), f"{gemm_mode}, start")
    for k in range(FU.REF_STEPS):
        eager.run(1), rx.run(1)
        a = _relax_snapshot(rx)
        _same(a, _relax_snapshot(eager), f"{gemm_mode}, step {k + 1}")
        assert rx.edge_count == eager.edge_count
        if host is not None:
            host.run(1)
            _same(a, _relax_snapshot(host), f"f32 against host mode, step {k + 1}")
    assert rx.step == eager.step == FU.REF_STEPS and rx.rebuilds == eager.rebuilds == 0
    assert torch.equal(rx.log().cpu(), eager.log().cpu())
    rx8 = _relax(True, "device", check_every=8).run(FU.REF_STEPS)
    _same(_relax_snapshot(rx8), a, f"{gemm_mode}, check_every=8")
    if host is not None:
        assert host.rebuilds >= 1, "test input: the host-mode list never changed"
        assert rx.converged_at.tolist() == host.converged_at.tolist() == FU.REF_CONVERGED_AT
        assert torch.equal(rx.pos.cpu(), host.pos.cpu())
