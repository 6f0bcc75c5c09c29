"""GPU: the MD driver.  The captured mode (one hipGraph replay per step on a fixed list that is verified on the device) is held
to the eager mode (the same kernels, the list rebuilt by the search in every step): bit for bit, after every step."""
import functools

import pytest
import torch

from tests import md_util as MU
from tests import pbc_multi_util as PM
from tests import pbc_util as U

pytestmark = pytest.mark.gpu

DT, FORCE_SCALE, STEPS = 0.2, 0.05, 24
THERMOSTAT = dict(kT=0.02, gamma=0.5, key=(77, 5))


@pytest.fixture(params=["f32", "f16x2"])
def arithmetic(request):
    from gotennet_amd import engine
    old = engine.GEMM_MODE
    engine.GEMM_MODE = request.param
    yield request.param
    engine.GEMM_MODE = old


@functools.lru_cache(maxsize=None)
def _model():
    net, head, *_ = U.make_model(32, 2, 2, seed=1)
    return net.cuda().eval(), head.cuda().eval()


def _driver(s, captured, **kw):
    from gotennet_amd.md import MDRun
    from gotennet_amd.pipeline import EnergyForces
    net, head = _model()
    kw.setdefault("log_len", 256)
    return MDRun(EnergyForces(net, head, check_edges=False), s["z"].cuda(), s["pos"].float().cuda(), s["batch"].cuda(), s["n_mol"],
                 dt=DT, force_scale=FORCE_SCALE, vel=s["vel"].float().cuda(), captured=captured, **kw)


def _snapshot(md):
    torch.cuda.synchronize()
    out = [md.pos.cpu(), md.vel.cpu(), md.potential_energy.cpu(), md.kinetic_energy.cpu()]
    return out + ([md.stress.cpu()] if md._cell is not None else [])


def _trajectory(md, steps):
    traj = []
    for _ in range(steps):
        md.run(1)
        traj.append(_snapshot(md))
    return traj


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: entry {k} differs, max |difference| {float((x - y).abs().max()):.3e}"


@functools.lru_cache(maxsize=None)
def _eager_reference(mode, thermostat):
    """The eager trajectory of the three molecules in the current arithmetic (``mode`` is the cache key), computed once:
    (per-step snapshots, energy log, rebuilds).  Read-only."""
    md = _driver(MU.md_molecules(), False, thermostat=THERMOSTAT if thermostat else None)
    traj = _trajectory(md, STEPS)
    return traj, md.energy_log().cpu(), md.rebuilds


@pytest.mark.parametrize("thermostat", [False, True], ids=["nve", "langevin"])
def test_captured_equals_eager_after_every_step(arithmetic, thermostat):
    ref, ref_log, ref_rebuilds = _eager_reference(arithmetic, thermostat)
    th = THERMOSTAT if thermostat else None
    md = _driver(MU.md_molecules(), True, thermostat=th, check_every=1)
    for k in range(STEPS):
        md.run(1)
        _same(_snapshot(md), ref[k], f"{arithmetic}, step {k + 1}")
    print(f"{arithmetic} thermostat={thermostat}: rebuilds captured {md.rebuilds}, eager {ref_rebuilds}, of {STEPS} steps")
    assert md.step == STEPS and 1 <= md.rebuilds <= STEPS // 2, md.rebuilds       # it did replay, and it did rebuild
    assert md.rebuilds == ref_rebuilds
    assert torch.equal(md.energy_log().cpu(), ref_log)
    # the check interval is invisible: 24 steps in one call, the host looks every 8 replays
    md8 = _driver(MU.md_molecules(), True, thermostat=th, check_every=8).run(STEPS)
    _same(_snapshot(md8), ref[-1], f"{arithmetic}, check_every=8")
    assert md8.step == STEPS and md8.rebuilds == md.rebuilds
    log = md8.energy_log().cpu()
    assert torch.equal(log, ref_log)
    for k in range(STEPS):
        assert torch.equal(log[k, :, 0], ref[k][2]) and torch.equal(log[k, :, 1], ref[k][3])


def test_thermostat_changes_the_trajectory_and_the_key_fixes_it(arithmetic):
    nve, _, _ = _eager_reference(arithmetic, False)
    th, _, _ = _eager_reference(arithmetic, True)
    assert not torch.equal(nve[0][1], th[0][1])
    other = _driver(MU.md_molecules(), True, thermostat=dict(THERMOSTAT, key=(78, 5))).run(1)
    assert not torch.equal(_snapshot(other)[1], th[0][1])


def test_a_stale_replay_advances_nothing(arithmetic):
    ref, _, _ = _eager_reference(arithmetic, False)
    md = _driver(MU.md_molecules(), True)
    md.run(1)
    k = None
    for _ in range(STEPS // 2):
        md._step.graph.replay()
        stale, count = md._state.tolist()
        if stale:
            k = count
            break
    assert k is not None, "no pair crossed the cutoff in the first dozen steps"
    frozen = [md._pos.clone(), md._vel.clone(), md._e.clone(), md._ke.clone(), md._log.clone()]
    for _ in range(3):
        md._step.graph.replay()
    assert md._state.tolist() == [1, k]
    _same([md._pos, md._vel, md._e, md._ke, md._log], frozen, "after further stale replays")
    # until the host intervenes: the driver repairs the list, finishes step k + 1 and is on the eager trajectory
    rebuilds = md.rebuilds
    md.run(1)
    assert md.step == k + 1 and md.rebuilds == rebuilds + 1 and md._state.tolist() == [0, k + 1]
    _same(_snapshot(md), ref[k], f"step {k + 1} after the repair")


def _periodic(name, images):
    s = dict((PM if images == "all" else U).system(name))
    g = torch.Generator().manual_seed(9)
    s["vel"] = 0.05 * torch.randn(s["pos"].shape, generator=g)
    return s


@pytest.mark.parametrize("name,images", [("a", "minimum"), ("n1", "all")])
def test_periodic_captured_equals_eager(arithmetic, name, images):
    s = _periodic(name, images)
    kw = dict(cell=s["cell"].float().cuda(), images=images)
    eager, md = _driver(s, False, **kw), _driver(s, True, **kw)
    for k in range(12):
        eager.run(1), md.run(1)
        a, b = _snapshot(md), _snapshot(eager)
        assert len(a) == 5                                     # stress included
        _same(a, b, f"{name} {arithmetic}, step {k + 1}")
    print(f"periodic {name} ({images}) {arithmetic}: rebuilds captured {md.rebuilds}, eager {eager.rebuilds}, of 12 steps")
    assert md.rebuilds == eager.rebuilds and md.step == eager.step == 12


def test_the_cell_check_is_distance_pbc_s():
    from gotennet_amd import graph
    s = _periodic("n1", "all")                                   # a cell narrower than 2 * cutoff
    d = dict(pos=s["pos"].float().cuda(), batch=s["batch"].cuda(), cell=s["cell"].float().cuda())
    with pytest.raises(ValueError) as want:
        graph.distance_pbc(d["pos"], d["batch"], d["cell"], U.CUTOFF, 32)
    with pytest.raises(ValueError) as got:
        _driver(s, True, cell=d["cell"])
    assert str(got.value) == str(want.value)
    tiny = d["cell"] * 0.2
    with pytest.raises(ValueError, match="cutoff / 3"):
        _driver(s, True, cell=tiny, images="all")


def test_nve_energy_excursion_is_the_eager_one():
    """200 NVE steps of one molecule: captured and eager agree bit for bit, so their total-energy excursions are equal.  The
    excursion itself is printed, not bounded."""
    s = MU.md_molecules()
    keep = s["batch"] == 2
    one = dict(pos=s["pos"][keep], vel=torch.zeros_like(s["pos"][keep]), z=s["z"][keep], batch=torch.zeros(int(keep.sum()), dtype=torch.int64),
               n_mol=1)
    eager, md = _driver(one, False).run(200), _driver(one, True, check_every=8).run(200)
    a, b = md.energy_log().cpu(), eager.energy_log().cpu()
    assert a.shape == (200, 1, 2) and torch.equal(a, b)
    _same(_snapshot(md), _snapshot(eager), "after 200 steps")
    total = a.double().sum(2).flatten()
    print(f"NVE 200 steps: total energy {float(total[0]):.6f} -> {float(total[-1]):.6f}, excursion max - min = "
          f"{float(total.max() - total.min()):.3e} (first 100 steps {float(total[:100].max() - total[:100].min()):.3e}), "
          f"rebuilds captured {md.rebuilds}, eager {eager.rebuilds}")
