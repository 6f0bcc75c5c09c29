"""GPU: the relaxation driver.  The captured mode (one hipGraph replay per step on a fixed list that is verified on the device)
is held to the eager mode (the same kernels, the list rebuilt by the search in every step) bit for bit after every step; every
step of the device run is held to the fp64 emulation of tests/fire_util.py applied to the device's own state; and the whole
run is held to the fp64 reference run (the oracle's forces on the brute-force list) whose decisions
tests/test_fire_host.py shows to be far from every threshold."""
import functools

import pytest
import torch

from tests import fire_util as FU
from tests import md_util as MU
from tests import pbc_multi_util as PM
from tests import pbc_util as U

pytestmark = pytest.mark.gpu

FMAX, STEPS = FU.REF_FMAX, FU.REF_STEPS
REF_CONVERGED_AT, REF_EDGE_COUNTS, _ulp = FU.REF_CONVERGED_AT, FU.REF_EDGE_COUNTS, FU.ulp32
REF_REBUILDS = len(REF_EDGE_COUNTS) - 1
#: max |pos_hip - pos_ref| (Angstrom) after 8 and after 24 steps and max |E_hip - E_ref| over both, against the fp64 reference
#: run: 4 x the worst value measured over the three projection arithmetics.  Measured on MI355X (f32 / f16x2 / split): positions
#: 2.952e-07 after 8 steps and 5.110e-07 after 24 in all three (an ulp of a coordinate of 2 to 5 Angstrom: the trajectories do
#: not separate), energies 9.615e-07 / 9.615e-07 / 7.157e-07.  The run is bit-reproducible; the factor covers the spread between
#: arithmetics, nothing else.
POS_BOUND_8, POS_BOUND_24, ENERGY_BOUND = 4 * 2.952e-07, 4 * 5.110e-07, 4 * 9.615e-07


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
    from gotennet_amd import Relax
    from gotennet_amd.pipeline import EnergyForces
    net, head = _model()
    kw.setdefault("log_len", 256)
    kw.setdefault("fmax", FMAX)
    return Relax(EnergyForces(net, head, check_edges=False), s["z"].cuda(), s["pos"].float().cuda(), s["batch"].cuda(), s["n_mol"],
                 captured=captured, **kw)


NAMES = ("pos", "vel", "energy", "forces", "dt", "alpha", "n_pos", "status", "converged_at", "coef", "stress")


def _snapshot(rx):
    torch.cuda.synchronize()
    out = [rx.pos, rx.vel, rx.potential_energy, rx.forces, rx._dt, rx._alpha, rx._n_pos, rx.status, rx.converged_at, rx._coef]
    return [t.cpu().clone() for t in out + ([rx.stress] if rx._cell is not None else [])]


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: {NAMES[k]} differs, max |difference| {float((x.double() - y.double()).abs().max()):.3e}"


@functools.lru_cache(maxsize=None)
def _eager_reference(mode):
    """The eager run of the three molecules in the current arithmetic (``mode`` is the cache key), computed once: (the snapshot
    at the start and after every step, the log, rebuilds).  Read-only."""
    rx = _driver(MU.md_molecules(), False)
    traj = [_snapshot(rx)]
    for _ in range(STEPS):
        rx.run(1)
        traj.append(_snapshot(rx))
    return traj, rx.log().cpu(), rx.rebuilds


def test_captured_equals_eager_after_every_step(arithmetic):
    ref, ref_log, ref_rebuilds = _eager_reference(arithmetic)
    rx = _driver(MU.md_molecules(), True, check_every=1)
    _same(_snapshot(rx), ref[0], f"{arithmetic}, start")
    for k in range(STEPS):
        rx.run(1)
        _same(_snapshot(rx), ref[k + 1], f"{arithmetic}, step {k + 1}")
    print(f"{arithmetic}: rebuilds captured {rx.rebuilds}, eager {ref_rebuilds}; converged_at {rx.converged_at.tolist()}")
    assert rx.step == STEPS and rx.rebuilds == ref_rebuilds == REF_REBUILDS
    assert rx.converged_at.tolist() == REF_CONVERGED_AT and rx.converged.tolist() == [c >= 0 for c in REF_CONVERGED_AT]
    assert torch.equal(rx.log().cpu(), ref_log) and ref_log.shape == (STEPS, 3, 2)
    # the check interval is invisible: 24 steps in one call, the host looks every 8 replays
    rx8 = _driver(MU.md_molecules(), True, check_every=8).run(STEPS)
    _same(_snapshot(rx8), ref[-1], f"{arithmetic}, check_every=8")
    assert rx8.step == STEPS and rx8.rebuilds == rx.rebuilds and torch.equal(rx8.log().cpu(), ref_log)
    # the log is the state BEFORE each step's move: the kept energy, and the largest force of the kept forces
    for k in range(STEPS):
        assert torch.equal(ref_log[k, :, 0], ref[k][2])
    assert torch.equal(rx.fmax.cpu(), _driver_fmax(ref[-1][3]))


def _driver_fmax(forces):
    """gn_fire_fmax on its own, for the kept forces of a snapshot."""
    from gotennet_amd._lib import call, ptr
    s = MU.md_molecules()
    mol_ptr = torch.tensor([0, 3, 7, 12], dtype=torch.int32).cuda()
    f, out = forces.cuda(), torch.empty(3, dtype=torch.float32).cuda()
    call("gn_fire_fmax", ptr(f), None, ptr(mol_ptr), s["pos"].shape[0], 3, ptr(out), torch.cuda.current_stream().cuda_stream)
    return out.cpu()


def test_every_step_is_the_fp64_rule_on_the_device_state(arithmetic):
    """fire_step in fp64 on the snapshot before a step (the device's own positions, velocities, kept forces and per-molecule
    state) against the snapshot after it, at the bounds of tests/test_hip_fire_kernels.py."""
    ref, log, _ = _eager_reference(arithmetic)
    p = dict(FU.DEFAULTS, fmax=FMAX)
    mol_ptr = [0, 3, 7, 12]
    atom_mol = torch.repeat_interleave(torch.arange(3), torch.tensor([3, 4, 5]))
    for k in range(STEPS):
        b, a = dict(zip(NAMES, ref[k])), dict(zip(NAMES, ref[k + 1]))
        st = dict(dt=b["dt"].double(), alpha=b["alpha"].double(), n_pos=b["n_pos"].long(), status=b["status"].long(),
                  converged_at=b["converged_at"].long())
        _, _, st1, info = FU.fire_step(b["pos"], b["vel"], b["forces"], mol_ptr, st, p, step=k)
        for name in ("n_pos", "status", "converged_at"):
            assert a[name].tolist() == st1[name].tolist(), (k, name)
        active = info["coef"][:, 3] == 1.0
        assert a["coef"][:, 3].tolist() == info["coef"][:, 3].tolist(), k
        for name in ("dt", "alpha"):
            assert bool(((a[name].double() - st1[name]).abs() <= _ulp(st1[name])).all()), (k, name)
        assert bool(((a["coef"].double() - info["coef"]).abs() <= _ulp(info["coef"]))[active].all()), k
        assert bool(((log[k, :, 1].double() - info["fmax"]).abs() <= 3 * _ulp(info["fmax"])).all()), k
        # the move, from the device's own coefficients
        coef = a["coef"].double()
        pos1, vel1, _, _ = FU.fire_step(b["pos"], b["vel"], b["forces"], mol_ptr, st, p, step=k, coef=coef)
        c, f64, v64 = coef[atom_mol], b["forces"].double(), b["vel"].double()
        big_v = torch.maximum(torch.maximum((c[:, 0:1] * v64).abs(), (c[:, 1:2] * f64).abs()), (c[:, 2:3] * f64).abs())
        moved = active[atom_mol]
        assert torch.equal(a["vel"][~moved], b["vel"][~moved]) and torch.equal(a["pos"][~moved], b["pos"][~moved]), k
        assert bool(((a["vel"].double() - vel1).abs() <= 4 * _ulp(big_v))[moved].all()), k
        big_p = torch.maximum(b["pos"].double().abs(), (pos1 - b["pos"].double()).abs())
        assert bool(((a["pos"].double() - pos1).abs() <= 8 * _ulp(big_p) + c[:, 2:3].abs() * 4 * _ulp(big_v))[moved].all()), k
        # finish: the kept values of a molecule that is not active are not refreshed
        done = (st1["status"] != 0)
        assert torch.equal(a["forces"][done[atom_mol]], b["forces"][done[atom_mol]]) and torch.equal(a["energy"][done], b["energy"][done]), k
        assert not torch.equal(a["forces"][~done[atom_mol]], b["forces"][~done[atom_mol]]), k


def test_a_converged_molecule_freezes_and_the_energy_falls(arithmetic):
    ref, _, _ = _eager_reference(arithmetic)
    for m, atoms in enumerate((slice(0, 3), slice(3, 7), slice(7, 12))):
        k = REF_CONVERGED_AT[m]
        if k < 0:
            assert not torch.equal(ref[-1][0][atoms], ref[-2][0][atoms])          # still moving
            continue
        assert 0 < k < STEPS - 1                                                  # it moved before and the others go on after
        for later in ref[k + 1:]:
            for i in (0, 1, 3):                                                   # pos, vel, kept forces
                assert torch.equal(later[i][atoms], ref[k][i][atoms]), (m, NAMES[i])
            assert torch.equal(later[2][m], ref[k][2][m])
        assert not torch.equal(ref[k][0][atoms], ref[k - 1][0][atoms])
    e0, e1 = ref[0][2], ref[1][2]
    print(f"{arithmetic}: energy at the start {e0.tolist()}, after step 1 {e1.tolist()}")
    assert bool((e1 < e0).all())


def test_a_stale_replay_advances_nothing(arithmetic):
    ref, _, _ = _eager_reference(arithmetic)
    rx = _driver(MU.md_molecules(), True)
    rx.run(1)
    k = None
    for _ in range(STEPS // 2):
        rx._step.graph.replay()
        stale, count = rx._state.tolist()
        if stale:
            k = count
            break
    assert k is not None, "no pair crossed the cutoff in the first dozen steps"
    buffers = lambda: [rx._pos, rx._vel, rx._e, rx._f, rx._dt, rx._alpha, rx._n_pos, rx._status, rx._converged_at, rx._coef, rx._log]
    frozen = [t.clone() for t in buffers()]
    for _ in range(3):
        rx._step.graph.replay()
    assert rx._state.tolist() == [1, k]
    for x, y in zip(buffers(), frozen):
        assert torch.equal(x, y)
    # until the host intervenes: the driver repairs the list, finishes step k + 1 and is on the eager trajectory
    rebuilds = rx.rebuilds
    rx.run(1)
    assert rx.step == k + 1 and rx.rebuilds == rebuilds + 1 and rx._state.tolist() == [0, k + 1]
    _same(_snapshot(rx), ref[k + 1], f"step {k + 1} after the repair")


def _periodic(name, images):
    return dict((PM if images == "all" else U).system(name))


@pytest.mark.parametrize("name,images", [("a", "minimum"), ("n1", "all")])
def test_periodic_captured_equals_eager(arithmetic, name, images):
    s = _periodic(name, images)
    kw = dict(cell=s["cell"].float().cuda(), images=images)
    eager, rx = _driver(s, False, **kw), _driver(s, True, **kw)
    start = _snapshot(rx)
    for k in range(12):
        eager.run(1), rx.run(1)
        a, b = _snapshot(rx), _snapshot(eager)
        assert len(a) == len(NAMES)                            # stress included
        _same(a, b, f"{name} {arithmetic}, step {k + 1}")
    print(f"periodic {name} ({images}) {arithmetic}: rebuilds captured {rx.rebuilds}, eager {eager.rebuilds}, of 12 steps; "
          f"status {rx.status.tolist()}")
    assert rx.rebuilds == eager.rebuilds and rx.step == eager.step
    assert torch.equal(rx.log().cpu(), eager.log().cpu())
    assert not torch.equal(a[0], start[0]) and not torch.equal(a[-1], start[-1])      # it moved, and the stress followed
    assert torch.equal(rx._cell.cpu(), s["cell"].float().reshape(-1, 3, 3))             # the cell is fixed


def test_fixed_atoms_stay_put():
    s = MU.md_molecules()
    fixed = torch.zeros(12, dtype=torch.bool)
    fixed[[1, 3, 6, 9]] = True
    rx = _driver(s, True, fixed=fixed.cuda())
    free = _driver(s, True)
    rx.run(6), free.run(6)
    pos = rx.pos.cpu()
    assert torch.equal(pos[fixed], s["pos"][fixed]) and bool((rx.vel.cpu()[fixed] == 0).all())
    assert not bool((pos[~fixed] == s["pos"][~fixed]).all(1).any())
    assert not torch.equal(pos[~fixed], free.pos.cpu()[~fixed])
    # every atom fixed: no force counts, converged at step 0, nothing moves
    done = _driver(s, True, fixed=torch.ones(12, dtype=torch.uint8).cuda(), check_every=4).run(10)
    assert done.step == 0 and done.converged.tolist() == [True] * 3 and done.converged_at.tolist() == [0, 0, 0]
    assert torch.equal(done.pos.cpu(), s["pos"]) and bool((done.fmax.cpu() == 0).all())
    assert done.run(5).step == 0 and done.log().shape[0] == 0


def _error_of(kind, fn):
    """The message of the ``kind`` that ``fn()`` raises.  The exception is dropped here: one kept in a test's frame ties that frame,
    the traceback and the driver into a reference cycle, and a recorded hipGraph that only the cyclic collector frees may be
    destroyed in the middle of a later stream capture, which the runtime refuses."""
    try:
        fn()
    except kind as e:
        return str(e)
    raise AssertionError(f"{kind.__name__} was not raised")


@pytest.mark.parametrize("captured", [True, False], ids=["captured", "eager"])
def test_a_force_that_is_not_finite_stops_the_run(captured):
    s = MU.md_molecules()
    rx = _driver(s, captured)
    rx._f[4, 1] = float("nan")                      # molecule 1
    msg = _error_of(RuntimeError, lambda: rx.run(3))
    assert "molecule 1" in msg
    assert rx.status.tolist() == [0, 2, 0] and rx.converged_at.tolist() == [-1, 0, -1]
    atoms = slice(3, 7)
    assert torch.equal(rx.pos.cpu()[atoms], s["pos"][atoms]) and bool((rx.vel.cpu()[atoms] == 0).all())
    # in every molecule: nothing moves at all
    rx = _driver(s, captured)
    rx._f[[0, 4, 8], 2] = float("nan")
    msg = _error_of(RuntimeError, lambda: rx.run(3))
    assert "molecule 0" in msg and rx.status.tolist() == [2, 2, 2]
    assert torch.equal(rx.pos.cpu(), s["pos"]) and bool((rx.vel.cpu() == 0).all())


@pytest.mark.parametrize("mode", ["f32", "f16x2", "split"])
def test_trajectory_against_the_fp64_reference(mode):
    """The device run next to the fp64 reference run: the same decisions, and positions and energies within the bounds at the
    head of this file."""
    from gotennet_amd import engine
    r = FU.molecule_reference()
    old = engine.GEMM_MODE
    engine.GEMM_MODE = mode
    try:
        rx = _driver(MU.md_molecules(), True, check_every=8)
        rx.run(8)
        pos8, e8 = rx.pos.cpu().double(), rx.potential_energy.cpu().double()
        rx.run(STEPS - 8)
        pos24, e24 = rx.pos.cpu().double(), rx.potential_energy.cpu().double()
    finally:
        engine.GEMM_MODE = old
    h = r["history"]
    d8, d24 = float((pos8 - h[7]["pos"]).abs().max()), float((pos24 - h[-1]["pos"]).abs().max())
    de = max(float((e8 - h[7]["energy"]).abs().max()), float((e24 - h[-1]["energy"]).abs().max()))
    print(f"trajectory {mode}: max |pos - ref| after 8 steps {d8:.3e}, after 24 steps {d24:.3e}; max |E - ref| {de:.3e}; "
          f"rebuilds {rx.rebuilds}, converged_at {rx.converged_at.tolist()}")
    assert rx.converged_at.tolist() == REF_CONVERGED_AT and rx.rebuilds == REF_REBUILDS and rx.step == r["steps"] == STEPS
    assert d8 <= POS_BOUND_8 and d24 <= POS_BOUND_24 and de <= ENERGY_BOUND
