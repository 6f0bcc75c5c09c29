"""GPU: the nudged-elastic-band driver.  Two bands of 5 images (3 and 4 atoms per image) between two distorted copies of the
``md_util.md_molecules()`` geometries, ``pbc_util.make_model(32, 2, 2, seed=1)``, 16 steps with a climbing image.  The captured
mode is held to the eager mode bit for bit after every step, the device-rebuilt list to the host-rebuilt one, every step of
the device run to the fp64 rule of tests/neb_util.py applied to the device's own previous state, and the whole run to the
fp64 reference run (the oracle's forces on the brute-force list) whose decisions and tangent branches
tests/test_neb_host.py shows to be far from every threshold."""
import functools

import pytest
import torch

from tests import fire_util as FU
from tests import neb_util as NU
from tests import pbc_util as U

pytestmark = pytest.mark.gpu

STEPS, N_IMG, K, CLIMB, FMAX = NU.REF_STEPS, NU.REF_N_IMG, NU.REF_K, NU.REF_CLIMB, NU.REF_FMAX
_ulp = FU.ulp32
#: max |pos_hip - pos_ref| (Angstrom) and max |E_hip - E_ref| after 16 steps against the fp64 reference run: 4 x the worst value
#: measured over the two projection arithmetics.  Measured on MI355X (f32 / f16x2): positions 4.198e-07 in both (an ulp of a
#: coordinate of 2 to 5 Angstrom: the trajectories do not separate), energies 6.462e-07 / 2.828e-07.  The run is
#: bit-reproducible; the factor covers the spread between arithmetics, nothing else.
POS_BOUND, ENERGY_BOUND = 4 * 4.198e-07, 4 * 6.462e-07


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


def _driver(captured, **kw):
    from gotennet_amd import NEB
    from gotennet_amd.pipeline import EnergyForces
    net, head = _model()
    s = NU.band_start()
    kw.setdefault("log_len", 64)
    kw.setdefault("fmax", FMAX)
    return NEB(EnergyForces(net, head, check_edges=False), s["z"].cuda(), s["pos"].cuda(), s["batch"].cuda(), s["n_mol"],
               n_images=N_IMG, k=K, climb=CLIMB, captured=captured, **kw)


NAMES = ("pos", "vel", "energy", "forces", "dt", "alpha", "n_pos", "status", "converged_at", "coef", "g", "e_band", "climbing")


def _snapshot(nb):
    torch.cuda.synchronize()
    out = [nb.pos, nb.vel, nb.potential_energy, nb.forces, nb._dt, nb._alpha, nb._n_pos, nb.status, nb.converged_at, nb._coef,
           nb._g, nb._e_band, nb._climbing]
    return [t.cpu().clone() for t in out]


def _same(a, b, what, names=NAMES):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: {names[k]} differs, max |difference| {float((x.double() - y.double()).abs().max()):.3e}"


@functools.lru_cache(maxsize=None)
def _eager_reference(mode):
    """The eager run (host-rebuilt list) in the current arithmetic (``mode`` is the cache key), computed once: (the snapshot at
    the start and after every step, the log, rebuilds).  Read-only."""
    nb = _driver(False)
    traj = [_snapshot(nb)]
    for _ in range(STEPS):
        nb.run(1)
        traj.append(_snapshot(nb))
    return traj, nb.log().cpu(), nb.rebuilds


def test_captured_equals_eager_after_every_step(arithmetic):
    ref, ref_log, ref_rebuilds = _eager_reference(arithmetic)
    nb = _driver(True, check_every=1)
    _same(_snapshot(nb), ref[0], f"{arithmetic}, start")
    for k in range(STEPS):
        nb.run(1)
        _same(_snapshot(nb), ref[k + 1], f"{arithmetic}, step {k + 1}")
    print(f"{arithmetic}: rebuilds captured {nb.rebuilds}, eager {ref_rebuilds}; climbing {nb.climbing_image.tolist()}")
    assert nb.step == STEPS and nb.rebuilds == ref_rebuilds
    assert torch.equal(nb.log().cpu(), ref_log) and ref_log.shape == (STEPS, 2, 2)
    # the check interval is invisible: 16 steps in one call, the host looks every 8 replays
    nb8 = _driver(True, check_every=8).run(STEPS)
    _same(_snapshot(nb8), ref[-1], f"{arithmetic}, check_every=8")
    assert nb8.step == STEPS and torch.equal(nb8.log().cpu(), ref_log)
    # the log is the state BEFORE each step's move: the band's largest kept energy and the largest |g| of that step's g
    for k in range(STEPS):
        assert torch.equal(ref_log[k, :, 0], ref[k][2].reshape(2, N_IMG).max(1).values)
        assert torch.equal(ref_log[k, :, 0], ref[k + 1][11])
    # the queries speak of the kept state: they are what the next step computes and logs
    g, fm, ci, barrier = nb.neb_forces.cpu(), nb.fmax.cpu(), nb.climbing_image.cpu(), nb.barrier.cpu()
    e = nb.potential_energy.cpu().double().reshape(2, N_IMG)
    assert barrier.dtype == torch.float64 and torch.equal(barrier, e.max(1).values - e[:, 0])
    nb.run(1)
    torch.cuda.synchronize()
    assert torch.equal(nb._g.cpu(), g) and torch.equal(nb._climbing.cpu(), ci) and torch.equal(nb.log()[-1, :, 1].cpu(), fm)
    ends = torch.isin(NU.band_start()["batch"] % N_IMG, torch.tensor([0, N_IMG - 1]))
    assert bool((g[ends] == 0).all()) and not bool((g[~ends] == 0).any())


def test_device_rebuilt_list_equals_host_rebuilt_list():
    """``rebuild="device"`` against ``rebuild="host"`` at the end of the run, bit for bit, in the f32 arithmetic."""
    from gotennet_amd import engine
    old, engine.GEMM_MODE = engine.GEMM_MODE, "f32"
    try:
        ref, ref_log, _ = _eager_reference("f32")
        nb = _driver(True, rebuild="device", check_every=4).run(STEPS)
        _same(_snapshot(nb), ref[-1], "device list against host list")
        assert nb.step == STEPS and nb.rebuilds == 0 and torch.equal(nb.log().cpu(), ref_log)
    finally:
        engine.GEMM_MODE = old


def test_every_step_is_the_fp64_rule_on_the_device_state(arithmetic):
    """``neb_util.neb_forces`` and ``fire_util.fire_step`` in fp64 on the snapshot before a step (the device's own positions,
    velocities, kept forces and energies, per-band state) against the snapshot after it: g at ``neb_util.g_bound``, the plan and
    the move at the bounds of tests/test_hip_fire_kernels.py."""
    ref, log, _ = _eager_reference(arithmetic)
    s = NU.band_start()
    p = dict(FU.DEFAULTS, fmax=FMAX)
    mol_ptr = s["mol_ptr"]
    band_ptr, band_fixed = NU.band_ptr(mol_ptr, N_IMG), NU.band_fixed(mol_ptr, N_IMG)
    atom_band = s["batch"] // N_IMG
    worst = 0.0
    for k in range(STEPS):
        b, a = dict(zip(NAMES, ref[k])), dict(zip(NAMES, ref[k + 1]))
        # the band forces, from the fp32 energies as they are: the same branch by construction
        g64, e_band, ci, info = NU.neb_forces(b["pos"], b["forces"], b["energy"], mol_ptr, N_IMG, K, CLIMB, detail=True)
        assert torch.equal(a["e_band"], e_band) and a["climbing"].tolist() == ci.tolist(), k
        err, bound = (a["g"].double() - g64).abs(), NU.g_bound(g64, info, K)
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (k, float((err / bound).max()))
        assert bool((a["g"][band_fixed] == 0).all()), k
        # the plan, from the device's own g
        st = dict(dt=b["dt"].double(), alpha=b["alpha"].double(), n_pos=b["n_pos"].long(), status=b["status"].long(),
                  converged_at=b["converged_at"].long())
        _, _, st1, finfo = FU.fire_step(b["pos"], b["vel"], a["g"], band_ptr, st, p, fixed=band_fixed, step=k)
        for name in ("n_pos", "status", "converged_at"):
            assert a[name].tolist() == st1[name].tolist(), (k, name)
        active = finfo["coef"][:, 3] == 1.0
        assert a["coef"][:, 3].tolist() == finfo["coef"][:, 3].tolist(), k
        for name in ("dt", "alpha"):
            assert bool(((a[name].double() - st1[name]).abs() <= _ulp(st1[name])).all()), (k, name)
        assert bool(((a["coef"].double() - finfo["coef"]).abs() <= _ulp(finfo["coef"]))[active].all()), k
        assert bool(((log[k, :, 1].double() - finfo["fmax"]).abs() <= 3 * _ulp(finfo["fmax"])).all()), k
        # the move, from the device's own coefficients
        coef = a["coef"].double()
        pos1, vel1, _, _ = FU.fire_step(b["pos"], b["vel"], a["g"], band_ptr, st, p, fixed=band_fixed, step=k, coef=coef)
        c, f64, v64 = coef[atom_band], a["g"].double(), b["vel"].double()
        big_v = torch.maximum(torch.maximum((c[:, 0:1] * v64).abs(), (c[:, 1:2] * f64).abs()), (c[:, 2:3] * f64).abs())
        moved = active[atom_band] & ~band_fixed
        assert torch.equal(a["vel"][~moved], b["vel"][~moved]) and torch.equal(a["pos"][~moved], b["pos"][~moved]), k
        assert bool(((a["vel"].double() - vel1).abs() <= 4 * _ulp(big_v))[moved].all()), k
        big_p = torch.maximum(b["pos"].double().abs(), (pos1 - b["pos"].double()).abs())
        assert bool(((a["pos"].double() - pos1).abs() <= 8 * _ulp(big_p) + c[:, 2:3].abs() * 4 * _ulp(big_v))[moved].all()), k
        # finish: both bands are active throughout, so every kept value is replaced
        assert st1["status"].tolist() == [0, 0] and not torch.equal(a["forces"], b["forces"]) and not torch.equal(a["energy"], b["energy"])
    print(f"{arithmetic}: worst |g - fp64 rule| / bound over {STEPS} steps: {worst:.3f}")


def test_end_images_stay_put(arithmetic):
    ref, _, _ = _eager_reference(arithmetic)
    s = NU.band_start()
    ends = torch.isin(s["batch"] % N_IMG, torch.tensor([0, N_IMG - 1]))
    assert torch.equal(ref[-1][0][ends], s["pos"][ends]) and bool((ref[-1][1][ends] == 0).all())
    assert not bool((ref[-1][0][~ends] == s["pos"][~ends]).all(1).any())
    # ... and the model still evaluates them: their energies and forces are kept, and constant
    e = [snap[2].reshape(2, N_IMG) for snap in ref]
    assert all(torch.equal(x[:, [0, -1]], e[0][:, [0, -1]]) for x in e) and not torch.equal(e[-1], e[0])


def test_a_band_below_fmax_freezes_while_the_other_goes_on(arithmetic):
    """fmax between the two bands' largest |g| at the start (tests/test_neb_host.py checks the input): band 0 is converged at
    step 0 and never moves, band 1 goes on."""
    s = NU.band_start()
    nb = _driver(True, fmax=NU.FREEZE_FMAX, check_every=3)
    start = _snapshot(nb)
    first = nb.fmax.cpu().tolist()
    assert first[0] < NU.FREEZE_FMAX < first[1]
    nb.run(6)
    end = dict(zip(NAMES, _snapshot(nb)))
    assert end["status"].tolist() == [1, 0] and end["converged_at"].tolist() == [0, -1] and nb.step == 6
    assert nb.converged.tolist() == [True, False]
    cut, e_cut = s["mol_ptr"][N_IMG], N_IMG
    for i, name in ((0, "pos"), (1, "vel"), (3, "forces")):
        assert torch.equal(end[name][:cut], start[i][:cut]), name
        assert not torch.equal(end[name][cut:], start[i][cut:]), name
    assert torch.equal(end["energy"][:e_cut], start[2][:e_cut]) and not torch.equal(end["energy"][e_cut:], start[2][e_cut:])
    assert end["n_pos"].tolist()[0] == -1 and float(end["dt"][0]) == float(start[4][0])
    assert nb.log().shape == (6, 2, 2)


def _error_of(kind, fn):
    """The message of the ``kind`` that ``fn()`` raises.  The exception is dropped here: one kept in a test's frame ties that frame,
    the traceback and the driver into a reference cycle, and a recorded hipGraph that only the cyclic collector frees may be
    destroyed in the middle of a later stream capture, which the runtime refuses."""
    try:
        fn()
    except kind as e:
        return str(e)
    raise AssertionError(f"{kind.__name__} was not raised")


def test_an_energy_that_is_not_finite_stops_the_band():
    s = NU.band_start()
    nb = _driver(True)
    nb._e[N_IMG + 2] = float("nan")                   # band 1, image 2
    msg = _error_of(RuntimeError, lambda: nb.run(3))
    assert "band 1" in msg
    assert nb.status.tolist() == [0, 2] and nb.converged_at.tolist() == [-1, 0]
    cut = s["mol_ptr"][N_IMG]
    assert torch.equal(nb.pos.cpu()[cut:], s["pos"][cut:]) and bool((nb.vel.cpu()[cut:] == 0).all())
    assert not torch.equal(nb.pos.cpu()[:cut], s["pos"][:cut])


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_trajectory_against_the_fp64_reference(mode):
    """The device run next to the fp64 reference run: the same decisions and climbing images, and positions and energies
    within the bounds at the head of this file."""
    from gotennet_amd import engine
    r = NU.band_reference()
    old = engine.GEMM_MODE
    engine.GEMM_MODE = mode
    try:
        nb = _driver(True, check_every=8).run(STEPS)
        pos, e = nb.pos.cpu().double(), nb.potential_energy.cpu().double()
        n_pos, status, climbing = nb._n_pos.tolist(), nb.status.tolist(), nb.climbing_image.tolist()
    finally:
        engine.GEMM_MODE = old
    h = r["history"]
    d, de = float((pos - h[-1]["pos"]).abs().max()), float((e - h[-1]["energy"]).abs().max())
    print(f"trajectory {mode}: max |pos - ref| after {STEPS} steps {d:.3e}; max |E - ref| {de:.3e}; rebuilds {nb.rebuilds}")
    assert nb.step == r["steps"] == STEPS and status == r["state"]["status"].tolist() and n_pos == r["state"]["n_pos"].tolist()
    kept = NU.neb_forces(h[-1]["pos"], h[-1]["forces"], h[-1]["energy"], r["mol_ptr"], N_IMG, K, CLIMB)
    assert climbing == kept[2].tolist()
    assert d <= POS_BOUND and de <= ENERGY_BOUND
