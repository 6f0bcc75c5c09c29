"""GPU: the MD driver with a barostat.  Captured against eager bit for bit, every step against the fp64 formula of
tests/npt_util.py, the direction of the volume move, the cell guard and ``max_step`` in both modes."""
import functools
import math
import re

import numpy as np
import pytest
import torch

from tests import npt_util as NU
from tests import pbc_util as U
from tests import test_hip_md_run as R          # its model, driver factory, snapshot helpers and eager references

pytestmark = pytest.mark.gpu

DT, THERMOSTAT = R.DT, R.THERMOSTAT
TAU = 20 * DT


@pytest.fixture(params=["f32", "f16x2"])
def arithmetic(request):
    from gotennet_amd import engine
    old = engine.GEMM_MODE
    engine.GEMM_MODE = request.param
    yield request.param
    engine.GEMM_MODE = old


def _system(name, images, scale=1.0, still=False):
    s = R._periodic(name, images)
    if still:                                       # start at rest: no kinetic pressure
        s["vel"] = torch.zeros_like(s["vel"])
    if scale != 1.0:
        s["pos"], s["cell"] = (s["pos"] * scale).float().double(), (s["cell"] * scale).float().double()
    return s


def _driver(s, captured, images, cell=None, **kw):
    return R._driver(s, captured, cell=s["cell"].float().cuda() if cell is None else cell, images=images, **kw)


def _error_of(kind, fn):
    """The message of the ``kind`` that ``fn()`` raises.  The exception is dropped here: one kept in a test's frame (``as err``)
    ties that frame, the traceback and the driver into a reference cycle, and a recorded hipGraph that only the cyclic
    collector frees may be destroyed in the middle of a later stream capture, which the runtime refuses."""
    try:
        fn()
    except kind as e:
        return str(e)
    raise AssertionError(f"{kind.__name__} was not raised")


def _formula_pressure(md):
    """2 K / (3 V) - tr(stress) / 3 in fp64 from the driver's own kinetic energy, stress and volume."""
    return NU.pressure(md.kinetic_energy.cpu().numpy(), md.stress.cpu().numpy(), md.volume.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _start(name, images, mode, scale=1.0, still=False):
    """Start pressure (fp64 formula), volume, stress trace / 3 and perpendicular widths per box of a system in the current
    arithmetic (``mode`` is the cache key), from an eager run without a barostat.  Read-only."""
    md = _driver(_system(name, images, scale, still), False, images)
    torch.cuda.synchronize()
    st = md.stress.cpu().numpy().astype(np.float64)
    assert bool((NU.ulps32(md.pressure.cpu().numpy(), _formula_pressure(md)) <= 2.0).all())      # without a barostat: on demand
    return dict(p=_formula_pressure(md), vol=md.volume.cpu().numpy().astype(np.float64),
                tr3=(st[:, 0, 0] + st[:, 1, 1] + st[:, 2, 2]) / 3.0, widths=NU.widths(md.cell.cpu().numpy())[0])


def _snapshot(md):
    torch.cuda.synchronize()
    return [md.pos.cpu(), md.vel.cpu(), md.cell.cpu(), md.potential_energy.cpu(), md.kinetic_energy.cpu(), md.stress.cpu(),
            md.pressure.cpu(), md.volume.cpu()]


def _coupling(start, kT):
    """beta_T such that the deterministic move towards P0 = 0 starts at |d_eps| <= 1e-3 per step and the noise has a standard
    deviation of at most 2e-3 (far inside max_step = 0.05 even at Box-Muller's largest |xi| = 5.8)."""
    r = 1e-3 / float(np.abs(start["p"]).max())                 # r = beta dt / tau
    if kT > 0:
        r = min(r, (2e-3) ** 2 * float(start["vol"].min()) / (2 * kT))
    return r * TAU / DT


@pytest.mark.parametrize("noise", [True, False], ids=["langevin_kT", "deterministic"])
@pytest.mark.parametrize("name,images", [("a", "minimum"), ("n1", "all")])
def test_captured_equals_eager_after_every_step(arithmetic, name, images, noise):
    start = _start(name, images, arithmetic)
    th = THERMOSTAT if noise else None
    baro = dict(pressure=0.0, tau=TAU, compressibility=_coupling(start, THERMOSTAT["kT"] if noise else 0.0))
    if not noise:
        baro["kT"] = 0.0
    s = _system(name, images)
    mine = s["cell"].float().cuda()                             # the caller's tensor: read, never moved
    eager = _driver(s, False, images, cell=mine, thermostat=th, barostat=baro)
    md = _driver(s, True, images, cell=mine, thermostat=th, barostat=baro, check_every=1)
    R._same(_snapshot(md), _snapshot(eager), "at the start")
    assert bool((NU.ulps32(md.pressure.cpu().numpy(), start["p"]) <= 2.0).all())       # the constructor's kept pressure
    traj = []
    for k in range(12):
        eager.run(1), md.run(1)
        traj.append(_snapshot(eager))
        R._same(_snapshot(md), traj[-1], f"{name} {arithmetic}, step {k + 1}")
    assert md.step == eager.step == 12 and torch.equal(mine.cpu(), s["cell"].float())
    assert not torch.equal(traj[-1][2], s["cell"].float()) and not torch.equal(traj[0][2], traj[1][2])       # the cell does move
    print(f"npt {name} ({images}) {arithmetic} noise={noise}: V {start['vol']} -> {traj[-1][7].tolist()}, P {start['p']} -> "
          f"{traj[-1][6].tolist()}, rebuilds captured {md.rebuilds}, eager {eager.rebuilds}")
    log, ref_log = md.npt_log().cpu(), eager.npt_log().cpu()
    assert log.shape == (12, s["n_mol"], 2) and torch.equal(log, ref_log)
    assert torch.equal(md.energy_log().cpu(), eager.energy_log().cpu())
    for k in range(12):
        assert torch.equal(log[k, :, 0], traj[k][7]) and torch.equal(log[k, :, 1], traj[k][6])
    # the check interval is invisible
    md8 = _driver(s, True, images, thermostat=th, barostat=baro, check_every=8).run(12)
    R._same(_snapshot(md8), traj[-1], f"{name} {arithmetic}, check_every=8")
    assert md8.step == 12 and torch.equal(md8.npt_log().cpu(), ref_log)


@pytest.mark.parametrize("noise", [True, False], ids=["langevin_kT", "deterministic"])
def test_each_step_is_the_formula(arithmetic, noise):
    from gotennet_amd._lib import call, ptr
    start = _start("a", "minimum", arithmetic)
    th = THERMOSTAT if noise else None
    kT = THERMOSTAT["kT"] if noise else 0.0
    beta = _coupling(start, kT)
    baro = dict(pressure=0.0, tau=TAU, compressibility=beta, kT=kT, key=(5, 11) if noise else None)
    md = _driver(_system("a", "minimum"), True, "minimum", thermostat=th, barostat=baro)
    n_mol = 2
    key = torch.tensor([5, 11], dtype=torch.int64, device="cuda")
    for k in range(6):
        cell_b, vol_b, p_b = (t.cpu().numpy().astype(np.float64) for t in (md.cell, md.volume, md.pressure))
        xi = None
        if noise:
            out = torch.empty((n_mol, 3), dtype=torch.float32, device="cuda")
            call("gn_md_noise", ptr(key), md.step, 2, n_mol, ptr(out), torch.cuda.current_stream().cuda_stream)
            xi = out[:, 0].cpu().numpy().astype(np.float64)
        s_ref = NU.scale(NU.delta_eps(p_b, vol_b, 0.0, beta, TAU, DT, kT, xi))
        md.run(1)
        torch.cuda.synchronize()
        cell_a = md.cell.cpu().numpy().astype(np.float64)
        for m in range(n_mol):
            nz = cell_b[m] != 0
            u = NU.ulps32(cell_a[m][nz] / cell_b[m][nz], np.full(int(nz.sum()), s_ref[m]))
            assert bool((u <= 2.0).all()), (k, m, u)
            assert np.array_equal(cell_a[m][~nz], cell_b[m][~nz])
        up = NU.ulps32(md.pressure.cpu().numpy(), _formula_pressure(md))
        print(f"step {k + 1}: s - 1 = {s_ref - 1}, pressure {md.pressure.tolist()}, ulps {up}")
        assert bool((up <= 2.0).all()), (k, up)
        assert bool((s_ref != 1.0).all())


@pytest.mark.parametrize("direction", ["compress", "expand"])
def test_sign_and_direction(arithmetic, direction):
    """kT = 0.  A target above the internal pressure must shrink every box in every step, one below must grow it.  The atoms
    start at rest, so the start pressure is the stress term alone (the kinetic term the forces build up in six steps stays far
    below it) and the margin is half the smallest |P_int(0)|: a pressure formed with the opposite stress sign moves some box
    the other way in one of the two directions (asserted on the input)."""
    start = _start("a", "minimum", arithmetic, 1.0, True)
    p, tr3 = start["p"], start["tr3"]
    assert np.array_equal(p, -tr3)
    margin = 0.5 * float(np.abs(p).min())
    assert margin > 0
    p0 = float(p.max()) + margin if direction == "compress" else float(p.min()) - margin
    beta = 1e-3 * TAU / (DT * margin)                           # |d_eps| = 1e-3 per step for the box at the margin
    de = NU.delta_eps(p, start["vol"], p0, beta, TAU, DT, 0.0)
    assert bool((np.abs(de) >= 1e-3 * (1 - 1e-9)).all()) and bool((np.abs(de) < 0.05).all()), de
    wrong = NU.delta_eps(p + 2.0 * tr3, start["vol"], float(p.max()) + margin, beta, TAU, DT, 0.0), \
        NU.delta_eps(p + 2.0 * tr3, start["vol"], float(p.min()) - margin, beta, TAU, DT, 0.0)
    assert bool((wrong[0] > 0).any()) or bool((wrong[1] < 0).any()), "the input cannot tell the stress sign"
    md = _driver(_system("a", "minimum", still=True), True, "minimum",
                 barostat=dict(pressure=p0, tau=TAU, compressibility=beta, kT=0.0))
    vol = [md.volume.cpu().numpy().astype(np.float64)]
    for _ in range(6):
        md.run(1)
        vol.append(md.volume.cpu().numpy().astype(np.float64))
    print(f"{direction}: P(0) {p}, P0 {p0:.4e}, d_eps(0) {de}, P after {md.pressure.tolist()}, volumes {[v.tolist() for v in vol]}")
    for a, b in zip(vol, vol[1:]):
        assert bool((b < a).all()) if direction == "compress" else bool((b > a).all())


GUARD_SCALE_MARGIN = 1.002


def _guard_case(arithmetic):
    """System ``a`` scaled so that its smallest perpendicular width is 2 * cutoff * 1.002, and a barostat whose deterministic
    move is d_eps = -3e-3 per step for every box to within a tenth: the width shrinks by 1e-3 per step and crosses
    2 * cutoff in the second or third step."""
    w0 = _start("a", "minimum", arithmetic)["widths"]
    scale = 2 * U.CUTOFF * GUARD_SCALE_MARGIN / float(w0.min())
    start = _start("a", "minimum", arithmetic, scale)
    assert abs(float(start["widths"].min()) / (2 * U.CUTOFF) - GUARD_SCALE_MARGIN) < 1e-5
    gap = 10.0 * float(np.abs(start["p"]).max())               # P0 - P: ten times any start pressure, so it hardly varies
    p0 = float(start["p"].max()) + gap
    beta = 3e-3 * TAU / (DT * gap)
    de = NU.delta_eps(start["p"], start["vol"], p0, beta, TAU, DT, 0.0)
    assert bool((de <= -3e-3 * (1 - 1e-9)).all()) and bool((de > -3.7e-3).all()), de
    w = float(start["widths"].min())
    assert w * math.exp(float(de.max()) / 3) > 2 * U.CUTOFF > w * math.exp(3 * float(de.max()) / 3)     # after one step / after three
    return _system("a", "minimum", scale), dict(pressure=p0, tau=TAU, compressibility=beta, kT=0.0)


def test_guard_minimum_image_raises_in_both_modes(arithmetic):
    from gotennet_amd import graph
    s, baro = _guard_case(arithmetic)
    done = []
    for captured, check_every in ((False, 1), (True, 1), (True, 8)):
        md = _driver(s, captured, "minimum", barostat=baro, check_every=check_every)
        err = _error_of(ValueError, lambda: md.run(8))
        assert "2 * cutoff" in err
        assert err == _error_of(ValueError, lambda: graph.check_cell(md.cell, U.CUTOFF))      # check_cell's own, on the reported cell
        done.append((md.step, md.cell.cpu(), md.pos.cpu()))
    print(f"guard, minimum image: completed steps {[d[0] for d in done]}")
    assert 1 <= done[0][0] <= 3 and done[0][0] == done[1][0] == done[2][0]
    for d in done[1:]:
        assert torch.equal(d[1], done[0][1]) and torch.equal(d[2], done[0][2])


def test_guard_auto_switches_to_image_ranges(arithmetic):
    s, baro = _guard_case(arithmetic)
    eager, md = _driver(s, False, "auto", barostat=baro), _driver(s, True, "auto", barostat=baro)
    assert md._ranges is None and eager._ranges is None         # it starts on the minimum-image kernels
    for k in range(8):
        eager.run(1), md.run(1)
        R._same(_snapshot(md), _snapshot(eager), f"auto {arithmetic}, step {k + 1}")
    print(f"guard, auto: rebuilds captured {md.rebuilds}, eager {eager.rebuilds}, widths {NU.widths(md.cell.cpu().numpy())[0].min():.4f}")
    assert md.step == eager.step == 8 and md.rebuilds >= 1
    assert float(NU.widths(md.cell.cpu().numpy())[0].min()) < 2 * U.CUTOFF
    assert md._ranges is not None and torch.equal(md._ranges.cpu(), eager._ranges.cpu())
    assert torch.equal(md.npt_log().cpu(), eager.npt_log().cpu())


def test_max_step_stops_the_run_at_the_start(arithmetic):
    start = _start("a", "minimum", arithmetic)
    max_step = 0.01
    gap = 10.0 * float(np.abs(start["p"]).max())
    p0 = float(start["p"][0]) + gap
    beta = 2 * max_step * TAU / (DT * gap)
    de = NU.delta_eps(start["p"], start["vol"], p0, beta, TAU, DT, 0.0)
    assert abs(abs(float(de[0])) - 2 * max_step) < 1e-6 * max_step
    s = _system("a", "minimum")
    for captured in (False, True):
        md = _driver(s, captured, "minimum", barostat=dict(pressure=p0, tau=TAU, compressibility=beta, kT=0.0, max_step=max_step))
        assert re.search("box 0.*max_step = 0.01", _error_of(RuntimeError, lambda: md.run(3)))
        torch.cuda.synchronize()
        assert md.step == 0
        assert torch.equal(md.pos.cpu(), s["pos"].float()) and torch.equal(md.vel.cpu(), s["vel"].float())
        assert torch.equal(md.cell.cpu(), s["cell"].float())
        # half the coupling is inside the limit: the same run goes on
    ok = _driver(s, True, "minimum", barostat=dict(pressure=p0, tau=TAU, compressibility=beta / 4, kT=0.0, max_step=max_step)).run(2)
    assert ok.step == 2 and not torch.equal(ok.cell.cpu(), s["cell"].float())


@pytest.mark.parametrize("thermostat", [False, True], ids=["nve", "langevin"])
def test_no_barostat_is_the_existing_run(arithmetic, thermostat):
    """``barostat=None`` spelled out: the eager references of test_hip_md_run.py, bit for bit."""
    from tests import md_util as MU
    ref, ref_log, ref_rebuilds = R._eager_reference(arithmetic, thermostat)
    md = R._driver(MU.md_molecules(), True, thermostat=THERMOSTAT if thermostat else None, barostat=None)
    for k in range(R.STEPS):
        md.run(1)
        R._same(R._snapshot(md), ref[k], f"{arithmetic}, step {k + 1}")
    assert md.rebuilds == ref_rebuilds and torch.equal(md.energy_log().cpu(), ref_log)
    assert "no barostat" in _error_of(ValueError, md.npt_log) and "no cell" in _error_of(ValueError, lambda: md.cell)
