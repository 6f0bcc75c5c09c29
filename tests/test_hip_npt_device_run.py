"""GPU: constant-pressure MD on the device-rebuilt list (``MDRun(rebuild="device", barostat=)``) and the moving-cell form of
``pipeline.RebuiltStep``.  Recorded against eager bit for bit after every step; device mode against the ``rebuild="host"``
trajectory (bit for bit in "f32" and "split", 1e-4 relative in "f16x2"); runs whose search parameters change under the
barostat; the refusals of gn_cell_image_ranges and of ``max_step``; the step on its own against ``distance_pbc`` and
``EnergyForces`` at a new cell."""
import functools
import math
import re

import numpy as np
import pytest
import torch

from tests import npt_util as NU
from tests import pbc_multi_util as PM
from tests import pbc_util as U

pytestmark = pytest.mark.gpu

DT, FORCE_SCALE = 0.2, 0.05                                            # tests/test_hip_md_run.py's set-up
THERMOSTAT = dict(kT=0.02, gamma=0.5, key=(77, 5))
TAU = 20 * DT
CUTOFF = U.CUTOFF
F16X2_BOUND = 1e-4                                                     # the project's relative bound of the f16x2 arithmetic
RANGE_STEP = CUTOFF / (0.5 - 2.0 ** -6)                                # the width below which the rule asks for R = 1: 2.0645 cutoff


@pytest.fixture(params=["f32", "f16x2"])
def arithmetic(request):
    from gotennet_amd import engine
    old = engine.GEMM_MODE
    engine.GEMM_MODE = request.param
    yield request.param
    engine.GEMM_MODE = old


@pytest.fixture(params=["f32", "split"])
def exact(request):
    """The arithmetics whose rows do not depend on what else is in the batch: padded equals unpadded bit for bit."""
    from gotennet_amd import engine
    old = engine.GEMM_MODE
    engine.GEMM_MODE = request.param
    yield request.param
    engine.GEMM_MODE = old


@functools.lru_cache(maxsize=None)
def _model():
    net, head, *_ = U.make_model(32, 2, 2, seed=1)
    return net.cuda().eval(), head.cuda().eval()


def _ef():
    from gotennet_amd.pipeline import EnergyForces
    return EnergyForces(*_model(), check_edges=False)


def _system(name, scale=1.0, still=False):
    s = dict((U if name == "a" else PM).system(name))
    s["vel"] = 0.05 * torch.randn(s["pos"].shape, generator=torch.Generator().manual_seed(9))
    if still:
        s["vel"] = torch.zeros_like(s["vel"])
    if scale != 1.0:
        s["pos"], s["cell"] = (s["pos"] * scale).float().double(), (s["cell"] * scale).float().double()
    return s


def _driver(s, captured, images, rebuild, **kw):
    from gotennet_amd.md import MDRun
    kw.setdefault("log_len", 64)
    return MDRun(_ef(), s["z"].cuda(), s["pos"].float().cuda(), s["batch"].cuda(), s["n_mol"], dt=DT, force_scale=FORCE_SCALE,
                 vel=s["vel"].float().cuda(), cell=s["cell"].float().cuda(), images=images, captured=captured, rebuild=rebuild, **kw)


def _error_of(kind, fn):
    """The message of the ``kind`` that ``fn()`` raises.  The exception is dropped here: one kept in a test's frame ties that
    frame, the traceback and the driver into a reference cycle, and a recorded hipGraph that only the cyclic collector frees
    may be destroyed in the middle of a later stream capture, which the runtime refuses."""
    try:
        fn()
    except kind as e:
        return str(e)
    raise AssertionError(f"{kind.__name__} was not raised")


NAMES = ("pos", "vel", "cell", "potential energy", "kinetic energy", "stress", "pressure", "volume")


def _snapshot(md):
    torch.cuda.synchronize()
    return [md.pos.cpu(), md.vel.cpu(), md.cell.cpu(), md.potential_energy.cpu(), md.kinetic_energy.cpu(), md.stress.cpu(),
            md.pressure.cpu(), md.volume.cpu()]


def _same(a, b, what):
    assert len(a) == len(b)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), f"{what}: {name} differs, max |difference| {float((x.double() - y.double()).abs().max()):.3e}"


@functools.lru_cache(maxsize=None)
def _start(name, images, mode, scale=1.0, still=False):
    """Start pressure, volume and perpendicular widths per box of a system in the current arithmetic (``mode`` is the cache
    key), from an eager host-mode run without a barostat.  Read-only."""
    md = _driver(_system(name, scale, still), False, images, "host")
    torch.cuda.synchronize()
    return dict(p=NU.pressure(md.kinetic_energy.cpu().numpy(), md.stress.cpu().numpy(), md.volume.cpu().numpy()),
                vol=md.volume.cpu().numpy().astype(np.float64), widths=NU.widths(md.cell.cpu().numpy())[0])


def _coupling(start, kT):
    """beta_T such that the deterministic move towards P0 = 0 starts at |d_eps| <= 1e-3 per step and the noise has a standard
    deviation of at most 2e-3 (far inside max_step = 0.05 even at Box-Muller's largest |xi| = 5.8)."""
    r = 1e-3 / float(np.abs(start["p"]).max())                 # r = beta dt / tau
    if kT > 0:
        r = min(r, (2e-3) ** 2 * float(start["vol"].min()) / (2 * kT))
    return r * TAU / DT


def _baro(start, noise):
    baro = dict(pressure=0.0, tau=TAU, compressibility=_coupling(start, THERMOSTAT["kT"] if noise else 0.0))
    if not noise:
        baro["kT"] = 0.0
    return baro


#: a narrow cell, and a wide one: system ``a`` 5 % larger, every width above 2.0645 * cutoff + 3 %, so that every range is 0
SEARCHES = [("n1", "all", 1.0), ("a", "auto", 1.05)]


# --------------------------------------------------------------------------------------------- recorded against eager
@pytest.mark.parametrize("noise", [True, False], ids=["langevin_kT", "deterministic"])
@pytest.mark.parametrize("name,images,scale", SEARCHES)
def test_device_recorded_equals_device_eager_after_every_step(arithmetic, name, images, scale, noise):
    from gotennet_amd import graph
    start = _start(name, images, arithmetic, scale)
    th, baro = THERMOSTAT if noise else None, _baro(start, noise)
    s = _system(name, scale)
    eager = _driver(s, False, images, "device", thermostat=th, barostat=baro)
    md = _driver(s, True, images, "device", thermostat=th, barostat=baro, check_every=1)
    _same(_snapshot(md), _snapshot(eager), "at the start")
    want = graph.image_ranges(s["cell"].float(), CUTOFF)
    assert torch.equal(md._step._ranges.cpu(), want) and md._step.layout.periodic_images
    assert bool((want == 0).all()) == (name == "a")
    traj = []
    for k in range(12):
        eager.run(1), md.run(1)
        traj.append(_snapshot(eager))
        _same(_snapshot(md), traj[-1], f"{name} {arithmetic}, step {k + 1}")
        assert md.edge_count == eager.edge_count
    assert md.step == eager.step == 12 and md.rebuilds == eager.rebuilds == 0
    assert not torch.equal(traj[-1][2], s["cell"].float()) and not torch.equal(traj[0][2], traj[1][2])      # the cell does move
    log, ref_log = md.npt_log().cpu(), eager.npt_log().cpu()
    assert log.shape == (12, s["n_mol"], 2) and torch.equal(log, ref_log)
    assert torch.equal(md.energy_log().cpu(), eager.energy_log().cpu())
    for k in range(12):
        assert torch.equal(log[k, :, 0], traj[k][7]) and torch.equal(log[k, :, 1], traj[k][6])
    lay = md._step.layout
    print(f"npt device {name} ({images}) {arithmetic} noise={noise}: V {start['vol']} -> {traj[-1][7].tolist()}, edges "
          f"{md.edge_count}, capacity / E_real {lay.edge_capacity / md.edge_count:.2f}, n_pad / N {lay.n_pad / lay.N:.2f}")
    # the check interval is invisible
    md8 = _driver(s, True, images, "device", thermostat=th, barostat=baro, check_every=8).run(12)
    _same(_snapshot(md8), traj[-1], f"{name} {arithmetic}, check_every=8")
    assert md8.step == 12 and torch.equal(md8.npt_log().cpu(), ref_log)


# ------------------------------------------------------------------------------------- device mode against host mode
def _host_and_device(name, images, scale, noise=True, steps=12):
    """Per-step snapshots of the recorded device-mode run and of the eager host-mode run on the same inputs."""
    from gotennet_amd import engine
    start = _start(name, images, engine.GEMM_MODE, scale)
    th, baro = THERMOSTAT if noise else None, _baro(start, noise)
    s = _system(name, scale)
    host = _driver(s, False, images, "host", thermostat=th, barostat=baro)
    dev = _driver(s, True, images, "device", thermostat=th, barostat=baro)
    out = []
    for _ in range(steps):
        host.run(1), dev.run(1)
        out.append((_snapshot(dev), _snapshot(host)))
    assert dev.rebuilds == 0 and dev.step == host.step == steps
    return out, dev, host


@pytest.mark.parametrize("name,images,scale", SEARCHES)
def test_device_mode_is_the_host_mode_trajectory(exact, name, images, scale):
    """On the wide box host mode runs the minimum-image kernels and device mode the multi-image ones with R = 0: the same walk
    candidate for candidate, so the same bits are REQUIRED, not hoped for."""
    out, dev, host = _host_and_device(name, images, scale)
    if name == "a":
        assert host._ranges is None and bool((dev._step._ranges == 0).all())
    for k, (a, b) in enumerate(out):
        _same(a, b, f"{name} ({images}) {exact}, device against host mode, step {k + 1}")
    assert torch.equal(dev.npt_log().cpu(), host.npt_log().cpu()) and torch.equal(dev.energy_log().cpu(), host.energy_log().cpu())
    print(f"device against host, {name} ({images}) {exact}: equal bits over 12 steps; host-mode rebuilds {host.rebuilds}")


def test_device_mode_against_host_mode_f16x2():
    """"f16x2" shares block exponents between neighbouring rows, so the padded batch may differ from the unpadded one: the
    project's bound for that is 1e-4 relative, each quantity against its own largest entry.  The pressure is a difference,
    2 K / (3 V) - tr(stress) / 3, of two terms that each carry that bound: it is measured against the sum of their magnitudes.
    Measured on MI355X: worst relative difference 1.8e-8 over the 12 steps, not equal bits."""
    from gotennet_amd import engine
    old = engine.GEMM_MODE
    engine.GEMM_MODE = "f16x2"
    try:
        out, dev, host = _host_and_device("n1", "all", 1.0)
    finally:
        engine.GEMM_MODE = old
    worst, bits = 0.0, True
    for a, b in out:
        for name, x, y in zip(NAMES, a, b):
            x, y = x.double(), y.double()
            scale = float(y.abs().max())
            if name == "pressure":
                ke, st, vol = b[4].double(), b[5].double(), b[7].double()
                scale = float((2 * ke / (3 * vol)).abs().max() + (st.diagonal(dim1=1, dim2=2).sum(1) / 3).abs().max())
            worst = max(worst, float((x - y).abs().max()) / scale)
            bits = bits and torch.equal(x, y)
    print(f"device against host, n1 (all) f16x2: worst relative difference over 12 steps {worst:.3e}, equal bits: {bits}")
    assert worst <= F16X2_BOUND


# ------------------------------------------------------------------------------- runs whose search parameters change
GUARD_SCALE_MARGIN = 1.002


def _shrink_case(mode, width):
    """tests/test_hip_npt_run.py's ``_guard_case``, restated, for a width to cross: system ``a`` scaled so that its smallest
    perpendicular width is ``width`` * 1.002, and a barostat whose deterministic move is d_eps = -3e-3 per step for every box to
    within a tenth: the width shrinks by 1e-3 per step and crosses ``width`` in the second or third step."""
    w0 = _start("a", "minimum", mode)["widths"]
    scale = width * GUARD_SCALE_MARGIN / float(w0.min())
    start = _start("a", "minimum", mode, scale)
    assert abs(float(start["widths"].min()) / width - GUARD_SCALE_MARGIN) < 1e-5
    gap = 10.0 * float(np.abs(start["p"]).max())               # P0 - P: ten times any start pressure, so it hardly varies
    p0 = float(start["p"].max()) + gap
    beta = 3e-3 * TAU / (DT * gap)
    de = NU.delta_eps(start["p"], start["vol"], p0, beta, TAU, DT, 0.0)
    assert bool((de <= -3e-3 * (1 - 1e-9)).all()) and bool((de > -3.7e-3).all()), de
    w = float(start["widths"].min())
    assert w * math.exp(float(de.max()) / 3) > width > w * math.exp(3 * float(de.max()) / 3)     # after one step / after three
    return _system("a", scale), dict(pressure=p0, tau=TAU, compressibility=beta, kT=0.0)


@pytest.mark.parametrize("crossing", ["twice_the_cutoff", "range_step"])
def test_a_run_whose_search_parameters_change(crossing):
    """Device mode against the host-mode "auto" run, "f32", 8 steps, bit for bit; nothing is re-recorded.

    ``twice_the_cutoff``: the pressure case of tests/test_hip_npt_run.py -- the smallest width crosses 2 * cutoff within three
    steps, where host mode leaves the minimum-image kernels for the multi-image ones.  The device's range array cannot change
    in that run: the rule floor(cutoff / w + 1/2 + 2^-6) asks for R = 1 from w = 2.0645 * cutoff down, so it holds [1, 0, 0] for
    both boxes from the start (asserted), and stays what ``graph.image_ranges`` gives for the final cell.
    ``range_step``: the same system and barostat one step of the rule further out -- the smallest width crosses
    2.0645 * cutoff.  Host mode stays on the minimum-image kernels; the device's range array starts all zero, ends different
    and equals ``graph.image_ranges`` of the final cell: a changed search parameter inside one recorded graph."""
    from gotennet_amd import engine, graph
    old = engine.GEMM_MODE
    engine.GEMM_MODE = "f32"
    try:
        s, baro = _shrink_case("f32", 2 * CUTOFF if crossing == "twice_the_cutoff" else RANGE_STEP)
        host, md = _driver(s, False, "auto", "host", barostat=baro), _driver(s, True, "auto", "device", barostat=baro)
        assert host._ranges is None                             # it starts on the minimum-image kernels
        first = md._step._ranges.cpu().clone()
        assert torch.equal(first, graph.image_ranges(s["cell"].float(), CUTOFF))
        for k in range(8):
            host.run(1), md.run(1)
            _same(_snapshot(md), _snapshot(host), f"{crossing}, device against host mode, step {k + 1}")
            assert md.edge_count == host.edge_count
    finally:
        engine.GEMM_MODE = old
    last, w = md._step._ranges.cpu(), float(NU.widths(md.cell.cpu().numpy())[0].min())
    print(f"{crossing}: smallest width {w:.4f}, ranges {first.tolist()} -> {last.tolist()}, host-mode rebuilds {host.rebuilds}")
    assert md.step == host.step == 8 and md.rebuilds == 0
    assert torch.equal(last, graph.image_ranges(md.cell.cpu(), CUTOFF))
    assert torch.equal(md.npt_log().cpu(), host.npt_log().cpu())
    if crossing == "twice_the_cutoff":
        assert w < 2 * CUTOFF and host._ranges is not None and host.rebuilds >= 1
        assert first.tolist() == [[1, 0, 0], [1, 0, 0]]
    else:
        assert 2 * CUTOFF < w < RANGE_STEP and host._ranges is None
        assert bool((first == 0).all()) and not torch.equal(last, first)


# ------------------------------------------------------------------------------------------------------ refusals
def test_a_cell_driven_below_a_third_of_the_cutoff_stops_both_modes():
    """One atom in a cube that starts 0.3 % above cutoff / 3, under a pressure that shrinks every width by some 6 % per step
    (d_eps = -0.2, ``max_step`` = 1 out of the way; P0 - P is a thousand times the start pressure, so the move hardly varies).
    gn_cell_image_ranges refuses once R = 4 is needed, at a width of cutoff / (3.5 - 2^-6) = 0.86 * cutoff / 3: in the third
    step at that rate."""
    from gotennet_amd import engine, graph
    old = engine.GEMM_MODE
    engine.GEMM_MODE = "f32"
    try:
        w0 = float(PM.system("n3")["cell"][0, 0, 0])
        scale = CUTOFF / 3.0 * 1.003 / w0
        start = _start("n3", "all", "f32", scale)
        assert CUTOFF / 3.0 < float(start["widths"].min()) < CUTOFF / 3.0 * 1.004
        gap = 1000.0 * float(np.abs(start["p"]).max())
        assert gap > 0
        p0, beta = float(start["p"].max()) + gap, 0.2 * TAU / (DT * gap)
        baro = dict(pressure=p0, tau=TAU, compressibility=beta, kT=0.0, max_step=1.0)
        s, done = _system("n3", scale), []
        for captured, check_every in ((False, 1), (True, 1), (True, 8)):
            md = _driver(s, captured, "all", "device", barostat=baro, check_every=check_every)
            err = _error_of(ValueError, lambda: md.run(8))
            assert "cutoff / 3" in err
            assert err == _error_of(ValueError, lambda: graph.image_ranges(md.cell, CUTOFF))     # the host's own, on the reported cell
            torch.cuda.synchronize()
            assert md._reason.tolist() == [1] and md.rebuilds == 0
            done.append((md.step, md.cell.cpu(), md.pos.cpu(), md._step._ranges.cpu()))
    finally:
        engine.GEMM_MODE = old
    print(f"below cutoff / 3: completed steps {[d[0] for d in done]}, reported width {float(done[0][1][0, 0, 0]):.4f}")
    assert 1 <= done[0][0] <= 6 and done[0][0] == done[1][0] == done[2][0]
    assert float(done[0][1][0, 0, 0]) < CUTOFF / (3.5 - 2.0 ** -6)
    for d in done[1:]:
        assert torch.equal(d[1], done[0][1]) and torch.equal(d[2], done[0][2]) and torch.equal(d[3], done[0][3])
    assert done[0][3].tolist() == [[3, 3, 3]]                    # the refused box kept its row


def test_max_step_stops_the_device_run_at_the_start():
    from gotennet_amd import engine
    old = engine.GEMM_MODE
    engine.GEMM_MODE = "f32"
    try:
        start = _start("n1", "all", "f32")
        max_step = 0.01
        gap = 10.0 * float(np.abs(start["p"]).max())
        p0 = float(start["p"][0]) + gap
        beta = 2 * max_step * TAU / (DT * gap)
        de = NU.delta_eps(start["p"], start["vol"], p0, beta, TAU, DT, 0.0)
        assert abs(abs(float(de[0])) - 2 * max_step) < 1e-6 * max_step
        s, errors = _system("n1"), []
        for captured in (False, True):
            md = _driver(s, captured, "all", "device", barostat=dict(pressure=p0, tau=TAU, compressibility=beta, kT=0.0, max_step=max_step))
            errors.append(_error_of(RuntimeError, lambda: md.run(3)))
            assert re.search("box 0.*max_step = 0.01", errors[-1])
            torch.cuda.synchronize()
            assert md.step == 0 and md._reason.tolist() == [2]
            assert torch.equal(md.pos.cpu(), s["pos"].float()) and torch.equal(md.vel.cpu(), s["vel"].float())
            assert torch.equal(md.cell.cpu(), s["cell"].float())
        assert errors[0] == errors[1]
        # a quarter of the coupling is inside the limit: the same run goes on
        ok = _driver(s, True, "all", "device", barostat=dict(pressure=p0, tau=TAU, compressibility=beta / 4, kT=0.0, max_step=max_step)).run(2)
        assert ok.step == 2 and not torch.equal(ok.cell.cpu(), s["cell"].float())
    finally:
        engine.GEMM_MODE = old


# ------------------------------------------------------------------------------------------ the step on its own
def test_moving_cell_step_follows_set_cell(gemm_mode):
    from gotennet_amd import graph
    from gotennet_amd.pipeline import RebuiltStep
    s = PM.system("n1")
    z, batch, pos, cell = s["z"].cuda(), s["batch"].cuda(), s["pos"].float().cuda(), s["cell"].float().cuda()
    ef = _ef()
    step = RebuiltStep(ef, z, batch, s["n_mol"], cell=cell, images="all", cell_moves=True)
    fixed = RebuiltStep(ef, z, batch, s["n_mol"], cell=cell, images="all")
    assert step.cell_moves and not fixed.cell_moves and fixed.reason is None and step.capacity == fixed.capacity
    a, b = step(pos), fixed(pos)
    torch.cuda.synchronize()
    for what, x, y in zip(("energy", "forces", "stress"), a, b):
        assert torch.equal(x, y), f"{gemm_mode}: a cell that never moves: {what} differs from the fixed-cell step"
    assert int(step.edge_count.item()) == int(fixed.edge_count.item())
    for new in (cell * 0.97, (cell * 0.97)[0]):                            # [n_mol, 3, 3], and a [3, 3] cell broadcast
        if new.dim() == 2:
            step.set_cell(cell)                                            # back first: the next cell is a change again
            step(pos)
        step.set_cell(new)
        new = new.reshape(-1, 3, 3)
        got = [t.clone() for t in step(pos)]
        torch.cuda.synchronize()
        assert step.state.tolist() == [0] and step.reason.tolist() == [0]
        assert torch.equal(step.cell, new) and torch.equal(step._ranges.cpu(), graph.image_ranges(new.cpu(), CUTOFF))
        ei, ed, ev, sh = graph.distance_pbc(pos, batch, new, CUTOFF, 32, n_mol=s["n_mol"], images="all")
        E = int(step.edge_count.item())
        assert E == ei.shape[1] != int(fixed.edge_count.item())             # the list did change with the cell
        assert torch.equal(step.edge_index[:, :E], ei) and torch.equal(step.edge_shift[:E], sh)
        assert torch.equal(step.edge_vec[:E], ev) and torch.equal(step.edge_diff[:E], ed)
        want = ef(z, ei, ed, ev, batch, s["n_mol"], cell=new)
        torch.cuda.synchronize()
        worst = 0.0
        for what, x, y in zip(("energy", "forces", "stress"), got, want):
            rel = float((x.double() - y.double()).abs().max() / y.double().abs().max())
            worst = max(worst, rel)
            print(f"moving-cell step against EnergyForces, {gemm_mode}: {what} relative difference {rel:.3e}, equal bits: {torch.equal(x, y)}")
        assert worst <= F16X2_BOUND if gemm_mode == "f16x2" else worst == 0.0
    assert "fixed at construction" in _error_of(ValueError, lambda: step(pos, cell=cell))       # a cell per call: as before
    assert "cell_moves" in _error_of(ValueError, lambda: fixed.set_cell(cell))
    # a cell the range kernel refuses: the word, the reason, and the ranges kept
    keep = step._ranges.clone()
    step.set_cell(cell * 0.1)
    step(pos)
    torch.cuda.synchronize()
    assert step.state.tolist() == [1] and step.reason.tolist() == [1] and torch.equal(step._ranges, keep)


def test_one_replay_advances_one_step(arithmetic):
    """One graph per driver; the first replay is ``run(1)``'s and is followed by its synchronisation."""
    start = _start("n1", "all", arithmetic)
    baro, s = _baro(start, True), _system("n1")
    eager = _driver(s, False, "all", "device", thermostat=THERMOSTAT, barostat=baro).run(13)
    md = _driver(s, True, "all", "device", thermostat=THERMOSTAT, barostat=baro)
    md.run(1)
    cells = [md.cell.cpu()]
    for k in range(2, 14):
        md._step.graph.replay()
        assert md._state.tolist() == [0, k]                            # (a host read: a synchronisation per replay)
        cells.append(md._cell.cpu().clone())
    assert all(not torch.equal(x, y) for x, y in zip(cells, cells[1:]))       # every replay moved the cell
    _same(_snapshot(md), _snapshot(eager), "after 13 replays")
