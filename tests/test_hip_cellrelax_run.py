"""GPU: the variable-cell relaxation driver on ``pbc_multi_util.system("n4")`` -- a wide 12-atom triclinic box and a narrow
2-atom box in one batch, so the image ranges are zero in one and non-zero in the other.  The recorded mode is held to the
eager mode bit for bit after every step; every step of the device run is held to the fp64 rule of tests/cellrelax_util.py
applied to the device's own state before it (the bounds of tests/test_hip_fire_kernels.py for plan and move, 1 ulp for the
generalised forces and the apply step: fp64 rounded once)."""
import functools

import pytest
import torch

from tests import cellrelax_util as CU
from tests import fire_util as FU
from tests import pbc_multi_util as PM
from tests import pbc_util as U

pytestmark = pytest.mark.gpu

STEPS, FMAX = 12, 1e-3
MOL_PTR = [0, 12, 14]
ATOM_MOL = torch.repeat_interleave(torch.arange(2), torch.tensor([12, 2]))
_ulp = FU.ulp32


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
    from gotennet_amd import CellRelax
    from gotennet_amd.pipeline import EnergyForces
    net, head = _model()
    kw.setdefault("log_len", 64)
    kw.setdefault("fmax", FMAX)
    return CellRelax(EnergyForces(net, head, check_edges=False), s["z"].cuda(), s["pos"].float().cuda(), s["batch"].cuda(),
                     s["n_mol"], cell=s["cell"].float().cuda(), captured=captured, **kw)


NAMES = ("pos", "cell", "vel", "cell_vel", "energy", "forces", "stress", "dt", "alpha", "n_pos", "status", "converged_at", "coef",
         "x_ext", "vel_ext", "g_ext")


def _snapshot(rx):
    torch.cuda.synchronize()
    out = [rx.pos, rx.cell, rx.vel, rx.cell_vel, rx.potential_energy, rx.forces, rx.stress, rx._dt, rx._alpha, rx._n_pos, rx.status,
           rx.converged_at, rx._coef, rx._x_ext, rx._vel_ext, rx._g_ext]
    return [t.cpu().clone() for t in out]


def _same(a, b, what):
    assert len(a) == len(b) == len(NAMES)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: {NAMES[k]} differs, max |difference| {float((x.double() - y.double()).abs().max()):.3e}"


@functools.lru_cache(maxsize=None)
def _eager_reference(mode):
    """The eager run of n4 in the current arithmetic (``mode`` is the cache key), computed once: (the snapshot at the start and
    after every step, the log, the enthalpy at the start and at the end, fmax at the start, reason).  Read-only."""
    rx = _driver(PM.system("n4"), False)
    traj, h0, fmax0 = [_snapshot(rx)], rx.enthalpy.cpu(), rx.fmax.cpu()
    for _ in range(STEPS):
        rx.run(1)
        traj.append(_snapshot(rx))
    return traj, rx.log().cpu(), h0, rx.enthalpy.cpu(), fmax0, rx._reason.tolist(), rx.rebuilds


def test_captured_equals_eager_after_every_step(arithmetic):
    ref, ref_log, _, _, _, reason, ref_rebuilds = _eager_reference(arithmetic)
    s = PM.system("n4")
    rx = _driver(s, True, check_every=1)
    assert rx.rebuild == "device"
    _same(_snapshot(rx), ref[0], f"{arithmetic}, start")
    assert torch.equal(ref[0][0], s["pos"].float()) and torch.equal(ref[0][1], s["cell"].float())
    for k in range(STEPS):
        rx.run(1)
        _same(_snapshot(rx), ref[k + 1], f"{arithmetic}, step {k + 1}")
    print(f"{arithmetic}: status {rx.status.tolist()}, edges {rx.edge_count}, cell moved by "
          f"{float((ref[-1][1] - ref[0][1]).abs().max()):.3e}, volume {rx.volume.tolist()}")
    assert rx.step == STEPS and rx.rebuilds == ref_rebuilds == 0 and reason == [0, 0] and rx._reason.tolist() == [0, 0]
    assert torch.equal(rx.log().cpu(), ref_log) and ref_log.shape == (STEPS, 2, 2)
    for m in range(2):                                                   # the cell does move, in both boxes
        assert not torch.equal(ref[-1][1][m], ref[0][1][m])
    # the check interval is invisible
    rx8 = _driver(s, True, check_every=8).run(STEPS)
    _same(_snapshot(rx8), ref[-1], f"{arithmetic}, check_every=8")
    assert rx8.step == STEPS and rx8.rebuilds == 0 and torch.equal(rx8.log().cpu(), ref_log)
    # the queries: the extended fmax is what the next step would log; G and F are the cell rows
    lay = CU.layout(MOL_PTR)
    assert torch.equal(rx.deformation.cpu(), (ref[-1][13][lay["cell_rows"]].double() / rx._w.cpu().double().reshape(2, 1, 1)).float())
    assert torch.equal(rx.vel.cpu(), ref[-1][14][lay["atom_rows"]]) and torch.equal(rx.cell_vel.cpu(), ref[-1][14][lay["cell_rows"]])


def test_every_step_is_the_fp64_rule_on_the_device_state(arithmetic):
    ref, log, *_ = _eager_reference(arithmetic)
    p = dict(FU.DEFAULTS, fmax=FMAX)
    lay, w = CU.layout(MOL_PTR), CU.weights(MOL_PTR)
    cell0 = ref[0][1]
    ext_mol = torch.repeat_interleave(torch.arange(2), torch.tensor([15, 5]))
    for k in range(STEPS):
        b, a = dict(zip(NAMES, ref[k])), dict(zip(NAMES, ref[k + 1]))
        # the generalised forces of the kept state: fp64, rounded once
        g64 = CU.generalised_forces(b["forces"], b["stress"], b["cell"], b["x_ext"], MOL_PTR, w)
        assert bool(CU.within_ulps(a["g_ext"], g64, 1).all()), k
        # the plan, from the device's own generalised forces
        st = dict(dt=b["dt"].double(), alpha=b["alpha"].double(), n_pos=b["n_pos"].long(), status=b["status"].long(),
                  converged_at=b["converged_at"].long())
        _, _, st1, info = FU.fire_step(b["x_ext"], b["vel_ext"], a["g_ext"], lay["mol_ptr_ext"], st, p, step=k)
        for name in ("n_pos", "status", "converged_at"):
            assert a[name].tolist() == st1[name].tolist(), (k, name)
        active = info["coef"][:, 3] == 1.0
        assert a["coef"][:, 3].tolist() == info["coef"][:, 3].tolist(), k
        for name in ("dt", "alpha"):
            assert bool(((a[name].double() - st1[name]).abs() <= _ulp(st1[name])).all()), (k, name)
        assert bool(((a["coef"].double() - info["coef"]).abs() <= _ulp(info["coef"]))[active].all()), k
        assert bool(((log[k, :, 1].double() - info["fmax"]).abs() <= 3 * _ulp(info["fmax"])).all()), k
        assert torch.equal(log[k, :, 0], b["energy"]), k
        # the move of the extended rows, from the device's own coefficients
        coef = a["coef"].double()
        x1, v1, _, _ = FU.fire_step(b["x_ext"], b["vel_ext"], a["g_ext"], lay["mol_ptr_ext"], st, p, step=k, coef=coef)
        c, f64, v64 = coef[ext_mol], a["g_ext"].double(), b["vel_ext"].double()
        big_v = torch.maximum(torch.maximum((c[:, 0:1] * v64).abs(), (c[:, 1:2] * f64).abs()), (c[:, 2:3] * f64).abs())
        moved = active[ext_mol]
        assert torch.equal(a["vel_ext"][~moved], b["vel_ext"][~moved]) and torch.equal(a["x_ext"][~moved], b["x_ext"][~moved]), k
        assert bool(((a["vel_ext"].double() - v1).abs() <= 4 * _ulp(big_v))[moved].all()), k
        big_p = torch.maximum(b["x_ext"].double().abs(), (x1 - b["x_ext"].double()).abs())
        assert bool(((a["x_ext"].double() - x1).abs() <= 8 * _ulp(big_p) + c[:, 2:3].abs() * 4 * _ulp(big_v))[moved].all()), k
        # apply, from the device's own moved rows: fp64, rounded once; a box that did not move keeps its bits
        pos1, cell1 = CU.apply(a["x_ext"], cell0, MOL_PTR, w, b["pos"], b["cell"], active=active)
        assert bool(CU.within_ulps(a["pos"], pos1, 1).all()) and bool(CU.within_ulps(a["cell"], cell1, 1).all()), k
        assert torch.equal(a["pos"][~active[ATOM_MOL]], b["pos"][~active[ATOM_MOL]]) and torch.equal(a["cell"][~active], b["cell"][~active]), k
        # finish: the kept values of a box that is not active are not refreshed
        done = st1["status"] != 0
        assert torch.equal(a["forces"][done[ATOM_MOL]], b["forces"][done[ATOM_MOL]]) and torch.equal(a["energy"][done], b["energy"][done]), k
        assert torch.equal(a["stress"][done], b["stress"][done]), k
        assert not torch.equal(a["forces"][~done[ATOM_MOL]], b["forces"][~done[ATOM_MOL]]), k


def test_the_enthalpy_falls(arithmetic):
    ref, _, h0, h1, _, reason, _ = _eager_reference(arithmetic)
    status = ref[-1][NAMES.index("status")]
    print(f"{arithmetic}: enthalpy at the start {h0.tolist()}, after {STEPS} steps {h1.tolist()}, status {status.tolist()}")
    assert reason == [0, 0] and bool((status == 0).any())
    assert bool((h1 < h0)[status == 0].all())


def test_a_box_below_fmax_freezes_at_step_0_and_the_other_goes_on():
    """fmax between the largest generalised forces of the two boxes at the start (an input condition, asserted)."""
    from gotennet_amd import engine
    old = engine.GEMM_MODE
    engine.GEMM_MODE = "f32"
    try:
        fmax0 = _eager_reference("f32")[4]
        lo, hi = int(fmax0.argmin()), int(fmax0.argmax())
        assert float(fmax0[lo]) * 1.05 < float(fmax0[hi])
        s = PM.system("n4")
        rx = _driver(s, True, fmax=0.5 * float(fmax0[lo] + fmax0[hi]), check_every=4).run(6)
    finally:
        engine.GEMM_MODE = old
    want = [0, 0]
    want[lo] = 1
    assert rx.status.tolist() == want and rx.converged_at.tolist()[lo] == 0 and rx.step == 6
    atoms = ATOM_MOL == lo
    assert torch.equal(rx.cell.cpu()[lo], s["cell"].float()[lo]) and torch.equal(rx.pos.cpu()[atoms], s["pos"].float()[atoms])
    assert bool((rx.vel.cpu()[atoms] == 0).all()) and bool((rx.cell_vel.cpu()[lo] == 0).all())
    assert not torch.equal(rx.cell.cpu()[hi], s["cell"].float()[hi]) and not torch.equal(rx.pos.cpu()[~atoms], s["pos"].float()[~atoms])


def _deformation64(rx):
    torch.cuda.synchronize()
    return CU.deformation(rx._x_ext.cpu(), MOL_PTR, rx._w.cpu())


def test_hydrostatic_and_masked_cells():
    from gotennet_amd import engine
    old = engine.GEMM_MODE
    engine.GEMM_MODE = "f32"
    s = PM.system("n4")
    c0 = s["cell"].float()
    try:
        hyd = _driver(s, True, hydrostatic=True, check_every=6).run(6)
        mask = torch.tensor([[1, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=torch.bool)
        msk = _driver(s, True, cell_mask=mask.cuda(), check_every=6).run(6)
    finally:
        engine.GEMM_MODE = old
    # hydrostatic: F = s 1.  The off-diagonal cell rows see forces and velocities that are exactly zero; the diagonal ones see
    # the same numbers, so they agree (2 ulp allows for nothing but a different contraction of equal expressions)
    F = hyd.deformation.cpu()
    F64 = _deformation64(hyd)                                           # what gn_cellrelax_apply reads: cell rows / w in fp64
    eye = torch.eye(3, dtype=torch.bool)
    for m in range(2):
        assert bool((F[m][~eye] == 0).all()) and float(F[m][0, 0]) != 1.0
        assert bool(((F[m][eye].double() - F[m][0, 0].double()).abs() <= 2 * _ulp(F[m][0, 0:1])).all())
        assert bool(CU.within_ulps(hyd.cell.cpu()[m], c0[m].double() * F64[m][0, 0], 1).all())
    assert hyd._reason.tolist() == [0, 0] and msk._reason.tolist() == [0, 0]
    # a mask on the third row and column: those entries of F keep their start values EXACTLY (0, 0, 1).  For a triclinic C0 that
    # means: the third COLUMN of the cell, sum_j C0[i, j] F[j, 2] = C0[i, 2], keeps its bits; the first two entries of the third
    # ROW change only through the free block, cell[2, :2] = C0[2, :2] F[:2, :2]
    F, F64, cell = msk.deformation.cpu(), _deformation64(msk), msk.cell.cpu()
    for m in range(2):
        assert torch.equal(F[m][~mask], torch.eye(3)[~mask]) and not torch.equal(F[m][mask], torch.eye(3)[mask])
        assert torch.equal(cell[m][:, 2], c0[m][:, 2])
        want = c0[m][2, :2].double() @ F64[m][:2, :2]
        assert bool(CU.within_ulps(cell[m][2, :2], want, 1).all()) and not torch.equal(cell[m][:2, :2], c0[m][:2, :2])


def _error_of(kind, fn):
    """The message of the ``kind`` that ``fn()`` raises.  The exception is dropped here: one kept in a test's frame ties that frame,
    the traceback and the driver into a reference cycle, and a recorded hipGraph that only the cyclic collector frees may be
    destroyed in the middle of a later stream capture, which the runtime refuses."""
    try:
        fn()
    except kind as e:
        return str(e)
    raise AssertionError(f"{kind.__name__} was not raised")


def test_a_cell_driven_below_a_third_of_the_cutoff_stops_both_modes():
    """One atom in a cube that starts 0.3 % above cutoff / 3, under a pressure so large that every step is the clamped one: the
    three diagonal cell rows share ``max_step`` = 0.2 (w = 1), 0.2 / sqrt(3) = 0.115 of F each.  gn_cell_image_ranges refuses once
    R = 4 is needed, at a width of cutoff / (3.5 - 2^-6) = 0.86 * cutoff / 3: in the second step at that rate.  A host-side raise
    on a device flag."""
    from gotennet_amd import engine, graph
    old = engine.GEMM_MODE
    engine.GEMM_MODE = "f32"
    try:
        s = dict(PM.system("n3"))
        scale = U.CUTOFF / 3.0 * 1.003 / float(s["cell"][0, 0, 0])
        s["pos"], s["cell"] = (s["pos"] * scale).float().double(), (s["cell"] * scale).float().double()
        done = []
        for captured, check_every in ((False, 1), (True, 1), (True, 8)):
            rx = _driver(s, captured, pressure=1000.0, check_every=check_every)
            err = _error_of(ValueError, lambda: rx.run(8))
            assert "cutoff / 3" in err
            assert err == _error_of(ValueError, lambda: graph.image_ranges(rx.cell, U.CUTOFF))     # the host's own, on the reported cell
            torch.cuda.synchronize()
            assert rx._reason.tolist() == [1] and rx.rebuilds == 0
            done.append((rx.step, rx.cell.cpu(), rx.pos.cpu(), rx.status.tolist()))
    finally:
        engine.GEMM_MODE = old
    print(f"below cutoff / 3: completed steps {[d[0] for d in done]}, reported width {float(done[0][1][0, 0, 0]):.4f}")
    assert 1 <= done[0][0] <= 3 and done[0][0] == done[1][0] == done[2][0]
    assert float(done[0][1][0, 0, 0]) < U.CUTOFF / (3.5 - 2.0 ** -6)
    for d in done[1:]:
        assert torch.equal(d[1], done[0][1]) and torch.equal(d[2], done[0][2]) and d[3] == done[0][3]


@pytest.mark.parametrize("captured", [True, False], ids=["captured", "eager"])
def test_a_force_or_stress_that_is_not_finite_stops_the_run(captured):
    s = PM.system("n4")
    rx = _driver(s, captured)
    rx._f[13, 1] = float("nan")                      # box 1
    msg = _error_of(RuntimeError, lambda: rx.run(3))
    assert "molecule 1" in msg
    assert rx.status.tolist() == [0, 2] and rx.converged_at.tolist() == [-1, 0]
    assert torch.equal(rx.pos.cpu()[12:], s["pos"].float()[12:]) and torch.equal(rx.cell.cpu()[1], s["cell"].float()[1])
    assert bool((rx.vel.cpu()[12:] == 0).all()) and bool((rx.cell_vel.cpu()[1] == 0).all())
    rx = _driver(s, captured)
    rx._stress[0, 2, 1] = float("inf")               # box 0
    msg = _error_of(RuntimeError, lambda: rx.run(3))
    assert "molecule 0" in msg and rx.status.tolist() == [2, 0]
    assert torch.equal(rx.pos.cpu()[:12], s["pos"].float()[:12]) and torch.equal(rx.cell.cpu()[0], s["cell"].float()[0])
