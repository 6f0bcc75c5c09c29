"""GPU: the relaxation kernels of csrc/gn_fire.hip, each on its own, against the fp64 emulation of tests/fire_util.py.

One batch of synthetic forces and velocities holds every molecule size at which the reductions change path (0, 1, the wave
edge 63 / 64 / 65, the stride edge 256 / 257, 600) and every branch of the plan.  ``mol_ptr`` is written by hand, and every
output lies between guard words.

Bounds (derived, not measured).  ulp(x) is the spacing of fp32 at |x|.
  * dt, alpha, coef: formed in fp64 from fp32 inputs and rounded once -> within 1 ulp of the fp64 value (the fp64 sums of the
    kernel and of the emulation differ by their order alone, ~1e-16 relative: it can move a rounding, never more).
  * the largest force: the kernel accumulates |f|^2 as fl(fl(fl(x x) + fl(y y)) + fl(z z)) in fp32 and takes a correctly rounded
    square root.  Every operation is an IEEE one (the library is built without contraction), so the value is held to its fp32
    emulation BIT FOR BIT; against the fp64 value that is 3 roundings of the square (relative 3 u, u = 2^-24), halved by the
    root, plus the root's own: 2.5 u, at most 2.5 ulps (1 ulp is between u and 2 u relative) -> 3 ulps.
  * vel = fmaf(dt, f, fmaf(c_f, f, c_v v)): three roundings, of c_v v, of the inner sum (at most 2 M, M the largest of the
    three terms) and of the result (at most 3 M): (1/2) ulp(M) + (1/2) ulp(2 M) + (1/2) ulp(3 M) <= 3.5 ulp(M) -> 4 ulp(M).
  * pos += scale (dt vel): three roundings again, (1/2) ulp(D) twice for the displacement D and (1/2) ulp(2 M') for the sum
    (M' the larger of |pos| and D), plus the rounding of scale, (1/2) ulp(D) -> 4 ulp(M'), with the emulation fed the
    kernel's own velocities (an input of this expression; their own error is bounded above).
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import fire_util as FU

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 256, 257, 600, 4, 5, 3, 7, 6)
(EMPTY, FIRST, AT_NMIN, PAST_NMIN, UPHILL, CAPPED, BIG_FORCE, MASKED, EQUAL, ZERO, NAN, DONE, MASK_CONVERGES) = range(13)
P = dict(FU.DEFAULTS, fmax=0.25, max_step=0.5)
STEP, LOG_LEN, PAD, GUARD = 21, 4, 8, 7.0


_ulp = FU.ulp32


def _f2_emulated(force, free):
    """max_a fl(fl(fl(x x) + fl(y y)) + fl(z z)) over the free atoms, and its fp32 root, in numpy fp32; (0, 0) for none."""
    f = force.numpy().astype(np.float32)[free.numpy()]
    if f.shape[0] == 0:
        return np.float32(0), np.float32(0)
    d = f[:, 0] * f[:, 0]
    d = d + f[:, 1] * f[:, 1]
    d = d + f[:, 2] * f[:, 2]
    m = np.float32(np.nan) if np.isnan(d).any() else d.max()
    return m, np.sqrt(m)


@functools.lru_cache(maxsize=None)
def _batch():
    """The synthetic batch on the host (fp32 values) and its fp64 expectation.  Read-only."""
    g = torch.Generator().manual_seed(4)
    ptr_ = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    N, n_mol = int(ptr_[-1]), len(SIZES)
    sl = [slice(int(ptr_[m]), int(ptr_[m + 1])) for m in range(n_mol)]
    f = torch.randn((N, 3), generator=g).float()
    v = (0.05 * f + 0.02 * torch.randn((N, 3), generator=g)).float()               # downhill: P > 0 by a wide margin
    pos = (3.0 * torch.randn((N, 3), generator=g)).float()
    fixed = torch.zeros(N, dtype=torch.bool)
    f[sl[FIRST]], v[sl[FIRST]] = torch.tensor([0.6, -0.8, 0.3]), 0.0
    v[sl[UPHILL]] = (-0.05 * f[sl[UPHILL]] + 0.02 * torch.randn((SIZES[UPHILL], 3), generator=g)).float()
    f[sl[BIG_FORCE]] *= 40.0                                                     # the clamp binds hard
    a = sl[MASKED].start
    f[a + 17] = torch.tensor([9.0, 0.0, 0.0])                                    # the largest force of the batch, masked out
    fixed[a + 17] = fixed[a + 300] = fixed[a + 599] = True
    f[sl[EQUAL]] = torch.tensor([[0.25, 0, 0], [0, 0.125, 0], [0, 0, -0.25], [0.125, 0, 0]])     # fm2 = fmax^2 exactly
    f[sl[ZERO]] = 0.0
    f[sl[NAN].start + 1, 2] = float("nan")
    a = sl[MASK_CONVERGES].start
    f[sl[MASK_CONVERGES]] = (0.05 * torch.randn((SIZES[MASK_CONVERGES], 3), generator=g)).float()
    f[a + 2] = torch.tensor([3.0, 0.0, 0.0])
    fixed[a + 2] = True
    st = FU.new_state(n_mol, P)
    st["dt"] = torch.tensor([0.1, 0.1, 0.1, 0.13, 0.2, 0.95, 0.1, 0.1, 0.1, 0.1, 0.1, 0.3, 0.1], dtype=torch.float32).double()
    st["alpha"] = torch.tensor([0.1, 0.1, 0.1, 0.099, 0.07, 0.05, 0.1, 0.0813, 0.1, 0.1, 0.1, 0.02, 0.1], dtype=torch.float32).double()
    st["n_pos"] = torch.tensor([3, -1, P["n_min"], P["n_min"] + 1, 4, 9, 2, 7, 1, 1, 1, 8, 1])
    st["status"][DONE], st["converged_at"][DONE] = 1, 3
    e_keep = torch.randn(n_mol, generator=g).float()
    pos1, vel1, st1, info = FU.fire_step(pos, v, f, ptr_.tolist(), st, P, fixed=fixed, step=STEP)
    return dict(N=N, n_mol=n_mol, ptr=ptr_, sl=sl, f=f, v=v, pos=pos, fixed=fixed, st=st, e_keep=e_keep, st1=st1, info=info,
                pos1=pos1, vel1=vel1)


def test_the_batch_takes_every_branch():
    """Conditions on the INPUT, from the fp64 emulation alone."""
    b = _batch()
    info, st, st1 = b["info"], b["st"], b["st1"]
    assert st1["status"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 1, 1]
    assert st1["converged_at"].tolist() == [STEP, -1, -1, -1, -1, -1, -1, -1, STEP, STEP, STEP, 3, STEP]
    assert st1["n_pos"].tolist() == [3, 0, P["n_min"] + 1, P["n_min"] + 2, 0, 10, 3, 8, 1, 1, 1, 8, 1]
    assert float(st1["dt"][AT_NMIN]) == float(st["dt"][AT_NMIN]) and float(st1["dt"][PAST_NMIN]) > float(st["dt"][PAST_NMIN])
    assert float(st1["dt"][CAPPED]) == P["dt_max"] < float(st["dt"][CAPPED]) * P["f_inc"]
    assert float(st1["dt"][UPHILL]) == float(st["dt"][UPHILL]) * P["f_dec"] and float(info["P"][UPHILL]) < 0
    assert float(info["fmax"][EQUAL]) == P["fmax"] and float(info["fmax"][ZERO]) == 0.0 and math.isnan(float(info["fmax"][NAN]))
    # the masks matter: without them MASKED reports 9 and MASK_CONVERGES stays active
    assert float(info["fmax"][MASKED]) < 9.0 == float(b["f"][b["sl"][MASKED]].norm(dim=1).max())
    assert float(info["fmax"][MASK_CONVERGES]) < P["fmax"] < float(b["f"][b["sl"][MASK_CONVERGES]].norm(dim=1).max())
    moved = [m for m in range(b["n_mol"]) if float(info["coef"][m, 3]) == 1.0]
    assert moved == [FIRST, AT_NMIN, PAST_NMIN, UPHILL, CAPPED, BIG_FORCE, MASKED]
    for m in moved:
        if m != FIRST:
            assert abs(float(info["P"][m])) >= 1e-3 * float(info["absP"][m]), m          # no decision near P = 0
        assert abs(float(info["fmax"][m]) - P["fmax"]) > 0.1 * P["fmax"], m
        assert abs(math.sqrt(float(info["n2"][m])) - P["max_step"]) > 1e-3 * P["max_step"], m      # nor near the clamp
    scales = [float(info["scale"][m]) for m in moved]
    assert any(s == 1.0 for s in scales) and any(s < 1.0 for s in scales) and float(info["scale"][BIG_FORCE]) < 0.1


def _guarded(t, fill=GUARD):
    """A device copy of ``t`` between ``PAD`` guard words on either side -> (the view to hand to a kernel, the whole buffer)."""
    flat = t.reshape(-1)
    whole = torch.full((flat.numel() + 2 * PAD,), fill, dtype=t.dtype).cuda()
    view = whole[PAD:PAD + flat.numel()]
    view.copy_(flat)
    return view.view(t.shape), whole


def _guards_intact(whole, fill=GUARD):
    w = whole.cpu()
    return bool((w[:PAD] == fill).all()) and bool((w[-PAD:] == fill).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Device:
    """The batch on the device, every kernel output between guard words."""

    def __init__(self, stale=0, coef=None):
        from gotennet_amd._lib import ptr
        b = _batch()
        self.b, self.ptr_of = b, ptr
        self.f, self.mol_ptr = b["f"].cuda(), torch.from_numpy(b["ptr"].astype(np.int32)).cuda()
        self.fixed = b["fixed"].to(torch.uint8).cuda()
        self.e_keep = b["e_keep"].cuda()
        self.state = torch.tensor([stale, STEP], dtype=torch.int32).cuda()
        i32 = torch.int32
        init = dict(pos=b["pos"], vel=b["v"], dt=b["st"]["dt"].float(), alpha=b["st"]["alpha"].float(), n_pos=b["st"]["n_pos"].to(i32),
                    status=b["st"]["status"].to(i32), converged_at=b["st"]["converged_at"].to(i32),
                    coef=torch.full((b["n_mol"], 4), GUARD) if coef is None else coef.float(),
                    log=torch.full((LOG_LEN, b["n_mol"], 2), GUARD))
        self.init, self.view, self.whole = init, {}, {}
        for k, t in init.items():
            self.view[k], self.whole[k] = _guarded(t, GUARD if t.dtype.is_floating_point else 7)

    def plan(self):
        from gotennet_amd._lib import call
        p, v, b = self.ptr_of, self.view, self.b
        call("gn_fire_plan", p(self.f), p(v["vel"]), p(self.fixed), p(self.mol_ptr), b["N"], b["n_mol"], P["fmax"], P["dt_max"],
             P["n_min"], P["f_inc"], P["f_dec"], P["alpha"], P["f_alpha"], p(v["dt"]), p(v["alpha"]), p(v["n_pos"]), p(v["status"]),
             p(v["converged_at"]), p(v["coef"]), p(self.e_keep), p(v["log"]), LOG_LEN, p(self.state), _stream())
        torch.cuda.synchronize()

    def move(self):
        from gotennet_amd._lib import call
        p, v, b = self.ptr_of, self.view, self.b
        call("gn_fire_move", p(v["pos"]), p(v["vel"]), p(self.f), p(self.fixed), p(self.mol_ptr), b["N"], b["n_mol"], p(v["coef"]),
             P["max_step"], p(self.state), _stream())
        torch.cuda.synchronize()

    def untouched(self, *names):
        for k in names or self.init:
            a, b = self.view[k].cpu(), self.init[k]
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b), k

    def guards(self):
        for k, w in self.whole.items():
            assert _guards_intact(w, GUARD if w.dtype.is_floating_point else 7), f"a guard word of {k} was written"


def _within(dev, ref, ulps, what):
    """|dev - ref| <= ulps * ulp(ref), element-wise (NaN matches NaN)."""
    dev, ref = dev.double().cpu().reshape(-1), ref.double().reshape(-1)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(dev), nan), what
    err, bound = (dev - ref).abs()[~nan], ulps * _ulp(ref[~nan])
    worst = float((err / _ulp(ref[~nan])).max()) if err.numel() else 0.0
    print(f"{what}: worst {worst:.2f} ulp (bound {ulps})")
    assert bool((err <= bound).all()), f"{what}: {worst:.2f} ulp"


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no_mask"])
def test_fmax(masked):
    from gotennet_amd._lib import call, ptr
    b = _batch()
    d = _Device()
    out, whole = _guarded(torch.full((b["n_mol"],), GUARD))
    call("gn_fire_fmax", ptr(d.f), ptr(d.fixed) if masked else None, ptr(d.mol_ptr), b["N"], b["n_mol"], ptr(out), _stream())
    torch.cuda.synchronize()
    free = ~b["fixed"] if masked else torch.ones(b["N"], dtype=torch.bool)
    want = torch.tensor([float(_f2_emulated(b["f"][s], free[s])[1]) for s in b["sl"]], dtype=torch.float32)
    got = out.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(got)[NAN])
    assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), (got, want)     # bit for bit
    assert float(got[EMPTY]) == 0.0 and float(got[ZERO]) == 0.0 and float(got[EQUAL]) == 0.25
    assert float(got[MASKED]) == (9.0 if not masked else float(want[MASKED])) and (masked or float(got[MASK_CONVERGES]) == 3.0)
    if masked:
        _within(got, b["info"]["fmax"], 3, "fmax against fp64")
    assert _guards_intact(whole)


def test_plan():
    b = _batch()
    d = _Device()
    d.plan()
    st1, info, v = b["st1"], b["info"], d.view
    # the integers: exact
    assert v["n_pos"].cpu().tolist() == st1["n_pos"].tolist()
    assert v["status"].cpu().tolist() == st1["status"].tolist()
    assert v["converged_at"].cpu().tolist() == st1["converged_at"].tolist()
    _within(v["dt"], st1["dt"], 1, "dt")
    _within(v["alpha"], st1["alpha"], 1, "alpha")
    assert float(v["dt"].cpu()[CAPPED]) == P["dt_max"]
    coef = v["coef"].cpu()
    active = info["coef"][:, 3] == 1.0
    assert coef[:, 3].tolist() == info["coef"][:, 3].tolist()
    _within(coef[active][:, :3], info["coef"][active][:, :3], 1, "coef")
    assert torch.equal(coef[active][:, 2], v["dt"].cpu()[active])                         # the move's dt is the stored one
    assert bool((coef[~active][:, :3] == GUARD).all())                                    # a molecule that does not move writes no coefficient
    # a molecule that was done before is not touched, whatever its forces say
    for k in ("dt", "alpha", "n_pos", "status", "converged_at"):
        assert v[k].cpu()[DONE] == d.init[k][DONE], k
    # the log: row STEP % LOG_LEN only, (kept energy, largest force) of EVERY molecule
    log = v["log"].cpu()
    row = STEP % LOG_LEN
    assert bool((log[[r for r in range(LOG_LEN) if r != row]] == GUARD).all())
    assert torch.equal(log[row, :, 0], b["e_keep"])
    want = torch.tensor([float(_f2_emulated(b["f"][s], ~b["fixed"][s])[1]) for s in b["sl"]], dtype=torch.float32)
    assert torch.equal(torch.nan_to_num(log[row, :, 1], nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    _within(log[row, :, 1], info["fmax"], 3, "logged fmax against fp64")
    d.untouched("pos", "vel")
    d.guards()


def test_move():
    b = _batch()
    coef = b["info"]["coef"].float()                   # the plan's coefficients, rounded once: an INPUT of this kernel
    d = _Device(coef=coef)
    d.move()
    pos1, vel1, _, info = FU.fire_step(b["pos"], b["v"], b["f"], b["ptr"].tolist(), b["st"], P, fixed=b["fixed"], coef=coef.double())
    vel, pos = d.view["vel"].cpu(), d.view["pos"].cpu()
    # who must not move: molecules that are not active, and fixed atoms -- to the bit
    still = b["fixed"].clone()
    for m, s in enumerate(b["sl"]):
        if float(coef[m, 3]) == 0.0:
            still[s] = True
    assert torch.equal(vel[still], b["v"][still]) and torch.equal(pos[still], b["pos"][still])
    assert int(still.sum()) > 20 and not torch.equal(pos[~still], b["pos"][~still])
    atom_mol = torch.repeat_interleave(torch.arange(b["n_mol"]), torch.tensor(SIZES))
    c = coef.double()[atom_mol]                        # per atom
    f64, v64 = b["f"].double(), b["v"].double()
    big_v = torch.maximum(torch.maximum((c[:, 0:1] * v64).abs(), (c[:, 1:2] * f64).abs()), (c[:, 2:3] * f64).abs())
    err = (vel.double() - vel1).abs()[~still]
    bound = 4 * _ulp(big_v[~still])
    print(f"vel: worst {float((err / _ulp(big_v[~still])).max()):.2f} ulp of the largest term (bound 4)")
    assert bool((err <= bound).all())
    # pos: the expression evaluated in fp64 on the kernel's own velocities
    pos2 = b["pos"].double().clone()
    for m, s in enumerate(b["sl"]):
        if float(coef[m, 3]) == 0.0:
            continue
        free = ~b["fixed"][s]
        dr = float(coef[m, 2]) * vel[s].double()
        n2 = float((dr[free] ** 2).sum())
        scale = min(1.0, P["max_step"] / math.sqrt(n2)) if n2 > 0 else 1.0
        assert abs(scale - float(info["scale"][m])) <= 1e-6 * scale                      # (the clamp decides the same way)
        pos2[s] = torch.where(free.unsqueeze(1), pos2[s] + scale * dr, pos2[s])
        if scale < 1.0:                                                                  # the displacement of the whole molecule is max_step
            assert abs(float((pos[s].double() - b["pos"][s].double()).norm()) - P["max_step"]) < 1e-5
    big = torch.maximum(b["pos"].double().abs(), (pos2 - b["pos"].double()).abs())
    err = (pos.double() - pos2).abs()[~still]
    print(f"pos: worst {float((err / _ulp(big[~still])).max()):.2f} ulp of the largest term (bound 4)")
    assert bool((err <= 4 * _ulp(big[~still])).all())
    # and the whole step against the emulation: the velocity's bound carried through dt (and, through the clamp, into scale: a
    # relative 1e-7 of the displacement, another 4 ulps at most) on top
    total = 8 * _ulp(big) + c[:, 2:3].abs() * 4 * _ulp(big_v)
    assert bool(((pos.double() - pos1).abs() <= total)[~still].all())
    d.untouched("dt", "alpha", "n_pos", "status", "converged_at", "coef", "log")
    d.guards()


def test_a_set_sticky_word_freezes_plan_and_move():
    b = _batch()
    d = _Device(stale=1, coef=b["info"]["coef"].float())
    d.plan()
    d.move()
    d.untouched()
    d.guards()
    assert d.state.cpu().tolist() == [1, STEP]


@pytest.mark.parametrize("stale", [0, 1])
def test_finish(stale):
    from gotennet_amd._lib import call, ptr
    b = _batch()
    N, n_mol = b["N"], b["n_mol"]
    g = torch.Generator().manual_seed(8)
    status = torch.tensor([1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 1, 1], dtype=torch.int32)
    batch = torch.repeat_interleave(torch.arange(n_mol), torch.tensor(SIZES))
    new = dict(force=torch.randn((N, 3), generator=g), energy=torch.randn(n_mol, generator=g), stress=torch.randn((n_mol, 3, 3), generator=g))
    old = dict(force=torch.randn((N, 3), generator=g), energy=torch.randn(n_mol, generator=g), stress=torch.randn((n_mol, 3, 3), generator=g))
    keep = {k: _guarded(t) for k, t in old.items()}
    state = torch.tensor([stale, STEP], dtype=torch.int32).cuda()
    dev = {k: t.cuda() for k, t in new.items()}
    status_d, batch_d = status.cuda(), batch.cuda()
    call("gn_fire_finish", ptr(state), ptr(status_d), ptr(batch_d), ptr(dev["force"]), ptr(keep["force"][0]), N,
         ptr(dev["energy"]), ptr(keep["energy"][0]), ptr(dev["stress"]), ptr(keep["stress"][0]), n_mol, _stream())
    # without a stress
    f2, w2 = _guarded(old["force"])
    e2, _ = _guarded(old["energy"])
    state2 = state.clone() if stale else torch.tensor([0, STEP], dtype=torch.int32).cuda()
    call("gn_fire_finish", ptr(state2), ptr(status_d), ptr(batch_d), ptr(dev["force"]), ptr(f2), N, ptr(dev["energy"]), ptr(e2),
         None, None, n_mol, _stream())
    torch.cuda.synchronize()
    assert state.cpu().tolist() == state2.cpu().tolist() == ([1, STEP] if stale else [0, STEP + 1])
    act = (status == 0) & (stale == 0)
    want = dict(force=torch.where(act[batch].unsqueeze(1), new["force"], old["force"]), energy=torch.where(act, new["energy"], old["energy"]),
                stress=torch.where(act.reshape(-1, 1, 1), new["stress"], old["stress"]))
    for k in want:
        assert torch.equal(keep[k][0].cpu(), want[k]), k
        assert _guards_intact(keep[k][1]), k
    assert torch.equal(f2.cpu(), want["force"]) and torch.equal(e2.cpu(), want["energy"]) and _guards_intact(w2)
    assert stale or (not torch.equal(want["force"], old["force"]) and not torch.equal(want["force"], new["force"]))
