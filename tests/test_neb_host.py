"""CPU: the nudged elastic band -- the fp64 yardstick of tests/neb_util.py finding the saddle of an analytic surface (with and
without a climbing image), its rules one by one, what ``NEB`` refuses before any launch, the two gn_neb_* entry points in the
header and the ctypes table, the public surface, and the conditions on the input of the GPU run test (the fp64 reference
run: its decisions and tangent branches must not sit on a threshold)."""
import functools
import inspect
import math
import os
import re
import types

import pytest
import torch

from tests import fire_util as FU
from tests import neb_util as NU
from tests import pbc_util as U


# ------------------------------------------------------------------------------------------------ the analytic surface
def _surface(pos):
    """V = (x^2 - 1)^2 + 2 (y - (1 - x^2) / 2)^2 + 2 z^2 on one-atom images: minima at (+-1, 0, 0) with V = 0, the saddle at
    (0, 1/2, 0) with V = 1 and curvatures -4 (along x) and +4 (y, z).  -> (energy [n], forces [n, 3]) in fp64."""
    q = pos.clone().requires_grad_(True)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    v = (x * x - 1.0) ** 2 + 2.0 * (y - 0.5 * (1.0 - x * x)) ** 2 + 2.0 * z * z
    return v.detach(), -torch.autograd.grad(v.sum(), q)[0]


SURFACE_FMAX, SURFACE_K = 0.01, 0.1


@functools.lru_cache(maxsize=None)
def _surface_run(n_img, climb):
    """A straight start between the minima, the interior images lifted by z = 0.05; FIRE's defaults, fmax = 0.01, k = 0.1."""
    pos = torch.zeros((n_img, 3), dtype=torch.float64)
    pos[:, 0] = torch.linspace(-1.0, 1.0, n_img, dtype=torch.float64)
    pos[1:-1, 2] = 0.05
    out = NU.neb_run(_surface, pos, list(range(n_img + 1)), n_img, SURFACE_K, climb, 1000, dict(FU.DEFAULTS, fmax=SURFACE_FMAX))
    return out, pos


def test_the_saddle_surface_is_what_it_says():
    e, f = _surface(torch.tensor([[-1.0, 0, 0], [1.0, 0, 0], [0.0, 0.5, 0]], dtype=torch.float64))
    assert e.tolist() == [0.0, 0.0, 1.0] and float(f.abs().max()) == 0.0
    q = torch.tensor([[0.0, 0.5, 0.0]], dtype=torch.float64, requires_grad=True)
    hess = torch.autograd.functional.hessian(lambda p: ((p[:, 0] ** 2 - 1) ** 2 + 2 * (p[:, 1] - 0.5 * (1 - p[:, 0] ** 2)) ** 2
                                                        + 2 * p[:, 2] ** 2).sum(), q).reshape(3, 3)
    assert torch.equal(hess, torch.diag(torch.tensor([-4.0, 4.0, 4.0], dtype=torch.float64)))


@pytest.mark.parametrize("n_img", [4, 6])
def test_the_climbing_image_finds_the_saddle(n_img):
    """An even number of images puts none on the saddle by symmetry.  Converged, |g| <= fmax on the climbing image, and a
    reflection keeps |g| = |f|; near a saddle with curvatures of magnitude 4, |V - 1| <= |f|^2 / (2 * 4) = fmax^2 / 8."""
    out, start = _surface_run(n_img, True)
    assert out["state"]["status"].tolist() == [1] and 0 < out["steps"] < 1000
    ci = int(out["history"][-1]["info"]["climb"][0])
    top = float(out["energy"][ci])
    print(f"{n_img} images, climbing: image {ci} at V = {top:.7f} (|V - 1| = {abs(top - 1):.2e}) after {out['steps']} steps")
    assert top == float(out["energy"].max()) and abs(top - 1.0) <= SURFACE_FMAX ** 2 / 8
    assert float(out["forces"][ci].norm()) <= SURFACE_FMAX * (1 + 1e-12)
    # the end images have not moved, the others have
    assert torch.equal(out["pos"][0], start[0]) and torch.equal(out["pos"][-1], start[-1])
    assert not bool((out["pos"][1:-1] == start[1:-1]).all(1).any())
    # without the climbing image the same band converges below the saddle
    plain, _ = _surface_run(n_img, False)
    low = float(plain["energy"].max())
    print(f"{n_img} images, plain: the highest image at V = {low:.4f} after {plain['steps']} steps")
    assert plain["state"]["status"].tolist() == [1] and low < 0.95


@pytest.mark.parametrize("n_img", [3, 5, 7])
@pytest.mark.parametrize("climb", [False, True])
def test_odd_bands_converge(n_img, climb):
    out, start = _surface_run(n_img, climb)
    assert out["state"]["status"].tolist() == [1] and 0 < out["steps"] < 1000
    g, _, _ = NU.neb_forces(out["pos"], out["forces"], out["energy"], list(range(n_img + 1)), n_img, SURFACE_K, climb)
    assert float(g.norm(dim=1).max()) <= SURFACE_FMAX
    mid = out["pos"][n_img // 2]                      # by symmetry the middle image sits on x = 0; it relaxes onto the saddle
    assert abs(float(mid[0])) < 1e-9 and abs(float(out["energy"].max()) - 1.0) <= SURFACE_FMAX ** 2 / 8


# ------------------------------------------------------------------------------------------------------------ the rules
def _band3(energy, k=0.3, climb=False, fixed=None, pos=None, dtype=torch.float32):
    """One band of 3 images with 2 atoms each and hand-made numbers -> (g of the middle image's two atoms, the whole output,
    t+, t-, f), everything about the middle image over the atoms that are not fixed."""
    if pos is None:
        pos = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, 0.1, 0.0], [1.2, 0.3, 0.1], [0.4, 0.5, 0.2], [1.9, 0.2, -0.3]],
                           dtype=torch.float64)
    force = torch.tensor([[9.0, 9, 9], [9, 9, 9], [0.5, -0.2, 0.1], [-0.3, 0.4, 0.2], [9, 9, 9], [9, 9, 9]], dtype=torch.float64)
    out = NU.neb_forces(pos, force, torch.tensor(energy, dtype=dtype), [0, 2, 4, 6], 3, k, climb, fixed, detail=True)
    free = torch.ones(2, dtype=torch.bool) if fixed is None else ~fixed[2:4].bool()
    return out[0][2:4], out, (pos[4:6] - pos[2:4])[free], (pos[2:4] - pos[0:2])[free], force[2:4][free]


def _by_hand(t, tp, tm, f, k, climbing=False):
    """g from the tangent t written out: normalise, project, add the spring."""
    that = t / t.norm()
    along = (f * that).sum()
    return f - 2 * along * that if climbing else f - along * that + k * (tp.norm() - tm.norm()) * that


@pytest.mark.parametrize("energy,mix", [([0.0, 1.0, 2.0], (1.0, 0.0)),        # a rise: t+
                                        ([2.0, 1.0, 0.0], (0.0, 1.0)),        # a fall: t-
                                        ([0.0, 2.0, 1.0], (2.0, 1.0)),        # a maximum, E+ > E-: dmax t+ + dmin t-
                                        ([1.0, 2.0, 0.0], (1.0, 2.0)),        # a maximum, E+ < E-: dmin t+ + dmax t-
                                        ([2.0, 0.0, 1.0], (1.0, 2.0)),        # a minimum, E+ < E-: dmin t+ + dmax t-
                                        ([1.0, 0.0, 2.5], (2.5, 1.0)),        # a minimum, E+ > E-: dmax t+ + dmin t-
                                        ([1.0, 3.0, 1.0], (2.0, 2.0)),        # the tie E+ == E-: the "else" side (dmin = dmax here)
                                        ([0.0, 1.0, 1.0], (1.0, 0.0)),        # the tie E == E+ is no rise: dmax = |E- - E|, E+ > E-
                                        ([1.0, 1.0, 0.0], (0.0, 1.0))])       # the tie E == E- is no fall: dmax = |E+ - E|, E+ < E-
def test_every_tangent_branch(energy, mix):
    """``mix`` = (c+, c-) of t = c+ t+ + c- t-, worked out by hand from the rule."""
    g, out, tp, tm, f = _band3(energy)
    t = mix[0] * tp + mix[1] * tm
    assert float((g - _by_hand(t, tp, tm, f, 0.3)).abs().max()) <= 1e-14
    # the perpendicular part of f is kept, the parallel part is the spring's
    that = t / t.norm()
    assert abs(float((g * that).sum()) - 0.3 * float(tp.norm() - tm.norm())) <= 1e-14
    assert float(((g - f) - ((g - f) * that).sum() * that).abs().max()) <= 1e-14
    assert out[1].tolist() == [max(energy)] and out[2].tolist() == [-1]


def test_coincident_images_not_finite_energies_fixed_atoms_and_zero_rows():
    # |t| = 0: all three images in one place -> g = f, bit for bit
    same = torch.tensor([[0.0, 0, 0], [1, 0, 0]] * 3, dtype=torch.float64)
    g, out, _, _, f = _band3([0.0, 1.0, 2.0], pos=same)
    assert torch.equal(g, f) and out[3]["branch"][2:4].tolist() == [5.0, 5.0]
    # an energy that is not finite, in each of the three places -> NaN on the free rows of the middle image, zeros elsewhere
    for energy in ([float("nan"), 1.0, 2.0], [0.0, float("inf"), 2.0], [0.0, 1.0, -float("inf")]):
        g, out, _, _, _ = _band3(energy)
        assert bool(torch.isnan(g).all()) and bool((out[0][:2] == 0).all()) and bool((out[0][4:] == 0).all())
    assert math.isnan(float(_band3([float("nan"), 1.0, 2.0])[1][1][0]))             # a NaN wins the band's largest energy
    assert float(_band3([0.0, float("inf"), 2.0])[1][1][0]) == float("inf")
    # a fixed atom: its row is exactly zero and it is left out of every sum -- the other atom sees a one-atom band
    fixed = torch.tensor([0, 1, 0, 1, 0, 1], dtype=torch.uint8)
    g, out, tp, tm, f = _band3([0.0, 2.0, 1.0], fixed=fixed)
    assert tp.shape == (1, 3) and bool((g[1] == 0).all())
    assert float((g[0] - _by_hand(2.0 * tp + 1.0 * tm, tp, tm, f, 0.3)[0]).abs().max()) <= 1e-14
    g_free, _, tp2, tm2, f2 = _band3([0.0, 2.0, 1.0])
    assert float((g_free[0] - g[0]).abs().max()) > 1e-3                            # the sums did change
    # end images: exactly zero
    assert bool((out[0][:2] == 0).all()) and bool((out[0][4:] == 0).all())


def test_the_climbing_image_is_the_first_of_equal_maxima():
    n_img, n = 6, 1
    pos = torch.tensor([[float(i), 0.1 * i * i, 0.0] for i in range(n_img)], dtype=torch.float64)
    force = torch.tensor([[0.3, -0.2, 0.1]] * n_img, dtype=torch.float64)
    mol_ptr = list(range(n_img + 1))
    energy = torch.tensor([0.0, 1.0, 3.0, 3.0, 2.0, 5.0])           # the end image's 5 does not count; 3 twice: the first
    g, e_band, ci, info = NU.neb_forces(pos, force, energy, mol_ptr, n_img, 0.3, True, detail=True)
    assert ci.tolist() == [2] and e_band.tolist() == [5.0]
    assert info["branch"].tolist() == [0.0, 1.0, 13.0, 4.0, 3.0, 0.0]         # (1, 3, 3) and (3, 3, 2) are ties: the mix
    # image 2 climbs: E = (1, 3, 3) is the tie E == E+, t = dmax t+ + dmin t- = 2 t+ + 0 t-; reflected, no spring
    tp, tm = pos[3:4] - pos[2:3], pos[2:3] - pos[1:2]
    assert float((g[2] - _by_hand(2.0 * tp, tp, tm, force[2:3], 0.3, climbing=True)[0]).abs().max()) <= 1e-14
    assert abs(float(g[2].norm()) - float(force[2].norm())) <= 1e-14           # a reflection keeps the length
    # image 3, E = (3, 3, 2), the tie E == E-: t = dmin t+ + dmax t- = 0 t+ + 1 t-; ordinary, with its spring
    tp, tm = pos[4:5] - pos[3:4], pos[3:4] - pos[2:3]
    assert float((g[3] - _by_hand(tm, tp, tm, force[3:4], 0.3)[0]).abs().max()) <= 1e-14
    # without climb nobody climbs
    assert NU.neb_forces(pos, force, energy, mol_ptr, n_img, 0.3, False)[2].tolist() == [-1]
    # two bands: each its own
    two = NU.neb_forces(torch.cat([pos, pos]), torch.cat([force, force]), torch.cat([energy, energy.flip(0)]),
                        list(range(2 * n_img + 1)), n_img, 0.3, True)
    assert two[2].tolist() == [2, 2] and two[1].tolist() == [5.0, 5.0]          # flipped: (5, 2, 3, 3, 1, 0) -> image 2 again


def test_neb_step_is_fire_on_the_band():
    """One step from rest: every free atom of a band moves by dt^2 g, the band's largest |g| is judged against fmax, and a
    band below it freezes while the other goes on."""
    n_img = 3
    pos = torch.tensor([[0.0, 0, 0], [1.0, 0.2, 0], [2.0, 0, 0], [0.0, 0, 0], [1.0, 0.1, 0], [2.0, 0, 0]], dtype=torch.float64)
    force = torch.tensor([[1.0, 1, 1], [0.0, 0.4, 0.0], [1, 1, 1], [1, 1, 1], [0.0, 0.02, 0.0], [1, 1, 1]], dtype=torch.float64)
    energy = torch.tensor([0.0, 1.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float64)
    p = dict(FU.DEFAULTS, fmax=0.05)
    pos1, vel1, st, info = NU.neb_step(pos, torch.zeros_like(pos), force, energy, list(range(7)), n_img, 0.0, False,
                                       FU.new_state(2, p), p)
    assert st["status"].tolist() == [0, 1] and st["converged_at"].tolist() == [-1, 0]
    assert torch.equal(pos1[[0, 2, 3, 4, 5]], pos[[0, 2, 3, 4, 5]])
    assert float((pos1[1] - pos[1] - 0.01 * info["g"][1]).abs().max()) <= 1e-16 and float(info["g"][1].norm()) > 0.05
    assert NU.band_ptr(list(range(7)), 3) == [0, 3, 6]
    assert NU.band_fixed([0, 2, 4, 6], 3).tolist() == [True, True, False, False, True, True]


# -------------------------------------------------------------------------------------------------------------- refusals
def _no_launch(fn, match):
    """``fn()`` raises a ``ValueError`` matching ``match`` before any entry point of the library is called."""
    from gotennet_amd import _lib

    def no_call(name, args):
        raise AssertionError(f"{name} was called before the refusal")

    old = _lib.TIMER
    _lib.TIMER = types.SimpleNamespace(want=no_call, events=[])
    try:
        with pytest.raises(ValueError, match=match):
            fn()
    finally:
        _lib.TIMER = old


def _make(**kw):
    from gotennet_amd import NEB
    ef = types.SimpleNamespace(rep=types.SimpleNamespace(cutoff=5.0), head=None)
    base = dict(z=torch.tensor([8, 1, 8, 1, 8, 1]), pos=torch.zeros((6, 3)), batch=torch.tensor([0, 0, 1, 1, 2, 2]), n_mol=3,
                n_images=3)
    base.update(kw)
    return NEB(ef, **base)


def test_refusals_come_before_any_launch():
    nan, inf = float("nan"), float("inf")
    _no_launch(lambda: _make(n_images=2, n_mol=2, batch=torch.tensor([0, 0, 0, 1, 1, 1])), "n_images")
    _no_launch(lambda: _make(n_images=1), "n_images")
    _no_launch(lambda: _make(n_images=4), "multiple")
    _no_launch(lambda: _make(n_images=7), "multiple")
    _no_launch(lambda: _make(batch=torch.tensor([0, 0, 0, 1, 2, 2])), "atoms")                 # atom counts differ
    _no_launch(lambda: _make(batch=torch.tensor([0, 0, 0, 0, 2, 2])), "atoms")                 # an empty image among full ones
    _no_launch(lambda: _make(z=torch.tensor([8, 1, 8, 1, 1, 8])), "atomic numbers")            # the same atoms, another order
    _no_launch(lambda: _make(z=torch.tensor([8, 1, 8, 6, 8, 1])), "atomic numbers")
    for bad in (-0.1, nan, inf, -inf):
        _no_launch(lambda: _make(k=bad), "spring")
    _no_launch(lambda: _make(fixed=torch.tensor([1, 0, 1, 0, 0, 1], dtype=torch.uint8)), "fixed mask")
    _no_launch(lambda: _make(fixed=torch.tensor([True, False, True, False, False, False])), "fixed mask")
    # Relax's own still hold
    _no_launch(lambda: _make(fmax=-0.01), "fmax")
    _no_launch(lambda: _make(max_step=0.0), "max_step")
    _no_launch(lambda: _make(fixed=torch.zeros(4, dtype=torch.bool)), "fixed")
    _no_launch(lambda: _make(fixed=torch.zeros(6, dtype=torch.int64)), "fixed")
    _no_launch(lambda: _make(pos=torch.zeros((6, 3), requires_grad=True)), "pos requires grad")
    _no_launch(lambda: _make(cell=torch.eye(3) * 9.0), "2 \\* cutoff")
    _no_launch(lambda: _make(images="some", cell=torch.eye(3) * 12.0), "images")
    _no_launch(lambda: _make(rebuild="gpu"), "rebuild")
    _no_launch(lambda: _make(check_every=0), "check_every")


def test_band_interpolates_in_fp64_and_tiles():
    from gotennet_amd import neb
    s = NU.band_start()
    z, pos, batch, n_mol = neb.band(s["z_ab"], s["pos_first"], s["pos_last"], s["batch_ab"], 2, n_images=NU.REF_N_IMG)
    assert n_mol == s["n_mol"] == 10 and pos.dtype == torch.float32
    assert torch.equal(pos, s["pos"]) and torch.equal(z, s["z"]) and torch.equal(batch, s["batch"])
    # the end images are the end points, bit for bit; image i of n is the fp64 interpolation rounded once
    assert torch.equal(pos[batch == 0], s["pos_first"][:3]) and torch.equal(pos[batch == 9], s["pos_last"][3:])
    a, b = s["pos_first"][:3].double(), s["pos_last"][:3].double()
    assert torch.equal(pos[batch == 3], (a + 0.75 * (b - a)).float())
    with pytest.raises(ValueError, match="n_images"):
        neb.band(s["z_ab"], s["pos_first"], s["pos_last"], s["batch_ab"], 2, n_images=2)
    with pytest.raises(ValueError, match="expected"):
        neb.band(s["z_ab"], s["pos_first"], s["pos_last"][:5], s["batch_ab"], 2)


# ---------------------------------------------------------------------------------------------------------- entry points
NEB_ENTRIES = {"gn_neb_forces": 15, "gn_neb_finish": 13}


def test_entry_points_in_header_and_ctypes_table(repo_root):
    from gotennet_amd import _lib
    header = open(os.path.join(repo_root, "include", "gotennet_hip.h")).read()
    src = open(os.path.join(repo_root, "gotennet_amd", "csrc", "gn_neb.hip")).read()
    for name, n_args in NEB_ENTRIES.items():
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/gotennet_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]) == n_args, name
        assert re.search(r'extern "C" int ' + name + r"\(", src), name
    C = _lib.C
    assert _lib.SIGNATURES["gn_neb_forces"] == ([C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_double, C.c_int] + [C.c_void_p] * 5)
    assert _lib.SIGNATURES["gn_neb_finish"] == [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p]
    declared = set(re.findall(r"^(?:int|long) (gn_\w+)\(", header, flags=re.M))
    assert {n for n in declared if n.startswith("gn_neb_")} == set(NEB_ENTRIES)
    assert {n for n in _lib.SIGNATURES if n.startswith("gn_neb_")} == set(NEB_ENTRIES)
    fire = {"gn_fire_fmax", "gn_fire_plan", "gn_fire_move", "gn_fire_finish"}
    assert {n for n in declared if n.startswith("gn_fire_")} == fire == {n for n in _lib.SIGNATURES if n.startswith("gn_fire_")}
    assert _lib.ABI_VERSION == 11 and "#define GN_ABI_VERSION 11" in header      # additive entries: the ABI number stays
    assert "atomic" not in src.lower()


# --------------------------------------------------------------------------------------------------------------- surface
def test_public_surface_and_defaults():
    import gotennet_amd
    from gotennet_amd import md, neb, relax
    assert gotennet_amd.NEB is neb.NEB and issubclass(neb.NEB, relax.Relax) and not issubclass(neb.NEB, relax.CellRelax)
    p = inspect.signature(neb.NEB.__init__).parameters
    base = inspect.signature(relax.Relax.__init__).parameters
    assert list(p)[:6] == list(base)[:6] and list(p)[6:9] == ["n_images", "k", "climb"] and list(p)[9:] == list(base)[6:]
    assert [p[k].default for k in ("n_images", "k", "climb")] == [7, 0.1, False]
    for k in list(base)[6:]:
        assert p[k].default == base[k].default, k
    assert "rebuild" not in p and isinstance(neb.NEB, md._RebuildOption)
    for name in ("pos", "forces", "neb_forces", "potential_energy", "barrier", "climbing_image", "fmax", "status", "converged",
                 "converged_at", "step", "stress", "vel"):
        assert isinstance(getattr(neb.NEB, name), property), name
    assert callable(neb.NEB.run) and callable(neb.NEB.log) and callable(neb.band)
    # the step goes through _pre and _post only: no second loop, recorder or list handling
    for name in ("run", "_advance", "_record", "_repair", "_stuck", "_list", "_verify", "_ring", "log", "step", "forces", "pos"):
        assert name not in vars(neb.NEB), name
    assert "_pre" in vars(neb.NEB) and "_post" in vars(neb.NEB)
    src = inspect.getsource(neb)
    assert "CUDAGraph" not in src and ".replay(" not in src and src.count('"gn_fire_finish"') == 0
    doc = neb.NEB.__doc__
    for word in ("never wraps positions", "continuous", "IDPP", "rotation and translation", "variable springs", "moving cell",
                 "end images"):
        assert word in doc, word


# ------------------------------------------------------------------------- the input of the GPU run test (fp64 reference)
ENERGY_MARGIN = 1e-4        # two energies that are compared differ by at least this: a hundred fp32 ulps of an energy of 1 to 2


def test_the_band_reference_run_is_a_fair_input():
    r = NU.band_reference()
    h, n_img, p = r["history"], NU.REF_N_IMG, r["params"]
    assert len(h) == r["steps"] == NU.REF_STEPS == 16 and p["fmax"] == NU.REF_FMAX
    assert r["state"]["status"].tolist() == [0, 0]
    # no pair distance within MIN_GAP of the cutoff at any step: an fp32 rounding cannot change a list
    assert r["gap"] > U.MIN_GAP, r["gap"]
    print("edge counts", sorted(set(r["edges"])), "gap", r["gap"])
    kept_e = [r["e0"]] + [s["energy"] for s in h]
    branches, climbers, margin = set(), set(), float("inf")
    for k, step in enumerate(h):
        info, e = step["info"], kept_e[k].reshape(2, n_img)         # the energies step k was judged on
        for b in range(2):
            # every decision on the sign of P is far from zero; every decision on fmax is at least 10 % off the threshold
            if k > 0:
                assert abs(float(info["P"][b])) >= 0.05 * float(info["absP"][b]), (k, b)
            assert abs(float(info["fmax"][b]) - p["fmax"]) >= 0.1 * p["fmax"], (k, b)
            # every comparison of two energies the tangent rule makes: neighbours, and E+ against E- at an extremum
            for i in range(1, n_img - 1):
                Em, E0, Ep = (float(x) for x in e[b, i - 1:i + 2])
                margin = min(margin, abs(Ep - E0), abs(E0 - Em))
                if not (Ep > E0 > Em or Ep < E0 < Em):
                    margin = min(margin, abs(Ep - Em))
                    branches.add("max" if E0 > Ep else "min")
                else:
                    branches.add("up" if Ep > E0 else "down")
            # the climbing image: the largest interior energy leads the second by the margin
            top = sorted((float(x) for x in e[b, 1:-1]), reverse=True)
            margin = min(margin, top[0] - top[1])
            climbers.add((b, int(info["climb"][b])))
    print(f"smallest energy margin {margin:.3e}; tangent branches {sorted(branches)}; climbing images {sorted(climbers)}")
    assert margin >= ENERGY_MARGIN
    assert {"up", "down", "max"} <= branches and len(climbers) >= 3          # the run visits them, and the climber changes once
    # the end images never move; every interior image does; the energy of the highest image of each band falls
    s = NU.band_start()
    for b, m in ((0, 0), (0, 4), (1, 5), (1, 9)):
        atoms = slice(r["mol_ptr"][m], r["mol_ptr"][m + 1])
        assert torch.equal(r["pos"][atoms], s["pos"][atoms].double())
    for m in (1, 2, 3, 6, 7, 8):
        atoms = slice(r["mol_ptr"][m], r["mol_ptr"][m + 1])
        assert not bool((r["pos"][atoms] == s["pos"][atoms].double()).all(1).any())
    assert math.isfinite(float(r["energy"].sum()))


def test_a_band_below_fmax_freezes_at_step_0_in_the_reference():
    """fmax between the two bands' first largest |g|: band 0 is converged at step 0 and keeps its bits, band 1 goes on."""
    r = NU.band_reference()
    first = r["history"][0]["info"]["fmax"].tolist()
    assert first[0] * 1.5 < NU.FREEZE_FMAX < first[1] / 1.5, first
    out = NU.band_reference(fmax=NU.FREEZE_FMAX, steps=6)
    assert out["state"]["status"].tolist() == [1, 0] and out["state"]["converged_at"].tolist() == [0, -1] and out["steps"] == 6
    s = NU.band_start()
    cut = r["mol_ptr"][NU.REF_N_IMG]
    assert torch.equal(out["pos"][:cut], s["pos"][:cut].double()) and not torch.equal(out["pos"][cut:], s["pos"][cut:].double())
