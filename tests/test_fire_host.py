"""CPU: the relaxation driver's refusals (raised before any library call), its public surface, the ctypes table of the
gn_fire_* entry points, the fp64 emulation of tests/fire_util.py on analytic potentials, and the conditions on the input of
the GPU run test (the fp64 reference run: its decisions must not sit on a threshold)."""
import inspect
import math
import re
import types

import pytest
import torch

from tests import fire_util as FU
from tests import pbc_util as U


def _args(**kw):
    base = dict(z=torch.tensor([8, 1, 1]), pos=torch.zeros((3, 3)), batch=torch.zeros(3, dtype=torch.int64), n_mol=1)
    base.update(kw)
    return base


def _refused(match, **kw):
    """``Relax`` raises ``ValueError`` without touching the library: every entry point is replaced by one that fails."""
    from gotennet_amd import _lib, relax
    ef = types.SimpleNamespace(rep=types.SimpleNamespace(cutoff=5.0), head=None)

    def no_call(name, args):
        raise AssertionError(f"{name} was called before the refusal")

    old = _lib.TIMER
    _lib.TIMER = types.SimpleNamespace(want=no_call, events=[])
    try:
        with pytest.raises(ValueError, match=match):
            relax.Relax(ef, **_args(**kw))
    finally:
        _lib.TIMER = old


def test_refusals_come_before_any_launch():
    nan, inf = float("nan"), float("inf")
    _refused("fmax", fmax=-0.01)
    _refused("fmax", fmax=nan)
    for name in ("dt", "dt_max", "max_step"):
        for bad in (0.0, -1.0, nan, inf):
            _refused(name, **{name: bad})
    _refused("exceeds dt_max", dt=0.5, dt_max=0.25)
    _refused("f_inc", f_inc=0.99)
    for name in ("f_dec", "f_alpha"):
        for bad in (0.0, 1.0, -0.5, 1.5, nan):
            _refused(name, **{name: bad})
    for bad in (0.0, -0.1, 1.01, nan):
        _refused("alpha", alpha=bad)
    _refused("n_min", n_min=-1)
    _refused("fixed", fixed=torch.zeros(4, dtype=torch.bool))                  # shape
    _refused("fixed", fixed=torch.zeros((3, 1), dtype=torch.bool))
    _refused("fixed", fixed=torch.zeros(3, dtype=torch.int64))                 # dtype
    _refused("fixed", fixed=[False, False, True])
    _refused("pos requires grad", pos=torch.zeros((3, 3), requires_grad=True))
    _refused("cell requires grad", cell=(torch.eye(3) * 12.0).requires_grad_())
    _refused("2 \\* cutoff", cell=torch.eye(3) * 9.0)                          # graph.resolve_images' refusals
    _refused("cutoff / 3", cell=torch.eye(3) * 1.0, images="all")
    _refused("images", cell=torch.eye(3) * 12.0, images="some")
    _refused("check_every", check_every=0)


def test_public_surface_and_defaults():
    import gotennet_amd
    from gotennet_amd import md, relax
    assert gotennet_amd.Relax is relax.Relax and issubclass(relax.Relax, md._ListDriver) and issubclass(md.MDRun, md._ListDriver)
    p = inspect.signature(relax.Relax.__init__).parameters
    assert [k for k in p][1:6] == ["ef", "z", "pos", "batch", "n_mol"]
    want = dict(fmax=0.05, dt=0.1, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, fixed=None,
                cell=None, images="minimum", max_num_neighbors=32, check_every=1, log_len=1024, captured=True)
    assert {k: p[k].default for k in want} == want and [k for k in p][6:] == list(want)
    assert {k: FU.DEFAULTS[k] for k in FU.DEFAULTS} == {k: want[k] for k in FU.DEFAULTS}       # the emulation's are the same
    for name in ("pos", "forces", "potential_energy", "stress", "fmax", "converged", "converged_at", "step"):
        assert isinstance(getattr(relax.Relax, name), property), name
    assert callable(relax.Relax.run) and callable(relax.Relax.log)
    # one copy of the shared pieces: neither driver defines them itself
    for name in ("_list", "_verify", "_record", "_repair", "_start", "_ring"):
        assert name not in vars(relax.Relax) and name not in vars(md.MDRun), name
    assert "run" not in vars(md.MDRun)
    doc = relax.Relax.__doc__ + relax.__doc__
    assert "dr = dt^2 f" in doc and "cell is fixed" in doc


FIRE = {"gn_fire_fmax": 7, "gn_fire_plan": 24, "gn_fire_move": 11, "gn_fire_finish": 12}


def test_entry_points_in_header_and_ctypes_table(repo_root):
    import os
    from gotennet_amd import _lib
    header = open(os.path.join(repo_root, "include", "gotennet_hip.h")).read()
    for name, n_args in FIRE.items():
        assert name in _lib.SIGNATURES, name
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/gotennet_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]) == n_args, name
    declared = set(re.findall(r"^(?:int|long) (gn_\w+)\(", header, flags=re.M))
    assert {n for n in declared if n.startswith("gn_fire_")} == set(FIRE)
    assert {n for n in _lib.SIGNATURES if n.startswith("gn_fire_")} == set(FIRE)
    assert _lib.ABI_VERSION == 11 and "#define GN_ABI_VERSION 11" in header      # additive entries: the ABI number stays
    src = open(os.path.join(repo_root, "gotennet_amd", "csrc", "gn_fire.hip")).read()
    for name in FIRE:
        assert re.search(r'extern "C" int ' + name + r"\(", src), name
    assert "atomic" not in src.replace("No atomics", "")


# ------------------------------------------------------------------------------------------------ analytic potentials
def _chain(n, kind):
    """n atoms on a slightly bent line, bonded neighbours only.  harmonic: (k/2) (r - 1)^2, k = 4; Morse: D (1 - exp(-a (r - 1)))^2,
    D = 0.5, a = 1.5.  -> (start positions, energy_forces_fn) in fp64."""
    g = torch.Generator().manual_seed(100 + n)
    pos = torch.stack([torch.arange(n, dtype=torch.float64) * 1.3, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)], 1)
    pos = pos + 0.08 * torch.randn((n, 3), generator=g, dtype=torch.float64)

    def fn(p):
        q = p.clone().requires_grad_(True)
        r = (q[1:] - q[:-1]).norm(dim=1)
        e = (2.0 * (r - 1.0) ** 2).sum() if kind == "harmonic" else (0.5 * (1.0 - torch.exp(-1.5 * (r - 1.0))) ** 2).sum()
        return e.detach().reshape(1), -torch.autograd.grad(e, q)[0]
    return pos, fn


@pytest.mark.parametrize("kind", ["harmonic", "morse"])
@pytest.mark.parametrize("n", [2, 5, 9])
def test_fire_run_relaxes_analytic_chains(n, kind):
    pos, fn = _chain(n, kind)
    e0, f0 = fn(pos)
    assert float(f0.norm(dim=1).max()) > 5 * FU.DEFAULTS["fmax"]           # the start is far from converged
    out = FU.fire_run(fn, pos, [0, n], 400)
    assert out["state"]["status"].tolist() == [1] and 0 < out["steps"] < 400, out["steps"]
    assert out["steps"] == int(out["state"]["converged_at"][0])
    e1, f1 = fn(out["pos"])
    assert float(f1.norm(dim=1).max()) <= FU.DEFAULTS["fmax"] and float(e1) < float(e0)
    assert torch.equal(out["forces"], f1) and torch.equal(out["energy"], e1)      # the kept values are those of the end


def test_fire_step_rules():
    """The emulation against hand-computed numbers: one atom, f = (2, 0, 0)."""
    p = dict(FU.DEFAULTS, fmax=0.05)
    pos, vel, f = torch.zeros((1, 3), dtype=torch.float64), torch.zeros((1, 3), dtype=torch.float64), torch.tensor([[2.0, 0, 0]], dtype=torch.float64)
    st = FU.new_state(1, p)
    pos, vel, st, info = FU.fire_step(pos, vel, f, [0, 1], st, p)                         # first step: v = dt f, dr = dt^2 f
    assert vel[0, 0] == 0.2 and abs(float(pos[0, 0]) - 0.02) < 1e-17 and st["n_pos"].tolist() == [0]
    pos, vel, st, info = FU.fire_step(pos, vel, f, [0, 1], st, p, step=1)                 # downhill: v = 0.9 v + 0.1 |v| f/|f| + dt f
    assert abs(float(vel[0, 0]) - 0.4) < 1e-15 and st["n_pos"].tolist() == [1] and float(st["dt"][0]) == 0.1
    st["n_pos"][0] = 6                                                                    # beyond n_min: dt and alpha move
    _, _, st2, _ = FU.fire_step(pos, vel, f, [0, 1], st, p, step=2)
    assert abs(float(st2["dt"][0]) - 0.11) < 1e-15 and abs(float(st2["alpha"][0]) - 0.099) < 1e-15 and st2["n_pos"].tolist() == [7]
    pos3, vel3, st3, info = FU.fire_step(pos, vel, -f, [0, 1], st, p, step=2)              # uphill: v = 0 + dt f with dt halved
    assert float(st3["dt"][0]) == 0.05 and float(st3["alpha"][0]) == 0.1 and st3["n_pos"].tolist() == [0]
    assert abs(float(vel3[0, 0]) + 0.1) < 1e-15
    big = 100.0 * f                                                                       # the clamp: |dr| = max_step
    pos4, _, _, info = FU.fire_step(pos, vel, big, [0, 1], st, p, step=2)
    assert abs(float((pos4 - pos).norm()) - p["max_step"]) < 1e-15 and float(info["scale"][0]) < 1
    _, _, st5, _ = FU.fire_step(pos, vel, 0.025 * f, [0, 1], st, p, step=9)                # |f| = 0.05 = fmax: converged (<=)
    assert st5["status"].tolist() == [1] and st5["converged_at"].tolist() == [9]
    _, _, st6, _ = FU.fire_step(pos, vel, f * float("nan"), [0, 1], st, p, step=4)
    assert st6["status"].tolist() == [2] and st6["converged_at"].tolist() == [4]
    fixed = torch.tensor([True])
    pos7, _, st7, _ = FU.fire_step(pos, vel, f, [0, 1], st, p, fixed=fixed, step=3)        # all atoms fixed: no force counts
    assert st7["status"].tolist() == [1] and torch.equal(pos7, pos)


# ------------------------------------------------------------------------- the input of the GPU run test (fp64 reference)
REF_CONVERGED_AT, REF_EDGE_COUNTS = FU.REF_CONVERGED_AT, FU.REF_EDGE_COUNTS


def test_the_reference_run_is_a_fair_input():
    r = FU.molecule_reference()
    h = r["history"]
    assert len(h) == FU.REF_STEPS == 24 and r["params"]["fmax"] == 0.06
    assert r["state"]["converged_at"].tolist() == REF_CONVERGED_AT and r["state"]["status"].tolist() == [1, 0, 0]
    counts = [r["edges"][0]] + [b for a, b in zip(r["edges"], r["edges"][1:]) if a != b]
    assert counts == REF_EDGE_COUNTS, r["edges"]
    # no pair distance within MIN_GAP of the cutoff at any step: an fp32 rounding cannot change a list
    assert r["gap"] > U.MIN_GAP, r["gap"]
    # the energy falls in the first step, for every molecule
    drop = r["e0"] - h[0]["energy"]
    print("first-step energy drop", drop.tolist())
    assert bool((drop > 1e-4).all()), drop
    for k, step in enumerate(h):
        info, before = step["info"], (h[k - 1]["state"] if k else FU.new_state(3, r["params"]))
        for m in range(3):
            if int(before["status"][m]) != 0:
                continue
            # every decision on the sign of P is far from zero
            if k > 0 and int(step["state"]["status"][m]) == 0:
                assert abs(float(info["P"][m])) >= 0.05 * float(info["absP"][m]), (k, m)
            # every decision on fmax is at least 10 % away from the threshold
            assert abs(float(info["fmax"][m]) - 0.06) >= 0.1 * 0.06, (k, m, float(info["fmax"][m]))
    k = REF_CONVERGED_AT[0]
    print("molecule 0: fmax", float(h[k - 1]["info"]["fmax"][0]), "->", float(h[k]["info"]["fmax"][0]))
    assert float(h[k]["info"]["fmax"][0]) <= 0.9 * 0.06 < 1.1 * 0.06 <= float(h[k - 1]["info"]["fmax"][0])
    # the frozen molecule stays put while the others go on
    atoms = slice(r["mol_ptr"][0], r["mol_ptr"][1])
    for step in h[k:]:
        assert torch.equal(step["pos"][atoms], h[k - 1]["pos"][atoms]) and torch.equal(step["forces"][atoms], h[k - 1]["forces"][atoms])
    assert not torch.equal(h[-1]["pos"], h[k]["pos"])
    assert math.isfinite(float(r["energy"].sum()))
