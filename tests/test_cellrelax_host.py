"""CPU: variable-cell relaxation -- the generalised forces of tests/cellrelax_util.py against ``torch.autograd`` on a periodic
Morse potential, the fp64 emulation relaxing strained cells, what ``CellRelax`` refuses before any launch, the two
gn_cellrelax_* entry points in the header and the ctypes table, and the public surface."""
import functools
import inspect
import math
import os
import re
import types

import pytest
import torch

from tests import cellrelax_util as CU
from tests import fire_util as FU

PRESSURE = 0.3
C0 = torch.tensor([[2.3, 0.0, 0.0], [0.3, 2.1, 0.0], [-0.2, 0.4, 2.5]], dtype=torch.float64)          # triclinic


# ----------------------------------------------------------------------------------------------------------- the formula
@functools.lru_cache(maxsize=None)
def _formula_case(n):
    """A triclinic box of n atoms with F != 1 (a 5 % random perturbation) and w != n -> everything the checks below share: the
    yardstick's inputs and -dH/d(x~, U) from autograd, H = E + PRESSURE |det cell|."""
    gen = torch.Generator().manual_seed(40 + n)
    F = torch.eye(3, dtype=torch.float64) + 0.05 * torch.randn((3, 3), generator=gen, dtype=torch.float64)
    x = torch.rand((n, 3), generator=gen, dtype=torch.float64) @ C0
    w = torch.tensor([1.7 * n], dtype=torch.float64)
    i, j, img = CU.morse_edges(n)
    X, U = x.clone().requires_grad_(True), (w * F).clone().requires_grad_(True)
    Fv = U / w
    H = CU.morse_energy_of_vectors((X[j] - X[i]) @ Fv + img @ (C0 @ Fv)) + PRESSURE * torch.linalg.det(C0 @ Fv).abs()
    dX, dU = torch.autograd.grad(H, (X, U))
    pos, cell = x @ F, C0 @ F
    _, f, stress = CU.morse_box(pos, cell)
    return dict(F=F, w=w, mol_ptr=[0, n], f=f, stress=stress.reshape(1, 3, 3), cell=cell.reshape(1, 3, 3),
                x_ext=CU.extend(x, [0, n], w, F.reshape(1, 3, 3)), g=-dX, G=-dU)


def _yardstick(c, **kw):
    out = CU.generalised_forces(c["f"], c["stress"], c["cell"], c["x_ext"], c["mol_ptr"], c["w"], pressure=PRESSURE, **kw)
    lay = CU.layout(c["mol_ptr"])
    return out[lay["atom_rows"]], out[lay["cell_rows"][0]]


def _close(got, want, rel=1e-9):
    return float((got - want).abs().max()) <= rel * float(want.abs().max())


@pytest.mark.parametrize("n", [1, 2, 6])
def test_generalised_forces_are_minus_the_gradient_of_the_enthalpy(n):
    c = _formula_case(n)
    g, G = _yardstick(c)
    assert float(c["G"].abs().max()) > 1e-3 and float((c["F"] - torch.eye(3)).abs().max()) > 0.01       # a fair input
    # the stress of a pair potential is symmetric up to rounding; the formula symmetrises it
    assert _close(c["stress"][0], c["stress"][0].T, 1e-12)
    assert _close(G, c["G"]), (G, c["G"])
    if n > 1:
        assert _close(g, c["g"]), (g, c["g"])
    else:                                   # one atom: every force vanishes by symmetry, in the formula and in autograd
        assert float(g.abs().max()) <= 1e-9 * float(c["G"].abs().max()) and float(c["g"].abs().max()) <= 1e-9 * float(c["G"].abs().max())


@pytest.mark.parametrize("n", [1, 2, 6])
def test_hydrostatic_and_masked_generalised_forces(n):
    c = _formula_case(n)
    g_full, _ = _yardstick(c)
    # hydrostatic: F^T (-dH/dU) = -(V / w) S, so G_h = (tr(F^T G) / 3) F^-T: proportional to F^-T, the factor from autograd's G
    g, G = _yardstick(c, hydrostatic=True)
    want = torch.trace(c["F"].T @ c["G"]) / 3.0 * torch.linalg.inv(c["F"]).T
    assert _close(G, want) and torch.equal(g, g_full)
    ratio = G / torch.linalg.inv(c["F"]).T
    assert float((ratio - ratio[0, 0]).abs().max()) <= 1e-9 * abs(float(ratio[0, 0]))
    # a mask: the masked components are exactly 0, the others are the full ones
    mask = torch.tensor([[1, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=torch.uint8)
    g, G = _yardstick(c, cell_mask=mask)
    assert bool((G[~mask.bool()] == 0).all()) and _close(G[mask.bool()], c["G"][mask.bool()]) and torch.equal(g, g_full)
    # a fixed atom: its row counts as zero
    fixed = torch.zeros(n, dtype=torch.bool)
    fixed[0] = True
    g, G2 = _yardstick(c, fixed=fixed)
    assert bool((g[0] == 0).all()) and torch.equal(g[1:], g_full[1:]) and _close(G2, c["G"])


def test_extended_layout():
    lay = CU.layout([0, 2, 2, 5])                                    # boxes of 2, 0 and 3 atoms
    assert lay["mol_ptr_ext"] == [0, 5, 8, 14] and lay["NE"] == 14
    assert lay["atom_rows"].tolist() == [0, 1, 8, 9, 10] and lay["cell_rows"].tolist() == [[2, 3, 4], [5, 6, 7], [11, 12, 13]]
    assert CU.weights([0, 2, 2, 5]).tolist() == [2.0, 1.0, 3.0] and CU.weights([0, 2, 2, 5], 4.0).tolist() == [4.0] * 3
    x = CU.extend(torch.ones((5, 3)), [0, 2, 2, 5], CU.weights([0, 2, 2, 5]))
    assert torch.equal(x[lay["cell_rows"]], torch.tensor([2.0, 1.0, 3.0], dtype=torch.float64).reshape(3, 1, 1) * torch.eye(3, dtype=torch.float64))
    assert CU.extend_fixed(torch.tensor([1, 0, 0, 0, 1]), [0, 2, 2, 5]).nonzero().flatten().tolist() == [0, 10]


# ------------------------------------------------------------------------------------------------- the emulation relaxes
MOL_PTR = [0, 2, 3]
P = dict(FU.DEFAULTS, fmax=0.01)


def _strained():
    """Two boxes: two atoms in a sheared 2 x 1 x 1 simple-cubic cell, one atom in a sheared cube."""
    strain = torch.tensor([[1.04, 0.02, 0.0], [0.0, 0.97, -0.015], [0.01, 0.0, 1.02]], dtype=torch.float64)
    cell = torch.stack([torch.diag(torch.tensor([2.1, 1.05, 1.05], dtype=torch.float64)) @ strain,
                        torch.eye(3, dtype=torch.float64) * 1.08 @ strain.T])
    pos = torch.tensor([[0.03, 0.0, -0.02], [1.09, 0.04, 0.01], [0.2, 0.3, 0.1]], dtype=torch.float64)
    return pos, cell


@functools.lru_cache(maxsize=None)
def _run(kind):
    pos, cell = _strained()
    kw = dict(full={}, pressure=dict(pressure=0.05), hydrostatic=dict(hydrostatic=True),
              mask=dict(cell_mask=torch.tensor([[1, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=torch.uint8)))[kind]
    return CU.relax_run(CU.morse_model(MOL_PTR), pos, cell, MOL_PTR, 400, P, **kw), kw


@pytest.mark.parametrize("kind", ["full", "pressure"])
def test_emulation_relaxes_strained_cells(kind):
    out, kw = _run(kind)
    p = kw.get("pressure", 0.0)
    assert out["state"]["status"].tolist() == [1, 1], out["state"]
    assert 0 < out["steps"] < 400
    V = torch.linalg.det(out["cell"]).abs()
    F = CU.deformation(out["x_ext"], MOL_PTR, out["w"])
    for m in range(2):
        # converged: every cell row of G = -(V / w) F^-T S is at most fmax long, so S = -(w / V) F^T G has
        # |S|_F <= (w / V) |F|_2 sqrt(3) fmax
        S = 0.5 * (out["stress"][m] + out["stress"][m].T) + p * torch.eye(3, dtype=torch.float64)
        bound = float(out["w"][m] / V[m] * torch.linalg.matrix_norm(F[m], 2) * math.sqrt(3.0) * P["fmax"])
        assert float(S.norm()) <= bound, (m, float(S.norm()), bound)
    h = out["history"][-1]["enthalpy"]
    assert bool((h < out["enthalpy0"]).all())
    assert float(out["forces"].norm(dim=1).max()) <= P["fmax"] * float(torch.linalg.matrix_norm(torch.linalg.inv(F), 2).max())
    # the state is consistent: pos = x~ F, cell = C0 F
    _, cell0 = _strained()
    assert torch.allclose(out["cell"], cell0 @ F, rtol=0, atol=1e-14)


def test_emulation_hydrostatic_and_masked():
    _, cell0 = _strained()
    out, _ = _run("hydrostatic")
    assert out["state"]["status"].tolist() == [1, 1]
    for m in range(2):
        s = out["cell"][m][0, 0] / cell0[m][0, 0]
        assert abs(float(s) - 1.0) > 1e-3 and torch.allclose(out["cell"][m], s * cell0[m], rtol=1e-13, atol=0)
    out, kw = _run("mask")
    masked = ~kw["cell_mask"].bool()
    eye = torch.eye(3, dtype=torch.float64)
    assert out["state"]["status"].tolist() == [1, 1]
    for h in out["history"]:
        for m in range(2):
            assert torch.equal(h["F"][m][masked], eye[masked])              # bit-identical to the start
    assert not torch.equal(out["history"][-1]["F"][0][~masked], eye[~masked])


def test_emulation_a_box_below_fmax_freezes_at_step_0():
    """fmax lies between the largest generalised forces of the two boxes at the start: box 1 is converged at step 0 and keeps
    its bits, box 0 goes on."""
    pos, cell = _strained()
    model = CU.morse_model(MOL_PTR)
    _, f, s = model(pos, cell)
    w = CU.weights(MOL_PTR)
    g = CU.generalised_forces(f, s, cell, CU.extend(pos, MOL_PTR, w), MOL_PTR, w)
    lay = CU.layout(MOL_PTR)
    big = [float(g[lay["mol_ptr_ext"][m]:lay["mol_ptr_ext"][m + 1]].norm(dim=1).max()) for m in range(2)]
    assert big[1] * 1.1 < big[0]                                       # the input: room for an fmax in between
    out = CU.relax_run(model, pos, cell, MOL_PTR, 10, dict(FU.DEFAULTS, fmax=0.5 * (big[0] + big[1])))
    assert out["state"]["status"].tolist() == [0, 1] and out["state"]["converged_at"].tolist() == [-1, 0] and out["steps"] == 10
    assert torch.equal(out["cell"][1], cell[1]) and torch.equal(out["pos"][2:], pos[2:])
    assert not torch.equal(out["cell"][0], cell[0]) and not torch.equal(out["pos"][:2], pos[:2])


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
    from gotennet_amd import CellRelax
    ef = types.SimpleNamespace(rep=types.SimpleNamespace(cutoff=5.0), head=None)
    base = dict(z=torch.tensor([8, 1, 1]), pos=torch.zeros((3, 3)), batch=torch.zeros(3, dtype=torch.int64), n_mol=1,
                cell=torch.eye(3) * 12.0)
    base.update(kw)
    return CellRelax(ef, **base)


def test_refusals_come_before_any_launch():
    nan, inf = float("nan"), float("inf")
    _no_launch(lambda: _make(rebuild="host"), "device")
    _no_launch(lambda: _make(rebuild="gpu"), "rebuild")
    _no_launch(lambda: _make(images="minimum"), "minimum")
    _no_launch(lambda: _make(cell=None), "needs a cell")
    for bad in (nan, inf, -inf):
        _no_launch(lambda: _make(pressure=bad), "pressure")
    for bad in (0.0, -1.0, nan, inf, torch.tensor([0.0]), torch.tensor([1.0, 2.0])):
        _no_launch(lambda: _make(cell_factor=bad), "cell_factor")
    _no_launch(lambda: _make(cell_mask=torch.ones((3, 3))), "cell_mask")                       # dtype
    _no_launch(lambda: _make(cell_mask=torch.ones(9, dtype=torch.uint8)), "cell_mask")         # shape
    _no_launch(lambda: _make(cell_mask=[[1, 1, 1]] * 3), "cell_mask")
    _no_launch(lambda: _make(cell=(torch.eye(3) * 12.0).requires_grad_()), "cell requires grad")
    # Relax's own still hold
    _no_launch(lambda: _make(fmax=-0.01), "fmax")
    _no_launch(lambda: _make(max_step=0.0), "max_step")
    _no_launch(lambda: _make(fixed=torch.zeros(4, dtype=torch.bool)), "fixed")
    _no_launch(lambda: _make(pos=torch.zeros((3, 3), requires_grad=True)), "pos requires grad")
    _no_launch(lambda: _make(cell=torch.eye(3) * 1.0), "cutoff / 3")
    _no_launch(lambda: _make(images="some"), "images")


def test_the_cell_grad_message_is_stated_once(repo_root):
    text = "".join(open(os.path.join(repo_root, "gotennet_amd", name)).read()
                   for name in sorted(os.listdir(os.path.join(repo_root, "gotennet_amd"))) if name.endswith(".py"))
    assert text.count('cell requires grad: autograd with respect to the cell is not supported")') == 1


# ---------------------------------------------------------------------------------------------------------- entry points
CELLRELAX = {"gn_cellrelax_forces": 15, "gn_cellrelax_apply": 11}


def test_entry_points_in_header_and_ctypes_table(repo_root):
    from gotennet_amd import _lib
    header = open(os.path.join(repo_root, "include", "gotennet_hip.h")).read()
    src = open(os.path.join(repo_root, "gotennet_amd", "csrc", "gn_cellrelax.hip")).read()
    for name, n_args in CELLRELAX.items():
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/gotennet_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]) == n_args, name
        assert re.search(r'extern "C" int ' + name + r"\(", src), name
    C = _lib.C
    assert _lib.SIGNATURES["gn_cellrelax_forces"] == ([C.c_void_p] * 5 + [C.c_double, C.c_int] + [C.c_void_p] * 3
                                                      + [C.c_int] * 2 + [C.c_void_p] * 3)
    assert _lib.SIGNATURES["gn_cellrelax_apply"] == [C.c_void_p] * 5 + [C.c_int] * 2 + [C.c_void_p] * 4
    declared = set(re.findall(r"^(?:int|long) (gn_\w+)\(", header, flags=re.M))
    assert {n for n in declared if n.startswith("gn_cellrelax_")} == set(CELLRELAX)
    assert {n for n in _lib.SIGNATURES if n.startswith("gn_cellrelax_")} == set(CELLRELAX)
    fire = {"gn_fire_fmax", "gn_fire_plan", "gn_fire_move", "gn_fire_finish"}
    assert {n for n in declared if n.startswith("gn_fire_")} == fire == {n for n in _lib.SIGNATURES if n.startswith("gn_fire_")}
    assert _lib.ABI_VERSION == 11 and "#define GN_ABI_VERSION 11" in header      # additive entries: the ABI number stays
    assert "atomic" not in src


# --------------------------------------------------------------------------------------------------------------- surface
def test_public_surface_and_defaults():
    import gotennet_amd
    from gotennet_amd import relax
    assert gotennet_amd.CellRelax is relax.CellRelax and issubclass(relax.CellRelax, relax.Relax)
    assert relax.CellRelax._cell_moves is True
    p = inspect.signature(relax.CellRelax.__init__).parameters
    base = inspect.signature(relax.Relax.__init__).parameters
    assert list(p)[:len(base)] == list(base)
    for k in base:
        if k not in ("self", "images"):
            assert p[k].default == base[k].default, k
    assert p["images"].default == "all" and p["fmax"].default == 0.05 and p["cell"].default is None
    assert list(p)[len(base):] == ["pressure", "hydrostatic", "cell_mask", "cell_factor"]
    assert [p[k].default for k in list(p)[len(base):]] == [0.0, False, None, None]
    for name in ("cell", "volume", "deformation", "cell_forces", "enthalpy", "vel", "cell_vel", "fmax", "forces", "pos", "stress",
                 "potential_energy", "converged", "status"):
        assert isinstance(getattr(relax.CellRelax, name), property), name
    assert "forces" not in vars(relax.CellRelax)                        # the real forces: Relax's
    # Relax is what it was
    want = dict(fmax=0.05, dt=0.1, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, fixed=None,
                cell=None, images="minimum", max_num_neighbors=32, check_every=1, log_len=1024, captured=True)
    assert [k for k in base][1:6] == ["ef", "z", "pos", "batch", "n_mol"] and [k for k in base][6:] == list(want)
    assert {k: base[k].default for k in want} == want
    assert "cell is fixed" in relax.Relax.__doc__ and "rebuild" not in base
