"""GPU: the two kernels of csrc/gn_cellrelax.hip, each on its own, against the fp64 yardstick of tests/cellrelax_util.py.

One batch holds boxes of 1, 2, 6 and 300 atoms (past the 256-thread stride) and an empty box, in triclinic cells with F != 1;
every output lies between guard rows.

The bound (derived, not measured): both kernels form every value in fp64 from the fp32 inputs and round it once, and so does
the yardstick; the two fp64 values differ by the order of a handful of operations, ~1e-16 relative, which can move a rounding,
never more -> within 1 fp32 ulp of the fp64 value."""
import functools

import pytest
import torch

from tests import cellrelax_util as CU
from tests import pbc_multi_util as PM
from tests import pbc_util as U

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 6, 300, 0)
CELLS = (U.TRICLINIC, PM.N1_CELL, PM.N2_CELL, U.TRICLINIC, PM.N1_CELL)
PRESSURE, PAD, GUARD = 0.37, 8, 7.0
MASK = torch.tensor([[1, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=torch.uint8)
VARIANTS = dict(plain={}, fixed=dict(fixed=True), hydrostatic=dict(hydrostatic=True), mask=dict(cell_mask=MASK),
                weighted=dict(cell_factor=2.5))


@functools.lru_cache(maxsize=None)
def _batch():
    """The synthetic batch on the host, fp32 values.  Read-only."""
    g = torch.Generator().manual_seed(9)
    mol_ptr = [0]
    for s in SIZES:
        mol_ptr.append(mol_ptr[-1] + s)
    N, n = mol_ptr[-1], len(SIZES)
    cell0 = torch.tensor(CELLS, dtype=torch.float32)
    F = torch.eye(3) + 0.05 * torch.randn((n, 3, 3), generator=g)
    frac = torch.rand((N, 3), generator=g)
    batch = torch.repeat_interleave(torch.arange(n), torch.tensor(SIZES))
    x = torch.einsum("na,nab->nb", frac, cell0[batch]).float()
    fixed = torch.zeros(N, dtype=torch.uint8)
    fixed[[1, 4, 9 + 17, 9 + 256, 9 + 299]] = 1
    coef = torch.rand((n, 4), generator=g).float()
    coef[:, 3] = torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0])
    return dict(mol_ptr=mol_ptr, N=N, n=n, cell0=cell0, F=F, x=x, fixed=fixed, coef=coef,
                force=torch.randn((N, 3), generator=g).float(), stress=(0.05 * torch.randn((n, 3, 3), generator=g)).float(),
                # the current cell the forces kernel reads: C0 F rounded to fp32, as gn_cellrelax_apply leaves it
                cell=(cell0.double() @ F.double()).float(),
                pos_in=torch.randn((N, 3), generator=g).float(), cell_in=torch.randn((n, 3, 3), generator=g).float())


def _inputs(variant):
    b, kw = _batch(), VARIANTS[variant]
    w = CU.weights(b["mol_ptr"], kw.get("cell_factor")).float()
    x_ext = CU.extend(b["x"], b["mol_ptr"], w, b["F"]).float()           # (the cell rows: w F rounded to fp32)
    return b, kw, w, x_ext


def _guarded(rows, width=3):
    buf = torch.full((PAD + rows + PAD, width), GUARD, dtype=torch.float32).cuda()
    return buf, buf[PAD:PAD + rows]


def _guards_intact(buf, rows):
    return bool((buf[:PAD] == GUARD).all()) and bool((buf[PAD + rows:] == GUARD).all())


def _forces(variant, state0=0, stress=None):
    from gotennet_amd._lib import call, ptr
    b, kw, w, x_ext = _inputs(variant)
    NE = b["N"] + 3 * b["n"]
    buf, g = _guarded(NE)
    dev = lambda t: t.cuda().contiguous()
    mask = dev(kw["cell_mask"].reshape(9)) if "cell_mask" in kw else None
    fixed = dev(b["fixed"]) if kw.get("fixed") else None
    keep = [dev(t) for t in (b["force"], b["stress"] if stress is None else stress, b["cell"], x_ext, w)]
    mol_ptr, state = torch.tensor(b["mol_ptr"], dtype=torch.int32).cuda(), torch.tensor([state0, 5], dtype=torch.int32).cuda()
    call("gn_cellrelax_forces", *(ptr(t) for t in keep), PRESSURE, int(bool(kw.get("hydrostatic"))), ptr(mask), ptr(fixed),
         ptr(mol_ptr), b["N"], b["n"], ptr(g), ptr(state), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _guards_intact(buf, NE) and state.tolist() == [state0, 5]
    return g.cpu().clone()


def _forces_expected(variant, stress=None):
    b, kw, w, x_ext = _inputs(variant)
    return CU.generalised_forces(b["force"], b["stress"] if stress is None else stress, b["cell"], x_ext, b["mol_ptr"], w,
                                 pressure=PRESSURE, hydrostatic=bool(kw.get("hydrostatic")), cell_mask=kw.get("cell_mask"),
                                 fixed=b["fixed"] if kw.get("fixed") else None)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_forces_against_the_fp64_yardstick(variant):
    b = _batch()
    got, want = _forces(variant), _forces_expected(variant)
    ok = CU.within_ulps(got, want, 1)
    worst = float(((got.double() - want).abs() / CU.FU.ulp32(want)).max())
    print(f"gn_cellrelax_forces {variant}: worst |difference| {worst:.3f} ulp over {got.numel()} values")
    assert bool(ok.all()), (variant, ok.logical_not().nonzero().tolist()[:8])
    lay = CU.layout(b["mol_ptr"])
    assert bool(torch.isfinite(got).all()) and bool((got[lay["cell_rows"]] != 0).any())
    if variant == "mask":
        assert bool((got[lay["cell_rows"]][:, ~MASK.bool()] == 0).all())
    if variant == "fixed":
        assert bool((got[lay["atom_rows"]][b["fixed"].bool()] == 0).all())
    assert torch.equal(got, _forces(variant))                        # identical inputs, identical bits


def test_a_stress_that_is_not_finite_reaches_that_box_alone():
    b = _batch()
    stress = b["stress"].clone()
    stress[2, 0, 1] = float("nan")
    got, base = _forces("plain", stress=stress), _forces("plain")
    lay = CU.layout(b["mol_ptr"])
    rows = lay["cell_rows"][2]
    assert bool(torch.isnan(got[rows]).any())
    others = torch.ones(got.shape[0], dtype=torch.bool)
    others[rows] = False
    assert torch.equal(got[others], base[others])
    assert bool(CU.within_ulps(got, _forces_expected("plain", stress=stress), 1).all())


def _apply(variant, state0=0):
    from gotennet_amd._lib import call, ptr
    b, kw, w, x_ext = _inputs(variant)
    pbuf, pos = _guarded(b["N"])
    cbuf, cell = _guarded(b["n"], 9)
    pos.copy_(b["pos_in"]), cell.copy_(b["cell_in"].reshape(-1, 9))
    keep = [t.cuda().contiguous() for t in (x_ext, b["cell0"], w, b["coef"])]
    mol_ptr, state = torch.tensor(b["mol_ptr"], dtype=torch.int32).cuda(), torch.tensor([state0, 5], dtype=torch.int32).cuda()
    call("gn_cellrelax_apply", *(ptr(t) for t in keep), ptr(mol_ptr), b["N"], b["n"], ptr(pos), ptr(cell), ptr(state),
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _guards_intact(pbuf, b["N"]) and _guards_intact(cbuf, b["n"]) and state.tolist() == [state0, 5]
    return pos.cpu().clone(), cell.cpu().clone().reshape(-1, 3, 3)


@pytest.mark.parametrize("variant", ["plain", "weighted"])
def test_apply_against_the_fp64_yardstick(variant):
    b, kw, w, x_ext = _inputs(variant)
    pos, cell = _apply(variant)
    active = b["coef"][:, 3] == 1.0
    want_pos, want_cell = CU.apply(x_ext, b["cell0"], b["mol_ptr"], w, b["pos_in"], b["cell_in"], active=active)
    assert bool(CU.within_ulps(pos, want_pos, 1).all()) and bool(CU.within_ulps(cell, want_cell, 1).all())
    # the box FIRE did not move (coef[1][3] == 0) keeps its bits; the others are written, fixed atoms or not
    assert torch.equal(pos[1:3], b["pos_in"][1:3]) and torch.equal(cell[1], b["cell_in"][1])
    moved = torch.ones(b["N"], dtype=torch.bool)
    moved[1:3] = False
    assert not bool((pos[moved] == b["pos_in"][moved]).all(1).any()) and not bool((cell[active] == b["cell_in"][active]).any())
    again = _apply(variant)
    assert torch.equal(pos, again[0]) and torch.equal(cell, again[1])


def test_a_set_sticky_word_writes_nothing():
    b = _batch()
    assert bool((_forces("plain", state0=1) == GUARD).all())
    pos, cell = _apply("plain", state0=1)
    assert torch.equal(pos, b["pos_in"]) and torch.equal(cell, b["cell_in"])
