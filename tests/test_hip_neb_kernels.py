"""GPU: the two entry points of csrc/gn_neb.hip, each on its own, against the fp64 yardstick of tests/neb_util.py.  No model:
positions, forces and energies are synthetic fp32 numbers, ``mol_ptr`` is written by hand, every output lies between guard
words.

The energies are fed as fp32 and the yardstick compares them as fp32, so both take the same tangent branch by construction;
``g`` is then held per element to ``neb_util.g_bound`` (one fp32 ulp of the reference value plus the fp64 summation-order term
derived in that module's docstring).  Everything else -- the band's largest energy, the climbing image, the zero rows, g = f
on coincident images, NaN propagation, repeatability, the predicate on ``state[0]``, ``gn_neb_finish`` -- is checked exactly."""
import functools

import pytest
import torch

from tests import neb_util as NU

pytestmark = pytest.mark.gpu

PAD, GUARD = 8, 7.0
NAN = float("nan")

#: name -> (atoms per image for every band, n_img, energies per band, k, climb, fixed offsets per band, branches expected)
#: branches: neb_util.neb_forces' codes over the interior images, in order (+10: the climbing image)
CASES = {
    # the smallest band, one atom per image, once per branch of the tangent rule
    "rise": ([1], 3, [[0.5, 1.25, 2.0]], 0.3, False, [[]], [1]),
    "fall": ([1], 3, [[2.0, 1.25, 0.5]], 0.3, False, [[]], [2]),
    "max_up": ([1], 3, [[0.5, 2.0, 1.25]], 0.3, False, [[]], [3]),
    "max_down": ([1], 3, [[1.25, 2.0, 0.5]], 0.3, True, [[]], [14]),
    "min_up": ([1], 3, [[1.25, 0.5, 2.0]], 0.3, False, [[]], [3]),
    "min_down": ([1], 3, [[2.0, 0.5, 1.25]], 0.3, False, [[]], [4]),
    "tie_ends": ([1], 3, [[1.0, 2.0, 1.0]], 0.3, True, [[]], [14]),
    "tie_next": ([1], 3, [[0.5, 1.0, 1.0]], 0.3, False, [[]], [3]),
    "tie_previous": ([1], 3, [[1.0, 1.0, 0.5]], 0.3, False, [[]], [4]),
    # two bands of 5 images with 3 and 5 atoms per image; a fixed atom in the second band; equal maxima in the second band
    "two_bands": ([3, 5], 5, [[0.0, 1.0, 3.0, 2.0, 2.5], [5.0, 4.0, 4.0, 1.0, 2.0]], 0.1, True, [[], [1]], [1, 13, 4, 14, 4, 4]),
    "two_bands_plain": ([3, 5], 5, [[3.0, 2.0, 1.0, 1.5, 9.0], [0.0, 1.0, 2.0, 3.0, 2.5]], 0.7, False, [[2], [0, 4]],
                        [2, 4, 1, 1, 1, 3]),
    # one band of 4 images with 300 atoms per image: the stride-256 loop runs twice and all four waves carry data
    "wide": ([300], 4, [[0.0, 2.0, 1.0, 3.0]], 0.1, True, [[7, 255, 256, 299]], [13, 3]),
    "wide_fall": ([300], 4, [[3.0, 2.0, 1.0, 0.5]], 0.25, False, [[]], [2, 2]),
    # a band whose images are all empty, next to a band of coincident images (|t| = 0: g = f) and an ordinary one
    "empty": ([0, 2, 2], 3, [[0.0, 1.0, 0.5], [0.0, 1.0, 2.0], [0.0, 1.0, 2.0]], 0.1, True, [[], [], []], [15, 11]),
    # an energy that is not finite: NaN on the three images that read it, the other band untouched
    "not_finite": ([3, 5], 5, [[0.0, 1.0, NAN, 2.0, 2.5], [5.0, 4.0, 3.0, float("inf"), 2.0]], 0.1, False, [[], [1]],
                   [6, 6, 6, 2, 6, 6]),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case on the host (fp32 values) and its fp64 expectation.  Read-only."""
    sizes, n_img, energies, k, climb, fixed_at, branches = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    mol_ptr = [0]
    for s in sizes:
        for _ in range(n_img):
            mol_ptr.append(mol_ptr[-1] + s)
    N, n_mol = mol_ptr[-1], len(mol_ptr) - 1
    base = 2.0 * torch.randn((N, 3), generator=gen)
    pos = torch.empty((N, 3))
    fixed = torch.zeros(N, dtype=torch.uint8)
    for m in range(n_mol):
        a0, a1, b, i = mol_ptr[m], mol_ptr[m + 1], m // n_img, m % n_img
        first = mol_ptr[b * n_img]
        # a bent path: image i = the band's first image + i * (a common direction) + a small random part
        pos[a0:a1] = base[first:first + a1 - a0] + i * torch.tensor([0.4, 0.1, -0.2]) + 0.15 * torch.randn((a1 - a0, 3), generator=gen)
        for o in fixed_at[b]:
            fixed[a0 + o] = 1
    if name == "empty":                                   # band 1: three images in one place
        pos[mol_ptr[4]:mol_ptr[5]] = pos[mol_ptr[3]:mol_ptr[4]]
        pos[mol_ptr[5]:mol_ptr[6]] = pos[mol_ptr[3]:mol_ptr[4]]
    pos = pos.float()
    force = torch.randn((N, 3), generator=gen).float()
    energy = torch.tensor([e for row in energies for e in row], dtype=torch.float32)
    fx = fixed if bool(fixed.any()) else None
    ref, e_band, ci, info = NU.neb_forces(pos, force, energy, mol_ptr, n_img, k, climb, fx, detail=True)
    return dict(name=name, mol_ptr=mol_ptr, N=N, n_mol=n_mol, n_img=n_img, k=k, climb=climb, pos=pos, force=force, energy=energy,
                fixed=fx, ref=ref, e_band=e_band, ci=ci, info=info, bound=NU.g_bound(ref, info, k), branches=branches)


def _padded(n, dtype, fill=GUARD):
    return torch.full((n + 2 * PAD,), fill, dtype=dtype, device="cuda")


def _launch(c, stuck=0):
    """gn_neb_forces on the case -> (g [N, 3], e_band, climb_out, the three padded buffers) on the host."""
    from gotennet_amd._lib import call, ptr
    dev = dict(device="cuda")
    pos, force, energy = c["pos"].to(**dev), c["force"].to(**dev), c["energy"].to(**dev)
    fixed = None if c["fixed"] is None else c["fixed"].to(**dev)
    mol_ptr = torch.tensor(c["mol_ptr"], dtype=torch.int32, **dev)
    n_band = c["n_mol"] // c["n_img"]
    g, eb, co = _padded(3 * c["N"], torch.float32), _padded(n_band, torch.float32), _padded(n_band, torch.int32, 77)
    state = torch.tensor([stuck, 5], dtype=torch.int32, **dev)
    esz, isz = g.element_size(), co.element_size()
    call("gn_neb_forces", ptr(pos), ptr(force), ptr(energy), ptr(fixed), ptr(mol_ptr), c["N"], c["n_mol"], c["n_img"], c["k"],
         int(c["climb"]), g.data_ptr() + PAD * esz, eb.data_ptr() + PAD * esz, co.data_ptr() + PAD * isz, ptr(state),
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert state.tolist() == [stuck, 5]
    g, eb, co = g.cpu(), eb.cpu(), co.cpu()
    return g[PAD:-PAD].reshape(-1, 3), eb[PAD:-PAD], co[PAD:-PAD], (g, eb, co)


@pytest.mark.parametrize("name", list(CASES))
def test_the_case_takes_the_branches_it_names(name):
    """Conditions on the INPUT, from the fp64 yardstick alone."""
    c = _case(name)
    got = [int(c["info"]["branch"][c["mol_ptr"][m]]) if c["mol_ptr"][m + 1] > c["mol_ptr"][m] else None
           for m in range(c["n_mol"]) if m % c["n_img"] not in (0, c["n_img"] - 1)]
    if c["fixed"] is not None:                            # (a fixed first atom reads 0: take the image's largest code)
        got = [int(c["info"]["branch"][c["mol_ptr"][m]:c["mol_ptr"][m + 1]].max())
               for m in range(c["n_mol"]) if m % c["n_img"] not in (0, c["n_img"] - 1)]
    assert [x for x in got if x is not None] == c["branches"], got
    assert float(c["info"]["kappa2"].max()) < 16.0        # no tangent of the mix branch is a near-cancellation


@pytest.mark.parametrize("name", list(CASES))
def test_band_forces_against_the_fp64_rule(name):
    c = _case(name)
    g, e_band, ci, padded = _launch(c)
    # exact: guard words, the band's largest energy (a NaN wins), the climbing image
    for buf, fill in zip(padded, (GUARD, GUARD, 77)):
        assert bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all())
    assert torch.equal(torch.isnan(e_band), torch.isnan(c["e_band"]))
    assert torch.equal(e_band[~torch.isnan(e_band)], c["e_band"][~torch.isnan(e_band)])
    assert ci.tolist() == c["ci"].tolist()
    # exact: zeros on end images, fixed rows (and nowhere else by accident), g = f on coincident images, NaN where not finite
    branch = (c["info"]["branch"] % 10).long()
    assert bool((g[branch == 0] == 0).all()) and not bool(torch.signbit(g[branch == 0]).any())
    assert torch.equal(g[branch == 5], c["force"][branch == 5])
    assert bool(torch.isnan(g[branch == 6]).all())
    live = (branch >= 1) & (branch <= 4)
    assert not bool(torch.isnan(g[live]).any())
    if name not in ("not_finite",):
        assert bool(live.any())
    # the bound: one fp32 ulp of the reference plus the summation-order term (neb_util's docstring)
    err = (g.double() - c["ref"]).abs()[live]
    bound = c["bound"][live]
    if err.numel():
        worst = float((err / bound).max())
        print(f"{name}: max |g - ref| {float(err.max()):.3e}, worst error / bound {worst:.3f}, "
              f"largest order term {float((bound - NU.FU.ulp32(c['ref'])[live]).max()):.3e}")
        assert bool((err <= bound).all()), worst


@pytest.mark.parametrize("name", ["two_bands", "wide", "empty", "not_finite"])
def test_repeatable_and_predicated(name):
    c = _case(name)
    one, two = _launch(c), _launch(c)
    for x, y in zip(one[3], two[3]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))          # bit for bit, NaNs included
    # state[0] set: no output byte changes
    for buf, fill in zip(_launch(c, stuck=1)[3], (GUARD, GUARD, 77)):
        assert bool((buf == fill).all())


def test_bad_arguments_are_refused():
    from gotennet_amd import _lib
    c = _case("two_bands")
    lib = _lib.load()
    dev = dict(device="cuda")
    pos, force, energy = c["pos"].to(**dev), c["force"].to(**dev), c["energy"].to(**dev)
    mol_ptr = torch.tensor(c["mol_ptr"], dtype=torch.int32, **dev)
    g, eb, co = torch.zeros((c["N"], 3), **dev), torch.zeros(2, **dev), torch.zeros(2, dtype=torch.int32, **dev)
    state = torch.zeros(2, dtype=torch.int32, **dev)
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(pos=pos.data_ptr(), force=force.data_ptr(), energy=energy.data_ptr(), fixed=None, mol_ptr=mol_ptr.data_ptr(),
                N=c["N"], n_mol=c["n_mol"], n_img=c["n_img"], k=0.1, climb=1, g=g.data_ptr(), eb=eb.data_ptr(), co=co.data_ptr(),
                state=state.data_ptr(), stream=stream)
    assert lib.gn_neb_forces(*good.values()) == 0
    for change in (dict(n_img=2), dict(n_img=0), dict(n_img=3), dict(n_img=4), dict(N=-1), dict(n_mol=-5), dict(k=-0.1), dict(k=NAN),
                   dict(k=float("inf")), dict(pos=None), dict(force=None), dict(energy=None), dict(mol_ptr=None), dict(g=None),
                   dict(eb=None), dict(co=None), dict(state=None)):
        assert lib.gn_neb_forces(*dict(good, **change).values()) == _lib.GN_ERR_BAD_ARG, change
    batch = torch.zeros(c["N"], dtype=torch.int64, **dev)
    status = torch.zeros(2, dtype=torch.int32, **dev)
    fin = dict(state=state.data_ptr(), status=status.data_ptr(), batch=batch.data_ptr(), force=force.data_ptr(), keep=g.data_ptr(),
               N=c["N"], energy=energy.data_ptr(), e_keep=torch.zeros(10, **dev).data_ptr(), stress=None, s_keep=None, n_mol=10,
               n_img=5, stream=stream)
    for change in (dict(n_img=2), dict(n_img=3), dict(n_mol=9), dict(state=None), dict(status=None), dict(batch=None),
                   dict(keep=None), dict(e_keep=None), dict(stress=energy.data_ptr())):
        assert lib.gn_neb_finish(*dict(fin, **change).values()) == _lib.GN_ERR_BAD_ARG, change
    torch.cuda.synchronize()
    assert state.tolist() == [0, 0]                       # none of the refused calls launched anything


@pytest.mark.parametrize("with_stress", [True, False])
def test_finish_keeps_per_band(with_stress):
    """Two bands of 3 images (2 and 3 atoms per image), statuses (1, 0): the frozen band keeps forces, energies and stress of all
    its images, the active band's are replaced, the counter advances by one; with state[0] set nothing changes."""
    from gotennet_amd._lib import call, ptr
    dev = dict(device="cuda")
    gen = torch.Generator().manual_seed(9)
    sizes, n_img, n_mol = [2, 2, 2, 3, 3, 3], 3, 6
    batch = torch.repeat_interleave(torch.arange(n_mol), torch.tensor(sizes))
    N = batch.numel()
    new = [torch.randn((N, 3), generator=gen), torch.randn(n_mol, generator=gen), torch.randn((n_mol, 3, 3), generator=gen)]
    old = [torch.randn((N, 3), generator=gen), torch.randn(n_mol, generator=gen), torch.randn((n_mol, 3, 3), generator=gen)]
    for statuses, stuck in (([1, 0], 0), ([0, 2], 0), ([0, 0], 0), ([1, 0], 1)):
        status = torch.tensor(statuses, dtype=torch.int32, **dev)
        state = torch.tensor([stuck, 41], dtype=torch.int32, **dev)
        d_new, keep = [t.to(**dev) for t in new], [t.to(**dev).clone() for t in old]
        call("gn_neb_finish", ptr(state), ptr(status), ptr(batch.to(**dev)), ptr(d_new[0]), ptr(keep[0]), N, ptr(d_new[1]),
             ptr(keep[1]), ptr(d_new[2]) if with_stress else None, ptr(keep[2]) if with_stress else None, n_mol, n_img,
             torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert state.tolist() == [stuck, 41 if stuck else 42] and status.tolist() == statuses
        active_mol = torch.tensor([statuses[m // n_img] == 0 and not stuck for m in range(n_mol)])
        want = [torch.where(active_mol[batch].unsqueeze(1), new[0], old[0]), torch.where(active_mol, new[1], old[1]),
                torch.where(active_mol.reshape(-1, 1, 1), new[2], old[2]) if with_stress else old[2]]
        for got, w in zip(keep, want):
            assert torch.equal(got.cpu(), w), (statuses, stuck)
