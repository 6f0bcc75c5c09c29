"""The X-cat input-gradient launch of a layer with an edge update, gX1 = gX + [gXp | gEQ | gEK_l] [W_vu^T | W_vq^T | W_vk_l^T]^T per
degree block (K = 768, K-segmented A, row maps, ``res``): on the eight-wave 128 x 256 slab tile from GN_F16_XCAT_MIN_ROWS rows up
(gn_gemm.hip ``xcat_big8``), on the K-resident panel kernel below.  f16x2 results are held to the per-row bound of DESIGN section
4 against the fp64 product, max_n |C - ref| <= 32 max(2^-23, 2^(d - 41)) max_n |ref|, d = log2 of (the largest |A| in the row's
exponent group / the row's own), with the row grouping of the kernel the launch runs on."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BIG8 = 2                                           # GN_GEMM_FORM_BIG8
MIN_ROWS = 16384                                   # GN_F16_XCAT_MIN_ROWS (gn_tune.h)
PANEL_GROUP = lambda r: r // 8                     # rows that share a block exponent, by the problem's logical row
BIG8_GROUP = lambda r: (r // 128) * 8 + (r % 64) // 8


def _ratio(C, ref, amax, group):
    """max_n |C - ref| of every row over 32 max(2^-23, 2^(d - 41)) max_n |ref| (rows in the problem's logical order)."""
    grp = group(torch.arange(C.shape[0], device="cuda"))
    gmax = torch.zeros(int(grp.max()) + 1, dtype=torch.float64, device="cuda").scatter_reduce_(
        0, grp, amax, "amax", include_self=True)[grp]
    d = torch.log2(gmax / amax.clamp_min(1e-300))
    bound = 32.0 * torch.maximum(torch.full_like(d, 2.0 ** -23), 2.0 ** (d - 41)) * ref.abs().amax(1)
    return float(((C.double() - ref).abs().amax(1) / bound.clamp_min(1e-300)).max())


def _block_rows(N, D, rowmap):
    cnt, stride, off = rowmap
    r = torch.arange(N * cnt, device="cuda")
    return (r // cnt) * stride + off + r % cnt


def _energy_forces(mode, n_mol, lmax=2, L=2):
    import gotennet_amd
    from gotennet_amd import synthetic
    from gotennet_amd.graph import distance
    from gotennet_amd.outputs import Atomwise
    from gotennet_amd.pipeline import EnergyForces
    torch.manual_seed(17)
    rep = gotennet_amd.GotenNet(n_atom_basis=256, n_interactions=L, n_rbf=16, cutoff_fn=gotennet_amd.CosineCutoff(5.0),
                                num_heads=8, scale_edge=True, lmax=lmax, sep_dir=True, sep_tensor=True).to("cuda").eval()
    rep.gemm_mode = mode
    torch.manual_seed(5)
    head = Atomwise(n_in=256, n_hidden=128, derivative="forces", activation="silu").to("cuda").eval()
    ef = EnergyForces(rep, head)
    pos, batch, z = synthetic.make_batch("rmd17_aspirin", n_mol, seed=4)
    pos, batch, z = pos.cuda(), batch.cuda(), z.cuda()
    ei, ed, ev = distance(pos, batch, 5.0, 32)
    return ef, pos, batch, z, ei, ed, ev


def _xcat_group(n_atoms, res=True, seed=0):
    """The X-cat group of the force backward at lmax 2 with its real row maps: -> (problems without C, fp64 reference rows per
    block, |A| row maxima per block, block row indices)."""
    F, D = 256, 8
    g = torch.Generator(device="cuda").manual_seed(1000 + n_atoms + seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    dec = torch.randint(-4, 1, (n_atoms * D, 1), device="cuda", generator=g).float()
    sc = lambda t: (t.view(-1, F) * 10.0 ** dec).view(t.shape)
    gXp, gEQ, gEK, gX = sc(r(n_atoms, D, F)), sc(r(n_atoms, D, F)), sc(r(n_atoms, D, F)), sc(r(n_atoms, D, F))
    probs, refs, amaxs, idxs = [], [], [], []
    for l, (cnt, off) in enumerate(((3, 0), (5, 3))):
        W = r(F, 3 * F) / 8
        idx = _block_rows(n_atoms, D, (cnt, D, off))
        f = lambda t: t.view(-1, F)[idx]
        probs.append(dict(A=gXp, A2=gEQ, A3=gEK, a_seg=F, lda=F, W=W, ldc=F, rows=n_atoms * cnt, nout=F, K=3 * F,
                          rowmap=(cnt, D, off), res=gX if res else None))
        A = torch.cat([f(gXp), f(gEQ), f(gEK)], 1)
        refs.append((f(gX).double() if res else 0.0) + A.double() @ W.double().T)
        amaxs.append(A.abs().amax(1).double())
        idxs.append(idx)
    return probs, refs, amaxs, idxs


@pytest.mark.parametrize("n_atoms", [8, 33])
def test_xcat_on_the_eight_wave_tile(n_atoms):
    """Rows 24 + 40 and 99 + 165: partial 128-row tiles, row maps (3, 8, 0) and (5, 8, 3), three A tensors, ``res`` set --
    forced onto GN_GEMM_FORM_BIG8, and routed (below the row threshold: the panel kernel), each within the per-row bound
    of its own row grouping; rows outside the blocks' row maps do not exist here (the two blocks cover every row)."""
    from gotennet_amd import engine
    probs, refs, amaxs, idxs = _xcat_group(n_atoms)
    for form, group in ((BIG8, BIG8_GROUP), (0, PANEL_GROUP)):
        C = torch.full((n_atoms, 8, 256), float("nan"), device="cuda")
        engine.gemm_group([dict(q, C=C) for q in probs], mode="f16x2", form=form)
        assert bool(torch.isfinite(C).all())
        for ref, amax, idx in zip(refs, amaxs, idxs):
            ratio = _ratio(C.view(-1, 256)[idx], ref, amax, group)
            print(f"atoms {n_atoms} form {form} rows {len(idx)}: max err / bound {ratio:.3f}")
            assert ratio <= 1.0


def test_xcat_one_molecule_keeps_the_panel_kernel():
    """21 atoms (63 + 105 rows): the routed group equals, bit for bit, the same problems launched one by one (which stay under
    the row threshold whatever it is) -- and not the eight-wave tile, whose exponent groups differ."""
    from gotennet_amd import engine
    probs, _, _, _ = _xcat_group(21)
    out = {}
    for what in ("group", "single", "big8"):
        C = torch.full((21, 8, 256), float("nan"), device="cuda")
        if what == "single":
            for q in probs:
                engine.gemm_group([dict(q, C=C)], mode="f16x2")
        else:
            engine.gemm_group([dict(q, C=C) for q in probs], mode="f16x2", form=BIG8 if what == "big8" else 0)
        out[what] = C
    assert torch.equal(out["group"], out["single"])
    assert not torch.equal(out["group"], out["big8"])


def test_xcat_routed_to_the_eight_wave_tile_from_the_row_threshold():
    """2 049 atoms (6 147 + 10 245 = 16 392 rows >= GN_F16_XCAT_MIN_ROWS): the routed group is the eight-wave tile -- its bits, within
    the per-row bound of that tile's row grouping, and not the panel kernel's bits (the same problems launched one by one: 6 147 and
    10 245 rows each stay under the threshold).  2 047 atoms (16 376 rows): the routed group is still the panel kernel's."""
    from gotennet_amd import engine
    def run(probs, n_atoms, how):
        C = torch.full((n_atoms, 8, 256), float("nan"), device="cuda")
        if how == "single":
            for q in probs:
                engine.gemm_group([dict(q, C=C)], mode="f16x2")
        else:
            engine.gemm_group([dict(q, C=C) for q in probs], mode="f16x2", form=BIG8 if how == "big8" else 0)
        return C
    n_atoms = 2049
    probs, refs, amaxs, idxs = _xcat_group(n_atoms)
    assert sum(q["rows"] for q in probs) >= MIN_ROWS and all(q["rows"] < MIN_ROWS for q in probs)
    routed, big8, panel = run(probs, n_atoms, "group"), run(probs, n_atoms, "big8"), run(probs, n_atoms, "single")
    assert torch.equal(routed, big8) and not torch.equal(routed, panel)
    for ref, amax, idx in zip(refs, amaxs, idxs):
        ratio = _ratio(routed.view(-1, 256)[idx], ref, amax, BIG8_GROUP)
        print(f"routed, {len(idx)} rows: max err / bound {ratio:.3f}")
        assert ratio <= 1.0
    n_atoms = 2047
    probs, _, _, _ = _xcat_group(n_atoms)
    assert sum(q["rows"] for q in probs) < MIN_ROWS
    routed, big8, panel = run(probs, n_atoms, "group"), run(probs, n_atoms, "big8"), run(probs, n_atoms, "single")
    assert torch.equal(routed, panel) and not torch.equal(routed, big8)


def test_captured_step_replays_bit_identical():
    """pipeline.CapturedStep against the eager path, F = 256, two molecules, f16x2: the X-cat launch inside a replayed graph."""
    from gotennet_amd.pipeline import CapturedStep
    ef, pos, batch, z, ei, ed, ev = _energy_forces("f16x2", 2)
    step = CapturedStep(ef, z, ei, batch, 2)
    g = torch.Generator().manual_seed(9)
    for k in range(3):
        q = pos + 0.05 * k * torch.randn(pos.shape, generator=g).cuda()
        e_g, f_g = (t.clone() for t in step(q))
        src, dst = ei[0], ei[1]
        vec = q[src] - q[dst]
        diff = torch.where(src == dst, torch.zeros_like(vec[:, 0]),
                           torch.sqrt(vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1] + vec[:, 2] * vec[:, 2]))
        e_e, f_e = ef(z, ei, diff, vec, batch, 2)
        assert torch.equal(e_g, e_e) and torch.equal(f_g, f_e), k
