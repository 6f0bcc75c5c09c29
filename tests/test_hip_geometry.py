"""GPU: gn_edge_geometry, gn_cosine_cutoff, gn_edge_geometry_backward (both with their `_images` entry points) and
gn_pos_scatter called directly, against the fp64 restatement and the a-priori per-element bounds of tests/geometry_util.py (proved
on the CPU by tests/test_geometry_host.py).  Each case prints its worst error / bound per output; the last test prints the worst
per output and per lmax."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import gotennet_oracle as orc
from tests import geometry_util as G
from tests.gather_util import U32
from tests.golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

PAD_ROWS = 8                                       # sentinel rows past the last row of every output array
SENTINEL = 12345.678
BAD_ARG = 10001
WORST = {}                                         # lmax -> {output: worst error / bound seen by this module}
CASES = range(len(G.GEO_CASES))
IDS = [G.geo_id(c) for c in G.GEO_CASES]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _padded(rows, cols):
    """[rows + PAD_ROWS, cols]: NaN inside (a skipped element fails its bound), the sentinel past the end."""
    t = torch.full((rows + PAD_ROWS, cols), SENTINEL, device="cuda")
    t[:rows] = math.nan
    return t


def _f32(*pairs):
    for t, n in pairs:
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, (tuple(t.shape), n)


def _i32(*pairs):
    for t, n in pairs:
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n, (tuple(t.shape), n)


def _dev(t):
    """On the device with one NaN / -1 element past the end: never a NULL pointer at E = 0, and an over-read is seen."""
    fill = math.nan if t.is_floating_point() else -1
    return torch.cat([t.reshape(-1), torch.full((1,), fill, dtype=t.dtype)]).cuda()


def _check_outputs(outs, rows, refused):
    for name, t in outs.items():
        assert bool((t[rows[name]:] == SENTINEL).all()), f"{name}: a row past the end was written"
        assert not refused or bool(torch.isnan(t[:rows[name]]).all()), f"{name}: written by a refused call"


def _launch_k1(c, expect_rc=0, null_diff=False, **over):
    """The ONE place K1's inputs reach the library: everything the kernels index with is asserted before the launch.  Two
    launches into fresh arrays: same bits; sentinel rows keep their value.  -> dict(rl, phi, cut) on the CPU.  ``expect_rc``:
    a refusal -- one call, nothing written; ``over`` overrides arguments for those (the arrays are sized for lmax 9)."""
    from gotennet_amd import _lib
    lib = _lib.load()
    E, R, lmax = c["E"], c["R"], c["lmax"]
    D = G.ndim(9 if expect_rc else lmax)
    _f32((c["vec"], 3 * E), (c["diff"], E), (c["p0"], R), (c["p1"], R))
    _i32((c["src"], E), (c["dst"], E))
    if not expect_rc:
        assert not over and 1 <= lmax <= 8 and R > 0 and c["basis"] in (0, 1, 2) and c["cutoff"] == float(np.float32(c["cutoff"]))
    dev = {k: _dev(c[k]) for k in ("vec", "diff", "src", "dst", "p0", "p1")}
    fn = lib.gn_edge_geometry_images if c["images"] else lib.gn_edge_geometry
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for _ in range(2):
        rl, phi, cut = _padded(E, D), _padded(E, R), _padded(E, 1)
        rc = fn(dev["vec"].data_ptr(), None if null_diff else dev["diff"].data_ptr(), dev["src"].data_ptr(), dev["dst"].data_ptr(),
                over.get("E", E), over.get("lmax", lmax), over.get("R", R), over.get("basis", c["basis"]), dev["p0"].data_ptr(),
                dev["p1"].data_ptr(), c["cutoff"], rl.data_ptr(), phi.data_ptr(), cut.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == expect_rc, rc
        outs = dict(rl=rl, phi=phi, cut=cut)
        _check_outputs(outs, dict(rl=E, phi=E, cut=E), expect_rc)
        if expect_rc:
            return None
        cc = _padded(E, 1)                                                  # gn_cosine_cutoff: the same expression, the same bits
        assert lib.gn_cosine_cutoff(dev["diff"].data_ptr(), E, c["cutoff"], cc.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert bool((cc[E:] == SENTINEL).all()) and torch.equal(_bits(cc[:E]), _bits(cut[:E])), "gn_cosine_cutoff differs from K1's cut"
        res.append({k: t[:E].cpu() for k, t in outs.items()})
    for k in res[0]:
        assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), f"{k}: two launches differ"
    return dict(rl=res[0]["rl"], phi=res[0]["phi"], cut=res[0]["cut"][:, 0])


def _launch_k1_bwd(c, expect_rc=0, null_diff=False, **over):
    """The ONE place the geometry backward's inputs reach the library; same rules as _launch_k1.  The slice arrays carry one NaN
    slice past n_rl / n_cut: a slice too many poisons the row.  -> dict(g_vec, g_diff)."""
    from gotennet_amd import _lib
    lib = _lib.load()
    E, R, lmax, n_rl, n_cut = c["E"], c["R"], c["lmax"], c["n_rl"], c["n_cut"]
    D = G.ndim(lmax)
    _f32((c["vec"], 3 * E), (c["diff"], E), (c["p0"], R), (c["p1"], R), (c["g_rl"], n_rl * E * D), (c["g_cut"], n_cut * E),
         (c["g_phi"], E * R))
    _i32((c["src"], E), (c["dst"], E))
    if not expect_rc:
        assert not over and 1 <= lmax <= 8 and R > 0 and c["basis"] in (0, 1, 2) and n_rl >= 0 and n_cut >= 0
    dev = {k: _dev(c[k]) for k in ("vec", "diff", "src", "dst", "p0", "p1", "g_phi")}
    dev["g_rl"] = torch.cat([c["g_rl"].reshape(-1), torch.full((E * D + 1,), math.nan)]).cuda()
    dev["g_cut"] = torch.cat([c["g_cut"].reshape(-1), torch.full((E + 1,), math.nan)]).cuda()
    fn = lib.gn_edge_geometry_backward_images if c["images"] else lib.gn_edge_geometry_backward
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for _ in range(2):
        g_vec, g_diff = _padded(E, 3), _padded(E, 1)
        rc = fn(dev["vec"].data_ptr(), None if null_diff else dev["diff"].data_ptr(), dev["src"].data_ptr(), dev["dst"].data_ptr(),
                over.get("E", E), over.get("lmax", lmax), over.get("R", R), over.get("basis", c["basis"]), dev["p0"].data_ptr(),
                dev["p1"].data_ptr(), c["cutoff"], dev["g_rl"].data_ptr(), over.get("n_rl", n_rl), dev["g_cut"].data_ptr(),
                over.get("n_cut", n_cut), dev["g_phi"].data_ptr(), g_vec.data_ptr(), g_diff.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == expect_rc, rc
        outs = dict(g_vec=g_vec, g_diff=g_diff)
        _check_outputs(outs, dict(g_vec=E, g_diff=E), expect_rc)
        if expect_rc:
            return None
        res.append({k: t[:E].cpu() for k, t in outs.items()})
    for k in res[0]:
        assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), f"{k}: two launches differ"
    return dict(g_vec=res[0]["g_vec"], g_diff=res[0]["g_diff"][:, 0])


def _launch_scatter(s, expect_rc=0, **over):
    """The ONE place gn_pos_scatter's inputs reach the library.  -> g_pos [N, 3]."""
    from gotennet_amd import _lib
    lib = _lib.load()
    N, E = s["N"], s["E"]
    G.check_graph(s)
    _f32((s["g_vec"], 3 * E), (s["g_diff"], E), (s["vec"], 3 * E))
    _i32((s["rowptr"], N + 1), (s["colptr"], N + 1), (s["perm"], E))
    dev = {k: _dev(s[k]) for k in ("g_vec", "g_diff", "vec", "rowptr", "colptr", "perm")}
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for _ in range(2):
        out = _padded(N, 3)
        rc = lib.gn_pos_scatter(dev["g_vec"].data_ptr(), dev["g_diff"].data_ptr(), dev["vec"].data_ptr(), dev["rowptr"].data_ptr(),
                                dev["colptr"].data_ptr(), dev["perm"].data_ptr(), over.get("N", N), s["sign"], out.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == expect_rc, rc
        _check_outputs(dict(g_pos=out), dict(g_pos=N), expect_rc)
        if expect_rc:
            return None
        res.append(out[:N].cpu())
    assert torch.equal(_bits(res[0]), _bits(res[1])), "g_pos: two launches differ"
    return res[0]


def _note(lmax, rs):
    w = WORST.setdefault(lmax, {})
    for k, v in rs.items():
        w[k] = max(w.get(k, 0.0), v)


def _fmt(rs):
    return " ".join(f"{k}={v:.3f}" for k, v in rs.items())


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("n", CASES, ids=IDS)
def test_forward_within_bound(n):
    """rl, phi, cut per element on every case, through gn_edge_geometry AND gn_edge_geometry_images (each under its own loop
    rule: a self-image edge is a loop for the first and a real edge for the second)."""
    for images in (False, True):
        c = G.built(n, images)
        fr, _, fb, _ = G.reference(n, images)
        out = _launch_k1(c)
        rs = {k: G.ratio(out[k], fr[k], fb[k]) for k in ("rl", "phi", "cut")}
        print(f"{c['id']} images={images}: {_fmt(rs)}")
        _note(c["lmax"], rs)
        assert all(v <= 1.0 for v in rs.values()), rs
        if c["E"] == 0:
            continue
        gone = G.tag_mask(c, "at_cutoff", "above_cutoff", "beyond")
        assert bool((out["cut"][gone] == 0).all()), "cut is not exactly zero at / beyond the cutoff"
        if c["basis"] == 0:
            assert bool((out["phi"][gone] == 0).all())
        loop = G.loop_mask(c)
        zero_vec = c["vec"].abs().sum(1) == 0
        assert bool((out["rl"][loop & zero_vec] == 0).all()), "rl of a zero vector is not exactly zero"
        raw = loop & ~zero_vec                                               # a loop with a vector: the raw vector's polynomial
        if bool(raw.any()):
            want = orc.real_harmonics(c["lmax"], c["vec"].double()[raw])
            assert G.ratio(out["rl"][raw], want, fb["rl"][raw]) <= 1.0
            assert float((want[:, :3] - c["vec"].double()[raw]).abs().max()) == 0.0 and torch.equal(out["rl"][raw][:, :3], c["vec"][raw])


@pytest.mark.parametrize("lmax", [5, 6, 7, 8])
def test_harmonics_known_answers_per_element(lmax):
    """The known answers of degrees 5..8 (tests/golden/kat_sh_l8.npz), row by row: one wrong row among 80 fails."""
    k = np.load(os.path.join(GOLDEN_DIR, "kat_sh_l8.npz"))
    vec = torch.from_numpy(k["vec"])
    unit = torch.cat([vec[:32], vec[40:]])                                  # unit vectors, axes, zero
    want = torch.cat([torch.from_numpy(k[f"sh{lmax}"])[:32], torch.from_numpy(k[f"sh{lmax}"])[40:]])
    E, R = unit.shape[0], 8
    ev = (unit * torch.linspace(0.5, 3.0, E, dtype=torch.float64).unsqueeze(1)).float().contiguous()
    ev[-1] = 0.0
    src = torch.arange(E, dtype=torch.int32)
    dst = ((src + 1) % E).to(torch.int32)
    dst[-1] = src[-1]
    p0, p1 = G.basis_params(0, R, 5.0)
    c = dict(lmax=lmax, E=E, R=R, basis=0, cutoff=5.0, images=False, vec=ev, diff=ev.norm(dim=1).contiguous(), src=src, dst=dst, p0=p0, p1=p1)
    out = _launch_k1(c)
    ref, bnd = G.restate_forward(c), G.bounds(G.k1_forward(G.RE, c))
    r = G.ratio(out["rl"], ref["rl"], bnd["rl"])
    # the golden rows are harmonics of the exact unit vectors; the kernel normalises the rounded fp32 ones: the restatement on
    # the same fp32 input is the yardstick, the golden values pin the restatement (to the rounding of the scaled input)
    assert float((ref["rl"][:-1] - want[:-1]).abs().max()) < 1e-5
    print(f"kat l{lmax}: rl={r:.3f}")
    _note(lmax, {"rl": r})
    assert r <= 1.0 and float(out["rl"][-1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("n", CASES, ids=IDS)
def test_backward_within_bound(n):
    for images in (False, True):
        c = G.built(n, images)
        _, br, _, bb = G.reference(n, images)
        out = _launch_k1_bwd(c)
        rs = {k: G.ratio(out[k], br[k], bb[k]) for k in ("g_vec", "g_diff")}
        print(f"{c['id']} images={images}: {_fmt(rs)}")
        _note(c["lmax"], rs)
        assert all(v <= 1.0 for v in rs.values()), rs
        if c["E"] == 0:
            continue
        loop = G.loop_mask(c)
        assert bool((out["g_vec"][loop] == 0).all()) and bool((out["g_diff"][loop] == 0).all()), "a loop row is not exactly zero"
        gone = G.tag_mask(c, "at_cutoff", "above_cutoff", "beyond") & ~loop
        if c["basis"] == 0:                                                 # nothing but the cutoff reaches d: exactly zero
            assert bool((out["g_diff"][gone] == 0).all()) and bool((br["g_diff"][gone] == 0).all())
        elif not c["hostile"]:                                              # bases 1 and 2 still contribute (a narrow trained
            assert bool((br["g_diff"][gone] != 0).all())                    # Gaussian underflows to zero out there: as restated)
            assert bool((out["g_diff"][gone] != 0).any())
        # the cutoff's own contribution at d >= c, alone (G_phi = 0): exactly zero
        alone = _launch_k1_bwd(dict(c, g_phi=torch.zeros_like(c["g_phi"])))
        assert bool((alone["g_diff"][gone] == 0).all()), "the cutoff contributes to g_diff at / beyond the cutoff"


def test_table_reaches_both_vector_paths():
    assert {c["R"] % 4 == 0 for c in G.GEO_CASES} == {True, False}
    assert {G.ndim(c["lmax"]) % 4 == 0 for c in G.GEO_CASES} == {True, False}


# ------------------------------------------------------------------------------------------------ gn_pos_scatter
@pytest.mark.parametrize("N,sign,hub", G.SCATTER_CASES)
def test_pos_scatter_within_bound(N, sign, hub):
    s = G.scatter_case(N, sign, hub)
    out = _launch_scatter(s)
    r = G.ratio(out, G.restate_scatter(s), G.bound_scatter(s))
    print(f"{s['id']}: E={s['E']} g_pos={r:.3f}")
    _note(0, {"g_pos": r})
    assert r <= 1.0
    if N >= 4:
        assert bool((out[N - 1] == 0).all())                                # the isolated atom


# ------------------------------------------------------------------------------------------------ the chain
def _cluster(pbc):
    """Nine atoms on a 2^-8 grid (position differences and lattice shifts are exact in fp32), every pair inside the cutoff,
    one index self-loop; ``pbc``: a cubic cell of 4 (narrower than twice the cutoff) with shifted edges and a self-image."""
    g = torch.Generator().manual_seed(11)
    N, cutoff, L = 9, 5.0, 4.0
    pos = (torch.randint(0, int(3.5 * 256), (N, 3), generator=g).float() / 256.0).contiguous()
    pairs = []
    for i in range(N):
        for j in range(N):
            if i == j:
                continue
            sh = (0, 0, 0)
            if pbc and (i + j) % 3 == 0:
                sh = (1, 0, 0) if j > i else (-1, 0, 0)
            v = pos[j] - pos[i] + torch.tensor(sh).float() * L
            if 0 < float(v.norm()) < cutoff:
                pairs.append((j, i, sh))
    pairs.append((2, 2, (0, 0, 0)))                                         # the self-loop
    if pbc:
        pairs.append((4, 4, (0, 1, 0)))                                     # the atom's own image at |s @ cell| = 4
    pairs.sort(key=lambda p: p[1])
    src = torch.tensor([p[0] for p in pairs], dtype=torch.int32)
    dst = torch.tensor([p[1] for p in pairs], dtype=torch.int32)
    shift = torch.tensor([p[2] for p in pairs], dtype=torch.int32).contiguous()
    return N, cutoff, L, pos, src, dst, shift


@pytest.mark.parametrize("pbc", [False, True], ids=["open", "pbc-images"])
@pytest.mark.parametrize("basis", [0, 1, 2])
def test_chain_matches_autograd_of_positions(pbc, basis):
    """gn_edge_vectors[_pbc] -> gn_edge_geometry -> gn_edge_geometry_backward -> gn_pos_scatter with fixed cotangents against the
    fp64 autograd gradient of the same scalar with respect to the positions.  The bound is composed from the parts: the
    backward's bound per edge, the sensitivity of g_diff to the rounded distance (|d g_diff / dd| 4 u d: three products, two
    adds and a square root are below 4 u), both carried through the scatter, and the scatter's own bound."""
    from gotennet_amd import _lib
    lib = _lib.load()
    N, cutoff, L, pos, src, dst, shift = _cluster(pbc)
    E, lmax, R = src.numel(), 4, 7
    D = G.ndim(lmax)
    colptr, perm = G.csc_of(src, N)
    graph = dict(N=N, E=E, src=src, dst=dst, rowptr=G.rowptr_of(dst, N), colptr=colptr, perm=perm)
    G.check_graph(graph)
    dv = {k: _dev(t) for k, t in dict(pos=pos, src=src, dst=dst, shift=shift).items()}
    vec_d, diff_d = _padded(E, 3), _padded(E, 1)
    st = torch.cuda.current_stream().cuda_stream
    if pbc:
        cell = (torch.eye(3) * L).reshape(1, 3, 3).contiguous().cuda()
        batch = torch.zeros(N, dtype=torch.int64).cuda()
        rc = lib.gn_edge_vectors_pbc(dv["pos"].data_ptr(), dv["src"].data_ptr(), dv["dst"].data_ptr(), dv["shift"].data_ptr(),
                                     cell.data_ptr(), batch.data_ptr(), E, 1, vec_d.data_ptr(), diff_d.data_ptr(), st)
    else:
        rc = lib.gn_edge_vectors(dv["pos"].data_ptr(), dv["src"].data_ptr(), dv["dst"].data_ptr(), E, vec_d.data_ptr(),
                                 diff_d.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == 0 and bool((vec_d[E:] == SENTINEL).all()) and bool((diff_d[E:] == SENTINEL).all())
    vec, diff = vec_d[:E].cpu().contiguous(), diff_d[:E, 0].cpu().contiguous()
    p64 = pos.double()
    v64 = p64[src.long()] - p64[dst.long()] + shift.double() * L
    assert torch.equal(vec.double(), v64), "edge vectors on the grid are exact"
    d64 = v64.norm(dim=1)
    assert bool(((diff.double() - d64).abs() <= 4 * U32 * d64).all())
    g = torch.Generator().manual_seed(5 + basis)
    p0, p1 = G.basis_params(basis, R, cutoff)
    c = dict(lmax=lmax, E=E, R=R, basis=basis, n_rl=1, n_cut=1, images=pbc, cutoff=cutoff, vec=vec, diff=diff, src=src, dst=dst,
             p0=p0, p1=p1, g_rl=torch.randn(1, E, D, generator=g), g_cut=torch.randn(1, E, generator=g),
             g_phi=torch.randn(E, R, generator=g), tags=["x"] * E)
    keep = ~G.loop_mask(c)
    assert int((~keep).sum()) == 1 and (not pbc or int((src == dst).sum()) == 2)
    fwd = _launch_k1(c)
    fr, fb = G.restate_forward(c), G.bounds(G.k1_forward(G.RE, c))
    assert all(G.ratio(fwd[k], fr[k], fb[k]) <= 1.0 for k in ("rl", "phi", "cut"))
    bwd = _launch_k1_bwd(c)
    bb = G.bounds(G.k1_backward(G.RE, c))
    s = dict(graph, sign=1.0, vec=vec, g_vec=bwd["g_vec"].contiguous(), g_diff=bwd["g_diff"].contiguous())
    got = _launch_scatter(s)
    # the reference: autograd of the scalar with respect to the positions, and d g_diff / dd for the sensitivity term
    with torch.enable_grad():
        P = p64.clone().requires_grad_(True)
        V = (P[src.long()] - P[dst.long()] + shift.double() * L)[keep]
        Dd = V.norm(dim=1)
        S = (c["g_rl"][0].double()[keep] * orc.real_harmonics(lmax, V / Dd[:, None])).sum() \
            + (c["g_phi"].double()[keep] * G.basis_values(c, Dd)).sum() + (c["g_cut"][0].double()[keep] * orc.cosine_cutoff(Dd, cutoff)).sum()
        (want,) = torch.autograd.grad(S, P)
        dd = d64[keep].clone().requires_grad_(True)
        rad = (c["g_phi"].double()[keep] * G.basis_values(c, dd)).sum() + (c["g_cut"][0].double()[keep] * orc.cosine_cutoff(dd, cutoff)).sum()
        (g1,) = torch.autograd.grad(rad, dd, create_graph=True)
        (g2,) = torch.autograd.grad(g1.sum(), dd)
    e_diff = bb["g_diff"].clone()
    e_diff[keep] += g2.abs() * 4 * U32 * d64[keep]
    unit = torch.zeros(E, 3, dtype=torch.float64)
    unit[keep] = (v64[keep] / d64[keep, None]).abs()
    per_edge = bb["g_vec"] + e_diff[:, None] * unit * (1 + 8 * U32)
    per_edge[~keep] = 0.0
    carried = torch.zeros(N, 3, dtype=torch.float64).index_add_(0, src.long(), per_edge).index_add_(0, dst.long(), per_edge)
    br = G.restate_backward(dict(c, diff=d64.float()))                     # magnitudes for the scatter's own bound
    bound = G.bound_scatter(dict(s, g_vec=br["g_vec"].float(), g_diff=br["g_diff"].float())) + carried * (1 + 64 * U32)
    r = G.ratio(got, want, bound)
    print(f"chain {'pbc' if pbc else 'open'} basis {basis}: E={E} g_pos={r:.3f}")
    _note(lmax, {"chain": r})
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------ NaN confinement
def test_zero_length_edge_poisons_only_its_own_rows():
    """One zero-length edge between DISTINCT atoms: non-finite values in its own rows of K1 and the backward, and in its two
    endpoint atoms after the scatter; every other row and atom is finite and inside its bound."""
    src, dst = G.scatter_graph(9, 77)
    N, E = 9, src.numel()
    g = torch.Generator().manual_seed(3)
    vec = (torch.randn(E, 3, generator=g) * 1.2).contiguous()
    bad = int(((src != dst) & (dst == 3)).nonzero()[0])
    vec[src == dst] = 0.0
    vec[bad] = 0.0
    lmax, R = 3, 7
    D = G.ndim(lmax)
    p0, p1 = G.basis_params(1, R, 5.0)
    c = dict(lmax=lmax, E=E, R=R, basis=1, n_rl=1, n_cut=1, images=False, cutoff=5.0, vec=vec, diff=vec.norm(dim=1).contiguous(),
             src=src, dst=dst, p0=p0, p1=p1, g_rl=torch.randn(1, E, D, generator=g), g_cut=torch.randn(1, E, generator=g),
             g_phi=torch.randn(E, R, generator=g), tags=["x"] * E)
    rows = torch.ones(E, dtype=torch.bool)
    rows[bad] = False
    fwd, bwd = _launch_k1(c), _launch_k1_bwd(c)
    assert not bool(torch.isfinite(fwd["rl"][bad]).any()) and not bool(torch.isfinite(bwd["g_vec"][bad]).any())
    assert bool(torch.isfinite(fwd["cut"]).all()) and bool(torch.isfinite(fwd["phi"]).all())         # d = 0 divides by 1
    for k in ("rl",):
        assert bool(torch.isfinite(fwd[k][rows]).all())
    assert bool(torch.isfinite(bwd["g_vec"][rows]).all()) and bool(torch.isfinite(bwd["g_diff"][rows]).all())
    sub = {k: (v[rows] if torch.is_tensor(v) and v.shape[:1] == (E,) else v) for k, v in c.items()}
    sub.update(E=E - 1, g_rl=c["g_rl"][:, rows], g_cut=c["g_cut"][:, rows], tags=["x"] * (E - 1))
    br, bb = G.restate_backward(sub), G.bounds(G.k1_backward(G.RE, sub))
    assert G.ratio(bwd["g_vec"][rows], br["g_vec"], bb["g_vec"]) <= 1.0 and G.ratio(bwd["g_diff"][rows], br["g_diff"], bb["g_diff"]) <= 1.0
    colptr, perm = G.csc_of(src, N)
    s = dict(N=N, E=E, sign=-1.0, src=src, dst=dst, rowptr=G.rowptr_of(dst, N), colptr=colptr, perm=perm, vec=vec,
             g_vec=bwd["g_vec"].contiguous(), g_diff=bwd["g_diff"].contiguous())
    got = _launch_scatter(s)
    ends = torch.zeros(N, dtype=torch.bool)
    ends[int(src[bad])] = ends[int(dst[bad])] = True
    assert not bool(torch.isfinite(got[ends]).all(1).any()) and bool(torch.isfinite(got[~ends]).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    c = G.built(0)
    for over in (dict(E=-1), dict(lmax=0), dict(lmax=9), dict(R=0), dict(basis=3)):
        _launch_k1(c, expect_rc=BAD_ARG, **over)
        _launch_k1_bwd(c, expect_rc=BAD_ARG, **over)
    _launch_k1_bwd(c, expect_rc=BAD_ARG, n_rl=-1)
    _launch_k1_bwd(c, expect_rc=BAD_ARG, n_cut=-1)
    ci = G.built(0, True)
    _launch_k1(ci, expect_rc=BAD_ARG, null_diff=True, E=ci["E"])
    _launch_k1_bwd(ci, expect_rc=BAD_ARG, null_diff=True, E=ci["E"])
    s = G.scatter_case(3, -1.0, False)
    _launch_scatter(s, expect_rc=BAD_ARG, N=-1)


def test_empty_problems_write_nothing():
    n0 = [n for n in CASES if G.GEO_CASES[n]["E"] == 0][0]
    for images in (False, True):
        c = G.built(n0, images)
        out, bwd = _launch_k1(c), _launch_k1_bwd(c)                         # (the sentinel rows are checked inside)
        assert out["rl"].numel() == 0 and bwd["g_vec"].numel() == 0
    from gotennet_amd import _lib
    lib = _lib.load()
    buf = _padded(0, 3)
    assert lib.gn_pos_scatter(None, None, None, None, None, None, 0, 1.0, buf.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


def test_yardstick_rejects_wrong_device_results():
    """The power of the comparison ON the device: results of launches that differ from the case as a listed mutation does
    (a slice short, the other loop rule, the other sign) are outside the case's bound."""
    n = [i for i in CASES if G.GEO_CASES[i]["images"] and G.GEO_CASES[i]["n_cut"] >= 3 and G.GEO_CASES[i]["n_rl"] >= 1][0]
    c = G.built(n)
    _, br, _, bb = G.reference(n)
    short_cut = _launch_k1_bwd(dict(c, n_cut=c["n_cut"] - 1, g_cut=c["g_cut"][:-1].contiguous()))
    assert G.ratio(short_cut["g_diff"], br["g_diff"], bb["g_diff"]) > 1.0
    short_rl = _launch_k1_bwd(dict(c, n_rl=c["n_rl"] - 1, g_rl=c["g_rl"][:-1].contiguous()))
    assert G.ratio(short_rl["g_vec"], br["g_vec"], bb["g_vec"]) > 1.0
    index_rule = _launch_k1_bwd(G.built(n, False))                           # the self-image treated as a loop
    assert G.ratio(index_rule["g_vec"], br["g_vec"], bb["g_vec"]) > 1.0
    s = G.scatter_case(9, -1.0, False)
    flipped = _launch_scatter(dict(s, sign=1.0))
    assert G.ratio(flipped, G.restate_scatter(s), G.bound_scatter(s)) > 1.0


# ------------------------------------------------------------------------------------------------ summary
def test_worst_ratios():
    for lmax in sorted(WORST):
        print(f"{'scatter' if lmax == 0 else 'lmax %d' % lmax}: {_fmt(WORST[lmax])}")
    assert WORST and all(v <= 1.0 for w in WORST.values() for v in w.values())
