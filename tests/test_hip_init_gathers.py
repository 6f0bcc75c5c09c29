"""GPU: gn_node_init (K2), gn_edge_init (K3), gn_node_init_backward and gn_edge_init_backward (with the `_images` entry points)
called as engine._init_forward / _init_backward call them -- the node half of `feat` at offset 0, the edge half F floats in, one
leading dimension (here ldf = 2 F + 4 > 2 F) -- against the fp64 restatement and per-element bounds of tests/geometry_util.py,
and the cross-kernel contract: the g_cut slices NodeInit's backward writes are the slices gn_edge_geometry_backward adds."""
import math

import pytest
import torch

from tests import geometry_util as G
from tests.gather_util import slots
from tests.test_hip_geometry import PAD_ROWS, SENTINEL, _bits, _dev, _f32, _i32, _launch_k1_bwd, _padded

pytestmark = pytest.mark.gpu

WORST = {}
CASES = [(F, images) for F in G.INIT_F for images in (False, True)]


def _check_args(d):
    """Everything K2 / K3 and their backwards index with, asserted before any launch."""
    F, N, E, ldf = d["F"], d["N"], d["E"], d["ldf"]
    G.check_graph(d)
    assert F in G.INIT_F and N <= 12 and ldf % 4 == 0 and ldf > 2 * F
    _f32((d["feat"], E * ldf), (d["cut"], E), (d["diff"], E), (d["A_na"], G.MAX_Z * F), (d["A_nbr"], G.MAX_Z * F), (d["h"], N * F),
         (d["g_ctx"], N * 2 * F), (d["g_t"], E * F), (d["g_h0"], N * F))
    _i32((d["z"], N), (d["rowptr"], N + 1), (d["src"], E), (d["colptr"], N + 1), (d["perm"], E))
    assert 0 <= int(d["z"].min()) and int(d["z"].max()) < G.MAX_Z
    assert bool(torch.isnan(d["feat"][:, 2 * F:]).all())                    # the pad columns: an over-read poisons the result


def _launch_forward(d):
    """The ONE place K2 / K3 inputs reach the library.  Two launches, same bits.  -> dict(ctx [N, 2F], t [E, F])."""
    from gotennet_amd import _lib
    lib = _lib.load()
    F, N, E, ldf = d["F"], d["N"], d["E"], d["ldf"]
    _check_args(d)
    dev = {k: _dev(d[k]) for k in ("z", "rowptr", "src", "feat", "cut", "A_na", "A_nbr", "h", "diff")}
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for _ in range(2):
        ctx, t = _padded(N, 2 * F), _padded(E, F)
        head = (dev["z"].data_ptr(), dev["rowptr"].data_ptr(), dev["src"].data_ptr(), dev["feat"].data_ptr(), ldf,
                dev["cut"].data_ptr(), dev["A_na"].data_ptr(), dev["A_nbr"].data_ptr(), N, F)
        if d["images"]:
            rc = lib.gn_node_init_images(*head, dev["diff"].data_ptr(), ctx.data_ptr(), st)
        else:
            rc = lib.gn_node_init(*head, ctx.data_ptr(), st)
        assert rc == 0, rc
        rc = lib.gn_edge_init(dev["h"].data_ptr(), dev["rowptr"].data_ptr(), dev["src"].data_ptr(), dev["feat"].data_ptr() + 4 * F,
                              ldf, N, F, t.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert bool((ctx[N:] == SENTINEL).all()) and bool((t[E:] == SENTINEL).all()), "a row past the end was written"
        res.append(dict(ctx=ctx[:N].cpu(), t=t[:E].cpu()))
    for k in res[0]:
        assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), f"{k}: two launches differ"
    return res[0]


def _launch_backward(d):
    """The ONE place the init backwards' inputs reach the library: gn_edge_init_backward, then gn_node_init_backward into the
    same g_feat, as the engine does.  g_cut: max(1, F / 256) slices at stride E, one sentinel slice behind them; g_h starts
    from g_h0.  -> dict(g_feat [E, ldf], g_cut [wide, E], g_h [N, F])."""
    from gotennet_amd import _lib
    lib = _lib.load()
    F, N, E, ldf, W = d["F"], d["N"], d["E"], d["ldf"], G.wide(d["F"])
    _check_args(d)
    dev = {k: _dev(d[k]) for k in ("z", "rowptr", "src", "colptr", "perm", "feat", "cut", "A_nbr", "h", "diff", "g_ctx", "g_t")}
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for _ in range(2):
        g_feat, g_cut = _padded(E, ldf), _padded((W + 1) * E, 1)
        g_cut[W * E:] = SENTINEL                                            # slice W: the sentinel that must survive
        g_h = torch.cat([d["g_h0"], torch.full((PAD_ROWS, F), SENTINEL)]).cuda()
        rc = lib.gn_edge_init_backward(dev["g_t"].data_ptr(), dev["h"].data_ptr(), dev["feat"].data_ptr(), ldf, dev["rowptr"].data_ptr(),
                                       dev["src"].data_ptr(), dev["colptr"].data_ptr(), dev["perm"].data_ptr(), N, F,
                                       g_feat.data_ptr(), g_h.data_ptr(), st)
        assert rc == 0, rc
        head = (dev["g_ctx"].data_ptr(), dev["z"].data_ptr(), dev["feat"].data_ptr(), ldf, dev["cut"].data_ptr(),
                dev["A_nbr"].data_ptr(), dev["rowptr"].data_ptr(), dev["src"].data_ptr(), N, F)
        if d["images"]:
            rc = lib.gn_node_init_backward_images(*head, dev["diff"].data_ptr(), g_feat.data_ptr(), g_cut.data_ptr(), st)
        else:
            rc = lib.gn_node_init_backward(*head, g_feat.data_ptr(), g_cut.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert bool((g_feat[E:] == SENTINEL).all()) and bool((g_h[N:] == SENTINEL).all()), "a row past the end was written"
        assert bool((g_cut[W * E:] == SENTINEL).all()), "more than max(1, F / 256) slices of g_cut were written"
        assert bool(torch.isfinite(g_cut[:W * E]).all()), "fewer than max(1, F / 256) slices of g_cut were written"
        assert bool(torch.isnan(g_feat[:E, 2 * F:]).all()), "a pad column of g_feat was written"
        res.append(dict(g_feat=g_feat[:E].cpu(), g_cut=g_cut[:W * E, 0].cpu().view(W, E), g_h=g_h[:N].cpu()))
    for k in res[0]:
        assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), f"{k}: two launches differ"
    return res[0]


def _outputs(d, fwd, bwd):
    F = d["F"]
    return dict(ctx_m=fwd["ctx"][:, F:], t=fwd["t"], g_fn=bwd["g_feat"][:, :F], g_fe=bwd["g_feat"][:, F:2 * F],
                g_cut=bwd["g_cut"].double().sum(0), g_h=bwd["g_h"])


def _fmt(rs):
    return " ".join(f"{k}={v:.3f}" for k, v in rs.items())


@pytest.mark.parametrize("F,images", CASES, ids=lambda v: str(v))
def test_init_gathers_within_bound(F, images):
    d = G.init_case(F, images)
    val, bnd = G.restate_init(d)
    fwd, bwd = _launch_forward(d), _launch_backward(d)
    out = _outputs(d, fwd, bwd)
    assert torch.equal(_bits(fwd["ctx"][:, :F]), _bits(d["A_na"][d["z"].long()])), "ctx[:, :F] is not the embedding row"
    rs = {k: G.ratio(out[k], val[k], bnd[k]) for k in bnd}
    print(f"{d['id']}: N={d['N']} E={d['E']} degs={d['degs']} ns={slots(F)} " + _fmt(rs))
    w = WORST.setdefault(F, {})
    for k, v in rs.items():
        w[k] = max(w.get(k, 0.0), v)
    assert all(v <= 1.0 for v in rs.values()), rs
    loop = G.loop_mask(d)
    same = d["src"] == d["dst"]
    assert int(loop.sum()) > 0 and (not images or int((same & ~loop).sum()) > 0)
    assert bool((out["g_fn"][loop] == 0).all()) and bool((bwd["g_cut"][:, loop] == 0).all()), "a loop row of the node half is not zero"
    assert bwd["g_cut"].shape[0] == max(1, F // 256)


@pytest.mark.parametrize("F", [256, 1024])
@pytest.mark.parametrize("images", [False, True], ids=["index", "images"])
def test_g_cut_slices_feed_the_geometry_backward(F, images):
    """The contract between the two kernels: the slices node_init_bwd_kernel writes at stride rowptr[N], passed with their count
    as n_cut, give the g_diff of fp64.  Bound: the geometry backward's own (on the device's slices) + the slices' bound times
    |d cut / dd|."""
    d = G.init_case(F, images)
    val, bnd = G.restate_init(d)
    slices = _launch_backward(d)["g_cut"].contiguous()
    E, W, cutoff = d["E"], G.wide(F), 5.0
    g = torch.Generator().manual_seed(F)
    vec = torch.nn.functional.normalize(torch.randn(E, 3, generator=g), dim=1) * d["diff"][:, None]
    c = dict(lmax=1, E=E, R=1, basis=0, n_rl=0, n_cut=W, images=images, cutoff=cutoff, vec=vec.contiguous(), diff=d["diff"],
             src=d["src"], dst=d["dst"], p0=torch.zeros(1), p1=torch.ones(1), g_rl=torch.zeros(0, E, 3), g_cut=slices,
             g_phi=torch.zeros(E, 1), tags=["x"] * E)
    out = _launch_k1_bwd(c)
    ref = G.restate_backward(dict(c, n_cut=1, g_cut=val["g_cut"][None]))
    dd = d["diff"].double()
    dc = (0.5 * math.pi / cutoff * torch.sin(dd * math.pi / cutoff)).abs() * (dd < cutoff)
    bound = G.bounds(G.k1_backward(G.RE, c))["g_diff"] + bnd["g_cut"] * dc * (1 + 1e-6)
    r = G.ratio(out["g_diff"], ref["g_diff"], bound)
    print(f"F{F} images={images}: n_cut={W} g_diff={r:.3f}")
    WORST.setdefault(F, {})["contract"] = max(WORST.get(F, {}).get("contract", 0.0), r)
    assert r <= 1.0 and bool((ref["g_diff"] != 0).any())
    assert bool((out["g_diff"][G.loop_mask(c)] == 0).all())


@pytest.mark.parametrize("F", [64, 512])
def test_relabelled_atoms_give_relabelled_results(F):
    """A random permutation of the atoms, edges re-sorted target-major: the permuted results, within the two bounds (the
    order of a sum changes with the labels, its value does not)."""
    d = G.init_case(F, True)
    _, bnd = G.restate_init(d)
    d2, old_of_new, emap = G.relabel_init(d)
    _, bnd2 = G.restate_init(d2)
    a = _outputs(d, _launch_forward(d), _launch_backward(d))
    b = _outputs(d2, _launch_forward(d2), _launch_backward(d2))
    rs = {}
    for k in bnd:
        m = old_of_new if k in ("ctx_m", "g_h") else emap
        rs[k] = G.ratio(b[k], a[k][m], bnd[k][m] + bnd2[k])
    print(f"F{F} relabelled: " + _fmt(rs))
    assert all(v <= 1.0 for v in rs.values()), rs


def test_no_atoms_write_nothing():
    """N = 0 returns OK from all six entry points before any launch."""
    from gotennet_amd import _lib
    lib = _lib.load()
    F, ldf = 64, 132
    st = torch.cuda.current_stream().cuda_stream
    bufs = [_padded(0, w) for w in (2 * F, F, ldf, 1, F)]
    ctx, t, g_feat, g_cut, g_h = (b.data_ptr() for b in bufs)
    head = (None, None, None, None, ldf, None, None, None, 0, F)
    assert lib.gn_node_init(*head, ctx, st) == 0 and lib.gn_node_init_images(*head, None, ctx, st) == 0
    assert lib.gn_edge_init(None, None, None, None, ldf, 0, F, t, st) == 0
    assert lib.gn_edge_init_backward(None, None, None, ldf, None, None, None, None, 0, F, g_feat, g_h, st) == 0
    bhead = (None, None, None, ldf, None, None, None, None, 0, F)
    assert lib.gn_node_init_backward(*bhead, g_feat, g_cut, st) == 0
    assert lib.gn_node_init_backward_images(*bhead, None, g_feat, g_cut, st) == 0
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs)


def test_worst_ratios():
    for F in sorted(WORST):
        print(f"F {F}: " + _fmt(WORST[F]))
    assert WORST and all(v <= 1.0 for w in WORST.values() for v in w.values())
