"""K-segmented A operand whose segments have leading dimensions of their own (``lda2`` of gn_gemm_desc) and the launch built
on it: dL/dt of a layer with an edge update as ONE product over the concatenated K of g_eproj and g_pre_t
(``engine.DT_KCAT``).  Projections against fp64 products with the bound of the other projection tests (2e-6 of the output's
max-norm); the force backward against itself with the switch off."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ("f32", "split", "f16x2")
NAN = float("nan")


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _r(g):
    return lambda *s: torch.randn(*s, device="cuda", generator=g)


def dd(t):
    return t.double()


def _padded(r, M, used, ld, scale=1.0):
    """[M, ld] with ``used`` live columns; the rest holds NaN: a kernel that reads past its segment shows up in the result."""
    t = torch.full((M, ld), NAN, device="cuda")
    t[:, :used] = r(M, used) * scale
    return t


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,N", [(130, 256), (300, 64), (130, 64), (300, 256)])
def test_two_segments_two_leading_dimensions(mode, M, N):
    """C = res + A[:, :a_seg] W0^T + A2 W1^T: A a strided view (lda 1536, the 1024-column prefix a first layer uses), A2 dense
    or strided, 256 or 32 columns wide (K = 1280: the panel kernel's chunk walk in f16x2; K = 1056: the slab kernels),
    the segments six decades apart in both orders (the f16x2 block exponent grows at the boundary, or does not)."""
    from gotennet_amd import engine
    g = torch.Generator(device="cuda").manual_seed(1000 * M + N)
    r = _r(g)
    seg = 1024
    for w2, lda2 in ((256, 256), (256, 320), (32, 256), (32, 320)):
        for s1, s2 in ((1e3, 1e-3), (1e-3, 1e3), (1.0, 1.0)):
            A, A2 = _padded(r, M, seg, 1536, s1), _padded(r, M, w2, lda2, s2)
            W, res, C = r(N, seg + w2) / 8, r(M, N) * min(s1, s2), torch.empty(M, N, device="cuda")
            engine.gemm_group([dict(A=A, lda=1536, A2=A2, lda2=lda2, a_seg=seg, W=W, C=C, ldc=N, rows=M, nout=N,
                                    K=seg + w2, res=res)], mode=mode)
            ref = dd(res) + dd(A[:, :seg]) @ dd(W[:, :seg]).T + dd(A2[:, :w2]) @ dd(W[:, seg:]).T
            e = rel_err(C, ref)
            print(f"{mode} M={M} N={N} w2={w2} lda2={lda2} scales=({s1:g}, {s2:g}): rel_err {e:.2e}")
            assert e < 2e-6, (w2, lda2, s1, s2, e)


@pytest.mark.parametrize("mode", MODES)
def test_two_segments_big_tiles_ragged_last_tile(mode):
    """M = 58 000 = 453 x 128 + 16, N = 256: 908 tiles of 128 x 128, the big-tile instantiation with the branch-free fetch two
    slabs ahead; K = 64 + 32, so the segment changes between the slabs in flight."""
    from gotennet_amd import engine
    g = torch.Generator(device="cuda").manual_seed(58)
    r = _r(g)
    M, N, seg, w2 = 58000, 256, 64, 32
    A, A2 = _padded(r, M, seg, 96), _padded(r, M, w2, 40, 1e2)
    W, res, C = r(N, seg + w2) / 8, r(M, N), torch.empty(M, N, device="cuda")
    engine.gemm_group([dict(A=A, lda=96, A2=A2, lda2=40, a_seg=seg, W=W, C=C, ldc=N, rows=M, nout=N, K=seg + w2, res=res)],
                      mode=mode)
    ref = dd(res) + dd(A[:, :seg]) @ dd(W[:, :seg]).T + dd(A2[:, :w2]) @ dd(W[:, seg:]).T
    e = rel_err(C, ref)
    print(f"{mode} big tiles: rel_err {e:.2e}")
    assert e < 2e-6
    assert rel_err(C[-16:], ref[-16:]) < 2e-6      # the ragged last row tile


@pytest.mark.parametrize("mode", MODES)
def test_lda2_zero_is_lda(mode):
    """lda2 = 0 means lda: the three-segment, row-mapped X-gradient product gives the same bits either way."""
    from gotennet_amd import engine
    g = torch.Generator(device="cuda").manual_seed(7)
    r = _r(g)
    n, D, Fd = 500, 8, 256
    X0, X1, X2 = r(n, D, Fd), r(n, D, Fd) * 1e3, r(n, D, Fd) * 1e-3
    Wc, Rr = r(Fd, 3 * Fd) / 8, r(n, D, Fd)
    outs = []
    for lda2 in (0, Fd):
        Cc = torch.zeros(n, D, Fd, device="cuda")
        engine.gemm_group([dict(A=X0, A2=X1, A3=X2, a_seg=Fd, lda=Fd, lda2=lda2, W=Wc, C=Cc, ldc=Fd, rows=n * 3, nout=Fd,
                                K=3 * Fd, rowmap=(3, D, 0), res=Rr),
                           dict(A=X0, A2=X1, A3=X2, a_seg=Fd, lda=Fd, lda2=lda2, W=Wc, C=Cc, ldc=Fd, rows=n * 5, nout=Fd,
                                K=3 * Fd, rowmap=(5, D, 3), res=Rr)], mode=mode)
        outs.append(Cc)
    ref = dd(Rr) + dd(X0) @ dd(Wc)[:, :Fd].T + dd(X1) @ dd(Wc)[:, Fd:2 * Fd].T + dd(X2) @ dd(Wc)[:, 2 * Fd:].T
    assert rel_err(outs[0], ref) < 2e-6
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("mode", MODES)
def test_four_problem_group_one_molecule(mode):
    """The input-gradient group of a one-molecule call: the fused dL/dt problem (K = 1536 + 256, M = 429) and its three
    riders (K = 1280, 1280, 512; M = 21).  In f16x2 the panel kernel walks 256-deep chunks and the segment boundary falls
    between the sixth and the seventh."""
    from gotennet_amd import engine
    g = torch.Generator(device="cuda").manual_seed(429)
    r = _r(g)
    E, Na, F = 429, 21, 256
    ge, gp = r(E, 1536), _padded(r, E, F, F, 30.0)
    Wdt, gt, C = r(F, 1792) / 8, r(E, F), torch.empty(E, F, device="cuda")
    gx, gv, Ws, Wv = r(Na, 1280), r(Na, 1280), r(F, 1280) / 8, r(F, 1280) / 8
    gn, pre_n = torch.zeros(Na, 4 * F, device="cuda"), r(Na, 4 * F)
    gq, Wqk, Rq, Dq = r(Na, 512), r(F, 512) / 8, r(Na, F), torch.empty(Na, F, device="cuda")
    engine.gemm_group([dict(A=ge, lda=1536, A2=gp, lda2=F, a_seg=1536, W=Wdt, C=C, ldc=F, rows=E, nout=F, K=1792, res=gt),
                       dict(A=gx, lda=1280, W=Ws, C=gn, ldc=4 * F, rows=Na, nout=F, K=1280, c_off=2 * F, dgate=pre_n, g_off=2 * F),
                       dict(A=gv, lda=1280, W=Wv, C=gn, ldc=4 * F, rows=Na, nout=F, K=1280, c_off=3 * F, dgate=pre_n, g_off=3 * F),
                       dict(A=gq, lda=512, W=Wqk, C=Dq, ldc=F, rows=Na, nout=F, K=512, res=Rq)], mode=mode)
    assert rel_err(C, dd(gt) + dd(ge) @ dd(Wdt[:, :1536]).T + dd(gp) @ dd(Wdt[:, 1536:]).T) < 2e-6
    ds = lambda x: torch.sigmoid(x) * (1 + x * (1 - torch.sigmoid(x)))
    assert rel_err(gn[:, 2 * F:3 * F], (dd(gx) @ dd(Ws).T) * ds(dd(pre_n[:, 2 * F:3 * F]))) < 2e-6
    assert rel_err(gn[:, 3 * F:], (dd(gv) @ dd(Wv).T) * ds(dd(pre_n[:, 3 * F:]))) < 2e-6
    assert float(gn[:, :2 * F].abs().max()) == 0.0
    assert rel_err(Dq, dd(Rq) + dd(gq) @ dd(Wqk).T) < 2e-6


@pytest.mark.parametrize("lmax", [2, 1])
def test_forces_kcat_against_two_launches(lmax):
    """Two aspirin molecules, F = 256, two interactions (the first one: zero X_in, the K-prefix of g_eproj, and the model's only
    edge update): forces with the K-concatenated dL/dt launch against the two-launch sequence, and twice for the same bits."""
    import gotennet_amd
    from gotennet_amd import engine, synthetic
    from gotennet_amd.graph import distance
    from gotennet_amd.outputs import Atomwise
    from gotennet_amd.pipeline import EnergyForces
    dev = "cuda"
    torch.manual_seed(21)
    rep = gotennet_amd.GotenNet(n_atom_basis=256, n_interactions=2, n_rbf=16, cutoff_fn=gotennet_amd.CosineCutoff(5.0),
                                num_heads=8, scale_edge=True, lmax=lmax, sep_dir=True, sep_tensor=True).to(dev).eval()
    head = Atomwise(n_in=256, n_hidden=128, derivative="forces", activation="silu").to(dev).eval()
    ef = EnergyForces(rep, head)
    pos, batch, z = synthetic.make_batch("rmd17_aspirin", 2, seed=4)
    pos, batch, z = pos.to(dev), batch.to(dev), z.to(dev)
    ei, ed, ev = distance(pos, batch, 5.0, 32)
    assert engine.DT_KCAT
    run = lambda: tuple(t.clone() for t in ef(z, ei, ed, ev, batch, 2))
    e_on, f_on = run()
    e_on2, f_on2 = run()
    engine.DT_KCAT = False
    try:
        e_off, f_off = run()
    finally:
        engine.DT_KCAT = True
    assert torch.equal(e_on, e_on2) and torch.equal(f_on, f_on2)
    assert torch.equal(e_on, e_off)                # the forward does not know the switch
    err = rel_err(f_on, f_off)
    print(f"lmax {lmax}: forces, one launch against two: rel_err {err:.2e}")
    assert float(f_off.abs().max()) > 0 and err < 2e-6
