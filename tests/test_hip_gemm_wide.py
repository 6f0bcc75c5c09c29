"""The 1 x 8-wave form of the f16x2 slab kernel (gn_gemm.hip: 128 x 256 tile, 512 threads, an A slab scaled and split once per
row panel) held against the four-wave 128 x 128 form of the same build and against fp64 products, both forms forced through
gn_gemm_group_f16x2_form at shapes of a few hundred rows.

The eight staging waves keep one block exponent each, so 16 rows share an exponent where the four-wave form has 32 (the kernel
comment says why).  What the two forms share bit for bit is everything else: with operands whose magnitudes lie in ONE binade
every block exponent of every slab is the same in both forms, so the split, the products and the accumulation order are the
same and the outputs must be equal bits.  With general operands each form is held to the per-row bound of
tests/test_hip_parity.py::test_fp16_block_exponent_per_row_bound with ITS row grouping; the factor 32 ~ 2 sqrt(256) of that
test is 2 sqrt(K) here."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BIG, BIG8 = 1, 2                                   # GN_GEMM_FORM_*
GROUPS = {BIG: lambda r: (r // 128) * 4 + (r % 32) // 8,          # (row panel, staging wave): rows that share an exponent
          BIG8: lambda r: (r // 128) * 8 + (r % 64) // 8}


def _gen(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return g, (lambda *s: torch.randn(*s, device="cuda", generator=g))


def _one_binade(t, g):
    """Same signs, magnitudes in [1, 2)."""
    return torch.sign(t) * (1.0 + torch.rand(t.shape, device="cuda", generator=g))


def _problem(M, N, case, r, scale=lambda t: t):
    """-> (argument dict without C, fp64 product, |A| row maximum).  The leading problems of the input-gradient launches."""
    dd = lambda t: t.double()
    if case == "kcat1792":                         # K = 1536 + 256: a second A tensor with a leading dimension of its own
        A, A2, W = scale(r(M, 1536)), scale(r(M, 320)), r(N, 1792) / 8
        q = dict(A=A, lda=1536, A2=A2, lda2=320, a_seg=1536, W=W, rows=M, nout=N, K=1792)
        prod = dd(A) @ dd(W)[:, :1536].T + dd(A2)[:, :256] @ dd(W)[:, 1536:].T
        amax = torch.maximum(A.abs().amax(1), A2[:, :256].abs().amax(1))
    elif case == "prefix1280":                     # K = 1024 + 256: a K-prefix of rows that are 1536 wide
        A, A2, W = scale(r(M, 1536)), scale(r(M, 256)), r(N, 1280) / 8
        q = dict(A=A, lda=1536, A2=A2, lda2=256, a_seg=1024, W=W, rows=M, nout=N, K=1280)
        prod = dd(A)[:, :1024] @ dd(W)[:, :1024].T + dd(A2) @ dd(W)[:, 1024:].T
        amax = torch.maximum(A[:, :1024].abs().amax(1), A2.abs().amax(1))
    else:                                          # K = 96: three slabs (first, steady state, peeled last)
        A, W = scale(r(M, 96)), r(N, 96) / 8
        q = dict(A=A, lda=96, W=W, rows=M, nout=N, K=96)
        prod = dd(A) @ dd(W).T
        amax = A.abs().amax(1)
    return q, prod, amax.double()


def _run(q, form, ldc=None, **extra):
    from gotennet_amd import engine
    ldc = ldc or q["nout"]
    C = torch.full((q["rows"], ldc), float("nan"), device="cuda")
    engine.gemm_group([dict(q, C=C, ldc=ldc, **extra)], mode="f16x2", form=form)
    return C[:, :q["nout"]]


def _row_err_over_bound(C, ref, prod, amax, K, form):
    """max_n |C - ref| per row over its bound: 2 sqrt(K) max(2^-23, 2^(d - 41)) max_n |prod| (d = log2 of the exponent group's
    maximum over the row's own) + 2^-23 max_n |ref| for the residual's add."""
    M = C.shape[0]
    group = GROUPS[form](torch.arange(M, device="cuda"))
    gmax = torch.zeros(int(group.max()) + 1, dtype=torch.float64, device="cuda").scatter_reduce_(
        0, group, amax, "amax", include_self=True)[group]
    d = torch.log2(gmax / amax.clamp_min(1e-300))
    bound = 2.0 * math.sqrt(K) * torch.maximum(torch.full_like(d, 2.0 ** -23), 2.0 ** (d - 41)) * prod.abs().amax(1) \
        + 2.0 ** -23 * ref.abs().amax(1)
    err = (C.double() - ref).abs().amax(1)
    return err / bound.clamp_min(1e-300), d


@pytest.mark.parametrize("case", ["kcat1792", "prefix1280", "k96"])
@pytest.mark.parametrize("N", [256, 160])
@pytest.mark.parametrize("M", [1, 127, 129, 300])
def test_wide_form_partial_panels(M, N, case):
    """Partial and several row panels, a partial last wave (N = 160), two A tensors, `res` set, a padded output row."""
    g, r = _gen(1000 * M + N + len(case))
    res = r(M, N)
    # one binade: both forms must give the same bits
    q, prod, _ = _problem(M, N, case, r, lambda t: _one_binade(t, g))
    res_p = torch.nn.functional.pad(res, (0, 8))
    c4, c8 = _run(q, BIG, ldc=N + 8, res=res_p), _run(q, BIG8, ldc=N + 8, res=res_p)
    assert torch.equal(c4, c8)
    ref = res.double() + prod
    assert float((c8.double() - ref).abs().max() / ref.abs().max()) < 2e-6
    # general operands, rows spread over four decades: each form within the per-row bound of its own row grouping
    dec = torch.randint(-4, 1, (M, 1), device="cuda", generator=g).float()
    q, prod, amax = _problem(M, N, case, r, lambda t: t * 10.0 ** dec)
    res = (res * amax[:, None].float()).contiguous()                  # a residual of the row's own scale
    ref = res.double() + prod
    for form in (BIG, BIG8):
        C = _run(q, form, res=res)
        ratio, _ = _row_err_over_bound(C, ref, prod, amax, q["K"], form)
        print(f"M {M} N {N} {case} form {form}: max err / bound {float(ratio.max()):.3f}")
        assert float(ratio.max()) <= 1.0


def test_wide_form_riders():
    """A group as the backward issues it: the leading product, two `dgate` riders writing column blocks of one tensor and a plain
    rider with a residual, every problem tiled by 256 columns."""
    from gotennet_amd import engine
    g, r = _gen(7)
    dd = lambda t: t.double()
    ob = lambda t: _one_binade(t, g)
    E, Na, F = 300, 141, 256
    G0, P0, W0, R0 = ob(r(E, 1536)), ob(r(E, F)), r(F, 1792) / 8, r(E, F)
    gx, gv, Ws, Wv = ob(r(Na, 1280)), ob(r(Na, 1280)), r(F, 1280) / 8, r(F, 1280) / 8
    pre_n = r(Na, 4 * F)
    gq, Wqk, Rq = ob(r(Na, 512)), r(F, 512) / 8, r(Na, F)
    out = {}
    for form in (BIG, BIG8):
        D0, gn, Dq = torch.empty(E, F, device="cuda"), torch.zeros(Na, 4 * F, device="cuda"), torch.empty(Na, F, device="cuda")
        engine.gemm_group([
            dict(A=G0, lda=1536, A2=P0, lda2=F, a_seg=1536, W=W0, C=D0, ldc=F, rows=E, nout=F, K=1792, res=R0),
            dict(A=gx, lda=1280, W=Ws, C=gn, ldc=4 * F, rows=Na, nout=F, K=1280, c_off=2 * F, dgate=pre_n, g_off=2 * F),
            dict(A=gv, lda=1280, W=Wv, C=gn, ldc=4 * F, rows=Na, nout=F, K=1280, c_off=3 * F, dgate=pre_n, g_off=3 * F),
            dict(A=gq, lda=512, W=Wqk, C=Dq, ldc=F, rows=Na, nout=F, K=512, res=Rq)], mode="f16x2", form=form)
        out[form] = (D0, gn, Dq)
    for a, b in zip(out[BIG], out[BIG8]):
        assert torch.equal(a, b)
    D0, gn, Dq = out[BIG8]
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    ds = lambda x: torch.sigmoid(x) * (1 + x * (1 - torch.sigmoid(x)))
    assert rel(D0, dd(R0) + dd(G0) @ dd(W0)[:, :1536].T + dd(P0) @ dd(W0)[:, 1536:].T) < 2e-6
    assert rel(gn[:, 2 * F:3 * F], (dd(gx) @ dd(Ws).T) * ds(dd(pre_n[:, 2 * F:3 * F]))) < 2e-6
    assert rel(gn[:, 3 * F:], (dd(gv) @ dd(Wv).T) * ds(dd(pre_n[:, 3 * F:]))) < 2e-6
    assert float(gn[:, :2 * F].abs().max()) == 0.0
    assert rel(Dq, dd(Rq) + dd(gq) @ dd(Wqk).T) < 2e-6


@pytest.mark.parametrize("form", [BIG, BIG8])
def test_wide_form_exponent_changes_and_rescale(form):
    """Columns that grow by 2^6 every 256 (the running block exponent rises six times along K: the accumulators are rescaled),
    one row scaled by 2^40 and one by 2^-40 inside a panel.  Every row stays within the per-row bound of the form's row grouping:
    the rows beside the large one lose bits, rows of every other exponent group keep all of theirs."""
    g, r = _gen(40 + form)
    M, N, K = 300, 256, 1792
    A = r(M, K) * (2.0 ** (6 * (torch.arange(K, device="cuda") // 256))).float()
    A[133] *= 2.0 ** 40
    A[150] *= 2.0 ** -40
    W = r(N, K) / 8
    q = dict(A=A, lda=K, W=W, rows=M, nout=N, K=K)
    prod, amax = A.double() @ W.double().T, A.abs().amax(1).double()
    C = _run(q, form)
    ratio, d = _row_err_over_bound(C, prod, prod, amax, K, form)
    print(f"form {form}: max err / bound {float(ratio.max()):.3f}; rows with d > 30: {int((d > 30).sum())}")
    assert float(ratio.max()) <= 1.0
    assert int((d > 30).sum()) == (32 if form == BIG else 16)          # row 150 and the neighbours of row 133 in its exponent group
    near = d <= 18
    err = (C.double() - prod).abs().amax(1) / prod.abs().amax(1)
    assert float(err[near].max()) < 2.0 * math.sqrt(K) * 2.0 ** -23


@pytest.mark.parametrize("form", [BIG, BIG8])
def test_wide_form_inf_row(form):
    """One row holds an Inf: only that row turns non-finite (block_exponent scans the block again for its finite maximum)."""
    g, r = _gen(50 + form)
    M, N, K = 300, 256, 1792
    A, W = r(M, K), r(N, K) / 8
    A[200, 1000] = float("inf")
    C = _run(dict(A=A, lda=K, W=W, rows=M, nout=N, K=K), form)
    assert not torch.isfinite(C[200]).any()
    keep = torch.ones(M, dtype=torch.bool, device="cuda")
    keep[200] = False
    assert torch.isfinite(C[keep]).all()
    ref = A[keep].double() @ W.double().T
    assert float((C[keep].double() - ref).abs().max() / ref.abs().max()) < 2e-6


def test_wide_form_routing():
    """The routed launch of an edge-sized group (>= 900 tiles of 128 x 128) with N = 256: the eight-wave form from K = 1024 up,
    the four-wave form below.  Rows spread over decades make the two forms' bits differ."""
    from gotennet_amd import engine
    g, r = _gen(3)
    M, N = 57600, 256
    dec = torch.randint(-6, 1, (M, 1), device="cuda", generator=g).float()
    A = r(M, 1024) * 10.0 ** dec
    for K, routed in ((1024, BIG8), (992, BIG)):
        W = r(N, K) / 8
        q = dict(A=A, lda=1024, W=W, rows=M, nout=N, K=K)
        c = {form: _run(q, form) for form in (0, BIG, BIG8)}
        assert not torch.equal(c[BIG], c[BIG8])
        assert torch.equal(c[0], c[routed])
