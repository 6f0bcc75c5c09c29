"""GPU: gn_message_aggregate and gn_htr_edge called directly, every kernel form the launchers can select, against the fp64
restatement and the a-priori per-element bound of tests/gather_util.py (proved on the CPU by tests/test_gather_host.py).
Each case prints the kernel form it selects and the worst error / bound; the last test prints the worst per form."""
import math

import pytest
import torch

from tests import gather_util as U

pytestmark = pytest.mark.gpu

PAD_ROWS = 8                                       # sentinel rows past N (K6) / E (K7) in every output array
SENTINEL = 12345.678
WORST = {}                                         # kernel form -> worst error / bound seen by this module
#: whether the degree-sliced kernels reproduce the tuned kernels' bits (measured on MI355X, then pinned): K6 on every case;
#: K7 where the tuned kernel uses the closed form (lmax >= 3, every `mode`), not against the literal form of lmax <= 2
SLICED_BITS_EQUAL = {"msg": True, "htr_closed": True, "htr_literal": False}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_graph(d):
    N, E, rp = d["N"], d["E"], d["rowptr"]
    assert rp.dtype == torch.int32 and d["src"].dtype == torch.int32 and rp.is_contiguous() and d["src"].is_contiguous()
    assert rp.numel() == N + 1 and d["src"].numel() == E
    assert int(rp[0]) == 0 and int(rp[-1]) == E and bool((rp[1:] >= rp[:-1]).all())
    assert E == 0 or (0 <= int(d["src"].min()) and int(d["src"].max()) < N)


def _launch_k6(d, expect_rc=0, lmax_arg=None, H=None, F=None, ldxv=None, ldt=None, alias_X=False, null_X=False):
    """The ONE place K6 inputs reach the library.  Everything the kernels index with is asserted here, before any launch: a
    wrong argument would be a device fault, not a failing test.  Launches twice (the second into fresh arrays): same bits;
    the sentinel rows past N keep theirs.  -> [N, 1 + D, F] on the CPU, row 0 = h_out.  ``expect_rc`` != 0: a refusal --
    returns after the ONE call, having checked that no output element was written; the other keywords override the
    arguments for those."""
    from gotennet_amd import _lib
    lib = _lib.load()
    S, Fd, N, E = d["S"], d["F"], d["N"], d["E"]
    M, D = S.M, S.D
    _check_graph(d)
    f32 = [d["xbuf"], d["vbuf"], d["tbuf"], d["a"], d["rl"], d["cut"], d["h_in"]] + ([] if d["X_in"] is None else [d["X_in"]])
    for t in f32:
        assert t.dtype == torch.float32 and t.is_contiguous()
    # a row is read at [row * ld, row * ld + M F): the last one must end inside its buffer (t_filter starts at column F)
    assert d["ldxv"] >= M * Fd and d["ldt"] >= M * Fd and d["ldxv"] % 4 == 0 and d["ldt"] % 4 == 0
    assert (N - 1) * d["ldxv"] + M * Fd <= d["xbuf"].numel() and (N - 1) * d["ldxv"] + M * Fd <= d["vbuf"].numel()
    assert E == 0 or Fd + (E - 1) * d["ldt"] + M * Fd <= d["tbuf"].numel()
    assert d["a"].numel() == E * d["H"] and d["rl"].numel() == E * D and d["cut"].numel() == E
    assert d["h_in"].numel() == N * Fd and (d["X_in"] is None or d["X_in"].numel() == N * D * Fd)
    if expect_rc == 0:
        assert lmax_arg is None and H is None and F is None and ldxv is None and ldt is None and not alias_X and not null_X
        assert U.head_ok(M, Fd, d["H"]) and Fd in (16, 32, 64, 128, 256, 512, 1024)
        assert (d["lmax_arg"] & 0xff) == S.lmax and (d["X_in"] is not None or not U.use_highl(S.lmax, d["lmax_arg"] & ~0xff))
    dev = {k: d[k].cuda() for k in ("xbuf", "vbuf", "tbuf", "a", "rl", "cut", "h_in", "rowptr", "src")}
    X_in = None if d["X_in"] is None else d["X_in"].cuda()
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for _ in range(2):
        h_out = torch.full((N + PAD_ROWS, Fd), SENTINEL, device="cuda")
        X_out = torch.full((N + PAD_ROWS, D, Fd), SENTINEL, device="cuda")
        h_out[:N], X_out[:N] = math.nan, math.nan   # an element the kernel skips fails every bound
        x_in_ptr = X_out.data_ptr() if alias_X else (None if (X_in is None or null_X) else X_in.data_ptr())
        rc = lib.gn_message_aggregate(
            dev["xbuf"].data_ptr(), dev["vbuf"].data_ptr(), d["ldxv"] if ldxv is None else ldxv,
            dev["tbuf"].data_ptr() + 4 * Fd, d["ldt"] if ldt is None else ldt, dev["a"].data_ptr(), dev["rl"].data_ptr(),
            dev["cut"].data_ptr(), dev["rowptr"].data_ptr(), dev["src"].data_ptr(), dev["h_in"].data_ptr(), x_in_ptr,
            h_out.data_ptr(), X_out.data_ptr(), N, Fd if F is None else F, d["H"] if H is None else H,
            d["lmax_arg"] if lmax_arg is None else lmax_arg, int(S.sd), int(S.st), st)
        torch.cuda.synchronize()
        assert rc == expect_rc, rc
        if expect_rc:
            assert bool(torch.isnan(h_out[:N]).all()) and bool(torch.isnan(X_out[:N]).all())       # nothing was launched
            assert bool((h_out[N:] == SENTINEL).all()) and bool((X_out[N:] == SENTINEL).all())
            return None
        assert bool((h_out[N:] == SENTINEL).all()) and bool((X_out[N:] == SENTINEL).all()), "a row past N was written"
        outs.append(torch.cat([h_out[:N, None], X_out[:N]], 1).cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two launches differ"
    return outs[0]


def _launch_k7(d, want_raw=None, expect_rc=0, mode=None, lmax_arg=None, F=None):
    """The ONE place K7 inputs reach the library; same rules as _launch_k6.  -> (w_raw or None, w), [E, F] on the CPU."""
    from gotennet_amd import _lib
    lib = _lib.load()
    S, Fd, N, E = d["S"], d["F"], d["N"], d["E"]
    want_raw = d["case"]["w_raw"] if want_raw is None else want_raw
    _check_graph(d)
    for t in (d["EQ"], d["EK"], d["rl"]):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert d["EQ"].numel() == N * S.D * Fd and d["EK"].numel() == N * S.D * Fd and d["rl"].numel() == E * S.D
    if expect_rc == 0:
        assert mode is None and lmax_arg is None and F is None
        assert 0 <= d["mode"] <= 15 and (d["lmax_arg"] & 0xff) == S.lmax and not (d["lmax_arg"] & ~(0xff | U.SLICED))
        assert Fd in (16, 32, 64, 128, 256, 512, 1024)
    dev = {k: d[k].cuda() for k in ("EQ", "EK", "rl", "rowptr", "src")}
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for _ in range(2):
        w = torch.full((E + PAD_ROWS, Fd), SENTINEL, device="cuda")
        w[:E] = math.nan
        w_raw = w.clone() if want_raw else None
        rc = lib.gn_htr_edge(dev["EQ"].data_ptr(), dev["EK"].data_ptr(), dev["rl"].data_ptr(), dev["rowptr"].data_ptr(),
                             dev["src"].data_ptr(), N, Fd if F is None else F, d["lmax_arg"] if lmax_arg is None else lmax_arg,
                             d["mode"] if mode is None else mode, None if w_raw is None else w_raw.data_ptr(), w.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == expect_rc, rc
        for o in (w, w_raw):
            if o is not None:
                assert bool((o[E:] == SENTINEL).all()), "a row past E was written"
                assert not expect_rc or bool(torch.isnan(o[:E]).all())
        if expect_rc:
            return None
        outs.append((None if w_raw is None else w_raw[:E].cpu(), w[:E].cpu()))
    for x, y in zip(outs[0], outs[1]):
        if x is not None:
            assert torch.equal(_bits(x), _bits(y)), "two launches differ"
    return outs[0]


def _note(form, ratio):
    WORST[form] = max(WORST.get(form, 0.0), ratio)


def _k7_ratio(d, r, bnds, got, mask=None):
    w_raw, w = got
    ratio = U.worst_ratio(w, r["w"], bnds[1], mask)
    return ratio if w_raw is None else max(ratio, U.worst_ratio(w_raw, r["w_raw"], bnds[0], mask))


# ------------------------------------------------------------------------------------------------ error / bound
K6_GROUPS = sorted({(c["F"], c["lmax"]) for c in U.K6_CASES})
K7_GROUPS = sorted({(c["lmax"], bool(c["mode"]), bool(c["flags"])) for c in U.K7_CASES})


@pytest.mark.parametrize("F,lmax", K6_GROUPS, ids=lambda v: str(v))
def test_message_aggregate_error_within_bound(F, lmax):
    """Every case of the table at this (F, lmax) on the ragged graph (in-degrees 0, 1, ns - 1, ns, ns + 1, 2 ns + 1, 63, 64, 65)
    and on the hub (301 edges, one a self-loop); the first case also at N = 9 and N = 1."""
    cases = [c for c in U.K6_CASES if (c["F"], c["lmax"]) == (F, lmax)]
    for n, c in enumerate(cases):
        for kind in ("ragged", "hub") + (("ragged9", "single") if n == 0 else ()):
            d, r, bnd = U.built_k6(c, kind)
            ratio = U.worst_ratio(_launch_k6(d), r["out"], bnd)
            print(f"{U.k6_id(c)} {kind}: kernel {U.k6_form(c)}, E={d['E']}, worst error / bound = {ratio:.3f}")
            assert ratio <= 1.0, (U.k6_id(c), kind, ratio)
            _note(U.k6_form(c), ratio)


@pytest.mark.parametrize("lmax,moded,sliced", K7_GROUPS, ids=lambda v: str(v))
def test_htr_edge_error_within_bound(lmax, moded, sliced):
    cases = [c for c in U.K7_CASES if (c["lmax"], bool(c["mode"]), bool(c["flags"])) == (lmax, moded, sliced)]
    for n, c in enumerate(cases):
        for kind in ("ragged", "hub") + (("ragged9", "single") if n == 0 else ()):
            d, r, bnds = U.built_k7(c, kind)
            ratio = _k7_ratio(d, r, bnds, _launch_k7(d))
            print(f"{U.k7_id(c)} {kind}: kernel {d['form']}, E={d['E']}, worst error / bound = {ratio:.3f}")
            assert ratio <= 1.0, (U.k7_id(c), kind, ratio)
            _note(d["form"], ratio)


# ------------------------------------------------------------------------------------------------ isolated targets, E = 0
ISOLATED = [U.k6_case(64, 2, True, True, "def"), U.k6_case(64, 3, False, True, "def", True), U.k6_case(256, 4, True, True, "def"),
            U.k6_case(1024, 2, True, True, "def"), U.k6_case(32, 5, True, True, "def"), U.k6_case(64, 2, True, True, "def", flags=U.MEAN),
            U.k6_case(64, 3, True, True, "def", flags=U.MAX)]


@pytest.mark.parametrize("c", ISOLATED, ids=U.k6_id)
def test_targets_without_edges_keep_their_rows(c):
    """h_out = h_in and X_out = X_in bit for bit on the degree-0 targets of the ragged graph (mean and max add their
    0 to the residual as well); X_out = 0 in the zero-X_in form.  E = 0, N = 5: the launch still runs and writes the same."""
    for kind in ("ragged", "empty"):
        d = U.build_k6(c, kind)
        out = _launch_k6(d)
        iso = torch.tensor(d["degs"]) == 0
        assert int(iso.sum()) >= (3 if kind == "ragged" else 5)       # (ns = 1: the target of degree ns - 1 is a fourth)
        assert torch.equal(_bits(out[iso, 0]), _bits(d["h_in"][iso]))
        want = torch.zeros_like(out[iso, 1:]) if d["X_in"] is None else d["X_in"][iso]
        assert torch.equal(_bits(out[iso, 1:]), _bits(want))


def test_htr_edge_without_edges_writes_nothing():
    for c in (U.k7_case(64, 2), U.k7_case(64, 3, U.HTR_JOINT | 4, True), U.k7_case(32, 5)):
        w_raw, w = _launch_k7(U.build_k7(c, "empty"))
        assert w.shape[0] == 0


# ------------------------------------------------------------------------------------------------ the zero-X_in form
@pytest.mark.parametrize("F,lmax,sd,st", [(64, 1, True, True), (64, 2, True, True), (64, 3, True, False), (64, 4, False, True),
                                          (256, 2, True, True), (256, 4, True, True), (16, 3, True, True)])
def test_zero_x_in_form_reads_no_tensor_gate_block(F, lmax, sd, st):
    """X_in = NULL with NaN in the tensor-gate blocks of t_filter / x / v: finite outputs, the bits of a call with a zero
    X_in tensor and finite blocks (the header's promise)."""
    c = U.k6_case(F, lmax, sd, st, "def", True)
    for kind in ("ragged", "hub"):
        d = U.build_k6(c, kind)
        S, lo = d["S"], (1 + d["S"].ND) * F
        assert bool(torch.isnan(d["xbuf"][:, lo:]).all()) and bool(torch.isnan(d["tbuf"][:, F + lo:]).all())
        out = _launch_k6(d)
        assert bool(torch.isfinite(out).all())
        g = torch.Generator().manual_seed(3)
        d0 = dict(d, case=dict(c, first=False), X_in=torch.zeros(d["N"], S.D, F))
        for key, col in (("xbuf", lo), ("vbuf", lo), ("tbuf", F + lo)):
            d0[key] = d[key].clone()
            d0[key][:, col:col + S.NT * F] = torch.randn(d[key].shape[0], S.NT * F, generator=g)
        out0 = _launch_k6(d0)
        assert torch.equal(_bits(out), _bits(out0)), (kind, U.k6_form(c), U.k6_form(d0["case"]))


# ------------------------------------------------------------------------------------------------ relabelling
def _perm(N):
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    assert not torch.equal(perm, torch.arange(N))
    return perm


@pytest.mark.parametrize("c", [U.k6_case(64, 2, True, True, "def"), U.k6_case(256, 4, True, True, "def"), U.k6_case(16, 3, False, True, "max"),
                               U.k6_case(64, 3, True, True, "def", True), U.k6_case(512, 2, True, True, "def"),
                               U.k6_case(32, 5, True, True, "def", flags=U.MEAN), U.k6_case(64, 3, True, True, "def", flags=U.MAX)], ids=U.k6_id)
def test_message_aggregate_relabelled_atoms(c):
    """Another numbering of the atoms (another workgroup, another XCD range; every target keeps its own edge order):
    h_out and X_out are permuted bit for bit."""
    for kind in ("ragged", "hub"):
        d, r, bnd = U.built_k6(c, kind)
        perm = _perm(d["N"])
        d2, _ = U.relabel(d, perm)
        out, out2 = _launch_k6(d), _launch_k6(d2)
        assert torch.equal(_bits(out2), _bits(out[perm])), (U.k6_id(c), kind)
        assert U.worst_ratio(out2, r["out"][perm], bnd[perm]) <= 1.0


@pytest.mark.parametrize("c", [U.k7_case(64, 2), U.k7_case(256, 3), U.k7_case(256, 4), U.k7_case(64, 3, U.HTR_JOINT | 8, True),
                               U.k7_case(32, 8)], ids=U.k7_id)
def test_htr_edge_relabelled_atoms(c):
    for kind in ("ragged", "hub"):
        d, r, bnds = U.built_k7(c, kind)
        d2, emap = U.relabel(d, _perm(d["N"]))
        got, got2 = _launch_k7(d), _launch_k7(d2)
        for x, y in zip(got, got2):
            assert (x is None) == (y is None)
            if x is not None:
                assert torch.equal(_bits(y), _bits(x[emap])), (U.k7_id(c), kind)


# ------------------------------------------------------------------------------------------------ confinement
CONFINE = [U.k6_case(64, 2, True, True, "def"), U.k6_case(64, 4, False, True, "def"), U.k6_case(256, 3, True, True, "def"),
           U.k6_case(64, 3, True, False, "one"), U.k6_case(32, 5, True, True, "def")]


def _row_blocks(S):
    """[1 + D] lists: the value-vector blocks whose gate feeds output row r."""
    return [[0]] + [[S.dblk(l), S.tblk(l)] for l in S.l_of]


@pytest.mark.parametrize("c", CONFINE, ids=U.k6_id)
def test_message_aggregate_non_finite_inputs_stay_where_they_belong(c):
    """One NaN at x[j, b F + ch]: exactly the targets with j among their sources, the rows whose gate is block b and channel
    ch are non-finite.  One Inf at a[e, h]: exactly that head's channels of the edge's target.  Everything else still meets
    the bound."""
    d, r, bnd = U.built_k6(c, "ragged")
    S, F, H = d["S"], d["F"], d["H"]
    ch = F // 2 + 1                                 # a channel in the middle of a row, not a lane's first
    e = int(d["rowptr"][d["degs"].index(64)]) + 5
    j = int(d["src"][e])
    targets = torch.zeros(d["N"], dtype=torch.bool)
    targets[d["seg"][d["src"].long() == j]] = True
    rb = _row_blocks(S)
    for b in (0, S.dblk(S.lmax), S.tblk(1)):
        xbuf = d["xbuf"].clone()
        xbuf[j, b * F + ch] = math.nan
        out = _launch_k6(dict(d, xbuf=xbuf))
        want = torch.zeros_like(out, dtype=torch.bool)
        rows = torch.tensor([b in blocks for blocks in rb])
        want[:, :, ch] = targets[:, None] & rows[None, :]
        assert bool(want.any()) and torch.equal(~torch.isfinite(out), want), (U.k6_id(c), b)
        assert U.worst_ratio(out, r["out"], bnd, ~want) <= 1.0
    e = int(d["rowptr"][d["degs"].index(65)]) + 7
    h = H // 2
    a = d["a"].clone()
    a[e, h] = math.inf
    out = _launch_k6(dict(d, a=a))
    hidx = U.head_index(S, F, H) == h               # [M, F]
    want = torch.zeros_like(out, dtype=torch.bool)
    want[int(d["seg"][e])] = torch.stack([torch.stack([hidx[b] for b in blocks]).any(0) for blocks in rb])
    assert bool(want.any()) and torch.equal(~torch.isfinite(out), want), U.k6_id(c)
    assert U.worst_ratio(out, r["out"], bnd, ~want) <= 1.0


@pytest.mark.parametrize("c", [U.k7_case(64, 2), U.k7_case(64, 3), U.k7_case(256, 4), U.k7_case(64, 3, U.HTR_JOINT | 4, True),
                               U.k7_case(32, 5)], ids=U.k7_id)
def test_htr_edge_nan_stays_in_its_rows_and_channel(c):
    d, r, bnds = U.built_k7(c, "ragged")
    F = d["F"]
    j, m, ch = int(d["src"][int(d["rowptr"][d["degs"].index(64)]) + 5]), d["S"].D - 2, F // 2 + 1
    EK = d["EK"].clone()
    EK[j, m, ch] = math.nan
    got = _launch_k7(dict(d, EK=EK))
    want = torch.zeros(d["E"], F, dtype=torch.bool)
    want[d["src"].long() == j, ch] = True
    for o in got:
        if o is not None:
            assert torch.equal(~torch.isfinite(o), want), U.k7_id(c)
    assert _k7_ratio(d, r, bnds, got, ~want) <= 1.0


# ------------------------------------------------------------------------------------------------ sliced against tuned
def test_sliced_kernels_against_the_tuned_ones():
    """The degree-sliced family on the inputs of the tuned kernels: both within the bound; their bits agree for K6 and for
    K7 wherever the tuned kernel uses the closed form."""
    for c in [c for c in U.K6_CASES if c["flags"] == U.SLICED]:
        for kind in ("ragged", "hub"):
            d, r, bnd = U.built_k6(dict(c, flags=0), kind)
            tuned, sliced = _launch_k6(d), _launch_k6(dict(d, lmax_arg=c["lmax"] | U.SLICED))
            same = torch.equal(_bits(tuned), _bits(sliced))
            ratios = U.worst_ratio(tuned, r["out"], bnd), U.worst_ratio(sliced, r["out"], bnd)
            print(f"{U.k6_id(c)} {kind}: tuned {ratios[0]:.3f}, sliced {ratios[1]:.3f} of the bound, same bits: {same}")
            assert max(ratios) <= 1.0 and same == SLICED_BITS_EQUAL["msg"]
    for c in (U.k7_case(64, 1), U.k7_case(64, 2), U.k7_case(64, 3), U.k7_case(256, 4), U.k7_case(64, 2, U.HTR_NOREJ | 4, True),
              U.k7_case(64, 4, U.HTR_JOINT | 8, True)):
        for kind in ("ragged", "hub"):
            d, r, bnds = U.built_k7(c, kind)
            ds = dict(d, lmax_arg=c["lmax"] | U.SLICED, form="hl_htr")
            tuned, sliced = _launch_k7(d), _launch_k7(ds)
            same = all(torch.equal(_bits(x), _bits(y)) for x, y in zip(tuned, sliced) if x is not None)
            ratios = _k7_ratio(d, r, bnds, tuned), _k7_ratio(ds, r, U.bound_k7(ds, r), sliced)
            print(f"{U.k7_id(c)} {kind}: {d['form']} {ratios[0]:.3f}, hl_htr {ratios[1]:.3f} of the bound, same bits: {same}")
            assert max(ratios) <= 1.0 and same == SLICED_BITS_EQUAL["htr_" + U.htr_arith(d["form"])]


def test_max_aggregation_with_exact_ties():
    """aggr = max on inputs where the first two edges of every target carry the same message: held to its own reference."""
    for c in [c for c in U.K6_CASES if c["flags"] & U.MAX]:
        for kind in ("ragged", "hub"):
            d, r, bnd = U.built_k6(c, kind)
            e0 = int(d["rowptr"][d["degs"].index(max(d["degs"]))])
            assert int(d["src"][e0]) == int(d["src"][e0 + 1]) and torch.equal(d["tbuf"][e0, d["F"]:], d["tbuf"][e0 + 1, d["F"]:])
            assert U.worst_ratio(_launch_k6(d), r["out"], bnd) <= 1.0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_before_any_launch():
    from gotennet_amd._lib import GN_ERR_BAD_ARG as BAD
    d = U.build_k6(U.k6_case(64, 2, True, True, "def"), "ragged9")          # M = 5
    _launch_k6(d, expect_rc=BAD, alias_X=True)                              # X_in == X_out
    _launch_k6(d, expect_rc=BAD, ldxv=d["ldxv"] + 2)                        # rows not 16-byte aligned
    _launch_k6(d, expect_rc=BAD, ldt=d["ldt"] + 2)
    _launch_k6(d, expect_rc=BAD, H=7)                                       # (M F) % H != 0
    _launch_k6(d, expect_rc=BAD, H=32)                                      # (M F / H) % 4 != 0
    _launch_k6(d, expect_rc=BAD, lmax_arg=0)
    _launch_k6(d, expect_rc=BAD, lmax_arg=9)
    _launch_k6(d, expect_rc=BAD, lmax_arg=2 | U.MEAN | U.MAX)
    _launch_k6(d, expect_rc=BAD, lmax_arg=2 | U.SLICED, null_X=True)        # the zero-X_in form: register-tiled kernels only
    _launch_k6(d, expect_rc=BAD, lmax_arg=2 | U.MEAN, null_X=True)
    _launch_k6(d, expect_rc=BAD, lmax_arg=2 | 0x800)                        # a stray bit
    _launch_k6(d, expect_rc=BAD, F=48)                                      # not a power of two
    d7 = U.build_k7(U.k7_case(64, 2, 0, True), "ragged9")
    _launch_k7(d7, expect_rc=BAD, mode=16)                                  # GN_HTR_DIRECT: backward only
    _launch_k7(d7, expect_rc=BAD, lmax_arg=2 | U.MEAN)                      # a stray bit in lmax
    _launch_k7(d7, expect_rc=BAD, lmax_arg=0)
    _launch_k7(d7, expect_rc=BAD, lmax_arg=9)
    _launch_k7(d7, expect_rc=BAD, F=48)


# ------------------------------------------------------------------------------------------------ the table
def test_worst_ratio_per_kernel_form():
    """Runs last: the worst error / bound of every kernel form over this module's cases (DESIGN section 2 quotes it).  Run on
    its own it launches one case per form that the session has not seen yet."""
    for c in U.K6_CASES:
        if U.k6_form(c) not in WORST:
            d, r, bnd = U.built_k6(c, "ragged")
            _note(U.k6_form(c), U.worst_ratio(_launch_k6(d), r["out"], bnd))
    for c in U.K7_CASES:
        if U.k7_form(c) not in WORST:
            d, r, bnds = U.built_k7(c, "ragged")
            _note(d["form"], _k7_ratio(d, r, bnds, _launch_k7(d)))
    for form, ratio in sorted(WORST.items()):
        print(f"== {form}: worst error / bound = {ratio:.3f}")
    assert max(WORST.values()) <= 1.0
    assert set(WORST) == {U.k6_form(c) for c in U.K6_CASES} | {U.k7_form(c) for c in U.K7_CASES}
