"""GPU: gn_attn_softmax / gn_attn_softmax_dropout called directly, every kernel form and both strip forms of each, against
the fp64 restatement and the a-priori per-element bound of tests/attn_util.py (proved on the CPU by
tests/test_attn_softmax_host.py).  Each case prints the kernel form it selects, the strip forms its targets take and the
worst error / bound."""
import pytest
import torch

from tests import attn_util as U
from tests.dropout_util import mask_reference

pytestmark = pytest.mark.gpu

PAD_ROWS = 8                                       # sentinel rows past E in every output array
SENTINEL = 12345.678


def _dev(t):
    return None if t is None else t.cuda()


def _launch(d, drop=None, ldqk=None, H=None, same_out=False, expect_rc=0):
    """The ONE place inputs reach the library.  Everything a kernel indexes with is asserted here, before any launch: a
    wrong argument would be a device fault, not a failing test.  ``drop`` = (seed, layer, p) selects the dropout entry.
    Launches twice (the second into fresh arrays): same bits; the sentinel rows past E keep theirs.
    -> a [E, H] on the CPU (and a_soft with ``drop``).  ``expect_rc`` != 0: a refusal -- returns after the ONE call, having
    checked that no output element was written; ``ldqk`` / ``H`` / ``same_out`` override the arguments for those."""
    from gotennet_amd import _lib
    lib = _lib.load()
    F, N, E = d["F"], d["N"], d["E"]
    H_arg = d["H"] if H is None else H
    ldqk_arg, ldt = d["ldqk"] if ldqk is None else ldqk, d["ldt"]
    bufs = {k: v.cuda() for k, v in d["bufs"].items()}
    if "qk" in bufs:
        q_ptr, k_ptr, qn, kn = bufs["qk"].data_ptr(), bufs["qk"].data_ptr() + 4 * F, bufs["qk"].numel(), bufs["qk"].numel() - F
    else:
        q_ptr, k_ptr, qn, kn = bufs["q"].data_ptr(), bufs["k"].data_ptr(), bufs["q"].numel(), bufs["k"].numel()
    rowptr, src, outdeg = d["rowptr"].cuda(), d["src"].cuda(), _dev(d["outdeg"])
    for t in list(bufs.values()):
        assert t.dtype == torch.float32 and t.is_contiguous()
    for t in (rowptr, src) + (() if outdeg is None else (outdeg,)):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert rowptr.numel() == N + 1 and src.numel() == E and (outdeg is None or outdeg.numel() == N)
    assert int(d["rowptr"][0]) == 0 and int(d["rowptr"][-1]) == E and bool((d["rowptr"][1:] >= d["rowptr"][:-1]).all())
    assert E == 0 or (0 <= int(d["src"].min()) and int(d["src"].max()) < N)
    # a row i / j / e is read at [row * ld, row * ld + F): the last one must end inside its buffer
    assert (N - 1) * d["ldqk"] + F <= qn and (N - 1) * d["ldqk"] + F <= kn and (E - 1) * ldt + F <= bufs["te"].numel()
    assert d["ldqk"] >= F and ldt >= F and d["ldqk"] % 4 == 0 and ldt % 4 == 0
    if expect_rc == 0:
        assert ldqk is None and H is None and not same_out
        assert H_arg in U.heads(F)
    st = torch.cuda.current_stream().cuda_stream
    key = None
    if drop is not None:
        key = torch.tensor([drop[0], 0], dtype=torch.int64, device="cuda")
    outs = []
    for _ in range(2):
        a = torch.full((E + PAD_ROWS, d["H"]), SENTINEL, device="cuda")
        a[:E] = float("nan")                       # an element the kernel skips fails every bound
        a_soft = a.clone() if drop is not None else None
        if drop is None:
            rc = lib.gn_attn_softmax(q_ptr, k_ptr, ldqk_arg, bufs["te"].data_ptr(), ldt, rowptr.data_ptr(), src.data_ptr(),
                                     None if outdeg is None else outdeg.data_ptr(), N, F, H_arg, a.data_ptr(), d["act"], st)
        else:
            rc = lib.gn_attn_softmax_dropout(q_ptr, k_ptr, ldqk_arg, bufs["te"].data_ptr(), ldt, rowptr.data_ptr(),
                                             src.data_ptr(), None if outdeg is None else outdeg.data_ptr(), N, F, H_arg,
                                             a.data_ptr() if same_out else a_soft.data_ptr(), a.data_ptr(), key.data_ptr(),
                                             drop[1], float(drop[2]), d["act"], st)
        torch.cuda.synchronize()
        assert rc == expect_rc, rc
        if expect_rc:
            assert bool(torch.isnan(a[:E]).all()) and bool((a[E:] == SENTINEL).all())       # nothing was launched
            return None
        for o in (a, a_soft):
            if o is not None:
                assert bool((o[E:] == SENTINEL).all()), "a row past E was written"
        outs.append((a[:E].cpu(), None if a_soft is None else a_soft[:E].cpu()))
    for x, y in zip(outs[0], outs[1]):
        if x is not None:
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "two launches differ"
    return outs[0] if drop is not None else outs[0][0]


def _strips(d):
    return sorted({U.strip_form(d["F"], d["H"], deg) for deg in d["degs"]})


@pytest.mark.parametrize("F,act", U.FORMS)
def test_attn_softmax_every_head_count_layout_and_regime(F, act):
    """Every H the entry point accepts x ordinary / saturating / degenerate scores x (engine | compact layout, with |
    without outdeg) in rotation, on graphs with in-degrees 0, 1, 2, 63, 64, 65 and both sides of the strip threshold(s)."""
    kern, worst = U.kernel_form(F, act), 0.0
    for c in U.cases(F, act):
        d, r, bnd = U.built_case(c)
        strips = _strips(d)
        assert "lds" in strips and "global" in strips
        ratio = U.worst_ratio(_launch(d), r, bnd)
        print(f"{U.case_id(c)}: kernel {kern}, strips {'/'.join(strips)}, E={d['E']}, worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0, (U.case_id(c), ratio)
        worst = max(worst, ratio)
    print(f"== {kern} F={F} act={act}: worst error / bound = {worst:.3f}")


def test_every_kernel_form_is_selected():
    """The cases above reach all five inference kernels, each with both strip forms; the dropout cases below their four."""
    seen = {(U.kernel_form(F, act), s) for F, act in U.FORMS for c in U.cases(F, act)
            for s in {U.strip_form(F, c["H"], deg) for deg in U.degrees(F, c["H"], c["seed"])}}
    for k in ("wave_f256", "wave_silu", "wave_generic", "workgroup_silu", "workgroup_generic"):
        assert (k, "lds") in seen and (k, "global") in seen, k
    assert {U.kernel_form(c["F"], c["act"], True) for c in DROP_CASES} == {
        "drop_wave_silu", "drop_wave_generic", "drop_workgroup_silu", "drop_workgroup_generic"}


PERM_CASES = [dict(F=256, act=U.ACT_SILU, H=8), dict(F=64, act=U.ACT_SILU, H=16), dict(F=64, act=U.ACT_TANH, H=1),
              dict(F=16, act=U.ACT_SILU, H=4), dict(F=512, act=U.ACT_SILU, H=8), dict(F=1024, act=U.ACT_TANH, H=256)]


@pytest.mark.parametrize("c", PERM_CASES, ids=lambda c: f"F{c['F']}-act{c['act']}-H{c['H']}")
def test_attn_softmax_position_independence(c):
    """The same segments with the targets in another order (another wave, another workgroup, other neighbours in the group
    of four): every segment's rows keep their bits.  A strip that leaks between the four waves of a workgroup moves them."""
    c = dict(c, regime="ordinary", layout="compact", outdeg=True, seed=U.heads(c["F"]).index(c["H"]))
    d, r, bnd = U.built_case(c)
    a = _launch(d)
    N = d["N"]
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    assert not torch.equal(perm, torch.arange(N))
    emap = torch.cat([torch.arange(int(d["rowptr"][i]), int(d["rowptr"][i + 1])) for i in perm.tolist()])
    d2 = U.build(c, degs=[d["degs"][i] for i in perm.tolist()])
    d2["src"] = d["src"][emap].contiguous()
    d2["q"], d2["k"], d2["t"] = d["q"][perm].contiguous(), d["k"], d["t"][emap].contiguous()
    d2["outdeg"] = d["outdeg"]
    d2["bufs"] = dict(q=d2["q"], k=d2["k"], te=d2["t"])
    a2 = _launch(d2)
    assert torch.equal(a2.view(torch.int32), a[emap].view(torch.int32))
    ratio = U.worst_ratio(a2, dict(a=r["a"][emap]), bnd[emap])
    print(f"{U.case_id(c)}: kernel {U.kernel_form(c['F'], c['act'])}, permuted targets: same bits, worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("c", [PERM_CASES[0], PERM_CASES[1], PERM_CASES[2], PERM_CASES[4]],
                         ids=lambda c: f"F{c['F']}-act{c['act']}-H{c['H']}")
def test_attn_softmax_non_finite_inputs_stay_in_their_target(c):
    """An Inf in the q row of a 64-neighbour target (scores in LDS) and a NaN in the q row of the longest one (scores in
    its own output rows): the head that holds the poisoned channel is non-finite in those two targets, every other element
    -- their other heads included -- still meets the bound.  (q is read by its own target only; the k rows stay finite.)"""
    c = dict(c, regime="ordinary", layout="compact", outdeg=False, seed=U.heads(c["F"]).index(c["H"]))
    d, r, bnd = U.built_case(c)
    F, H = d["F"], d["H"]
    i_inf, i_nan = d["degs"].index(64), d["degs"].index(max(d["degs"]))
    assert U.strip_form(F, H, 64) == ("lds" if 64 * H <= (512 if F <= 256 else 2048) else "global")
    assert U.strip_form(F, H, max(d["degs"])) == "global"
    ch = F // 2 + 1                                 # a channel in the middle of a row, not a lane's first
    q = d["q"].clone()
    q[i_inf, ch], q[i_nan, ch] = float("inf"), float("nan")
    d2 = dict(d, q=q, bufs=dict(q=q, k=d["k"], te=d["t"]))
    assert bool(torch.isfinite(d2["k"]).all()) and bool(torch.isfinite(d2["t"]).all())
    a = _launch(d2)
    bad = torch.zeros(d["E"], H, dtype=torch.bool)
    for i in (i_inf, i_nan):
        bad[int(d["rowptr"][i]):int(d["rowptr"][i + 1]), ch // (F // H)] = True
    assert not bool(torch.isfinite(a[bad]).any()), "a poisoned head came out finite"
    assert bool(torch.isfinite(a[~bad]).all()), "a non-finite value outside the two poisoned heads"
    ratio = float(((a.double() - r["a"]).abs() / bnd)[~bad].max())
    print(f"{U.case_id(c)}: kernel {U.kernel_form(F, c['act'])}, Inf / NaN confined; elsewhere worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0


DROP_CASES = [dict(F=64, act=U.ACT_SILU, H=8), dict(F=64, act=U.ACT_TANH, H=8), dict(F=512, act=U.ACT_SILU, H=8),
              dict(F=512, act=U.ACT_TANH, H=8)]


@pytest.mark.parametrize("p", [0.1, 1.0])
@pytest.mark.parametrize("c", DROP_CASES, ids=lambda c: f"F{c['F']}-act{c['act']}-H{c['H']}")
def test_attn_softmax_dropout(c, p):
    """The training entry: a_soft meets the inference bound; a = a_soft * m bit for bit, m the Philox mask of the header
    restated in tests/dropout_util.py.  Wave form (64 / 65 neighbours at H = 8 straddle the 512-float strip) and workgroup
    form (256 / 257 straddle 2048)."""
    c = dict(c, regime="ordinary", layout="engine", outdeg=True, seed=U.heads(c["F"]).index(c["H"]))
    d, r, bnd = U.built_case(c)
    cap = 512 if d["F"] <= 256 else 2048
    assert cap // d["H"] in d["degs"] and cap // d["H"] + 1 in d["degs"]
    seed, layer = -0x1234567855AA77EE, 3
    a, a_soft = _launch(d, drop=(seed, layer, p))
    ratio = U.worst_ratio(a_soft, r, bnd)
    print(f"{U.case_id(c)} p={p}: kernel {U.kernel_form(d['F'], d['act'], True)}, strips {'/'.join(_strips(d))}, "
          f"a_soft worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    m = torch.from_numpy(mask_reference(seed, layer, d["E"], d["H"], p))
    assert m.dtype == torch.float32 and (p >= 1.0 or 0.0 < float((m == 0).float().mean()) < 0.2)
    assert torch.equal((a_soft * m).view(torch.int32), a.view(torch.int32))


def test_attn_softmax_refusals_return_before_any_launch():
    from gotennet_amd._lib import GN_ERR_BAD_ARG
    c = dict(F=64, act=U.ACT_SILU, H=8, regime="ordinary", layout="compact", outdeg=False, seed=3)
    d, _, _ = U.built_case(c)
    _launch(d, H=3, expect_rc=GN_ERR_BAD_ARG)                            # not a power of two
    _launch(d, H=32, expect_rc=GN_ERR_BAD_ARG)                           # (F / 4) % H != 0
    _launch(d, ldqk=d["ldqk"] + 2, expect_rc=GN_ERR_BAD_ARG)             # rows not 16-byte aligned
    for kw in (dict(H=3), dict(H=32), dict(ldqk=d["ldqk"] + 2), dict(same_out=True)):
        _launch(d, drop=(1, 0, 0.1), expect_rc=GN_ERR_BAD_ARG, **kw)
