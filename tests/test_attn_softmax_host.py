"""CPU: the yardstick of tests/test_hip_attn_softmax.py (tests/attn_util.py) proved without a GPU -- a plain fp32 restatement
of the formula stays inside the bound on every input set the GPU test launches, the bound rejects a lost edge and a
score moved by 1e-3, the reference agrees with the oracle's segment softmax, and the hand-built graphs sit on every edge
the kernels have."""
import pytest
import torch

from tests import attn_util as U


@pytest.mark.parametrize("F,act", U.FORMS)
def test_fp32_restatement_is_within_the_bound(F, act):
    worst = 0.0
    for c in U.cases(F, act):
        d, r, bnd = U.built_case(c)
        ratio = U.worst_ratio(U.restate_fp32(d), r, bnd)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (U.case_id(c), ratio)
    print(f"F={F} act={act}: fp32 restatement, worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("F,act,H", [(256, U.ACT_SILU, 8), (64, U.ACT_SILU, 1), (64, U.ACT_TANH, 16), (16, U.ACT_SILU, 4),
                                     (512, U.ACT_SILU, 8), (1024, U.ACT_TANH, 16)])
@pytest.mark.parametrize("regime", ["ordinary", "degenerate"])
def test_bound_is_not_vacuous(F, act, H, regime):
    """One edge lost from one segment, or one raw score off by 1e-3, must violate the bound -- on a 63-, a 64- and a
    65-neighbour target and on the longest one (the strip boundaries the GPU test is about)."""
    c = dict(F=F, act=act, H=H, regime=regime, layout="compact", outdeg=False, seed=U.heads(F).index(H))
    d, r, bnd = U.built_case(c)
    for deg in (63, 64, 65, max(d["degs"])):
        i = d["degs"].index(deg)
        e0 = int(d["rowptr"][i])
        rows = torch.arange(e0, e0 + deg)
        # the first and the last edge of the segment; in the ordinary regime also the edge that carries most of head 0 (an
        # edge of weight 1e-8 can be lost without moving anything: no bound can see that, and no message would)
        top = e0 + int(r["a"][rows, 0].argmax())
        for e in (e0, e0 + deg - 1, top):
            lost = U.reference(d, remove=e)
            if regime == "degenerate" or e == top:  # judged on the edges that remain
                assert U.worst_ratio(lost["a"], r, bnd, rows[rows != e]) > 1.0, (deg, e)
            for h in (0, H - 1):
                moved = U.reference(d, shift=(e, h, 1e-3))
                assert U.worst_ratio(moved["a"][:, h], dict(a=r["a"][:, h]), bnd[:, h], rows) > 1.0, (deg, e, h)
    # and the unperturbed reference trivially meets it
    assert U.worst_ratio(r["a"], r, bnd) == 0.0


def test_reference_matches_oracle_segment_softmax():
    from oracle import gotennet_oracle as orc
    for c in (U.cases(64, U.ACT_SILU)[4], U.cases(512, U.ACT_TANH)[3], U.cases(16, U.ACT_SILU)[1]):
        d, r, _ = U.built_case(c)
        a = orc.segment_softmax(r["s"], r["seg"], d["N"]) * r["nrm"][:, None]
        assert torch.allclose(a, r["a"], rtol=1e-13, atol=0.0), U.case_id(c)
        # every non-empty segment sums to its norm-weighted one
        tot = torch.zeros(d["N"], d["H"], dtype=torch.float64).index_add_(0, r["seg"], r["a"] / r["nrm"][:, None])
        deg = torch.tensor(d["degs"])
        assert torch.allclose(tot[deg > 0], torch.ones_like(tot[deg > 0]), atol=1e-12) and bool((tot[deg == 0] == 0).all())


def test_graphs_sit_on_every_edge_and_reach_every_form():
    """The degrees of the issue on every graph; a degree-0 target on both sides of the longest one inside one group of
    four; both strip forms on either side of each threshold; every kernel form x layout x outdeg x regime is met."""
    seen_kernel, seen_strip, seen_combo = set(), set(), set()
    for F, act in U.FORMS:
        assert U.heads(F) == [H for H in range(1, 257) if H & (H - 1) == 0 and (F // 4) % H == 0 and (F // 4) // H <= 64]
        for c in U.cases(F, act):
            H, degs = c["H"], U.degrees(F, c["H"], c["seed"])
            want = {0, 1, 2, 63, 64, 65, 512 // H, 512 // H + 1} | ({2048 // H, 2048 // H + 1} if F > 256 else set())
            assert want <= set(degs) and len(degs) % 4 and 36 <= len(degs) <= 44
            i = degs.index(max(degs))
            assert i // 4 == (i - 1) // 4 == (i + 1) // 4 and degs[i - 1] == 0 and degs[i + 1] == 0
            assert sum(degs) <= 4500
            kern = U.kernel_form(F, act)
            seen_kernel.add(kern)
            seen_strip |= {(kern, U.strip_form(F, H, deg)) for deg in degs}
            seen_combo.add((kern, c["layout"], c["outdeg"], c["regime"]))
            cap = 512 if F <= 256 else 2048
            assert U.strip_form(F, H, cap // H) == "lds" and U.strip_form(F, H, cap // H + 1) == "global"
    kernels = {"wave_f256", "wave_silu", "wave_generic", "workgroup_silu", "workgroup_generic"}
    assert seen_kernel == kernels
    assert seen_strip >= {(k, s) for k in kernels for s in ("lds", "global")}
    assert seen_combo == {(k, lay, od, reg) for k in kernels for lay, od in U.LAYOUTS for reg in U.Q_SCALE}
