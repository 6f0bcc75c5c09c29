"""CPU: the yardstick of tests/geometry_util.py proved on the host.  The restatement's harmonics and bases equal the goldens, its
closed form equals fp64 autograd, the fp32 emulation of K1, its backward and gn_pos_scatter stays inside the a-priori bound on
every case (worst ratio printed), and every listed mutation of the restatement is rejected by at least one case."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import gotennet_oracle as orc
from tests import geometry_util as G
from tests.golden_util import GOLDEN_DIR, case_names, load_case

CASES = range(len(G.GEO_CASES))
IDS = [G.geo_id(c) for c in G.GEO_CASES]


def test_restatement_harmonics_equal_the_known_answers():
    k = np.load(os.path.join(GOLDEN_DIR, "kat_sh_l8.npz"))
    v = torch.from_numpy(k["vec"]).double()
    x, y, z = (G.F64(v[:, n]) for n in range(3))
    for l in (5, 6, 7, 8):
        want = torch.from_numpy(k[f"sh{l}"])
        got = G._stack(G.harmonics(G.F64, l, x, y, z))
        assert got.shape == want.shape
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-13), l
        assert torch.allclose(orc.real_harmonics(l, v), want, rtol=1e-12, atol=1e-13), l
    assert float(G._stack(G.harmonics(G.F64, 8, x, y, z))[-1].abs().max()) == 0.0


BASIS_GOLDENS = {"l2_sep_f32": (0, "means", "betas"), "l8_sep_tln_f32": (0, "means", "betas"),
                 "opt_bessel_norej": (1, "freqs", "freqs"), "opt_gauss_jointhtr_gated": (2, "offsets", "widths")}


@pytest.mark.parametrize("name", sorted(BASIS_GOLDENS))
def test_restatement_equals_basis_goldens(name):
    """The reference's own fp32 rl and phi (index self-loops among the edges) against the restatement and the closed form."""
    assert name in case_names()
    cfg, sd, _, t = load_case(name)
    basis, k0, k1 = BASIS_GOLDENS[name]
    ei = t["edge_index"]
    c = dict(lmax=cfg["lmax"], E=t["edge_diff"].shape[0], R=sd["radial_basis." + k0].numel(), basis=basis,
             cutoff=float(cfg["cutoff"]), images=False, vec=t["edge_vec"].float(), diff=t["edge_diff"].float(),
             src=ei[0].to(torch.int32), dst=ei[1].to(torch.int32), p0=sd["radial_basis." + k0].float(),
             p1=sd["radial_basis." + k1].float())
    assert int((c["src"] == c["dst"]).sum()) > 0
    r = G.restate_forward(c)
    assert float((r["rl"] - t["rl"].double()).abs().max()) < 2e-6 * float(t["rl"].abs().max())
    assert float((r["phi"] - t["phi"].double()).abs().max()) < 2e-6 * float(t["phi"].abs().max())
    tr = G.values(G.k1_forward(G.F64, c))
    assert float((tr["phi"] - r["phi"]).abs().max()) < 1e-12 and float((tr["rl"] - r["rl"]).abs().max()) < 1e-12


@pytest.mark.parametrize("n", CASES, ids=IDS)
def test_closed_form_equals_oracle_and_autograd(n):
    """The F64 transcript of the kernels' expressions is the oracle's forward and the autograd backward: the difference is
    fp64 rounding, held to 1e-6 of the fp32 bound."""
    c = G.built(n)
    fr, br, fb, bb = G.reference(n)
    f64, b64 = G.values(G.k1_forward(G.F64, c)), G.values(G.k1_backward(G.F64, c))
    for key in ("rl", "cut", "phi"):
        assert G.ratio(f64[key], fr[key], fb[key]) < 1e-6, key
    for key in ("g_vec", "g_diff"):
        assert G.ratio(b64[key], br[key], bb[key]) < 1e-6, key
    re_f, re_b = G.values(G.k1_forward(G.RE, c)), G.values(G.k1_backward(G.RE, c))
    for key in f64:                                                        # the running-error pass carries the same values
        assert torch.equal(torch.nan_to_num(re_f[key]), torch.nan_to_num(f64[key])) or G.ratio(re_f[key], f64[key], fb[key]) < 1e-6
    for key in b64:
        assert G.ratio(re_b[key], b64[key], bb[key]) < 1e-6


WORST = {}


@pytest.mark.parametrize("n", CASES, ids=IDS)
def test_emulation_within_bound(n):
    c = G.built(n)
    fr, br, fb, bb = G.reference(n)
    f32, b32 = G.values(G.k1_forward(G.F32, c)), G.values(G.k1_backward(G.F32, c))
    rs = {key: G.ratio(f32[key], fr[key], fb[key]) for key in ("rl", "cut", "phi")}
    rs.update({key: G.ratio(b32[key], br[key], bb[key]) for key in ("g_vec", "g_diff")})
    print(f"{c['id']}: " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))
    for key, v in rs.items():
        WORST[key] = max(WORST.get(key, 0.0), v)
        assert v < 1.0, (key, v)
    if c["E"] == 0:
        return
    loop = G.loop_mask(c)
    out = G.tag_mask(c, "at_cutoff", "above_cutoff", "beyond")
    assert bool((f32["cut"][out] == 0).all()) and bool((fr["cut"][out] == 0).all())
    assert bool((b32["g_vec"][loop] == 0).all()) and bool((b32["g_diff"][loop] == 0).all())
    assert bool((br["g_vec"][loop] == 0).all()) and bool((br["g_diff"][loop] == 0).all())
    zero_vec = loop & (c["vec"].abs().sum(1) == 0)
    assert bool((f32["rl"][zero_vec] == 0).all())


@pytest.mark.parametrize("N,sign,hub", G.SCATTER_CASES)
def test_scatter_emulation_within_bound(N, sign, hub):
    s = G.scatter_case(N, sign, hub)
    ref, bnd = G.restate_scatter(s), G.bound_scatter(s)
    r = G.ratio(G.emulate_scatter(s), ref, bnd)
    print(f"{s['id']}: E={s['E']} g_pos={r:.3f}")
    WORST["g_pos"] = max(WORST.get("g_pos", 0.0), r)
    assert r < 1.0
    if hub:
        deg_in = torch.bincount(s["dst"].long(), minlength=N)
        deg_out = torch.bincount(s["src"].long(), minlength=N)
        assert int(deg_in.max()) >= 150 and int(deg_out.max()) >= 150
    if N >= 4:
        assert bool((ref[N - 1] == 0).all())                               # the isolated atom


def _cutoff_part(c, mut):
    """g_diff with G_phi = 0: what the cutoff alone contributes (held to EXACT zero at and beyond the cutoff)."""
    cc = dict(c, g_phi=torch.zeros_like(c["g_phi"]))
    return G.values(G.k1_backward(G.F64, cc, mut))["g_diff"]


@pytest.mark.parametrize("mut", sorted(G.MUTATIONS))
def test_mutation_is_rejected(mut):
    """Each mutation of the restatement, compared with the fp32 emulation, breaches the bound on at least one case -- the
    table has the power to see it.  `cut_le` is the one the bound cannot see (the cosine cutoff and its derivative are both
    continuous at d = c): the case table holds the cutoff's contribution at d >= c to an exact zero instead."""
    kind = G.MUTATIONS[mut]
    worst, where = 0.0, None
    if kind == "scatter":
        for N, sign, hub in G.SCATTER_CASES:
            s = G.scatter_case(N, sign, hub)
            r = G.ratio(G.emulate_scatter(s), G.restate_scatter(s, mut), G.bound_scatter(s))
            if r > worst:
                worst, where = r, s["id"]
    elif mut == "cut_le":
        for n in CASES:
            c = G.built(n)
            if c["E"] == 0 or c["n_cut"] == 0:
                continue
            at = G.tag_mask(c, "at_cutoff") & ~G.loop_mask(c)
            if not bool(at.any()):
                continue
            assert bool((_cutoff_part(c, None)[at] == 0).all())
            if bool((_cutoff_part(c, mut)[at] != 0).any()):
                worst, where = math.inf, c["id"]
    else:
        for n in CASES:
            c = G.built(n)
            if c["E"] == 0:
                continue
            fr, br, fb, bb = G.reference(n)
            if kind == "fwd":
                got, m = G.values(G.k1_forward(G.F32, c)), G.values(G.k1_forward(G.F64, c, mut))
                r = G.ratio(got["rl"], m["rl"], fb["rl"])
            else:
                got, m = G.values(G.k1_backward(G.F32, c)), G.values(G.k1_backward(G.F64, c, mut))
                r = max(G.ratio(got[key], m[key], bb[key]) for key in ("g_vec", "g_diff"))
            if r > worst:
                worst, where = r, c["id"]
    print(f"{mut}: worst error / bound {worst:.3g} on {where}")
    assert worst > 1.0, mut


def test_mutation_count():
    assert len(G.MUTATIONS) >= 12


def test_table_reaches_both_vector_paths():
    assert {c["R"] % 4 == 0 for c in G.GEO_CASES} == {True, False}
    assert {G.ndim(c["lmax"]) % 4 == 0 for c in G.GEO_CASES} == {True, False}
    big = [G.built(n) for n in CASES if G.GEO_CASES[n]["E"] >= 127]
    for c in big:
        need = {"axis", "near_axis", "length", "at_cutoff", "below_cutoff", "above_cutoff", "beyond", "loop"}
        assert need <= set(c["tags"]) and (not c["images"] or "self_image" in c["tags"])
    assert {c["perturb"] for c in big} == {True, False} and {c["hostile"] for c in big} == {True, False}


def test_init_restatement_is_permutation_covariant():
    """K2 / K3 and their backwards on a relabelled graph are the relabelled results (fp64: to rounding)."""
    for F in (16, 256):
        d = G.init_case(F, images=True)
        v, _ = G.restate_init(d)
        d2, old_of_new, emap = G.relabel_init(d)
        v2, _ = G.restate_init(d2)
        for key in ("ctx_m", "ctx_a", "g_h"):
            assert torch.allclose(v2[key], v[key][old_of_new], rtol=1e-12, atol=1e-12), key
        for key in ("t", "g_fn", "g_cut", "g_fe"):
            assert torch.allclose(v2[key], v[key][emap], rtol=1e-12, atol=1e-12), key


def test_bessel_derivative_relative_accuracy_note():
    """The figure DESIGN.md records: the relative size of the absolute bound on d/dd [sin(a d) / d] at d = 0.5, a = pi / c."""
    c = dict(G.built(0), basis=1, R=1, E=1, lmax=1, n_rl=0, n_cut=0, images=False, vec=torch.tensor([[0.5, 0.0, 0.0]]),
             diff=torch.tensor([0.5]), src=torch.tensor([0], dtype=torch.int32), dst=torch.tensor([1], dtype=torch.int32),
             p0=torch.tensor([math.pi / 5.0]), p1=torch.tensor([math.pi / 5.0]), g_phi=torch.ones(1, 1),
             g_rl=torch.zeros(0, 1, 3), g_cut=torch.zeros(0, 1), tags=["half"])
    out = G.k1_backward(G.RE, c)
    val, bnd = float(out["g_diff"].v), float(out["g_diff"].e)
    print(f"bessel d=0.5 a=pi/5: value {val:.6e} bound {bnd:.3e} relative {bnd / abs(val):.3e}")
    assert bnd / abs(val) < 1e-3


def test_worst_ratios():
    print("worst emulation / bound: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v < 1.0 for v in WORST.values())
