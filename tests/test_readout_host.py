"""CPU: the yardstick of tests/readout_util.py proved on the host.  Every restatement is the oracle's function, every closed form
equals the restatement's fp64 forward and autograd, the fp32 emulation stays inside the a-priori bound on every case (worst
ratio printed), the conditions on the inputs hold from the reference alone, and every listed mutation of the emulation is
rejected by at least one case."""
import pytest
import torch
import torch.nn.functional as Fn

from oracle import gotennet_oracle as orc
from tests import readout_util as U

WORST = {}
CLOSED = 1e-6                                      # closed form against restatement: fp64 rounding, in units of the fp32 bound
BLOCK_IDS = [U.block_id(n) for n in range(len(U.BLOCK_CASES))]
DIPOLE_IDS = [U.dipole_id(n) for n in range(len(U.DIPOLE_CASES))]
EMB_IDS = [U.emb_id(n) for n in range(len(U.EMB_CASES))]
rn64 = lambda g, *s: torch.randn(*s, generator=g, dtype=torch.float64)


def _prove(fam, n, tag):
    """Closed form = restatement (exact elements bit for bit), emulation inside the bound."""
    _, case, expected, transcript = U.FAMILY[fam]
    c, ex = case(n), expected(n)
    f64 = U.ratios(transcript(U.F64, c), ex)
    assert all(v < CLOSED for v in f64.values()), (tag, f64)
    rs = {f"{fam}.{k}": v for k, v in U.ratios(transcript(U.F32, c), ex).items()}
    print(f"{tag}: " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))
    for k, v in rs.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= 1.0, (tag, k, v)
    return c, ex


# ------------------------------------------------------------------------------------------------ case tables
def test_tables_hold_every_listed_shape_and_stay_small():
    assert {c[0] for c in U.BLOCK_CASES} == set(U.BLOCK_N) == {0, 1, 5, 257}
    assert {U.BLOCK_W[c[1]] for c in U.BLOCK_CASES} == {(1, 1, 1), (3, 2, 1), (64, 64, 64), (65, 33, 65), (200, 7, 96)}
    assert {c[2] for c in U.BLOCK_CASES} == {0, 1, 2} and {c[3] for c in U.BLOCK_CASES} == {0, 5}
    sacts = {c[4] for c in U.BLOCK_CASES}
    assert {-1, U.SILU, U.SSP} < sacts and any(k in U.KINKED for k in sacts)
    assert any(c[0] >= 5 and U.BLOCK_W[c[1]][2] == 65 for c in U.BLOCK_CASES)          # an odd width across a 256-thread block
    for n in range(len(U.BLOCK_CASES)):
        c = U.block_case(n)
        assert c["ldgv"] > c["w_off"] + c["n_vout"] and c["N"] <= 700
    assert U.MOL_A == (0, 1, 2, 63, 64, 65, 0, 128, 129, 200, 0) and U.MOL_B == (3,) and sum(U.MOL_A) <= 700
    assert {(c[1], c[2]) for c in U.DIPOLE_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {c[3] for c in U.DIPOLE_CASES} == {True, False}
    for i in range(4):
        assert {c[4][i] for c in U.DIPOLE_CASES} == {1, 3}
    assert {c[0] for c in U.DIPOLE_CASES} == {U.MOL_A, U.MOL_B} == set(U.ESE_CASES)
    assert any(c[1] and c[5] == 0.0 for c in U.DIPOLE_CASES) and any(c[1] and c[5] != 0.0 for c in U.DIPOLE_CASES)
    assert {c[1] for c in U.EMB_CASES} == set(U.EMB_F) == {1, 48, 65, 256} and {c[2] for c in U.EMB_CASES} == {0, 3}
    assert {c[3] for c in U.EMB_CASES} == set(U.EMB_SPECIES) == {1, 5, 100} and {c[4] for c in U.EMB_CASES} == {True, False}
    assert {c[0] for c in U.EMB_CASES} == {"hub", "small", "empty", "one"}
    for n in range(len(U.EMB_CASES)):
        c = U.emb_case(n)
        assert c["N"] <= 700 and c["E"] <= 2000


def test_embedding_graphs_hold_what_they_are_for():
    for n in range(len(U.EMB_CASES)):
        c = U.emb_case(n)
        N, src, dst = c["N"], c["src"], c["dst"].long()
        colptr, perm = c["colptr"].long(), c["perm"].long()
        assert torch.equal(src[perm], torch.sort(src, stable=True)[0]) and int(colptr[-1]) == c["E"]     # the by-source view
        assert torch.equal(perm, torch.sort(src, stable=True)[1])
        if N:
            assert int(c["z"].min()) == 0                                                               # species 0 present
        if c["graph"] in ("hub", "small"):                                    # a walk without perm would read other edges
            assert not torch.equal(perm, torch.arange(c["E"]))
        if c["graph"] == "hub":
            deg = colptr[1:] - colptr[:-1]
            assert int(deg.max()) >= U.HUB_DEGREE and int((deg == 0).sum()) >= 9 and bool((src == dst).any())
        if c["graph"] in ("hub", "small"):
            cnt = torch.bincount(c["z"], minlength=c["n_species"])
            assert c["n_species"] == 1 or bool((cnt == 0).any())                                        # absent species
            pair = (src == dst) & (c["edge_diff"] > 0)
            assert bool(pair.any()) and bool(((src == dst) & (c["edge_diff"] == 0)).any())
            if c["images"]:
                assert not bool(U.emb_loop(c)[pair].any())                                              # kept
        assert bool(torch.isnan(c["feat"][:, c["F"]:]).all())


# ------------------------------------------------------------------------------------------------ GatedEquivariantBlock
@pytest.mark.parametrize("n", range(len(U.BLOCK_CASES)), ids=BLOCK_IDS)
def test_block_closed_form_emulation_and_conditions(n):
    c, ex = _prove("block", n, U.block_id(n))
    nv, wo = c["n_vout"], c["w_off"]
    nrm = c["vmix"][:, :, :nv].double().norm(dim=1)
    assert torch.equal(nrm == 0, c["zero_col"]) and bool((nrm[~c["zero_col"]] >= U.V_FLOOR).all())        # 0 or >= 2^-40: none between
    if c["N"]:
        assert bool(c["zero_col"].any()) and (nv == 1 or float(nrm[~c["zero_col"]].min()) == 5 * U.V_FLOOR)
    live = torch.zeros(c["ldv"], dtype=torch.bool)
    live[:nv], live[wo:wo + nv] = True, True
    assert bool(torch.isnan(c["vmix"][:, :, ~live]).all()) and bool(torch.isfinite(c["vmix"][:, :, live]).all())
    for key, w in (("s", c["n_sin"]), ("x", c["n_sout"] + nv), ("g_ctx", c["n_sin"] + nv), ("g_s_out", c["n_sout"]), ("g_v_out", nv)):
        assert bool(torch.isnan(c[key][..., w:]).all()) and bool(torch.isfinite(c[key][..., :w]).all()), key
    if c["sact"] in U.KINKED:                                                 # a direct input: the kink itself, then clear of it
        xs = c["x"][:, :c["n_sout"] + nv].reshape(-1)
        assert xs[:3].tolist() == [0.0, U.MIN_NORMAL, -U.MIN_NORMAL] and float(xs[3:].abs().min()) >= U.MARGIN * 2.0 ** -126
    for key, mask in U.block_exact(c).items():                                # what the contract makes exact is exactly 0
        assert float(ex[key][0][mask].abs().max() if mask.any() else 0.0) == 0.0, key


@pytest.mark.parametrize("sact", [None, "silu", "softplus", "relu"])
def test_block_restatement_is_the_oracle(sact):
    kind = {None: -1, "silu": U.SILU, "softplus": U.SSP, "relu": U.RELU}[sact]
    g = torch.Generator().manual_seed(5)
    N, ns, nvin, no, nv, hid = 6, 5, 4, 3, 2, 7
    sd = {"mix_vectors.weight": rn64(g, 2 * nv, nvin), "scalar_net.0.weight": rn64(g, hid, ns + nv), "scalar_net.0.bias": rn64(g, hid),
          "scalar_net.1.weight": rn64(g, no + nv, hid), "scalar_net.1.bias": rn64(g, no + nv)}
    s, vec = rn64(g, N, ns).requires_grad_(True), rn64(g, N, 3, nvin).requires_grad_(True)
    with torch.no_grad():
        vec[2] = 0.0                                                          # a zero norm: torch.norm's subgradient
    so, vo = orc.gated_equivariant_block(sd, "", s, vec, "silu", sact)
    vmix = Fn.linear(vec, sd["mix_vectors.weight"])
    net = lambda ctx: Fn.linear(Fn.silu(Fn.linear(ctx, sd["scalar_net.0.weight"], sd["scalar_net.0.bias"])), sd["scalar_net.1.weight"],
                                sd["scalar_net.1.bias"])
    _, _, s2, v2 = U.geb_halves(s, vmix[..., :nv], vmix[..., nv:], net, kind)
    assert torch.allclose(s2, so, rtol=1e-13, atol=1e-13) and torch.allclose(v2, vo, rtol=1e-13, atol=1e-13)
    cs, cv = rn64(g, N, no), rn64(g, N, 3, nv)
    for a, b in zip(torch.autograd.grad((cs * so).sum() + (cv * vo).sum(), (s, vec)), torch.autograd.grad((cs * s2).sum() + (cv * v2).sum(), (s, vec))):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12) and bool(torch.isfinite(a).all())


# ------------------------------------------------------------------------------------------------ dipole
@pytest.mark.parametrize("n", range(len(U.DIPOLE_CASES)), ids=DIPOLE_IDS)
def test_dipole_closed_form_emulation_and_conditions(n):
    c, ex = _prove("dipole", n, U.dipole_id(n))
    for key, ld in (("mu", c["ldm"]), ("q", c["ldq"])):
        assert bool(torch.isfinite(c[key][..., 0]).all()) and (ld == 1 or bool(torch.isnan(c[key][..., 1:]).all()))
    f32 = U.dipole_transcript(U.F32, c)
    for b, size in enumerate(c["sizes"]):
        if size == 0 or b == c["zero_mol"]:                                   # exactly zero in the reference and the emulation
            assert float(ex["y"][0][b].abs().max()) == 0.0 and float(f32["y"].v[b].abs().max()) == 0.0
    if c["zero_mol"] is not None and c["standardise"]:
        a = c["batch"] == c["zero_mol"]
        assert (c["shift"] == 0.0) != bool((c["pos"][a] == 0).all())           # shift = 0 with positions, or a shift at pos = 0
    if c["magnitude"]:
        m = U.dipole_margins(c)
        print(f"{c['id']}: min |d| / bound = {float(m.min()):.3g}")
        assert float(m.min()) > 2.0
        for key, mask in U.dipole_exact(c).items():
            want = c["g_yvec"][c["zero_mol"]].double().expand(int(mask[:, 0].sum()), 3) if (key == "g_mu" and c["yvec"]) else 0.0
            assert bool((ex[key][0][mask].reshape(-1, 3 if key == "g_mu" else 1) == want).all()), key


def _readout_sd(g, F, hid):
    sd = {}
    for i, (ns, nvin, no, nv, h) in enumerate([(F, F, hid, hid, F), (hid, hid, 1, 1, hid)]):
        p = f"equivariant_layers.{i}."
        sd.update({p + "mix_vectors.weight": rn64(g, 2 * nv, nvin) * 0.5, p + "scalar_net.0.weight": rn64(g, h, ns + nv) * 0.5,
                   p + "scalar_net.0.bias": rn64(g, h), p + "scalar_net.1.weight": rn64(g, no + nv, h) * 0.5,
                   p + "scalar_net.1.bias": rn64(g, no + nv)})
    return sd


@pytest.mark.parametrize("magnitude", [False, True])
@pytest.mark.parametrize("standardise", [False, True])
def test_dipole_restatement_is_the_oracle(standardise, magnitude):
    """Two restated blocks and the restated reduction are ``oracle.dipole``: outputs and the gradients w.r.t. h and X."""
    g = torch.Generator().manual_seed(6)
    F, hid, n_mol = 6, 4, 4
    batch = torch.tensor([0, 0, 0, 2, 2, 3])                                  # molecule 1 is empty
    N = batch.numel()
    sd = _readout_sd(g, F, hid)
    h, X, pos = rn64(g, N, F).requires_grad_(True), rn64(g, N, 8, F).requires_grad_(True), rn64(g, N, 3)
    mean, std = (torch.tensor(0.3, dtype=torch.float64), torch.tensor(1.7, dtype=torch.float64)) if standardise else (None, None)
    y, yv = orc.dipole(sd, h, X, pos, batch, n_mol, "silu", mean, std, magnitude)
    l0, l1 = h, X[:, :3]
    for i, k in ((0, U.SILU), (1, -1)):
        p = f"equivariant_layers.{i}."
        vm = Fn.linear(l1, sd[p + "mix_vectors.weight"])
        nv = vm.shape[-1] // 2
        net = lambda ctx, p=p: Fn.linear(Fn.silu(Fn.linear(ctx, sd[p + "scalar_net.0.weight"], sd[p + "scalar_net.0.bias"])),
                                         sd[p + "scalar_net.1.weight"], sd[p + "scalar_net.1.bias"])
        _, _, l0, l1 = U.geb_halves(l0, vm[..., :nv], vm[..., nv:], net, k)
    y2, yv2 = U.dipole_restatement(l1[..., 0], l0[:, 0], pos, batch, n_mol, std, mean, magnitude)
    assert torch.allclose(y2.reshape(y.shape), y, rtol=1e-13, atol=1e-13) and torch.allclose(yv2, yv[..., 0], rtol=1e-13, atol=1e-13)
    cy, cv = rn64(g, *y.shape), rn64(g, n_mol, 3)
    ga = torch.autograd.grad((cy * y).sum() + (cv * yv[..., 0]).sum(), (h, X))
    gb = torch.autograd.grad((cy * y2.reshape(y.shape)).sum() + (cv * yv2).sum(), (h, X))
    for a, b in zip(ga, gb):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ spatial extent
@pytest.mark.parametrize("n", range(len(U.ESE_CASES)), ids=["A", "B"])
def test_ese_closed_form_emulation_and_conditions(n):
    c, ex = _prove("ese", n, f"ese-{U.ese_case(n)['id']}")
    m = U.atom_mass(c).double()
    ms = torch.zeros(c["n_mol"], dtype=torch.float64).index_add_(0, c["batch"], m)
    assert bool(((ms == 0) | (ms >= 1.0)).all())                              # the ms > 0 branch: no near tie
    z = c["z"].long()
    if c["sizes"] is U.MOL_A:
        assert bool((z < 0).any()) and bool((z >= c["n_mass"]).any()) and float(ms[U.MASSLESS_MOL]) == 0.0
        assert float(c["pos"][c["batch"] == U.FAR_MOL].abs().min()) > 20.0
        a = c["batch"] == U.MASSLESS_MOL                                      # c = 0 there: y = sum |pos|^2 x
        want = (c["pos"][a].double().pow(2).sum(1) * c["x"][a].double()).sum()
        assert abs(float(ex["y"][0][U.MASSLESS_MOL] - want)) <= 1e-12 * float(want.abs())
        assert sum(int(ms[b] > 0) for b in (8, 9)) == 2 and bool((m[c["batch"] >= 8] == 0).any())
    for b, size in enumerate(c["sizes"]):
        if size == 0:
            assert float(ex["y"][0][b]) == 0.0


def test_ese_restatement_is_the_oracle():
    g = torch.Generator().manual_seed(7)
    batch = torch.tensor([0, 0, 0, 1, 2, 2])
    N, n_mol = batch.numel(), 3
    z = torch.tensor([1, 6, 8, 7, 1, 9])
    mass = torch.rand(12, generator=g, dtype=torch.float64) * 20.0 + 1.0
    head = {"out_net.1.out_net.0.weight": torch.ones(1, 1, dtype=torch.float64), "out_net.1.out_net.0.bias": torch.zeros(1, dtype=torch.float64),
            "atomic_mass": mass}
    x, pos = rn64(g, N).requires_grad_(True), rn64(g, N, 3) + 30.0
    y, _ = orc.electronic_spatial_extent(head, x[:, None], pos, z, batch, n_mol, "softplus")
    y2 = U.ese_restatement(x, pos, mass[z], batch, n_mol)
    assert torch.allclose(y2, y[:, 0], rtol=1e-13, atol=1e-13)
    cy = rn64(g, n_mol)
    (ga,), (gb,) = torch.autograd.grad((cy * y[:, 0]).sum(), x), torch.autograd.grad((cy * y2).sum(), x)
    assert torch.allclose(ga, gb, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("n", range(len(U.EMB_CASES)), ids=EMB_IDS)
def test_embedding_closed_form_emulation_and_conditions(n):
    c, ex = _prove("emb", n, U.emb_id(n))
    assert float(ex["dA_na"][0][0].abs().max()) == 0.0                       # the padding row
    for key, mask in U.emb_exact(c).items():
        assert float(ex[key][0][mask].abs().max() if mask.any() else 0.0) == 0.0, key
    if c["N"] == 0:
        assert all(float(ex[k][0].abs().max() if ex[k][0].numel() else 0.0) == 0.0 and bool((ex[k][1] == 0).all()) for k in ex)
    else:
        assert int(c["z"][0]) == 0 and float(ex["dA_nbr"][0][0].abs().max()) > 0          # row 0 of A_nbr is NOT zeroed


def test_embedding_restatement_is_the_oracle():
    """The gradients of ``oracle.node_init`` w.r.t. its two embeddings are the index_add_ restatement fed with dL/d[h0 | m].
    That cotangent is read off dL/dh0: the m half of the first layer's weight is the h0 half times a column scale d, so
    dL/dm = dL/dh0 * d."""
    g = torch.Generator().manual_seed(8)
    F, R, Fc, nsp = 5, 4, 6, 4
    N, src, dst, _ = U._graph("small", g)
    E = src.numel()
    z = torch.tensor([0, 1, 2, 0, 3, 1, 2])
    cfg = orc.default_config(n_atom_basis=F, n_rbf=R, cutoff=5.0)
    Wh, d = rn64(g, Fc, F), rn64(g, F)
    p = "node_init.W_nrd_nru.dense_layers."
    sd = {"node_init.A_nbr.weight": rn64(g, nsp, F).requires_grad_(True), "node_init.W_ndp.dense_layers.0.weight": rn64(g, F, R),
          "node_init.W_ndp.dense_layers.0.bias": rn64(g, F), p + "0.weight": torch.cat([Wh, Wh * d], 1), p + "0.bias": rn64(g, Fc),
          p + "0.norm.weight": rn64(g, Fc), p + "0.norm.bias": rn64(g, Fc), p + "1.weight": rn64(g, F, Fc), p + "1.bias": rn64(g, F)}
    A_na = rn64(g, nsp, F).requires_grad_(True)
    r, phi = torch.rand(E, generator=g, dtype=torch.float64) * 6.0, rn64(g, E, R)            # some edges past the cutoff
    h0 = A_na[z]
    y = orc.node_init(sd, cfg, z, h0, torch.stack([src, dst]), r, phi)
    g_h0, g_na, g_nbr = torch.autograd.grad((y * rn64(g, N, F)).sum(), (h0, A_na, sd["node_init.A_nbr.weight"]))
    feat, cut = orc.linear(phi, sd, "node_init.W_ndp.dense_layers.0").detach(), orc.cosine_cutoff(r, cfg["cutoff"])
    got = U.emb_restatement(torch.cat([g_h0, g_h0 * d], 1), feat, cut, src, dst, z, nsp, src == dst)
    assert torch.allclose(got["dA_nbr"], g_nbr, rtol=1e-12, atol=1e-12) and float(g_nbr.abs().max()) > 0
    assert torch.allclose(got["dA_na"][1:], g_na[1:], rtol=1e-12, atol=1e-12)
    assert float(got["dA_na"][0].abs().max()) == 0.0 and float(g_na[0].abs().max()) > 0       # padding_idx = 0: the model's rule


# ------------------------------------------------------------------------------------------------ mutations
@pytest.mark.parametrize("mut", sorted(U.MUTATIONS))
def test_mutation_is_rejected(mut):
    """Each mutated emulation breaches the bound, or an exactness demand, on at least one case of each of its families."""
    for fam in U.MUTATIONS[mut].split("+"):
        cases, case, expected, transcript = U.FAMILY[fam]
        worst = (0.0, "")
        for n in range(len(cases)):
            c = case(n)
            worst = max(worst, (max(U.ratios(transcript(U.F32, c, mut), expected(n)).values()), c["id"]))
        print(f"{mut} [{fam}]: worst error / bound {worst[0]:.3g} on {worst[1]}")
        assert worst[0] > 1.0, (mut, fam)


def test_mutation_list_is_complete():
    assert len(U.MUTATIONS) >= 24
    for fam, cnt in dict(block=8, dipole=9, ese=5, emb=7).items():
        assert sum(1 for v in U.MUTATIONS.values() if fam in v.split("+")) >= cnt, fam


def test_worst_ratios():
    print("worst emulation / bound: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
