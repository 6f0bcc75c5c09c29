"""GPU: the eight entry points of csrc/gn_heads.hip -- gn_geb_context, gn_geb_gate, gn_dipole_reduce, gn_ese_reduce and their
backwards -- called directly, against the fp64 restatement and the a-priori per-element bounds of tests/readout_util.py (proved
on the CPU by tests/test_readout_host.py).  Every output lies between sentinel guard rows, every launch runs twice (same bits),
the columns an entry point must not write keep a second sentinel, each case prints its worst error / bound per output; the last
test prints the worst per entry point."""
import math
import types

import pytest
import torch

from tests import readout_util as U
from tests.norm_gpu import SENTINEL, Out
from tests.norm_gpu import bits as _bits, dev as _dev, launch as _launch, lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu

WORST = {}
FILL2 = -54321.25                                  # the second sentinel: in the columns an entry point must leave alone
BLOCK_IDS = [U.block_id(n) for n in range(len(U.BLOCK_CASES))]
DIPOLE_IDS = [U.dipole_id(n) for n in range(len(U.DIPOLE_CASES))]


def _note(entry, rs, tag):
    print(f"{tag}: " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))
    for k, v in rs.items():
        WORST[entry + "." + k] = max(WORST.get(entry + "." + k, 0.0), v)
    assert all(v <= 1.0 for v in rs.values()), (tag, rs)


def _devs(c, keys):
    d = {k: _dev(c[k]) for k in keys}
    return d, {k: t.data_ptr() for k, t in d.items()}


def _untouched(call, specs, widths, ran):
    """A third run into arrays filled with the second sentinel: the columns past ``widths[name]`` keep it, the rest repeat."""
    outs = {k: Out(r, c, fill=FILL2) for k, (r, c) in specs.items()}
    assert call({k: o.ptr() for k, o in outs.items()}) == 0
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.check(k)
        w = widths.get(k, specs[k][1])
        got = o.inner().cpu()
        assert bool((got[:, w:] == FILL2).all()), f"{k}: a column past its width was written"
        assert torch.equal(_bits(got[:, :w]), _bits(ran[k][:, :w])), k


def _replay(call, specs):
    """Capture ``call`` in a graph, replay it into re-poisoned outputs.  -> name -> CPU tensor."""
    outs = {k: Out(r, c) for k, (r, c) in specs.items()}
    ptrs = {k: o.ptr() for k, o in outs.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call(ptrs) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert call(ptrs) == 0
    for o in outs.values():
        o.inner().fill_(math.nan)
    g.replay()
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.check(k)
    return {k: o.inner().cpu() for k, o in outs.items()}


# ------------------------------------------------------------------------------------------------ GatedEquivariantBlock
def _block_job(c, over=None):
    """-> (keep-alive, call, specs, widths): the four entry points in order; both backwards write into the one g_vmix."""
    lib = _lib()
    keep, p = _devs(dict(c, **(over or {})), ("s", "vmix", "x", "g_s_out", "g_v_out", "g_ctx"))
    N, ns, no, nv, wo, k = c["N"], c["n_sin"], c["n_sout"], c["n_vout"], c["w_off"], c["sact"]

    def call(o):
        st = _stream()
        return (lib.gn_geb_context(p["s"], c["lds"], ns, p["vmix"], c["ldv"], nv, N, o["ctx"], c["ldc"], st)
                or lib.gn_geb_gate(p["x"], c["ldx"], no, nv, p["vmix"], c["ldv"], wo, N, k, o["s_out"], c["ldso"], o["v_out"], c["ldo"], st)
                or lib.gn_geb_gate_backward(p["g_s_out"], c["ldgs"], p["g_v_out"], c["ldgo"], p["x"], c["ldx"], no, nv, p["vmix"], c["ldv"],
                                            wo, N, k, o["g_x"], c["ldgx"], o["g_vmix"], c["ldgv"], st)
                or lib.gn_geb_context_backward(p["g_ctx"], c["ldc"], ns, p["vmix"], c["ldv"], nv, wo, N, o["g_s"], c["ldgsin"],
                                               o["g_vmix"], c["ldgv"], st))

    specs = dict(ctx=(N, c["ldc"]), s_out=(N, c["ldso"]), v_out=(3 * N, c["ldo"]), g_x=(N, c["ldgx"]), g_vmix=(3 * N, c["ldgv"]),
                 g_s=(N, c["ldgsin"]))
    return keep, call, specs, dict(s_out=no, v_out=nv, g_s=ns)


def _block_view(c, out):
    """The raw arrays in the layout of ``block_transcript``."""
    N, ns, no, nv = c["N"], c["n_sin"], c["n_sout"], c["n_vout"]
    return dict(ctx=out["ctx"], s_out=out["s_out"][:, :no], v_out=out["v_out"].view(N, 3, c["ldo"])[:, :, :nv].reshape(N, 3 * nv),
                g_x=out["g_x"], g_s=out["g_s"][:, :ns], g_vmix=out["g_vmix"].reshape(N, 3 * c["ldgv"]))


BLOCK_ENTRY = dict(ctx="gn_geb_context", s_out="gn_geb_gate", v_out="gn_geb_gate", g_x="gn_geb_gate_backward",
                   g_s="gn_geb_context_backward")


@pytest.mark.parametrize("n", range(len(U.BLOCK_CASES)), ids=BLOCK_IDS)
def test_block_within_bound(n):
    c, ex = U.block_case(n), U.block_expected(n)
    keep, call, specs, widths = _block_job(c)
    raw = _launch(call, specs)
    _untouched(call, specs, widths, raw)
    assert bool(torch.isfinite(raw["g_vmix"]).all()), "an element of g_vmix was left unwritten by both backwards"
    got = _block_view(c, raw)
    for key, entry in BLOCK_ENTRY.items():
        _note(entry, {key: U.worst(got[key], *ex[key])}, c["id"])
    half = lambda t, a, b: t.reshape(c["N"], 3, c["ldgv"])[:, :, a:b]       # the V half is the context's, the W half the gate's
    for entry, (a, b) in (("gn_geb_context_backward", (0, c["w_off"])), ("gn_geb_gate_backward", (c["w_off"], c["ldgv"]))):
        _note(entry, {"g_vmix": U.worst(half(got["g_vmix"], a, b), half(ex["g_vmix"][0], a, b), half(ex["g_vmix"][1], a, b))}, c["id"])


def test_block_nan_stays_in_its_atom():
    c = U.block_case(BLOCK_IDS.index("N5-65x33x65-ld2-w70-silu"))
    keep, call, specs, _ = _block_job(c)
    clean = _launch(call, specs)
    a, over = 2, {}
    for key in ("s", "vmix", "x", "g_s_out", "g_v_out", "g_ctx"):
        t = c[key].clone()
        t[a] = math.nan
        over[key] = t
    keep2, call2, _, _ = _block_job(c, over)
    dirty = _launch(call2, specs)
    for key, t in clean.items():
        per = t.shape[0] // c["N"]
        rows = torch.ones(t.shape[0], dtype=torch.bool)
        rows[a * per:(a + 1) * per] = False
        assert torch.equal(_bits(dirty[key][rows]), _bits(t[rows])), key


def test_block_replays_in_a_graph():
    c = U.block_case(BLOCK_IDS.index("N257-65x33x65-ld1-w70-relu"))
    keep, call, specs, _ = _block_job(c)
    eager, replay = _launch(call, specs), _replay(call, specs)
    for key in eager:
        assert torch.equal(_bits(eager[key]), _bits(replay[key])), key


# ------------------------------------------------------------------------------------------------ dipole
def _dipole_job(c, over=None):
    lib = _lib()
    keep, p = _devs(dict(c, **(over or {})), ("mu", "q", "pos", "mol_ptr", "g_y", "g_yvec"))
    N, n_mol, st_, mag = c["N"], c["n_mol"], c["standardise"], c["magnitude"]

    def call(o):
        st = _stream()
        return (lib.gn_dipole_reduce(p["mu"], c["ldm"], p["q"], c["ldq"], p["pos"], p["mol_ptr"], n_mol, c["scale"], c["shift"], st_, mag,
                                     o["y"], o.get("y_vec"), st)
                or lib.gn_dipole_reduce_backward(p["g_y"], p["g_yvec"] if c["yvec"] else None, p["mu"], c["ldm"], p["q"], c["ldq"], p["pos"],
                                                 p["mol_ptr"], n_mol, c["scale"], c["shift"], st_, mag, o["g_mu"], c["ldgm"], o["g_q"],
                                                 c["ldgq"], st))

    specs = dict(y=(n_mol, 1 if mag else 3), g_mu=(3 * N, c["ldgm"]), g_q=(N, c["ldgq"]))
    if c["yvec"]:
        specs["y_vec"] = (n_mol, 3)
    return keep, call, specs, dict(g_mu=1, g_q=1)


def _dipole_view(c, out):
    got = dict(y=out["y"][:, 0] if c["magnitude"] else out["y"], g_mu=out["g_mu"][:, 0].reshape(c["N"], 3), g_q=out["g_q"][:, 0])
    if c["yvec"]:
        got["y_vec"] = out["y_vec"]
    return got


DIPOLE_ENTRY = dict(y="gn_dipole_reduce", y_vec="gn_dipole_reduce", g_mu="gn_dipole_reduce_backward", g_q="gn_dipole_reduce_backward")


@pytest.mark.parametrize("n", range(len(U.DIPOLE_CASES)), ids=DIPOLE_IDS)
def test_dipole_within_bound(n):
    c, ex = U.dipole_case(n), U.dipole_expected(n)
    keep, call, specs, widths = _dipole_job(c)
    raw = _launch(call, specs)
    _untouched(call, specs, widths, raw)
    got = _dipole_view(c, raw)
    for key in ex:
        _note(DIPOLE_ENTRY[key], {key: U.worst(got[key], *ex[key])}, c["id"])
    for b, size in enumerate(c["sizes"]):
        if size == 0 or b == c["zero_mol"]:
            assert float(got["y"][b].abs().max()) == 0.0, "an empty molecule or the zero dipole"


def test_dipole_nan_stays_in_its_molecule():
    for n in (DIPOLE_IDS.index("A-st1-mag1-yvec-ld1313-shift0.3"), DIPOLE_IDS.index("A-st0-mag0-yvec-ld1331-shift0.3")):
        c = U.dipole_case(n)
        keep, call, specs, _ = _dipole_job(c)
        clean = _launch(call, specs)
        b = 5
        mu = c["mu"].clone()
        mu[int(c["mol_ptr"][b]) + 7, 1, 0] = math.nan
        keep2, call2, _, _ = _dipole_job(c, dict(mu=mu))
        dirty = _launch(call2, specs)
        mols, atoms = torch.arange(c["n_mol"]) != b, c["batch"] != b
        for key in ("y", "y_vec"):
            assert torch.equal(_bits(dirty[key][mols]), _bits(clean[key][mols])), key
        assert torch.equal(_bits(dirty["g_q"][atoms]), _bits(clean["g_q"][atoms]))
        assert torch.equal(_bits(dirty["g_mu"][atoms.repeat_interleave(3)]), _bits(clean["g_mu"][atoms.repeat_interleave(3)]))
        assert bool(torch.isnan(dirty["y"][b]).any())


# ------------------------------------------------------------------------------------------------ spatial extent
def _ese_job(c, over=None):
    lib = _lib()
    keep, p = _devs(dict(c, **(over or {})), ("x", "pos", "z", "mass", "mol_ptr", "g_y"))
    n_mol = c["n_mol"]

    def call(o):
        st = _stream()
        return (lib.gn_ese_reduce(p["x"], p["pos"], p["z"], p["mass"], c["n_mass"], p["mol_ptr"], n_mol, o["y"], st)
                or lib.gn_ese_reduce_backward(p["g_y"], p["pos"], p["z"], p["mass"], c["n_mass"], p["mol_ptr"], n_mol, o["u"], st))

    return keep, call, dict(y=(n_mol, 1), u=(c["N"], 1))


@pytest.mark.parametrize("n", range(len(U.ESE_CASES)), ids=["A", "B"])
def test_ese_within_bound(n):
    c, ex = U.ese_case(n), U.ese_expected(n)
    keep, call, specs = _ese_job(c)
    raw = _launch(call, specs)
    _note("gn_ese_reduce", {"y": U.worst(raw["y"][:, 0], *ex["y"])}, c["id"])
    _note("gn_ese_reduce_backward", {"u": U.worst(raw["u"][:, 0], *ex["u"])}, c["id"])
    for b, size in enumerate(c["sizes"]):
        if size == 0:
            assert float(raw["y"][b, 0]) == 0.0


def test_ese_nan_stays_in_its_molecule():
    c = U.ese_case(0)
    keep, call, specs = _ese_job(c)
    clean = _launch(call, specs)
    b = 8
    pos = c["pos"].clone()
    pos[int(c["mol_ptr"][b]) + 100, 2] = math.nan
    keep2, call2, _ = _ese_job(c, dict(pos=pos))
    dirty = _launch(call2, specs)
    mols, atoms = torch.arange(c["n_mol"]) != b, c["batch"] != b
    assert torch.equal(_bits(dirty["y"][mols]), _bits(clean["y"][mols])) and bool(torch.isnan(dirty["y"][b]))
    assert torch.equal(_bits(dirty["u"][atoms]), _bits(clean["u"][atoms])) and bool(torch.isnan(dirty["u"][~atoms]).all())


def test_reductions_replay_in_a_graph():
    cd, ce = U.dipole_case(DIPOLE_IDS.index("A-st1-mag1-yvec-ld1313-shift0.3")), U.ese_case(0)
    keep_d, call_d, specs_d, _ = _dipole_job(cd)
    keep_e, call_e, specs_e = _ese_job(ce)
    specs = dict(specs_d, ese_y=specs_e["y"], u=specs_e["u"])
    call = lambda o: call_d(o) or call_e(dict(y=o["ese_y"], u=o["u"]))
    eager, replay = _launch(call, specs), _replay(call, specs)
    for key in eager:
        assert torch.equal(_bits(eager[key]), _bits(replay[key])), key


# ------------------------------------------------------------------------------------------------ zero sizes, refusals
def test_zero_sizes_touch_nothing():
    lib, st = _lib(), _stream()
    d, i = _dev(torch.randn(64)), _dev(torch.zeros(8, dtype=torch.int32))
    p, ip = d.data_ptr(), i.data_ptr()
    o = Out(4, 8, fill=SENTINEL)
    q = o.ptr()
    assert lib.gn_geb_context(p, 4, 4, p, 4, 2, 0, q, 8, st) == 0 and lib.gn_geb_gate(p, 4, 2, 2, p, 4, 2, 0, 0, q, 2, q, 2, st) == 0
    assert lib.gn_geb_gate_backward(p, 2, p, 2, p, 4, 2, 2, p, 4, 2, 0, 0, q, 4, q, 4, st) == 0
    assert lib.gn_geb_context_backward(p, 8, 4, p, 4, 2, 2, 0, q, 4, q, 4, st) == 0
    assert lib.gn_dipole_reduce(p, 1, p, 1, p, ip, 0, 1.0, 0.0, 1, 1, q, q, st) == 0
    assert lib.gn_dipole_reduce_backward(p, p, p, 1, p, 1, p, ip, 0, 1.0, 0.0, 1, 1, q, 1, q, 1, st) == 0
    assert lib.gn_ese_reduce(p, p, ip, p, 4, ip, 0, q, st) == 0 and lib.gn_ese_reduce_backward(p, p, ip, p, 4, ip, 0, q, st) == 0
    torch.cuda.synchronize()
    assert bool((o.t == SENTINEL).all())


def _refuse(fn, base, clauses):
    """``base`` is accepted; each (position, value) alone makes the call GN_ERR_BAD_ARG.  Every pointer of ``base`` lies in the
    middle of a live zero-filled buffer, so a call that is wrongly accepted stays inside allocated memory."""
    from gotennet_amd import _lib as L
    assert fn(*base) == 0, fn.__name__
    for pos, bad in clauses:
        args = list(base)
        args[pos] = bad
        assert fn(*args) == L.GN_ERR_BAD_ARG, (fn.__name__, pos, bad)
    torch.cuda.synchronize()


def test_entry_points_refuse_bad_arguments():
    lib, st = _lib(), _stream()
    fbuf, ibuf = torch.zeros(1 << 16, device="cuda"), torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    P, I = fbuf[1 << 15:].data_ptr(), ibuf[1 << 15:].data_ptr()              # 128 KiB of live zeros on either side
    N = 2
    # gn_geb_context(s, lds, n_sin, vmix, ldv, n_vout, N, ctx, ldc)
    _refuse(lib.gn_geb_context, [P, 4, 4, P, 6, 2, N, P, 8, st],
            [(6, -1), (2, 0), (5, 0), (8, 5), (1, 3), (4, 1), (0, None), (3, None), (7, None)])
    # gn_geb_gate(x, ldx, n_sout, n_vout, vmix, ldv, w_off, N, sact, s_out, lds, v_out, ldo)
    _refuse(lib.gn_geb_gate, [P, 6, 3, 2, P, 6, 3, N, 0, P, 3, P, 2, st],
            [(7, -1), (2, 0), (3, 0), (6, -1), (1, 4), (10, 2), (12, 1), (5, 4), (8, -2), (8, 12), (0, None), (4, None), (9, None), (11, None)])
    # gn_geb_gate_backward(g_s_out, ldgs, g_v_out, ldgo, x, ldx, n_sout, n_vout, vmix, ldv, w_off, N, sact, g_x, ldgx, g_vmix, ldgv)
    _refuse(lib.gn_geb_gate_backward, [P, 3, P, 2, P, 6, 3, 2, P, 6, 3, N, 0, P, 6, P, 6, st],
            [(11, -1), (6, 0), (7, 0), (10, -1), (5, 4), (14, 4), (1, 2), (3, 1), (9, 4), (16, 4), (12, -2), (12, 12), (0, None), (2, None),
             (4, None), (8, None), (13, None), (15, None)])
    # gn_geb_context_backward(g_ctx, ldc, n_sin, vmix, ldv, n_vout, w_off, N, g_s, lds, g_vmix, ldgv)
    _refuse(lib.gn_geb_context_backward, [P, 8, 4, P, 6, 2, 3, N, P, 4, P, 6, st],
            [(7, -1), (2, 0), (5, 0), (6, 1), (1, 5), (9, 3), (4, 1), (11, 2), (0, None), (3, None), (8, None), (10, None)])
    # gn_dipole_reduce(mu, ldm, q, ldq, pos, mol_ptr, n_mol, scale, shift, standardise, magnitude, y, y_vec)
    _refuse(lib.gn_dipole_reduce, [P, 1, P, 1, P, I, N, 1.0, 0.0, 1, 1, P, P, st],
            [(6, -1), (1, 0), (3, 0), (11, None), (0, None), (2, None), (4, None), (5, None)])
    assert lib.gn_dipole_reduce(P, 1, P, 1, P, I, N, 1.0, 0.0, 1, 1, P, None, st) == 0           # y_vec is optional
    # gn_dipole_reduce_backward(g_y, g_yvec, mu, ldm, q, ldq, pos, mol_ptr, n_mol, scale, shift, standardise, magnitude, g_mu, ldgm, g_q, ldgq)
    _refuse(lib.gn_dipole_reduce_backward, [P, P, P, 1, P, 1, P, I, N, 1.0, 0.0, 1, 1, P, 1, P, 1, st],
            [(8, -1), (3, 0), (5, 0), (14, 0), (16, 0), (0, None), (2, None), (4, None), (6, None), (7, None), (13, None), (15, None)])
    assert lib.gn_dipole_reduce_backward(P, None, P, 1, P, 1, P, I, N, 1.0, 0.0, 1, 1, P, 1, P, 1, st) == 0      # so is g_yvec
    # gn_ese_reduce(x, pos, z, mass, n_mass, mol_ptr, n_mol, y) and its backward (g_y first, u last)
    for fn in (lib.gn_ese_reduce, lib.gn_ese_reduce_backward):
        _refuse(fn, [P, P, I, P, 4, I, N, P, st], [(6, -1), (4, 0), (0, None), (1, None), (2, None), (3, None), (5, None), (7, None)])
    torch.cuda.synchronize()
    assert float(fbuf.abs().max()) == 0.0                                     # zeros in, zeros out: nothing else was written


def test_massless_molecule_is_refused_by_the_module():
    """The kernel defines c = 0 for a molecule without mass (``test_ese_within_bound`` calls it so); the module never gets there."""
    from tests.test_hip_qm9_training import _kat_head
    from tests.test_qm9_training_host import qm9_grad_kat
    t, sd, _, _ = qm9_grad_kat()
    head = _kat_head("ese", sd)
    z = t["z"].clone()
    z[9] = 99                                                                 # molecule 1 is this one atom
    inp = types.SimpleNamespace(z=z.cuda(), batch=t["batch"].cuda(), pos=t["pos"].cuda(), representation=t["h"].cuda(),
                                vector_representation=t["X"].cuda())
    with pytest.raises(ValueError):
        head(inp)


# ------------------------------------------------------------------------------------------------ the heads end to end
@pytest.mark.parametrize("tag", ["dip_task", "ese"])
def test_head_on_long_molecules_matches_oracle(tag):
    """``Dipole`` (standardised magnitude) and ``ElectronicSpatialExtentV2`` with the fixture's weights on molecules of 70, 1 and
    130 atoms: the lane-stride loops take a second and a third trip.  Outputs, dL/dh, dL/dX and every parameter gradient against
    the fp64 oracle, at the tolerance of the 24-atom fixture."""
    from tests.test_hip_param_grads import TOL, _err
    from tests.test_hip_qm9_training import _compare, _kat_head, _kat_inputs, _kat_loss
    from tests.test_qm9_training_host import oracle_grads, oracle_outputs, qm9_grad_kat
    t0, sd, cot0, _ = qm9_grad_kat()
    g = torch.Generator().manual_seed(21)
    sizes = (70, 1, 130)
    N = sum(sizes)
    zs = t0["z"].unique()
    t = dict(h=torch.randn(N, *t0["h"].shape[1:], generator=g), X=torch.randn(N, *t0["X"].shape[1:], generator=g),
             pos=torch.randn(N, 3, generator=g) * 3.0, z=zs[torch.randint(0, zs.numel(), (N,), generator=g)],
             batch=torch.repeat_interleave(torch.arange(3), torch.tensor(sizes)).to(t0["batch"].dtype), n_mol=torch.tensor(3))
    assert int(t0["n_mol"]) == 3
    cot = {o: torch.randn(c.shape, generator=g, dtype=c.dtype) for o, c in cot0[tag].items()}
    head = _kat_head(tag, sd)
    inp, h, X = _kat_inputs(t)
    loss, res = _kat_loss(head, inp, cot)
    loss.backward()
    sd64 = {n: (v.double() if v.is_floating_point() else v) for n, v in sd[tag].items()}
    want = oracle_outputs(tag, sd64, t["h"].double(), t["X"].double(), t["pos"].double(), t["z"], t["batch"], 3)
    for o in cot:
        e = _err(res[o].reshape(want[o].shape), want[o])
        print(f"long {tag} {o}: {e:.3e}")
        assert e <= TOL, (tag, o, e)
    _compare(tag, head, h, X, oracle_grads(tag, t, sd[tag], cot), "long")


def test_worst_ratios_per_entry_point():
    print("worst error / bound: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())))
    assert WORST and all(v <= 1.0 for v in WORST.values())
