"""GPU: the stale-list check (gn_radius_verify*) against the project's own searches, and the integrator kernels of
csrc/gn_md.hip against their fp64 formulas."""
import math

import pytest
import torch

from tests import md_util as MU

pytestmark = pytest.mark.gpu

SEARCHES = ("open", "minimum", "all")
CASES = ("unchanged", "unchanged_cap", "leaves", "enters", "swap", "beyond_cap", "inside_cap", "threshold", "middle_only")


# ------------------------------------------------------------------------------------------------ 1. the verify kernels
def _case(search, name):
    """-> (base, new, batch, cutoff, cap, expected stale molecules, keyword arguments of the search / the check) on the device."""
    if search == "all":
        base, new, cell, batch, cap, stale = MU.image_cases()[name]
        return base.cuda(), new.cuda(), batch.cuda(), MU.CUTOFF_IMAGES, cap, stale, dict(cell=cell.cuda(), images="all")
    base, new, cap, stale = MU.cases()[name]
    batch = MU.batch_vector().cuda()
    if search == "open":
        return base.cuda(), new.cuda(), batch, MU.CUTOFF, cap, stale, {}
    cell = (torch.eye(3) * MU.BOX).cuda()
    return MU.wrapped(base).cuda(), MU.wrapped(new).cuda(), batch, MU.CUTOFF, cap, stale, dict(cell=cell, images="minimum")


def _search(pos, batch, cutoff, cap, kw):
    """The yardstick: the project's own search -> (edge_index, edge_shift or None)."""
    from gotennet_amd import graph
    if not kw:
        return graph.distance(pos, batch, cutoff, cap)[0], None
    ei, _, _, sh = graph.distance_pbc(pos, batch, kw["cell"], cutoff, cap, n_mol=3, images=kw["images"])
    return ei, sh


def _rows(ei, sh, N):
    """Per target, the tuple of its row's entries (source, shift) in list order, on the host."""
    ei = ei.cpu()
    sh = torch.zeros((ei.shape[1], 3), dtype=torch.int32) if sh is None else sh.cpu()
    rows = [[] for _ in range(N)]
    for e in range(ei.shape[1]):
        rows[int(ei[1, e])].append((int(ei[0, e]),) + tuple(sh[e].tolist()))
    return rows


def _changed_rows(old, new, batch, n_mol):
    """(rows that differ per molecule, the row pairs) by comparing two lists row by row on the host."""
    N = batch.shape[0]
    r0, r1 = _rows(*old, N), _rows(*new, N)
    ref = torch.zeros(n_mol, dtype=torch.int32)
    for i in range(N):
        ref[int(batch[i])] += int(r0[i] != r1[i])
    return ref, r0, r1


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("search", SEARCHES)
def test_verify_agrees_with_the_search(search, name):
    """A list is current exactly when the search at the new positions returns it: ``changed`` must equal the number of rows
    that differ between the stored and the rebuilt list, per molecule; the sticky word is 1 exactly when some entry is
    non-zero and is not cleared by a later clean check; the words around ``changed`` and behind the sticky word stay."""
    from gotennet_amd import graph
    base, new, batch, cutoff, cap, stale, kw = _case(search, name)
    stored, rebuilt = _search(base, batch, cutoff, cap, kw), _search(new, batch, cutoff, cap, kw)
    ref, r0, r1 = _changed_rows(stored, rebuilt, batch.cpu(), 3)
    # the case is what it claims (statements about the input, by the yardstick alone)
    assert tuple(int(m) for m in ref.nonzero().flatten()) == tuple(stale), (ref.tolist(), stale)
    if not name.startswith("unchanged"):
        assert 0 < int((ref != 0).sum()) < 3, "both outcomes must be present"
    if name == "swap":
        assert any(a != b and len(a) == len(b) for a, b in zip(r0, r1)), "no row changed members at the same degree"
    if name == "beyond_cap":
        quiet = 0 if search == "all" else 2
        full = _changed_rows(_search(base, batch, cutoff, 32, kw), _search(new, batch, cutoff, 32, kw), batch.cpu(), 3)[0]
        assert int(ref[quiet]) == 0 and int(full[quiet]) > 0, "the uncapped list of the quiet molecule must change"
        assert max(len(r) for r in r0) == cap, "the cap must bind"
    guard = torch.full((3 + 8,), -7, dtype=torch.int32, device="cuda")
    state = torch.tensor([0, -5, -5, -5], dtype=torch.int32, device="cuda")
    shift = dict(edge_shift=stored[1]) if kw else {}
    changed = graph.list_is_current(new, batch, stored[0], cutoff, cap, n_mol=3, state=state, out=guard[4:7], **kw, **shift)
    torch.cuda.synchronize()
    print(f"{search} {name}: changed {changed.tolist()} reference {ref.tolist()} E {stored[0].shape[1]}")
    assert changed.cpu().tolist() == ref.tolist()
    assert guard.cpu().tolist() == [-7] * 4 + ref.tolist() + [-7] * 4
    assert state.cpu().tolist() == [int(bool(ref.any())), -5, -5, -5]
    # sticky: a clean check (the stored list at its own positions) reports zeros and leaves the word alone
    again = graph.list_is_current(base, batch, stored[0], cutoff, cap, n_mol=3, state=state, **kw, **shift)
    assert again.cpu().tolist() == [0, 0, 0] and state.cpu().tolist() == [int(bool(ref.any())), -5, -5, -5]


# --------------------------------------------------------------------------------------------- 2. the integrator kernels
SIZES = (1, 63, 64, 65, 257)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _atoms(N, seed):
    """Random velocities / forces / positions, atomic numbers 1 .. 8, the built-in mass table, molecules of uneven size."""
    from gotennet_amd.md import default_masses
    from gotennet_amd.outputs import molecule_ptr
    g = torch.Generator().manual_seed(seed)
    v, f, x = (torch.randn((N, 3), generator=g) for _ in range(3))
    z = torch.randint(1, 9, (N,), generator=g, dtype=torch.int32)
    sizes = [n for n in (1, N // 3, N - 1 - N // 3) if n > 0]
    batch = MU.batch_vector(sizes).cuda()
    return dict(v=v.cuda(), f=f.cuda(), x=x.cuda(), z=z.cuda(), mass=default_masses().cuda(), sizes=sizes,
                mol_ptr=molecule_ptr(batch, len(sizes)))


def _state(stale=0, step=0):
    return torch.tensor([stale, step], dtype=torch.int32, device="cuda")


def _key(a=1234, b=0):
    return torch.tensor([a, b], dtype=torch.int64, device="cuda")


def _noise(key, step, draw, N):
    from gotennet_amd._lib import call, ptr
    out = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    call("gn_md_noise", ptr(key), step, draw, N, ptr(out), _stream())
    return out


def _close(got, ref, scale, what):
    """Element-wise: within 1e-6 of |v| + |increment| (three fp32 roundings stay below 2e-7 of it)."""
    err = (got.double() - ref).abs()
    worst = float((err / scale.clamp_min(1e-300)).max())
    print(f"{what}: max err / (|v| + |increment|) = {worst:.2e}")
    assert bool((err <= 1e-6 * scale).all()), (what, worst)


@pytest.mark.parametrize("N", SIZES)
def test_kick_drift_langevin_kinetic_against_fp64(N):
    from gotennet_amd._lib import call, ptr
    a = _atoms(N, 100 + N)
    m = a["mass"][a["z"].long()].double().unsqueeze(1)
    st, s, dt, c1, c2, fs = _state(0, 7), 0.37, 0.25, 0.9, 0.3, 0.05
    s32, dt32, c132, c232 = (float(torch.tensor(x, dtype=torch.float32)) for x in (s, dt, c1, c2))
    v = a["v"].clone()
    call("gn_md_kick", ptr(v), ptr(a["f"]), ptr(a["z"]), ptr(a["mass"]), a["mass"].numel(), N, s, ptr(st), _stream())
    inc = s32 * a["f"].double() / m
    _close(v, a["v"].double() + inc, a["v"].double().abs() + inc.abs(), f"kick N={N}")
    x = a["x"].clone()
    call("gn_md_drift", ptr(x), ptr(a["v"]), N, dt, ptr(st), _stream())
    inc = dt32 * a["v"].double()
    _close(x, a["x"].double() + inc, a["x"].double().abs() + inc.abs(), f"drift N={N}")
    key = _key()
    xi = _noise(key, 7, 1, N).double()
    v = a["v"].clone()
    call("gn_md_langevin", ptr(v), ptr(a["z"]), ptr(a["mass"]), a["mass"].numel(), N, c1, c2, ptr(key), 1, ptr(st), _stream())
    inc = c232 * xi / m.sqrt()
    _close(v, c132 * a["v"].double() + inc, a["v"].double().abs() + inc.abs(), f"langevin N={N}")
    n_mol = len(a["sizes"])
    ke = torch.empty(n_mol, dtype=torch.float32, device="cuda")
    call("gn_md_kinetic", ptr(a["v"]), ptr(a["z"]), ptr(a["mass"]), a["mass"].numel(), ptr(a["mol_ptr"]), N, n_mol, fs, ptr(ke),
         ptr(st), _stream())
    per_atom = 0.5 * (m * a["v"].double() ** 2).sum(1) / float(torch.tensor(fs, dtype=torch.float32))
    ref = torch.stack([p.sum() for p in per_atom.split(a["sizes"])])
    rel = ((ke.double() - ref).abs() / ref).max()
    print(f"kinetic N={N} molecules {a['sizes']}: max rel err {float(rel):.2e}")
    assert float(rel) <= 1e-6


def test_a_set_flag_freezes_every_integrator_kernel():
    from gotennet_amd._lib import call, ptr
    N, n_mol = 65, 3
    a = _atoms(N, 5)
    st, key = _state(1, 9), _key()
    v, x = a["v"].clone(), a["x"].clone()
    ke = torch.full((n_mol,), -3.0, device="cuda")
    f_keep, e_keep = torch.full((N, 3), -1.0, device="cuda"), torch.full((n_mol,), -2.0, device="cuda")
    s_keep, log = torch.full((n_mol, 3, 3), -4.0, device="cuda"), torch.full((4, n_mol, 2), -5.0, device="cuda")
    e, stress = torch.randn(n_mol, device="cuda"), torch.randn((n_mol, 3, 3), device="cuda")
    mt = (ptr(a["z"]), ptr(a["mass"]), a["mass"].numel())
    call("gn_md_kick", ptr(v), ptr(a["f"]), *mt, N, 0.5, ptr(st), _stream())
    call("gn_md_drift", ptr(x), ptr(v), N, 0.5, ptr(st), _stream())
    call("gn_md_langevin", ptr(v), *mt, N, 0.5, 0.5, ptr(key), 0, ptr(st), _stream())
    call("gn_md_kinetic", ptr(v), *mt, ptr(a["mol_ptr"]), N, n_mol, 1.0, ptr(ke), ptr(st), _stream())
    call("gn_md_finish", ptr(st), ptr(a["f"]), ptr(f_keep), N, ptr(e), ptr(ke), ptr(e_keep), ptr(stress), ptr(s_keep), ptr(log), 4,
         n_mol, _stream())
    torch.cuda.synchronize()
    assert torch.equal(v, a["v"]) and torch.equal(x, a["x"]) and st.tolist() == [1, 9]
    for t, fill in ((ke, -3.0), (f_keep, -1.0), (e_keep, -2.0), (s_keep, -4.0), (log, -5.0)):
        assert bool((t == fill).all())
    # the same calls with the flag clear do act (the assertion above is not vacuous), and finish does its bookkeeping
    st = _state(0, 9)
    call("gn_md_kick", ptr(v), ptr(a["f"]), *mt, N, 0.5, ptr(st), _stream())
    call("gn_md_drift", ptr(x), ptr(v), N, 0.5, ptr(st), _stream())
    call("gn_md_kinetic", ptr(v), *mt, ptr(a["mol_ptr"]), N, n_mol, 1.0, ptr(ke), ptr(st), _stream())
    call("gn_md_finish", ptr(st), ptr(a["f"]), ptr(f_keep), N, ptr(e), ptr(ke), ptr(e_keep), ptr(stress), ptr(s_keep), ptr(log), 4,
         n_mol, _stream())
    torch.cuda.synchronize()
    assert not torch.equal(v, a["v"]) and not torch.equal(x, a["x"]) and bool((ke > 0).all())
    assert st.tolist() == [0, 10] and torch.equal(f_keep, a["f"]) and torch.equal(e_keep, e) and torch.equal(s_keep, stress)
    assert torch.equal(log[9 % 4, :, 0], e) and torch.equal(log[9 % 4, :, 1], ke)
    assert bool((log[[0, 2, 3]] == -5.0).all())


def test_noise():
    """196 608 samples: |mean| <= 4 / sqrt(n), |variance - 1| <= 4 sqrt(2 / n), all finite; a pure function of
    (key, step, draw, atom, component), whatever the launch geometry."""
    from gotennet_amd._lib import call, ptr
    N = 65536
    key = _key(20240607, 3)
    xi = _noise(key, 11, 0, N)
    n = xi.numel()
    mean, var = float(xi.double().mean()), float(xi.double().var(unbiased=False))
    print(f"noise: n = {n}, mean {mean:.3e} (bound {4 / math.sqrt(n):.3e}), variance - 1 {var - 1:.3e} (bound {4 * math.sqrt(2 / n):.3e}), "
          f"max |xi| {float(xi.abs().max()):.3f}")
    assert bool(torch.isfinite(xi).all())
    assert abs(mean) <= 4 / math.sqrt(n) and abs(var - 1) <= 4 * math.sqrt(2 / n)
    # a shorter launch (another grid) gives the same leading samples
    assert torch.equal(_noise(key, 11, 0, 1000), xi[:1000])
    # the O step's own geometry (a thread per atom and component pair, 256 per workgroup): v = 0 * 0 + 1 * sqrt(1 / 1) * xi
    ones, z = torch.ones(2, device="cuda"), torch.ones(N, dtype=torch.int32, device="cuda")
    v = torch.zeros((N, 3), device="cuda")
    call("gn_md_langevin", ptr(v), ptr(z), ptr(ones), 2, N, 0.0, 1.0, ptr(key), 0, ptr(_state(0, 11)), _stream())
    assert torch.equal(v, xi)
    for other in (_noise(key, 12, 0, N), _noise(key, 11, 1, N), _noise(_key(20240608, 3), 11, 0, N), _noise(_key(20240607, 4), 11, 0, N)):
        assert float((other == xi).float().mean()) < 1e-3
        assert abs(float((other.double() * xi.double()).mean())) <= 4 / math.sqrt(n)      # uncorrelated: a product of unit normals
