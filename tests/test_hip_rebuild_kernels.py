"""GPU: the kernels of a neighbour list that is rebuilt on the device -- gn_degree_scan, gn_padded_tail and gn_graph_refresh,
called directly, around the searches' own count and fill.  The real columns are held to ``graph.distance`` /
``graph.distance_pbc`` bit for bit, the tail to the torch restatement of tests/rebuild_util.py, the refresh to the three entry
points it stands for; every output buffer carries guard words behind it."""
import functools

import pytest
import torch

from tests import md_util as MU
from tests import rebuild_util as RU

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = {torch.int32: -7, torch.int64: -7, torch.float32: 12345.0}


def _guarded(shape, dtype):
    """(the whole allocation, a contiguous view of ``shape`` at its head): pattern-filled, GUARD words behind the view."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + GUARD,), PATTERN[dtype], dtype=dtype, device="cuda")
    return flat, flat[:n].view(shape)


def _guards_intact(bufs):
    for name, (flat, view) in bufs.items():
        tail = flat[view.numel():]
        assert tail.numel() == GUARD and bool((tail == PATTERN[flat.dtype]).all()), f"guard words behind {name} were written"


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------ the scan
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_degree_scan_is_cumsum(N):
    from gotennet_amd._lib import call, ptr
    deg = torch.randint(1, 34, (N,), generator=torch.Generator().manual_seed(N), dtype=torch.int32)
    bufs = dict(rowptr64=_guarded((N + 1,), torch.int64), n_edges=_guarded((1,), torch.int32))
    d = deg.cuda()
    call("gn_degree_scan", ptr(d), N, ptr(bufs["rowptr64"][1]), ptr(bufs["n_edges"][1]), _stream())
    torch.cuda.synchronize()
    want = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(deg.long(), 0)])
    assert torch.equal(bufs["rowptr64"][1].cpu(), want)
    assert int(bufs["n_edges"][1].item()) == int(want[-1])
    assert torch.equal(d.cpu(), deg)                                   # the input is read only
    _guards_intact(bufs)


# -------------------------------------------------------------------------------- count -> scan -> fill -> tail
def _search_cases():
    """name -> dict(pos, batch, n_mol, cutoff, cap, cell or None, images): every case of md_util at its new positions, open and
    wrapped into the minimum-image box, the multi-image ones, and the extremes."""
    out = {}
    batch = MU.batch_vector()
    box = torch.eye(3) * MU.BOX
    for name, (_, new, cap, _) in MU.cases().items():
        out["open-" + name] = dict(pos=new, batch=batch, n_mol=3, cutoff=MU.CUTOFF, cap=cap, cell=None, images="minimum")
        out["box-" + name] = dict(pos=MU.wrapped(new), batch=batch, n_mol=3, cutoff=MU.CUTOFF, cap=cap, cell=box, images="minimum")
    for name, (_, new, cell, b, cap, _) in MU.image_cases().items():
        out["images-" + name] = dict(pos=new, batch=b, n_mol=3, cutoff=MU.CUTOFF_IMAGES, cap=cap, cell=cell, images="all")
    # only self-loops remain: the longest tail
    far = torch.zeros((16, 3))
    far[:, 0] = 100.0 * torch.arange(16)
    out["open-far"] = dict(pos=far, batch=batch, n_mol=3, cutoff=MU.CUTOFF, cap=32, cell=None, images="minimum")
    # molecule C alone with cap 4: every target is at its cap, E = e_bound, the tail is one slot per dummy
    c = MU.base_positions()[7:]
    out["open-C-cap4"] = dict(pos=c, batch=torch.zeros(9, dtype=torch.int64), n_mol=1, cutoff=MU.CUTOFF, cap=4, cell=None,
                              images="minimum")
    # E_real == e_bound on a batch of four molecules (tests/test_dynamic_step_host.py: 498 edges)
    sizes = [3, 21, 1, 40]
    pos = torch.rand((65, 3), generator=torch.Generator().manual_seed(2)) * 4.0 / 3 ** 0.5
    out["open-full"] = dict(pos=pos, batch=torch.repeat_interleave(torch.arange(4), torch.tensor(sizes)), n_mol=4, cutoff=5.0,
                            cap=8, cell=None, images="minimum", expect_edges=498)
    return out


CASES = _search_cases()


@functools.lru_cache(maxsize=None)
def _rebuilt(name):
    """The chain on case ``name`` through the entry points -> dict(layout, the guarded buffers, state, the reference list of
    ``graph.distance*``).  Computed once; read-only."""
    from gotennet_amd import graph
    from gotennet_amd._lib import call, ptr
    from gotennet_amd.outputs import molecule_ptr
    c = CASES[name]
    pos, batch, n_mol, cutoff, cap = c["pos"].float().cuda().contiguous(), c["batch"].cuda(), c["n_mol"], c["cutoff"], c["cap"]
    ranges = graph.resolve_images(c["cell"], cutoff, c["images"]) if c["cell"] is not None else None
    lay = graph.PaddedLayout(c["batch"], n_mol, cap, periodic_images=ranges is not None)
    N, capacity = lay.N, lay.edge_capacity
    bufs = dict(deg=_guarded((N,), torch.int32), rowptr64=_guarded((N + 1,), torch.int64), n_edges=_guarded((1,), torch.int32),
                edge_index=_guarded((2, capacity), torch.int64), edge_vec=_guarded((capacity, 3), torch.float32),
                edge_diff=_guarded((capacity,), torch.float32), state=_guarded((2,), torch.int32))
    bufs["state"][1].zero_()
    v = {k: b[1] for k, b in bufs.items()}
    if c["cell"] is None:
        entry, search, outs, shift = "", (ptr(pos), ptr(batch), N, cutoff, cap), (ptr(v["edge_index"]),), None
        ref = graph.distance(pos, batch, cutoff, cap) + (None,)
    else:
        bufs["edge_shift"] = _guarded((capacity, 3), torch.int32)
        shift = bufs["edge_shift"][1]
        cell, inv_cell, rng = graph.box_arrays(c["cell"].float(), ranges, n_mol, pos.device)
        mol_ptr = molecule_ptr(batch, n_mol)
        box = (ptr(cell), ptr(inv_cell)) + (() if rng is None else (ptr(rng),))
        entry = "_pbc" if rng is None else "_pbc_images"
        search = (ptr(pos), ptr(batch), ptr(mol_ptr), *box, N, n_mol, cutoff, cap)
        outs = (ptr(v["edge_index"]), ptr(shift))
        ref = graph.distance_pbc(pos, batch, c["cell"].float().cuda(), cutoff, cap, n_mol=n_mol, images=c["images"])
    st = _stream()
    call("gn_radius_count" + entry, *search, ptr(v["deg"]), st)
    call("gn_degree_scan", ptr(v["deg"]), N, ptr(v["rowptr64"]), ptr(v["n_edges"]), st)
    call("gn_radius_fill" + entry, *search, ptr(v["rowptr64"]), capacity, *outs, ptr(v["edge_vec"]), ptr(v["edge_diff"]), st)
    call("gn_padded_tail", ptr(v["rowptr64"]), N, lay.n_pad, capacity, ptr(v["edge_index"]), ptr(shift), ptr(v["edge_vec"]),
         ptr(v["edge_diff"]), ptr(v["state"]), st)
    torch.cuda.synchronize()
    return dict(lay=lay, bufs=bufs, ref=ref)


@pytest.mark.parametrize("name", sorted(CASES))
def test_rebuilt_list_is_the_search_plus_the_tail(name):
    r = _rebuilt(name)
    lay, bufs = r["lay"], r["bufs"]
    ei, ed, ev, sh = r["ref"]                                          # graph.distance*: (index, diff, vec, shift)
    E, N, capacity = ei.shape[1], lay.N, lay.edge_capacity
    v = {k: b[1] for k, b in bufs.items()}
    assert N <= E <= lay.e_bound
    if "expect_edges" in CASES[name]:
        assert E == CASES[name]["expect_edges"] == lay.e_bound
    if name == "open-far":
        assert E == N
    if name == "open-C-cap4":
        assert E == lay.e_bound == 36
    assert int(v["n_edges"].item()) == E == int(v["rowptr64"][-1].item())
    assert v["state"].tolist() == [0, 0]                               # the sticky word stays clear; its neighbour is untouched
    # the real columns: the search's own bits
    assert torch.equal(v["edge_index"][:, :E], ei)
    assert torch.equal(v["edge_vec"][:E], ev) and torch.equal(v["edge_diff"][:E], ed)
    if sh is not None:
        assert torch.equal(v["edge_shift"][:E], sh)
    # the tail: the restatement
    own = RU.tail_owner(N, lay.n_pad, capacity, E)
    want, wv, wd, ws = RU.padded_list(N, lay.n_pad, capacity, ei.cpu(), ev.cpu(), ed.cpu(), None if sh is None else sh.cpu())
    assert torch.equal(v["edge_index"].cpu(), want) and torch.equal(v["edge_index"][0, E:].cpu(), own)
    assert torch.equal(v["edge_vec"].cpu(), wv) and torch.equal(v["edge_diff"].cpu(), wd)
    if sh is not None:
        assert torch.equal(v["edge_shift"].cpu(), ws)
    assert torch.bincount(own - N, minlength=lay.n_pad).tolist() == lay.tail_degrees(E)
    if E == lay.e_bound:
        assert own.tolist() == list(range(N, N + lay.n_pad))           # exactly one slot per dummy
    assert bool((v["edge_index"][1, 1:] >= v["edge_index"][1, :-1]).all())      # target-major throughout
    _guards_intact(bufs)


# ------------------------------------------------------------------------------------------------------ the refresh
def _topology_reference(ei, n_atoms):
    """gn_build_csr + gn_out_degree + gn_build_csc on fresh buffers -> the seven arrays."""
    from gotennet_amd._lib import call, ptr
    E = ei.shape[1]
    i32 = dict(dtype=torch.int32, device="cuda")
    src, dst, rowptr = torch.empty(E, **i32), torch.empty(E, **i32), torch.empty(n_atoms + 1, **i32)
    outdeg = torch.zeros(n_atoms, **i32)
    colptr, perm, tgt, work = torch.empty(n_atoms + 1, **i32), torch.empty(E, **i32), torch.empty(E, **i32), torch.empty(n_atoms + E, **i32)
    st = _stream()
    call("gn_build_csr", ptr(ei), E, n_atoms, ptr(src), ptr(dst), ptr(rowptr), st)
    call("gn_out_degree", ptr(src), E, ptr(outdeg), st)
    call("gn_build_csc", ptr(src), ptr(dst), E, n_atoms, ptr(colptr), ptr(perm), ptr(tgt), ptr(work), st)
    torch.cuda.synchronize()
    return dict(src=src, dst=dst, rowptr=rowptr, outdeg=outdeg, colptr=colptr, perm=perm, tgt_by_src=tgt)


@pytest.mark.parametrize("names", [("open-unchanged", "open-far", "open-leaves"), ("box-swap", "box-middle_only"),
                                   ("images-enters", "images-leaves"), ("open-full",), ("open-C-cap4",)],
                         ids=lambda n: "+".join(n))
def test_graph_refresh_is_csr_outdegree_csc(names):
    """The lists of ``names`` share one layout: each is refreshed into the SAME buffers (garbage at first, then the previous
    list's arrays and counters), which shows the zeroing inside the kernels."""
    from gotennet_amd._lib import call, ptr
    lay = _rebuilt(names[0])["lay"]
    n_atoms, capacity = lay.n_atoms, lay.edge_capacity
    sizes = dict(src=capacity, dst=capacity, rowptr=n_atoms + 1, outdeg=n_atoms, colptr=n_atoms + 1, perm=capacity,
                 tgt_by_src=capacity, work=n_atoms + capacity)
    bufs = {k: _guarded((n,), torch.int32) for k, n in sizes.items()}
    v = {k: b[1] for k, b in bufs.items()}
    for name in names:
        r = _rebuilt(name)
        assert (r["lay"].n_atoms, r["lay"].edge_capacity) == (n_atoms, capacity)
        ei = r["bufs"]["edge_index"][1]
        for with_outdeg in (True, False):
            kept = v["outdeg"].clone()
            call("gn_graph_refresh", ptr(ei), capacity, n_atoms, ptr(v["src"]), ptr(v["dst"]), ptr(v["rowptr"]),
                 ptr(v["outdeg"]) if with_outdeg else None, ptr(v["colptr"]), ptr(v["perm"]), ptr(v["tgt_by_src"]), ptr(v["work"]),
                 _stream())
            torch.cuda.synchronize()
            want = _topology_reference(ei, n_atoms)
            for k, w in want.items():
                if k == "outdeg" and not with_outdeg:
                    assert torch.equal(v[k], kept), "outdeg was written though none was asked for"
                    continue
                assert torch.equal(v[k], w), f"{name}: {k} differs"
            _guards_intact(bufs)
    # every row of a padded list holds an edge: no atom, real or dummy, is isolated
    assert int((v["rowptr"][1:] - v["rowptr"][:-1]).min()) >= 1


def test_graph_refresh_empty_list():
    from gotennet_amd._lib import call, ptr
    bufs = {k: _guarded((n,), torch.int32) for k, n in dict(rowptr=6, outdeg=5, colptr=6, work=5).items()}
    v = {k: b[1] for k, b in bufs.items()}
    call("gn_graph_refresh", None, 0, 5, None, None, ptr(v["rowptr"]), ptr(v["outdeg"]), ptr(v["colptr"]), None, None,
         ptr(v["work"]), _stream())
    torch.cuda.synchronize()
    assert v["rowptr"].tolist() == [0] * 6 and v["colptr"].tolist() == [0] * 6 and v["outdeg"].tolist() == [0] * 5
    _guards_intact(bufs)


# ------------------------------------------------------------------------------------------------------ the guard
@pytest.mark.parametrize("shifts", [False, True], ids=["open", "periodic"])
@pytest.mark.parametrize("e_real", ["capacity", "above", "below", "negative"])
def test_tail_guard_sets_the_word_and_writes_nothing(e_real, shifts):
    """An edge count outside [N, capacity - n_pad] -- an argument the host's bound excludes -- is handled in bounds: nothing is
    written, the sticky word is set."""
    from gotennet_amd._lib import call, ptr
    N, n_pad, capacity = 16, 5, 160
    E = dict(capacity=capacity, above=capacity - n_pad + 1, below=N - 1, negative=-3)[e_real]
    rowptr64 = torch.zeros(N + 1, dtype=torch.int64)
    rowptr64[N] = E
    rowptr64 = rowptr64.cuda()
    bufs = dict(edge_index=_guarded((2, capacity), torch.int64), edge_vec=_guarded((capacity, 3), torch.float32),
                edge_diff=_guarded((capacity,), torch.float32), edge_shift=_guarded((capacity, 3), torch.int32),
                state=_guarded((2,), torch.int32))
    bufs["state"][1].zero_()
    v = {k: b[1] for k, b in bufs.items()}
    call("gn_padded_tail", ptr(rowptr64), N, n_pad, capacity, ptr(v["edge_index"]), ptr(v["edge_shift"]) if shifts else None,
         ptr(v["edge_vec"]), ptr(v["edge_diff"]), ptr(v["state"]), _stream())
    torch.cuda.synchronize()
    assert v["state"].tolist() == [1, 0]
    for k in ("edge_index", "edge_vec", "edge_diff", "edge_shift"):
        assert bool((bufs[k][0] == PATTERN[bufs[k][0].dtype]).all()), f"{k} was written"
    _guards_intact(bufs)
    # the two ends of the valid range write their tails and leave the word alone (the shortest tail first: the columns in front
    # of either tail still hold the pattern)
    for ok in (capacity - n_pad, N):
        rowptr64[N] = ok
        v["state"].zero_()
        call("gn_padded_tail", ptr(rowptr64), N, n_pad, capacity, ptr(v["edge_index"]), ptr(v["edge_shift"]) if shifts else None,
             ptr(v["edge_vec"]), ptr(v["edge_diff"]), ptr(v["state"]), _stream())
        torch.cuda.synchronize()
        assert v["state"].tolist() == [0, 0]
        own = RU.tail_owner(N, n_pad, capacity, ok).cuda()
        assert torch.equal(v["edge_index"][0, ok:], own) and torch.equal(v["edge_index"][1, ok:], own)
        assert bool((v["edge_index"][:, :ok] == PATTERN[torch.int64]).all())       # the real columns are the fill's, not the tail's
        assert bool((v["edge_vec"][ok:] == 0).all()) and bool((v["edge_diff"][ok:] == 0).all())
        assert bool(((v["edge_shift"][ok:] == 0) if shifts else (v["edge_shift"] == PATTERN[torch.int32])).all())
        _guards_intact(bufs)
