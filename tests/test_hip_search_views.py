"""GPU: count, fill and verify are three views of one search.  For each of the three searches (isolated molecules, periodic
minimum image, periodic multi-image), on one batch of boxes whose sizes sit on either side of the 64-lane trip of the
wave-per-target walk: the count's degrees are the row lengths of the filled list, the verify of that list at its own
positions reports nothing, and the list is the host brute force bit for bit in index and shift.

The multi-image cells are between ``cutoff`` and ``2 * cutoff`` wide: image range 1, 27 candidates per pair, so two atoms stay
inside one trip (54 candidates) and three cross it (81).  One cap for all three searches; that it binds in some rows and not
in others is a statement about the INPUT, asserted on the brute force before any launch."""
import functools

import pytest
import torch

from tests import pbc_multi_util as MU
from tests import pbc_util as U

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 63, 64, 65, 129)
CAP = 40
WIDE = (U.TRICLINIC, U.ORTHO, U.CUBE, U.LEFT_HANDED)                       # widths >= 2 * cutoff: the minimum image
NARROW = (MU.N1_CELL, [[8.0, 0.0, 0.0], [0.0, 7.5, 0.0], [0.0, 0.0, 9.0]])    # widths in (cutoff, 2 * cutoff): R = 1
SEARCHES = ("open", "minimum", "all")


@functools.lru_cache(maxsize=None)
def _case(search):
    """-> dict(pos fp64 (fp32-representable), batch, cell or None, index, shift or None, degree = UNCAPPED hits per target,
    gap): the input of one search and its brute-force list under ``CAP``.  Computed once and shared: read-only."""
    cells = NARROW if search == "all" else WIDE
    # (seeds for which no pair image lies within pbc_util.MIN_GAP of the cutoff: the test asserts that about the input)
    gen = torch.Generator().manual_seed({"open": 31, "minimum": 32, "all": 38}[search])
    boxes = [(cells[k % len(cells)], n) for k, n in enumerate(SIZES)]
    pos = torch.cat([U._fill_box(c, n, gen) for c, n in boxes]).float().double()
    batch = torch.cat([torch.full((n,), m, dtype=torch.int64) for m, n in enumerate(SIZES)])
    cell = torch.tensor([c for c, _ in boxes], dtype=torch.float64).float().double()
    if search == "open":                             # the reference of test_hip_parity's radius-graph tests
        from oracle import gotennet_oracle as orc
        index = orc.radius_graph(pos, batch, U.CUTOFF, CAP, loop=True)
        dist = (pos.unsqueeze(1) - pos.unsqueeze(0)).norm(dim=2)
        pair = (batch.unsqueeze(1) == batch.unsqueeze(0)) & ~torch.eye(len(batch), dtype=torch.bool)
        return dict(pos=pos, batch=batch, cell=None, index=index, shift=None, gap=float((dist[pair] - U.CUTOFF).abs().min()),
                    degree=((dist < U.CUTOFF) & (batch.unsqueeze(1) == batch.unsqueeze(0))).sum(1))
    if search == "minimum":
        bf = U.brute_force(pos, batch, cell, U.CUTOFF, CAP)
        degree = torch.cat([h.sum(1) for h in bf["hits"]])
    else:
        bf = MU.brute_force(pos, batch, cell, MU.CUTOFF, CAP)
        assert not bf["border"], "test input: a hit on the border of the enumerated images"
        degree = bf["degree"]
    return dict(pos=pos, batch=batch, cell=cell, index=bf["edge_index"], shift=bf["edge_shift"], gap=bf["gap"], degree=degree)


@pytest.mark.parametrize("search", SEARCHES)
def test_count_fill_verify_agree_with_brute_force(search):
    from gotennet_amd import graph
    from gotennet_amd._lib import call, ptr
    from gotennet_amd.outputs import molecule_ptr
    c = _case(search)
    # ---- the input, on the CPU, before any launch
    assert c["gap"] > U.MIN_GAP, f"test input: a pair lies {c['gap']:.2e} from the cutoff (needs > {U.MIN_GAP})"
    assert bool((c["degree"] > CAP).any()) and bool((c["degree"] < CAP).any()), "test input: the cap must bind in some rows only"
    assert torch.equal(torch.bincount(c["index"][1], minlength=len(c["batch"])), c["degree"].clamp(max=CAP))
    n_mol = len(SIZES)
    if search == "all":
        assert bool((graph.image_ranges(c["cell"], MU.CUTOFF) == 1).all()), "test input: image range 1 on every axis"
    elif search == "minimum":
        graph.check_cell(c["cell"], U.CUTOFF)
    # ---- fill: the brute force, bit for bit in index and shift
    pos, batch = c["pos"].float().cuda(), c["batch"].cuda()
    N, st = pos.shape[0], torch.cuda.current_stream().cuda_stream
    deg = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    state = torch.zeros(1, dtype=torch.int32, device="cuda")
    if search == "open":
        ei = graph.distance(pos, batch, U.CUTOFF, CAP)[0]
        call("gn_radius_count", ptr(pos), ptr(batch), N, U.CUTOFF, CAP, ptr(deg), st)
        changed = graph.list_is_current(pos, batch, ei, U.CUTOFF, CAP, n_mol=n_mol, state=state)
    else:
        cell = c["cell"].float().cuda()
        ei, _, _, sh = graph.distance_pbc(pos, batch, cell, U.CUTOFF, CAP, images=search)
        assert torch.equal(sh.cpu().long(), c["shift"])
        ranges = graph.resolve_images(cell, U.CUTOFF, search)
        assert (ranges is None) == (search == "minimum")
        cell32, inv_cell, ranges = graph.box_arrays(cell, ranges, n_mol, pos.device)
        mol_ptr = molecule_ptr(batch, n_mol)
        box = (ptr(cell32), ptr(inv_cell)) if ranges is None else (ptr(cell32), ptr(inv_cell), ptr(ranges))
        call("gn_radius_count_pbc" + ("" if ranges is None else "_images"), ptr(pos), ptr(batch), ptr(mol_ptr), *box, N, n_mol,
             U.CUTOFF, CAP, ptr(deg), st)
        changed = graph.list_is_current(pos, batch, ei, U.CUTOFF, CAP, cell=cell, edge_shift=sh, images=search, state=state)
    torch.cuda.synchronize()
    assert torch.equal(ei.cpu(), c["index"])
    # ---- count: the row lengths of the filled list
    assert torch.equal(deg.cpu().long(), torch.bincount(ei[1], minlength=N).cpu())
    # ---- verify: the list is current at its own positions, and the sticky word stays 0
    assert tuple(changed.shape) == (n_mol,) and not bool(changed.any())
    assert int(state[0]) == 0
