"""The fp64 yardstick of the multi-image periodic tests (cells narrower than twice the cutoff): a brute-force neighbour list
over ALL images of every pair, the seeded narrow systems, and the replica builder that turns a narrow cell into a
minimum-image system ``pbc_util.brute_force`` / ``pbc_util.oracle_efs`` handle (translation symmetry: the energy of a
k_a x k_b x k_c replica is k_a k_b k_c times the cell's, its forces tile, its stress is equal, its parameter gradients are
k_a k_b k_c times the cell's).  Everything here runs on the CPU in fp64 and shares no code with ``gotennet_amd.graph``."""
import functools
import itertools

import torch

from tests import pbc_util as U

CUTOFF = U.CUTOFF
M = 4                                                                                              # images {-4..4}^3
_IMAGES = torch.tensor(list(itertools.product(range(-M, M + 1), repeat=3)), dtype=torch.float64)   # lexicographic
_ZERO = (len(_IMAGES) - 1) // 2                                                                    # image (0, 0, 0)


def brute_force(pos, batch, cell, cutoff=CUTOFF, max_num_neighbors=32, ranges=None):
    """Every image in {-4..4}^3 of every pair of a box, on positions wrapped into the cell first (so the enumeration covers
    unwrapped inputs); the shifts are mapped back to the ORIGINAL positions.  Order: target-major, sources ascending, within a
    (target, source) pair the shifts ascending lexicographically in (sx, sy, sz) (the map back adds one constant per pair:
    the order of the enumeration survives); the first ``max_num_neighbors`` hits of a target are kept, the self-loop
    (j == i, shift 0) among them.
    -> dict(edge_index int64 [2, E], edge_shift int64 [E, 3], edge_vec fp64 [E, 3], edge_diff fp64 [E] (0 on the self-loop
    only), gap = min | |r| - cutoff | over all pair images but the self-loop, degree int64 [N] (UNCAPPED hits per target),
    t_max int64 [n_mol, 3] = max |s_k + rint(f_k)| over the uncapped hits (f = fractional difference of the original
    positions: the range of images around the rounded difference that the list needs), border = a hit used image index
    +-4 on some axis (the enumeration may then be incomplete: callers assert it is False), and with ``ranges`` (int
    [n_mol, 3]) cand int64 [E]: the position (j - j0) * n_img + t_flat of each kept edge among the candidates of its
    target in a search over t in [-R, R]^3 around -rint(f), tx slowest)."""
    pos, cell = pos.double(), cell.double().reshape(-1, 3, 3)
    N = pos.shape[0]
    src, dst, shifts, cands, gap, border = [], [], [], [], float("inf"), False
    degree = torch.zeros(N, dtype=torch.int64)
    t_max = torch.zeros((cell.shape[0], 3), dtype=torch.int64)
    for m in range(cell.shape[0]):
        idx = (batch == m).nonzero().flatten()
        n = idx.numel()
        if n == 0:
            continue
        c = cell[m]
        inv = torch.linalg.inv(c)
        frac = pos[idx] @ inv
        wrap = torch.floor(frac)                                   # pos_wrapped = pos - wrap @ c
        pw = (frac - wrap) @ c
        d = pw.unsqueeze(0) - pw.unsqueeze(1)                      # [i, j] = pw[j] - pw[i]
        r = d.unsqueeze(2) + (_IMAGES @ c).reshape(1, 1, -1, 3)    # [i, j, image]
        dist = r.norm(dim=3)
        real = torch.ones_like(dist, dtype=torch.bool)
        real[torch.arange(n), torch.arange(n), _ZERO] = False      # the self-loop is no pair image
        gap = min(gap, float((dist[real] - cutoff).abs().min()))
        hit = dist * dist < cutoff * cutoff
        degree[idx] = hit.flatten(1).sum(1)
        ti, sj, im = hit.nonzero(as_tuple=True)                    # row-major: targets, sources, images ascending
        border = border or bool((_IMAGES[im].abs() == M).any())
        rank = torch.cat([torch.arange(int(k)) for k in hit.flatten(1).sum(1)])        # position among the target's hits
        s_all = (_IMAGES[im] - wrap[sj] + wrap[ti]).long()         # shift for the original positions
        f = (pos[idx][sj] - pos[idx][ti]) @ inv
        t = s_all + torch.round(f).long()
        t_max[m] = t.abs().max(0).values
        keep = rank < max_num_neighbors
        src.append(idx[sj][keep]), dst.append(idx[ti][keep]), shifts.append(s_all[keep])
        if ranges is not None:
            R = torch.as_tensor(ranges).reshape(-1, 3)[m].long()
            ny, nz = 2 * int(R[1]) + 1, 2 * int(R[2]) + 1
            n_img = (2 * int(R[0]) + 1) * ny * nz
            tt = t[keep] + R
            cands.append(sj[keep] * n_img + (tt[:, 0] * ny + tt[:, 1]) * nz + tt[:, 2])
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    sh = torch.cat(shifts)
    vec, diff = U.edge_geometry(pos, ei, sh, cell, batch)
    out = dict(edge_index=ei, edge_shift=sh, edge_vec=vec, edge_diff=diff, gap=gap, degree=degree, t_max=t_max, border=border)
    if ranges is not None:
        out["cand"] = torch.cat(cands)
    return out


def assert_input(bf, max_num_neighbors=None):
    """Conditions on a test INPUT, not tolerances: no pair image within ``pbc_util.MIN_GAP`` of the cutoff, the enumeration
    complete, and -- where the caller says the cap must not bite -- every uncapped degree within it."""
    U.assert_gap(bf)
    assert not bf["border"], "test input: a hit on the border of the enumerated images"
    if max_num_neighbors is not None:
        assert int(bf["degree"].max()) <= max_num_neighbors, "test input: the cap bites"


# ------------------------------------------------------------------------------------------------------------ systems
N1_CELL = [[7.2, 0.0, 0.0], [1.0, 6.4, 0.0], [-0.8, 1.2, 8.1]]          # widths 7.06 / 6.33 / 8.10: two images of some pairs
N2_CELL = [[3.9, 0.0, 0.0], [0.7, 4.3, 0.0], [-0.5, 0.9, 3.6]]          # widths 3.79 / 4.17 / 3.60: self-images
R2_CELL = [[2.4, 0.0, 0.0], [0.0, 2.9, 0.0], [0.0, 0.0, 3.3]]           # one atom, image range 2 on every axis
N3_CELL = [[2.9, 0.0, 0.0], [0.0, 2.9, 0.0], [0.0, 0.0, 2.9]]           # one atom: 18 self-images + the self-loop

#: name -> (boxes [(cell, atoms)], seed, replica counts per box)
_SYSTEMS = {
    "n1": ([(N1_CELL, 6)], 21, [(3, 3, 3)]),
    "n2": ([(N2_CELL, 2)], 22, [(3, 3, 3)]),
    "r2": ([(R2_CELL, 1)], 23, [(5, 4, 4)]),
    "n3": ([(N3_CELL, 1)], 24, [(4, 4, 4)]),
    "n4": ([(U.TRICLINIC, 12), (N2_CELL, 2)], 25, [(1, 1, 1), (3, 3, 3)]),      # a wide and a narrow box in one batch
    "n5": ([(N1_CELL, 6)], 21, [(3, 3, 3)]),                                    # n1, every atom moved by up to +-2 lattice vectors
}
#: caps for the list tests, each a statement about the input that test_pbc_multi_host asserts: on n2 a cap that falls
#: between two images of one (target, source) pair; on n1 and r2 a cap that some target first reaches beyond its first 64
#: candidates (a second trip of the wave)
CAP_N2_SPLITS_PAIR = 10
CAP_N1_SECOND_TRIP = 5
CAP_R2_SECOND_TRIP = 16


@functools.lru_cache(maxsize=None)
def system(name: str):
    """-> dict(pos fp64 [N, 3], batch, z, cell fp64 [n_mol, 3, 3], n_mol, reps): fp32-representable values, as
    ``pbc_util.system`` makes them.  Cached: treat as read-only."""
    boxes, seed, reps = _SYSTEMS[name]
    gen = torch.Generator().manual_seed(seed)
    pos = torch.cat([U._fill_box(c, n, gen) for c, n in boxes])
    batch = torch.cat([torch.full((n,), m, dtype=torch.int64) for m, (_, n) in enumerate(boxes)])
    cell = torch.tensor([c for c, _ in boxes], dtype=torch.float64)
    z = torch.randint(1, 9, (pos.shape[0],), generator=gen)
    if name == "n5":
        k = torch.randint(-2, 3, (pos.shape[0], 3), generator=gen).double()
        pos = pos + torch.einsum("na,nab->nb", k, cell[batch])
        assert bool((k != 0).any())
    pos, cell = pos.float().double(), cell.float().double()
    return dict(pos=pos, batch=batch, z=z, cell=cell, n_mol=len(boxes), reps=reps)


def replicate(s):
    """The k_a x k_b x k_c replica of every box of ``s`` (``s["reps"]``) as one system of the same number of boxes ->
    (replica system, owner int64 [N_rep]: the atom of ``s`` each replica atom is a copy of, count fp64 [n_mol]: copies per
    box).  Box by box, copy-major: a box's atoms stay contiguous."""
    pos, cell = s["pos"].double(), s["cell"].double().reshape(-1, 3, 3)
    P, B, Z, own, cells, count = [], [], [], [], [], []
    for m, k in enumerate(s["reps"]):
        idx = (s["batch"] == m).nonzero().flatten()
        for a, b, c in itertools.product(range(k[0]), range(k[1]), range(k[2])):
            P.append(pos[idx] + torch.tensor([a, b, c], dtype=torch.float64) @ cell[m])
            B.append(torch.full((idx.numel(),), m, dtype=torch.int64))
            Z.append(s["z"][idx]), own.append(idx)
        cells.append(cell[m] * torch.tensor(k, dtype=torch.float64).unsqueeze(1))
        count.append(float(k[0] * k[1] * k[2]))
    rep = dict(pos=torch.cat(P), batch=torch.cat(B), z=torch.cat(Z), cell=torch.stack(cells), n_mol=s["n_mol"])
    return rep, torch.cat(own), torch.tensor(count, dtype=torch.float64)


def replica_oracle(sd, cfg, hsd, s, params=False):
    """The fp64 oracle on the replica of ``s``, reduced to the cell: energy / count, the forces of the first copy, the
    stress and its un-cancelled scale, parameter gradients / count (one box only).  Asserts the replica's input conditions
    (gap, minimum image -- ``pbc_util.brute_force`` asserts one image per pair --, the cap does not bite) and that its forces
    tile to 1e-10."""
    rep, owner, count = replicate(s)
    bf = U.brute_force(rep["pos"], rep["batch"], rep["cell"])
    U.assert_gap(bf)
    assert max(int(h.sum(1).max()) for h in bf["hits"] if h.numel()) <= 32, "test input: the cap bites in the replica"
    o = U.oracle_efs(sd, cfg, hsd, rep, bf["edge_index"], bf["edge_shift"], params=params)
    N = s["pos"].shape[0]
    first = torch.stack([(owner == a).nonzero()[0, 0] for a in range(N)])
    forces = o["forces"][first]
    # the force on an atom is a signed sum of its edges' dE/dr_e: ``force_scale`` is the largest un-cancelled such sum (the
    # yardstick for a force that vanishes by symmetry, as on a one-atom cell; what ``scale`` is to the stress)
    r = o["edge_vec"]
    dEdr = o["g_vec"] + o["g_diff"].unsqueeze(1) * r / r.norm(dim=1, keepdim=True).clamp_min(1e-300)
    mass = torch.zeros(rep["pos"].shape[0], dtype=torch.float64)
    mass.index_add_(0, bf["edge_index"][0], dEdr.norm(dim=1)).index_add_(0, bf["edge_index"][1], dEdr.norm(dim=1))
    force_scale = float(mass.max())
    assert float((o["forces"] - forces[owner]).abs().max()) <= 1e-10 * force_scale, "forces do not tile"
    out = dict(energy=o["energy"] / count.reshape(o["energy"].shape), forces=forces, stress=o["stress"], scale=o["scale"],
               n_edges=bf["edge_index"].shape[1], count=count, force_scale=force_scale)
    if params:
        assert s["n_mol"] == 1
        out["param_grads"] = {k: v / count[0] for k, v in o["param_grads"].items()}
    return out
