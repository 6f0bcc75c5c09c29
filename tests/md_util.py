"""Inputs of the MD tests: the stale-list cases of the verify kernels and the small systems of the driver tests.  Plain
torch on the CPU; shares no code with ``gotennet_amd``.

A stale-list case is (base positions, new positions, cap, the molecules expected to be stale): the stored list is the
project's own search at the base positions, the question is whether it still is the search's result at the new ones.
Every expectation here is a statement about the INPUT that the tests assert against the search itself."""
import functools

import numpy as np
import torch

from tests import pbc_multi_util as PM

# ------------------------------------------------------------------------------------- open and minimum-image cases
CUTOFF = 1.5                       # r^2 = 2.25 exactly in fp32
SIZES = (2, 5, 9)
BOX = 10.0                         # cubic cell of the minimum-image runs: width >= 2 * cutoff


def _f32(x):
    return np.float32(x)


def below_threshold(r: float) -> float:
    """An fp32 x whose fp32 square is the nearest representable value below fl(r * r) (asserted)."""
    r2 = _f32(r) * _f32(r)
    want = np.nextafter(r2, _f32(0))
    x = _f32(r)
    for _ in range(64):
        x = np.nextafter(x, _f32(0))
        if x * x == want:
            return float(x)
        assert x * x > want, "no fp32 x squares to the value just below r^2"
    raise AssertionError("no fp32 x squares to the value just below r^2")


def base_positions() -> torch.Tensor:
    """Molecule A: a pair 1.0 apart.  B: five atoms on a line, 1.0 apart (rows of 2 or 3: partly filled).  C: seven atoms
    0.1 apart on a line, one above and one below it, every pair inside the cutoff (rows of 9: the cap of 4 binds, and the
    pair (above, below) is the 8th / 9th hit of either row)."""
    a = [[0.0, 0, 0], [1.0, 0, 0]]
    b = [[float(k), 0, 0] for k in range(5)]
    c = [[0.1 * k, 0, 0] for k in range(7)] + [[0.3, 1.0, 0], [0.3, -0.4, 0]]
    return torch.tensor(a + b + c, dtype=torch.float32)


def batch_vector(sizes=SIZES) -> torch.Tensor:
    return torch.cat([torch.full((n,), m, dtype=torch.int64) for m, n in enumerate(sizes)])


def _moved(pos, moves):
    pos = pos.clone()
    for atom, xyz in moves.items():
        pos[atom] = torch.tensor(xyz, dtype=torch.float32)
    return pos


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (base [16, 3], new [16, 3], cap, stale molecules).  Atoms: A = 0, 1; B = 2 .. 6 (x = 0 .. 4); C = 7 .. 15."""
    p0 = base_positions()
    xb = below_threshold(CUTOFF)
    far = _moved(p0, {1: [1.6, 0, 0], 6: [4.6, 0, 0]})           # A and the last pair of B outside the cutoff
    return {
        "unchanged": (p0, p0, 32, ()),
        "unchanged_cap": (p0, p0, 4, ()),
        "leaves": (p0, _moved(p0, {6: [4.6, 0, 0]}), 32, (1,)),                  # 5-6 at 1.6
        "enters": (p0, _moved(p0, {6: [3.4, 0, 0]}), 32, (1,)),                  # 4-6 at 1.4
        "swap": (p0, _moved(p0, {4: [2.6, 0, 0]}), 32, (1,)),                    # row 4: {3, 4, 5} -> {4, 5, 6}
        # C's pair (14, 15) leaves, beyond the first four hits of either row; B loses an edge
        "beyond_cap": (p0, _moved(p0, {15: [0.3, -0.6, 0], 6: [4.6, 0, 0]}), 4, (1,)),
        "inside_cap": (p0, _moved(p0, {8: [0.1, 5.0, 0]}), 4, (2,)),             # C's second atom leaves every row
        # A lands on the largest d^2 below r^2 (enters); B's last pair lands on d^2 = r^2 exactly (strict <: stays out)
        "threshold": (far, _moved(far, {1: [xb, 0, 0], 6: [4.5, 0, 0]}), 32, (0,)),
        "middle_only": (p0, _moved(p0, {k + 2: [1.6 * k, 0, 0] for k in range(5)}), 32, (1,)),
    }


def wrapped(pos: torch.Tensor) -> torch.Tensor:
    """The same atoms for the periodic runs, two of them moved by a lattice vector of the cubic ``BOX`` (neither belongs to a
    threshold pair): their edges carry a shift."""
    pos = pos.clone()
    pos[2, 0] += BOX
    pos[9, 1] -= BOX
    return pos


# ------------------------------------------------------------------------------------- multi-image cases (cutoff 5.0)
CUTOFF_IMAGES = PM.CUTOFF
T_CELL = [[4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 4.0]]       # the threshold boxes: widths 4 < 2 * cutoff


def _boxes(names):
    pos, cell, sizes = [], [], []
    for n in names:
        if n == "t":                                 # two atoms; the second is placed by the case
            pos.append(torch.zeros((2, 3), dtype=torch.float64)), cell.append(torch.tensor(T_CELL, dtype=torch.float64))
        else:
            s = PM.system(n)
            assert s["n_mol"] == 1
            pos.append(s["pos"]), cell.append(s["cell"][0])
        sizes.append(pos[-1].shape[0])
    return torch.cat(pos).float(), torch.stack(cell).float(), batch_vector(sizes)


def _shifted(pos, moves):
    pos = pos.clone()
    for atom, d in moves.items():
        pos[atom] += torch.tensor(d, dtype=torch.float32)
    return pos


@functools.lru_cache(maxsize=None)
def image_cases():
    """name -> (base, new, cell [3, 3, 3], batch, cap, stale boxes).  Boxes: the two-atom narrow cell ``n2`` (atoms 0, 1),
    the six-atom one ``n1`` (2 .. 7) and the one-atom cell ``n3`` (8: 18 self-images and the self-loop; it moves in most
    cases and its list never changes).  The displacements were chosen on the fp64 brute-force list: no pair image within
    1e-2 of the cutoff before or after.  "threshold" swaps the outer boxes for two-atom cubic cells of width 4."""
    p0, cell, batch = _boxes(("n2", "n1", "n3"))
    drift = {8: [0.3, -0.2, 0.1]}
    out = {
        "unchanged": (p0, p0, 32, ()),
        "unchanged_cap": (p0, p0, 4, ()),
        "leaves": (p0, _shifted(p0, {4: [0.0156, 0.068, -0.0032], **drift}), 32, (1,)),
        "enters": (p0, _shifted(p0, {7: [0.1704, -0.006, 0.1854], **drift}), 32, (1,)),
        "swap": (p0, _shifted(p0, {4: [0.0404, 0.2909, 0.0233], **drift}), 32, (1,)),
        "beyond_cap": (p0, _shifted(p0, {1: [0.1704, -0.006, 0.1854], 4: [0.0156, 0.068, -0.0032], **drift}), 4, (1,)),
        "inside_cap": (p0, _shifted(p0, {0: [0.0404, 0.2909, 0.0233], **drift}), 4, (0,)),
        "middle_only": (p0, _shifted(p0, {4: [0.0156, 0.068, -0.0032], 7: [0.1704, -0.006, 0.1854]}), 32, (1,)),
    }
    out = {k: (b, n, cell, batch, cap, stale) for k, (b, n, cap, stale) in out.items()}
    # threshold: the image with shift 0 of the pair (0, 0, 0) -> (0, 3, z) has d^2 = fl(9 + fl(z^2)).  z = 4 - 2^-22: z^2 rounds to
    # 16 - 2^-19 and d^2 = 25 - 2^-19, the value just below r^2 = 25 (a hit: box 0 goes stale); z = 4: d^2 = 25 exactly, as for the
    # images (0, 3, -4), (+-4, 3, 0) and (0, -5, 0) (strict <: no hit): box 2 sits there and is translated as a whole by fp32-exact
    # amounts -- the same differences, the same list (any move of one atom alone would pull one of those images inside)
    t0, tcell, tbatch = _boxes(("t", "n1", "t"))
    lo = float(np.nextafter(_f32(4), _f32(0)))
    assert _f32(9) + _f32(lo) * _f32(lo) == np.nextafter(_f32(25), _f32(0)) and _f32(9) + _f32(4) * _f32(4) == _f32(25)
    base = _shifted(t0, {1: [0, 3, 4.0], 9: [0, 3, 4.0]})
    new = _shifted(t0, {1: [0, 3, lo], 8: [0.5, 0.25, 0.125], 9: [0.5, 3.25, 4.125]})
    out["threshold"] = (base, new, tcell, tbatch, 32, (0,))
    return out


# ------------------------------------------------------------------------------------------------ driver systems
def md_molecules():
    """Three small molecules (3, 4 and 5 atoms) for the driver tests, cutoff 5.0 (``pbc_util.CUTOFF``): spacings of about 1.6, and
    in the second one an end atom 4.9 from the other end that flies outwards -- its pair crosses the cutoff within the first few
    steps.  -> dict(pos, vel, z, batch, n_mol)."""
    pos = torch.tensor([[0.0, 0, 0], [1.5, 0.2, 0], [2.9, -0.3, 0.4],
                        [0.0, 0, 0], [1.6, 0.1, 0.0], [3.2, -0.1, 0.2], [4.88, 0.0, 0.3],
                        [0.0, 0, 0], [1.4, 0.5, 0], [2.7, -0.4, 0.3], [1.2, 1.9, -0.2], [3.9, 0.6, 0.8]], dtype=torch.float32)
    vel = torch.zeros_like(pos)
    vel[6] = torch.tensor([0.1, 0.0, 0.0])
    vel[3] = torch.tensor([-0.1, 0.0, 0.0])
    z = torch.tensor([8, 1, 1, 6, 6, 8, 1, 6, 7, 8, 1, 1], dtype=torch.int64)
    return dict(pos=pos, vel=vel, z=z, batch=batch_vector((3, 4, 5)), n_mol=3)
