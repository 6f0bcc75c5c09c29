"""Cost of periodic boundary conditions against the isolated-molecule path of the SAME run (a record, not a gate).

Two systems, the benchmark's model (n_atom_basis 256, 6 interactions, lmax 2, cutoff 5, 32 neighbours):
  box512   one 512-atom box (a jittered 8 x 8 x 8 grid in a 17.2 A cube, ~0.1 atoms / A^3)
  c2_boxes the C2 batch (128 aspirin molecules), each molecule in its own 12 A cubic box
and three ratios each, periodic over plain:
  distance   graph.distance_pbc against graph.distance on the same atoms (both include their host reads)
  eager      EnergyForces with and without ``cell`` on the same (periodic) edges: the cost of gn_cell_prepare + gn_virial
  captured   one CapturedStep replay with and without ``cell`` on the same edge list (the plain step drops the lattice shifts,
             so its geometry differs; the launches and their sizes do not)
Times are host clocks around work that ends in a device synchronise, the median of ``--rounds`` alternating rounds.  One
hipGraph is alive at a time, with a synchronise between phases and after the first replay.

    python tools/pbc_step_time.py --out profiles/pbc_step_time.json
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CUTOFF, MAX_NBR = 5.0, 32


def box512():
    g = torch.Generator().manual_seed(0)
    side, n = 17.2, 8
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float32)] * 3, indexing="ij"), dim=-1).reshape(-1, 3)
    pos = (grid + 0.5) * (side / n) + 0.3 * (torch.rand((n ** 3, 3), generator=g) - 0.5)
    return pos, torch.zeros(n ** 3, dtype=torch.int64), torch.randint(1, 9, (n ** 3,), generator=g), torch.eye(3).unsqueeze(0) * side


def c2_boxes():
    from gotennet_amd import synthetic
    pos, batch, z = synthetic.make_batch("rmd17_aspirin", 128, seed=0)
    n_mol = int(batch.max()) + 1
    lo = torch.full((n_mol, 3), float("inf")).scatter_reduce_(0, batch.unsqueeze(1).expand(-1, 3), pos, "amin")
    return pos - lo[batch] + 1.0, batch, z, (torch.eye(3) * 12.0).unsqueeze(0).repeat(n_mol, 1, 1)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(fa, fb, iters, rounds, warmup=3):
    """Median ms of two callables timed in alternating rounds -> (a, b)."""
    for f in (fa, fb):
        for _ in range(warmup):
            f()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, iters))
        tb.append(timed(fb, iters))
    return statistics.median(ta), statistics.median(tb)


def captured(make, pos, iters, rounds):
    """Median replay ms of a CapturedStep built by ``make()``; the step and its graph are dropped before returning."""
    step = make()
    torch.cuda.synchronize()
    step(pos)
    torch.cuda.synchronize()                         # after the first replay
    t = [timed(lambda: step(pos), iters) for _ in range(rounds)]
    del step
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return statistics.median(t)


def measure(name, system, rep, head, iters, rounds):
    from gotennet_amd import graph
    from gotennet_amd.pipeline import CapturedStep, EnergyForces
    pos, batch, z, cell = (t.cuda() for t in system)
    n_mol = cell.shape[0]
    graph.check_cell(cell, CUTOFF)
    out = dict(system=name, atoms=pos.shape[0], boxes=n_mol)
    a, b = alternate(lambda: graph.distance_pbc(pos, batch, cell, CUTOFF, MAX_NBR), lambda: graph.distance(pos, batch, CUTOFF, MAX_NBR),
                     iters * 5, rounds)
    ei, ed, ev, sh = graph.distance_pbc(pos, batch, cell, CUTOFF, MAX_NBR)
    out.update(edges=ei.shape[1], edges_isolated=graph.distance(pos, batch, CUTOFF, MAX_NBR)[0].shape[1],
               distance_pbc_ms=a, distance_ms=b, distance_ratio=a / b)
    torch.cuda.synchronize()
    ef = EnergyForces(rep, head, check_edges=False)
    a, b = alternate(lambda: ef(z, ei, ed, ev, batch, n_mol, cell=cell), lambda: ef(z, ei, ed, ev, batch, n_mol), iters, rounds)
    out.update(eager_cell_ms=a, eager_ms=b, eager_ratio=a / b)
    ef.clear_cache()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(2):                               # one graph alive at a time: periodic, plain, periodic, plain
        ta.append(captured(lambda: CapturedStep(ef, z, ei, batch, n_mol, cell=cell, edge_shift=sh), pos, iters, rounds))
        tb.append(captured(lambda: CapturedStep(ef, z, ei, batch, n_mol), pos, iters, rounds))
    a, b = statistics.median(ta), statistics.median(tb)
    out.update(captured_cell_ms=a, captured_ms=b, captured_ratio=a / b)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pbc_step_time needs a ROCm device: times are measured, never estimated")
    import gotennet_amd
    from gotennet_amd.outputs import Atomwise
    torch.manual_seed(0)
    rep = gotennet_amd.GotenNet(n_atom_basis=256, n_interactions=6, n_rbf=32, cutoff_fn=gotennet_amd.CosineCutoff(CUTOFF),
                                num_heads=8, scale_edge=False, lmax=2, sep_dir=True, sep_tensor=True).cuda().eval()
    head = Atomwise(n_in=256, n_hidden=256, derivative="forces", activation="silu").cuda().eval()
    rec = dict(tool="tools/pbc_step_time.py", device=torch.cuda.get_device_name(0), model="F=256 L=6 lmax=2 cutoff=5 max_nbr=32",
               iters=a.iters, rounds=a.rounds, note="ms per call, medians; ratios are periodic / plain of the same run",
               captured_note="the plain captured step runs on the periodic edge list without its lattice shifts: another "
                             "geometry (some edges beyond the cutoff), the same launches and sizes",
               systems=[measure("box512", box512(), rep, head, a.iters, a.rounds),
                        measure("c2_boxes", c2_boxes(), rep, head, a.iters, a.rounds)])
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
