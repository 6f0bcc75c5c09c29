"""Cost of the multi-image radius graph against the minimum-image one in the SAME run (a record, not a gate).

System (c) of tests/pbc_util.py: 70 atoms in a 10.5 A cube, cutoff 5, cap 32 -- a cell both searches accept.  Three searches,
each the count launch plus the fill launch on prepared buffers (no host read inside the timed window):
  minimum   gn_radius_count_pbc + gn_radius_fill_pbc
  all       the *_images entry points with the image range graph.image_ranges gives this cell (R = 0: one candidate per pair)
  all_r1    the same with R = 1 forced on every axis (27 candidates per pair: what a cell between cutoff and 2 * cutoff pays)
and the whole ``graph.distance_pbc`` call (cell check, two host reads) for images = "minimum" and "all".
Device events around ``--iters`` back-to-back repetitions, the median of ``--rounds`` rounds in which the variants alternate.

    python tools/pbc_multi_image_time.py --out profiles/pbc_multi_image_graph.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gotennet_amd import graph
    from gotennet_amd._lib import call, ptr
    from gotennet_amd.outputs import molecule_ptr
    from tests import pbc_util as U
    s = U.system("c")
    pos, batch, cell = s["pos"].float().cuda(), s["batch"].cuda(), s["cell"].float().cuda()
    N, n_mol, cap, st = pos.shape[0], 1, 32, torch.cuda.current_stream().cuda_stream
    ref = graph.distance_pbc(pos, batch, cell, U.CUTOFF, cap)
    E = ref[0].shape[1]
    mol_ptr = molecule_ptr(batch, n_mol)
    inv_cell, _ = graph.cell_prepare(cell)
    deg = torch.empty(N, dtype=torch.int32, device="cuda")
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    rowptr[1:] = torch.bincount(ref[0][1], minlength=N).cumsum(0)
    out = (torch.empty((2, E), dtype=torch.int64, device="cuda"), torch.empty((E, 3), dtype=torch.int32, device="cuda"),
           torch.empty((E, 3), dtype=torch.float32, device="cuda"), torch.empty(E, dtype=torch.float32, device="cuda"))
    r0 = graph.image_ranges(cell, U.CUTOFF).cuda()
    r1 = torch.ones((1, 3), dtype=torch.int32, device="cuda")

    def search(sfx, *extra):
        def run():
            box = (ptr(cell), ptr(inv_cell)) + tuple(ptr(t) for t in extra)
            call("gn_radius_count_pbc" + sfx, ptr(pos), ptr(batch), ptr(mol_ptr), *box, N, n_mol, U.CUTOFF, cap, ptr(deg), st)
            call("gn_radius_fill_pbc" + sfx, ptr(pos), ptr(batch), ptr(mol_ptr), *box, N, n_mol, U.CUTOFF, cap, ptr(rowptr), E,
                 *[ptr(t) for t in out], st)
        return run

    variants = {"minimum": search(""), "all": search("_images", r0), "all_r1": search("_images", r1),
                "distance_pbc(minimum)": lambda: graph.distance_pbc(pos, batch, cell, U.CUTOFF, cap),
                "distance_pbc(all)": lambda: graph.distance_pbc(pos, batch, cell, U.CUTOFF, cap, images="all")}
    for name, fn in variants.items():                # warm-up, and the lists are the same bits
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        if not name.startswith("distance"):
            assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[3]) and torch.equal(out[3], ref[1]), name
            out[0].zero_()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters * 1e3)
    lines = [f"# tools/pbc_multi_image_time.py: pbc_util system c ({N} atoms, cube 10.5 A, cutoff 5, cap {cap}, {E} edges); "
             f"image range of this cell {r0.flatten().tolist()}",
             f"# us per count + fill (or per whole call), device events over {a.iters} repetitions, median [min, max] of "
             f"{a.rounds} alternating rounds"]
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        lines.append(f"{k:24s} {med[k]:9.2f}  [{min(v):.2f}, {max(v):.2f}]")
    lines.append(f"ratio all / minimum        {med['all'] / med['minimum']:.2f}")
    lines.append(f"ratio all_r1 / minimum     {med['all_r1'] / med['minimum']:.2f}")
    lines.append(f"ratio distance_pbc all / minimum  {med['distance_pbc(all)'] / med['distance_pbc(minimum)']:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
