"""A/B of the neighbour searches of csrc/gn_graph.hip between two builds of the library (same ABI): the same bits, the same speed.

One run is one library (``GN_LIB_PATH`` selects it; default the product library) in a fresh process:

    GN_LIB_PATH=gotennet_amd/variants/lib_parent.so python tools/graph_search_ab.py --dump parent.pkl --time parent_0.json
    python tools/graph_search_ab.py --dump new.pkl --time new_0.json          (alternate the two for more timing rounds)
    python tools/graph_search_ab.py --compare parent.pkl new.pkl --times-first 'parent_*.json' --times-second 'new_*.json'

``--dump``: every output array of the nine gn_radius_{count,fill,verify}[_pbc[_images]] entry points and of the two
gn_edge_vectors* ones (deg; edge_index, edge_shift, edge_vec, edge_diff; row_flag, changed, state; the fixed-list vectors) on
the systems of tests/pbc_util.py, tests/pbc_multi_util.py, tests/md_util.cases() and image_cases().  Every system runs every
search its input allows (open: boxes as molecules; minimum image; multi-image with the host's range, and with R = 1 forced);
the list is built at the base positions and verified there and at the case's new positions.
``--time``: us per count + fill and per verify of each search on prepared buffers, no host read in the window: system c of
pbc_util (70 atoms) for the open and the minimum-image search, 70 atoms in a cell of width 7.5 .. 9 (R = 1) for the
multi-image one.  Device events around ``--iters`` back-to-back repetitions, ``--rounds`` rounds in which the entries alternate.
``--compare``: one EQUAL / DIFFERS line per system and entry, byte for byte; with ``--times-*``, per entry the second
library's median against the first one's [min, max] over all its rounds."""
import argparse
import glob
import json
import os
import pickle
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R1_CELL = [[8.0, 0.0, 0.0], [0.0, 7.5, 0.0], [0.0, 0.0, 9.0]]


class Search:
    """One search on prepared device buffers: count, scan (one host read, outside any timed window), fill, verify."""

    def __init__(self, kind, pos, batch, n_mol, cutoff, cap, cell=None, ranges=None):
        from gotennet_amd import graph
        from gotennet_amd._lib import ptr
        from gotennet_amd.outputs import molecule_ptr
        self.kind, self.pos, self.batch, self.n_mol, self.cutoff, self.cap = kind, pos, batch, n_mol, float(cutoff), int(cap)
        self.N, self.st = pos.shape[0], torch.cuda.current_stream().cuda_stream
        self.mol_ptr = molecule_ptr(batch, n_mol)
        self.cell = self.ranges = None
        self.sfx, self.box = "", ()
        if kind != "open":
            self.cell, self.inv_cell, self.ranges = graph.box_arrays(cell, ranges, n_mol, pos.device)
            self.sfx = "_pbc" if ranges is None else "_pbc_images"
            self.box = (ptr(self.mol_ptr), ptr(self.cell), ptr(self.inv_cell)) + (() if ranges is None else (ptr(self.ranges),))
        self.tail = (self.N,) + (() if kind == "open" else (n_mol,)) + (self.cutoff, self.cap)
        i32 = dict(dtype=torch.int32, device=pos.device)
        self.deg = torch.zeros(self.N, **i32)
        self.count()
        self.rowptr = torch.zeros(self.N + 1, dtype=torch.int64, device=pos.device)
        torch.cumsum(self.deg, 0, out=self.rowptr[1:])
        self.E = E = int(self.rowptr[-1].item()) if self.N else 0
        f32 = dict(dtype=torch.float32, device=pos.device)
        self.edge_index = torch.zeros((2, E), dtype=torch.int64, device=pos.device)
        self.edge_shift = torch.zeros((E, 3), **i32)
        self.edge_vec, self.edge_diff = torch.zeros((E, 3), **f32), torch.zeros(E, **f32)
        self.fixed_vec, self.fixed_diff = torch.zeros((E, 3), **f32), torch.zeros(E, **f32)
        self.fill()
        from gotennet_amd._lib import call
        self.src, self.dst, self.rowptr32 = torch.zeros(E, **i32), torch.zeros(E, **i32), torch.zeros(self.N + 1, **i32)
        call("gn_build_csr", ptr(self.edge_index), E, self.N, ptr(self.src), ptr(self.dst), ptr(self.rowptr32), self.st)
        self.row_flag, self.changed, self.state = torch.zeros(self.N, **i32), torch.zeros(n_mol, **i32), torch.zeros(1, **i32)

    def count(self):
        from gotennet_amd._lib import call, ptr
        call("gn_radius_count" + self.sfx, ptr(self.pos), ptr(self.batch), *self.box, *self.tail, ptr(self.deg), self.st)

    def fill(self):
        from gotennet_amd._lib import call, ptr
        outs = (ptr(self.edge_index),) + (() if self.kind == "open" else (ptr(self.edge_shift),))
        call("gn_radius_fill" + self.sfx, ptr(self.pos), ptr(self.batch), *self.box, *self.tail, ptr(self.rowptr), self.E,
             *outs, ptr(self.edge_vec), ptr(self.edge_diff), self.st)

    def verify(self, pos=None):
        from gotennet_amd import graph
        pos = self.pos if pos is None else pos
        kw = {} if self.kind == "open" else dict(shift=self.edge_shift, cell=self.cell, inv_cell=self.inv_cell,
                                                 image_range=self.ranges)
        graph.verify_list(pos, self.batch, self.mol_ptr, self.n_mol, self.rowptr32, self.src, self.cutoff, self.cap,
                          self.row_flag, self.changed, self.state, **kw)

    def fixed_list(self, pos):
        from gotennet_amd._lib import call, ptr
        if self.kind == "open":
            call("gn_edge_vectors", ptr(pos), ptr(self.src), ptr(self.dst), self.E, ptr(self.fixed_vec), ptr(self.fixed_diff), self.st)
        else:
            call("gn_edge_vectors_pbc", ptr(pos), ptr(self.src), ptr(self.dst), ptr(self.edge_shift), ptr(self.cell),
                 ptr(self.batch), self.E, self.n_mol, ptr(self.fixed_vec), ptr(self.fixed_diff), self.st)


def systems():
    """-> [(name, base pos, new pos, batch, cell or None, n_mol, cutoff, caps)], CPU tensors."""
    from tests import md_util as MD
    from tests import pbc_multi_util as MU
    from tests import pbc_util as U
    out = []
    for name in "abcde":
        s = U.system(name)
        out.append(("pbc_util/" + name, s["pos"], s["pos"], s["batch"], s["cell"], s["n_mol"], U.CUTOFF,
                    (32,) + (U.CAPS_C if name == "c" else ())))
    caps = {"n1": (32, MU.CAP_N1_SECOND_TRIP), "n2": (32, MU.CAP_N2_SPLITS_PAIR), "r2": (32, MU.CAP_R2_SECOND_TRIP)}
    for name in ("n1", "n2", "r2", "n3", "n4", "n5"):
        s = MU.system(name)
        out.append(("pbc_multi_util/" + name, s["pos"], s["pos"], s["batch"], s["cell"], s["n_mol"], MU.CUTOFF, caps.get(name, (32,))))
    box = torch.eye(3) * MD.BOX
    for name, (base, new, cap, _) in MD.cases().items():
        out.append(("md_util.cases/" + name, base, new, MD.batch_vector(), None, len(MD.SIZES), MD.CUTOFF, (cap,)))
        out.append(("md_util.cases/" + name + "/wrapped", MD.wrapped(base), MD.wrapped(new), MD.batch_vector(), box, len(MD.SIZES),
                    MD.CUTOFF, (cap,)))
    for name, (base, new, cell, batch, cap, _) in MD.image_cases().items():
        out.append(("md_util.image_cases/" + name, base, new, batch, cell, cell.shape[0], MD.CUTOFF_IMAGES, (cap,)))
    return out


def dump(path):
    from gotennet_amd import graph
    arrays = {}
    for name, base, new, batch, cell, n_mol, cutoff, caps in systems():
        base, new, batch = base.float().cuda(), new.float().cuda(), batch.cuda()
        kinds = [("open", None, None)]
        if cell is not None:
            cell = cell.float()
            r1 = torch.ones((n_mol, 3), dtype=torch.int32)
            kinds += [("minimum", cell, None), ("all", cell, graph.image_ranges(cell, cutoff)), ("all_r1", cell, r1)]
        for kind, c, ranges in kinds:
            for cap in caps:
                s = Search(kind, base, batch, n_mol, cutoff, cap, c, ranges)
                key = f"{name} cap {cap} {kind}"
                arrays[key + " count"] = [s.deg]
                arrays[key + " fill"] = [s.edge_index, s.edge_shift, s.edge_vec, s.edge_diff]
                for where, p in (("base", base), ("new", new)):
                    s.state.zero_()
                    s.verify(p)
                    s.fixed_list(p)
                    arrays[f"{key} verify@{where}"] = [s.row_flag.clone(), s.changed.clone(), s.state.clone()]
                    arrays[f"{key} edge_vectors@{where}"] = [s.fixed_vec.clone(), s.fixed_diff.clone()]
    torch.cuda.synchronize()
    with open(path, "wb") as fh:
        pickle.dump({k: [t.cpu().numpy().tobytes() for t in v] for k, v in arrays.items()}, fh)
    print(f"dumped {len(arrays)} entries of {len(systems())} systems to {path}")


def timing(path, iters, rounds):
    from gotennet_amd import graph
    from tests import pbc_util as U
    s = U.system("c")
    pos, batch, cell = s["pos"].float().cuda(), s["batch"].cuda(), s["cell"].float()
    narrow = torch.tensor([R1_CELL])
    pos_n = U._fill_box(R1_CELL, 70, torch.Generator().manual_seed(5)).float().cuda()
    ranges = graph.image_ranges(narrow, U.CUTOFF)
    assert bool((ranges == 1).all())
    searches = {"open": Search("open", pos, batch, 1, U.CUTOFF, 32),
                "minimum": Search("minimum", pos, batch, 1, U.CUTOFF, 32, cell, None),
                "all_r1": Search("all", pos_n, batch, 1, U.CUTOFF, 32, narrow, ranges)}
    entries = {}
    for name, sr in searches.items():
        entries[name + " count+fill"] = lambda sr=sr: (sr.count(), sr.fill())
        entries[name + " verify"] = sr.verify
    for fn in entries.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    assert all(int(sr.state[0]) == 0 for sr in searches.values())
    times = {k: [] for k in entries}
    for _ in range(rounds):
        for name, fn in entries.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters * 1e3)
    with open(path, "w") as fh:
        json.dump(dict(edges={k: sr.E for k, sr in searches.items()}, iters=iters, us=times), fh)
    for k, v in times.items():
        print(f"{k:22s} {statistics.median(v):8.2f} us  [{min(v):.2f}, {max(v):.2f}]")


def compare(a, b, first, second):
    A, B = (pickle.load(open(f, "rb")) for f in (a, b))
    differ = 0
    print(f"## Same bits: {a} against {b}, byte for byte")
    for key in sorted(set(A) | set(B)):
        same = key in A and key in B and A[key] == B[key]
        differ += not same
        print(("EQUAL   " if same else "DIFFERS ") + key)
    print(f"entries that differ: {differ} of {len(set(A) | set(B))}")
    if first and second:
        runs = [[json.load(open(f)) for f in sorted(glob.glob(pat))] for pat in (first, second)]
        print(f"## Same speed: us per entry, device events over {runs[0][0]['iters']} back-to-back repetitions; processes alternated, "
              f"{len(runs[0])} + {len(runs[1])} processes; edges {runs[0][0]['edges']}")
        for k in runs[0][0]["us"]:
            p, n = [sum((r["us"][k] for r in rs), []) for rs in runs]
            med = statistics.median(n)
            verdict = "within the first library's range" if med <= max(p) else f"OUTSIDE the first library's range (by {med - max(p):.2f} us)"
            print(f"{k:22s} first median {statistics.median(p):7.2f} [{min(p):.2f}, {max(p):.2f}]   second median {med:7.2f} "
                  f"[{min(n):.2f}, {max(n):.2f}]   -> {verdict}")
    return differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", default=None)
    ap.add_argument("--time", default=None)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--times-first", default=None)
    ap.add_argument("--times-second", default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(1 if compare(a.compare[0], a.compare[1], a.times_first, a.times_second) else 0)
    if a.dump:
        dump(a.dump)
    if a.time:
        timing(a.time, a.iters, a.rounds)


if __name__ == "__main__":
    main()
