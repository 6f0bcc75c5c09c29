"""Steps per second of the relaxation driver, captured against eager -- orientation, not a claim.

Two cases, each with both modes of ``gotennet_amd.Relax`` alive in ONE process and timed in alternating rounds (a host clock
around ``--steps`` steps that end in a device synchronise, every round from the same start with freshly built drivers, whose
construction is not timed):

  * the three molecules of the driver tests (tests/md_util.md_molecules(): 3, 4 and 5 atoms) with the tests' model (n_atom_basis
    32, 2 interactions, lmax 2);
  * one periodic box (tests/pbc_util.py system c: 70 atoms, cubic, 10.5 wide) with the benchmark's model (n_atom_basis 256, 6
    interactions, lmax 2).

``fmax`` is 0, so no molecule converges and every run takes exactly ``--steps`` steps; everything else is the default.  The list
of a structure that is being relaxed changes every few steps at first, and each change costs the captured mode a new recording:
no speed-up is promised, and the rebuild counts are printed next to the times.  Writes ``profiles/relax.txt``.

    python tools/relax_time.py --steps 60 --rounds 3
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUTOFF, MAX_NBR = 5.0, 32


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relax.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("relax_time needs a ROCm device: times are measured, never estimated")
    import gotennet_amd
    from gotennet_amd.outputs import Atomwise
    from gotennet_amd.pipeline import EnergyForces
    from tests import md_util, pbc_util

    def model(F, L, n_rbf, hidden):
        torch.manual_seed(0)
        rep = gotennet_amd.GotenNet(n_atom_basis=F, n_interactions=L, n_rbf=n_rbf, cutoff_fn=gotennet_amd.CosineCutoff(CUTOFF),
                                    num_heads=8, scale_edge=False, lmax=2, sep_dir=True, sep_tensor=True).cuda().eval()
        return EnergyForces(rep, Atomwise(n_in=F, n_hidden=hidden, derivative="forces", activation="silu").cuda().eval(),
                            check_edges=False)

    mols, box = md_util.md_molecules(), pbc_util.system("c")
    cases = [("3 molecules (3, 4, 5 atoms), F=32 L=2", model(32, 2, 16, 32), mols, {}),
             ("pbc_util system c (70 atoms), F=256 L=6", model(256, 6, 32, 256), box,
              dict(cell=box["cell"].float().cuda(), images="minimum"))]
    lines = [f"# tools/relax_time.py on {torch.cuda.get_device_name(0)}: gotennet_amd.Relax, fmax 0 (nobody converges), defaults otherwise;",
             f"# lmax 2, cutoff {CUTOFF:g}, cap {MAX_NBR}, f16x2 projections (the default).  Host clock around {a.steps} steps from the start, ending in a",
             f"# device synchronise; both modes in one process, steps/s as median [min, max] of {a.rounds} alternating rounds; construction",
             "# (the first list, the first recording) is not timed.  Orientation, not a claim: no gate, no speed-up promised.",
             "case                                        mode                       steps/s                    ms/step   rebuilds"]
    for name, ef, s, kw in cases:
        args = (ef, s["z"].cuda(), s["pos"].float().cuda(), s["batch"].cuda(), s["n_mol"])
        modes = {f"captured, check_every={a.check_every}": dict(captured=True, check_every=a.check_every),
                 "captured, check_every=1": dict(captured=True, check_every=1), "eager": dict(captured=False)}
        rate, rebuilds = {k: [] for k in modes}, {}
        for _ in range(a.rounds):
            for k, m in modes.items():
                rx = gotennet_amd.Relax(*args, fmax=0.0, max_num_neighbors=MAX_NBR, **kw, **m)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rx.run(a.steps)
                torch.cuda.synchronize()
                rate[k].append(a.steps / (time.perf_counter() - t0))
                assert rx.step == a.steps
                rebuilds[k] = rx.rebuilds
                del rx
        for k in modes:
            med = statistics.median(rate[k])
            lines.append(f"{name:<43} {k:<26} {med:7.1f}  [{min(rate[k]):.1f}, {max(rate[k]):.1f}]".ljust(98)
                         + f" {1e3 / med:7.3f}   {rebuilds[k]}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
