"""Steps per second of the drivers with the neighbour list rebuilt on the device (``rebuild="device"``) against the two modes
that were there before -- orientation, not a gate.  Two cases, the settings of profiles/md_driver.txt and profiles/relax.txt:

  md     md.MDRun on one aspirin-sized molecule (21 atoms), the benchmark's model (n_atom_basis 256, 6 interactions, lmax 2,
         cutoff 5, 32 neighbours), NVE from seeded Maxwell-Boltzmann velocities (kT = 0.0259, dt = 0.5), ``--steps`` steps after
         ``--warmup``
  relax  gotennet_amd.Relax on the 70-atom periodic box of tests/pbc_util.py (system c), the same model, fmax 0, ``--relax-steps``
         steps from the start

and three modes:

  eager   captured=False, rebuild="host": the kernels launched eagerly, the list rebuilt by graph.distance* in every step
  host    captured=True,  rebuild="host": one hipGraph replay per step on a fixed list that is verified on the device; a stale
          list is rebuilt by the host and a new graph recorded (the baseline: the code as it was)
  device  captured=True,  rebuild="device": one hipGraph replay per step, the list rebuilt inside it (pipeline.RebuiltStep)

Every (case, mode) measurement runs in its OWN fresh process (``--mode`` given: measure and print one JSON line), so one graph is
alive at a time; the driver synchronises after the first replay of a recorded graph.  Without ``--mode`` this program only starts
those processes one after the other, in alternating rounds, stops at the first that fails, and writes the medians to
``profiles/md_rebuild.txt`` with the padding overhead of the device mode (capacity / E_real and n_pad / N) next to them.  The
clock is a host clock around the steps, which end in a device synchronise; construction is not timed.

    python tools/md_rebuild_time.py --rounds 3
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUTOFF, MAX_NBR, DT, KT = 5.0, 32, 0.5, 0.0259
MODES = {"eager": dict(captured=False, rebuild="host"), "host": dict(captured=True, rebuild="host"),
         "device": dict(captured=True, rebuild="device")}
CASES = ("md", "relax")


def measure(a):
    """One (case, mode) in this process -> one JSON line."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("md_rebuild_time needs a ROCm device: times are measured, never estimated")
    import gotennet_amd
    from gotennet_amd import graph, md, synthetic
    from gotennet_amd.outputs import Atomwise
    from gotennet_amd.pipeline import EnergyForces
    torch.manual_seed(0)
    rep = gotennet_amd.GotenNet(n_atom_basis=256, n_interactions=6, n_rbf=32, cutoff_fn=gotennet_amd.CosineCutoff(CUTOFF),
                                num_heads=8, scale_edge=False, lmax=2, sep_dir=True, sep_tensor=True).cuda().eval()
    head = Atomwise(n_in=256, n_hidden=256, derivative="forces", activation="silu").cuda().eval()
    ef = EnergyForces(rep, head, check_edges=False)
    kw = dict(MODES[a.mode], max_num_neighbors=MAX_NBR, check_every=a.check_every)
    if a.case == "md":
        pos, batch, z = (t.cuda() for t in synthetic.make_batch("rmd17_aspirin", 1, seed=0))
        fs = md.EV_ANGSTROM_AMU_FS
        mass = md.default_masses().cuda()[z.long()].unsqueeze(1)
        vel = (torch.randn(pos.shape, generator=torch.Generator().manual_seed(1)).cuda() * (KT * fs / mass).sqrt()).float()
        drv = md.MDRun(ef, z, pos, batch, 1, dt=DT, force_scale=fs, vel=vel, log_len=a.steps + a.warmup, **kw)
        n_mol, steps, warmup = 1, a.steps, a.warmup
    else:
        from tests import pbc_util
        s = pbc_util.system("c")
        z, batch, n_mol = s["z"].cuda(), s["batch"].cuda(), s["n_mol"]
        drv = gotennet_amd.Relax(ef, z, s["pos"].float().cuda(), batch, n_mol, fmax=0.0, cell=s["cell"].float().cuda(),
                                 images="minimum", **kw)
        steps, warmup = a.relax_steps, 0
    torch.cuda.synchronize()
    if warmup:
        drv.run(warmup)
        torch.cuda.synchronize()
    edges = [drv.edge_count]
    t0 = time.perf_counter()
    drv.run(steps)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert drv.step == steps + warmup
    edges.append(drv.edge_count)
    lay = graph.PaddedLayout(batch.cpu(), n_mol, MAX_NBR)              # (host arithmetic: the sizes the device mode allocates)
    print(json.dumps(dict(tool="tools/md_rebuild_time.py", case=a.case, mode=a.mode, device=torch.cuda.get_device_name(0),
                          atoms=lay.N, steps=steps, warmup=warmup, check_every=a.check_every, seconds=round(wall, 4),
                          steps_per_second=round(steps / wall, 1), ms_per_step=round(wall / steps * 1e3, 4), rebuilds=drv.rebuilds,
                          edges_before=edges[0], edges_after=edges[1], capacity=lay.edge_capacity, n_pad=lay.n_pad)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=tuple(MODES), help="measure this mode in this process (default: run them all, one process each)")
    ap.add_argument("--case", choices=CASES, default="md")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--relax-steps", type=int, default=60)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md_rebuild.txt"))
    a = ap.parse_args()
    if a.mode is not None:
        return measure(a)
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--relax-steps", str(a.relax_steps), "--check-every",
              str(a.check_every)]
    recs = {(c, m): [] for c in CASES for m in MODES}
    for c in CASES:
        for _ in range(a.rounds):
            for m in MODES:                              # alternating: a drift of the machine hits every mode alike
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", c, "--mode", m] + common,
                                     capture_output=True, text=True, timeout=600, cwd=ROOT)
                lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
                if out.returncode != 0 or len(lines) != 1:
                    sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                    raise SystemExit(f"{c} / {m} ended with status {out.returncode}: nothing more is started")
                recs[(c, m)].append(json.loads(lines[0]))
                print(lines[0], flush=True)
    first = recs[(CASES[0], "eager")][0]
    text = [f"# tools/md_rebuild_time.py on {first['device']}: F=256 L=6 lmax=2 cutoff={CUTOFF:g} cap={MAX_NBR}, f16x2 projections (the default).",
            f"# md: md.MDRun, one 21-atom molecule, NVE, dt {DT}, {a.steps} steps after {a.warmup}; relax: gotennet_amd.Relax, system c of",
            f"# tests/pbc_util.py (70 atoms, periodic), fmax 0, {a.relax_steps} steps from the start.  check_every {a.check_every}.  Every measurement in a",
            f"# fresh process; steps/s as median [min, max] of {a.rounds} alternating rounds; a host clock around the steps, ending in a device",
            "# synchronise; construction is not timed.  eager / host: rebuild=\"host\" (the code as it was, the baseline); device:",
            "# rebuild=\"device\", captured.  Padding of the device mode: capacity / E_real and n_pad / N.  Orientation, not a gate.",
            "case   mode     steps/s                       ms/step   rebuilds   E_real (before -> after)   capacity   capacity/E_real   n_pad/N"]
    for c in CASES:
        for m in MODES:
            r = recs[(c, m)]
            rate = [x["steps_per_second"] for x in r]
            med, last = statistics.median(rate), r[-1]
            text.append(f"{c:<6} {m:<8} {med:7.1f}  [{min(rate):.1f}, {max(rate):.1f}]".ljust(46) + f" {1e3 / med:7.3f}   {last['rebuilds']:<8}"
                        f"   {last['edges_before']} -> {last['edges_after']}".ljust(40)
                        + f"   {last['capacity']:<8}   {last['capacity'] / last['edges_after']:.3f}             "
                          f"{last['n_pad']} / {last['atoms']} = {last['n_pad'] / last['atoms']:.3f}")
    text = "\n".join(text) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
