"""Steps per second of the nudged-elastic-band driver (``gotennet_amd.NEB``) in its three modes -- orientation, not a gate.

The case: ``--bands`` bands of ``--images`` images of one aspirin-sized molecule (21 atoms) between the synthetic geometry and a
copy displaced by a seeded 0.15 Angstrom of noise, the benchmark's model (n_atom_basis 256, 6 interactions, lmax 2, cutoff 5,
32 neighbours), k = 0.1, a climbing image, fmax 0 (no band converges), ``--steps`` steps after ``--warmup``.  The modes:

  eager   captured=False, rebuild="host": the kernels launched eagerly, the list rebuilt by graph.distance in every step
  host    captured=True,  rebuild="host": one hipGraph replay per step on a fixed list that is verified on the device
  device  captured=True,  rebuild="device": one hipGraph replay per step, the list rebuilt inside it

Every measurement runs in its OWN fresh process (``--mode`` given: measure and print one JSON line), so one graph is alive at a
time.  Without ``--mode`` this program only starts those processes one after the other, in alternating rounds, stops at the
first that fails, and writes the medians to ``--out`` (default ``profiles/neb.txt``).  The clock is a host clock around the steps,
which end in a device synchronise; construction is not timed.

    python tools/neb_time.py --rounds 3
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

CUTOFF, MAX_NBR, K = 5.0, 32, 0.1
MODES = {"eager": dict(captured=False, rebuild="host"), "host": dict(captured=True, rebuild="host"),
         "device": dict(captured=True, rebuild="device")}


def measure(a):
    """One mode in this process -> one JSON line."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("neb_time needs a ROCm device: times are measured, never estimated")
    import gotennet_amd
    from gotennet_amd import neb, synthetic
    from gotennet_amd.outputs import Atomwise
    from gotennet_amd.pipeline import EnergyForces
    torch.manual_seed(0)
    rep = gotennet_amd.GotenNet(n_atom_basis=256, n_interactions=6, n_rbf=32, cutoff_fn=gotennet_amd.CosineCutoff(CUTOFF),
                                num_heads=8, scale_edge=False, lmax=2, sep_dir=True, sep_tensor=True).cuda().eval()
    head = Atomwise(n_in=256, n_hidden=256, derivative="forces", activation="silu").cuda().eval()
    first, batch, z = synthetic.make_batch("rmd17_aspirin", a.bands, seed=0)
    last = first + 0.15 * torch.randn(first.shape, generator=torch.Generator().manual_seed(1))
    z, pos, batch, n_mol = neb.band(z, first, last, batch, a.bands, n_images=a.images)
    drv = neb.NEB(EnergyForces(rep, head, check_edges=False), z.cuda(), pos.cuda(), batch.cuda(), n_mol, n_images=a.images, k=K,
                  climb=True, fmax=0.0, max_num_neighbors=MAX_NBR, check_every=a.check_every, log_len=a.steps + a.warmup,
                  **MODES[a.mode])
    torch.cuda.synchronize()
    drv.run(a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    drv.run(a.steps)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert drv.step == a.steps + a.warmup
    print(json.dumps(dict(tool="tools/neb_time.py", mode=a.mode, device=torch.cuda.get_device_name(0), bands=a.bands,
                          images=a.images, atoms=int(pos.shape[0]), steps=a.steps, warmup=a.warmup, check_every=a.check_every,
                          seconds=round(wall, 4), steps_per_second=round(a.steps / wall, 1),
                          ms_per_step=round(wall / a.steps * 1e3, 4), rebuilds=drv.rebuilds, edges=drv.edge_count,
                          barrier=[round(x, 6) for x in drv.barrier.tolist()], fmax=[round(x, 6) for x in drv.fmax.tolist()])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=tuple(MODES), help="measure this mode in this process (default: run them all, one process each)")
    ap.add_argument("--bands", type=int, default=4)
    ap.add_argument("--images", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neb.txt"))
    a = ap.parse_args()
    if a.mode is not None:
        return measure(a)
    common = ["--bands", str(a.bands), "--images", str(a.images), "--steps", str(a.steps), "--warmup", str(a.warmup),
              "--check-every", str(a.check_every)]
    recs = {m: [] for m in MODES}
    for _ in range(a.rounds):
        for m in MODES:                                  # alternating: a drift of the machine hits every mode alike
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", m] + common, capture_output=True, text=True,
                                 timeout=600, cwd=ROOT)
            lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
            if out.returncode != 0 or len(lines) != 1:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                raise SystemExit(f"{m} ended with status {out.returncode}: nothing more is started")
            recs[m].append(json.loads(lines[0]))
            print(lines[0], flush=True)
    first = recs["eager"][0]
    text = [f"# tools/neb_time.py on {first['device']}: F=256 L=6 lmax=2 cutoff={CUTOFF:g} cap={MAX_NBR}, f16x2 projections (the default).",
            f"# gotennet_amd.NEB: {a.bands} bands x {a.images} images x 21 atoms = {first['atoms']} atoms, k {K}, climbing image, fmax 0,",
            f"# {a.steps} steps after {a.warmup}; check_every {a.check_every}.  Every measurement in a fresh process; steps/s as median [min, max] of",
            f"# {a.rounds} alternating rounds; a host clock around the steps, ending in a device synchronise; construction is not timed.",
            "# Orientation, not a gate.",
            "mode     steps/s                       ms/step   rebuilds   edges"]
    for m in MODES:
        rate = [x["steps_per_second"] for x in recs[m]]
        med, last = statistics.median(rate), recs[m][-1]
        text.append(f"{m:<8} {med:7.1f}  [{min(rate):.1f}, {max(rate):.1f}]".ljust(39) + f" {1e3 / med:7.3f}   {last['rebuilds']:<8}   {last['edges']}")
    text = "\n".join(text) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
