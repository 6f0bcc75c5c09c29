"""Steps per second of the MD driver on one aspirin-sized molecule (21 atoms), the benchmark's model (n_atom_basis 256, 6
interactions, lmax 2, cutoff 5, 32 neighbours) -- orientation, not a gate.  One mode per invocation, in a fresh process:

  captured      md.MDRun(captured=True): one hipGraph replay per step, the list verified on the device, rebuilt when stale
  eager         md.MDRun(captured=False): the same kernels launched eagerly, the list rebuilt by graph.distance in every step
  replay_torch  a bare pipeline.CapturedStep replay on the INITIAL list plus a velocity-Verlet integrator written in torch ops:
                what a user had before the driver (no list check: not the same trajectory once the list changes)

NVE from seeded Maxwell-Boltzmann velocities (kT = 0.0259, eV / Angstrom / amu / fs units, dt = 0.5).  The clock is a host
clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps; the first replay of every recorded
graph is followed by a synchronise (the driver does that itself).  Prints one JSON line.

    python tools/md_driver_time.py --mode captured --steps 300
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CUTOFF, MAX_NBR, DT, KT = 5.0, 32, 0.5, 0.0259


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("captured", "eager", "replay_torch"), required=True)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--check-every", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("md_driver_time needs a ROCm device: times are measured, never estimated")
    import gotennet_amd
    from gotennet_amd import graph, md, synthetic
    from gotennet_amd.outputs import Atomwise
    from gotennet_amd.pipeline import CapturedStep, EnergyForces
    torch.manual_seed(0)
    rep = gotennet_amd.GotenNet(n_atom_basis=256, n_interactions=6, n_rbf=32, cutoff_fn=gotennet_amd.CosineCutoff(CUTOFF),
                                num_heads=8, scale_edge=False, lmax=2, sep_dir=True, sep_tensor=True).cuda().eval()
    head = Atomwise(n_in=256, n_hidden=256, derivative="forces", activation="silu").cuda().eval()
    pos, batch, z = (t.cuda() for t in synthetic.make_batch("rmd17_aspirin", 1, seed=0))
    fs = md.EV_ANGSTROM_AMU_FS
    mass = md.default_masses().cuda()[z.long()].unsqueeze(1)
    g = torch.Generator().manual_seed(1)
    vel = (torch.randn(pos.shape, generator=g).cuda() * (KT * fs / mass).sqrt()).float()
    ef = EnergyForces(rep, head, check_edges=False)
    rec = dict(tool="tools/md_driver_time.py", mode=a.mode, device=torch.cuda.get_device_name(0), atoms=pos.shape[0],
               model="F=256 L=6 lmax=2 cutoff=5 max_nbr=32", dt=DT, steps=a.steps, warmup=a.warmup)
    if a.mode == "replay_torch":
        ei = graph.distance(pos, batch, CUTOFF, MAX_NBR)[0]
        step = CapturedStep(ef, z, ei, batch, 1)
        torch.cuda.synchronize()
        x, v = pos.clone(), vel.clone()
        f = step(x)[1].clone()
        torch.cuda.synchronize()                     # after the first replay
        s = 0.5 * DT * fs

        def run(n):
            nonlocal f
            for _ in range(n):
                v.add_(f / mass, alpha=s)
                x.add_(v, alpha=DT)
                f = step(x)[1]
                v.add_(f / mass, alpha=s)
            torch.cuda.synchronize()
        rec.update(edges=ei.shape[1], rebuilds=None)
    else:
        drv = md.MDRun(ef, z, pos, batch, 1, dt=DT, force_scale=fs, vel=vel, max_num_neighbors=MAX_NBR, check_every=a.check_every,
                       log_len=a.steps + a.warmup, captured=a.mode == "captured")
        rec.update(check_every=a.check_every if a.mode == "captured" else None)

        def run(n):
            drv.run(n)
            torch.cuda.synchronize()
    run(a.warmup)
    t0 = time.perf_counter()
    run(a.steps)
    wall = time.perf_counter() - t0
    rec.update(seconds=round(wall, 4), steps_per_second=round(a.steps / wall, 1), ms_per_step=round(wall / a.steps * 1e3, 4))
    if a.mode != "replay_torch":
        total = drv.energy_log().double().sum(2).flatten()
        rec.update(rebuilds=drv.rebuilds, total_energy_first=float(total[0]), total_energy_last=float(total[-1]),
                   total_energy_excursion=float(total.max() - total.min()))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
