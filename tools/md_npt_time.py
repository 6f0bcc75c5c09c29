"""Step time of the captured MD driver at constant volume against constant pressure -- orientation, not a gate.

One periodic box (tests/pbc_util.py system c: 70 atoms, cubic, 10.5 wide), the benchmark's model (n_atom_basis 256, 6
interactions, lmax 2, cutoff 5, 32 neighbours), Langevin thermostat in both runs; the second adds the barostat (target = its own
start pressure; images="auto").  Both drivers live in ONE process and are timed in alternating rounds: a host clock around
``--steps`` steps that end in a device synchronise, after ``--warmup`` steps each.  Prints one JSON line.

The defaults are a COLD, slow run (kT 2.59e-5, dt 0.01): atoms move about 1e-6 of a length unit per step, the list of this
random 70-atom box then changes once in hundreds of steps, and the figure is the replayed step itself.  ``--kT 0.0259 --dt 0.5``
is a thermal run in eV / Angstrom / amu / fs units: there this box changes its list in nearly every step and both figures are
the cost of a rebuild.

    python tools/md_npt_time.py --steps 200 --rounds 5
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CUTOFF, MAX_NBR = 5.0, 32


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--kT", type=float, default=2.59e-5)
    a = ap.parse_args()
    DT, KT = a.dt, a.kT
    if not torch.cuda.is_available():
        raise SystemExit("md_npt_time needs a ROCm device: times are measured, never estimated")
    import gotennet_amd
    from gotennet_amd import md
    from gotennet_amd.outputs import Atomwise
    from gotennet_amd.pipeline import EnergyForces
    from tests import pbc_util
    torch.manual_seed(0)
    rep = gotennet_amd.GotenNet(n_atom_basis=256, n_interactions=6, n_rbf=32, cutoff_fn=gotennet_amd.CosineCutoff(CUTOFF),
                                num_heads=8, scale_edge=False, lmax=2, sep_dir=True, sep_tensor=True).cuda().eval()
    head = Atomwise(n_in=256, n_hidden=256, derivative="forces", activation="silu").cuda().eval()
    s = pbc_util.system("c")
    pos, batch, z, cell = s["pos"].float().cuda(), s["batch"].cuda(), s["z"].cuda(), s["cell"].float().cuda()
    fs = md.EV_ANGSTROM_AMU_FS
    mass = md.default_masses().cuda()[z.long()].unsqueeze(1)
    g = torch.Generator().manual_seed(1)
    vel = (torch.randn(pos.shape, generator=g).cuda() * (KT * fs / mass).sqrt()).float()
    thermostat = dict(kT=KT, gamma=0.01, key=(2024, 7))

    def driver(barostat):
        return md.MDRun(EnergyForces(rep, head, check_edges=False), z, pos, batch, 1, dt=DT, force_scale=fs, vel=vel, cell=cell,
                        images="auto", max_num_neighbors=MAX_NBR, thermostat=thermostat, check_every=a.check_every,
                        barostat=barostat)

    nvt = driver(None)
    p_start = float(nvt.pressure[0])
    # water's compressibility (4.5e-5 / bar) and a relaxation time of 500 steps
    npt = driver(dict(pressure=p_start, tau=500 * DT, compressibility=4.5e-5 / md.BAR_EV_ANGSTROM3))
    runs = {"nvt": nvt, "npt": npt}
    for d in runs.values():
        d.run(a.warmup)
    torch.cuda.synchronize()
    times, rebuilds = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, d in runs.items():
            r0 = d.rebuilds
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.run(a.steps)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / a.steps * 1e3)
            rebuilds[k].append(d.rebuilds - r0)
    rec = dict(tool="tools/md_npt_time.py", device=torch.cuda.get_device_name(0), atoms=pos.shape[0], system="pbc_util c",
               model="F=256 L=6 lmax=2 cutoff=5 max_nbr=32", dt=DT, kT=KT, steps=a.steps, warmup=a.warmup, rounds=a.rounds,
               check_every=a.check_every, start_pressure_bar=p_start / md.BAR_EV_ANGSTROM3,
               volume_start=float(nvt.volume[0]), volume_end_npt=float(npt.volume[0]),
               pressure_end_npt_bar=float(npt.pressure[0]) / md.BAR_EV_ANGSTROM3)
    for k in runs:
        rec[k] = dict(ms_per_step_median=statistics.median(times[k]), ms_per_step_min=min(times[k]), ms_per_step_max=max(times[k]),
                      rebuilds_per_round=rebuilds[k])
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
