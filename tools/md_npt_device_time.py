"""Step time of the constant-pressure MD driver with the list rebuilt on the device against the captured ``rebuild="host"``
driver -- orientation, not a gate.  The sibling of tools/md_npt_time.py: the same 70-atom periodic box (tests/pbc_util.py
system c), the same model (n_atom_basis 256, 6 interactions, lmax 2, cutoff 5, 32 neighbours), thermostat, barostat (target =
the start pressure, tau = 500 dt, water's compressibility) and ``images="auto"``, in its two cases:

    cold     kT 2.59e-5, dt 0.01   the list changes once in hundreds of steps without a barostat
    thermal  kT 0.0259,  dt 0.5    eV / Angstrom / amu / fs: the list changes in nearly every step

Every measurement is a FRESH process with one driver, so one recorded graph, alive: it builds the model, runs ``--warmup``
steps, then times ``--steps`` steps with a host clock around a run that ends in a device synchronise, and prints one JSON
line.  The parent (which never touches the device) starts them one after the other, alternating host and device mode within
each of ``--rounds`` rounds, and prints every child's line and a closing summary line.  All rounds of a mode start from the
same state and so time the same steps.

    python tools/md_npt_device_time.py --steps 200 --rounds 5
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

CUTOFF, MAX_NBR = 5.0, 32
CASES = {"cold": dict(kT=2.59e-5, dt=0.01), "thermal": dict(kT=0.0259, dt=0.5)}


def child(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("md_npt_device_time needs a ROCm device: times are measured, never estimated")
    import gotennet_amd
    from gotennet_amd import md
    from gotennet_amd.outputs import Atomwise
    from gotennet_amd.pipeline import EnergyForces
    from tests import pbc_util
    DT, KT = CASES[a.case]["dt"], CASES[a.case]["kT"]
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
    ef = EnergyForces(rep, head, check_edges=False)
    kw = dict(dt=DT, force_scale=fs, vel=vel, cell=cell, images="auto", max_num_neighbors=MAX_NBR, thermostat=thermostat,
              check_every=a.check_every)
    # the target: the start pressure, from an eager evaluation that records nothing (dropped before the timed driver is built)
    probe = md.MDRun(ef, z, pos, batch, 1, captured=False, **kw)
    p_start = float(probe.pressure[0])
    del probe
    run = md.MDRun(ef, z, pos, batch, 1, rebuild=a.mode, **kw,
                   barostat=dict(pressure=p_start, tau=500 * DT, compressibility=4.5e-5 / md.BAR_EV_ANGSTROM3))
    run.run(a.warmup)
    torch.cuda.synchronize()
    r0 = run.rebuilds
    t0 = time.perf_counter()
    run.run(a.steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    rec = dict(tool="tools/md_npt_device_time.py", device=torch.cuda.get_device_name(0), case=a.case, mode=a.mode, dt=DT, kT=KT,
               atoms=pos.shape[0], steps=a.steps, warmup=a.warmup, check_every=a.check_every, ms_per_step=ms,
               rebuilds=run.rebuilds - r0, edges_end=run.edge_count, volume_end=float(run.volume[0]),
               pressure_end_bar=float(run.pressure[0]) / md.BAR_EV_ANGSTROM3, start_pressure_bar=p_start / md.BAR_EV_ANGSTROM3)
    if a.mode == "device":
        lay = run._step.layout
        rec.update(capacity=lay.edge_capacity, capacity_over_e_real=lay.edge_capacity / run.edge_count, n_pad=lay.n_pad,
                   n_pad_over_n=lay.n_pad / lay.N, image_ranges_end=run._step._ranges.tolist())
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--cases", nargs="+", choices=list(CASES), default=list(CASES))
    ap.add_argument("--child-timeout", type=float, default=240.0, help="seconds a measurement may take")
    ap.add_argument("--case", choices=list(CASES), help="(a measurement process: its case)")
    ap.add_argument("--mode", choices=["host", "device"], help="(a measurement process: its mode)")
    a = ap.parse_args()
    if a.mode is not None:
        return child(a)
    times = {}
    for case in a.cases:
        for _ in range(a.rounds):
            for mode in ("host", "device"):
                cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--mode", mode, "--steps", str(a.steps),
                       "--warmup", str(a.warmup), "--check-every", str(a.check_every)]
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout, cwd=ROOT)
                if out.returncode != 0:                       # nothing more is started on the device after a failure
                    sys.stderr.write(out.stdout + out.stderr)
                    raise SystemExit(f"{case} / {mode}: the measurement process ended with status {out.returncode}")
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
                print(line, flush=True)
                times.setdefault((case, mode), []).append(json.loads(line)["ms_per_step"])
    summary = {f"{case}/{mode}": dict(ms_per_step_median=statistics.median(t), ms_per_step_min=min(t), ms_per_step_max=max(t))
               for (case, mode), t in times.items()}
    print(json.dumps(dict(tool="tools/md_npt_device_time.py", summary=summary)))


if __name__ == "__main__":
    main()
