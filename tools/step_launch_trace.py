"""The launches of every way to run a step, by name and in order, and a hash of what each computes.

``_lib.call`` asks ``_lib.TIMER.want(name, args)`` before every launch; a ``want`` that notes the name and returns None is a launch
trace with no change to the library.  This program uses that hook and the public API only, so it runs unchanged on any commit
that has the step classes and the drivers: a host-side change that must leave every launch where it was is checked by running it
before and after.

Per mode -- ``EnergyForces`` (open, periodic, energy only, across its recording), ``CapturedStep``, ``RebuiltStep``, ``md.MDRun`` and
``Relax`` in every combination of host / device list and captured / eager, the systems and the model of the driver tests (F = 32, two
layers, lmax 2) -- it notes the entry points from construction to the end of the run and a SHA-256 over the final positions,
velocities or forces, energies and stress.  A recorded mode launches while it warms up and records and never again: its replays
are the recorded nodes.  Every mode gets a model of its own, so the weight planes and transposes a pack builds on first use are
part of each trace; one untraced step comes first and fills what the process builds once.

    python tools/step_launch_trace.py --arithmetic f32 --out trace_f32.json         # traces (folded) and hashes
    python tools/step_launch_trace.py --golden tests/golden/step_launches.json       # the traces alone: names only

The hashes belong to one machine, compiler and arithmetic and are compared between two commits there, never stored as a
fixture.  A trace is stored folded (``fold``: immediate repeats of a block written once, with a count); ``unfold`` gives the list
back exactly.
"""
import argparse
import functools
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, FORCE_SCALE, STEPS, NPT_STEPS = 0.2, 0.05, 24, 12          # the set-up of tests/test_hip_md_run.py and test_hip_npt_run.py
THERMOSTAT = dict(kT=0.02, gamma=0.5, key=(77, 5))
TAU = 20 * DT


# ------------------------------------------------------------------------------------------------ folding
def _fold_once(seq, max_period):
    out, i, n = [], 0, len(seq)
    while i < n:
        best = None
        for p in range(1, min(max_period, (n - i) // 2) + 1):
            if seq[i] == seq[i + p] and seq[i:i + p] == seq[i + p:i + 2 * p]:
                reps = 2
                while seq[i + reps * p:i + (reps + 1) * p] == seq[i:i + p]:
                    reps += 1
                best = (p, reps)
                break
        if best is None:
            out.append(seq[i])
            i += 1
        else:
            p, reps = best
            out.append((tuple(seq[i:i + p]), reps))
            i += p * reps
    return out


def fold(names, max_period=600):
    """A list of names -> nested [[block, repeats] | name ...]: the shortest immediate repeat first, then repeats of what that
    left (a layer inside a step, a step inside a run).  Lossless: ``unfold(fold(x)) == x``."""
    seq = list(names)
    while True:
        nxt = _fold_once(seq, max_period)
        if len(nxt) == len(seq):
            break
        seq = nxt

    def plain(item):
        return item if isinstance(item, str) else [[plain(x) for x in item[0]], item[1]]
    return [plain(x) for x in seq]


def unfold(folded):
    out = []
    for item in folded:
        if isinstance(item, str):
            out.append(item)
        else:
            out.extend(unfold(item[0]) * item[1])
    return out


# ------------------------------------------------------------------------------------------------ the hook
class Trace:
    """``_lib.TIMER`` for the length of a ``with``: every launch's name, nothing timed."""

    def __init__(self):
        self.names, self.events = [], []

    def want(self, name, args):
        self.names.append(name)
        return None

    def __enter__(self):
        from gotennet_amd import _lib
        self._old, _lib.TIMER = _lib.TIMER, self
        return self

    def __exit__(self, *exc):
        from gotennet_amd import _lib
        _lib.TIMER = self._old


# ------------------------------------------------------------------------------------------------ systems and model
def _model():
    from tests import pbc_util as U
    net, head, *_ = U.make_model(32, 2, 2, seed=1)
    return net.cuda().eval(), head.cuda().eval()


def _ef(**kw):
    from gotennet_amd.pipeline import EnergyForces
    kw.setdefault("check_edges", False)
    return EnergyForces(*_model(), **kw)


@functools.lru_cache(maxsize=None)
def _system(name):
    """"molecules": ``md_util.md_molecules``; "a": the two wide boxes of ``pbc_util``; "n1": the narrow box of ``pbc_multi_util``.
    -> dict(z, batch, n_mol, pos, vel, cell or None, images, positions: three sets for a bare step), on the device."""
    import torch
    from tests import md_util as MU
    from tests import pbc_multi_util as PM
    from tests import pbc_util as U
    if name == "molecules":
        s = dict(MU.md_molecules(), cell=None, images="minimum")
    else:
        s = dict((PM if name == "n1" else U).system(name), images="all" if name == "n1" else "minimum")
        s["vel"] = 0.05 * torch.randn(s["pos"].shape, generator=torch.Generator().manual_seed(9))
    pos = s["pos"].float()
    moved = pos + 0.05 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(4))
    out = dict(z=s["z"].cuda(), batch=s["batch"].cuda(), n_mol=s["n_mol"], pos=pos.cuda(), vel=s["vel"].float().cuda(),
               cell=None if s["cell"] is None else s["cell"].float().cuda(), images=s["images"])
    out["positions"] = (out["pos"], moved.cuda(), out["pos"])
    return out


def _list(s, pos):
    from gotennet_amd import graph
    from tests import pbc_util as U
    if s["cell"] is None:
        return graph.distance(pos, s["batch"], U.CUTOFF, 32) + (None,)
    return graph.distance_pbc(pos, s["batch"], s["cell"], U.CUTOFF, 32, n_mol=s["n_mol"], images=s["images"])


@functools.lru_cache(maxsize=None)
def _barostat(arithmetic):
    """The coupling of tests/test_hip_npt_run.py on system n1: a deterministic move of at most 1e-3 per step towards P0 = 0 from
    the start pressure, noise of at most 2e-3.  From an eager run without a barostat, outside every trace."""
    from gotennet_amd import _lib
    old, _lib.TIMER = _lib.TIMER, None
    try:
        md = _md_run("n1", captured=False, rebuild="host")
        p, vol = md.pressure.cpu().double(), md.volume.cpu().double()
    finally:
        _lib.TIMER = old
    r = min(1e-3 / float(p.abs().max()), (2e-3) ** 2 * float(vol.min()) / (2 * THERMOSTAT["kT"]))
    return dict(pressure=0.0, tau=TAU, compressibility=r * TAU / DT)


# ------------------------------------------------------------------------------------------------ the modes
def _energy_forces(name, forces=True, calls=5):
    """``replay=True``: calls 1 and 2 are eager, call 3 records, 4 and 5 replay.  A call with ``cell`` never records."""
    s = _system(name)
    ef = _ef(replay=True, replay_after=2)
    ei, ed, ev, _ = _list(s, s["pos"])
    out = None
    for _ in range(calls):
        out = ef(s["z"], ei, ed, ev, s["batch"], s["n_mol"], forces=forces, cell=s["cell"])
    return [t for t in out if t is not None]


def _captured_step(name):
    import torch
    from gotennet_amd.pipeline import CapturedStep
    s = _system(name)
    ei, _, _, sh = _list(s, s["pos"])
    step = CapturedStep(_ef(), s["z"], ei, s["batch"], s["n_mol"], cell=s["cell"], edge_shift=sh, images=s["images"])
    kept = []
    for pos in s["positions"]:
        kept += [t.clone() for t in step(pos)]
    if s["cell"] is not None:
        kept += [t.clone() for t in step(s["positions"][1], cell=s["cell"] * 1.001)]
    return kept


def _rebuilt_step(name, capture, cell_moves=False):
    from gotennet_amd.pipeline import RebuiltStep
    s = _system(name)
    step = RebuiltStep(_ef(), s["z"], s["batch"], s["n_mol"], cell=s["cell"], images=s["images"], capture=capture,
                       cell_moves=cell_moves)
    kept = []
    for k, pos in enumerate(s["positions"]):
        if cell_moves and k == 1:
            step.set_cell(s["cell"] * 1.001)
        kept += [t.clone() for t in step(pos)]
    return kept + [step.edge_count.clone(), step.state.clone()]


def _md_run(name, captured, rebuild, thermostat=None, barostat=None, check_every=8):
    from gotennet_amd.md import MDRun
    s = _system(name)
    return MDRun(_ef(), s["z"], s["pos"], s["batch"], s["n_mol"], dt=DT, force_scale=FORCE_SCALE, vel=s["vel"], cell=s["cell"],
                 images=s["images"], thermostat=thermostat, barostat=barostat, check_every=check_every, log_len=64,
                 captured=captured, rebuild=rebuild)


def _md(name, captured, rebuild, thermostat=False, barostat=False, arithmetic=None):
    baro = _barostat(arithmetic) if barostat else None
    md = _md_run(name, captured, rebuild, THERMOSTAT if thermostat else None, baro, check_every=1 if thermostat else 8)
    md.run(NPT_STEPS if barostat else STEPS)
    out = [md.pos, md.vel, md.potential_energy, md.kinetic_energy, md.energy_log()]
    if _system(name)["cell"] is not None:
        out += [md.stress, md.cell]
    return out + ([md.npt_log()] if barostat else [])


def _relax(name, captured, rebuild):
    from gotennet_amd import Relax
    from tests import fire_util as FU
    s = _system(name)
    rx = Relax(_ef(), s["z"], s["pos"], s["batch"], s["n_mol"], fmax=FU.REF_FMAX, cell=s["cell"], images=s["images"],
               check_every=8, log_len=64, captured=captured, rebuild=rebuild).run(STEPS)
    return [rx.pos, rx.vel, rx.forces, rx.potential_energy, rx.log()] + ([rx.stress] if s["cell"] is not None else [])


def _modes():
    m = {"EnergyForces open replay": lambda a: _energy_forces("molecules"),
         "EnergyForces periodic": lambda a: _energy_forces("a", calls=2),
         "EnergyForces energy only": lambda a: _energy_forces("molecules", forces=False, calls=2),
         "CapturedStep open": lambda a: _captured_step("molecules"),
         "CapturedStep minimum image": lambda a: _captured_step("a"),
         "CapturedStep multi image": lambda a: _captured_step("n1")}
    for cap, how in ((True, "recorded"), (False, "eager")):
        m[f"RebuiltStep open {how}"] = lambda a, cap=cap: _rebuilt_step("molecules", cap)
        m[f"RebuiltStep fixed cell {how}"] = lambda a, cap=cap: _rebuilt_step("a", cap)
        m[f"RebuiltStep cell moves {how}"] = lambda a, cap=cap: _rebuilt_step("n1", cap, cell_moves=True)
    for rebuild in ("host", "device"):
        for cap, how in ((True, "captured"), (False, "eager")):
            for th, ens in ((False, "NVE"), (True, "thermostat")):
                m[f"MDRun {rebuild} {how} {ens}"] = lambda a, r=rebuild, c=cap, t=th: _md("molecules", c, r, t)
            # with a barostat: the narrow box, multi-image lists (device mode refuses "minimum")
            m[f"MDRun {rebuild} {how} barostat"] = lambda a, r=rebuild, c=cap: _md("n1", c, r, True, True, a)
        m[f"MDRun {rebuild} captured periodic"] = lambda a, r=rebuild: _md("a", True, r)
    for rebuild, cap, how in (("host", True, "host captured"), ("host", False, "host eager"), ("device", True, "device captured")):
        m[f"Relax {how}"] = lambda a, r=rebuild, c=cap: _relax("molecules", c, r)
    m["Relax host captured periodic"] = lambda a: _relax("a", True, "host")
    return m


MODES = _modes()


def prepare(arithmetic=None):
    """Set the projection arithmetic (None: leave it) and run one untraced eager step: what the process builds once, whatever
    the model, is built here and is in no trace.  -> the arithmetic in use."""
    from gotennet_amd import engine
    if arithmetic is not None:
        engine.GEMM_MODE = arithmetic
    _energy_forces("molecules", calls=1)
    _energy_forces("a", calls=1)
    return engine.GEMM_MODE


def run_mode(name, arithmetic):
    """-> (the launches of mode ``name`` in order, SHA-256 of its results).  ``prepare`` comes first, once per process."""
    import torch
    with Trace() as tr:
        out = MODES[name](arithmetic)
        torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in out:
        t = t.detach().cpu().contiguous()
        h.update(str((t.dtype, tuple(t.shape))).encode())
        h.update(t.numpy().tobytes())
    return tr.names, h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arithmetic", default=None, help='engine.GEMM_MODE: "f32", "f16x2", ... (default: the package\'s)')
    ap.add_argument("--modes", nargs="*", default=None, help="run these modes only, in this order")
    ap.add_argument("--out", default=None, help="write traces (folded) and hashes here")
    ap.add_argument("--golden", default=None, help="write the traces alone here (names only: a fixture)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("step_launch_trace needs a ROCm device: launches are traced, never predicted")
    arithmetic = prepare(a.arithmetic)
    traces, hashes = {}, {}
    for name in (a.modes if a.modes else MODES):
        names, digest = run_mode(name, arithmetic)
        traces[name], hashes[name] = fold(names), digest
        assert unfold(traces[name]) == names
        print(f"{arithmetic:<6} {name:<36} {len(names):6d} launches  sha256 {digest}", flush=True)
    for path, doc in ((a.out, dict(arithmetic=arithmetic, launches=traces, sha256=hashes)),
                      (a.golden, dict(arithmetic=arithmetic, launches=traces))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(doc, fh, separators=(",", ":"))
                fh.write("\n")


if __name__ == "__main__":
    main()
