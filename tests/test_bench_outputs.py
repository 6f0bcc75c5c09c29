"""GPU: the path bench.py times is the correct path.  A plain `bench.py --dump-outputs` run at the headline size
(128 aspirin molecules, `InFlight` with 3 lanes, fresh topology every step, no edge check) dumps the energies and forces of
its last timed step; here they must equal a plain `EnergyForces` on the same model and batch bit for bit, for ALL 128
molecules, match the fp64 oracle per molecule (tests/test_full_size_oracle.py's bounds and selected molecules), and the
other launch modes of the bench (one lane, cached topology, hipGraph replay) must dump the same bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_full_size_oracle import CONFIGS, check_molecules

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 128
MODE = "f16x2"                     # pinned in the bench subprocess and in this process
_RUNS = {}


def _bench(tmp_root, lmax, *extra):
    """`bench.py --steps 2 --warmup 1 --dump-outputs DIR` (one subprocess per distinct command line and test session)
    -> (JSON line, energies [B, 1], forces [N, 3])."""
    key = (lmax,) + extra
    if key not in _RUNS:
        out_dir = os.path.join(str(tmp_root), "lmax%d%s" % (lmax, "".join(extra).replace("-", "_")))
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", str(B),
               "--lmax", str(lmax), "--dump-outputs", out_dir, *extra]
        env = dict(os.environ, GN_GEMM_MODE=MODE)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        e, f = np.load(os.path.join(out_dir, "energy.npy")), np.load(os.path.join(out_dir, "forces.npy"))
        # the dump comes from THIS run: its energies add up to the run's checksum
        assert abs(float(e.astype(np.float64).sum()) - res["energy_checksum"]) <= 1e-9 * max(1.0, abs(res["energy_checksum"]))
        _RUNS[key] = (res, torch.from_numpy(e), torch.from_numpy(f))
    return _RUNS[key]


def _bench_model(lmax):
    """The model bench.py measure() builds, mirrored line for line (on the CPU: the same generator draws)."""
    import gotennet_amd
    from gotennet_amd.outputs import Atomwise
    F, L, R, H = 256, 6, 32, 8
    torch.manual_seed(0)
    rep = gotennet_amd.GotenNet(n_atom_basis=F, n_interactions=L, n_rbf=R, cutoff_fn=gotennet_amd.CosineCutoff(5.0),
                                num_heads=H, scale_edge=False, lmax=lmax, sep_dir=True, sep_tensor=True).eval()
    head = Atomwise(n_in=F, n_hidden=256, derivative="forces", activation="silu").eval()
    return rep, head


@pytest.mark.parametrize("lmax", [2, 4])
def test_bench_dump_is_the_plain_path_and_matches_oracle(lmax, tmp_path_factory):
    from gotennet_amd import engine, synthetic
    from gotennet_amd.graph import distance
    from gotennet_amd.pipeline import EnergyForces
    res, e_b, f_b = _bench(tmp_path_factory.getbasetemp(), lmax)
    assert res["batches_in_flight"] == 3                           # the headline path: three lanes in flight
    pos, batch, z = synthetic.make_batch("rmd17_aspirin", B, seed=0)
    assert e_b.shape == (B, 1) and f_b.shape == (pos.shape[0], 3)
    rep, head = _bench_model(lmax)
    sd, hsd = rep.state_dict(), head.state_dict()
    old, engine.GEMM_MODE = engine.GEMM_MODE, MODE
    try:
        rep_c, head_c = rep.cuda(), head.cuda()
        ei, ed, ev = distance(pos.cuda(), batch.cuda(), 5.0, 32)
        e, f = EnergyForces(rep_c, head_c, cache_topology=False)(z.cuda(), ei, ed, ev, batch.cuda(), B)
        e, f = e.cpu(), f.cpu()
    finally:
        engine.GEMM_MODE = old
    drift = ("the dumped outputs differ from a plain EnergyForces on the model this test mirrors: if bench.py measure() "
             "changed how it builds its model (manual_seed(0) -> GotenNet -> Atomwise), mirror it in _bench_model")
    assert torch.equal(e_b, e), drift + " (energies, %d of %d molecules differ)" % (int((e_b != e).any(1).sum()), B)
    assert torch.equal(f_b, f), drift + " (forces)"
    # per molecule against the fp64 oracle (the bench model: default initialisation, all-zero biases)
    from oracle import gotennet_oracle as orc
    cfg = orc.default_config(n_atom_basis=256, n_interactions=6, n_rbf=32, num_heads=8, scale_edge=False, lmax=lmax,
                             sep_dir=True, sep_tensor=True)
    mols = CONFIGS["c2_lmax2" if lmax == 2 else "c2_lmax4"][1]
    check_molecules(f"bench_lmax{lmax}", MODE, cfg, sd, hsd, pos, batch, z, mols, e=e_b, f=f_b)


@pytest.mark.parametrize("extra", [("--lanes", "1"), ("--static-topology",), ("--replay",)])
def test_bench_launch_modes_dump_the_same_bits(extra, tmp_path_factory):
    """One lane, the cached topology and the hipGraph replay of the static-topology step compute what the headline's three
    lanes on a fresh topology compute: the same bits."""
    base = tmp_path_factory.getbasetemp()
    _, e0, f0 = _bench(base, 2)
    res, e1, f1 = _bench(base, 2, *extra)
    if extra == ("--replay",):
        assert "hipGraph replay" in res["launch_mode"], res["launch_mode"]          # the last step really was a replay
    assert torch.equal(e0, e1), extra
    assert torch.equal(f0, f1), extra
