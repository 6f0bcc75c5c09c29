#!/usr/bin/env python
"""Time one first-order training step (``parameter_grads``): the saving forward, the backward with parameter gradients
and torch.optim.Adam.step, with HIP events, on two shapes:

  qm9  -- the QM9 recipe's model (F=256, L=4, n_rbf=64, lmax=2), 32 QM9-sized synthetic molecules, energy loss;
  c2   -- rMD17 aspirin, 128 molecules, F=256, L=6 (BASELINE configs[1]).

Prints ms per step, molecules per second, the time spent in the weight-gradient calls (gn_weight_grad_group: a partial
and a reduction kernel per 8 problems) and their FLOP rate, and -- on its own, back to back -- the largest problem, dWe =
g_eproj^T t ([(1+M)F x F] over the E edge rows), against the fp32 MFMA peak.  ``--json PATH`` also writes the record.

    python tools/train_step_time.py --steps 20 --warmup 5 --json profiles/train_step_time.json

``--attn-dropout P[,P...]`` times every shape once per attention-dropout probability (the modules are in train() mode, so
P > 0 runs the dropout kernels: one more [E,H] write per layer forward, one more [E,H] read per layer backward, one key
launch per call), same weights and inputs:

    python tools/train_step_time.py --shapes c2 --attn-dropout 0,0.1 --json profiles/train_step_dropout.json

``--wgrad-mode M[,M...]`` times every shape once per listed weight-gradient arithmetic (``wgrad_mode`` of the model and the
head: f32 | f16x2), in the order given -- list the modes alternately (f32,f16x2,f32,f16x2) and the f32 rows are the
yardstick of the same run.  ``dwe_alone`` is measured in the row's mode and carries the bytes its tiling fetches per launch:

    python tools/train_step_time.py --wgrad-mode f32,f16x2,f32,f16x2 --json profiles/train_step_wgrad_modes.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = {
    "qm9": dict(model=dict(n_atom_basis=256, n_interactions=4, n_rbf=64, lmax=2), workload="qm9_small", n_mol=32),
    "c2": dict(model=dict(n_atom_basis=256, n_interactions=6, n_rbf=32, lmax=2), workload="rmd17_aspirin", n_mol=128),
}


FP32_MFMA_PEAK_TFLOPS = 157.3


class _WgradTimer:
    """``_lib.TIMER``: brackets every gn_weight_grad_group / gn_weight_grad_group_mode call with HIP events and counts
    its FLOPs and kernels."""

    def __init__(self):
        self.events, self.flops, self.kernels = [], 0.0, 0

    def want(self, name, args):
        if name not in ("gn_weight_grad_group", "gn_weight_grad_group_mode"):
            return None
        arr, n = args[0], args[1]
        self.flops += sum(2.0 * d.rows * d.nout * d.K for d in arr[:n])
        self.kernels += 2 * ((n + 7) // 8)
        return name


#: output tile (nout, K) of the partial kernel of each arithmetic: dY is fetched ceil(K / tile K) times per launch and A
#: ceil(nout / tile nout) times
WGRAD_TILE = {"f32": (64, 64), "f16x2": (128, 256)}


def fetched_bytes(rows: int, nout: int, K: int, mode: str) -> int:
    """Operand bytes the partial kernel's tiling reads per launch (before any cache)."""
    tn, tk = WGRAD_TILE[mode]
    return 4 * rows * (nout * -(-K // tk) + K * -(-nout // tn))


def _dwe_alone(E: int, F: int, M: int, reps: int = 20, mode: str = "f32"):
    """The dWe problem of one layer as a launch of its own (with db), timed back to back."""
    from gotennet_amd import engine
    torch.manual_seed(0)
    nout = (1 + M) * F
    g_eproj, t_in = torch.randn(E, nout, device="cuda"), torch.randn(E, F, device="cuda")
    dW, db = torch.empty(nout, F, device="cuda"), torch.empty(nout, device="cuda")
    prob = [dict(dY=g_eproj, ldy=nout, A=t_in, lda=F, dW=dW, db=db, rows=E, nout=nout, K=F)]
    engine.weight_grad_group(prob, mode=mode)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        engine.weight_grad_group(prob, mode=mode)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    tf = 2.0 * E * nout * F / us / 1e6
    return dict(shape=f"{nout}x{F} over {E} rows", us=round(us, 1), tflops=round(tf, 2),
                frac_of_fp32_mfma_peak=round(tf / FP32_MFMA_PEAK_TFLOPS, 3),
                fetched_bytes=fetched_bytes(E, nout, F, mode),
                fetched_tb_per_s=round(fetched_bytes(E, nout, F, mode) / us / 1e6, 2))


def run(shape: str, steps: int, warmup: int, attn_dropout: float = 0.0, wgrad_mode: str = "f32"):
    import gotennet_amd
    from gotennet_amd import _lib
    from gotennet_amd.outputs import Atomwise
    from gotennet_amd.synthetic import make_batch
    sp = SHAPES[shape]
    torch.manual_seed(0)
    net = gotennet_amd.GotenNetWrapper(cutoff_fn=gotennet_amd.CosineCutoff(5.0), num_heads=8, scale_edge=False,
                                       sep_dir=True, sep_tensor=True, max_z=10, attn_dropout=attn_dropout,
                                       **sp["model"]).cuda().train()
    head = Atomwise(n_in=256, n_hidden=128, activation="silu").cuda().train()
    net.parameter_grads = head.parameter_grads = True
    net.wgrad_mode = head.wgrad_mode = wgrad_mode
    pos, batch, z = make_batch(sp["workload"], sp["n_mol"])
    inp = types.SimpleNamespace(z=z.cuda(), pos=pos.cuda(), batch=batch.cuda())
    target = torch.randn(sp["n_mol"], 1, device="cuda")
    opt = torch.optim.Adam(list(net.parameters()) + list(head.parameters()), lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        inp.representation, _ = net(inp)
        loss = ((head(inp)["y"] - target) ** 2).mean()
        loss.backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    timer = _WgradTimer()                          # a separate, instrumented step for the weight-gradient launches
    _lib.TIMER = timer
    try:
        step()
    finally:
        _lib.TIMER = None
    torch.cuda.synchronize()
    wg_ms = sum(a.elapsed_time(b) for _, a, b in timer.events)
    from gotennet_amd.graph import distance
    E = int(distance(inp.pos, inp.batch, net.cutoff, net.max_num_neighbors)[0].shape[1])
    return dict(shape=shape, attn_dropout=attn_dropout, wgrad_mode=wgrad_mode, n_mol=sp["n_mol"], atoms=int(z.shape[0]), edges=E, ms_per_step=round(ms, 3),
                molecules_per_s=round(sp["n_mol"] / ms * 1e3, 1), wgrad_ms=round(wg_ms, 3),
                wgrad_calls=len(timer.events), wgrad_kernels=timer.kernels, wgrad_gflop=round(timer.flops / 1e9, 2),
                wgrad_tflops=round(timer.flops / wg_ms / 1e9, 2) if wg_ms > 0 else None,
                dwe_alone=_dwe_alone(E, 256, net.gata_list[0].multiplier, mode=wgrad_mode))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="qm9,c2")
    ap.add_argument("--json", default=None)
    ap.add_argument("--attn-dropout", default="0", help="comma-separated attention-dropout probabilities, one run each")
    ap.add_argument("--wgrad-mode", default="f32", help="comma-separated weight-gradient arithmetics (f32 | f16x2), one run "
                    "each in the order given: alternate them (f32,f16x2,f32,f16x2) to compare within one run")
    a = ap.parse_args()
    from gotennet_amd import engine
    modes = [engine.resolve_wgrad_mode(m) for m in a.wgrad_mode.split(",")]
    out = [run(s, a.steps, a.warmup, float(p), m) for s in a.shapes.split(",") for p in a.attn_dropout.split(",")
           for m in modes]
    for r in out:
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(steps=a.steps, warmup=a.warmup, results=out), fh, indent=1)


if __name__ == "__main__":
    main()
