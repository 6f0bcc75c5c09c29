"""fp64 adjoints of the oracle at the stage boundaries of ``engine.backward(..., trace=)`` (test infrastructure).

``forward_with_intermediates`` restates ``orc.gotennet_forward``'s loop (gotennet.py:956-1010) from the oracle's public
pieces and keeps the tensors whose adjoints the HIP backward's trace records: h0, t0 and phi of the init; per layer the
normalised inputs, the message stage's output, the layer's output (h, X and t after HTR); the edge inputs.
``tests/test_hip_adjoints.py`` pins the restatement to ``orc.gotennet_forward`` (bit-identical h, X) and to
``orc.energy_and_forces`` before any GPU result is compared with it.

``adjoints`` returns dL/d of each kept tensor for a scalar loss, keyed like the HIP trace: ("layer", li), ("message", li),
("norm", li), ("init", -1).  ``check_adjoint`` is the comparison: max-norm relative error per molecule (and per degree
block of X-like tensors), each group measured against its own largest value.
"""
import math

import torch

from oracle import gotennet_oracle as orc
from tests.golden_util import degree_blocks, group_rel_err, rel_err


def forward_with_intermediates(sd, cfg, z, edge_index, edge_diff, edge_vec):
    """-> (h, X, st).  ``st`` holds the kept tensors: phi, h0, t0, X0, vec, diff (identity views of ``edge_vec`` /
    ``edge_diff``: their adjoints are the partial derivatives the HIP backward returns, not the totals through
    edge_diff = |edge_vec| when the caller built one from the other) and ``layers``, one dict per layer with h_norm,
    X_norm, h_msg, X_msg, h, X, t.  Same arithmetic as orc.gotennet_forward, op for op."""
    Fd, L, lmax = cfg["n_atom_basis"], cfg["n_interactions"], cfg["lmax"]
    dt = sd["A_na.weight"].dtype
    grad = torch.is_grad_enabled()
    edge_vec, edge_diff = edge_vec.view_as(edge_vec), edge_diff.view_as(edge_diff)
    h = sd["A_na.weight"][z]
    phi = orc.radial_basis(sd, cfg, edge_diff)
    h = orc.node_init(sd, cfg, z, h, edge_index, edge_diff, phi)
    h0 = h
    t = orc.edge_init(sd, edge_index, phi, h)
    t0 = t
    # rl and n_edges as in orc.gotennet_forward
    mask = (edge_index[0] != edge_index[1]).unsqueeze(1)
    nrm = torch.norm(edge_vec, dim=1, keepdim=True)
    unit = torch.where(mask, edge_vec / torch.where(mask, nrm, torch.ones_like(nrm)), edge_vec)
    rl = orc.real_harmonics(lmax, unit)
    N = h.shape[0]
    deg = torch.zeros(N, dtype=edge_diff.dtype).index_add_(0, edge_index[0], torch.ones_like(edge_diff))
    n_edges = deg[edge_index[0]]
    D = (lmax + 1) ** 2 - 1
    X = torch.zeros((N, D, Fd), dtype=torch.promote_types(dt, torch.float32), requires_grad=grad)
    X0 = X
    layers = []
    for li in range(L):
        p = f"gata_list.{li}."
        hn, Xn = orc.gata_input_norms(sd, cfg, p, h, X)
        hm, Xm = orc.gata_message_aggregate(sd, cfg, p, edge_index, hn, Xn, rl, t, edge_diff, n_edges)
        if li != L - 1 and cfg.get("edge_updates", True):
            t = orc.gata_htr(sd, cfg, p, edge_index, Xm, rl, t)
        elif grad:
            t = t.view_as(t)            # the layer's own output t: its adjoint counts the later layers' reads only
        h, X = orc.eqff(sd, cfg, f"eqff_list.{li}.", hm, Xm)
        layers.append(dict(h_norm=hn, X_norm=Xn, h_msg=hm, X_msg=Xm, h=h, X=X, t=t))
    return h, X, dict(phi=phi, h0=h0, t0=t0, X0=X0, vec=edge_vec, diff=edge_diff, layers=layers)


def _checkpoints(st, cfg):
    """(trace key, name in the trace dict, kept tensor) of every checkpoint of engine.backward's trace."""
    out = []
    norms = bool(cfg.get("layernorm", "")) or bool(cfg.get("steerable_norm", ""))
    for li, d in enumerate(st["layers"]):
        out += [(("layer", li), "h", d["h"]), (("layer", li), "X", d["X"]), (("layer", li), "t", d["t"]),
                (("message", li), "h", d["h_msg"]), (("message", li), "X", d["X_msg"])]
        if norms:
            out += [(("norm", li), "h", d["h_norm"]), (("norm", li), "X", d["X_norm"])]
    out += [(("init", -1), k, st[s]) for k, s in (("h", "h0"), ("t", "t0"), ("phi", "phi"), ("X", "X0"), ("vec", "vec"),
                                                  ("diff", "diff"))]
    return out


def adjoints(loss, st, cfg):
    """dL/d of every checkpoint tensor of ``st`` (fp64; zeros where the loss does not depend on it), as
    {(stage, layer): {name: tensor}}.  The graph is retained: several losses may be taken from one forward."""
    cps = _checkpoints(st, cfg)
    inputs = [v for _, _, v in cps]
    grads = torch.autograd.grad(loss, inputs, retain_graph=True, allow_unused=True)
    out = {}
    for (key, name, v), g in zip(cps, grads):
        out.setdefault(key, {})[name] = (torch.zeros_like(v) if g is None else g).detach()
    return out


def oracle_adjoints(sd, cfg, head_sd, z, pos, batch, n_mol, max_num_neighbors, upstream):
    """The fp64 oracle on a batch with its adjoints for two losses: (a) the Atomwise energy summed over the molecules,
    (b) sum(wh * h) + sum(wX * X) with ``upstream = (wh, wX)``.  -> dict: edge_index, h, X, forces, adj_a, adj_b."""
    d64 = lambda s: {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in s.items()}
    sd64, hsd64 = d64(sd), d64(head_sd)
    with torch.enable_grad():
        p64 = pos.detach().cpu().double().clone().requires_grad_(True)
        ei, w, vec = orc.distance(p64, batch, cfg["cutoff"], max_num_neighbors)
        h, X, st = forward_with_intermediates(sd64, cfg, z, ei, w, vec)
        e = orc.atomwise_energy(hsd64, h, batch, n_mol, z=z)
        adj_a = adjoints(e.sum(), st, cfg)
        (g,) = torch.autograd.grad(e.sum(), p64, retain_graph=True)
        wh, wX = (u.detach().cpu().double() for u in upstream)
        adj_b = adjoints((wh * h).sum() + (wX * X).sum(), st, cfg)
    return dict(edge_index=ei, h=h.detach(), X=X.detach(), forces=-g, adj_a=adj_a, adj_b=adj_b)


def seeded_model(hp, seed, head_hidden=32):
    """(net, head, oracle config) on the CPU: a mirror GotenNet with constructor arguments ``hp`` and an Atomwise SiLU head,
    every bias non-zero and every norm weight other than 1 (so each epilogue and norm backward sees general values)."""
    import gotennet_amd
    from gotennet_amd.outputs import Atomwise
    torch.manual_seed(seed)
    net = gotennet_amd.GotenNet(cutoff_fn=gotennet_amd.CosineCutoff(5.0), max_z=10, **hp)
    head = Atomwise(n_in=hp["n_atom_basis"], n_hidden=head_hidden, derivative="forces", activation="silu")
    with torch.no_grad():
        for m in (net, head):
            for n, p in m.named_parameters():
                if p.dim() == 1:
                    p.uniform_(-0.05, 0.05) if not n.endswith("norm.weight") else p.uniform_(0.9, 1.1)
        for n, b in net.named_buffers():
            if n.endswith("tensor_layernorm.weight"):
                b.uniform_(0.9, 1.1)
    cfg = orc.default_config(cutoff=5.0, **{k: v for k, v in hp.items() if k not in ("evec_dim", "emlp_dim", "edge_ln")})
    return net, head, cfg


# ------------------------------------------------------------------------------------------------------------ comparison
#: kind of each checkpoint name: atom rows (h), atom rows per degree block (X), edge rows (t, phi), non-self edge rows
KIND = {"h": "atom", "X": "block", "t": "edge", "phi": "edge", "vec": "bond", "diff": "bond"}


def groups(batch, edge_index):
    """Index tensors of each molecule's atoms, edges (by target) and non-self-loop edges: the groups errors are measured in.
    (The edge-input adjoints of a self-loop are not defined: its edge_vec is 0 whatever the positions.)"""
    b = batch.detach().cpu()
    src, dst = edge_index[0].cpu(), edge_index[1].cpu()
    eb = b[dst]
    out = {"atom": [], "edge": [], "bond": []}
    for m in range(int(b.max()) + 1 if b.numel() else 0):
        out["atom"].append(torch.nonzero(b == m).squeeze(1))
        out["edge"].append(torch.nonzero(eb == m).squeeze(1))
        out["bond"].append(torch.nonzero((eb == m) & (src != dst)).squeeze(1))
    out["block"] = out["atom"]
    return out


def adjoint_error(got, ref, kind, grp, lmax):
    """Worst per-molecule (X-like: per molecule AND degree block) max-norm relative error of ``got`` against ``ref``."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    errs = []
    for idx in grp[kind]:
        if idx.numel() == 0:
            continue
        a, b = got[idx], ref[idx]
        errs += group_rel_err(a, b, degree_blocks(lmax)) if kind == "block" else [rel_err(a, b)]
    return max(errs) if errs else 0.0


def check_adjoint(got, ref, kind, grp, lmax, bound):
    """(ok, error).  An adjoint that is zero in truth must be exactly zero (a relative error would be undefined)."""
    if not bool(ref.ne(0).any()):
        nz = int(torch.count_nonzero(got.detach().cpu()))
        return nz == 0, (0.0 if nz == 0 else math.inf)
    err = adjoint_error(got, ref, kind, grp, lmax)
    return err < bound, err
