"""The fp64 yardstick of the relaxation tests: FIRE (Bitzek et al., PRL 97, 170201, the variant ASE's ``FIRE`` implements)
with per-molecule state, unit masses and a fixed-atom mask.  Plain torch on the CPU in fp64; shares no code with
``gotennet_amd``.

Per molecule, from the KEPT forces f (of the last completed step) and the velocities v, over the free atoms::

    status != 0                     nothing
    max |f_a| not finite            status 2, converged_at = step
    max |f_a|^2 <= fmax^2           status 1, converged_at = step
    n_pos < 0 (first step, v = 0)   n_pos = 0, c_v = 1, c_f = 0
    P = sum f.v > 0                 c_v = 1 - alpha, c_f = alpha sqrt(sum v^2 / sum f^2) (the OLD alpha); then, if n_pos > n_min,
                                    dt = min(dt f_inc, dt_max), alpha *= f_alpha; then n_pos += 1
    else                            c_v = c_f = 0, alpha = alpha_start, dt *= f_dec, n_pos = 0
    move                            v = c_v v + c_f f + dt f;  dr = dt v;  dr *= min(1, max_step / |dr|) (norm over the molecule);
                                    pos += dr
"""
import math

import numpy as np
import torch

DEFAULTS = dict(fmax=0.05, dt=0.1, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99)


def ulp32(x):
    """The spacing of fp32 at |x|, element-wise, as fp64."""
    return torch.from_numpy(np.spacing(np.abs(x.double().numpy()).astype(np.float32)).astype(np.float64))


def new_state(n_mol, p=DEFAULTS):
    return dict(dt=torch.full((n_mol,), p["dt"], dtype=torch.float64), alpha=torch.full((n_mol,), p["alpha"], dtype=torch.float64),
                n_pos=torch.full((n_mol,), -1, dtype=torch.int64), status=torch.zeros(n_mol, dtype=torch.int64),
                converged_at=torch.full((n_mol,), -1, dtype=torch.int64))


def fire_step(pos, vel, force, mol_ptr, state, p=DEFAULTS, fixed=None, step=0, coef=None):
    """One plan + move in fp64 -> (pos, vel, state, info); the inputs are left as they are.  ``mol_ptr``: n_mol + 1 ints.
    ``coef`` [n_mol, 4]: the move alone, with these coefficients (c_v, c_f, dt, active) instead of the plan's -- the state is
    handed back as it came.
    info (per molecule): fmax, P, ff, vv, absP = sum_a |f_a . v_a|, coef [n_mol, 4] = (c_v, c_f, dt, active), n2 = |dt v'|^2
    (0 where nothing moved), scale."""
    pos, vel, force = pos.double().clone(), vel.double().clone(), force.double()
    st = {k: v.clone() for k, v in state.items()}
    n_mol = len(mol_ptr) - 1
    free = torch.ones(pos.shape[0], dtype=torch.bool) if fixed is None else ~fixed.bool()
    info = {k: torch.zeros(n_mol, dtype=torch.float64) for k in ("fmax", "P", "ff", "vv", "absP", "n2")}
    info["scale"] = torch.ones(n_mol, dtype=torch.float64)
    info["coef"] = torch.zeros((n_mol, 4), dtype=torch.float64)
    for m in range(n_mol):
        idx = torch.arange(int(mol_ptr[m]), int(mol_ptr[m + 1]))
        idx = idx[free[idx]]
        f, v = force[idx], vel[idx]
        fm2 = float((f * f).sum(1).max()) if idx.numel() else 0.0
        if idx.numel() and bool(torch.isnan(f).any()):
            fm2 = float("nan")
        info["fmax"][m] = math.sqrt(fm2) if fm2 == fm2 else float("nan")
        info["P"][m], info["ff"][m], info["vv"][m] = (f * v).sum(), (f * f).sum(), (v * v).sum()
        info["absP"][m] = (f * v).sum(1).abs().sum() if idx.numel() else 0.0
        if coef is not None:
            c_v, c_f, dt, active = (float(x) for x in coef[m])
            if active == 0.0:
                continue
        elif int(st["status"][m]) != 0:
            continue
        elif not math.isfinite(fm2) or fm2 <= p["fmax"] ** 2:
            st["status"][m] = 1 if math.isfinite(fm2) else 2
            st["converged_at"][m] = step
            continue
        else:
            a_old, dt, P = float(st["alpha"][m]), float(st["dt"][m]), float(info["P"][m])
            if int(st["n_pos"][m]) < 0:
                st["n_pos"][m] = 0
                c_v, c_f = 1.0, 0.0
            elif P > 0:
                c_v, c_f = 1.0 - a_old, a_old * math.sqrt(float(info["vv"][m]) / float(info["ff"][m]))
                if int(st["n_pos"][m]) > p["n_min"]:
                    dt = min(dt * p["f_inc"], p["dt_max"])
                    st["alpha"][m] = a_old * p["f_alpha"]
                st["n_pos"][m] += 1
            else:
                c_v = c_f = 0.0
                st["alpha"][m] = p["alpha"]
                dt *= p["f_dec"]
                st["n_pos"][m] = 0
            st["dt"][m] = dt
        info["coef"][m] = torch.tensor([c_v, c_f, dt, 1.0], dtype=torch.float64)
        v = c_v * v + c_f * f + dt * f
        dr = dt * v
        n2 = float((dr * dr).sum())
        scale = min(1.0, p["max_step"] / math.sqrt(n2)) if n2 > 0 else 1.0
        info["n2"][m], info["scale"][m] = n2, scale
        vel[idx] = v
        pos[idx] = pos[idx] + scale * dr
    return pos, vel, st, info


def fire_run(energy_forces_fn, pos, mol_ptr, steps, p=DEFAULTS, fixed=None, on_step=None):
    """Up to ``steps`` steps from rest.  ``energy_forces_fn(pos) -> (energy [n_mol], forces [N, 3])``.  The kept energy and
    forces of a molecule are refreshed only while its status is 0.  Stops once no molecule is active.
    -> dict(pos, vel, energy, forces, state, steps (completed), history: per step dict(pos, vel, energy, forces, state, info) AFTER
    the step).  ``on_step(k, pos)``: a hook called with the moved positions of step k (before the model)."""
    n_mol = len(mol_ptr) - 1
    pos = pos.double().clone()
    vel = torch.zeros_like(pos)
    st = new_state(n_mol, p)
    e, f = energy_forces_fn(pos)
    e, f = e.double().clone().reshape(-1), f.double().clone()
    atom_mol = torch.repeat_interleave(torch.arange(n_mol), torch.as_tensor(mol_ptr[1:]) - torch.as_tensor(mol_ptr[:-1]))
    history, done = [], 0
    for k in range(steps):
        pos, vel, st, info = fire_step(pos, vel, f, mol_ptr, st, p, fixed, step=k)
        if on_step is not None:
            on_step(k, pos)
        e_new, f_new = energy_forces_fn(pos)
        act = st["status"] == 0
        e = torch.where(act, e_new.double().reshape(-1), e)
        f = torch.where(act[atom_mol].unsqueeze(1), f_new.double(), f)
        done = k + 1
        history.append(dict(pos=pos.clone(), vel=vel.clone(), energy=e.clone(), forces=f.clone(),
                            state={a: b.clone() for a, b in st.items()}, info=info))
        if not bool(act.any()):
            break
    if not bool((st["status"] == 0).any()):
        done = min(done, int(st["converged_at"].max()))
    return dict(pos=pos, vel=vel, energy=e, forces=f, state=st, steps=done, history=history)


# ----------------------------------------------------------------------------------------- the molecule reference run
REF_FMAX, REF_STEPS = 0.06, 24
#: what the fp64 reference run gives on the stated input (test_fire_host.test_the_reference_run_is_a_fair_input computes and
#: asserts it): molecule 0 converges at step 20, the others do not within 24 steps, and the list changes once (50 -> 48 edges:
#: the 4.88 pair of the second molecule leaves).
REF_CONVERGED_AT, REF_EDGE_COUNTS = [20, -1, -1], [50, 48]


def open_graph(pos, batch, cutoff):
    """Brute-force radius graph of isolated molecules in fp64: target-major, sources ascending, self-loops included (no cap: the
    callers' molecules are smaller than any).  -> (edge_index int64 [2, E], gap = min | |r| - cutoff | over the pairs of a molecule)."""
    pos = pos.double()
    dist = (pos.unsqueeze(0) - pos.unsqueeze(1)).norm(dim=2)
    same = batch.unsqueeze(0) == batch.unsqueeze(1)
    ti, sj = (same & (dist * dist < cutoff * cutoff)).nonzero(as_tuple=True)
    pairs = same & ~torch.eye(pos.shape[0], dtype=torch.bool)
    return torch.stack([sj, ti]), float((dist[pairs] - cutoff).abs().min())


_REFERENCE = {}


def molecule_reference(p=None, steps=REF_STEPS):
    """The fp64 run the GPU test is held to: ``md_util.md_molecules()`` from rest, ``pbc_util.make_model(32, 2, 2, seed=1)``, the
    oracle's forces on the brute-force radius graph (cutoff 5.0), ASE's defaults with fmax = 0.06, 24 steps.  Computed once;
    read-only.  -> ``fire_run``'s result plus edges (the edge count at the start and after every step), gap (the smallest distance
    of a pair from the cutoff over all steps), e0 / f0 (energy and forces at the start), mol_ptr, params."""
    from tests import md_util as MU
    from tests import pbc_util as U
    p = dict(DEFAULTS, fmax=REF_FMAX) if p is None else p
    key = (tuple(sorted(p.items())), steps)
    if key in _REFERENCE:
        return _REFERENCE[key]
    s = MU.md_molecules()
    _, _, sd, hsd, cfg = U.make_model(32, 2, 2, seed=1)
    batch, z, n_mol = s["batch"], s["z"], s["n_mol"]
    mol_ptr = [0] + torch.cumsum(torch.bincount(batch, minlength=n_mol), 0).tolist()
    zero_cell = torch.zeros((n_mol, 3, 3), dtype=torch.float64)
    edges, gaps = [], []

    def model(pos):
        ei, gap = open_graph(pos, batch, U.CUTOFF)
        edges.append(ei.shape[1]), gaps.append(gap)
        q = pos.clone().requires_grad_(True)
        vec, diff = U.edge_geometry(q, ei, torch.zeros((ei.shape[1], 3), dtype=torch.int64), zero_cell, batch)
        e = U.oracle_energy(sd, cfg, hsd, z, ei, diff, vec, batch, n_mol)
        return e.detach(), -torch.autograd.grad(e.sum(), q)[0]

    e0, f0 = model(s["pos"].double())
    edges.clear(), gaps.clear()
    out = fire_run(model, s["pos"], mol_ptr, steps, p)
    out.update(edges=edges, gap=min(gaps), e0=e0.reshape(-1), f0=f0, mol_ptr=mol_ptr, params=p)
    _REFERENCE[key] = out
    return out
