"""The fp64 yardstick of the variable-cell relaxation tests: the extended system (atom rows, then three cell rows per box), its
generalised forces, the apply step, and one relaxation step built as ``fire_util.fire_step`` on the extended system.  Plain
torch on the CPU in fp64; shares no code with ``gotennet_amd``.

Row-vector convention, per box m (ASE's ``UnitCellFilter``)::

    pos = x~ F,  cell = C0 F,  degrees of freedom: the rows of x~ and U = w F
    H = E + pressure |det cell|
    -dH/dx~ = f F^T                                  f: the forces,  sigma = (1/V) sum r (x) dE/dr: the stress (not symmetrised)
    -dH/dU  = -(V / w) F^-T S,   S = (sigma + sigma^T) / 2 + pressure 1   [hydrostatic: S <- (tr S / 3) 1;  then G *= cell_mask]

test_cellrelax_host.py proves the two lines against ``torch.autograd``.  Box m owns rows [mol_ptr[m] + 3 m,
mol_ptr[m + 1] + 3 (m + 1)) of the extended arrays."""
import itertools

import torch

from tests import fire_util as FU


def layout(mol_ptr):
    """-> dict(mol_ptr_ext: n_mol + 1 ints, atom_rows int64 [N], cell_rows int64 [n_mol, 3], NE = N + 3 n_mol)."""
    mol_ptr = [int(x) for x in mol_ptr]
    n = len(mol_ptr) - 1
    atom_rows = torch.tensor([a + 3 * m for m in range(n) for a in range(mol_ptr[m], mol_ptr[m + 1])], dtype=torch.int64)
    cell_rows = torch.tensor([[mol_ptr[m + 1] + 3 * m + c for c in range(3)] for m in range(n)], dtype=torch.int64).reshape(n, 3)
    return dict(mol_ptr_ext=[mol_ptr[m] + 3 * m for m in range(n + 1)], atom_rows=atom_rows, cell_rows=cell_rows,
                NE=mol_ptr[-1] + 3 * n)


def weights(mol_ptr, cell_factor=None):
    """fp64 [n_mol]: ``cell_factor``, default the atom count of the box, at least 1."""
    n = len(mol_ptr) - 1
    if cell_factor is None:
        return torch.tensor([max(int(mol_ptr[m + 1]) - int(mol_ptr[m]), 1) for m in range(n)], dtype=torch.float64)
    return torch.as_tensor(cell_factor, dtype=torch.float64).expand(n).clone()


def extend(x, mol_ptr, w, F=None):
    """The extended array of atom rows ``x`` [N, 3] and cell rows w F (F [n_mol, 3, 3], default the identity), fp64."""
    lay, n = layout(mol_ptr), len(mol_ptr) - 1
    F = torch.eye(3, dtype=torch.float64).expand(n, 3, 3) if F is None else F.double()
    out = torch.zeros((lay["NE"], 3), dtype=torch.float64)
    out[lay["atom_rows"]] = x.double()
    out[lay["cell_rows"]] = w.double().reshape(n, 1, 1) * F
    return out


def extend_fixed(fixed, mol_ptr):
    """The fixed mask of the extended rows: the cell rows are free."""
    lay = layout(mol_ptr)
    out = torch.zeros(lay["NE"], dtype=torch.bool)
    out[lay["atom_rows"]] = fixed.bool()
    return out


def deformation(x_ext, mol_ptr, w):
    """F [n_mol, 3, 3] = cell rows / w."""
    return x_ext.double()[layout(mol_ptr)["cell_rows"]] / w.double().reshape(-1, 1, 1)


def generalised_forces(force, stress, cell, x_ext, mol_ptr, w, pressure=0.0, hydrostatic=False, cell_mask=None, fixed=None):
    """g_ext fp64 [N + 3 n_mol, 3] of the forces [N, 3], the stress [n_mol, 3, 3] and the current cell [n_mol, 3, 3]."""
    lay, n = layout(mol_ptr), len(mol_ptr) - 1
    force, stress, cell, w = force.double(), stress.double().reshape(n, 3, 3), cell.double().reshape(n, 3, 3), w.double()
    F = deformation(x_ext, mol_ptr, w)
    out = torch.zeros((lay["NE"], 3), dtype=torch.float64)
    eye = torch.eye(3, dtype=torch.float64)
    for m in range(n):
        a0, a1 = int(mol_ptr[m]), int(mol_ptr[m + 1])
        g = force[a0:a1] @ F[m].T
        if fixed is not None:
            g = torch.where(fixed[a0:a1].bool().unsqueeze(1), torch.zeros_like(g), g)
        out[lay["atom_rows"][a0:a1]] = g
        V = torch.linalg.det(cell[m]).abs()
        S = 0.5 * (stress[m] + stress[m].T) + pressure * eye
        if hydrostatic:
            S = torch.trace(S) / 3.0 * eye
        G = -(V / w[m]) * torch.linalg.inv(F[m]).T @ S
        if cell_mask is not None:
            G = torch.where(cell_mask.bool().reshape(3, 3), G, torch.zeros_like(G))
        out[lay["cell_rows"][m]] = G
    return out


def apply(x_ext, cell0, mol_ptr, w, pos, cell, active=None):
    """pos = x~ F and cell = C0 F for the boxes with ``active`` [n_mol] (default: all); the others keep ``pos`` / ``cell``."""
    lay, n = layout(mol_ptr), len(mol_ptr) - 1
    x_ext, pos, cell = x_ext.double(), pos.double().clone(), cell.double().reshape(n, 3, 3).clone()
    F = deformation(x_ext, mol_ptr, w)
    for m in range(n):
        if active is not None and not bool(active[m]):
            continue
        a0, a1 = int(mol_ptr[m]), int(mol_ptr[m + 1])
        pos[a0:a1] = x_ext[lay["atom_rows"][a0:a1]] @ F[m]
        cell[m] = cell0.double().reshape(n, 3, 3)[m] @ F[m]
    return pos, cell


def relax_step(x_ext, vel_ext, force, stress, pos, cell, cell0, mol_ptr, w, state, p=FU.DEFAULTS, pressure=0.0, hydrostatic=False,
               cell_mask=None, fixed=None, step=0, coef=None):
    """One step before the model: generalised forces -> ``fire_util.fire_step`` on the extended system -> apply.
    -> (x_ext, vel_ext, pos, cell, state, info); info as fire_step's plus g_ext."""
    lay = layout(mol_ptr)
    g = generalised_forces(force, stress, cell, x_ext, mol_ptr, w, pressure, hydrostatic, cell_mask, fixed)
    fx = None if fixed is None else extend_fixed(fixed, mol_ptr)
    x1, v1, st, info = FU.fire_step(x_ext, vel_ext, g, lay["mol_ptr_ext"], state, p, fx, step=step, coef=coef)
    pos1, cell1 = apply(x1, cell0, mol_ptr, w, pos, cell, active=info["coef"][:, 3] == 1.0)
    info["g_ext"] = g
    return x1, v1, pos1, cell1, st, info


def relax_run(model, pos, cell, mol_ptr, steps, p=FU.DEFAULTS, pressure=0.0, hydrostatic=False, cell_mask=None, fixed=None,
              cell_factor=None):
    """Up to ``steps`` steps from rest.  ``model(pos, cell) -> (energy [n_mol], forces [N, 3], stress [n_mol, 3, 3])``.  The kept
    values of a box are refreshed only while its status is 0.  -> dict(pos, cell, x_ext, vel_ext, energy, forces, stress, state, w,
    steps, history: per step dict(pos, cell, F, energy, enthalpy, state) AFTER the step, enthalpy0)."""
    n = len(mol_ptr) - 1
    w = weights(mol_ptr, cell_factor)
    pos, cell = pos.double().clone(), cell.double().reshape(n, 3, 3).clone()
    cell0 = cell.clone()
    x, v = extend(pos, mol_ptr, w), torch.zeros((layout(mol_ptr)["NE"], 3), dtype=torch.float64)
    st = FU.new_state(n, p)
    e, f, s = (t.double().clone() for t in model(pos, cell))
    e = e.reshape(-1)
    atom_mol = torch.repeat_interleave(torch.arange(n), torch.tensor([int(mol_ptr[m + 1]) - int(mol_ptr[m]) for m in range(n)]))
    enthalpy = lambda: e + pressure * torch.linalg.det(cell).abs()
    h0, history, done = enthalpy(), [], 0
    for k in range(steps):
        x, v, pos, cell, st, _ = relax_step(x, v, f, s, pos, cell, cell0, mol_ptr, w, st, p, pressure, hydrostatic, cell_mask, fixed,
                                            step=k)
        e1, f1, s1 = model(pos, cell)
        act = st["status"] == 0
        e = torch.where(act, e1.double().reshape(-1), e)
        f = torch.where(act[atom_mol].unsqueeze(1), f1.double(), f)
        s = torch.where(act.reshape(n, 1, 1), s1.double(), s)
        done = k + 1
        history.append(dict(pos=pos.clone(), cell=cell.clone(), F=deformation(x, mol_ptr, w), energy=e.clone(), enthalpy=enthalpy(),
                            state={a: b.clone() for a, b in st.items()}))
        if not bool(act.any()):
            break
    return dict(pos=pos, cell=cell, x_ext=x, vel_ext=v, energy=e, forces=f, stress=s, state=st, w=w, steps=done, history=history,
                enthalpy0=h0)


# ------------------------------------------------------------------------------- an analytic periodic potential, in fp64
MORSE = dict(D=0.5, a=2.0, r0=1.0)
_IMAGES = torch.tensor(list(itertools.product(range(-2, 3), repeat=3)), dtype=torch.float64)


def morse_edges(n_atoms):
    """Every image in {-2..2}^3 of every ordered pair of a box but the atom itself -> (i [E], j [E], image fp64 [E, 3]).  The set
    is FIXED (no cutoff), so the energy below is a smooth function of positions and cell."""
    i, j, t = torch.meshgrid(torch.arange(n_atoms), torch.arange(n_atoms), torch.arange(len(_IMAGES)), indexing="ij")
    keep = ~((i == j) & (_IMAGES[t].abs().sum(-1) == 0))
    return i[keep], j[keep], _IMAGES[t[keep]]


def morse_energy_of_vectors(vec):
    """(1/2) sum over directed edges of D ((1 - exp(-a (r - r0)))^2 - 1)."""
    r = vec.norm(dim=1)
    return 0.5 * (MORSE["D"] * ((1.0 - torch.exp(-MORSE["a"] * (r - MORSE["r0"]))) ** 2 - 1.0)).sum()


def morse_box(pos, cell):
    """One box -> (energy, forces [n, 3], stress [3, 3] = (1/V) sum_edges r (x) dE/dr by autograd over the edge vectors)."""
    pos, cell = pos.double(), cell.double()
    i, j, img = morse_edges(pos.shape[0])
    vec = (pos[j] - pos[i] + img @ cell).detach().requires_grad_(True)
    e = morse_energy_of_vectors(vec)
    dEdr, = torch.autograd.grad(e, vec)
    stress = torch.einsum("el,ek->lk", vec.detach(), dEdr) / torch.linalg.det(cell).abs()
    q = pos.detach().clone().requires_grad_(True)
    f = -torch.autograd.grad(morse_energy_of_vectors(q[j] - q[i] + img @ cell), q)[0]
    return e.detach(), f, stress


def morse_model(mol_ptr):
    """``relax_run``'s model for a batch of boxes."""
    n = len(mol_ptr) - 1

    def model(pos, cell):
        out = [morse_box(pos[int(mol_ptr[m]):int(mol_ptr[m + 1])], cell.reshape(n, 3, 3)[m]) for m in range(n)]
        return torch.stack([o[0] for o in out]), torch.cat([o[1] for o in out]), torch.stack([o[2] for o in out])
    return model


def within_ulps(got, want, k=1):
    """|got - want| <= k fp32 spacings at |want|, element-wise (``want`` fp64); NaN matches NaN."""
    got, want = got.double(), want.double()
    both_nan = torch.isnan(got) & torch.isnan(want)
    return both_nan | ((got - want).abs() <= k * FU.ulp32(want))
