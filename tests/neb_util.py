"""The fp64 yardstick of the nudged-elastic-band tests: the band forces (improved tangent of Henkelman and Jonsson, J. Chem.
Phys. 113, 9978, ASE's ``improvedtangent``; optional climbing image) and the band-wise FIRE step built on
``fire_util.fire_step``.  Plain torch on the CPU in fp64; shares no code with ``gotennet_amd``.

Molecules ``b * n_img .. (b + 1) * n_img - 1`` are the images of band b; atom a of image i pairs with the atom at the same
offset from ``mol_ptr`` in the neighbouring images.  Interior image i, over its free atoms, with t+ = R_{i+1} - R_i,
t- = R_i - R_{i-1} and the energies E-, E, E+ compared AS THEY ARE GIVEN (fp32 in, fp32 compared: the same branch as the
device by construction)::

    E+ > E > E-        t = t+
    E+ < E < E-        t = t-
    otherwise          dmax / dmin = the larger / smaller of |E+ - E|, |E- - E|;  E+ > E-: t = dmax t+ + dmin t-,
                       else (ties included) t = dmin t+ + dmax t-
    ordinary image     g = f - (f.t / |t|^2) t + k (|t+| - |t-|) t / |t|
    climbing image     g = f - 2 (f.t / |t|^2) t       (climb: the interior image with the largest energy, the first of equal ones)
    |t|^2 == 0         g = f
    an energy of the three not finite      g = NaN
    end images, fixed atoms, atoms beyond the shortest of the three images      g = 0


The bound of the device test (``g_bound``)
------------------------------------------
The device forms the same expression in fp64 from the same fp32 inputs and rounds once to fp32, so it differs from this
yardstick by (a) the final cast and (b) the order of the five fp64 sums (and a dozen elementary fp64 roundings).

(a) The cast: |fp32(x) - x| <= ulp32(x) / 2; the device casts x' = x + e with e from (b), so |fp32(x') - x| <= ulp32(x) / 2
    + |e| + (a neighbouring binade's half ulp) <= ulp32(x) + |e|.  That is the first term: one fp32 ulp of the reference value.

(b) With u = 2^-53 and n = 3 * (atoms of the image) terms per sum, a sum of n fp64 terms in ANY order is off by at most
    (n - 1) u sum |terms|.  By Cauchy-Schwarz sum |f t+-| <= |f| |t+-| and sum |t+ t-| <= |t+| |t-|, with |f| the norm of the
    image's free forces.  Write t = c+ t+ + c- t- (c+-  >= 0) and kappa = (c+ |t+| + c- |t-|) / |t| >= 1, the conditioning of the
    tangent (1 on the two single-sided branches; large only where t+ and t- nearly cancel in the mix).  Then, to first order,
        f.t       is off by  n u |f| (c+ |t+| + c- |t-|)  =  n u kappa |f| |t|
        |t|^2     is off by  n u (c+ |t+| + c- |t-|)^2    =  n u kappa^2 |t|^2        (relative: n u kappa^2)
        |t+|, |t-|  are off by  n u |t+-| / 2    (sums of squares: relative n u, halved by the root)
    and every component |t_ac| <= |t|, so the projection term (f.t / |t|^2) t_ac is off by at most n u (kappa + kappa^2) |f|, and
    the spring term k (|t+| - |t-|) t_ac / |t| by at most n u k (|t+| + |t-|) (1 + kappa^2) / 2.  With kappa <= kappa^2 both
    sides -- device and yardstick -- stay within  2 n u kappa^2 (|f| + k (|t+| + |t-|))  of the exact value of an ordinary image
    and twice the |f| part for the climbing image (its projection is doubled), so they differ from each other by at most
        8 n u kappa^2 (|f| + k (|t+| + |t-|))  +  the elementary roundings, about 40 u of the same magnitudes.
    The tests' largest image has 300 atoms, n = 900:  8 * 900 + 40 = 7240 < 8192 = 2^13, and 2^13 u = 2^-40.  That is the second
    term:  2^-40 kappa^2 (|f| + k (|t+| + |t-|)).

This differs from the form 2^-40 (|f_a| + k (|t+| + |t-|)) in two places, both forced by the derivation: the error of the
projection COEFFICIENT f.t / |t|^2 scales with the image's |f|, not with the atom's |f_a| (an atom with f_a = 0 and t_a != 0
inherits it), and the mix branch carries kappa^2.  kappa is a property of the input, computed here in fp64.
"""
import math

import torch

from tests import fire_util as FU


def _counts(mol_ptr):
    return [int(mol_ptr[m + 1]) - int(mol_ptr[m]) for m in range(len(mol_ptr) - 1)]


def climbing_image(energy, first, n_img):
    """The interior image of the band starting at molecule ``first`` with the largest energy, the first of equal ones."""
    ci, best = 1, energy[first + 1]
    for j in range(2, n_img - 1):
        if bool(energy[first + j] > best):
            ci, best = j, energy[first + j]
    return ci


def neb_forces(pos, force, energy, mol_ptr, n_img, k, climb, fixed=None, detail=False):
    """-> (g [N, 3] fp64, e_band [n_band] in ``energy``'s dtype: the largest energy of the band, a NaN wins, climb [n_band]: the
    climbing image's index or -1).  ``energy`` is compared in the dtype it comes in; everything else is fp64.
    ``detail=True`` adds a dict of per-ATOM fp64 tensors of the atom's image: kappa2, fnorm (|f| over the free atoms), tp, tm
    (|t+|, |t-|) and branch (0 end / fixed / unpaired, 1 t+, 2 t-, 3 mix towards t+, 4 mix towards t-, 5 |t| = 0, 6 not finite;
    +10 for the climbing image)."""
    pos, force = pos.double(), force.double()
    N, n_mol = pos.shape[0], len(mol_ptr) - 1
    assert n_img >= 3 and n_mol % n_img == 0
    free = torch.ones(N, dtype=torch.bool) if fixed is None else ~fixed.bool()
    g = torch.zeros((N, 3), dtype=torch.float64)
    n_band = n_mol // n_img
    e_band, ci_out = torch.zeros(n_band, dtype=energy.dtype), torch.full((n_band,), -1, dtype=torch.int64)
    info = {name: torch.zeros(N, dtype=torch.float64) for name in ("kappa2", "fnorm", "tp", "tm", "branch")}
    count = _counts(mol_ptr)
    for b in range(n_band):
        first = b * n_img
        e = energy[first:first + n_img]
        e_band[b] = float("nan") if bool(torch.isnan(e).any()) else e.max()
        ci = climbing_image(energy, first, n_img) if climb else -1
        ci_out[b] = ci
        for i in range(1, n_img - 1):
            m = first + i
            n = min(count[m - 1], count[m], count[m + 1])
            idx = torch.arange(n)
            idx = idx[free[int(mol_ptr[m]) + idx]]
            a, lo, hi = int(mol_ptr[m]) + idx, int(mol_ptr[m - 1]) + idx, int(mol_ptr[m + 1]) + idx
            Em, E0, Ep = energy[m - 1], energy[m], energy[m + 1]
            tp, tm, f = pos[hi] - pos[a], pos[a] - pos[lo], force[a]
            if bool(Ep > E0) and bool(E0 > Em):
                cp, cm, branch = 1.0, 0.0, 1
            elif bool(Ep < E0) and bool(E0 < Em):
                cp, cm, branch = 0.0, 1.0, 2
            else:
                dp, dm = abs(float(Ep.double()) - float(E0.double())), abs(float(Em.double()) - float(E0.double()))
                dmax, dmin = (dp, dm) if dp > dm else (dm, dp)
                cp, cm, branch = (dmax, dmin, 3) if bool(Ep > Em) else (dmin, dmax, 4)
            pp, mm, pm = float((tp * tp).sum()), float((tm * tm).sum()), float((tp * tm).sum())
            fp, fm = float((f * tp).sum()), float((f * tm).sum())
            finite = all(math.isfinite(float(x)) for x in (Em, E0, Ep))
            if not finite:
                g[a], branch = float("nan"), 6
            else:
                tt = cp * cp * pp + 2.0 * cp * cm * pm + cm * cm * mm
                ft = cp * fp + cm * fm
                t = cp * tp + cm * tm
                if tt == 0.0:
                    g[a], branch = f, 5
                elif i == ci:
                    g[a] = f - 2.0 * (ft / tt) * t
                else:
                    g[a] = f + (k * (math.sqrt(pp) - math.sqrt(mm)) / math.sqrt(tt) - ft / tt) * t
                if tt > 0.0:
                    info["kappa2"][a] = (cp * math.sqrt(pp) + cm * math.sqrt(mm)) ** 2 / tt
            info["fnorm"][a], info["tp"][a], info["tm"][a] = float(f.norm()), math.sqrt(pp), math.sqrt(mm)
            info["branch"][a] = branch + (10 if i == ci else 0)
    return (g, e_band, ci_out, info) if detail else (g, e_band, ci_out)


def g_bound(ref, info, k):
    """[N, 3]: the a-priori bound on |g_device - ref| of the module docstring (``ref``, ``info``: ``neb_forces(..., detail=True)``)."""
    scale = info["kappa2"].clamp_min(1.0) * (info["fnorm"] + k * (info["tp"] + info["tm"]))
    return FU.ulp32(ref) + (2.0 ** -40 * scale).unsqueeze(1)


def band_ptr(mol_ptr, n_img):
    return [int(x) for x in list(mol_ptr)[::n_img]]


def band_fixed(mol_ptr, n_img, fixed=None):
    """The mask FIRE sees: the user's OR the atoms of the end images."""
    n_mol, N = len(mol_ptr) - 1, int(mol_ptr[-1])
    out = torch.zeros(N, dtype=torch.bool) if fixed is None else fixed.bool().clone()
    for m in range(n_mol):
        if m % n_img in (0, n_img - 1):
            out[int(mol_ptr[m]):int(mol_ptr[m + 1])] = True
    return out


def neb_step(pos, vel, force, energy, mol_ptr, n_img, k, climb, state, p=FU.DEFAULTS, fixed=None, step=0):
    """``neb_forces`` on the kept (force, energy), then one ``fire_util.fire_step`` per BAND on g -> (pos, vel, state, info);
    info is fire_step's plus g, e_band, climb."""
    g, e_band, ci = neb_forces(pos, force, energy, mol_ptr, n_img, k, climb, fixed)
    pos, vel, st, info = FU.fire_step(pos, vel, g, band_ptr(mol_ptr, n_img), state, p, band_fixed(mol_ptr, n_img, fixed), step=step)
    info.update(g=g, e_band=e_band, climb=ci)
    return pos, vel, st, info


def neb_run(energy_forces_fn, pos, mol_ptr, n_img, k, climb, steps, p=FU.DEFAULTS, fixed=None):
    """Up to ``steps`` steps from rest.  ``energy_forces_fn(pos) -> (energy [n_mol], forces [N, 3])``.  The kept energies and forces
    of a band's images are refreshed only while the band's status is 0.  Stops once no band is active.
    -> dict(pos, vel, energy, forces, state, steps (completed), history: per step dict(pos, vel, energy, forces, state, info)
    AFTER the step)."""
    n_mol = len(mol_ptr) - 1
    n_band = n_mol // n_img
    pos = pos.double().clone()
    vel = torch.zeros_like(pos)
    st = FU.new_state(n_band, p)
    e, f = energy_forces_fn(pos)
    e, f = e.double().clone().reshape(-1), f.double().clone()
    atom_band = torch.repeat_interleave(torch.arange(n_mol), torch.tensor(_counts(mol_ptr))) // n_img
    history, done = [], 0
    for s in range(steps):
        pos, vel, st, info = neb_step(pos, vel, f, e, mol_ptr, n_img, k, climb, st, p, fixed, step=s)
        e_new, f_new = energy_forces_fn(pos)
        act = st["status"] == 0
        e = torch.where(act.repeat_interleave(n_img), e_new.double().reshape(-1), e)
        f = torch.where(act[atom_band].unsqueeze(1), f_new.double(), f)
        done = s + 1
        history.append(dict(pos=pos.clone(), vel=vel.clone(), energy=e.clone(), forces=f.clone(),
                            state={a: b.clone() for a, b in st.items()}, info=info))
        if not bool(act.any()):
            break
    if not bool((st["status"] == 0).any()):
        done = min(done, int(st["converged_at"].max()))
    return dict(pos=pos, vel=vel, energy=e, forces=f, state=st, steps=done, history=history)


# ------------------------------------------------------------------------------------------- the band reference run
REF_N_IMG, REF_K, REF_CLIMB, REF_STEPS, REF_FMAX = 5, 0.1, True, 16, 0.05
#: between the two bands' largest |g| at the start (0.236 and 1.110): band 0 is converged at step 0, band 1 is not
FREEZE_FMAX = 0.5
#: the displacements of the two end points from ``md_util.md_molecules()``' first two geometries (3 and 4 atoms), Angstrom
REF_SHIFT_FIRST = [[-0.10, 0.05, 0.00], [0.05, -0.10, 0.05], [0.10, 0.05, -0.05],
                   [-0.05, 0.10, 0.05], [0.00, -0.05, 0.10], [0.05, 0.10, -0.10], [-0.20, -0.05, 0.00]]
REF_SHIFT_LAST = [[0.15, -0.10, 0.10], [-0.10, 0.25, -0.15], [-0.15, -0.20, 0.20],
                  [0.10, -0.15, -0.10], [-0.05, 0.30, -0.20], [0.10, -0.25, 0.25], [-0.45, 0.20, -0.15]]


def band_start(n_img=REF_N_IMG):
    """Two bands (3 and 4 atoms per image) between two distorted copies of the first two ``md_util.md_molecules()`` geometries,
    interpolated linearly in fp64 and rounded to fp32 -> dict(z, pos fp32, batch, n_mol, mol_ptr).  Built here, without the
    package, so that the yardstick stands alone; ``test_neb_host`` checks that ``gotennet_amd.neb.band`` gives the same bits."""
    from tests import md_util as MU
    s = MU.md_molecules()
    base, z = s["pos"][:7].double(), s["z"][:7]
    first = (base + torch.tensor(REF_SHIFT_FIRST, dtype=torch.float64)).float().double()
    last = (base + torch.tensor(REF_SHIFT_LAST, dtype=torch.float64)).float().double()
    zs, ps, bs, mol_ptr = [], [], [], [0]
    for b, sel in enumerate((slice(0, 3), slice(3, 7))):
        for i in range(n_img):
            zs.append(z[sel])
            ps.append((first[sel] + (i / (n_img - 1)) * (last[sel] - first[sel])).float())
            bs.append(torch.full((ps[-1].shape[0],), b * n_img + i, dtype=torch.int64))
            mol_ptr.append(mol_ptr[-1] + ps[-1].shape[0])
    return dict(z=torch.cat(zs), pos=torch.cat(ps), batch=torch.cat(bs), n_mol=2 * n_img, mol_ptr=mol_ptr,
                z_ab=z, batch_ab=s["batch"][:7], pos_first=first.float(), pos_last=last.float())


_REFERENCE = {}


def band_reference(climb=REF_CLIMB, fmax=REF_FMAX, steps=REF_STEPS):
    """The fp64 run the GPU test is held to: ``band_start()`` from rest, ``pbc_util.make_model(32, 2, 2, seed=1)``, the oracle's
    forces on the brute-force radius graph (cutoff 5.0), FIRE's defaults, k = 0.1.  Computed once; read-only.
    -> ``neb_run``'s result plus edges (the edge count at the start and after every step), gap (the smallest distance of a pair
    from the cutoff over all steps), e0 / f0 (energy and forces at the start), mol_ptr, params."""
    from tests import pbc_util as U
    key = (bool(climb), float(fmax), int(steps))
    if key in _REFERENCE:
        return _REFERENCE[key]
    p = dict(FU.DEFAULTS, fmax=fmax)
    s = band_start()
    _, _, sd, hsd, cfg = U.make_model(32, 2, 2, seed=1)
    batch, z, n_mol = s["batch"], s["z"], s["n_mol"]
    zero_cell = torch.zeros((n_mol, 3, 3), dtype=torch.float64)
    edges, gaps = [], []

    def model(pos):
        ei, gap = FU.open_graph(pos, batch, U.CUTOFF)
        edges.append(ei.shape[1]), gaps.append(gap)
        q = pos.clone().requires_grad_(True)
        vec, diff = U.edge_geometry(q, ei, torch.zeros((ei.shape[1], 3), dtype=torch.int64), zero_cell, batch)
        e = U.oracle_energy(sd, cfg, hsd, z, ei, diff, vec, batch, n_mol)
        return e.detach(), -torch.autograd.grad(e.sum(), q)[0]

    e0, f0 = model(s["pos"].double())
    edges.clear(), gaps.clear()
    out = neb_run(model, s["pos"], s["mol_ptr"], REF_N_IMG, REF_K, climb, steps, p)
    out.update(edges=edges, gap=min(gaps), e0=e0.reshape(-1), f0=f0, mol_ptr=s["mol_ptr"], params=p)
    _REFERENCE[key] = out
    return out
