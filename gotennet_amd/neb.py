"""Minimum-energy paths on the fused energy + force step: the nudged elastic band (NEB) method with the improved tangent of
Henkelman and Jonsson (J. Chem. Phys. 113, 9978; ASE's ``improvedtangent``) and, optionally, a climbing image (Henkelman,
Uberuaga and Jonsson, J. Chem. Phys. 113, 9901), relaxed by ``relax.Relax``'s FIRE inside the replayed step (kernels:
csrc/gn_neb.hip, csrc/gn_fire.hip).

The images of a band are molecules of the batch: molecules ``b * n_images .. (b + 1) * n_images - 1`` are band ``b``, the first
and the last of them the fixed end points.  One step, in every mode of the driver::

    gn_neb_forces -> gn_fire_plan -> gn_fire_move -> [verify | rebuilt list] -> model -> gn_neb_finish

``gn_neb_forces`` (one workgroup per image) turns the kept forces f and the kept energies of the last completed step into the
band forces g: with t+ = R_{i+1} - R_i and t- = R_i - R_{i-1}, the tangent t is t+ where the energy rises along the band, t-
where it falls, and the energy-weighted mix of the two at an extremum; an ordinary interior image gets
g = f - (f.t^) t^ + k (|t+| - |t-|) t^, the climbing image -- the interior image with the largest energy -- gets
g = f - 2 (f.t^) t^ and no spring, the end images and fixed atoms get 0.  FIRE's unit is the BAND, as in ASE, where one
optimiser owns all images: ``gn_fire_plan`` and ``gn_fire_move`` run unchanged on g with a band pointer (every ``n_images``-th
entry of the molecule pointer) and a mask that fixes the end images, so dt, alpha, the convergence test against ``fmax`` and
the ``max_step`` clamp are per band.  ``gn_neb_finish`` is ``gn_fire_finish`` with the status read per band: a band whose status
has left 0 freezes, all its images together, while the other bands go on.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import engine
from ._lib import call, ptr
from .pipeline import EnergyForces
from .relax import Relax


def band(z: torch.Tensor, pos_first: torch.Tensor, pos_last: torch.Tensor, batch: torch.Tensor, n_band: int, n_images: int = 7):
    """The straight-line start of ``n_band`` bands -> (z, pos, batch, n_mol) for ``NEB``.  ``z`` [n], ``batch`` [n] (sorted, values
    below ``n_band``) and the two end points ``pos_first`` / ``pos_last`` [n, 3] describe one batch of ``n_band`` molecules; image i
    of every band is pos_first + (i / (n_images - 1)) (pos_last - pos_first), formed in fp64 and rounded to fp32.  The images of
    a band are consecutive molecules; ``z`` and ``batch`` are tiled to match."""
    n_band, n_images = int(n_band), int(n_images)
    if n_images < 3:
        raise ValueError(f"n_images must be >= 3 (two end points and at least one image between them), got {n_images}")
    if pos_first.shape != pos_last.shape or pos_first.dim() != 2 or pos_first.shape[1] != 3 or z.shape[0] != pos_first.shape[0] \
            or batch.shape[0] != pos_first.shape[0]:
        raise ValueError("band: z [n], batch [n], pos_first [n, 3] and pos_last [n, 3] are expected")
    a, b = pos_first.detach().double(), pos_last.detach().double()
    zs, ps, bs = [], [], []
    for m in range(n_band):
        sel = (batch == m).nonzero().flatten()
        for i in range(n_images):
            zs.append(z[sel])
            ps.append((a[sel] + (i / (n_images - 1)) * (b[sel] - a[sel])).float())
            bs.append(torch.full((sel.numel(),), m * n_images + i, dtype=torch.int64, device=batch.device))
    return torch.cat(zs), torch.cat(ps), torch.cat(bs), n_band * n_images


def validate_band(z, batch, n_mol, n_images, k, fixed) -> None:
    """What ``NEB`` refuses on top of ``relax.validate``, before any launch.  Raises ``ValueError``.  Reads ``z``, ``batch`` and
    ``fixed`` on the host."""
    n_mol, n_images = int(n_mol), int(n_images)
    if n_images < 3:
        raise ValueError(f"n_images must be >= 3 (two end points and at least one image between them), got {n_images}")
    if n_mol % n_images != 0:
        raise ValueError(f"n_mol = {n_mol} is not a multiple of n_images = {n_images}")
    if not (math.isfinite(float(k)) and float(k) >= 0):
        raise ValueError(f"k (the spring constant) must be finite and >= 0, got {k}")
    zc, bc = z.detach().cpu().long(), batch.detach().cpu().long()
    count = torch.bincount(bc, minlength=n_mol)[:n_mol].tolist()
    mask = None
    if fixed is not None and torch.is_tensor(fixed) and fixed.dtype in (torch.bool, torch.uint8) and tuple(fixed.shape) == tuple(zc.shape):
        mask = fixed.detach().cpu().bool()           # (anything else is ``relax.validate``'s to refuse)
    for b in range(n_mol // n_images):
        first = b * n_images
        z0 = zc[bc == first]
        f0 = mask[bc == first] if mask is not None else None
        for i in range(1, n_images):
            if count[first + i] != count[first]:
                raise ValueError(f"band {b}: image {i} has {count[first + i]} atoms, image 0 has {count[first]}")
            if not torch.equal(zc[bc == first + i], z0):
                raise ValueError(f"band {b}: the atomic numbers z of image {i} differ from those of image 0")
            if mask is not None and not torch.equal(mask[bc == first + i], f0):
                raise ValueError(f"band {b}: the fixed mask of image {i} differs from that of image 0")


class NEB(Relax):
    """Relax bands of images between fixed end points to minimum-energy paths with ``ef``'s model (``pipeline.EnergyForces``).

        z, pos, batch, n_mol = neb.band(z_ab, pos_first, pos_last, batch_ab, n_band, n_images=7)
        nb = NEB(EnergyForces(rep, head, check_edges=False), z, pos, batch, n_mol, n_images=7, k=0.1, climb=True, fmax=0.05)
        nb.run(500)                     # returns nb; stops early once no band is active
        nb.pos, nb.forces, nb.neb_forces, nb.potential_energy, nb.barrier, nb.climbing_image, nb.fmax, nb.converged, nb.log()

    ``pos`` holds every image of every band, the images of a band as ``n_images`` consecutive molecules with the same atoms in
    the same order (``neb.band`` builds the straight-line start from two end points).  The first and the last image of a band
    never move; relax them beforehand (``Relax``).  ``k``: the spring constant, energy per length^2, the same between all images.
    ``climb``: the interior image with the largest energy of the last completed step (the first of equal ones) climbs -- its
    force along the tangent is reflected and it feels no spring -- from the first step on; which image that is may change from
    step to step.  Everything else is ``Relax``'s, with a BAND where ``Relax`` has a molecule: ``fmax`` -- a band is converged when
    the largest band force |g_a| on a free atom of its interior images is at most this; ``max_step`` bounds the move of the whole
    band; dt and alpha adapt per band; a band whose status has left 0 is frozen, all images together, while the others go on.
    ``fixed`` marks atoms that never move and are left out of the tangent, the projection and the spring lengths; it must be the
    same in every image of a band.  ``rebuild="host"`` (default) and ``rebuild="device"`` work as for ``Relax``.

    ``forces`` / ``potential_energy`` (/ ``stress``) are the model's, per atom / image, of the last completed step; ``neb_forces``
    [N, 3] are the band forces g of that state; ``barrier`` [n_band] is the largest image energy minus the first image's
    (subtracted in fp64); ``climbing_image`` [n_band] is the index of the climbing image in its band (-1 without ``climb``);
    ``fmax``, ``status``, ``converged`` and ``converged_at`` are per band; ``log()`` is [k, n_band, 2]: the band's largest image
    energy and its largest |g_a| BEFORE each move.  ``run`` raises ``RuntimeError`` naming the band when a force or an energy is
    not finite; nothing of that band has moved.

    Periodic runs keep the cell fixed.  Image differences are RAW position differences: this project never wraps positions,
    so the path must be continuous -- an atom that crosses a cell face keeps its unwrapped coordinate in every image.

    Out of scope: IDPP interpolation (the start is the caller's; ``neb.band`` is linear); removal of rotation and translation;
    variable springs; a moving cell; skipping the model on the fixed end images (they are evaluated with the rest of the
    batch in every step).

    Refused with ``ValueError`` before any launch, besides what ``Relax`` refuses: ``n_images`` < 3; ``n_mol`` not a multiple of
    ``n_images``; images of a band that differ in atom count or in ``z``; ``k`` not finite or negative; a ``fixed`` mask that differs
    between images of a band."""

    def __init__(self, ef: EnergyForces, z: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, n_mol: int, n_images: int = 7,
                 k: float = 0.1, climb: bool = False, fmax: float = 0.05, dt: float = 0.1, dt_max: float = 1.0,
                 max_step: float = 0.2, n_min: int = 5, f_inc: float = 1.1, f_dec: float = 0.5, alpha: float = 0.1,
                 f_alpha: float = 0.99, fixed: Optional[torch.Tensor] = None, cell: Optional[torch.Tensor] = None,
                 images: str = "minimum", max_num_neighbors: int = 32, check_every: int = 1, log_len: int = 1024,
                 captured: bool = True):
        validate_band(z, batch, n_mol, n_images, k, fixed)
        self.n_images, self.n_band, self.k, self.climb = int(n_images), int(n_mol) // int(n_images), float(k), bool(climb)
        super().__init__(ef, z, pos, batch, n_mol, fmax=fmax, dt=dt, dt_max=dt_max, max_step=max_step, n_min=n_min, f_inc=f_inc,
                         f_dec=f_dec, alpha=alpha, f_alpha=f_alpha, fixed=fixed, cell=cell, images=images,
                         max_num_neighbors=max_num_neighbors, check_every=check_every, log_len=log_len, captured=captured)

    def _start(self, start):
        """The per-band FIRE buffers (the driver's own, in place of the per-molecule ones), the band pointer and the mask that
        fixes the end images, then ``_ListDriver``'s start: every buffer of the recorded chain is made here, by torch, before the
        recording."""
        dev, nb, ni = start.device, self.n_band, self.n_images
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self._band_ptr = self._mol_ptr[::ni].contiguous()
        image = self._batch % ni
        ends = ((image == 0) | (image == ni - 1)).to(torch.uint8)
        self._fixed_band = (ends if self._fixed is None else (ends | self._fixed)).contiguous()
        self._dt, self._alpha = torch.full((nb,), self.dt, **f32), torch.full((nb,), self.alpha, **f32)
        self._n_pos, self._status = torch.full((nb,), -1, **i32), torch.zeros(nb, **i32)
        self._converged_at = torch.full((nb,), -1, **i32)
        self._coef = torch.zeros((nb, 4), **f32)
        self._log = torch.zeros((self.log_len, nb, 2), **f32)
        self._host_status = [0] * nb
        self._g = torch.zeros((self.N, 3), **f32)                 # the band forces: what plan judges and move follows
        self._e_band, self._climbing = torch.zeros(nb, **f32), torch.full((nb,), -1, **i32)
        self._go = torch.zeros(2, **i32)                          # a state pair that is never set: the queries' launches
        super()._start(start)

    # ---- the pieces of a step: the same launches whether recorded or eager -------------------------------------------
    def _band_forces(self, pos, g, e_band, climbing, state):
        call("gn_neb_forces", ptr(pos), ptr(self._f), ptr(self._e), ptr(self._fixed), ptr(self._mol_ptr), self.N, self.n_mol,
             self.n_images, self.k, int(self.climb), ptr(g), ptr(e_band), ptr(climbing), ptr(state), engine._stream())

    def _pre(self, pos, cell=None):
        """Everything before the neighbour list: the band forces of the kept state, then FIRE's decision and move per band."""
        self._band_forces(pos, self._g, self._e_band, self._climbing, self._state)
        call("gn_fire_plan", ptr(self._g), ptr(self._vel), ptr(self._fixed_band), ptr(self._band_ptr), self.N, self.n_band,
             self.fmax_target, self.dt_max, self.n_min, self.f_inc, self.f_dec, self.alpha, self.f_alpha, ptr(self._dt),
             ptr(self._alpha), ptr(self._n_pos), ptr(self._status), ptr(self._converged_at), ptr(self._coef), ptr(self._e_band),
             ptr(self._log), self.log_len, ptr(self._state), engine._stream())
        call("gn_fire_move", ptr(pos), ptr(self._vel), ptr(self._g), ptr(self._fixed_band), ptr(self._band_ptr), self.N,
             self.n_band, ptr(self._coef), self.max_step, ptr(self._state), engine._stream())

    def _post(self, energy, forces, stress=None):
        call("gn_neb_finish", ptr(self._state), ptr(self._status), ptr(self._batch), ptr(forces), ptr(self._f), self.N,
             ptr(energy), ptr(self._e), ptr(stress), ptr(self._stress), self.n_mol, self.n_images, engine._stream())

    def _looked(self) -> bool:
        """The host's look at the per-band status (one read): a band force that is not finite ends the run with an error, no
        active band ends it early."""
        self._host_status = status = self._status.tolist()
        if 2 in status:
            b = status.index(2)
            raise RuntimeError(f"neb: a force or an energy of band {b} is not finite in step {self._converged_at.tolist()[b]}; "
                               "the band has not moved since")
        return 0 not in status

    # ---- state and queries -------------------------------------------------------------------------------------------
    def _kept(self):
        """(g [N, 3], largest energy [n_band], climbing image [n_band]) of the kept state: what the next step is judged on."""
        g, e_band = torch.empty_like(self._g), torch.empty_like(self._e_band)
        climbing = torch.empty_like(self._climbing)
        self._band_forces(self._pos, g, e_band, climbing, self._go)
        return g, e_band, climbing

    @property
    def neb_forces(self) -> torch.Tensor:
        """[N, 3]: the band forces g of the last completed step (0 on the end images and on fixed atoms)."""
        return self._kept()[0]

    @property
    def barrier(self) -> torch.Tensor:
        """fp64 [n_band]: the largest image energy of the band minus the energy of its first image."""
        return self._kept()[1].double() - self._e[::self.n_images].double()

    @property
    def climbing_image(self) -> torch.Tensor:
        """int32 [n_band]: the index, in its band, of the image that climbs in the next step; -1 without ``climb``."""
        return self._kept()[2]

    @property
    def fmax(self) -> torch.Tensor:
        """[n_band]: the largest band force |g_a| on a free atom (gn_fire_fmax on ``neb_forces``)."""
        g, out = self._kept()[0], torch.empty(self.n_band, dtype=torch.float32, device=self._f.device)
        call("gn_fire_fmax", ptr(g), ptr(self._fixed_band), ptr(self._band_ptr), self.N, self.n_band, ptr(out), engine._stream())
        return out
