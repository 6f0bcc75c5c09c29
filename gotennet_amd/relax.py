"""Structure relaxation on the fused energy + force step: FIRE (Bitzek et al., PRL 97, 170201, in the variant ASE's ``FIRE``
implements) with PER-MOLECULE state on the device, updated inside the replayed step (kernels: csrc/gn_fire.hip).

One step, in both modes of ``Relax``::

    plan (kept forces, velocities) -> move -> neighbour list -> model -> finish

``plan`` (gn_fire_plan, one workgroup per molecule) judges every molecule on the forces of the last completed step: converged
when the largest force on a free atom is at most ``fmax`` (status 1), stopped when a force is not finite (status 2), else it
takes FIRE's decision from P = sum f.v -- downhill: mix the velocity towards the force and, after ``n_min`` such steps, grow
``dt`` and shrink ``alpha``; uphill: zero the velocity, halve ``dt``, reset ``alpha`` -- and leaves the coefficients of the move.
``move`` (gn_fire_move) is v <- c_v v + c_f f + dt f, dr = dt v, clamped to ``max_step`` over the whole molecule, pos += dr.
``finish`` (gn_fire_finish) advances the step counter and keeps the new forces, energies and stress of the molecules that
are still active.  A molecule whose status has left 0 is frozen: it never moves again and keeps the values it was judged
on, while the other molecules of the batch go on; each adapts ``dt`` and ``alpha`` on its own.

The driver is ``md.MDRun``'s: ``captured=True`` records the chain around ``CapturedStep``'s body into one hipGraph on a fixed
edge list with "neighbour list" = gn_radius_verify*; a stale list sets the sticky device word, every kernel here is
predicated on it, the host looks every ``check_every`` replays, rebuilds the list at the frozen state (after the move of the
first incomplete step), records anew and finishes that step eagerly.  ``captured=False`` launches the same kernels eagerly
with the list rebuilt by ``graph.distance*`` in every step; the two agree bit for bit.

Not done here: the cell is fixed (no strain degrees of freedom; the stress is only reported), the only constraint is a mask of
fixed atoms, the only optimiser is FIRE.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import engine, graph
from ._lib import call, ptr
from .md import _ListDriver
from .pipeline import EnergyForces


def validate(pos, N, fmax, dt, dt_max, max_step, n_min, f_inc, f_dec, alpha, f_alpha, fixed, cell, cutoff, images="minimum",
             check_every=1, log_len=1):
    """Everything ``Relax`` refuses, before any launch -> ``graph.resolve_images``' result or None.  Raises ``ValueError``."""
    if not (float(fmax) >= 0):
        raise ValueError(f"fmax must be >= 0, got {fmax}")
    for name, v in (("dt", dt), ("dt_max", dt_max), ("max_step", max_step)):
        if not (math.isfinite(float(v)) and float(v) > 0):
            raise ValueError(f"{name} must be positive and finite, got {v}")
    if float(dt) > float(dt_max):
        raise ValueError(f"dt = {dt} exceeds dt_max = {dt_max}")
    if not (math.isfinite(float(f_inc)) and float(f_inc) >= 1):
        raise ValueError(f"f_inc must be finite and >= 1, got {f_inc}")
    for name, v in (("f_dec", f_dec), ("f_alpha", f_alpha)):
        if not 0 < float(v) < 1:
            raise ValueError(f"{name} must lie in (0, 1), got {v}")
    if not 0 < float(alpha) <= 1:
        raise ValueError(f"alpha must lie in (0, 1], got {alpha}")
    if int(n_min) < 0:
        raise ValueError(f"n_min must be >= 0, got {n_min}")
    if int(check_every) < 1 or int(log_len) < 0:
        raise ValueError("check_every must be >= 1 and log_len >= 0")
    if fixed is not None and (not torch.is_tensor(fixed) or fixed.dtype not in (torch.bool, torch.uint8)
                              or tuple(fixed.shape) != (N,)):
        raise ValueError(f"fixed: a bool or uint8 mask of shape [{N}] is expected")
    if pos.requires_grad:
        raise ValueError("pos requires grad: the driver moves plain tensors")
    graph.check_periodic_args(cell, images)
    return graph.resolve_images(cell, float(cutoff), images) if cell is not None else None


class Relax(_ListDriver):
    """Relax the molecules (or periodic boxes) of a batch with ``ef``'s model (``pipeline.EnergyForces``) from ``pos``.

        rx = Relax(EnergyForces(rep, head, check_edges=False), z, pos, batch, n_mol, fmax=0.05)
        rx.run(500)                     # returns rx; stops early once no molecule is active
        rx.pos, rx.forces, rx.potential_energy, rx.fmax, rx.converged, rx.converged_at, rx.step, rx.rebuilds, rx.log()
        rx.stress                       # periodic runs: reported, the cell is fixed

    The defaults are ASE's and fit eV and Angstrom.  Masses are 1, so ``dt`` is no physical time: a step from rest moves an
    atom by dr = dt^2 f (v = dt f, dr = dt v).  ``fmax``: a molecule is converged when the largest force on one of its free atoms
    is at most this.  ``dt`` / ``dt_max``: the first and the largest time step;  ``max_step``: the longest displacement of a
    whole molecule in one step (the norm over all its atoms, as in ASE);  ``n_min``: downhill steps before ``dt`` grows;
    ``f_inc`` / ``f_dec``: the factors of ``dt``;  ``alpha`` / ``f_alpha``: the mixing coefficient at a (re)start and its factor.
    ``fixed``: a bool or uint8 mask [N] of atoms that never move and whose forces count as zero.  ``cell`` / ``images`` /
    ``max_num_neighbors``: as ``graph.distance_pbc``; the cell is fixed.  ``check_every``: replays between two host reads of the
    device state (the trajectory does not depend on it; replays after the last molecule has converged move nothing and are
    not counted).  ``log_len``: rows of the (energy, largest force) ring, one row per step, written BEFORE the step's move.
    ``captured=False``: the eager reference (module docstring).  ``rebuild`` (a keyword of the constructor call,
    ``Relax(..., rebuild="device")``, as for ``md.MDRun``): "host" (default) or "device": the
    list is rebuilt inside every step on the device (``pipeline.RebuiltStep``), nothing is verified or re-recorded and
    ``rebuilds`` stays 0 -- for relaxations whose list changes in most steps.

    ``run`` raises ``RuntimeError`` naming the molecule when a force is not finite; nothing of that molecule has moved.
    ``vel`` are FIRE's velocities (unit masses).  ``forces``, ``potential_energy`` and ``stress`` are those of the last completed
    step; of a frozen molecule, the values it was judged on.  The stress is reported only: the cell is fixed.

    Refused with ``ValueError`` before any launch: fmax < 0; dt, dt_max or max_step not positive and finite; dt > dt_max;
    f_inc < 1; f_dec or f_alpha outside (0, 1); alpha outside (0, 1]; n_min < 0; ``fixed`` of the wrong shape or dtype; ``pos`` or
    ``cell`` requiring grad; a cell that ``graph.resolve_images`` refuses; an unknown ``rebuild``."""

    def __init__(self, ef: EnergyForces, z: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, n_mol: int, fmax: float = 0.05,
                 dt: float = 0.1, dt_max: float = 1.0, max_step: float = 0.2, n_min: int = 5, f_inc: float = 1.1,
                 f_dec: float = 0.5, alpha: float = 0.1, f_alpha: float = 0.99, fixed: Optional[torch.Tensor] = None,
                 cell: Optional[torch.Tensor] = None, images: str = "minimum", max_num_neighbors: int = 32,
                 check_every: int = 1, log_len: int = 1024, captured: bool = True):
        ranges = validate(pos, pos.shape[0], fmax, dt, dt_max, max_step, n_min, f_inc, f_dec, alpha, f_alpha, fixed, cell,
                          float(ef.rep.cutoff), images, check_every, log_len)
        dev = pos.device
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self._setup(ef, z, pos, batch, n_mol, cell, ranges, images, max_num_neighbors, check_every, captured, log_len)
        self.fmax_target, self.dt, self.dt_max, self.max_step = float(fmax), float(dt), float(dt_max), float(max_step)
        self.n_min, self.f_inc, self.f_dec, self.alpha, self.f_alpha = int(n_min), float(f_inc), float(f_dec), float(alpha), float(f_alpha)
        self._fixed = None if fixed is None else fixed.to(device=dev, dtype=torch.uint8).contiguous()
        # every buffer of the recorded chain is initialised here (or in ``_setup``), by torch, never inside the recording
        self._dt, self._alpha = torch.full((self.n_mol,), self.dt, **f32), torch.full((self.n_mol,), self.alpha, **f32)
        self._n_pos, self._status = torch.full((self.n_mol,), -1, **i32), torch.zeros(self.n_mol, **i32)
        self._converged_at = torch.full((self.n_mol,), -1, **i32)
        self._coef = torch.zeros((self.n_mol, 4), **f32)
        self._host_status = [0] * self.n_mol                      # as of the host's last look
        self._start(pos.detach().to(**f32).contiguous())          # (the kept forces: what plan judges)

    # ---- the pieces of a step: the same launches whether recorded or eager -----------------------------------------
    def _pre(self, pos, cell=None):
        """Everything before the neighbour list.  ``pos``: the buffer the step reads (a recording passes its own)."""
        call("gn_fire_plan", ptr(self._f), ptr(self._vel), ptr(self._fixed), ptr(self._mol_ptr), self.N, self.n_mol,
             self.fmax_target, self.dt_max, self.n_min, self.f_inc, self.f_dec, self.alpha, self.f_alpha, ptr(self._dt),
             ptr(self._alpha), ptr(self._n_pos), ptr(self._status), ptr(self._converged_at), ptr(self._coef), ptr(self._e),
             ptr(self._log), self.log_len, ptr(self._state), engine._stream())
        call("gn_fire_move", ptr(pos), ptr(self._vel), ptr(self._f), ptr(self._fixed), ptr(self._mol_ptr), self.N, self.n_mol,
             ptr(self._coef), self.max_step, ptr(self._state), engine._stream())

    def _post(self, energy, forces, stress=None):
        call("gn_fire_finish", ptr(self._state), ptr(self._status), ptr(self._batch), ptr(forces), ptr(self._f), self.N,
             ptr(energy), ptr(self._e), ptr(stress), ptr(self._stress), self.n_mol, engine._stream())

    def _looked(self) -> bool:
        """The host's look at the per-molecule status (one read): a force that is not finite ends the run with an error, no
        active molecule ends it early."""
        self._host_status = status = self._status.tolist()
        if 2 in status:
            m = status.index(2)
            raise RuntimeError(f"relax: a force on molecule {m} is not finite in step {self._converged_at.tolist()[m]}; the "
                               "molecule has not moved since")
        return 0 not in status

    def run(self, n: int) -> "Relax":
        """Up to ``n`` more steps; stops early once no molecule is active (and does nothing when none is)."""
        if 0 not in self._host_status:
            return self
        return super().run(n)

    # ---- state and queries -----------------------------------------------------------------------------------------
    # (``pos``, ``vel``, ``potential_energy`` and ``stress`` are ``_ListDriver``'s)
    @property
    def forces(self) -> torch.Tensor:
        """[N, 3]: of the last completed step; of a frozen molecule, the forces it was judged on."""
        return self._f.clone()

    @property
    def fmax(self) -> torch.Tensor:
        """[n_mol]: the largest force on a free atom, from ``forces`` (gn_fire_fmax: what the next step is judged on)."""
        out = torch.empty(self.n_mol, dtype=torch.float32, device=self._f.device)
        call("gn_fire_fmax", ptr(self._f), ptr(self._fixed), ptr(self._mol_ptr), self.N, self.n_mol, ptr(out), engine._stream())
        return out

    @property
    def status(self) -> torch.Tensor:
        """int32 [n_mol]: 0 active, 1 converged, 2 a force that is not finite."""
        return self._status.clone()

    @property
    def converged(self) -> torch.Tensor:
        """bool [n_mol]."""
        return self._status == 1

    @property
    def converged_at(self) -> torch.Tensor:
        """int32 [n_mol]: the number of steps a molecule had taken when it was found converged; -1 while it is active."""
        return self._converged_at.clone()

    @property
    def step(self) -> int:
        """Completed steps; once every molecule is done, the step at which the last one was: idle replays between that and the
        host's look moved nothing and are not counted."""
        if 0 in self._host_status:
            return self._done
        return min(self._done, max(self._converged_at.tolist(), default=0))

    def log(self) -> torch.Tensor:
        """[k, n_mol, 2]: (energy, largest force) BEFORE the move of each of the last k = min(step, log_len) steps, oldest first."""
        return self._ring(self._log)
