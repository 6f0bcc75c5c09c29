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

Not done in ``Relax``: the cell is fixed (no strain degrees of freedom; the stress is only reported), the only constraint is a
mask of fixed atoms, the only optimiser is FIRE.

``CellRelax`` relaxes the cell as well (kernels: csrc/gn_cellrelax.hip), on the device-rebuilt list only.  The formulation is
ASE's ``UnitCellFilter`` for row vectors.  Per box: the reference cell C0 (the start), a deformation gradient F (the identity
at the start) and reference coordinates x~ (the start positions); pos = x~ F and cell = C0 F; the degrees of freedom are the
rows of x~ and three "cell rows" U = w F, w = ``cell_factor``.  With H = E + pressure V, the kept forces f and the kept stress
sigma = (1/V) sum r (x) dE/dr, the generalised forces -dH/d(dof) are::

    atom rows   g_a = f_a F^T                          (dE/dx~_ai = sum_j dE/dpos_aj F_ij)
    cell rows   G   = -(V / w) F^-T S,   S = (sigma + sigma^T) / 2 + pressure I
                (dF strains every vector, r -> r (I + F^-1 dF), so dE = V sigma : F^-1 dF and dV = V tr(F^-1 dF))

``hydrostatic`` replaces S by (tr S / 3) I; ``cell_mask`` then zeroes components of G.  The extended system of a box -- its atom
rows, then its cell rows -- is one "molecule" of n + 3 atoms to gn_fire_plan and gn_fire_move, which run on it unchanged: P,
the norms, the convergence test against ``fmax`` and the ``max_step`` clamp are taken over both kinds of rows together.  One
step::

    gn_cellrelax_forces -> plan -> move (on x~, U) -> gn_cellrelax_apply (pos = x~ F, cell = C0 F)
        -> gn_cell_prepare -> gn_cell_image_ranges -> rebuilt list -> model -> finish

``pipeline.RebuiltStep(cell_moves=True)`` recomputes the image ranges of the moved cell in every step, so nothing is repaired
or recorded anew when they change.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import engine, graph
from ._lib import call, ptr
from .md import _ListDriver, _RebuildOption
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


def validate_cell(rebuild, cell, images, n_mol, pressure, cell_mask, cell_factor) -> None:
    """What ``CellRelax`` refuses on top of ``validate``, before any launch.  Raises ``ValueError``."""
    if rebuild != "device":
        raise ValueError(f'CellRelax runs on the device-rebuilt list only: rebuild="device", got {rebuild!r} (a moved cell on '
                         'the host-rebuilt list would need a guard, a repair and a new recording)')
    if cell is None:
        raise ValueError("CellRelax needs a cell: there is nothing to relax besides the atoms (use Relax)")
    graph.check_periodic_args(cell, images)
    if images == "minimum":
        raise ValueError('CellRelax with images="minimum": whether a moved cell is still at least 2 * cutoff wide is the '
                         'host\'s decision; images="all" (the default) or "auto" recomputes the image ranges on the device')
    if not math.isfinite(float(pressure)):
        raise ValueError(f"pressure must be finite, got {pressure}")
    if cell_mask is not None and (not torch.is_tensor(cell_mask) or cell_mask.dtype not in (torch.bool, torch.uint8)
                                  or tuple(cell_mask.shape) != (3, 3)):
        raise ValueError("cell_mask: a bool or uint8 mask of shape [3, 3] is expected")
    if cell_factor is not None:
        if torch.is_tensor(cell_factor) and cell_factor.numel() != 1:
            if tuple(cell_factor.shape) != (int(n_mol),):
                raise ValueError(f"cell_factor: a positive number or a tensor of shape [{int(n_mol)}] is expected")
            w = cell_factor.detach().double().cpu()
            ok = bool(torch.isfinite(w).all()) and bool((w > 0).all())
        else:
            ok = math.isfinite(float(cell_factor)) and float(cell_factor) > 0
        if not ok:
            raise ValueError(f"cell_factor must be positive and finite, got {cell_factor}")


class _DeviceRebuild(_RebuildOption):
    """``_RebuildOption`` for a driver that exists in device mode only: ``rebuild="device"`` is the default of its constructor
    call (another value is the driver's to refuse)."""

    def __call__(cls, *args, rebuild: str = "device", **kw):
        return super().__call__(*args, rebuild=rebuild, **kw)


class CellRelax(Relax, metaclass=_DeviceRebuild):
    """Relax the atoms AND the cell of every periodic box of a batch: ``Relax``'s FIRE over the extended system of the module
    docstring (the atoms' reference coordinates plus the nine components of a per-box deformation gradient), one graph replay
    per step on the device-rebuilt list.

        rx = CellRelax(EnergyForces(rep, head, check_edges=False), z, pos, batch, n_mol, cell=cell, fmax=0.05, pressure=0.0)
        rx.run(500)
        rx.pos, rx.cell, rx.volume, rx.deformation, rx.stress, rx.cell_forces, rx.enthalpy, rx.fmax, rx.converged

    Everything of ``Relax`` holds, with these differences.  ``cell`` is required and ``images`` is "all" (default) or "auto".
    ``rebuild`` is "device" (default; the only mode).  ``fmax`` and ``max_step`` act on the extended system: a box is converged
    when the largest generalised force on a free atom row or a cell row is at most ``fmax``, and ``max_step`` bounds the norm of
    the move of all rows together.  ``pressure``: the external pressure of H = E + pressure V, in the model's energy unit per
    length^3.  ``hydrostatic``: only the volume changes (cell = s C0).  ``cell_mask``: bool or uint8 [3, 3], the components of
    the generalised cell force that are kept (default: all); a masked component of the deformation gradient never changes.
    ``cell_factor``: the weight w of the cell rows U = w F, a positive number or a tensor [n_mol] (default: the box's atom
    count, at least 1): it balances the cell's step against the atoms'.  A ``fixed`` atom keeps its reference coordinates, so
    it follows the cell affinely.

    ``vel`` / ``cell_vel``: FIRE's velocities of the atom rows [N, 3] and the cell rows [n_mol, 3, 3].  ``forces`` stay the real
    forces, ``cell_forces`` [n_mol, 3, 3] are the G of the kept state, ``fmax`` is taken over the extended rows, ``enthalpy`` is
    E + pressure V.  A box whose status has left 0 is frozen: its positions, cell, velocities and kept values stay as they are.

    ``run`` raises, besides what ``Relax.run`` raises, when a cell has been driven to where gn_cell_image_ranges refuses it
    (no volume, or a width a little below cutoff / 3): ``graph.image_ranges``' own ``ValueError`` on the reported cell; the
    kept values are those of the last completed step.

    Refused with ``ValueError`` before any launch, besides what ``Relax`` refuses: ``rebuild="host"``; no ``cell``;
    ``images="minimum"``; a ``pressure`` that is not finite; ``cell_factor`` <= 0; a ``cell_mask`` of the wrong shape or dtype."""

    _cell_moves = True

    def __init__(self, ef: EnergyForces, z: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, n_mol: int, fmax: float = 0.05,
                 dt: float = 0.1, dt_max: float = 1.0, max_step: float = 0.2, n_min: int = 5, f_inc: float = 1.1,
                 f_dec: float = 0.5, alpha: float = 0.1, f_alpha: float = 0.99, fixed: Optional[torch.Tensor] = None,
                 cell: Optional[torch.Tensor] = None, images: str = "all", max_num_neighbors: int = 32,
                 check_every: int = 1, log_len: int = 1024, captured: bool = True, pressure: float = 0.0,
                 hydrostatic: bool = False, cell_mask: Optional[torch.Tensor] = None, cell_factor=None):
        validate_cell(self.rebuild, cell, images, n_mol, pressure, cell_mask, cell_factor)
        self.pressure, self.hydrostatic = float(pressure), bool(hydrostatic)
        self._cell_args = (cell_mask, cell_factor)
        super().__init__(ef, z, pos, batch, n_mol, fmax=fmax, dt=dt, dt_max=dt_max, max_step=max_step, n_min=n_min, f_inc=f_inc,
                         f_dec=f_dec, alpha=alpha, f_alpha=f_alpha, fixed=fixed, cell=cell, images=images,
                         max_num_neighbors=max_num_neighbors, check_every=check_every, log_len=log_len, captured=captured)

    def _start(self, start):
        """The extended system at ``start`` (x~ = start, F = 1, C0 = the cell), then ``_ListDriver``'s start: every buffer of the
        recorded chain is made here, by torch, before the recording."""
        dev, n, N = start.device, self.n_mol, self.N
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        mask, factor = self._cell_args
        count = (self._mol_ptr[1:] - self._mol_ptr[:-1]).to(**f32)
        if factor is None:
            self._w = count.clamp_min(1.0)
        elif torch.is_tensor(factor) and factor.numel() != 1:
            self._w = factor.detach().to(**f32).contiguous()
        else:
            self._w = torch.full((n,), float(factor), **f32)
        self._mask = None if mask is None else mask.to(device=dev, dtype=torch.uint8).reshape(9).contiguous()
        self.NE = N + 3 * n
        self._mol_ptr_ext = (self._mol_ptr + 3 * torch.arange(n + 1, **i32)).to(torch.int32).contiguous()
        self._atom_rows = torch.arange(N, device=dev) + 3 * self._batch
        self._cell_rows = ((self._mol_ptr[1:].long() + 3 * torch.arange(n, device=dev)).unsqueeze(1)
                           + torch.arange(3, device=dev).unsqueeze(0))
        self._x_ext, self._vel_ext = torch.zeros((self.NE, 3), **f32), torch.zeros((self.NE, 3), **f32)
        self._g_ext = torch.zeros((self.NE, 3), **f32)
        self._x_ext[self._atom_rows] = start
        self._x_ext[self._cell_rows] = self._w.reshape(n, 1, 1) * torch.eye(3, **f32)
        self._fixed_ext = None
        if self._fixed is not None:                               # (the cell rows are free)
            self._fixed_ext = torch.zeros(self.NE, dtype=torch.uint8, device=dev)
            self._fixed_ext[self._atom_rows] = self._fixed
        self._cell0 = self._cell.contiguous().clone()             # (C0: the driver's cell becomes the step's moving buffer)
        self._reason = torch.zeros(n, **i32)                      # why a box set the sticky word: 1 gn_cell_image_ranges
        self._go = torch.zeros(2, **i32)                          # a state pair that is never set: the queries' launches
        super()._start(start)

    # ---- the pieces of a step ----------------------------------------------------------------------------------------
    def _generalised(self, cell, out, state):
        call("gn_cellrelax_forces", ptr(self._f), ptr(self._stress), ptr(cell), ptr(self._x_ext), ptr(self._w), self.pressure,
             int(self.hydrostatic), ptr(self._mask), ptr(self._fixed), ptr(self._mol_ptr), self.N, self.n_mol, ptr(out),
             ptr(state), engine._stream())

    def _pre(self, pos, cell=None):
        """Everything before the neighbour list: the generalised forces of the kept state, FIRE's decision and move on the
        extended system, then positions and cell of the moved boxes into the buffers the step reads."""
        self._generalised(cell, self._g_ext, self._state)
        call("gn_fire_plan", ptr(self._g_ext), ptr(self._vel_ext), ptr(self._fixed_ext), ptr(self._mol_ptr_ext), self.NE,
             self.n_mol, self.fmax_target, self.dt_max, self.n_min, self.f_inc, self.f_dec, self.alpha, self.f_alpha,
             ptr(self._dt), ptr(self._alpha), ptr(self._n_pos), ptr(self._status), ptr(self._converged_at), ptr(self._coef),
             ptr(self._e), ptr(self._log), self.log_len, ptr(self._state), engine._stream())
        call("gn_fire_move", ptr(self._x_ext), ptr(self._vel_ext), ptr(self._g_ext), ptr(self._fixed_ext),
             ptr(self._mol_ptr_ext), self.NE, self.n_mol, ptr(self._coef), self.max_step, ptr(self._state), engine._stream())
        call("gn_cellrelax_apply", ptr(self._x_ext), ptr(self._cell0), ptr(self._w), ptr(self._coef), ptr(self._mol_ptr), self.N,
             self.n_mol, ptr(pos), ptr(cell), ptr(self._state), engine._stream())

    def _guarded(self):
        """The sticky word is set: was it gn_cell_image_ranges?  Then what ``graph.image_ranges`` raises on the reported cell."""
        reason = self._reason.tolist()
        if 1 in reason:
            graph.image_ranges(self._cell, self.cutoff)
            raise RuntimeError(f"cell relaxation: the device refused the image ranges of box {reason.index(1)} in step "
                               f"{self._done + 1}, but graph.image_ranges accepts the reported cell; the run stops at step "
                               f"{self._done}")

    # ---- state and queries -------------------------------------------------------------------------------------------
    def _kept_g(self) -> torch.Tensor:
        """[N + 3 n_mol, 3]: the generalised forces of the kept state (what the next step is judged on)."""
        out = torch.empty_like(self._g_ext)
        self._generalised(self._cell, out, self._go)
        return out

    @property
    def vel(self) -> torch.Tensor:
        """[N, 3]: FIRE's velocities of the atom rows (of the reference coordinates)."""
        return self._vel_ext[self._atom_rows]

    @property
    def cell_vel(self) -> torch.Tensor:
        """[n_mol, 3, 3]: FIRE's velocities of the cell rows."""
        return self._vel_ext[self._cell_rows]

    @property
    def cell(self) -> torch.Tensor:
        """[n_mol, 3, 3]: the current cell, C0 F."""
        return self._cell.clone()

    @property
    def volume(self) -> torch.Tensor:
        """[n_mol]: |det cell| (gn_cell_prepare's)."""
        return graph.cell_prepare(self._cell)[1]

    @property
    def deformation(self) -> torch.Tensor:
        """[n_mol, 3, 3]: the deformation gradient F (cell rows / ``cell_factor``, divided in fp64)."""
        return (self._x_ext[self._cell_rows].double() / self._w.double().reshape(-1, 1, 1)).float()

    @property
    def cell_forces(self) -> torch.Tensor:
        """[n_mol, 3, 3]: the generalised forces G on the cell rows, of the kept state."""
        return self._kept_g()[self._cell_rows]

    @property
    def enthalpy(self) -> torch.Tensor:
        """[n_mol]: E + pressure V of the last completed step."""
        return (self._e.double() + self.pressure * self.volume.double()).float()

    @property
    def fmax(self) -> torch.Tensor:
        """[n_mol]: the largest generalised force on a free atom row or a cell row (gn_fire_fmax over the extended rows)."""
        g, out = self._kept_g(), torch.empty(self.n_mol, dtype=torch.float32, device=self._f.device)
        call("gn_fire_fmax", ptr(g), ptr(self._fixed_ext), ptr(self._mol_ptr_ext), self.NE, self.n_mol, ptr(out), engine._stream())
        return out
