"""Molecular dynamics on the fused energy + force step: velocity Verlet, an optional Langevin thermostat, an optional
barostat, and a neighbour list that is CHECKED on the device inside every replayed step (kernels: csrc/gn_md.hip,
gn_radius_verify* in csrc/gn_graph.hip).

One step, in both modes of ``MDRun`` (in brackets: with a thermostat; in braces: with a barostat)::

    kick (previous forces) -> [Langevin half] -> drift -> [Langevin half] -> {barostat -> rescale -> cell inverse -> cell guard}
        -> neighbour list -> model -> kick -> kinetic -> {pressure} -> finish

``captured=True`` records that chain around ``CapturedStep``'s body into ONE hipGraph on a fixed edge list, with "neighbour
list" = gn_radius_verify*: the search's own predicates, in the search's order, compared with the stored rows.  A row that
differs sets a sticky device word; every integrator kernel is predicated on that word, so a replay on a stale list
advances nothing.  The host reads the word every ``check_every`` steps; when it is set it rebuilds the list at the frozen
positions, records a new graph, finishes the interrupted step eagerly with the same kernels, clears the word and goes on.
``captured=False`` is the same kernel sequence launched eagerly with the list rebuilt by ``graph.distance*`` in every step: the
reference of the captured mode -- the two trajectories agree bit for bit -- and the better choice for systems whose list
changes in almost every step.

``rebuild="device"`` (opt-in; ``rebuild="host"``, the default, is the paragraph above) replaces "neighbour list" by the REBUILD of
the list inside the step: the search's own count and fill kernels around a device scan, into a list of fixed capacity whose
unused tail belongs to dummy atoms (``pipeline.RebuiltStep``, ``graph.PaddedLayout``).  The list is never stale, so there is no
verify kernel, no repair and no second recording; the sticky word is set only by the overflow guard of gn_padded_tail, and the
host reads the state every ``check_every`` replays for the step counter.  ``captured=False`` launches the same chain eagerly on
the same padded buffers.  With a barostat the step is ``RebuiltStep(cell_moves=True)`` (``images`` "all" or "auto"; "minimum" is
refused): the braces above read {barostat -> rescale -> cell inverse}, the driver's own inverse and volume by a gn_cell_prepare
launch of its own, and the rebuilt list starts gn_cell_prepare -> gn_cell_image_ranges -> count, so the ranges of the search are
those of the moved cell in every step and nothing is re-recorded when they change.  gn_cell_image_ranges takes the guard's
place: a cell without volume or narrower than its bound (R > 3, a little below ``cutoff / 3``) stores reason 1 and the sticky
word, and ``run`` raises what ``graph.image_ranges`` raises on the reported cell.

Constant pressure (``barostat=``): isotropic stochastic cell rescaling (Bernetti and Bussi, J. Chem. Phys. 153, 114107, 2020)
written in eps = ln V.  Per box and step::

    P_int = 2 K / (3 V) - tr(sigma) / 3        sigma = (1/V) dE/d(strain), the stress of ``EnergyForces(cell=)`` (tensile positive)
    d_eps = -(beta_T / tau) (P0 - P_int) dt + sqrt(2 kT beta_T dt / (V tau)) xi
    s     = exp(d_eps / 3):   cell <- s cell,   pos <- s pos,   vel <- vel / s

xi is a standard normal, a pure function of (key, step, box): ``gn_md_noise(key, step, 2, n_mol)[:, 0]``.  The barostat moves
the cell BEFORE the model runs, so forces, energy and stress at the end of a step belong to the (pos, cell) the driver
reports; the pressure that drives a move is the kept one of the last completed step and so lags the move by one drift.  This
is a first-order splitting, nothing more is claimed.  The move is formed by gn_npt_barostat from (kept pressure, volume, step
counter, key) alone -- nothing the kick, the O steps or the drift touch -- so that kernel is launched at the head of the step:
the trajectory is, bit for bit, that of the placement above, and a move larger than ``max_step`` (or a non-finite one) sets
the sticky word before any atom has moved, leaves every cell as it is and stops the run with positions, velocities and cell
of the last completed step (``RuntimeError``).  gn_npt_rescale, gn_cell_prepare and gn_npt_cell_guard follow the drift.

The guard: the search parameters of a run (minimum image, or the image ranges of ``graph.image_ranges``) are conditions on
the cell's perpendicular widths.  gn_npt_cell_guard checks the moved cell against the parameters IN USE on the device and
sets the sticky word (reason 1) when they no longer hold; the rest of that replay, and every later one, advances nothing.  The
host then runs ``graph.resolve_images`` on the current cell -- ``images="minimum"`` raises ``check_cell``'s ``ValueError``,
"auto" / "all" give new ranges or raise below cutoff / 3 -- and repairs as for a stale list: new list at the frozen state
(after the drift and the cell move of the first incomplete step), new recording, the rest of the step eagerly.  The eager
mode launches the same guard and changes its ranges only when it fires, so both modes decide from the same bits.  Ranges
larger than a grown cell needs cost candidates, never edges.
"""
from __future__ import annotations

import math
import weakref
from typing import Optional

import torch

from . import engine, graph
from ._lib import call, ptr
from .outputs import _ATOMIC_MASS, molecule_ptr
from .pipeline import CapturedStep, EnergyForces, RebuiltStep, energy_forces

#: ``force_scale`` turns force / mass into an acceleration in the caller's length and time units:
#: a = force_scale * F / m.  1 when the units are consistent already (the default).  Two common sets, masses in amu,
#: lengths in Angstrom, times in fs:  forces in eV / Angstrom: 1 eV / (amu Angstrom^2) = 9.648533212e-3 fs^-2 (the Faraday
#: constant, 96485.33212 C / mol, times 1e-7);  forces in kcal / (mol Angstrom): 4184 J / mol over 1e-3 kg / mol =
#: 4.184e6 m^2 / s^2 = 4.184e-4 Angstrom^2 / fs^2.  The thermostat's ``kT`` is in the model's energy unit.
EV_ANGSTROM_AMU_FS = 9.648533212e-3
KCAL_MOL_ANGSTROM_AMU_FS = 4.184e-4
#: The barostat's ``pressure`` (and 1 / ``compressibility``) is in the model's energy unit per length^3.  1 bar = 1e5 J / m^3;
#: in eV / Angstrom^3: 1e5 / 1.602176634e-19 (J per eV) * 1e-30 (m^3 per Angstrom^3) = 6.241509074e-7;  in
#: kcal / (mol Angstrom^3): 1e5 * 6.02214076e23 (per mol) / 4184 (J per kcal) * 1e-30 = 1.439325e-5.
BAR_EV_ANGSTROM3 = 1e5 / 1.602176634e-19 * 1e-30
BAR_KCAL_MOL_ANGSTROM3 = 1e5 * 6.02214076e23 / 4184.0 * 1e-30


def default_masses() -> torch.Tensor:
    """The built-in table of standard atomic weights by atomic number (Z <= 36; index 0 is the dummy element, weight 1): the
    one ``ElectronicSpatialExtentV2`` uses."""
    return torch.tensor(_ATOMIC_MASS, dtype=torch.float32)


def langevin_coefficients(kT: float, gamma: float, h: float, force_scale: float = 1.0):
    """(c1, c2) of the O step v = c1 v + c2 xi / sqrt(m) over a time h, in fp64: c1 = exp(-gamma h),
    c2 = sqrt(kT force_scale (1 - c1^2))."""
    c1 = math.exp(-float(gamma) * float(h))
    return c1, math.sqrt(float(kT) * float(force_scale) * (1.0 - c1 * c1))


_BAROSTAT_KEYS = ("pressure", "tau", "compressibility", "kT", "key", "max_step")


def barostat_parameters(barostat: dict, thermostat: Optional[dict], cell) -> dict:
    """``MDRun(barostat=)`` with its defaults filled in (kT and key from the thermostat, max_step 0.05), or ``ValueError``."""
    if cell is None:
        raise ValueError("barostat: a constant-pressure run needs a cell")
    unknown = set(barostat) - set(_BAROSTAT_KEYS)
    if unknown:
        raise ValueError(f"barostat: unknown entries {sorted(unknown)}; known: {list(_BAROSTAT_KEYS)}")
    missing = {"pressure", "tau", "compressibility"} - set(barostat)
    if missing:
        raise ValueError(f"barostat needs pressure, tau and compressibility; missing {sorted(missing)}")
    out = dict(pressure=float(barostat["pressure"]), tau=float(barostat["tau"]),
               compressibility=float(barostat["compressibility"]), max_step=float(barostat.get("max_step", 0.05)))
    for name in ("tau", "compressibility", "max_step"):
        if not (math.isfinite(out[name]) and out[name] > 0):
            raise ValueError(f"barostat: {name} must be positive and finite, got {out[name]}")
    if not math.isfinite(out["pressure"]):
        raise ValueError(f"barostat: pressure must be finite, got {out['pressure']}")
    kT = barostat.get("kT")
    if kT is None:
        if thermostat is None:
            raise ValueError("barostat: kT is required when there is no thermostat (0: the deterministic weak-coupling limit)")
        kT = thermostat["kT"]
    kT = float(kT)
    if not math.isfinite(kT) or kT < 0:
        raise ValueError(f"barostat: kT must be finite and >= 0, got {kT}")
    key = barostat.get("key")
    if key is None and thermostat is not None:
        key = thermostat["key"]
    if kT > 0 and key is None:
        raise ValueError("barostat: kT > 0 draws noise and needs a key (there is no thermostat to take it from)")
    out.update(kT=kT, key=key)
    return out


REBUILD_MODES = ("host", "device")


def check_rebuild(rebuild, barostat=None, images="minimum") -> None:
    """``rebuild=`` of ``MDRun`` / ``relax.Relax``, or ``ValueError``: a known mode, and in device mode no barostat with
    ``images="minimum"`` (the multi-image search recomputes its ranges on the device; whether a moved cell is still a
    minimum-image cell is a host decision)."""
    if rebuild not in REBUILD_MODES:
        raise ValueError(f"rebuild must be one of {REBUILD_MODES}, got {rebuild!r}")
    if rebuild == "device" and barostat is not None and images == "minimum":
        raise ValueError('rebuild="device" with a barostat and images="minimum": a cell that shrinks below 2 * cutoff is the '
                         'host\'s decision; images="all" (or "auto") runs on the device, its image ranges recomputed in every '
                         'step, or use rebuild="host"')


def validate(z, pos, dt, masses, force_scale, thermostat, cell, cutoff, images="minimum", check_every=1, log_len=1,
             rebuild="host", barostat=None):
    """Everything ``MDRun`` refuses, before any launch -> (mass table fp32 on the CPU, ``graph.resolve_images``' result or None).
    Raises ``ValueError``.  Reads ``z`` (and ``cell``) on the host."""
    check_rebuild(rebuild, barostat, images)
    if not (math.isfinite(float(dt)) and float(dt) > 0):
        raise ValueError(f"dt must be positive and finite, got {dt}")
    if not (math.isfinite(float(force_scale)) and float(force_scale) > 0):
        raise ValueError(f"force_scale must be positive and finite, got {force_scale}")
    if int(check_every) < 1 or int(log_len) < 0:
        raise ValueError("check_every must be >= 1 and log_len >= 0")
    table = default_masses() if masses is None else torch.as_tensor(masses).detach().cpu().to(torch.float32).flatten()
    if table.numel() == 0 or not bool(torch.isfinite(table).all()) or bool((table < 0).any()):
        raise ValueError("masses: a table of finite, positive masses indexed by atomic number is expected (0 marks an "
                         "element without a mass)")
    zc = z.detach().cpu().long()
    if zc.numel() and (int(zc.min()) < 0 or int(zc.max()) >= table.numel() or bool((table[zc] <= 0).any())):
        raise ValueError(f"an atomic number has no positive mass in the table ({table.numel()} entries; the built-in one "
                         "covers Z <= 36): pass masses=")
    if thermostat is not None:
        missing = {"kT", "gamma", "key"} - set(thermostat)
        if missing:
            raise ValueError(f"thermostat needs kT, gamma and key; missing {sorted(missing)}")
        kT, gamma = float(thermostat["kT"]), float(thermostat["gamma"])
        if not (math.isfinite(kT) and math.isfinite(gamma)) or kT < 0 or gamma < 0:
            raise ValueError(f"thermostat: kT and gamma must be finite and >= 0, got kT={kT}, gamma={gamma}")
    if barostat is not None:
        barostat_parameters(barostat, thermostat, cell)
    if pos.requires_grad:
        raise ValueError("pos requires grad: the driver integrates plain tensors")
    graph.check_periodic_args(cell, images)
    ranges = graph.resolve_images(cell, float(cutoff), images) if cell is not None else None
    return table, ranges


def _key_words(key) -> list:
    """The thermostat's key as two signed int64 words (an int: {key, 0}; a pair: both)."""
    words = list(key) if isinstance(key, (tuple, list)) else [key, 0]
    if len(words) != 2:
        raise ValueError("thermostat key: an int or a pair of ints")
    words = [int(w) & (2 ** 64 - 1) for w in words]
    return [w - 2 ** 64 if w >= 2 ** 63 else w for w in words]


class _RecordedStep(CapturedStep):
    """``CapturedStep`` with the integrator recorded around its body.  The body is run for warm-up while it is recorded: the
    driver holds the sticky word set during construction, which makes every integrator kernel a no-op.

    The driver is held weakly: driver -> step -> driver would be a reference cycle, and a recorded hipGraph that only the
    cyclic garbage collector frees may be destroyed in the middle of a later stream capture, which the runtime refuses.  This
    way the step dies with its driver, or when the driver drops it."""

    def __init__(self, md: "MDRun", edge_index: torch.Tensor, edge_shift: Optional[torch.Tensor]):
        self.md = weakref.proxy(md)
        super().__init__(md.ef, md._z, edge_index, md._batch, md.n_mol, cell=md._cell, edge_shift=edge_shift,
                         check_cell=False, images=md.images)

    def model(self):
        """The step ``CapturedStep`` records, eagerly: (energy, forces[, stress]) of ``self.pos`` on the stored list."""
        return super()._body()

    def _body(self):
        self.md._pre(self.pos, self.cell)
        self.md._verify(self.pos, self.g, self.cell)
        out = super()._body()
        self.md._post(*out)
        return out


class _RebuiltRecordedStep(RebuiltStep):
    """``rebuild="device"``: ``RebuiltStep`` with the integrator around its body -- ``_pre`` -> the rebuild -> model -> ``_post`` --
    recorded (``capture``) or launched eagerly on the same padded buffers.  No verify kernel: the list is never stale.  The
    driver's sticky word is the one gn_padded_tail sets; the driver is held weakly, as in ``_RecordedStep``.  A driver whose
    cell moves (``_ListDriver._cell_moves``) gets the moving-cell form of the step: gn_cell_image_ranges, inside the rebuild,
    writes the driver's sticky word and its ``_reason``."""

    def __init__(self, md: "_ListDriver", capture: bool):
        self.md = weakref.proxy(md)
        moves = md._cell_moves
        super().__init__(md.ef, md._z, md._batch, md.n_mol, max_num_neighbors=md.max_num_neighbors, cell=md._cell,
                         images=md.images, capture=capture, state=md._state, cell_moves=moves,
                         reason=md._reason if moves else None)

    def _body(self):
        self.md._pre(self.pos, self.cell)
        out = super()._body()
        self.md._post(*out)
        return out


class _EagerStep:
    """``rebuild="host"``, ``captured=False``: the holder of the ``engine.Graph`` of the current list -- a new one for the list of
    every step (``set_list``) -- and of the position buffer the driver integrates.  ``model`` launches what ``CapturedStep``
    records, [gn_cell_prepare ->] edge vectors -> geometry -> ``pipeline.energy_forces``, eagerly."""

    def __init__(self, md: "_ListDriver", edge_index: torch.Tensor, edge_shift: Optional[torch.Tensor]):
        rep, dev = md.ef.rep, md._z32.device
        self.md, self.cfg, self.pw = weakref.proxy(md), rep.config(), rep.packed_weights()
        self.pos, self.cell = torch.zeros((md.N, 3), dtype=torch.float32, device=dev), md._cell
        self.inv_cell = self.volume = None
        if self.cell is not None:
            self.inv_cell, self.volume = torch.empty_like(self.cell), torch.empty(md.n_mol, dtype=torch.float32, device=dev)
        self.set_list(edge_index, edge_shift)

    def set_list(self, edge_index, edge_shift):
        self.g = engine.Graph(self.cfg, self.pw, self.md.N, edge_index.contiguous(), self_images=self.cell is not None)
        if self.cell is not None:
            self.g.set_periodic(edge_shift, self.md._batch, self.cell)
        self.g.csc()

    def model(self):
        md = self.md
        if self.cell is not None:
            graph.cell_prepare(self.cell, self.inv_cell, self.volume)
        self.g.set_positions(self.pos, self.cell)
        return energy_forces(cfg=self.cfg, pw=self.pw, head=md.ef.head, z32=md._z32, g=self.g, mol_ptr=md._mol_ptr,
                             n_mol=md.n_mol, volume=self.volume)


class _RebuildOption(type):
    """The constructor call of a driver takes ``rebuild="host" | "device"`` next to the arguments of its ``__init__``, whose
    parameter lists are a pinned public surface and stay what they were.  The mode is checked and stored on the instance
    (``self.rebuild``) before ``__init__`` runs, so everything ``__init__`` refuses it still refuses before any launch."""

    def __call__(cls, *args, rebuild: str = "host", **kw):
        check_rebuild(rebuild)
        self = cls.__new__(cls)
        self.rebuild = rebuild
        self.__init__(*args, **kw)
        return self


class _ListDriver(metaclass=_RebuildOption):
    """What ``MDRun`` and ``relax.Relax`` share, once: the kept buffers of the last completed step and their properties, the
    neighbour search, the device check of the stored list, the record / repair / replay loop and the handling of the sticky
    word.  A driver supplies ``_pre(pos, cell)`` (everything before the neighbour list) and ``_post(energy, forces[, stress])``
    (everything after the model) -- the protocol the three step classes above talk to -- and may override ``_cell_moves``,
    ``_guarded`` (the sticky word is set: was it something other than the list?), ``_after_pre`` (eager mode, between ``_pre`` and
    the search) and ``_looked`` (the host has just read the device state: True ends ``run`` early).

    The three modes differ in the step they build (``_record``), in what advances one step (``_advance``) and in what a set
    sticky word means (``_stuck``); ``run`` is written once."""

    #: the cell changes between two steps (a barostat): the device-rebuilt step recomputes its image ranges in every step
    _cell_moves = False

    def _setup(self, ef, z, pos, batch, n_mol, cell, ranges, images, max_num_neighbors, check_every, captured, log_len, vel=None):
        dev = pos.device
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.ef, self.n_mol, self.N, self.images = ef, int(n_mol), pos.shape[0], images
        self.cutoff, self.max_num_neighbors = float(ef.rep.cutoff), int(max_num_neighbors)
        self.captured, self.check_every, self.log_len = bool(captured), int(check_every), int(log_len)
        self._z, self._z32 = z, z.to(torch.int32).contiguous()
        self._batch = batch.to(torch.int64).contiguous()
        self._mol_ptr = molecule_ptr(self._batch, self.n_mol)
        self._cell = self._inv_cell = self._ranges = None
        if cell is not None:
            self._cell, self._inv_cell, self._ranges = graph.box_arrays(cell, ranges, self.n_mol, dev)
        self._state = torch.zeros(2, **i32)                       # {stale list (sticky), completed steps}
        self._row_flag, self._changed = torch.zeros(self.N, **i32), torch.zeros(self.n_mol, **i32)
        self._done, self.rebuilds, self._fresh = 0, 0, False
        # every buffer of the recorded chain is made and initialised here, by torch, never inside the recording
        self._vel = torch.zeros((self.N, 3), **f32) if vel is None else vel.detach().to(**f32).clone().contiguous()
        self._f = torch.empty((self.N, 3), **f32)                 # forces of the last completed step: what the next one starts from
        self._e = torch.empty(self.n_mol, **f32)
        self._stress = torch.empty((self.n_mol, 3, 3), **f32) if cell is not None else None
        self._log = torch.zeros((self.log_len, self.n_mol, 2), **f32)

    def _start(self, start):
        """The first step object and the first model evaluation, at ``start``: its forces, energies and stress are the kept
        ones of step 0."""
        self._record(start)
        self._state[:1].zero_()
        with torch.no_grad():
            out = self._step.model()
        self._f.copy_(out[1])
        self._e.copy_(out[0].reshape(-1))
        if self._stress is not None:
            self._stress.copy_(out[2])

    def _list(self, pos):
        """(edge_index, edge_shift or None) of ``pos``: the project's own search (one host read of the edge count)."""
        if self._cell is None:
            return graph.distance(pos, self._batch, self.cutoff, self.max_num_neighbors)[0], None
        ei, _, _, sh = graph.distance_pbc(pos, self._batch, self._cell, self.cutoff, self.max_num_neighbors, n_mol=self.n_mol,
                                          check=False, image_range=self._ranges)
        return ei, sh

    def _verify(self, pos, g, cell=None):
        graph.verify_list(pos, self._batch, self._mol_ptr, self.n_mol, g.rowptr, g.src, self.cutoff, self.max_num_neighbors,
                          self._row_flag, self._changed, self._state, shift=g.shift, cell=cell,
                          inv_cell=self._inv_cell, image_range=self._ranges)

    def _record(self, pos):
        """Build the mode's step at ``pos`` -- device list: the step that owns the padded buffers, recorded or not; host list: the
        search, then the recording on that list or the eager holder of it -- and move ``pos`` into its buffer; the step's position
        buffer and its cell (a recording's clone of the current one) become the driver's.  The sticky word is held at 1 meanwhile
        (a recording's warm-up runs advance nothing) and LEFT at 1: the caller clears it."""
        self._state[:1].fill_(1)
        if self.rebuild == "device":
            self._step = _RebuiltRecordedStep(self, capture=self.captured)
        else:
            self._lst = self._list(pos)
            self._step = (_RecordedStep if self.captured else _EagerStep)(self, *self._lst)
        self._step.pos.copy_(pos)
        self._pos, self._cell, self._fresh = self._step.pos, self._step.cell, self.captured

    def _guarded(self):
        pass

    def _after_pre(self):
        pass

    def _looked(self) -> bool:
        return False

    def _repair(self):
        """The sticky word is set: the state is the one after the move (MD: the drift and the cell move) of the first incomplete
        step.  New list there, new graph (the old one is dropped first: one alive at a time), then the rest of that step eagerly."""
        torch.cuda.synchronize()
        pos, self._step = self._pos, None
        self._record(pos)
        self._state[:1].zero_()
        self._post(*self._step.model())
        self.rebuilds += 1
        self._done += 1

    def _advance(self):
        """One step of the mode: a replay of the recording, the device-list chain launched eagerly, or (host list, eager) the
        chain around a new search."""
        if self.captured:
            self._step.graph.replay()
        elif self.rebuild == "device":
            self._step._body()
        else:
            self._pre(self._pos, self._cell)
            self._after_pre()
            lst = self._list(self._pos)
            if not (torch.equal(lst[0], self._lst[0]) and (lst[1] is None or torch.equal(lst[1], self._lst[1]))):
                self.rebuilds += 1
            self._lst = lst
            self._step.set_list(*lst)
            self._post(*self._step.model())

    def _stuck(self):
        """The sticky word is set and it was not the driver's own doing (``_guarded`` raises then).  Host list: the list is stale,
        repair it.  Device list: nothing is verified, repaired or re-recorded; it is the overflow guard of gn_padded_tail."""
        if self.rebuild == "device":
            raise RuntimeError(f"the neighbour search found {self.edge_count} edges, outside the padded layout's bound "
                               f"[{self.N}, {self._step.layout.e_bound}]: the run stops at step {self._done}")
        self._repair()

    @torch.no_grad()
    def run(self, n: int):
        """Advance ``n`` steps.  The host reads the device state -- the sticky word, the step counter, then ``_looked`` -- after
        every ``check_every`` steps, after the first replay of a newly recorded graph and at the end (a stream synchronisation
        each).  Host list, eager: the search reads its edge count in every step anyway and the sticky word is the driver's own
        business (``_after_pre``), so the steps are counted on the host and the state is not read."""
        target = self._done + int(n)
        polled = self.captured or self.rebuild == "device"
        while self._done < target:
            burst = 1 if self._fresh or not polled else min(self.check_every, target - self._done)
            for _ in range(burst):
                self._advance()
            self._fresh = False
            if polled:
                stuck, self._done = self._state.tolist()         # (the synchronisation)
                if stuck:
                    self._guarded()                              # (a driver's own reasons first: they raise, or steer the repair)
                    self._stuck()
            else:
                self._done += 1
            if self._looked():
                break
        return self

    @property
    def edge_count(self) -> int:
        """The real edges of the current neighbour list (device mode: one host read of the device word)."""
        return int(self._step.edge_count.item()) if self.rebuild == "device" else self._step.g.E

    def _ring(self, log):
        k = min(self.step, self.log_len)
        rows = [(s % self.log_len) for s in range(self.step - k, self.step)]
        return log[torch.tensor(rows, dtype=torch.long, device=log.device)]

    # ---- state and queries -----------------------------------------------------------------------------------------
    @property
    def pos(self) -> torch.Tensor:
        return self._pos.clone()

    @property
    def vel(self) -> torch.Tensor:
        return self._vel.clone()

    @property
    def potential_energy(self) -> torch.Tensor:
        """[n_mol], of the last completed step (of the start before the first)."""
        return self._e.clone()

    @property
    def stress(self) -> torch.Tensor:
        """[n_mol, 3, 3] of the last completed step (periodic runs: ``EnergyForces``' stress)."""
        if self._stress is None:
            raise ValueError("stress: this run has no cell")
        return self._stress.clone()


class MDRun(_ListDriver):
    """A trajectory of ``ef``'s model (``pipeline.EnergyForces``) from ``pos`` (and ``vel``, default zero) with time step ``dt``.

        md = MDRun(EnergyForces(rep, head, check_edges=False), z, pos, batch, n_mol, dt=0.5, force_scale=EV_ANGSTROM_AMU_FS,
                   thermostat=dict(kT=0.0259, gamma=0.01, key=1234))
        md.run(1000)
        md.pos, md.vel, md.potential_energy, md.kinetic_energy, md.energy_log(), md.rebuilds
        md.cell, md.volume, md.pressure, md.npt_log()              # periodic runs / runs with a barostat

    ``masses``: a table indexed by atomic number (default ``default_masses()``).  ``force_scale``: a = force_scale * F / m in
    the caller's units (``EV_ANGSTROM_AMU_FS``, ``KCAL_MOL_ANGSTROM_AMU_FS``; default 1: consistent units).  ``cell`` / ``images`` /
    ``max_num_neighbors``: as ``graph.distance_pbc``; the cell is fixed unless there is a barostat.  ``thermostat``: None (NVE) or
    ``dict(kT=, gamma=, key=)``: a Langevin O step of half a time step on either side of the drift, its noise a pure function
    of (key, step, half, atom, component) -- ``gn_md_noise`` reproduces it.  ``check_every``: replays between two host reads of
    the stale-list word (the trajectory does not depend on it).  ``log_len``: rows of the (potential, kinetic) energy ring
    buffer.  ``captured=False``: the eager reference (module docstring).

    ``rebuild`` (a keyword of the constructor call, ``MDRun(..., rebuild="device")``, taken by the drivers' metaclass; not a
    parameter of ``__init__``): "host" (default: the modes of the module docstring) or "device": the list is REBUILT inside every step by the
    search's own kernels into a list of fixed capacity (``pipeline.RebuiltStep``) -- no verify kernel, no repair, no second
    recording; ``rebuilds`` stays 0 and ``edge_count`` reports the current number of real edges.  For systems whose list changes
    often (a host rebuild costs about ten eager steps).  ``captured=False, rebuild="device"`` launches the same chain eagerly on
    the same padded buffers and agrees with the recorded one bit for bit; in the "f32" and "split" arithmetics both are the
    ``rebuild="host"`` trajectory, bit for bit.  With ``barostat=`` it needs ``images="all"`` or ``"auto"``: the step then always
    runs the multi-image search and recomputes its image ranges from the moved cell on the device (module docstring), so a
    constant-pressure run replays one graph from start to end; ``images="minimum"`` with a barostat is refused in this mode.

    ``barostat``: None (the cell is fixed: the launches and the bits of a run without this argument) or
    ``dict(pressure=, tau=, compressibility=, kT=None, key=None, max_step=0.05)``: isotropic stochastic cell rescaling on the
    device, inside the replay (module docstring: the scheme, its placement -- a first-order splitting, the driving pressure lags
    the move by one drift -- and the guard).  ``pressure``: the target in the model's energy unit per length^3
    (``BAR_EV_ANGSTROM3``, ``BAR_KCAL_MOL_ANGSTROM3``); ``tau``: the relaxation time in the caller's time unit;
    ``compressibility``: beta_T in inverse pressure units; ``kT``: default the thermostat's, required without one, 0 = the
    deterministic weak-coupling limit; ``key``: an int or a pair, default the thermostat's, required when kT > 0 without one;
    ``max_step``: the largest |d ln V| of one step -- a larger (or non-finite) one stops the run with ``RuntimeError`` at the
    last completed step.  A cell that shrinks below what ``images`` allows raises ``graph.resolve_images``' ``ValueError``
    from ``run``.

    Refused with ``ValueError`` before any launch: dt <= 0, a negative or missing mass, kT < 0, gamma < 0, a cell that
    ``graph.resolve_images`` refuses, ``pos`` or ``cell`` requiring grad; a barostat without a cell, with entries missing, with
    tau, compressibility or max_step not positive and finite, a non-finite pressure, kT < 0, or kT > 0 without a key; an
    unknown ``rebuild``, or ``rebuild="device"`` with a barostat and ``images="minimum"``."""

    def __init__(self, ef: EnergyForces, z: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, n_mol: int, dt: float,
                 masses=None, force_scale: float = 1.0, vel: Optional[torch.Tensor] = None,
                 cell: Optional[torch.Tensor] = None, images: str = "minimum", max_num_neighbors: int = 32,
                 thermostat: Optional[dict] = None, check_every: int = 1, log_len: int = 1024, captured: bool = True,
                 barostat: Optional[dict] = None):
        table, ranges = validate(z, pos, dt, masses, force_scale, thermostat, cell, float(ef.rep.cutoff), images, check_every,
                                 log_len, rebuild=self.rebuild, barostat=barostat)
        dev = pos.device
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self._setup(ef, z, pos, batch, n_mol, cell, ranges, images, max_num_neighbors, check_every, captured, log_len, vel=vel)
        self.dt, self.force_scale = float(dt), float(force_scale)
        self._mass = table.to(dev)
        self._thermo = None
        if thermostat is not None:
            c1, c2 = langevin_coefficients(thermostat["kT"], thermostat["gamma"], 0.5 * self.dt, self.force_scale)
            self._thermo = (c1, c2, torch.tensor(_key_words(thermostat["key"]), dtype=torch.int64, device=dev))
        self._ke = torch.empty(self.n_mol, **f32)
        self._baro = None
        if barostat is not None:
            self._baro = b = barostat_parameters(barostat, thermostat, cell)
            self._cell = self._cell.clone()                    # it moves in place: never the caller's tensor
            self._baro_key = torch.tensor(_key_words(b["key"]), dtype=torch.int64, device=dev) if b["kT"] > 0 else None
            self._volume, self._p = torch.empty(self.n_mol, **f32), torch.empty(self.n_mol, **f32)
            self._s, self._inv_s = torch.ones(self.n_mol, **f32), torch.ones(self.n_mol, **f32)
            self._reason = torch.zeros(self.n_mol, **i32)      # why a box set the sticky word: 1 cell guard, 2 max_step
            self._npt_log = torch.zeros((self.log_len, self.n_mol, 2), **f32)
        self._start(pos.detach().to(**f32).contiguous())
        self._kinetic()
        if self._baro is not None:
            graph.cell_prepare(self._cell, self._inv_cell, self._volume)
            self._pressure(self._stress, ring=False)

    # ---- the pieces of a step: the same launches whether recorded or eager -----------------------------------------
    def _kick(self, force):
        call("gn_md_kick", ptr(self._vel), ptr(force), ptr(self._z32), ptr(self._mass), self._mass.numel(), self.N,
             float(0.5 * self.dt * self.force_scale), ptr(self._state), engine._stream())

    def _langevin(self, draw):
        if self._thermo is not None:
            c1, c2, key = self._thermo
            call("gn_md_langevin", ptr(self._vel), ptr(self._z32), ptr(self._mass), self._mass.numel(), self.N, float(c1),
                 float(c2), ptr(key), draw, ptr(self._state), engine._stream())

    def _kinetic(self):
        call("gn_md_kinetic", ptr(self._vel), ptr(self._z32), ptr(self._mass), self._mass.numel(), ptr(self._mol_ptr), self.N,
             self.n_mol, float(self.force_scale), ptr(self._ke), ptr(self._state), engine._stream())

    def _pressure(self, stress, ring=True):
        call("gn_npt_pressure", ptr(self._ke), ptr(stress), ptr(self._volume), self.n_mol, ptr(self._p),
             ptr(self._npt_log) if ring else None, self.log_len, ptr(self._state), engine._stream())

    def _pre(self, pos, cell=None):
        """Everything before the neighbour list.  ``pos`` / ``cell``: the buffers the step reads (a recording passes its own)."""
        b = self._baro
        if b is not None:          # the move and its refusal, from the kept pressure: at the head of the step (module docstring)
            call("gn_npt_barostat", ptr(cell), ptr(self._volume), ptr(self._p), self.n_mol, b["pressure"], b["compressibility"],
                 b["tau"], self.dt, b["kT"], b["max_step"], ptr(self._baro_key), ptr(self._s), ptr(self._inv_s), ptr(self._state),
                 ptr(self._reason), engine._stream())
        self._kick(self._f)
        self._langevin(0)
        call("gn_md_drift", ptr(pos), ptr(self._vel), self.N, float(self.dt), ptr(self._state), engine._stream())
        self._langevin(1)
        if b is not None:
            call("gn_npt_rescale", ptr(pos), ptr(self._vel), ptr(self._batch), ptr(self._s), ptr(self._inv_s), self.N, self.n_mol,
                 ptr(self._state), engine._stream())
            graph.cell_prepare(cell, self._inv_cell, self._volume)     # (the driver's own volume: the pressure's and the next move's)
            if self.rebuild != "device":   # device mode: gn_cell_image_ranges inside the step takes the guard's place
                call("gn_npt_cell_guard", ptr(cell), self.n_mol, self.cutoff, ptr(self._ranges), ptr(self._state),
                     ptr(self._reason), engine._stream())

    def _post(self, energy, forces, stress=None):
        self._kick(forces)
        self._kinetic()
        if self._baro is not None:
            self._pressure(stress)
        call("gn_md_finish", ptr(self._state), ptr(forces), ptr(self._f), self.N, ptr(energy), ptr(self._ke), ptr(self._e),
             ptr(stress), ptr(self._stress), ptr(self._log), self.log_len, self.n_mol, engine._stream())

    def _guarded(self):
        """The sticky word is set: was it the barostat?  Reason 2 (a move beyond ``max_step``) ends the run; reason 1 (the cell
        outgrew the search parameters) gets new ones from ``graph.resolve_images`` on the current cell, or what that raises.
        The caller repairs the list next.  Device mode repairs nothing: reason 1 is gn_cell_image_ranges' refusal and raises
        what ``graph.image_ranges`` raises on the reported cell."""
        if self._baro is None:
            return
        reason = self._reason.tolist()
        if 2 in reason:
            raise RuntimeError(f"barostat: box {reason.index(2)} asks for a volume move |d ln V| that is not finite or exceeds "
                               f"max_step = {self._baro['max_step']} in step {self._done + 1}; the run stops at step {self._done}")
        if 1 in reason and self.rebuild == "device":            # gn_cell_image_ranges refused the moved cell: the host's words
            graph.image_ranges(self._cell, self.cutoff)
            raise RuntimeError(f"barostat: the device refused the image ranges of box {reason.index(1)} in step {self._done + 1}, "
                               f"but graph.image_ranges accepts the reported cell; the run stops at step {self._done}")
        if 1 in reason:
            ranges = graph.resolve_images(self._cell, self.cutoff, self.images)
            self._ranges = None if ranges is None else ranges.expand(self.n_mol, 3).contiguous().to(self._cell.device)
            self._reason.zero_()

    def _after_pre(self):
        if self._baro is not None and self._state.tolist()[0]:      # the guard's verdict, from the guard's kernel
            self._guarded()
            self._state[:1].zero_()

    # ---- state and queries (``pos``, ``vel``, ``potential_energy``, ``stress``: ``_ListDriver``'s) -----------------------------
    @property
    def _cell_moves(self) -> bool:
        return self._baro is not None

    @property
    def step(self) -> int:
        """Completed steps."""
        return self._done

    @property
    def kinetic_energy(self) -> torch.Tensor:
        """[n_mol]: (1/2) sum m v^2 / force_scale, in the model's energy unit."""
        return self._ke.clone()

    @property
    def cell(self) -> torch.Tensor:
        """[n_mol, 3, 3]: the current cell (periodic runs)."""
        if self._cell is None:
            raise ValueError("cell: this run has no cell")
        return self._cell.clone()

    @property
    def volume(self) -> torch.Tensor:
        """[n_mol]: |det cell| (gn_cell_prepare's)."""
        if self._cell is None:
            raise ValueError("volume: this run has no cell")
        return self._volume.clone() if self._baro is not None else graph.cell_prepare(self._cell)[1]

    @property
    def pressure(self) -> torch.Tensor:
        """[n_mol]: the internal pressure 2 K / (3 V) - tr(stress) / 3 of the last completed step (of the start before the
        first), in the model's energy unit per length^3."""
        if self._cell is None:
            raise ValueError("pressure: this run has no cell")
        if self._baro is not None:
            return self._p.clone()
        p, vol = torch.empty(self.n_mol, dtype=torch.float32, device=self._ke.device), self.volume
        call("gn_npt_pressure", ptr(self._ke), ptr(self._stress), ptr(vol), self.n_mol, ptr(p), None, 0, None,
             engine._stream())
        return p

    def energy_log(self) -> torch.Tensor:
        """[k, n_mol, 2]: (potential, kinetic) energy after each of the last k = min(step, log_len) steps, oldest first."""
        return self._ring(self._log)

    def npt_log(self) -> torch.Tensor:
        """[k, n_mol, 2]: (volume, internal pressure) after each of the last k = min(step, log_len) steps, oldest first (runs
        with a barostat)."""
        if self._baro is None:
            raise ValueError("npt_log: this run has no barostat")
        return self._ring(self._npt_log)
