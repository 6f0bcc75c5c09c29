"""Fused energy + force step: representation forward (with tape) -> Atomwise head ->
head gradient -> hand-written backward -> force scatter, all through the C ABI with no
autograd graph and no host synchronisation (hipGraph-capturable).  This is the path
bench.py times; the autograd.Function wrappers in gotennet.py expose the same kernels to
reference-style callers (GotenModel / torch.autograd.grad).

``CapturedStep`` records that step on a fixed edge list into one hipGraph; ``RebuiltStep`` records it behind a rebuild of
the list on the device, for a fixed cell or (``cell_moves=True``) for one that moves between the replays, its image ranges
recomputed inside the chain by gn_cell_image_ranges.  The chain itself is stated once (``energy_forces``), and so is the recording
(``_record``): each class adds only what is its own in front of them."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import engine, graph
from ._lib import call, ptr
from .gotennet import GotenNet
from .outputs import Atomwise, molecule_ptr


def energy_forces(cfg, pw, head, z32, g, mol_ptr, n_mol, volume=None):
    """The energy-and-force chain, stated once for every step class and driver: forward (with tape) -> ``head.energy_raw`` ->
    ``head.grad_h_raw`` -> backward -> force scatter, and gn_virial when ``volume`` (fp32 [n_mol], gn_cell_prepare's) is given.
    ``g``: the ``engine.Graph`` with its geometry set.  -> (energy, forces) or (energy, forces, stress)."""
    h, X, tape = engine.forward(cfg, pw, z32, g, save=True)
    e, y, pre1 = head.energy_raw(h, z32, mol_ptr, n_mol, mode=cfg.gemm_mode)
    gh = head.grad_h_raw(pre1, cfg.F_model or cfg.F, mode=cfg.gemm_mode)
    g_vec, g_diff = engine.backward(cfg, pw, z32, g, tape, gh, None)
    f = engine.pos_gradient(g, g_vec, g_diff, sign=-1.0)
    if volume is None:
        return e, f
    return e, f, engine.virial(g, g_vec, g_diff, mol_ptr, n_mol, volume)


def _record(body, device, warmup):
    """``warmup`` runs of ``body`` on a side stream (weight planes / transposes are built there, off the capture), then one run
    recorded into a ``torch.cuda.CUDAGraph`` (hipGraph on ROCm) on the default memory pool -> (graph, what that run returned:
    the static output buffers of every replay)."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(warmup):
            body()
    torch.cuda.current_stream(device).wait_stream(side)
    recorded = torch.cuda.CUDAGraph()
    with torch.cuda.graph(recorded), torch.no_grad():
        out = body()
    return recorded, out


class EnergyForces:
    """``check_edges`` (default on): validate the caller's edge list on the device (index range, target-major order;
    one host sync per call) and stable-sort it by target when needed -- energies and forces are per molecule / per atom,
    so the order of the edge list never shows in the result; the ``batch`` vector must be non-decreasing (molecules
    contiguous) and is checked too.  Callers that pass radius-graph output
    (``gotennet_amd.graph.distance``: target-major by construction) switch it off and stay sync-free.

    An inference tool: attention dropout is never applied, whatever the representation's ``training`` flag says."""

    def __init__(self, representation: GotenNet, head: Atomwise, check_edges: bool = True, cache_topology: bool = True,
                 replay: bool = False, replay_after: int = 2):
        self.rep, self.head, self.check_edges = representation, head, check_edges
        #: ``replay``: after ``replay_after`` consecutive energy+force calls on the SAME topology (a ``cache_topology``
        #: hit: same edge_index tensor, same sizes, same packed weights and configuration) the step -- geometry kernel,
        #: forward, head, backward, force scatter: every launch of the eager step, nothing skipped -- is recorded into
        #: ONE hipGraph (torch.cuda.CUDAGraph) and later calls replay it on fresh copies of ``edge_diff`` / ``edge_vec`` /
        #: ``z`` / ``mol_ptr``: the ~190 launches of a step are dispatched by the GPU's command processor instead of the
        #: host (-2.8 % on the C2 batch, 2.3 -> 1.9 ms for one molecule), bit-identical to the eager step.  The graph's
        #: private memory pool (the step's work buffers, ~4.5 GB at C2) stays allocated until the topology changes or
        #: ``clear_cache()``.  Returned tensors are copies.  Off by default (a library should not capture behind the
        #: caller's back); an MD driver or a benchmark on a fixed neighbour list switches it on.
        self.replay, self.replay_after = bool(replay), max(1, int(replay_after))
        self._hits, self._graph_state = 0, None
        #: ``cache_topology``: a repeated call with the SAME ``edge_index`` tensor (same storage, shape and PyTorch
        #: version counter -- an MD loop or a benchmark on a fixed neighbour list) reuses the CSR / CSC index arrays,
        #: the validation verdict and the stable-sort permutation of the previous call: no sort / scan / fill launch and
        #: no host read on such a step, only the geometry kernel runs on the new ``edge_diff`` / ``edge_vec``.  The cache
        #: holds a reference to the tensor (its memory cannot be recycled under the key) and the E-sized index / geometry
        #: buffers of its Graph until the next different edge list or ``clear_cache()``; writes that bypass PyTorch's
        #: version counter (raw pointers, ``.data``) are not seen: pass ``cache_topology=False`` for such callers.
        #: Inference tensors (made under ``torch.inference_mode()``) have no version counter and are never cached.
        self.cache_topology = cache_topology
        self._topo = None
        self._mol_ptr = None                         # (key, batch tensor, offsets) of the last call without mol_ptr

    def clear_cache(self):
        """Drop the cached topology (it keeps the last ``edge_index`` tensor and E-sized index / geometry buffers alive)
        and the recorded hipGraph with its memory pool."""
        self._topo = self._mol_ptr = None
        self._hits, self._graph_state = 0, None

    def _graph(self, cfg, pw, N, edge_index, edge_diff, edge_vec, need_csc, self_images=False):
        key = None
        if self.cache_topology and not edge_index.is_inference():
            # (inference tensors -- a neighbour list built under torch.inference_mode() -- carry no version counter:
            #  reading ``_version`` raises, and a write to one cannot be seen, so they are never cached)
            key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), tuple(edge_index.stride()), N,
                   id(pw), cfg.lmax, cfg.R, cfg.basis, bool(cfg.scale_edge), bool(self.check_edges))
        hit = key is not None and self._topo is not None and self._topo[0] == key and self._topo[1] is edge_index
        self._hits = self._hits + 1 if hit else 0
        if not hit:
            self._graph_state = None
        if hit:
            _, _, g, order = self._topo
            g.cfg = cfg                              # cutoff / eps may have changed under the same packed weights
            g.self_images = self_images
            if order is not None:
                edge_diff, edge_vec = edge_diff[order], edge_vec[order]
            g.set_geometry(edge_diff.contiguous(), edge_vec.contiguous())
        else:
            ei, order = edge_index.contiguous(), None
            if self.check_edges:
                ei, edge_diff, edge_vec, order = engine.sorted_edges(ei, edge_diff, edge_vec, N)
            g = engine.Graph(cfg, pw, N, ei, edge_diff.contiguous(), edge_vec.contiguous(), self_images=self_images)
            self._topo = (key, edge_index, g, order) if key is not None else None
        if need_csc:
            g.csc()
        return g

    @torch.no_grad()
    def __call__(self, z: torch.Tensor, edge_index: torch.Tensor, edge_diff: torch.Tensor, edge_vec: torch.Tensor,
                 batch: torch.Tensor, n_mol: int, mol_ptr: Optional[torch.Tensor] = None,
                 forces: bool = True, cell: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], ...]:
        """-> (energy [n_mol,1], forces [N,3]), or with ``cell`` (energy, forces, stress [n_mol,3,3]); without ``forces``
        the entries after the energy are None.

        ``cell`` (fp32 [n_mol, 3, 3] or [3, 3], rows = lattice vectors): the edges are those of a periodic system
        (``graph.distance_pbc``, any ``images``: ``edge_vec`` already carries the lattice shifts; an atom's own images -- ``src == dst``
        with ``edge_diff`` > 0 -- are neighbours, the self-loop is ``src == dst`` with ``edge_diff == 0``) and the call returns
        (energy, forces, stress [n_mol, 3, 3]) with stress[m] = (1 / |det cell_m|) sum_{e in box m} r_e (x) dE/dr_e = (1/V) dE/d(strain),
        ASE's sign, not symmetrised (None without ``forces``).  Energies and forces are those of the same call without
        ``cell``.  A call with ``cell`` neither uses nor creates the recorded step of ``replay=True``: it runs eagerly (a
        periodic MD loop records its step with ``CapturedStep(..., cell=, edge_shift=)``), and it leaves the count of consecutive calls that
        decides when a call without ``cell`` records (``replay_after``) where it was."""
        graph.check_periodic_args(cell)                            # before any launch
        rep = self.rep
        cfg, pw = rep.config(), rep.packed_weights()
        N = z.shape[0]
        if mol_ptr is None:
            # (bincount + cumsum + two fills per call otherwise: kept per batch tensor, like the topology)
            mkey = None if (batch.is_inference() or not self.cache_topology) else (batch.data_ptr(), batch._version, tuple(batch.shape), n_mol)
            if mkey is not None and self._mol_ptr is not None and self._mol_ptr[0] == mkey and self._mol_ptr[1] is batch:
                mol_ptr = self._mol_ptr[2]
            else:
                if self.check_edges and N > 1 and bool((batch[1:] < batch[:-1]).any()):
                    # (a host read, like the edge validation; not repeated for a cached batch vector)
                    raise ValueError("batch must be non-decreasing (each molecule's atoms contiguous)")
                mol_ptr = molecule_ptr(batch, n_mol)
                self._mol_ptr = (mkey, batch, mol_ptr) if mkey is not None else None
        if cell is not None:
            volume = graph.cell_prepare(graph.broadcast_cell(cell.to(z.device), n_mol))[1] if forces else None
            hits = self._hits
            g = self._graph(cfg, pw, N, edge_index, edge_diff, edge_vec, forces, self_images=True)
            if self._hits:                           # a topology hit: the replay counter of the plain path does not move
                self._hits = hits                    # (a miss has reset it, as any new topology does)
            return self._step(cfg, pw, g, z.to(torch.int32), mol_ptr, n_mol, forces, volume=volume, periodic=True)
        gs = self._graph_state
        if self.replay and gs is not None and forces and self._replay_ok(gs, cfg, pw, N, edge_index, n_mol):
            return self._replay(gs, z, edge_diff, edge_vec, mol_ptr)
        z32 = z.to(torch.int32)
        g = self._graph(cfg, pw, N, edge_index, edge_diff, edge_vec, forces)
        if (self.replay and forces and self._hits >= self.replay_after and self._topo is not None
                and not torch.cuda.is_current_stream_capturing()):
            gs = self._capture(cfg, pw, g, z32, edge_index, n_mol, mol_ptr)
            return self._replay(gs, z, edge_diff, edge_vec, mol_ptr)
        return self._step(cfg, pw, g, z32, mol_ptr, n_mol, forces)

    def _step(self, cfg, pw, g, z32, mol_ptr, n_mol, forces, volume=None, periodic=False):
        if forces:                                   # (a periodic call with forces always brings its volume)
            return energy_forces(cfg, pw, self.head, z32, g, mol_ptr, n_mol, volume)
        h, X, tape = engine.forward(cfg, pw, z32, g, save=False)
        e = self.head.energy_raw(h, z32, mol_ptr, n_mol, mode=cfg.gemm_mode)[0]
        return (e, None, None) if periodic else (e, None)

    # ---- hipGraph replay of the eager step on a cached topology --------------------------------------------------
    def _replay_ok(self, gs, cfg, pw, N, edge_index, n_mol) -> bool:
        # (the head's scalars -- last bias, scale / shift, AtomwiseV3's molecule shift -- are baked into the captured kernel
        #  arguments and its transposed weights are captured pointers: its cache key is part of the replay key)
        ok = (self._topo is not None and self._topo[1] is edge_index and not edge_index.is_inference()
              and gs["key"] == (self._topo[0], cfg, id(pw), n_mol, self._head_key()) and self._topo[0][1] == edge_index._version)
        if not ok:
            self._graph_state = None
        return ok

    def _head_key(self):
        """Everything of the head a recorded step depends on: its packed-cache key (parameter addresses / versions,
        incl. the ScaleShift buffers) and the host scalars that become kernel arguments."""
        packed = self.head._packed()
        c = packed[1] if isinstance(packed, tuple) else packed
        return (id(self.head), c["key"], c.get("scale"), c.get("shift"), c.get("b2"), c.get("mol_shift"),
                tuple(c.get("scales") or ()), tuple(c.get("shifts") or ()), tuple(c.get("b2s") or ()))

    def _capture(self, cfg, pw, g, z32, edge_index, n_mol, mol_ptr):
        dev = z32.device
        order = self._topo[3]
        st = dict(key=(self._topo[0], cfg, id(pw), n_mol, self._head_key()), g=g, order=order, z32=z32.clone(), mol_ptr=mol_ptr.clone(),
                  ed=torch.empty(g.E, dtype=torch.float32, device=dev), ev=torch.empty((g.E, 3), dtype=torch.float32, device=dev))
        st["ed"].copy_(g.edge_diff)
        st["ev"].copy_(g.edge_vec)

        def body():
            g.set_geometry(st["ed"], st["ev"])
            return self._step(cfg, pw, g, st["z32"], st["mol_ptr"], n_mol, True)

        st["graph"], (st["e"], st["f"]) = _record(body, dev, 1)
        self._graph_state = st
        return st

    def _replay(self, st, z, edge_diff, edge_vec, mol_ptr):
        order = st["order"]
        st["ed"].copy_(edge_diff if order is None else edge_diff[order])
        st["ev"].copy_(edge_vec if order is None else edge_vec[order])
        st["z32"].copy_(z)
        st["mol_ptr"].copy_(mol_ptr)
        st["graph"].replay()
        return st["e"].clone(), st["f"].clone()


class InFlight:
    """Several independent energy+force evaluations in flight at once: ``lanes`` ``EnergyForces`` objects, each on its own
    HIP stream, fed round-robin -- call k runs on lane k % lanes while call k - 1 is still executing.

    Why it pays on MI355X: the projection launches of a step run at the socket power cap, the
    gather / scatter launches between them do not come near it, and every launch of ONE step depends on the one before.  Two
    steps on two streams let the command processor run one step's memory-bound kernels beside the other's matrix
    kernels: 7.46 -> 6.73 ms per 128-molecule batch (lmax 2), 13.77 -> 12.56 (lmax 4), measured with hipGraph replays.  The
    price is latency (a batch takes as long as before, or longer) and a second set of work buffers.

        lanes = InFlight(rep, head, lanes=2, check_edges=False)
        for batch in stream_of_batches:
            results.append(lanes(z, edge_index, edge_diff, edge_vec, batch, n_mol))     # returns at once
        lanes.wait()                      # the CURRENT stream now waits for every lane: results are safe to read

    Inputs must be ready on the current stream when a call is made (each lane waits for the current stream first).
    Every lane keeps its own topology cache.

    Memory lifetime across the streams (PyTorch's caching allocator hands a freed block back to the stream it was
    allocated on, without waiting for OTHER streams that still read it):
      * every tensor argument of a call is ``record_stream``-ed on the lane's stream, so the caller may drop or overwrite-by-
        reallocation its inputs right after the call returns (the normal data-loader loop);
      * the tensors a call returns were allocated on the lane's stream; the object keeps a reference to them until the next
        ``wait()``, which marks them as used on the stream that waits -- read results only after ``wait()``, on that stream;
      * a weight update (a stale pack) makes the call wait for ALL lanes before the old pack's operands are freed.

    An inference tool, like the ``EnergyForces`` lanes it feeds: attention dropout is never applied."""

    def __init__(self, representation: GotenNet, head: Atomwise, lanes: int = 2, **kw):
        dev = next(representation.parameters()).device
        self.lanes = [EnergyForces(representation, head, **kw) for _ in range(max(1, int(lanes)))]
        self.streams = [torch.cuda.Stream(device=dev) for _ in self.lanes]
        self._k, self._seen = 0, set()
        self._pending = []                           # tensors returned since the last wait()
        self._pack = None                            # the weight pack the lanes were last fed with (kept alive across a rebuild)
        self._gen = 0                                # bumped with every new pack: the cold-call key (an id() of a freed pack
                                                     # can come back for a later one)

    @staticmethod
    def _tensors(objs):
        for o in objs:
            if isinstance(o, torch.Tensor):
                yield o
            elif isinstance(o, (tuple, list)):
                yield from InFlight._tensors(o)

    def __call__(self, *args, _then=None, **kw):
        """``_then(energy, forces)`` (optional) runs inside the lane's stream context right after the step is enqueued -- e.g. the
        per-step collective of a multi-GPU run."""
        k = self._k % len(self.lanes)
        self._k += 1
        st = self.streams[k]
        rep = self.lanes[k].rep
        pw = rep.packed_weights()                    # (a stale pack is rebuilt HERE, on the caller's stream, before the lane waits for it)
        if pw is not self._pack:
            # a weight update: the old pack's operands (cat'ed weights, fp16 planes, transposes) may still be read by kernels
            # queued on other lanes.  This object holds the OLD pack until every lane has drained into the current stream, so
            # its blocks are not handed to the rebuild above or to anything after it while they are in use
            self.wait()
            self._pack = pw
            self._gen += 1
            self._seen.clear()                       # keys of earlier packs can never match again
        st.wait_stream(torch.cuda.current_stream(st.device))
        for t in self._tensors(list(args) + list(kw.values())):
            if t.is_cuda:
                t.record_stream(st)                  # read on the lane's stream: not reusable by the caller's stream before that
        # The first call of a kind (with / without forces) builds lazily cached operands that ALL lanes share -- packed
        # weights, their fp16 planes, the transposes of the backward -- on THIS lane's stream: it runs alone, fenced against
        # the other lanes on both sides.  Later calls find the caches filled and overlap freely.
        kind = (bool(kw.get("forces", True)), self._gen)     # (a weight update makes a new pack: cold again)
        cold = kind not in self._seen
        if cold:
            for other in self.streams:
                if other is not st:
                    st.wait_stream(other)
        with torch.cuda.stream(st):
            out = self.lanes[k](*args, **kw)
            if _then is not None:
                _then(*out)
        if cold:
            self._seen.add(kind)
            for other in self.streams:
                if other is not st:
                    other.wait_stream(st)
        self._pending.extend(self._tensors(out))
        return out

    @property
    def next_lane(self) -> int:
        return self._k % len(self.lanes)

    def wait(self):
        """The CURRENT stream waits for every lane; the tensors returned since the last ``wait()`` are marked as used on it."""
        cur = torch.cuda.current_stream(self.streams[0].device)
        for st in self.streams:
            cur.wait_stream(st)
        for t in self._pending:
            if t.is_cuda:
                t.record_stream(cur)
        self._pending = []

    def clear_cache(self):
        for ef in self.lanes:
            ef.clear_cache()


class _StepOutputs:
    """What ``CapturedStep`` and ``RebuiltStep`` share: the kept outputs of ``_body`` -- the static buffers a recording writes
    in every replay -- and what a call returns.  ``self.cell`` is None for a step without a cell."""

    def _keep(self, out):
        self.energy, self.forces = out[0], out[1]
        self.stress = out[2] if self.cell is not None else None

    def _outputs(self):
        if self.cell is None:
            return self.energy, self.forces
        return self.energy, self.forces, self.stress


class CapturedStep(_StepOutputs):
    """Energy + forces for a FIXED edge list (static topology: an MD trajectory of molecules whose neighbour lists do
    not change, e.g. any molecule smaller than the cutoff) as ONE hipGraph replay per step.

    A step of the fused path is ~190 kernel launches; for one 21-atom molecule the eager path is launch-bound
    (2.7 ms on MI355X) while the kernels themselves need a fraction of that.  ``CapturedStep`` builds the CSR / CSC
    topology once, records edge vectors -> geometry -> forward -> head -> backward -> force scatter into a
    ``torch.cuda.CUDAGraph`` (hipGraph on ROCm) and replays it for every new set of positions.  Same kernels, same
    order, same buffers: results are bit-identical to ``EnergyForces`` on the same edge list.

        step = CapturedStep(EnergyForces(rep, head), z, edge_index, batch, n_mol)
        energy, forces = step(pos)          # views of static output buffers: copy them to keep them

    Periodic systems: pass ``cell`` (fp32 [n_mol, 3, 3] or [3, 3], rows = lattice vectors) and the ``edge_shift`` of
    ``graph.distance_pbc``.  The recorded step is then gn_cell_prepare -> gn_edge_vectors_pbc (the stored shifts, no image
    search) -> the same step -> gn_virial, all kernel nodes of the one graph:

        ei, ed, ev, sh = graph.distance_pbc(pos, batch, cell, cutoff)
        step = CapturedStep(EnergyForces(rep, head), z, ei, batch, n_mol, cell=cell, edge_shift=sh)
        energy, forces, stress = step(pos)                  # or step(pos, cell=new_cell): a barostat's move

    A new cell is copied into the static buffer and the recorded inverse / volume kernel follows it; it is width-checked on
    the host (``graph.check_cell``, one read of the cell) unless ``check_cell=False``.

    ``images="all"`` (or "auto"): the list is a multi-image one (``graph.distance_pbc(images="all")``: cells down to
    ``cutoff / 3`` wide, several images per pair, self-images).  The cell is then held to ``graph.image_ranges`` at
    construction.  A fixed list's stored shifts stay valid while the cell deforms, so all a NEW cell has to have is a finite,
    non-zero volume (``graph.check_volume``): the width conditions are conditions of the neighbour search, not of the step.

    An inference tool: attention dropout is never applied (the recorded step is ``EnergyForces``' own).
    """

    def __init__(self, ef: EnergyForces, z: torch.Tensor, edge_index: torch.Tensor, batch: torch.Tensor, n_mol: int,
                 warmup: int = 2, cell: Optional[torch.Tensor] = None, edge_shift: Optional[torch.Tensor] = None,
                 check_cell: bool = True, images: str = "minimum"):
        if (cell is None) != (edge_shift is None):           # before any launch
            raise ValueError("CapturedStep: a periodic step needs both cell and edge_shift (graph.distance_pbc returns the "
                             "shifts); neither for isolated molecules")
        graph.check_periodic_args(cell, images)
        rep, head = ef.rep, ef.head
        self.check_cell, self.images = bool(check_cell), images
        if cell is not None and self.check_cell:
            graph.resolve_images(cell, float(rep.cutoff), images)
        self.cfg, self.pw = rep.config(), rep.packed_weights()
        dev = z.device
        self.z32 = z.to(torch.int32)
        self.N, self.n_mol = z.shape[0], n_mol
        self.head = head
        self.mol_ptr = molecule_ptr(batch, n_mol)
        self.pos = torch.zeros((self.N, 3), dtype=torch.float32, device=dev)      # static input buffer
        edge_index = edge_index.contiguous()
        if ef.check_edges:                           # once, at construction: the topology is static
            bits = engine.validate_edges(edge_index, self.N)
            if bits & 2:
                raise ValueError(f"edge_index holds indices outside [0, {self.N})")
            if bits & 1:
                order = torch.sort(edge_index[1], stable=True).indices
                edge_index = edge_index[:, order].contiguous()
                edge_shift = edge_shift[order] if edge_shift is not None else None
        self.g = engine.Graph(self.cfg, self.pw, self.N, edge_index, self_images=cell is not None)
        self.cell = self.inv_cell = self.volume = None
        if cell is not None:                          # static buffers: the recorded kernels read these addresses
            self.cell = graph.broadcast_cell(cell.to(dev), n_mol).clone()
            self.inv_cell, self.volume = torch.empty_like(self.cell), torch.empty(n_mol, dtype=torch.float32, device=dev)
            self.g.set_periodic(edge_shift.to(dev), batch.to(dev), self.cell)
        self.g.csc()
        self.graph, out = _record(self._body, dev, max(1, warmup))
        self._keep(out)

    def _body(self):
        if self.cell is not None:
            graph.cell_prepare(self.cell, self.inv_cell, self.volume)
        self.g.set_positions(self.pos, self.cell)
        return energy_forces(self.cfg, self.pw, self.head, self.z32, self.g, self.mol_ptr, self.n_mol, self.volume)

    @torch.no_grad()
    def __call__(self, pos: torch.Tensor, cell: Optional[torch.Tensor] = None):
        """-> (energy, forces), or (energy, forces, stress) for a periodic step; ``cell``: a new cell for this and later steps."""
        if cell is not None:
            if self.cell is None:
                raise ValueError("CapturedStep: this step was recorded without a cell")
            if self.check_cell and self.images == "minimum":
                graph.check_cell(cell, float(self.cfg.cutoff))
            elif self.check_cell:
                graph.check_volume(cell)
            self.cell.copy_(graph.broadcast_cell(cell.to(self.cell.device), self.n_mol))
        self.pos.copy_(pos)
        self.graph.replay()
        return self._outputs()


class RebuiltStep(_StepOutputs):
    """Energy + forces with the neighbour list REBUILT inside the step: ``CapturedStep``'s counterpart for lists that change
    (liquids, hot molecules), still ONE hipGraph replay per step and no host read.

        step = RebuiltStep(EnergyForces(rep, head), z, batch, n_mol)             # or cell=, images= for periodic boxes
        energy, forces = step(pos)          # views of static output buffers: copy them to keep them
        step.edge_count                     # int32 [1] on the device: the real edges of the last step

    The list gets a fixed capacity (``graph.PaddedLayout``): ``n_pad`` dummy atoms of atomic number 0 in one extra molecule own
    the slots a step does not use, as self-loops with zero vector and distance.  The recorded chain is count (over the N real
    atoms) -> gn_degree_scan -> fill (E = capacity) -> gn_padded_tail -> gn_graph_refresh -> [gn_cell_prepare] -> geometry ->
    forward -> head -> backward -> force scatter -> [gn_virial]: kernel nodes only, on one stream.  The model runs on
    N + n_pad atoms and n_mol + 1 molecules; what is returned are the first n_mol energies (and stresses) and the first N
    forces.  No edge joins a dummy atom to a real one, so in the "f32" and "split" arithmetics these are the bits of
    ``EnergyForces`` on the unpadded list; "f16x2" shares block exponents between neighbouring rows and agrees to its usual
    1e-6 relative.  ``step.edge_index`` / ``step.edge_shift`` are the capacity-sized buffers.

    Periodic steps (``cell``, ``images`` as ``graph.distance_pbc``): the cell is FIXED unless ``cell_moves`` is set (below) -- the
    choice between the minimum-image and the multi-image kernels is a host decision -- and a cell passed per call is
    refused.  The dummy molecule gets the identity cell (volume 1, zero virial);
    ``step.cell`` is the [n_mol, 3, 3] view of the real boxes.

    ``cell_moves=True`` (opt-in; needs ``cell`` and ``images`` "all" or "auto"): the cell may change between two calls --
    ``step.set_cell(cell)``, or a kernel that writes ``step.cell`` (the barostat of ``md.MDRun``).  The step then always runs the
    multi-image kernels on a list of capacity sum_m n_m * max_num_neighbors, which holds for any image range, and owns the
    range array (int32 [n_mol, 3], initialised from ``graph.image_ranges``; all zero on a wide cell, where the multi-image walk
    is the minimum-image walk candidate for candidate).  The chain starts gn_cell_prepare -> gn_cell_image_ranges -> count: the
    inverse and the ranges belong to the current cell before the search reads them, and no second gn_cell_prepare follows
    the list.  A cell the range kernel refuses (no volume, or R > 3: a width below ``cutoff / 3.48``) keeps the old ranges, stores
    1 in ``step.reason`` [n_mol] (or the caller's ``reason`` tensor) and sets the sticky ``state`` word; the step still runs, and
    what it returns for such a cell means nothing.  A cell per call stays refused.  Without the keyword the step launches
    what it always launched, in the same order.

    ``capture=False``: the same launches on the same buffers, eagerly in every call (the reference of the recorded mode).
    ``state``: an int32 tensor whose first word gn_padded_tail sets when the edge count leaves the layout's bound (sticky;
    default: the step's own).  An inference tool, like ``CapturedStep``."""

    def __init__(self, ef: EnergyForces, z: torch.Tensor, batch: torch.Tensor, n_mol: int, max_num_neighbors: int = 32,
                 cell: Optional[torch.Tensor] = None, images: str = "minimum", warmup: int = 2, capture: bool = True,
                 state: Optional[torch.Tensor] = None, cell_moves: bool = False, reason: Optional[torch.Tensor] = None):
        rep, head = ef.rep, ef.head
        graph.check_periodic_args(cell, images)              # before any launch
        self.cell_moves = bool(cell_moves)
        if self.cell_moves and cell is None:
            raise ValueError("RebuiltStep: cell_moves=True needs a cell")
        if self.cell_moves and images == "minimum":
            raise ValueError('RebuiltStep: cell_moves=True with images="minimum": whether a moved cell is still at least '
                             '2 * cutoff wide is the host\'s decision; images="all" (or "auto") recomputes the image ranges on '
                             'the device')
        ranges = graph.resolve_images(cell, float(rep.cutoff), images) if cell is not None else None
        if self.cell_moves and ranges is None:                # "auto" on a wide cell: the multi-image kernels all the same
            ranges = graph.image_ranges(cell.detach().cpu(), float(rep.cutoff))
        dev = z.device
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.layout = lay = graph.PaddedLayout(batch, n_mol, max_num_neighbors, z=z, periodic_images=ranges is not None).to(dev)
        self.cfg, self.pw, self.head = rep.config(), rep.packed_weights(), head
        self.images, self.cutoff, self.max_num_neighbors = images, float(rep.cutoff), int(max_num_neighbors)
        self.N, self.n_mol, self.n_pad, self.capacity = lay.N, int(n_mol), lay.n_pad, lay.edge_capacity
        self.z32, self.mol_ptr = lay.z, lay.mol_ptr                      # the padded system: what the model runs on
        self.batch = batch.to(device=dev, dtype=torch.int64).contiguous()  # the real atoms: what the search runs on
        self._real_ptr = molecule_ptr(self.batch, self.n_mol)
        # every buffer of the chain is made and initialised here, by torch, never inside the recording
        self.pos = torch.zeros((self.N, 3), **f32)                      # static input buffer
        self.state = torch.zeros(1, **i32) if state is None else state
        self.edge_count = torch.zeros(1, **i32)
        self._deg, self._rowptr64 = torch.zeros(self.N, **i32), torch.zeros(self.N + 1, dtype=torch.int64, device=dev)
        self.edge_index = torch.zeros((2, self.capacity), dtype=torch.int64, device=dev)
        self.edge_vec, self.edge_diff = torch.zeros((self.capacity, 3), **f32), torch.zeros(self.capacity, **f32)
        self.edge_shift = self.cell = self._cell_all = self.inv_cell = self.volume = self._ranges = None
        if cell is not None:
            self.edge_shift = torch.zeros((self.capacity, 3), **i32)
            self._cell_all = torch.cat([graph.broadcast_cell(cell.to(dev), self.n_mol), torch.eye(3, **f32).unsqueeze(0)])
            self.cell = self._cell_all[:self.n_mol]                     # a view: the driver's [n_mol, 3, 3] cell
            self.inv_cell, self.volume = graph.cell_prepare(self._cell_all)     # (the search reads the inverse before step 6)
            self._ranges = None if ranges is None else ranges.expand(self.n_mol, 3).contiguous().to(dev)
        #: ``cell_moves``: why a box set the sticky word (1: gn_cell_image_ranges refused its cell), int32 [n_mol]
        self.reason = (torch.zeros(self.n_mol, **i32) if reason is None else reason) if self.cell_moves else None
        self.g = engine.Graph(self.cfg, self.pw, lay.n_atoms, self.edge_index, self_images=cell is not None)
        self.energy = self.forces = self.stress = self.graph = None
        if capture:
            self.graph, out = _record(self._body, dev, max(1, warmup))
            self._keep(out)

    def rebuild(self):
        """Steps 1 to 5 of the chain: the list of ``self.pos`` into the capacity-sized buffers, and the graph's topology."""
        graph.rebuild_padded(self.pos, self.batch, self._real_ptr, self.n_mol, self.cutoff, self.max_num_neighbors, self.n_pad,
                             self._deg, self._rowptr64, self.edge_count, self.edge_index, self.edge_shift, self.edge_vec,
                             self.edge_diff, self.state, cell=self._cell_all, inv_cell=self.inv_cell, image_range=self._ranges)
        self.g.refresh(self.edge_index)

    def model(self):
        """The whole chain, launched eagerly: (energy, forces[, stress]) of ``self.pos``."""
        return RebuiltStep._body(self)

    def _body(self):
        if self.cell_moves:       # the inverse and the ranges of the CURRENT cell, before the count reads them
            graph.cell_prepare(self._cell_all, self.inv_cell, self.volume)
            call("gn_cell_image_ranges", ptr(self.cell), self.n_mol, self.cutoff, graph.MAX_IMAGE_RANGE, ptr(self._ranges),
                 ptr(self.state), ptr(self.reason), engine._stream())
        self.rebuild()
        if self.cell is not None and not self.cell_moves:
            graph.cell_prepare(self._cell_all, self.inv_cell, self.volume)
        self.g.set_geometry(self.edge_diff, self.edge_vec)     # (the fill's unshifted() / shifted(): the bits set_positions would give)
        # the padded system: n_mol + 1 molecules, the dummy atoms behind the N real ones; what leaves is the real part
        e, f, *stress = energy_forces(self.cfg, self.pw, self.head, self.z32, self.g, self.mol_ptr, self.n_mol + 1, self.volume)
        return (e[:self.n_mol], f[:self.N], *(s[:self.n_mol] for s in stress))

    @torch.no_grad()
    def set_cell(self, cell: torch.Tensor) -> None:
        """``cell_moves=True``: copy a new cell (fp32 [n_mol, 3, 3] or [3, 3]) into the static buffer; the next call prepares it,
        recomputes its image ranges and searches in it.  Not checked on the host: a cell the range kernel refuses sets the
        sticky ``state`` word and ``reason`` of its box."""
        graph.check_periodic_args(cell)                       # before any launch
        if not self.cell_moves:
            raise ValueError("RebuiltStep.set_cell: this step was built for a fixed cell; pass cell_moves=True")
        self.cell.copy_(graph.broadcast_cell(cell.to(self.cell.device), self.n_mol))

    @torch.no_grad()
    def __call__(self, pos: torch.Tensor, cell: Optional[torch.Tensor] = None):
        """-> (energy [n_mol, 1], forces [N, 3]), plus stress [n_mol, 3, 3] for a periodic step."""
        if cell is not None:
            raise ValueError("RebuiltStep: the cell is fixed at construction (its image ranges are a host decision); a cell "
                             "per call is refused -- use CapturedStep for a moving cell")
        self.pos.copy_(pos)
        if self.graph is not None:
            self.graph.replay()
        else:
            self._keep(self._body())
        return self._outputs()
