"""Radius graph + edge vectors on the device (reference Distance.forward,
gotennet/models/components/layers.py:1566-1604, over torch_cluster.radius_graph).

Kernels: csrc/gn_graph.hip.  The only host work is the exclusive scan of the
per-target degrees and the read-back of the edge count needed to size the
outputs (one sync, as in torch_cluster).

``PaddedLayout`` is host-side index arithmetic only: the fixed sizes a radius graph needs
to be rebuilt on the device without that read-back (no kernel consumes it yet)."""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import GotenNetHipError, call, ptr


def distance(pos: torch.Tensor, batch: torch.Tensor, cutoff: float, max_num_neighbors: int = 32):
    """-> edge_index int64 [2,E] (row 0 = source j, row 1 = target i; target-major, sources
    ascending, self-loops included), edge_weight [E] (0 on self-loops), edge_vec [E,3] = pos[j]-pos[i]."""
    if not pos.is_cuda:
        raise GotenNetHipError("gotennet_amd.graph.distance runs on a ROCm device only (no CPU fallback)")
    pos = pos.detach().to(torch.float32).contiguous()
    batch = batch.to(torch.int64).contiguous()
    N = pos.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    deg = torch.empty(N, dtype=torch.int32, device=pos.device)
    call("gn_radius_count", ptr(pos), ptr(batch), N, float(cutoff), int(max_num_neighbors), ptr(deg), st)
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=pos.device)
    torch.cumsum(deg, 0, out=rowptr[1:])
    E = int(rowptr[-1].item()) if N else 0
    edge_index = torch.empty((2, E), dtype=torch.int64, device=pos.device)
    edge_vec = torch.empty((E, 3), dtype=torch.float32, device=pos.device)
    edge_diff = torch.empty(E, dtype=torch.float32, device=pos.device)
    call("gn_radius_fill", ptr(pos), ptr(batch), N, float(cutoff), int(max_num_neighbors), ptr(rowptr), E,
         ptr(edge_index), ptr(edge_vec), ptr(edge_diff), st)
    return edge_index, edge_diff, edge_vec


class PaddedLayout:
    """Fixed sizes for a radius graph that is rebuilt on the device -- an MD step recorded into one hipGraph whose neighbour
    list changes (host work, once per trajectory: the molecule sizes are read here).  The layout only; the kernels that
    fill such a list are not part of the library yet.

    ``e_bound`` = sum_m n_m * min(n_m, max_num_neighbors) bounds the edge count of ANY positions (gn_radius_count counts
    the self-loop inside the cap), so an edge list of that capacity cannot overflow.  The slots a step does not use must
    still be edges of something: ``n_pad`` = max(1, ceil((e_bound - N) / pad_degree)) dummy atoms (atomic number 0, the
    embeddings' ``padding_idx``) are appended behind the real ones, all in one extra molecule ``n_mol``, and the tail of the
    list -- ``edge_capacity`` - E_real >= n_pad slots, ``edge_capacity`` = e_bound + n_pad -- is dealt to them as self-loops with
    zero vector and distance, in a balanced contiguous partition (``tail_degrees``): the list stays target-major, every dummy
    row holds between 1 and ``pad_degree`` + 1 edges.  No edge joins a dummy atom to a real one: real rows see what they see
    in the unpadded graph.

    Provides ``batch`` (int64 [n_atoms]) and ``mol_ptr`` (int32 [n_mol + 2]) of the padded system, and ``z`` (int32
    [n_atoms]) when the atomic numbers are passed (``pad_z`` otherwise): call the engine with ``n_mol + 1`` molecules and
    keep ``energy[:n_mol]``, ``forces[:N]``."""

    def __init__(self, batch: torch.Tensor, n_mol: int, max_num_neighbors: int = 32, pad_degree: Optional[int] = None,
                 z: Optional[torch.Tensor] = None):
        from .outputs import molecule_ptr
        self.n_mol, self.max_num_neighbors = int(n_mol), int(max_num_neighbors)
        self.pad_degree = int(pad_degree) if pad_degree is not None else self.max_num_neighbors
        if self.n_mol < 1 or self.max_num_neighbors < 1 or self.pad_degree < 1:
            raise ValueError("PaddedLayout needs n_mol, max_num_neighbors and pad_degree >= 1")
        batch = batch.to(torch.int64).contiguous()
        self.N = N = batch.shape[0]
        b = batch.cpu()
        if N == 0 or int(b.min()) < 0 or int(b.max()) >= self.n_mol or bool((b[1:] < b[:-1]).any()):
            raise ValueError("batch must be non-empty, non-decreasing and hold molecule indices in [0, n_mol)")
        self.sizes = torch.bincount(b, minlength=self.n_mol).tolist()
        self.e_bound = sum(n * min(n, self.max_num_neighbors) for n in self.sizes)
        self.n_pad = max(1, -(-(self.e_bound - N) // self.pad_degree))
        self.edge_capacity = self.e_bound + self.n_pad
        self.n_atoms = N + self.n_pad
        self.batch = torch.cat([batch, torch.full((self.n_pad,), self.n_mol, dtype=torch.int64, device=batch.device)])
        self.mol_ptr = molecule_ptr(self.batch, self.n_mol + 1)
        self.z = self.pad_z(z) if z is not None else None

    def to(self, device) -> "PaddedLayout":
        """Move the layout's tensors to ``device`` (in place; nothing happens when they are there)."""
        if self.batch.device != torch.device(device):
            self.batch, self.mol_ptr = self.batch.to(device), self.mol_ptr.to(device)
            self.z = self.z.to(device) if self.z is not None else None
        return self

    def pad_z(self, z: torch.Tensor) -> torch.Tensor:
        """int32 [n_atoms]: ``z`` followed by the dummy atoms' 0."""
        if z.shape[0] != self.N:
            raise ValueError(f"z holds {z.shape[0]} atoms, the layout {self.N}")
        return torch.cat([z.to(torch.int32), torch.zeros(self.n_pad, dtype=torch.int32, device=z.device)])

    def tail_degrees(self, n_edges: int):
        """Edges of each dummy atom when the real list holds ``n_edges``: the balanced contiguous partition of the tail."""
        P = self.edge_capacity - int(n_edges)
        if not self.n_pad <= P <= self.edge_capacity - self.N:
            raise ValueError(f"{n_edges} edges: outside [{self.N}, {self.e_bound}]")
        base, rem = divmod(P, self.n_pad)
        return [base + (1 if k < rem else 0) for k in range(self.n_pad)]
