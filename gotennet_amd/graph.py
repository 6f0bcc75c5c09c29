"""Radius graph + edge vectors on the device (reference Distance.forward,
gotennet/models/components/layers.py:1566-1604, over torch_cluster.radius_graph).

Kernels: csrc/gn_graph.hip.  The only host work is the exclusive scan of the
per-target degrees and the read-back of the edge count needed to size the
outputs (one sync, as in torch_cluster).

``PaddedLayout`` is host-side index arithmetic only: the fixed sizes a radius graph needs
to be rebuilt on the device without that read-back.  ``rebuild_padded`` is that rebuild: the
searches' own count and fill kernels around a device scan, then the inert tail
(``pipeline.RebuiltStep`` records it in front of the model)."""
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
    search = (ptr(pos), ptr(batch), N, float(cutoff), int(max_num_neighbors))
    return _count_and_fill("", search, N, pos.device, shifts=False)[:3]


def _count_and_fill(entry: str, search: tuple, N: int, device, shifts: bool):
    """The host sequence of every search, gn_radius_count<entry> / gn_radius_fill<entry>: count, exclusive scan, ONE read of
    the edge count, allocate, fill -> (edge_index, edge_diff, edge_vec, edge_shift or None).  ``search``: the arguments the
    two entry points share, up to and including the cap."""
    st = torch.cuda.current_stream().cuda_stream
    deg = torch.empty(N, dtype=torch.int32, device=device)
    call("gn_radius_count" + entry, *search, ptr(deg), st)
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=device)
    torch.cumsum(deg, 0, out=rowptr[1:])
    E = int(rowptr[-1].item()) if N else 0
    edge_index = torch.empty((2, E), dtype=torch.int64, device=device)
    edge_shift = torch.empty((E, 3), dtype=torch.int32, device=device) if shifts else None
    edge_vec = torch.empty((E, 3), dtype=torch.float32, device=device)
    edge_diff = torch.empty(E, dtype=torch.float32, device=device)
    outs = (ptr(edge_index),) + ((ptr(edge_shift),) if shifts else ()) + (ptr(edge_vec), ptr(edge_diff))
    call("gn_radius_fill" + entry, *search, ptr(rowptr), E, *outs, st)
    return edge_index, edge_diff, edge_vec, edge_shift



# ---------------------------------------------------------------------------------------- periodic boundary conditions
# Conventions (include/gotennet_hip.h): ``cell`` fp32 [n_mol, 3, 3] (a [3, 3] cell is broadcast), ROWS are the lattice vectors,
# one cell per entry of ``batch`` -- a "molecule" is a periodic box; ``edge_shift`` int32 [E, 3];
# edge_vec[e] = pos[j] - pos[i] + edge_shift[e] @ cell[batch[i]].
def cell_widths(cell: torch.Tensor) -> torch.Tensor:
    """fp64 [n_mol, 3]: the perpendicular widths V / |a_j x a_k| of every cell (width k is the distance between the two faces
    spanned by the other two lattice vectors).  Plain torch, CPU tensors welcome."""
    c = cell.detach().to(torch.float64).reshape(-1, 3, 3)
    a, b, cc = c[:, 0], c[:, 1], c[:, 2]
    vol = (a * torch.cross(b, cc, dim=1)).sum(1).abs()
    faces = torch.stack([torch.cross(b, cc, dim=1), torch.cross(cc, a, dim=1), torch.cross(a, b, dim=1)], dim=1)
    return vol.unsqueeze(1) / faces.norm(dim=2)


def check_cell(cell: torch.Tensor, cutoff: float) -> torch.Tensor:
    """Raise ``ValueError`` unless every perpendicular width of every cell is at least ``2 * cutoff`` (the minimum-image
    condition: at most one image of a pair inside the cutoff, no atom sees an image of itself).  On the host in fp64, from
    one read of ``cell``; returns the widths."""
    if cell.dim() not in (2, 3) or tuple(cell.shape[-2:]) != (3, 3):
        raise ValueError("cell must be [n_mol, 3, 3] or [3, 3] (rows = lattice vectors)")
    w = cell_widths(cell.detach().cpu())
    if not bool(torch.isfinite(w).all()) or bool((w < 2.0 * float(cutoff)).any()):
        m = int(torch.where(torch.isfinite(w), w, torch.full_like(w, -1.0)).min(dim=1).values.argmin())
        raise ValueError(f"cell {m}: perpendicular widths {[round(float(x), 4) for x in w[m]]} are not all >= 2 * cutoff = "
                         f"{2.0 * float(cutoff)}: only the minimum image is supported (one image per pair, no self-images)")
    return w


#: slack of the image range (``image_ranges``).  The kernel rounds the fractional difference f in fp32, so the image it
#: centres the search on can be the second-nearest one when f lies within its rounding error of a half-integer:
#: |f_k - rint(f_k)| <= 1/2 + err.  err is a few ulps of |f| times the condition number of the cell (f = d @ inv_cell with an
#: fp32 inverse): below 1/64 for |f| * cond up to ~1e4, i.e. atoms unwrapped by thousands of cells.  A slack that is too
#: large costs candidates, never edges; 1/64 keeps R = 0 for widths above 2.07 * cutoff and R <= 3 down to cutoff / 3.
IMAGE_SLACK = 2.0 ** -6
MAX_IMAGE_RANGE = 3          # GN_PBC_MAX_IMAGE_RANGE: at most 7^3 images per pair


def image_ranges(cell: torch.Tensor, cutoff: float) -> torch.Tensor:
    """The relaxed cell check of the multi-image radius graph -> R int32 [n_mol, 3] (CPU): per box and axis the range of
    images around the rounded fractional difference that can hold a neighbour, R_k = floor(cutoff / w_k + 1/2 + IMAGE_SLACK)
    with w_k the perpendicular width.  (An image vector v with fractional coordinate g_k along axis k has |v| >= |g_k| w_k,
    and g_k = f_k - rint(f_k) + t_k with |f_k - rint(f_k)| <= 1/2: inside the cutoff means |t_k| < cutoff / w_k + 1/2.)
    On the host in fp64, from one read of ``cell``.  Raises ``ValueError`` for a width that is not finite and positive or is
    below ``cutoff / 3`` (R_k would exceed 3: more than 343 images per pair)."""
    if cell.dim() not in (2, 3) or tuple(cell.shape[-2:]) != (3, 3):
        raise ValueError("cell must be [n_mol, 3, 3] or [3, 3] (rows = lattice vectors)")
    w = cell_widths(cell.detach().cpu())
    ok = torch.isfinite(w) & (w > 0)
    if not bool(ok.all()) or bool((w < float(cutoff) / 3.0).any()):
        m = int(torch.where(ok, w, torch.full_like(w, -1.0)).min(dim=1).values.argmin())
        raise ValueError(f"cell {m}: perpendicular widths {[round(float(x), 4) for x in w[m]]} are not all finite and >= "
                         f"cutoff / 3 = {float(cutoff) / 3.0}: at most {2 * MAX_IMAGE_RANGE + 1} images per axis are searched")
    return torch.floor(float(cutoff) / w + 0.5 + IMAGE_SLACK).to(torch.int32).clamp_(max=MAX_IMAGE_RANGE)


def check_volume(cell: torch.Tensor) -> None:
    """Raise ``ValueError`` unless every cell has a finite, non-zero volume: all a FIXED periodic edge list asks of a new cell
    (its stored shifts stay valid while the cell deforms).  One host read of ``cell``."""
    if cell.dim() not in (2, 3) or tuple(cell.shape[-2:]) != (3, 3):
        raise ValueError("cell must be [n_mol, 3, 3] or [3, 3] (rows = lattice vectors)")
    c = cell.detach().cpu().to(torch.float64).reshape(-1, 3, 3)
    vol = (c[:, 0] * torch.cross(c[:, 1], c[:, 2], dim=1)).sum(1)          # a . (b x c), as cell_widths
    if not bool(torch.isfinite(c).all()) or not bool(torch.isfinite(vol).all()) or bool((vol == 0).any()):
        raise ValueError(f"cell volumes {[float(v) for v in vol]}: every cell needs a finite, non-zero volume")


def broadcast_cell(cell: torch.Tensor, n_mol: int) -> torch.Tensor:
    """fp32 contiguous [n_mol, 3, 3] (a [3, 3] cell repeated for every box)."""
    cell = cell.detach().to(torch.float32)
    if cell.dim() == 2:
        cell = cell.unsqueeze(0).expand(n_mol, 3, 3)
    if tuple(cell.shape) != (n_mol, 3, 3):
        raise ValueError(f"cell must be [{n_mol}, 3, 3] or [3, 3], got {tuple(cell.shape)}")
    return cell.contiguous()


def cell_prepare(cell: torch.Tensor, inv_cell: Optional[torch.Tensor] = None, volume: Optional[torch.Tensor] = None):
    """-> (inv_cell [n_mol, 3, 3], volume [n_mol]) of a contiguous fp32 [n_mol, 3, 3] cell (gn_cell_prepare; into the given
    buffers when passed)."""
    n_mol = cell.shape[0]
    if inv_cell is None:
        inv_cell, volume = torch.empty_like(cell), torch.empty(n_mol, dtype=torch.float32, device=cell.device)
    call("gn_cell_prepare", ptr(cell), n_mol, ptr(inv_cell), ptr(volume), torch.cuda.current_stream().cuda_stream)
    return inv_cell, volume


def default_n_mol(batch: torch.Tensor, cell: Optional[torch.Tensor] = None) -> int:
    """The number of molecules when the caller names none: one per cell of a [n_mol, 3, 3] ``cell``, else from the last entry
    of ``batch`` (a host read)."""
    if cell is not None and cell.dim() == 3:
        return cell.shape[0]
    return int(batch[-1].item()) + 1 if batch.shape[0] else 0


def box_arrays(cell: torch.Tensor, ranges: Optional[torch.Tensor], n_mol: int, device):
    """What the periodic kernels read per box, on ``device`` -> (cell fp32 [n_mol, 3, 3], its inverse (gn_cell_prepare), the
    image range int32 [n_mol, 3] or None).  ``ranges``: ``resolve_images``' result."""
    cell = broadcast_cell(cell.to(device), n_mol)
    return cell, cell_prepare(cell)[0], None if ranges is None else ranges.expand(n_mol, 3).contiguous().to(device)


IMAGE_MODES = ("minimum", "auto", "all")


def check_periodic_args(cell: Optional[torch.Tensor] = None, images: str = "minimum") -> None:
    """The two refusals every periodic entry point of the step classes and the drivers makes before any launch, stated once:
    a ``cell`` that requires grad, then an unknown ``images``.  Raises ``ValueError``; reads nothing on the device."""
    if cell is not None and cell.requires_grad:
        raise ValueError("cell requires grad: autograd with respect to the cell is not supported")
    if images not in IMAGE_MODES:
        raise ValueError(f"images must be one of {IMAGE_MODES}, got {images!r}")


def resolve_images(cell: torch.Tensor, cutoff: float, images: str) -> Optional[torch.Tensor]:
    """The cell check of ``distance_pbc(images=)``, from ONE host read of ``cell`` -> None (the minimum-image kernels: every
    box passed ``check_cell``) or the ``image_ranges`` array (the multi-image kernels).  Raises what those checks raise."""
    check_periodic_args(images=images)
    cell_host = cell.detach().cpu()
    if images == "all":
        return image_ranges(cell_host, cutoff)
    try:
        check_cell(cell_host, cutoff)
        return None
    except ValueError:
        if images == "minimum":
            raise
    return image_ranges(cell_host, cutoff)


def distance_pbc(pos: torch.Tensor, batch: torch.Tensor, cell: torch.Tensor, cutoff: float, max_num_neighbors: int = 32,
                 n_mol: Optional[int] = None, check: bool = True, images: str = "minimum",
                 image_range: Optional[torch.Tensor] = None):
    """``distance`` under periodic boundary conditions -> (edge_index, edge_diff, edge_vec, edge_shift): the same neighbour
    rule (target-major, sources ascending, strict d^2 < r^2 in fp32, the first ``max_num_neighbors`` hits, the self-loop
    inside the cap) over the periodic images of each box's atoms; edge_shift int32 [E, 3] with
    edge_vec = pos[j] - pos[i] + edge_shift @ cell[batch[i]].  Positions need not be wrapped into the cell.  ``batch`` must be
    non-decreasing (each box's atoms contiguous, as for ``distance``): it is not checked here, and a target's sources are the
    atom range of its box, so an unsorted vector gives a wrong list (in bounds, without an error).

    ``images`` selects the search:
      "minimum" (default)  one image per pair.  Cells narrower than ``2 * cutoff`` raise ``ValueError`` before any
                radius-graph launch (``check_cell``).
      "all"     every image inside the cutoff (gn_radius_*_pbc_images): cells down to ``cutoff / 3`` wide
                (``image_ranges``; narrower or non-finite ones raise ``ValueError`` before any launch).  Within a (target,
                source) pair the images ascend lexicographically in the shift; the cap keeps a target's first hits in
                (source, image) order.  An atom's own images are edges with ``src == dst`` and a non-zero shift,
                ``edge_diff`` > 0: the self-loop is the edge with ``src == dst`` AND ``edge_diff == 0``, and whoever consumes
                the list must use that rule (``EnergyForces(cell=)`` does; ``GotenNet.forward(self_images=True)``).
                On cells of width >= ``2 * cutoff`` the result is the "minimum" list, bit for bit.
      "auto"    "minimum" (same launches, same bits) when every box passes ``check_cell``, "all" for the whole batch otherwise.
    Either way the host reads ``cell`` once and the edge count once, as ``distance`` reads the count.  ``n_mol``: the number
    of boxes when a [3, 3] cell is broadcast (default: read from the last entry of ``batch``).  ``check=False``: the caller
    has run ``resolve_images`` on this cell and cutoff and passes what it returned as ``image_range`` (None: the minimum
    image); ``images`` is then not looked at and the cell is not read here."""
    if not pos.is_cuda:
        raise GotenNetHipError("gotennet_amd.graph.distance_pbc runs on a ROCm device only (no CPU fallback)")
    if cell.requires_grad:
        raise ValueError("cell requires grad: autograd with respect to the cell is not supported (stress comes from "
                         "EnergyForces / CapturedStep)")
    ranges = resolve_images(cell, cutoff, images) if check else image_range
    from .outputs import molecule_ptr
    pos = pos.detach().to(torch.float32).contiguous()
    batch = batch.to(torch.int64).contiguous()
    N = pos.shape[0]
    if n_mol is None:
        n_mol = default_n_mol(batch, cell)
    cell, inv_cell, ranges = box_arrays(cell, ranges, n_mol, pos.device)
    mol_ptr = molecule_ptr(batch, n_mol)
    box = (ptr(cell), ptr(inv_cell)) if ranges is None else (ptr(cell), ptr(inv_cell), ptr(ranges))
    search = (ptr(pos), ptr(batch), ptr(mol_ptr), *box, N, n_mol, float(cutoff), int(max_num_neighbors))
    return _count_and_fill("_pbc" if ranges is None else "_pbc_images", search, N, pos.device, shifts=True)


def verify_list(pos, batch, mol_ptr, n_mol: int, rowptr, src, cutoff: float, max_num_neighbors: int, row_flag, changed, state,
                shift=None, cell=None, inv_cell=None, image_range=None) -> None:
    """gn_radius_verify* on prepared device arrays, no allocation and no host read (what a recorded MD step launches): the
    stored list in CSR form (``rowptr`` int32 [N + 1], ``src`` int32 [E], ``shift`` int32 [E, 3] for a periodic list) against the
    radius graph of ``pos``.  Writes ``row_flag`` [N], ``changed`` [n_mol] and sets the sticky ``state[0]`` when a row differs.
    ``cell`` None: the open search; ``image_range`` None: the minimum-image search; else the multi-image one."""
    N, E = pos.shape[0], src.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    tail = (ptr(row_flag), ptr(changed), ptr(state), st)
    if cell is None:
        call("gn_radius_verify", ptr(pos), ptr(batch), ptr(mol_ptr), N, n_mol, float(cutoff), int(max_num_neighbors),
             ptr(rowptr), ptr(src), E, *tail)
        return
    box = (ptr(cell), ptr(inv_cell)) if image_range is None else (ptr(cell), ptr(inv_cell), ptr(image_range))
    call("gn_radius_verify_pbc" + ("" if image_range is None else "_images"), ptr(pos), ptr(batch), ptr(mol_ptr), *box, N, n_mol,
         float(cutoff), int(max_num_neighbors), ptr(rowptr), ptr(src), ptr(shift), E, *tail)


def list_is_current(pos: torch.Tensor, batch: torch.Tensor, edge_index: torch.Tensor, cutoff: float,
                    max_num_neighbors: int = 32, cell: Optional[torch.Tensor] = None,
                    edge_shift: Optional[torch.Tensor] = None, images: str = "minimum", n_mol: Optional[int] = None,
                    state: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Is ``edge_index`` (and ``edge_shift``) still what ``distance`` / ``distance_pbc`` would return for ``pos``?  ->
    ``changed`` int32 [n_mol]: the number of targets of each molecule whose row of the list differs (all zero: the list is
    current, to the bit at the threshold -- the check runs the searches' own predicates in their own order, cap included).
    No list is built and nothing is read back: the result stays on the device.

    ``edge_index`` must be target-major, as the searches return it.  ``cell`` / ``edge_shift`` / ``images`` as for
    ``distance_pbc`` (the cell is checked the same way, one host read).  ``n_mol``: default from ``cell`` or the last entry of
    ``batch`` (a host read).  ``state``: an int32 tensor whose first word is set to 1 when any row differs and is never
    cleared here (the sticky word the MD integrator kernels are predicated on).  ``out``: an int32 [n_mol] result buffer."""
    if not pos.is_cuda:
        raise GotenNetHipError("gotennet_amd.graph.list_is_current runs on a ROCm device only (no CPU fallback)")
    if (cell is None) != (edge_shift is None):
        raise ValueError("list_is_current: a periodic list needs both cell and edge_shift; neither for isolated molecules")
    ranges = resolve_images(cell, cutoff, images) if cell is not None else None
    from .outputs import molecule_ptr
    dev = pos.device
    pos = pos.detach().to(torch.float32).contiguous()
    batch = batch.to(torch.int64).contiguous()
    N, E = pos.shape[0], edge_index.shape[1]
    if n_mol is None:
        n_mol = default_n_mol(batch, cell)
    i32 = dict(dtype=torch.int32, device=dev)
    src, dst, rowptr = torch.empty(E, **i32), torch.empty(E, **i32), torch.empty(N + 1, **i32)
    st = torch.cuda.current_stream().cuda_stream
    call("gn_build_csr", ptr(edge_index.contiguous()), E, N, ptr(src), ptr(dst), ptr(rowptr), st)
    changed = torch.empty(n_mol, **i32) if out is None else out
    state = torch.zeros(1, **i32) if state is None else state
    kw = {}
    if cell is not None:
        cell, inv_cell, ranges = box_arrays(cell, ranges, n_mol, dev)
        kw = dict(shift=edge_shift.to(torch.int32).contiguous(), cell=cell, inv_cell=inv_cell, image_range=ranges)
    verify_list(pos, batch, molecule_ptr(batch, n_mol), n_mol, rowptr, src, cutoff, max_num_neighbors,
                torch.empty(N, **i32), changed, state, **kw)
    return changed


class PaddedLayout:
    """Fixed sizes for a radius graph that is rebuilt on the device -- an MD step recorded into one hipGraph whose neighbour
    list changes (host work, once per trajectory: the molecule sizes are read here).  The layout only; ``rebuild_padded``
    launches the kernels that fill such a list.

    ``e_bound`` = sum_m n_m * min(n_m, max_num_neighbors) bounds the edge count of ANY positions (gn_radius_count counts
    the self-loop inside the cap), so an edge list of that capacity cannot overflow.  The slots a step does not use must
    still be edges of something: ``n_pad`` = max(1, ceil((e_bound - N) / pad_degree)) dummy atoms (atomic number 0, the
    embeddings' ``padding_idx``) are appended behind the real ones, all in one extra molecule ``n_mol``, and the tail of the
    list -- ``edge_capacity`` - E_real >= n_pad slots, ``edge_capacity`` = e_bound + n_pad -- is dealt to them as self-loops with
    zero vector and distance, in a balanced contiguous partition (``tail_degrees``): the list stays target-major, every dummy
    row holds between 1 and ``pad_degree`` + 1 edges.  No edge joins a dummy atom to a real one: real rows see what they see
    in the unpadded graph.

    ``periodic_images=True``: the list comes from a multi-image search (``distance_pbc(images="all")``), where one pair can
    contribute several edges and an atom sees its own images, so a molecule of n atoms fills every row up to the cap
    whatever n is: ``e_bound`` = sum_m n_m * max_num_neighbors.  Open and minimum-image lists hold one edge per pair and keep
    the bound above.

    Provides ``batch`` (int64 [n_atoms]) and ``mol_ptr`` (int32 [n_mol + 2]) of the padded system, and ``z`` (int32
    [n_atoms]) when the atomic numbers are passed (``pad_z`` otherwise): call the engine with ``n_mol + 1`` molecules and
    keep ``energy[:n_mol]``, ``forces[:N]``."""

    def __init__(self, batch: torch.Tensor, n_mol: int, max_num_neighbors: int = 32, pad_degree: Optional[int] = None,
                 z: Optional[torch.Tensor] = None, periodic_images: bool = False):
        from .outputs import molecule_ptr
        self.n_mol, self.max_num_neighbors = int(n_mol), int(max_num_neighbors)
        self.periodic_images = bool(periodic_images)
        self.pad_degree = int(pad_degree) if pad_degree is not None else self.max_num_neighbors
        if self.n_mol < 1 or self.max_num_neighbors < 1 or self.pad_degree < 1:
            raise ValueError("PaddedLayout needs n_mol, max_num_neighbors and pad_degree >= 1")
        batch = batch.to(torch.int64).contiguous()
        self.N = N = batch.shape[0]
        b = batch.cpu()
        if N == 0 or int(b.min()) < 0 or int(b.max()) >= self.n_mol or bool((b[1:] < b[:-1]).any()):
            raise ValueError("batch must be non-empty, non-decreasing and hold molecule indices in [0, n_mol)")
        self.sizes = torch.bincount(b, minlength=self.n_mol).tolist()
        self.e_bound = sum(n * (self.max_num_neighbors if self.periodic_images else min(n, self.max_num_neighbors))
                           for n in self.sizes)
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


def rebuild_padded(pos, batch, mol_ptr, n_mol: int, cutoff: float, max_num_neighbors: int, n_pad: int, deg, rowptr64,
                   edge_count, edge_index, edge_shift, edge_vec, edge_diff, state, cell=None, inv_cell=None,
                   image_range=None) -> None:
    """The radius graph of the N real atoms ``pos`` into a list of fixed capacity (``PaddedLayout``: ``edge_index`` int64
    [2, capacity], ``edge_shift`` int32 [capacity, 3] or None, ``edge_vec`` [capacity, 3], ``edge_diff`` [capacity]), on prepared
    device arrays: count -> gn_degree_scan -> fill with E = capacity -> gn_padded_tail.  Four kernel launches, no allocation,
    no memset and no host read -- what a recorded step launches.  Columns [0, E_real) are ``distance`` / ``distance_pbc``'s, bit
    for bit (the same walk, the same sinks); E_real lands in ``edge_count`` int32 [1]; the tail belongs to the dummy atoms
    N .. N + n_pad - 1.  ``deg`` int32 [N] and ``rowptr64`` int64 [N + 1] are scratch; ``state[0]`` is set when the count leaves
    the layout's bound.  ``cell`` None: the open search; ``image_range`` None: the minimum-image search; else the multi-image one."""
    N, capacity = pos.shape[0], edge_index.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    if cell is None:
        entry, search, outs = "", (ptr(pos), ptr(batch), N, float(cutoff), int(max_num_neighbors)), (ptr(edge_index),)
    else:
        box = (ptr(cell), ptr(inv_cell)) if image_range is None else (ptr(cell), ptr(inv_cell), ptr(image_range))
        entry = "_pbc" if image_range is None else "_pbc_images"
        search = (ptr(pos), ptr(batch), ptr(mol_ptr), *box, N, n_mol, float(cutoff), int(max_num_neighbors))
        outs = (ptr(edge_index), ptr(edge_shift))
    call("gn_radius_count" + entry, *search, ptr(deg), st)
    call("gn_degree_scan", ptr(deg), N, ptr(rowptr64), ptr(edge_count), st)
    call("gn_radius_fill" + entry, *search, ptr(rowptr64), capacity, *outs, ptr(edge_vec), ptr(edge_diff), st)
    call("gn_padded_tail", ptr(rowptr64), N, int(n_pad), capacity, ptr(edge_index), ptr(edge_shift) if cell is not None else None,
         ptr(edge_vec), ptr(edge_diff), ptr(state), st)
