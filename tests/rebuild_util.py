"""The padded neighbour list of a device-rebuilt step, restated in plain torch on the CPU; shares no code with
``gotennet_amd``.

A list of ``capacity`` slots holds the E real edges first; the P = capacity - E slots behind them are self-loops of the
``n_pad`` dummy atoms N .. N + n_pad - 1 (shift, vector and distance zero), dealt in a balanced contiguous partition: with
q = P // n_pad and r = P % n_pad the first r dummies own q + 1 slots each, the others q."""
import torch


def tail_owner(N: int, n_pad: int, capacity: int, n_edges: int) -> torch.Tensor:
    """int64 [capacity - n_edges]: the dummy atom that owns each tail slot, in closed form per slot (no loop over dummies,
    no cumulative sum): slot t < r (q + 1) belongs to dummy t // (q + 1), a later one to r + (t - r (q + 1)) // q."""
    P = capacity - n_edges
    assert n_pad >= 1 and P >= n_pad, "the layout leaves at least one slot per dummy atom"
    q, r = P // n_pad, P % n_pad
    t = torch.arange(P, dtype=torch.int64)
    head = r * (q + 1)
    k = torch.where(t < head, t // (q + 1), r + (t - head).clamp(min=0) // q)
    return N + k


def padded_list(N: int, n_pad: int, capacity: int, edge_index, edge_vec, edge_diff, edge_shift=None):
    """The real list (edge_index int64 [2, E], edge_vec [E, 3], edge_diff [E], edge_shift int32 [E, 3] or None) followed by
    its inert tail -> (edge_index [2, capacity], edge_vec, edge_diff, edge_shift or None), on the inputs' device."""
    E, dev = edge_index.shape[1], edge_index.device
    own = tail_owner(N, n_pad, capacity, E).to(dev)
    P = own.shape[0]
    ei = torch.cat([edge_index, torch.stack([own, own])], dim=1).contiguous()
    ev = torch.cat([edge_vec, torch.zeros((P, 3), dtype=edge_vec.dtype, device=dev)]).contiguous()
    ed = torch.cat([edge_diff, torch.zeros(P, dtype=edge_diff.dtype, device=dev)]).contiguous()
    sh = None if edge_shift is None else torch.cat([edge_shift, torch.zeros((P, 3), dtype=edge_shift.dtype, device=dev)]).contiguous()
    return ei, ev, ed, sh
