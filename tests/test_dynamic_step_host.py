"""Host: the padded layout of a device-rebuilt neighbour list (graph.PaddedLayout) -- its sizes, its bound and its tail
partition.  No GPU."""
import pytest
import torch


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _brute_force_edges(pos, sizes, cutoff, cap):
    """Edge count of radius_graph(loop=True, max_num_neighbors=cap): per target the first `cap` sources in source order with
    d^2 < r^2 in fp32, the self-loop counted inside the cap."""
    E, start = 0, 0
    r2 = torch.tensor(cutoff * cutoff, dtype=torch.float32)
    for n in sizes:
        p = pos[start:start + n]
        d = p[:, None, :] - p[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        E += int((d2 < r2).sum(1).clamp(max=cap).sum())
        start += n
    return E


# sizes, cap, pad_degree -> e_bound, n_pad  (worked by hand:
#  [21], 32: 21 * 21 = 441, ceil((441 - 21) / 32) = 14;
#  [3, 21, 1, 40], 8: 9 + 168 + 1 + 320 = 498, ceil((498 - 65) / 8) = 55;
#  [1], 32: 1, max(1, 0) = 1;
#  [21] with pad_degree 64: ceil(420 / 64) = 7)
LAYOUTS = [([21], 32, None, 441, 14), ([3, 21, 1, 40], 8, None, 498, 55), ([1], 32, None, 1, 1), ([21], 32, 64, 441, 7)]


@pytest.mark.parametrize("sizes,cap,pad_degree,e_bound,n_pad", LAYOUTS)
def test_padded_layout_numbers(sizes, cap, pad_degree, e_bound, n_pad):
    from gotennet_amd.graph import PaddedLayout
    batch, n_mol, N = _batch(sizes), len(sizes), sum(sizes)
    z = torch.arange(1, N + 1)
    lay = PaddedLayout(batch, n_mol, cap, pad_degree, z=z)
    assert (lay.N, lay.n_mol, lay.sizes) == (N, n_mol, sizes)
    assert lay.pad_degree == (pad_degree or cap)
    assert (lay.e_bound, lay.n_pad) == (e_bound, n_pad)
    assert lay.edge_capacity == e_bound + n_pad and lay.n_atoms == N + n_pad
    assert lay.batch.dtype == torch.int64 and lay.batch.shape == (N + n_pad,)
    assert torch.equal(lay.batch[:N], batch) and bool((lay.batch[N:] == n_mol).all())
    assert lay.z.dtype == torch.int32 and torch.equal(lay.z[:N], z.to(torch.int32)) and bool((lay.z[N:] == 0).all())
    assert torch.equal(lay.pad_z(z), lay.z)
    ptr = [0]
    for n in sizes:
        ptr.append(ptr[-1] + n)
    assert lay.mol_ptr.dtype == torch.int32 and lay.mol_ptr.tolist() == ptr + [N + n_pad]


@pytest.mark.parametrize("sizes,cap", [([21], 32), ([3, 21, 1, 40], 8), ([1], 32), ([40, 7], 32)])
def test_edge_bound_holds_for_random_positions(sizes, cap):
    from gotennet_amd.graph import PaddedLayout
    lay = PaddedLayout(_batch(sizes), len(sizes), cap)
    g = torch.Generator().manual_seed(1)
    for box in (2.0, 4.0, 8.0, 16.0, 64.0):
        pos = torch.rand((sum(sizes), 3), generator=g) * box
        E = _brute_force_edges(pos, sizes, 5.0, cap)
        assert lay.N <= E <= lay.e_bound, box
        deg = lay.tail_degrees(E)
        assert sum(deg) == lay.edge_capacity - E and min(deg) >= 1 and max(deg) <= lay.pad_degree + 1


def test_edge_bound_is_attained_when_all_atoms_are_within_the_cutoff():
    from gotennet_amd.graph import PaddedLayout
    sizes, cap = [3, 21, 1, 40], 8
    lay = PaddedLayout(_batch(sizes), len(sizes), cap)
    pos = torch.rand((65, 3), generator=torch.Generator().manual_seed(2)) * 4.0 / 3 ** 0.5    # diameter < 5
    assert _brute_force_edges(pos, sizes, 5.0, cap) == lay.e_bound == 498
    pos = torch.rand((65, 3), generator=torch.Generator().manual_seed(2)) * 4.0               # the 4 A cube
    assert _brute_force_edges(pos, sizes, 5.0, cap) == 498                                    # (this draw: every target still reaches its cap)


@pytest.mark.parametrize("sizes,cap,pad_degree", [([21], 32, None), ([3, 21, 1, 40], 8, None), ([1], 32, None),
                                                  ([21], 32, 64), ([21] * 5, 32, 7)])
def test_tail_partition_bounds_at_both_extremes(sizes, cap, pad_degree):
    """P = edge_capacity - E between n_pad (E = e_bound) and edge_capacity - N (self-loops only): every dummy atom gets at
    least one and at most pad_degree + 1 edges, contiguous blocks, the first P % n_pad one more."""
    from gotennet_amd.graph import PaddedLayout
    lay = PaddedLayout(_batch(sizes), len(sizes), cap, pad_degree)
    for E in sorted({lay.e_bound, lay.N, (lay.e_bound + lay.N) // 2}):
        deg = lay.tail_degrees(E)
        P = lay.edge_capacity - E
        assert len(deg) == lay.n_pad and sum(deg) == P
        assert min(deg) >= 1 and max(deg) <= lay.pad_degree + 1
        assert deg == sorted(deg, reverse=True) and deg[0] - deg[-1] <= 1
        assert deg.count(deg[-1] + 1) == (P % lay.n_pad if deg[0] != deg[-1] else 0)
    assert lay.tail_degrees(lay.e_bound) == [1] * lay.n_pad
    for bad in (lay.N - 1, lay.e_bound + 1):
        with pytest.raises(ValueError):
            lay.tail_degrees(bad)


def test_layout_refuses_bad_batches():
    from gotennet_amd.graph import PaddedLayout
    with pytest.raises(ValueError):
        PaddedLayout(torch.tensor([0, 1, 0]), 2)                 # molecules not contiguous
    with pytest.raises(ValueError):
        PaddedLayout(torch.tensor([0, 2]), 2)                    # index outside [0, n_mol)
    with pytest.raises(ValueError):
        PaddedLayout(torch.zeros(0, dtype=torch.int64), 1)
    with pytest.raises(ValueError):
        PaddedLayout(torch.zeros(3, dtype=torch.int64), 1).pad_z(torch.ones(4))
