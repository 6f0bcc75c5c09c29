"""GPU: gn_embedding_grad and gn_embedding_grad_images (csrc/gn_wgrad.hip: emb_source_kernel, then emb_species_kernel twice)
called directly on graphs built on the host -- a hub source, sources without out-edges, self-loops, self-pairs at a distance,
absent species, N = 0 -- against the fp64 restatement and the a-priori bounds of tests/readout_util.py (proved on the CPU by
tests/test_readout_host.py).  Outputs between sentinel guard rows, every launch twice (same bits), worst error / bound printed
per output; the last test prints the worst per entry point."""
import math

import pytest
import torch

from tests import readout_util as U
from tests.norm_gpu import bits as _bits, dev as _dev, launch as _launch, lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu

WORST = {}
EMB_IDS = [U.emb_id(n) for n in range(len(U.EMB_CASES))]
KEYS = ("g_ctx", "feat", "cut", "dst", "colptr", "perm", "order", "sp_ptr", "edge_diff")


def _emb_run(c, over=None, images=None):
    lib, st = _lib(), _stream()
    src = dict(c, **(over or {}))
    d = {k: _dev(src[k]) for k in KEYS}
    p = {k: t.data_ptr() for k, t in d.items()}
    N, F, nsp = c["N"], c["F"], c["n_species"]
    head = (p["g_ctx"], p["feat"], c["ldf"], p["cut"], p["dst"], p["colptr"], p["perm"], p["order"], p["sp_ptr"], nsp, N, F)
    images = c["images"] if images is None else images

    def call(o):
        if images == "null":                       # the _images entry point without edge_diff: the plain self-loop rule
            return lib.gn_embedding_grad_images(*head, None, o["work"], o["dA_na"], o["dA_nbr"], st)
        if images:
            return lib.gn_embedding_grad_images(*head, p["edge_diff"], o["work"], o["dA_na"], o["dA_nbr"], st)
        return lib.gn_embedding_grad(*head, o["work"], o["dA_na"], o["dA_nbr"], st)

    return _launch(call, dict(work=(N, F), dA_na=(nsp, F), dA_nbr=(nsp, F)))


@pytest.mark.parametrize("n", range(len(U.EMB_CASES)), ids=EMB_IDS)
def test_embedding_grad_within_bound(n):
    c, ex = U.emb_case(n), U.emb_expected(n)
    out = _emb_run(c)
    entry = "gn_embedding_grad_images" if c["images"] else "gn_embedding_grad"
    rs = {k: U.worst(out[k], *ex[k]) for k in ex}
    print(f"{c['id']}: " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))
    for k, v in rs.items():
        WORST[f"{entry}.{k}"] = max(WORST.get(f"{entry}.{k}", 0.0), v)
    assert all(v <= 1.0 for v in rs.values()), (c["id"], rs)
    assert float(out["dA_na"][0].abs().max()) == 0.0                         # the padding row, whatever species 0 holds
    if c["N"] == 0:                                                          # plain stores: zeros, not whatever was there
        assert float(out["dA_na"].abs().max()) == 0.0 and float(out["dA_nbr"].abs().max()) == 0.0
    if not c["images"]:                                                      # edge_diff = NULL is the same entry point
        same = _emb_run(c, images="null")
        for k in out:
            assert torch.equal(_bits(same[k]), _bits(out[k])), k


def test_self_pairs_at_a_distance_are_kept_only_with_edge_diff():
    """The same graph through both entry points: they differ exactly in the rows whose sources own a self-pair."""
    c = U.emb_case(EMB_IDS.index("hub-F65-ldf133-sp100-images"))
    with_diff, without = _emb_run(c, images=True), _emb_run(c, images=False)
    pair = (c["src"] == c["dst"].long()) & (c["edge_diff"] > 0)
    owners = torch.zeros(c["N"], dtype=torch.bool)
    owners[c["src"][pair]] = True
    assert bool(owners.any()) and torch.equal(_bits(with_diff["work"][~owners]), _bits(without["work"][~owners]))
    assert bool((with_diff["work"][owners] != without["work"][owners]).any(dim=1).all())
    assert torch.equal(_bits(with_diff["dA_na"]), _bits(without["dA_na"]))


def test_nan_in_one_edge_stays_in_its_source_species():
    c = U.emb_case(EMB_IDS.index("hub-F48-ldf96-sp5"))
    clean = _emb_run(c)
    keep = torch.nonzero(~U.emb_loop(c))[:, 0]
    e = int(keep[keep.numel() // 2])
    j = int(c["src"][e])
    feat = c["feat"].clone()
    feat[e, 7] = math.nan
    dirty = _emb_run(c, dict(feat=feat))
    rows, sp = torch.arange(c["N"]) != j, torch.arange(c["n_species"]) != int(c["z"][j])
    assert torch.equal(_bits(dirty["work"][rows]), _bits(clean["work"][rows])) and bool(torch.isnan(dirty["work"][j, 7]))
    assert torch.equal(_bits(dirty["dA_nbr"][sp]), _bits(clean["dA_nbr"][sp])) and bool(torch.isnan(dirty["dA_nbr"][~sp][0, 7]))
    cols = torch.arange(c["F"]) != 7
    assert torch.equal(_bits(dirty["dA_nbr"][:, cols]), _bits(clean["dA_nbr"][:, cols]))
    assert torch.equal(_bits(dirty["dA_na"]), _bits(clean["dA_na"]))


def test_entry_points_refuse_bad_arguments():
    """One call per clause.  Every pointer lies in the middle of a live zero-filled buffer (colptr = sp_ptr = 0: no edges, no
    atoms of any species), so a call that is wrongly accepted stays inside allocated memory."""
    from gotennet_amd import _lib as L
    lib, st = _lib(), _stream()
    fbuf, ibuf = torch.zeros(1 << 16, device="cuda"), torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    P, I = fbuf[1 << 15:].data_ptr(), ibuf[1 << 15:].data_ptr()
    # (g_ctx, feat, ldf, cut, dst, colptr, perm, order, sp_ptr, n_species, N, F, [edge_diff,] work, dA_na, dA_nbr)
    head = [P, P, 8, P, I, I, I, I, I, 2, 3, 4]
    plain, images = head + [P, P, P, st], head + [P, P, P, P, st]
    clauses = [(10, -1), (11, 0), (9, 0), (2, 7), (0, None), (1, None), (3, None), (4, None), (5, None), (6, None), (7, None), (8, None)]
    for fn, base, tail in ((lib.gn_embedding_grad, plain, 12), (lib.gn_embedding_grad_images, images, 13)):
        assert fn(*base) == 0
        for pos, bad in clauses + [(tail, None), (tail + 1, None), (tail + 2, None)]:
            args = list(base)
            args[pos] = bad
            assert fn(*args) == L.GN_ERR_BAD_ARG, (fn.__name__, pos, bad)
    no_diff = list(images)
    no_diff[12] = None                                                       # edge_diff stays optional
    assert lib.gn_embedding_grad_images(*no_diff) == 0
    for pos in (8, 14, 15):                                           # N = 0 still reads sp_ptr and writes both outputs
        args = list(images)
        args[10], args[pos] = 0, None
        assert lib.gn_embedding_grad_images(*args) == L.GN_ERR_BAD_ARG, pos
    torch.cuda.synchronize()
    assert float(fbuf.abs().max()) == 0.0


def test_worst_ratios_per_entry_point():
    print("worst error / bound: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())))
    assert WORST and all(v <= 1.0 for v in WORST.values())
