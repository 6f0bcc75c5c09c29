"""CPU: the device-rebuilt neighbour list -- the three entry points in the header and the ctypes table, the closed-form map
from a tail slot to its dummy atom against ``PaddedLayout.tail_degrees``, the edge bound of a multi-image list, and what
``RebuiltStep`` / ``MDRun`` / ``Relax`` refuse before any launch."""
import inspect
import os
import re
import types

import pytest
import torch

from tests import pbc_multi_util as PM
from tests import rebuild_util as RU
from tests.test_dynamic_step_host import LAYOUTS, _batch

NEW = {"gn_degree_scan": 5, "gn_padded_tail": 10, "gn_graph_refresh": 12}


def test_entry_points_in_header_and_ctypes_table(repo_root):
    from gotennet_amd import _lib
    header = open(os.path.join(repo_root, "include", "gotennet_hip.h")).read()
    src = open(os.path.join(repo_root, "gotennet_amd", "csrc", "gn_graph.hip")).read()
    for name, n_args in NEW.items():
        assert name in _lib.SIGNATURES, name
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/gotennet_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]) == n_args, name
        assert re.search(r'extern "C" int ' + name + r"\(", src), name
    # what the binding passes by value: N, and the int64 capacity; everything else is a pointer
    C = _lib.C
    assert _lib.SIGNATURES["gn_degree_scan"] == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert _lib.SIGNATURES["gn_padded_tail"][1:4] == [C.c_int, C.c_int, C.c_int64]
    assert _lib.SIGNATURES["gn_graph_refresh"][1:3] == [C.c_int, C.c_int]
    assert _lib.ABI_VERSION == 11 and "#define GN_ABI_VERSION 11" in header      # additive entries: the ABI number stays


@pytest.mark.parametrize("sizes,cap,pad_degree,e_bound,n_pad", LAYOUTS)
def test_closed_form_tail_map_is_the_layouts_partition(sizes, cap, pad_degree, e_bound, n_pad):
    from gotennet_amd.graph import PaddedLayout
    lay = PaddedLayout(_batch(sizes), len(sizes), cap, pad_degree)
    N, capacity = lay.N, lay.edge_capacity
    assert (lay.e_bound, lay.n_pad) == (e_bound, n_pad)
    for E in range(N, e_bound + 1):
        own = RU.tail_owner(N, n_pad, capacity, E)
        assert own.shape[0] == capacity - E
        assert bool((own[1:] >= own[:-1]).all()) and int(own[0]) == N and int(own[-1]) == N + n_pad - 1
        assert torch.bincount(own - N, minlength=n_pad).tolist() == lay.tail_degrees(E), E


def test_padded_list_restatement():
    ei = torch.tensor([[0, 1, 0, 1], [0, 0, 1, 1]])
    ev, ed = torch.arange(12.0).reshape(4, 3), torch.tensor([0.0, 1.0, 1.0, 0.0])
    sh = torch.ones((4, 3), dtype=torch.int32)
    pei, pev, ped, psh = RU.padded_list(2, 2, 9, ei, ev, ed, sh)
    assert pei.tolist() == [[0, 1, 0, 1, 2, 2, 2, 3, 3], [0, 0, 1, 1, 2, 2, 2, 3, 3]]           # P = 5: 3 + 2
    assert torch.equal(pev[:4], ev) and bool((pev[4:] == 0).all()) and bool((ped[4:] == 0).all())
    assert torch.equal(psh[:4], sh) and bool((psh[4:] == 0).all()) and psh.dtype == torch.int32
    assert RU.padded_list(2, 2, 9, ei, ev, ed)[3] is None


def test_multi_image_bound():
    from gotennet_amd.graph import PaddedLayout
    for sizes, cap in (([21], 32), ([3, 21, 1, 40], 8), ([1], 32)):
        lay = PaddedLayout(_batch(sizes), len(sizes), cap, periodic_images=True)
        assert lay.e_bound == sum(sizes) * cap and lay.periodic_images
        assert lay.n_pad == max(1, -(-(lay.e_bound - lay.N) // cap)) and lay.edge_capacity == lay.e_bound + lay.n_pad
        assert lay.tail_degrees(lay.e_bound) == [1] * lay.n_pad
        plain = PaddedLayout(_batch(sizes), len(sizes), cap)
        assert not plain.periodic_images and plain.e_bound == sum(n * min(n, cap) for n in sizes) <= lay.e_bound
    assert inspect.signature(PaddedLayout.__init__).parameters["periodic_images"].default is False


@pytest.mark.parametrize("name", ["n1", "n2", "n3"])
@pytest.mark.parametrize("cap", [4, 32])
def test_brute_force_multi_image_count_is_within_the_bound(name, cap):
    """One pair contributes several edges and an atom sees its own images: the open bound n * min(n, cap) does not hold
    (asserted for the uncapped systems), n * cap does."""
    from gotennet_amd.graph import PaddedLayout
    s = PM.system(name)
    bf = PM.brute_force(s["pos"], s["batch"], s["cell"], max_num_neighbors=cap)
    E, N = bf["edge_index"].shape[1], s["pos"].shape[0]
    lay = PaddedLayout(s["batch"], s["n_mol"], cap, periodic_images=True)
    assert N <= E <= lay.e_bound == N * cap
    per_target = torch.bincount(bf["edge_index"][1], minlength=N)
    assert int(per_target.max()) <= cap and int(per_target.min()) >= 1
    if cap == 32:
        assert E > PaddedLayout(s["batch"], s["n_mol"], cap).e_bound              # the one-edge-per-pair bound is exceeded


# ------------------------------------------------------------------------------------------------------ refusals
def _no_launch(fn, match):
    from gotennet_amd import _lib

    def no_call(name, args):
        raise AssertionError(f"{name} was called before the refusal")

    old = _lib.TIMER
    _lib.TIMER = types.SimpleNamespace(want=no_call, events=[])
    try:
        with pytest.raises(ValueError, match=match):
            fn()
    finally:
        _lib.TIMER = old


def _ef():
    return types.SimpleNamespace(rep=types.SimpleNamespace(cutoff=5.0), head=None)


def _args(**kw):
    base = dict(z=torch.tensor([8, 1, 1]), pos=torch.zeros((3, 3)), batch=torch.zeros(3, dtype=torch.int64), n_mol=1)
    base.update(kw)
    return base


def test_drivers_refuse_before_any_launch():
    from gotennet_amd import md, relax
    wide = torch.eye(3) * 12.0
    baro = dict(pressure=0.0, tau=10.0, compressibility=1.0, kT=0.0)
    _no_launch(lambda: md.MDRun(_ef(), **_args(dt=0.5, rebuild="gpu")), "rebuild")
    _no_launch(lambda: md.MDRun(_ef(), **_args(dt=0.5, rebuild=None)), "rebuild")
    _no_launch(lambda: md.MDRun(_ef(), **_args(dt=0.5, rebuild="device", cell=wide, barostat=baro)), "barostat")
    _no_launch(lambda: relax.Relax(_ef(), **_args(rebuild="gpu")), "rebuild")
    # a keyword of the constructor call (the drivers' metaclass); the pinned parameter lists of __init__ are what they were
    assert inspect.signature(md.MDRun).parameters["rebuild"].default == "host"
    assert inspect.signature(relax.Relax).parameters["rebuild"].default == "host"
    assert "rebuild" not in inspect.signature(md.MDRun.__init__).parameters
    assert "rebuild" not in inspect.signature(relax.Relax.__init__).parameters
    assert md.REBUILD_MODES == ("host", "device")


def test_rebuilt_step_refuses_before_any_launch():
    from gotennet_amd import graph
    from gotennet_amd.pipeline import RebuiltStep
    a = _args()
    step_args = (a["z"], a["batch"], 1)
    narrow, tiny = torch.eye(3) * 9.0, torch.eye(3) * 1.0              # widths 9 < 2 * cutoff and 1 < cutoff / 3
    for cell, images, match in ((narrow, "minimum", "2 \\* cutoff"), (tiny, "all", "cutoff / 3"), (tiny, "auto", "cutoff / 3"),
                                (torch.eye(3) * 12.0, "some", "images")):
        _no_launch(lambda: RebuiltStep(_ef(), *step_args, cell=cell, images=images), match)
        if images in graph.IMAGE_MODES:                               # ... and it is resolve_images' own refusal
            with pytest.raises(ValueError) as want:
                graph.resolve_images(cell, 5.0, images)
            with pytest.raises(ValueError) as got:
                RebuiltStep(_ef(), *step_args, cell=cell, images=images)
            assert str(got.value) == str(want.value)
    _no_launch(lambda: RebuiltStep(_ef(), *step_args, cell=(torch.eye(3) * 12.0).requires_grad_()), "requires grad")
    # a cell per call: refused whatever the step holds (no step can be built without a device)
    blank = object.__new__(RebuiltStep)
    _no_launch(lambda: blank(a["pos"], cell=torch.eye(3) * 12.0), "cell")
    p = inspect.signature(RebuiltStep.__init__).parameters
    assert [k for k in p][1:5] == ["ef", "z", "batch", "n_mol"]
    assert (p["max_num_neighbors"].default, p["cell"].default, p["images"].default, p["warmup"].default) == (32, None, "minimum", 2)
