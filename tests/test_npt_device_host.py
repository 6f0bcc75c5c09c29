"""CPU: constant-pressure MD on the device-rebuilt list -- what ``md.validate`` now accepts, what ``MDRun`` and
``RebuiltStep(cell_moves=True)`` still refuse before any launch, the entry point gn_cell_image_ranges in the header and the
ctypes table, and an fp64 emulation of its range rule against ``graph.image_ranges``."""
import inspect
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import npt_util as NU
from tests import pbc_multi_util as PM
from tests import pbc_util as U

BARO = dict(pressure=0.0, tau=10.0, compressibility=1.0, kT=0.0)
WIDE, NARROW = torch.eye(3) * 12.0, torch.tensor(PM.N1_CELL)


def _no_launch(fn, match):
    """``fn()`` raises a ``ValueError`` matching ``match`` before any entry point of the library is called."""
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


def _validate(**kw):
    from gotennet_amd import md
    a = _args()
    return md.validate(a["z"], a["pos"], 0.5, None, 1.0, None, kw.pop("cell"), 5.0, **kw)


@pytest.mark.parametrize("images", ["all", "auto"])
@pytest.mark.parametrize("cell", [WIDE, NARROW], ids=["wide", "narrow"])
def test_device_mode_accepts_a_barostat_with_image_ranges(images, cell):
    from gotennet_amd import graph, md
    table, ranges = _validate(cell=cell, images=images, rebuild="device", barostat=BARO)
    want = graph.resolve_images(cell, 5.0, images)
    assert (ranges is None) == (want is None) and (ranges is None or torch.equal(ranges, want))
    assert table.dtype == torch.float32
    md.check_rebuild("device", BARO, images)
    md.check_rebuild("device", None, "minimum")                # a fixed cell: every search
    md.check_rebuild("host", BARO, "minimum")


def test_minimum_image_with_a_barostat_is_refused_in_device_mode():
    from gotennet_amd import md
    for cell in (WIDE, NARROW):
        _no_launch(lambda: _validate(cell=cell, images="minimum", rebuild="device", barostat=BARO), "barostat")
    _no_launch(lambda: _validate(cell=WIDE, rebuild="device", barostat=BARO), "barostat")               # the default search
    _no_launch(lambda: md.MDRun(_ef(), **_args(dt=0.5, rebuild="device", cell=WIDE, barostat=BARO)), "barostat")
    _no_launch(lambda: md.MDRun(_ef(), **_args(dt=0.5, rebuild="device", cell=WIDE, images="minimum", barostat=BARO)), "barostat")
    with pytest.raises(ValueError) as err:
        md.check_rebuild("device", BARO, "minimum")
    msg = str(err.value)
    assert "2 * cutoff" in msg and "host" in msg and 'images="all"' in msg
    # the other refusals are what they were
    _no_launch(lambda: _validate(cell=WIDE, images="all", rebuild="gpu", barostat=BARO), "rebuild")
    _no_launch(lambda: _validate(cell=None, images="all", rebuild="device", barostat=BARO), "needs a cell")
    _no_launch(lambda: _validate(cell=torch.eye(3) * 1.0, images="all", rebuild="device", barostat=BARO), "cutoff / 3")
    _no_launch(lambda: _validate(cell=WIDE, images="some", rebuild="device", barostat=BARO), "images")
    assert md.REBUILD_MODES == ("host", "device")
    assert "rebuild" not in inspect.signature(md.MDRun.__init__).parameters
    assert list(inspect.signature(md.MDRun.__init__).parameters)[-1] == "barostat"


def test_moving_cell_step_refuses_before_any_launch():
    from gotennet_amd.pipeline import RebuiltStep
    a = _args()
    step_args = (a["z"], a["batch"], 1)
    _no_launch(lambda: RebuiltStep(_ef(), *step_args, cell_moves=True), "needs a cell")
    _no_launch(lambda: RebuiltStep(_ef(), *step_args, images="all", cell_moves=True), "needs a cell")
    for cell in (WIDE, NARROW):
        _no_launch(lambda: RebuiltStep(_ef(), *step_args, cell=cell, images="minimum", cell_moves=True), "minimum")
        _no_launch(lambda: RebuiltStep(_ef(), *step_args, cell=cell, cell_moves=True), "minimum")
    _no_launch(lambda: RebuiltStep(_ef(), *step_args, cell=torch.eye(3) * 1.0, images="auto", cell_moves=True), "cutoff / 3")
    blank = object.__new__(RebuiltStep)
    blank.cell_moves = True
    _no_launch(lambda: blank.set_cell((torch.eye(3) * 12.0).requires_grad_()), "requires grad")
    fixed = object.__new__(RebuiltStep)
    fixed.cell_moves = False
    _no_launch(lambda: fixed.set_cell(torch.eye(3) * 12.0), "cell_moves")
    _no_launch(lambda: blank(a["pos"], cell=torch.eye(3) * 12.0), "cell")       # a cell per call: refused as before
    # the new keywords stand behind the existing parameters, whose order and defaults are what they were
    p = inspect.signature(RebuiltStep.__init__).parameters
    names = list(p)
    assert names[1:5] == ["ef", "z", "batch", "n_mol"]
    assert names[5:11] == ["max_num_neighbors", "cell", "images", "warmup", "capture", "state"]
    assert names.index("cell_moves") > names.index("state") and p["cell_moves"].default is False
    assert (p["max_num_neighbors"].default, p["cell"].default, p["images"].default, p["warmup"].default) == (32, None, "minimum", 2)


def test_entry_point_in_header_and_ctypes_table(repo_root):
    from gotennet_amd import _lib, graph
    header = open(os.path.join(repo_root, "include", "gotennet_hip.h")).read()
    src = open(os.path.join(repo_root, "gotennet_amd", "csrc", "gn_md.hip")).read()
    name = "gn_cell_image_ranges"
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/gotennet_hip.h"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]) == 8
    assert re.search(r'extern "C" int ' + name + r"\(", src)
    C = _lib.C
    assert _lib.SIGNATURES[name] == [C.c_void_p, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 4
    # one statement of the widths: both kernels call it
    assert len(re.findall(r"npt_cell_widths\(cell \+ 9 \* \(size_t\)m, w\)", src)) == 2
    assert re.search(r"#define\s+GN_PBC_MAX_IMAGE_RANGE\s+3\b", header) and graph.MAX_IMAGE_RANGE == 3
    assert _lib.ABI_VERSION == 11 and "#define GN_ABI_VERSION 11" in header      # an additive entry: the ABI number stays


# ------------------------------------------------------------------------------------------- the range rule in fp64
def emulate_ranges(cells, cutoff, max_range=3, ranges=None, state=0):
    """What gn_cell_image_ranges does, in numpy fp64 from the fp32 cell -> (ranges int [n, 3], reason [n], state).  A launch
    that starts with the word set writes nothing; a refused box keeps its row."""
    c = np.asarray(cells, dtype=np.float32).reshape(-1, 3, 3)
    n = c.shape[0]
    out = np.full((n, 3), -1, dtype=np.int64) if ranges is None else np.array(ranges, dtype=np.int64).reshape(n, 3)
    reason = np.zeros(n, dtype=np.int64)
    if state:
        return out, reason, state
    with np.errstate(all="ignore"):
        w, vol = NU.widths(c)
    for m in range(n):
        ok = bool(np.isfinite(vol[m])) and vol[m] != 0.0
        r = []
        for k in range(3):
            ok = ok and bool(np.isfinite(w[m, k])) and w[m, k] > 0.0
            if ok:
                r.append(math.floor(cutoff / w[m, k] + 0.5 + 2.0 ** -6))
                ok = r[-1] <= max_range
        if ok:
            out[m] = r
        else:
            reason[m], state = 1, 1
    return out, reason, state


def test_emulated_range_rule_is_graph_image_ranges():
    """The cells of test_pbc_multi_host.test_image_ranges_values_and_refusals."""
    from gotennet_amd import graph
    cells = torch.tensor([U.CUBE, PM.N1_CELL, PM.N2_CELL, PM.R2_CELL, PM.N3_CELL])
    got, reason, state = emulate_ranges(cells.numpy(), 5.0)
    assert got.tolist() == graph.image_ranges(cells, 5.0).tolist() == [[0, 0, 0], [1, 1, 1], [1, 1, 1], [2, 2, 2], [2, 2, 2]]
    assert state == 0 and not reason.any()
    skewed = torch.tensor([[10.5, 0.0, 0.0], [10.5, 10.5, 0.0], [0.0, 0.0, 10.5]])
    for cell, cutoff, want in ((torch.eye(3) * 10.0, 5.0, [[1, 1, 1]]), (torch.eye(3) * 10.4, 5.0, [[0, 0, 0]]),
                               (torch.diag(torch.tensor([20.0, 5.0, 1.7])), 5.0, [[0, 1, 3]]), (torch.eye(3) * 2.0, 6.0, [[3, 3, 3]]),
                               (skewed, 5.0, [[1, 0, 0]])):
        got, reason, state = emulate_ranges(cell.numpy(), cutoff)
        assert got.tolist() == graph.image_ranges(cell, cutoff).tolist() == want and state == 0
    # refusals: no volume, not finite, or R > 3 (a width below cutoff / (3.5 - 2^-6): inside what the host refuses, which is
    # every width below cutoff / 3)
    for bad in (torch.diag(torch.tensor([12.0, 12.0, 1.0])), torch.zeros((3, 3)), torch.eye(3) * float("nan"),
                torch.eye(3) * float("inf"), torch.eye(3) * 1.2):
        keep = [[2, 1, 0]]
        got, reason, state = emulate_ranges(bad.numpy(), 5.0, ranges=keep)
        assert (got.tolist(), reason.tolist(), state) == (keep, [1], 1)
        with pytest.raises(ValueError, match="cutoff / 3"):
            graph.image_ranges(bad, 5.0)
    # one bad box of two: the good one is written; a launch that starts frozen writes nothing
    two = torch.stack([torch.eye(3) * 12.0, torch.eye(3) * 1.2]).numpy()
    got, reason, state = emulate_ranges(two, 5.0, ranges=[[7, 7, 7], [2, 1, 0]])
    assert (got.tolist(), reason.tolist(), state) == ([[0, 0, 0], [2, 1, 0]], [0, 1], 1)
    got, reason, state = emulate_ranges(two, 5.0, ranges=[[7, 7, 7], [2, 1, 0]], state=1)
    assert (got.tolist(), reason.tolist(), state) == ([[7, 7, 7], [2, 1, 0]], [0, 0], 1)
    # between cutoff / 3.484 and cutoff / 3 the rule still gives R = 3 where the host already refuses
    assert emulate_ranges((torch.eye(3) * 1.6).numpy(), 5.0)[0].tolist() == [[3, 3, 3]]
