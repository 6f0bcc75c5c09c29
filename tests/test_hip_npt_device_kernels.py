"""GPU: gn_cell_image_ranges (csrc/gn_md.hip) called directly -- its values against ``graph.image_ranges``, its refusals, the
frozen launch, guard words around every buffer it writes, and its argument checks."""
import numpy as np
import pytest
import torch

from tests import npt_util as NU
from tests import pbc_multi_util as PM
from tests import pbc_util as U

pytestmark = pytest.mark.gpu

PAD, FILL = 4, -7                          # guard words on either side of every buffer the kernel writes
MAX_RANGE = 3
THRESHOLD_MARGIN = 1e-9                    # no width of a test cell this close (relative) to a width where the rule steps


def _padded(values, dtype=torch.int32):
    v = torch.as_tensor(np.asarray(values)).to(dtype).flatten()
    whole = torch.full((v.numel() + 2 * PAD,), FILL, dtype=dtype)
    whole[PAD:PAD + v.numel()] = v
    whole = whole.cuda()
    return whole, whole[PAD:PAD + v.numel()]


def _pads_intact(whole):
    w = whole.cpu()
    return bool((w[:PAD] == FILL).all()) and bool((w[-PAD:] == FILL).all())


def _launch(cells, cutoff, start=None, stale=0, step=5):
    """One launch on guarded buffers -> (ranges [n, 3], reason [n], state [2]) as lists.  ``start``: the rows before."""
    from gotennet_amd._lib import call
    c = torch.tensor(np.asarray(cells, dtype=np.float32)).reshape(-1, 3, 3).cuda()
    n = c.shape[0]
    r_w, r = _padded(np.full((n, 3), 9) if start is None else start)
    s_w, s = _padded([stale, step])
    q_w, q = _padded(np.zeros(n))
    call("gn_cell_image_ranges", c.data_ptr(), n, float(cutoff), MAX_RANGE, r.data_ptr(), s.data_ptr(), q.data_ptr(),
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _pads_intact(r_w) and _pads_intact(s_w) and _pads_intact(q_w)
    return r.cpu().reshape(n, 3).tolist(), q.cpu().tolist(), s.cpu().tolist()


def _clear_of_thresholds(cells, cutoff):
    """The rule floor(cutoff / w + 1/2 + 2^-6) steps at w = cutoff / (n - 1/2 - 2^-6): an input condition, asserted in fp64."""
    w, _ = NU.widths(np.asarray(cells, dtype=np.float32))
    steps = cutoff / (np.arange(1, 6, dtype=np.float64) - 0.5 - 2.0 ** -6)
    rel = np.abs(w.reshape(-1, 1) / steps.reshape(1, -1) - 1.0)
    assert float(rel.min()) > THRESHOLD_MARGIN, float(rel.min())


def test_values_are_graph_image_ranges():
    from gotennet_amd import graph
    skewed = [[10.5, 0.0, 0.0], [10.5, 10.5, 0.0], [0.0, 0.0, 10.5]]
    cells = [U.CUBE, U.TRICLINIC, PM.N1_CELL, PM.N2_CELL, PM.R2_CELL, PM.N3_CELL, np.diag([20.0, 5.0, 1.7]), np.diag([1.7, 20.0, 5.0]),
             skewed, U.LEFT_HANDED, np.eye(3) * 10.0, np.eye(3) * 10.4]
    _clear_of_thresholds(cells, 5.0)
    want = graph.image_ranges(torch.tensor(np.asarray(cells, dtype=np.float32)), 5.0).tolist()
    assert want[0] == [0, 0, 0] and want[4] == [2, 2, 2] and want[6] == [0, 1, 3] and want[7] == [3, 0, 1] and want[8] == [1, 0, 0]
    assert {r for row in want for r in row} == {0, 1, 2, 3}
    assert _launch(cells, 5.0) == (want, [0] * len(cells), [0, 5])
    # another cutoff: the narrowest cell the host accepts
    _clear_of_thresholds([np.eye(3) * 2.0], 6.0)
    assert graph.image_ranges(torch.eye(3) * 2.0, 6.0).tolist() == [[3, 3, 3]]
    assert _launch([np.eye(3) * 2.0], 6.0) == ([[3, 3, 3]], [0], [0, 5])


def test_more_boxes_than_threads():
    """1100 boxes: the workgroup's second trip; every box its own widths."""
    from gotennet_amd import graph
    n = 1100
    w = np.stack([np.linspace(1.7, 14.0, n), np.linspace(14.0, 1.7, n), np.linspace(3.0, 9.0, n)], axis=1).astype(np.float32)
    cells = np.zeros((n, 3, 3), dtype=np.float32)
    cells[:, 0, 0], cells[:, 1, 1], cells[:, 2, 2] = w[:, 0], w[:, 1], w[:, 2]
    cells[:, 1, 0] = 0.5                                            # a shear that leaves the widths near the diagonal
    _clear_of_thresholds(cells, 5.0)
    want = graph.image_ranges(torch.tensor(cells), 5.0)
    assert want[:, 0].unique().tolist() == [0, 1, 2, 3] and not torch.equal(want[-1], want[0])
    got, reason, state = _launch(cells, 5.0)
    assert got == want.tolist() and reason == [0] * n and state == [0, 5]


def test_refusals_keep_their_rows_and_freeze():
    from gotennet_amd import graph
    nan_entry = np.eye(3) * 12.0
    nan_entry[1, 2] = float("nan")
    flat = np.array([[4.0, 0, 0], [0, 4.0, 0], [4.0, 4.0, 0]])               # coplanar rows: no volume
    cells = [np.eye(3) * 12.0, np.eye(3) * 1.2, PM.N1_CELL, nan_entry, np.diag([12.0, 12.0, 1.0]), flat, np.diag([np.inf] * 3),
             PM.R2_CELL]
    assert 1.2 < 5.0 / 3.0 and 5.0 / 1.2 + 0.5 + 2.0 ** -6 >= MAX_RANGE + 1           # below cutoff / 3, and R would be 4
    start = np.arange(24).reshape(8, 3) + 10
    got, reason, state = _launch(cells, 5.0, start=start)
    assert reason == [0, 1, 0, 1, 1, 1, 1, 0] and state == [1, 5]
    for m, bad in enumerate(reason):
        if bad:
            assert got[m] == start[m].tolist()                               # untouched
            with pytest.raises(ValueError, match="cutoff / 3"):
                graph.image_ranges(torch.tensor(np.asarray(cells[m], dtype=np.float32)), 5.0)
        else:                                                                # the other boxes of the same launch are written
            assert got[m] == graph.image_ranges(torch.tensor(np.asarray(cells[m], dtype=np.float32)), 5.0).tolist()[0]
    # a launch that starts with the word set writes nothing: cells it would accept, and cells it would refuse
    for frozen in ([np.eye(3) * 12.0, PM.N1_CELL], cells):
        k = len(frozen)
        assert _launch(frozen, 5.0, start=start[:k], stale=1) == (start[:k].tolist(), [0] * k, [1, 5])
    # between cutoff / 3.484 and cutoff / 3 the rule still holds R = 3 (the host's bound is the round one)
    assert _launch([np.eye(3) * 1.6], 5.0) == ([[3, 3, 3]], [0], [0, 5])


def test_bad_arguments():
    from gotennet_amd import _lib
    fn, st = _lib.load().gn_cell_image_ranges, torch.cuda.current_stream().cuda_stream
    c = (torch.eye(3) * 12.0).reshape(1, 3, 3).cuda()
    r_w, r = _padded([9, 9, 9])
    s_w, s = _padded([0, 5])
    q_w, q = _padded([0])
    good = [c.data_ptr(), 1, 5.0, MAX_RANGE, r.data_ptr(), s.data_ptr(), q.data_ptr(), st]
    for k in (0, 4, 5, 6):                                                    # a null pointer with n_mol > 0
        args = list(good)
        args[k] = None
        assert fn(*args) == _lib.GN_ERR_BAD_ARG, k
    for k, v in ((1, -1), (2, 0.0), (2, float("nan")), (3, -1), (3, MAX_RANGE + 1)):
        args = list(good)
        args[k] = v
        assert fn(*args) == _lib.GN_ERR_BAD_ARG, (k, v)
    assert fn(None, 0, 5.0, MAX_RANGE, None, s.data_ptr(), None, st) == 0     # n_mol = 0: a no-op
    torch.cuda.synchronize()
    assert r.tolist() == [9, 9, 9] and s.tolist() == [0, 5] and q.tolist() == [0]
    assert fn(*good) == 0
    torch.cuda.synchronize()
    assert r.tolist() == [0, 0, 0] and s.tolist() == [0, 5] and q.tolist() == [0]
    assert _pads_intact(r_w) and _pads_intact(s_w) and _pads_intact(q_w)
