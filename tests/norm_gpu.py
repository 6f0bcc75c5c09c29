"""What the GPU tests of tests/norm_util.py share: the library handle, device copies with a poisoned element past the end,
output arrays between sentinel guard rows, and the launcher that runs every call twice."""
import math

import torch

GUARD = 8                                          # sentinel rows before and after every output array
SENTINEL = 12345.678


def lib():
    from gotennet_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32)


def dev(t):
    """On the device with one NaN / -1 element past the end: never a NULL pointer at size 0, and an over-read is seen."""
    fill = math.nan if t.is_floating_point() else -1
    return torch.cat([t.reshape(-1), torch.full((1,), fill, dtype=t.dtype)]).cuda()


class Out:
    """[GUARD + rows + GUARD, cols]: ``fill`` inside (NaN: a skipped element fails its bound), the sentinel around."""

    def __init__(self, rows, cols, fill=math.nan):
        self.rows = rows
        self.t = torch.full((rows + 2 * GUARD, max(cols, 1)), SENTINEL, device="cuda")
        self.t[GUARD:GUARD + rows] = fill

    def ptr(self):
        return self.t[GUARD:].data_ptr()

    def inner(self):
        return self.t[GUARD:GUARD + self.rows]

    def check(self, name):
        assert bool((self.t[:GUARD] == SENTINEL).all()), f"{name}: a row before the start was written"
        assert bool((self.t[GUARD + self.rows:] == SENTINEL).all()), f"{name}: a row past the end was written"


def launch(call, specs, runs=2):
    """Two launches into fresh arrays: rc 0, same bits, guards intact.  ``specs``: name -> (rows, cols).  -> name -> CPU tensor."""
    res = []
    for _ in range(runs):
        outs = {k: Out(r, c) for k, (r, c) in specs.items()}
        rc = call({k: o.ptr() for k, o in outs.items()})
        torch.cuda.synchronize()
        assert rc == 0, rc
        for k, o in outs.items():
            o.check(k)
        res.append({k: o.inner().cpu() for k, o in outs.items()})
    for k in res[0]:
        assert torch.equal(bits(res[0][k]), bits(res[-1][k])), f"{k}: two launches differ"
    return res[0]
