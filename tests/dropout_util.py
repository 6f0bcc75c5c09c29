"""numpy restatement of the attention-dropout mask function of include/gotennet_hip.h (Philox4x32-10, one evaluation per
element) and the oracle hook that applies a list of masks to the oracle's segment softmax."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints), key: two -> the four output words (uint64 arrays holding 32-bit values)."""
    c = [np.asarray(v, dtype=np.uint64) & _LO for v in ctr]
    k = [np.asarray(v, dtype=np.uint64) & _LO for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]        # 32 x 32 -> 64 bits: no overflow
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k[0]) & _LO, p1 & _LO, ((p0 >> np.uint64(32)) ^ c[3] ^ k[1]) & _LO, p0 & _LO]
        k = [(k[0] + np.uint64(W0)) & _LO, (k[1] + np.uint64(W1)) & _LO]
    return c


def mask_words(seed: int, layer: int, n: int):
    """Output word 0 for elements 0..n-1 of ``layer`` under the int64 ``seed`` (two's complement -> its two 32-bit halves)."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = np.arange(n, dtype=np.uint64)
    return philox4x32_10((idx & _LO, idx >> np.uint64(32), layer, 0), (s & 0xFFFFFFFF, s >> 32))[0]


def mask_reference(seed: int, layer: int, E: int, H: int, p: float):
    """The [E, H] fp32 multipliers: 0 or 1 / (1 - p) (rounded once to fp32); p >= 1 drops everything."""
    if p >= 1.0:
        return np.zeros((E, H), dtype=np.float32)
    keep = mask_words(seed, layer, E * H) >= np.uint64(int(np.floor(p * 2.0 ** 32)))
    return np.where(keep, np.float32(1.0 / (1.0 - p)), np.float32(0.0)).astype(np.float32).reshape(E, H)


def patch_oracle_softmax(monkeypatch, masks):
    """The oracle has no dropout: its k-th ``segment_softmax`` call (one per interaction) is multiplied by ``masks[k]``
    ([E, H]; the mask commutes with the scalar norm applied after it).  -> the call counter (a one-element list)."""
    import oracle.gotennet_oracle as orc
    real, count = orc.segment_softmax, [0]

    def wrapper(s, index, n):
        out = real(s, index, n)
        m = masks[count[0]]
        count[0] += 1
        return out * m.to(out.dtype)[:, :, None]

    monkeypatch.setattr(orc, "segment_softmax", wrapper)
    return count
