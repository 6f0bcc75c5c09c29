"""CPU: the attention-dropout mask definition (Philox4x32-10 known answers, kept fraction) and the ABI surface of the
dropout entry points."""
import os
import re

import numpy as np
import pytest

from tests.dropout_util import mask_words, philox4x32_10

# Random123 known-answer vectors (kat_vectors: philox4x32 10)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(w) for w in philox4x32_10(ctr, key)) == out


@pytest.mark.parametrize("seed", [1234, 7])
@pytest.mark.parametrize("layer", [0, 1, 2])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_fraction(seed, layer, p):
    """A binomial of n draws at 1 - p: the kept fraction lies within 3 standard deviations of 1 - p."""
    n = 4096 * 8
    kept = float((mask_words(seed, layer, n) >= np.uint64(int(np.floor(p * 2.0 ** 32)))).mean())
    sd = (p * (1 - p) / n) ** 0.5
    print(f"seed {seed} layer {layer} p {p}: kept {kept:.5f}, {(kept - (1 - p)) / sd:+.2f} sd")
    assert abs(kept - (1 - p)) <= 3 * sd


def test_layers_and_seeds_give_different_masks():
    a, b, c = mask_words(1234, 0, 4096), mask_words(1234, 1, 4096), mask_words(1235, 0, 4096)
    assert (a != b).mean() > 0.99 and (a != c).mean() > 0.99


def test_abi_surface(repo_root):
    from gotennet_amd import _lib
    header = open(os.path.join(repo_root, "include", "gotennet_hip.h")).read()
    assert re.search(r"#define\s+GN_ABI_VERSION\s+11\b", header)
    assert _lib.ABI_VERSION == 11
    lib = _lib.load()
    for name in ("gn_attn_softmax_dropout", "gn_attn_dropout_mask", "gn_message_backward_dropout"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the existing entry points keep their signatures
    assert len(_lib.SIGNATURES["gn_attn_softmax_dropout"]) == len(_lib.SIGNATURES["gn_attn_softmax"]) + 4
    assert len(_lib.SIGNATURES["gn_message_backward_dropout"]) == len(_lib.SIGNATURES["gn_message_backward"]) + 1
    assert "Philox4x32-10" in header
