"""Host: what the six projection entries refuse (gn_gemm_ex, gn_gemm_split, gn_gemm_f16x2 and their three group forms),
one case per clause of the argument checks, and what they accept without a launch (M == 0, an empty group).  No call here
reaches a launch: a refused call returns before it, and so does a problem with no rows."""
import ctypes as C

import pytest

FIELDS = dict(lda=64, ldc=64, M=8, N=64, K=64, act_lo=0, act_hi=0, row_cnt=1, row_gstride=1, row_goff=0,
              res=None, gate=None, gate_mode=0, pre_out=None, pro_mode=0, pro_lo=0, pro_hi=0, a_pre=None, ldp=0,
              a_gate=None, ldg=0, A2=None, A3=None, a_seg=0, act_kind=0, lda2=0, bias=None)
_buf = (C.c_float * 16)()
PTR = C.addressof(_buf)          # a non-null pointer: the cases below are refused (or have no rows) before anything reads it

# every clause of the checks shared by the single-problem and the group entries
REFUSED = {
    "K % 4": dict(K=66), "lda % 4": dict(lda=66), "N % 4": dict(N=66), "ldc % 4": dict(ldc=66),
    "act_lo % 4": dict(act_lo=2), "act_hi % 4": dict(act_hi=6),
    "row_cnt <= 0": dict(row_cnt=0), "row_cnt < 0": dict(row_cnt=-1), "N <= 0": dict(N=0), "K <= 0": dict(K=0), "M < 0": dict(M=-4),
    "gate without res at gate_mode 0": dict(gate=PTR),
    "pro_mode > 2": dict(pro_mode=3), "pro_mode < 0": dict(pro_mode=-1),
    "pro_mode 2 without a_pre": dict(pro_mode=2),
    "ldp % 4": dict(pro_mode=2, a_pre=PTR, ldp=66), "ldg % 4": dict(a_gate=PTR, ldg=66),
    "pro_lo % 4": dict(pro_mode=1, pro_lo=2, pro_hi=8), "pro_hi % 4": dict(pro_mode=1, pro_lo=0, pro_hi=6),
    "act_kind < 0": dict(act_kind=-1), "act_kind >= GN_ACT_COUNT": dict(act_kind=12),
}
# ... and the K-segment clauses, which only a descriptor can state
REFUSED_GROUP = {
    "a_seg % 32": dict(a_seg=48, A2=PTR), "a_seg < 0": dict(a_seg=-32, A2=PTR),
    "a_seg with pro_mode": dict(a_seg=32, A2=PTR, pro_mode=1), "a_seg with a_gate": dict(a_seg=32, A2=PTR, a_gate=PTR),
    "a_seg without A2": dict(a_seg=32),
    "K > 3 a_seg": dict(K=128, a_seg=32, A2=PTR, A3=PTR), "K > 2 a_seg without A3": dict(K=96, a_seg=32, A2=PTR),
    "lda2 % 4": dict(a_seg=32, A2=PTR, lda2=66), "lda2 < 0": dict(a_seg=32, A2=PTR, lda2=-4),
}
SINGLE = ("gn_gemm_ex", "gn_gemm_split", "gn_gemm_f16x2")
GROUP = ("gn_gemm_group", "gn_gemm_group_split", "gn_gemm_group_f16x2")


def _single(lib, name, **over):
    f = dict(FIELDS, **over)
    return getattr(lib, name)(PTR, f["lda"], PTR, f["bias"], PTR, f["ldc"], f["M"], f["N"], f["K"], f["act_lo"], f["act_hi"],
                              f["row_cnt"], f["row_gstride"], f["row_goff"], f["res"], f["gate"], f["gate_mode"], f["pre_out"],
                              f["pro_mode"], f["pro_lo"], f["pro_hi"], f["a_pre"], f["ldp"], f["a_gate"], f["ldg"],
                              f["act_kind"], None)


def _group(lib, name, overs, n=None):
    from gotennet_amd import _lib
    arr = (_lib.GemmDesc * max(len(overs), 1))()
    for d, over in zip(arr, overs):
        d.A, d.W, d.C = PTR, PTR, PTR
        for k, v in dict(FIELDS, **over).items():
            setattr(d, k, v)
    return getattr(lib, name)(arr, len(overs) if n is None else n, None)


@pytest.mark.parametrize("name", SINGLE)
def test_single_entries_refuse(name):
    from gotennet_amd import _lib
    lib = _lib.load()
    for what, over in REFUSED.items():
        assert _single(lib, name, **over) == _lib.GN_ERR_BAD_ARG, what
        assert _single(lib, name, **dict(over, M=over.get("M", 0))) == _lib.GN_ERR_BAD_ARG, what + " (no rows)"
    assert _single(lib, name, M=0) == 0
    assert _single(lib, name, M=0, gate=PTR, res=PTR, pro_mode=2, a_pre=PTR, ldp=64, a_gate=PTR, ldg=64, pro_hi=64) == 0
    assert _single(lib, name, M=0, gate=PTR, gate_mode=1, act_kind=11) == 0


def test_plain_entry_refuses():
    from gotennet_amd import _lib
    lib = _lib.load()
    call = lambda **o: (lambda f: lib.gn_gemm(PTR, f["lda"], PTR, None, PTR, f["ldc"], f["M"], f["N"], f["K"], f["act_lo"],
                                              f["act_hi"], f["row_cnt"], 1, 0, f["res"], f["gate"], None))(dict(FIELDS, **o))
    for what in ("K % 4", "lda % 4", "N % 4", "ldc % 4", "act_lo % 4", "act_hi % 4", "row_cnt <= 0", "N <= 0", "K <= 0",
                 "M < 0", "gate without res at gate_mode 0"):
        assert call(**REFUSED[what]) == _lib.GN_ERR_BAD_ARG, what
    assert call(M=0) == 0 and call(M=0, gate=PTR, res=PTR) == 0


@pytest.mark.parametrize("name", GROUP)
def test_group_entries_refuse(name):
    from gotennet_amd import _lib
    lib = _lib.load()
    for what, over in {**REFUSED, **REFUSED_GROUP}.items():
        assert _group(lib, name, [over]) == _lib.GN_ERR_BAD_ARG, what
        assert _group(lib, name, [dict(M=0), over]) == _lib.GN_ERR_BAD_ARG, what + " (second problem)"
    assert _group(lib, name, [dict(M=0)] * 5) == _lib.GN_ERR_BAD_ARG            # n > 4
    assert _group(lib, name, [], n=-1) == _lib.GN_ERR_BAD_ARG
    assert getattr(lib, name)(None, 1, None) == _lib.GN_ERR_BAD_ARG             # problems without descriptors
    assert getattr(lib, name)(None, 0, None) == 0                               # an empty group
    assert _group(lib, name, [dict(M=0)]) == 0 and _group(lib, name, [dict(M=0)] * 4) == 0
    assert _group(lib, name, [dict(M=0, K=96, a_seg=32, A2=PTR, A3=PTR, lda2=128, res=PTR)]) == 0
    assert _group(lib, name, [dict(M=0, K=64, a_seg=32, A2=PTR)]) == 0         # two segments need no A3
