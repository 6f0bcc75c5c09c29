"""CPU: the MD driver's refusals (raised before any library call), the thermostat coefficients, the ctypes table of the new
entry points and the inputs of the stale-list tests."""
import inspect
import math
import re
import types

import numpy as np
import pytest
import torch

from tests import md_util as MU


def _args(**kw):
    z = torch.tensor([8, 1, 1])
    base = dict(z=z, pos=torch.zeros((3, 3)), batch=torch.zeros(3, dtype=torch.int64), n_mol=1, dt=0.5)
    base.update(kw)
    return base


def _refused(match, **kw):
    """``MDRun`` raises ``ValueError`` without touching the library: every entry point is replaced by one that fails."""
    from gotennet_amd import _lib, md
    ef = types.SimpleNamespace(rep=types.SimpleNamespace(cutoff=5.0), head=None)
    def no_call(name, args):
        raise AssertionError(f"{name} was called before the refusal")

    old = _lib.TIMER
    _lib.TIMER = types.SimpleNamespace(want=no_call, events=[])
    try:
        with pytest.raises(ValueError, match=match):
            md.MDRun(ef, **_args(**kw))
    finally:
        _lib.TIMER = old


def test_refusals_come_before_any_launch():
    narrow = torch.eye(3) * 9.0                      # width 9 < 2 * cutoff
    tiny = torch.eye(3) * 1.0                        # width 1 < cutoff / 3
    _refused("dt", dt=0.0)
    _refused("dt", dt=-1.0)
    _refused("dt", dt=float("nan"))
    _refused("masses", masses=torch.tensor([1.0, -1.0, 2.0]))
    _refused("masses", masses=torch.tensor([1.0, float("nan")]))
    _refused("no positive mass", masses=torch.tensor([1.0, 0.0] + [1.0] * 7))         # Z = 1 has no mass
    _refused("no positive mass", masses=torch.tensor([1.0, 1.0]))                     # Z = 8 is outside the table
    _refused("no positive mass", z=torch.tensor([8, 1, 40]))                          # the built-in table stops at Kr
    _refused("kT", thermostat=dict(kT=-1.0, gamma=0.1, key=1))
    _refused("gamma", thermostat=dict(kT=1.0, gamma=-0.1, key=1))
    _refused("missing", thermostat=dict(kT=1.0, gamma=0.1))
    _refused("2 \\* cutoff", cell=narrow)
    _refused("cutoff / 3", cell=tiny, images="all")
    _refused("images", cell=torch.eye(3) * 12.0, images="some")
    _refused("cell requires grad", cell=(torch.eye(3) * 12.0).requires_grad_())
    _refused("pos requires grad", pos=torch.zeros((3, 3), requires_grad=True))
    _refused("force_scale", force_scale=0.0)
    _refused("check_every", check_every=0)


def test_the_cell_check_is_distance_pbc_s():
    """``validate`` hands back what ``graph.resolve_images`` returns: None for a wide cell, the image ranges for a narrow one."""
    from gotennet_amd import graph, md
    a = _args()
    wide, narrow = torch.eye(3) * 12.0, torch.eye(3) * 4.0
    assert md.validate(a["z"], a["pos"], 0.5, None, 1.0, None, wide, 5.0, "minimum")[1] is None
    assert md.validate(a["z"], a["pos"], 0.5, None, 1.0, None, wide, 5.0, "auto")[1] is None
    assert torch.equal(md.validate(a["z"], a["pos"], 0.5, None, 1.0, None, narrow, 5.0, "auto")[1], graph.image_ranges(narrow, 5.0))
    table = md.validate(a["z"], a["pos"], 0.5, None, 1.0, None, None, 5.0)[0]
    assert table.dtype == torch.float32 and abs(float(table[8]) - 15.999) < 1e-6 and float(table[1]) == pytest.approx(1.008)


def test_langevin_coefficients():
    from gotennet_amd import md
    for kT, gamma, h, fs in ((0.0259, 0.01, 0.25, md.EV_ANGSTROM_AMU_FS), (0.6, 2.0, 0.5, md.KCAL_MOL_ANGSTROM_AMU_FS),
                             (1.0, 0.0, 1.0, 1.0), (0.0, 0.3, 1.0, 1.0)):
        c1, c2 = md.langevin_coefficients(kT, gamma, h, fs)
        r1 = np.exp(np.float64(-gamma) * np.float64(h))
        x = -np.expm1(np.float64(-2.0 * gamma * h))                     # 1 - c1^2 without the cancellation
        r2 = np.sqrt(np.float64(kT) * np.float64(fs) * x)
        assert abs(c1 - r1) <= 4e-16 * r1
        # 1 - c1 * c1 in fp64 is off by at most 4 roundings of a number near 1 (c1, its square, the difference): 4.4e-16
        # absolute; through the square root that is 2.2e-16 sqrt(kT fs) / sqrt(x), plus the roundings of the products and the root
        assert abs(c2 - r2) <= (2.5e-16 * math.sqrt(kT * fs) / math.sqrt(x) if x > 0 else 0.0) + 4e-16 * r2
    assert md.langevin_coefficients(1.0, 0.0, 1.0) == (1.0, 0.0)
    # the documented unit factors: e / (amu * 1e-20 m^2) in fs^-2 and 4184 J / mol over 1e-3 kg / mol in Angstrom^2 / fs^2
    assert md.EV_ANGSTROM_AMU_FS == pytest.approx(1.602176634e-19 / 1.66053906660e-27 * 1e-10, rel=1e-9)
    assert md.KCAL_MOL_ANGSTROM_AMU_FS == pytest.approx(4184.0 / 1e-3 * 1e-10, rel=1e-12)


NEW = ("gn_radius_verify", "gn_radius_verify_pbc", "gn_radius_verify_pbc_images", "gn_md_kick", "gn_md_drift",
       "gn_md_langevin", "gn_md_noise", "gn_md_kinetic", "gn_md_finish")


def test_new_entry_points_in_header_and_ctypes_table(repo_root):
    import os
    from gotennet_amd import _lib
    header = open(os.path.join(repo_root, "include", "gotennet_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/gotennet_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    declared = set(re.findall(r"^(?:int|long) (gn_\w+)\(", header, flags=re.M))
    assert {n for n in declared if n.startswith(("gn_md_", "gn_radius_verify"))} == set(NEW)
    assert _lib.ABI_VERSION == 11 and "#define GN_ABI_VERSION 11" in header      # additive entries: the ABI number stays


def test_public_surface():
    import gotennet_amd
    from gotennet_amd import graph, md
    assert gotennet_amd.MDRun is md.MDRun
    p = inspect.signature(md.MDRun.__init__).parameters
    assert [k for k in p][1:7] == ["ef", "z", "pos", "batch", "n_mol", "dt"]
    assert p["captured"].default is True and p["check_every"].default == 1 and p["images"].default == "minimum"
    assert p["max_num_neighbors"].default == 32 and p["thermostat"].default is None and p["masses"].default is None
    q = inspect.signature(graph.list_is_current).parameters
    assert [k for k in q][:8] == ["pos", "batch", "edge_index", "cutoff", "max_num_neighbors", "cell", "edge_shift", "images"]


def test_stale_list_inputs():
    """The threshold inputs are what they claim in fp32, and every case names both outcomes or none."""
    xb = np.float32(MU.below_threshold(MU.CUTOFF))
    r2 = np.float32(MU.CUTOFF) * np.float32(MU.CUTOFF)
    assert r2 == np.float32(2.25) and xb * xb == np.nextafter(r2, np.float32(0)) and np.float32(4.5) - np.float32(3.0) == np.float32(1.5)
    for table in (MU.cases(), MU.image_cases()):
        assert {"unchanged", "leaves", "enters", "swap", "beyond_cap", "inside_cap", "threshold", "middle_only"} <= set(table)
        for name, c in table.items():
            stale = c[-1]
            assert name.startswith("unchanged") and stale == () or 0 < len(stale) < 3, name
        assert table["middle_only"][-1] == (1,)
    assert tuple(int(n) for n in torch.bincount(MU.batch_vector())) == (2, 5, 9)
