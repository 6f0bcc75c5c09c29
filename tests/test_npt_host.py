"""CPU: the barostat's refusals (raised before any library call), its public surface, the ctypes table of the gn_npt_* entry
points, the unit constants and the deterministic limit of the tests' own fp64 emulation."""
import inspect
import math
import re
import types

import numpy as np
import pytest
import torch

from tests import npt_util as NU

NPT = ("gn_npt_pressure", "gn_npt_barostat", "gn_npt_rescale", "gn_npt_cell_guard")
MD_AND_VERIFY = ("gn_radius_verify", "gn_radius_verify_pbc", "gn_radius_verify_pbc_images", "gn_md_kick", "gn_md_drift",
                 "gn_md_langevin", "gn_md_noise", "gn_md_kinetic", "gn_md_finish")
CELL = torch.eye(3) * 12.0
GOOD = dict(pressure=1e-3, tau=10.0, compressibility=2.0)
THERMOSTAT = dict(kT=0.02, gamma=0.5, key=(77, 5))


def _args(**kw):
    z = torch.tensor([8, 1, 1])
    base = dict(z=z, pos=torch.zeros((3, 3)), batch=torch.zeros(3, dtype=torch.int64), n_mol=1, dt=0.5, cell=CELL)
    base.update(kw)
    return base


def _refused(monkeypatch, match, **kw):
    """``MDRun`` raises ``ValueError`` without touching the library: ``call`` fails if it is reached."""
    from gotennet_amd import _lib, graph, md

    def no_call(name, *args):
        raise AssertionError(f"{name} was called before the refusal")

    for mod in (_lib, graph, md):
        monkeypatch.setattr(mod, "call", no_call)
    ef = types.SimpleNamespace(rep=types.SimpleNamespace(cutoff=5.0), head=None)
    with pytest.raises(ValueError, match=match):
        md.MDRun(ef, **_args(**kw))


def test_refusals_come_before_any_launch(monkeypatch):
    nan, inf = float("nan"), float("inf")
    _refused(monkeypatch, "needs a cell", cell=None, barostat=dict(GOOD, kT=0.0))
    for key in GOOD:
        _refused(monkeypatch, "missing", barostat={k: v for k, v in dict(GOOD, kT=0.0).items() if k != key})
    for name in ("tau", "compressibility", "max_step"):
        for bad in (0.0, -1.0, nan, inf):
            _refused(monkeypatch, name, barostat=dict(GOOD, kT=0.0, **{name: bad}))
    for bad in (nan, inf, -inf):
        _refused(monkeypatch, "pressure", barostat=dict(GOOD, kT=0.0, pressure=bad))
    _refused(monkeypatch, "kT", barostat=dict(GOOD, kT=-1.0, key=3))
    _refused(monkeypatch, "kT", barostat=dict(GOOD, kT=nan, key=3))
    _refused(monkeypatch, "kT is required", barostat=dict(GOOD))                          # no thermostat to take it from
    _refused(monkeypatch, "needs a key", barostat=dict(GOOD, kT=0.02))                    # kT > 0, no thermostat, no key
    _refused(monkeypatch, "unknown", barostat=dict(GOOD, kT=0.0, maxstep=0.1))
    # the cell is still distance_pbc's to refuse
    _refused(monkeypatch, "2 \\* cutoff", cell=torch.eye(3) * 9.0, barostat=dict(GOOD, kT=0.0))


def test_defaults_come_from_the_thermostat():
    from gotennet_amd import md
    b = md.barostat_parameters(dict(GOOD), THERMOSTAT, CELL)
    assert b["kT"] == 0.02 and b["key"] == (77, 5) and b["max_step"] == 0.05
    b = md.barostat_parameters(dict(GOOD, kT=0.0, key=9, max_step=0.01), THERMOSTAT, CELL)
    assert b["kT"] == 0.0 and b["key"] == 9 and b["max_step"] == 0.01
    assert md.barostat_parameters(dict(GOOD, kT=0.0), None, CELL)["key"] is None          # the deterministic limit needs no key


def test_validate_without_a_barostat_is_unchanged():
    from gotennet_amd import graph, md
    a = _args()
    narrow = torch.eye(3) * 4.0
    for cell, images in ((CELL, "minimum"), (CELL, "auto"), (narrow, "auto"), (None, "minimum")):
        old = md.validate(a["z"], a["pos"], 0.5, None, 1.0, None, cell, 5.0, images)
        new = md.validate(a["z"], a["pos"], 0.5, None, 1.0, None, cell, 5.0, images, barostat=None)
        assert torch.equal(old[0], new[0]) and torch.equal(old[0], md.default_masses())
        want = None if cell is None or cell is CELL else graph.image_ranges(narrow, 5.0)
        for got in (old[1], new[1]):
            assert got is None if want is None else torch.equal(got, want)
    with_b = md.validate(a["z"], a["pos"], 0.5, None, 1.0, None, CELL, 5.0, "minimum", barostat=dict(GOOD, kT=0.0))
    assert torch.equal(with_b[0], md.default_masses()) and with_b[1] is None
    p = inspect.signature(md.validate).parameters
    assert list(p)[-1] == "barostat" and p["barostat"].default is None


def test_public_surface():
    from gotennet_amd import md
    p = inspect.signature(md.MDRun.__init__).parameters
    names = list(p)
    assert names[-1] == "barostat" and p["barostat"].default is None
    assert names[:-1] == ["self", "ef", "z", "pos", "batch", "n_mol", "dt", "masses", "force_scale", "vel", "cell", "images",
                          "max_num_neighbors", "thermostat", "check_every", "log_len", "captured"]
    for name in ("cell", "volume", "pressure"):
        assert isinstance(getattr(md.MDRun, name), property) and getattr(md.MDRun, name).fset is None
    assert callable(md.MDRun.npt_log) and callable(md.MDRun.energy_log)


def test_entry_points_in_header_and_ctypes_table(repo_root):
    import os
    from gotennet_amd import _lib
    header = open(os.path.join(repo_root, "include", "gotennet_hip.h")).read()
    for name in NPT:
        assert name in _lib.SIGNATURES, name
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/gotennet_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    declared = set(re.findall(r"^(?:int|long) (gn_\w+)\(", header, flags=re.M))
    assert {n for n in declared if n.startswith("gn_npt_")} == set(NPT)
    assert {n for n in declared if n.startswith(("gn_md_", "gn_radius_verify"))} == set(MD_AND_VERIFY)
    assert _lib.ABI_VERSION == 11 and "#define GN_ABI_VERSION 11" in header


def test_unit_constants():
    from gotennet_amd import md
    assert md.BAR_EV_ANGSTROM3 == pytest.approx(1e5 * 6.241509074e18 * 1e-30, rel=1e-9)
    assert md.BAR_KCAL_MOL_ANGSTROM3 == pytest.approx(1e5 * 6.02214076e23 / 4184.0 * 1e-30, rel=1e-9)


def test_emulation_deterministic_limit():
    beta, tau, dt, p0 = 3.0, 7.0, 0.25, 0.125
    p = np.array([0.5, -0.25, p0, 1.0])
    vol = np.array([100.0, 1000.0, 10.0, 1.0])
    de = NU.delta_eps(p, vol, p0, beta, tau, dt, 0.0)
    assert np.array_equal(de, -(np.float64(beta) / np.float64(tau)) * (np.float64(p0) - p) * np.float64(dt))
    assert de[2] == 0.0 and NU.scale(de)[2] == 1.0
    # the noise term alone: P_int == P0
    xi = np.array([1.0, -2.0, 0.5, 0.0])
    dn = NU.delta_eps(np.full(4, p0), vol, p0, beta, tau, dt, 0.02, xi)
    assert np.allclose(dn, np.sqrt(2 * 0.02 * beta * dt / (vol * tau)) * xi, rtol=1e-15, atol=0.0)
    # signs: a target above the internal pressure shrinks the box
    assert de[1] < 0 < de[0] and math.isclose(float(NU.pressure([3.0], np.eye(3)[None] * -0.5, [4.0])[0]), 0.5 + 0.5)
    w, v = NU.widths(np.array([[10.5, 0, 0], [1.5, 11.0, 0], [-1.0, 2.0, 12.0]]))
    assert math.isclose(float(v[0]), 10.5 * 11.0 * 12.0) and bool((w[0] <= np.array([10.5, np.hypot(1.5, 11.0), np.sqrt(1 + 4 + 144.0)])).all())
