"""CPU: the yardstick of the QM9 vector read-outs' training path.  The fp64 oracle's autograd through ``orc.dipole`` and
``orc.electronic_spatial_extent`` against the reference autograd's gradients stored in ``kat_qm9_head_grads.npz``
(tools/make_golden.py qm9_head_grads_kat), and the four backward entry points in the header and the binding."""
import os
import re

import numpy as np
import pytest
import torch

from tests.golden_util import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: max-norm relative per tensor: the class of the project's 1e-12 fp64 forward check with room for the order of the
#: per-molecule and per-weight reductions (sums of up to 72 fp64 products, a few 1e-16 each)
TOL64 = 1e-10

HEADS = ("dip_task", "dip_vec", "ese")
#: outputs of each head that carry a cotangent in the fixture
OUTPUTS = {"dip_task": ("property",), "dip_vec": ("dipole", "dipole_vector"), "ese": ("property",)}
NEW_ENTRY_POINTS = ("gn_geb_gate_backward", "gn_geb_context_backward", "gn_dipole_reduce_backward",
                    "gn_ese_reduce_backward")


def qm9_grad_kat():
    """-> (inputs, {head: state_dict}, {head: {output: cotangent}}, {head: {"h" | "X" | parameter: reference gradient}})."""
    k = np.load(os.path.join(GOLDEN_DIR, "kat_qm9_heads.npz"))
    t = {n: torch.from_numpy(k[n]) for n in k.files if "/" not in n}
    sd = {tag: {n[len(tag) + 1:]: torch.from_numpy(k[n]) for n in k.files if n.startswith(tag + "/")} for tag in HEADS}
    g = np.load(os.path.join(GOLDEN_DIR, "kat_qm9_head_grads.npz"))
    cot = {tag: {o: torch.from_numpy(g[f"{tag}/c_{o}"]) for o in OUTPUTS[tag]} for tag in HEADS}
    ref = {tag: {n[len(tag) + 6:]: torch.from_numpy(g[n]) for n in g.files if n.startswith(tag + "/grad/")} for tag in HEADS}
    return t, sd, cot, ref


def is_param(name):
    """state_dict keys that are parameters (``standardize.*`` and ``atomic_mass`` are buffers)."""
    return name.startswith(("equivariant_layers.", "out_net."))


def oracle_outputs(tag, sd64, h, X, pos, z, batch, n_mol, mean=0.3):
    """The oracle's outputs of head ``tag`` by the names of ``OUTPUTS`` (``mean``: of the standardised ``dip_task``)."""
    from oracle import gotennet_oracle as orc
    if tag == "dip_task":
        y, _ = orc.dipole(sd64, h, X, pos, batch, n_mol, "silu", mean=torch.tensor(mean), stddev=torch.tensor(1.7),
                          predict_magnitude=True)
        return {"property": y}
    if tag == "dip_vec":
        y, yv = orc.dipole(sd64, h, X, pos, batch, n_mol, "silu")
        return {"dipole": y, "dipole_vector": yv}
    y, _ = orc.electronic_spatial_extent(sd64, h, pos, z, batch, n_mol, "softplus")
    return {"property": y}


def oracle_grads(tag, t, sd, cot, h=None, X=None, pos=None, mean=0.3):
    """fp64 autograd of sum_outputs (cotangent * output) w.r.t. h, X and every parameter (zeros where unused)."""
    sd64 = {n: (v.double().requires_grad_(is_param(n)) if v.is_floating_point() else v) for n, v in sd.items()}
    h = (t["h"] if h is None else h).double().requires_grad_(True)
    X = (t["X"] if X is None else X).double().requires_grad_(True)
    pos = (t["pos"] if pos is None else pos).double()
    out = oracle_outputs(tag, sd64, h, X, pos, t["z"], t["batch"], int(t["n_mol"]), mean=mean)
    loss = sum((c.double() * out[o]).sum() for o, c in cot.items())
    names = [n for n in sd64 if is_param(n)]
    leaves = [h, X] + [sd64[n] for n in names]
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return {n: (torch.zeros_like(p) if g is None else g) for n, g, p in zip(["h", "X"] + names, grads, leaves)}


def _err(a, b):
    m = float(b.abs().max())
    return float((a - b).abs().max()) / m if m > 0 else float(a.abs().max())


@pytest.mark.parametrize("tag", HEADS)
def test_oracle_autograd_matches_reference_gradients(tag):
    t, sd, cot, ref = qm9_grad_kat()
    got = oracle_grads(tag, t, sd[tag], cot[tag])
    params = [n for n in sd[tag] if is_param(n)]
    assert sorted(ref[tag]) == sorted(["h", "X"] + params)           # every parameter has a reference gradient
    for n, r in ref[tag].items():
        assert got[n].shape == r.shape, n
        e = _err(got[n], r)
        print(tag, n, e)
        assert e <= TOL64, (tag, n, e)
    assert torch.equal(ref[tag]["X"][:, 3:], torch.zeros_like(ref[tag]["X"][:, 3:]))   # only X[:, :3] is read
    if tag == "ese":
        assert not ref[tag]["X"].any()
    else:
        assert ref[tag]["X"][:, :3].abs().max() > 0


def test_fixture_is_small_and_holds_arrays_only():
    path = os.path.join(GOLDEN_DIR, "kat_qm9_head_grads.npz")
    assert os.path.getsize(path) < 1 << 20
    g = np.load(path, allow_pickle=False)
    assert all(g[n].dtype == np.float64 for n in g.files)


def test_backward_entry_points_are_declared_and_bound():
    from gotennet_amd import _lib
    header = open(os.path.join(ROOT, "include", "gotennet_hip.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 11 and re.search(r"#define\s+GN_ABI_VERSION\s+11\b", header)
    # argument counts of the binding = the header's
    for name in NEW_ENTRY_POINTS:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
