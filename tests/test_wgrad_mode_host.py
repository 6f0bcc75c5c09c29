"""Host: the opt-in weight-gradient arithmetic (``wgrad_mode``): defaults, the C ABI of the two ``_mode`` entries, and a
torch emulation of the f16x2 scheme (fp16 planes, block exponents, three terms) against fp64."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gn_weight_grad_workspace_mode", "gn_weight_grad_group_mode")


# ---------------------------------------------------------------------------------------------------- defaults
def test_default_is_fp32():
    from gotennet_amd import engine
    assert engine.WGRAD_MODES == ("f32", "f16x2")
    assert engine.WGRAD_MODE == os.environ.get("GN_WGRAD_MODE", "f32")     # "f32" when the variable is unset


def test_modules_do_not_choose_an_arithmetic():
    import gotennet_amd
    import gotennet_amd.outputs as out
    kw = dict(n_atom_basis=16, n_interactions=1, n_rbf=4, num_heads=2, lmax=1, cutoff_fn=gotennet_amd.CosineCutoff(5.0))
    mods = [gotennet_amd.GotenNet(**kw), gotennet_amd.GotenNetWrapper(**kw),
            out.Atomwise(n_in=16), out.AtomwiseV3(n_in=16), out.GatedEquivariantBlock(8, 8, 4, 4, 8),
            out.Dipole(n_in=16), out.ElectronicSpatialExtentV2(n_in=16)]
    for m in mods:
        assert m.wgrad_mode is None, type(m).__name__
    dip = mods[5]
    dip.wgrad_mode = "f16x2"                         # forwarded to both blocks, like parameter_grads
    assert [b.wgrad_mode for b in dip.equivariant_layers] == ["f16x2", "f16x2"] and dip.wgrad_mode == "f16x2"
    net = mods[0]
    assert net.config().wgrad_mode == "f32"
    net.wgrad_mode = "f16x2"
    assert net.config().wgrad_mode == "f16x2"
    net.wgrad_mode = "bf16"
    with pytest.raises(ValueError):
        net.config()


def test_unknown_mode_is_refused_before_any_launch():
    from gotennet_amd import engine
    assert engine.resolve_wgrad_mode(None) == engine.WGRAD_MODE
    assert engine.resolve_wgrad_mode("f16x2") == "f16x2"
    with pytest.raises(ValueError):
        engine.resolve_wgrad_mode("bf16")
    with pytest.raises(ValueError):
        engine.weight_grad_group([], mode="bf16")    # before the problems are even looked at


# ---------------------------------------------------------------------------------------------------- C ABI
def test_entries_are_exported_declared_and_bound():
    from gotennet_amd import _lib
    header = open(os.path.join(ROOT, "include", "gotennet_hip.h")).read()
    lib = _lib.load()
    for name, ret in zip(ENTRIES, ("long", "int")):
        assert hasattr(lib, name), name
        decl = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.ABI_VERSION == 11 and re.search(r"#define\s+GN_ABI_VERSION\s+11\b", header)
    assert re.search(r"#define\s+GN_WGRAD_F32\s+0\b", header) and re.search(r"#define\s+GN_WGRAD_F16X2\s+2\b", header)
    assert (_lib.WGRAD_F32, _lib.WGRAD_F16X2) == (0, 2)


def _descs(shapes):
    from gotennet_amd import _lib
    arr = (_lib.WgradDesc * len(shapes))()
    for d, (rows, nout, K) in zip(arr, shapes):
        d.rows, d.nout, d.K, d.ldy, d.lda, d.ldw = rows, nout, K, nout, K, K
        d.row_cnt, d.row_gstride, d.row_goff = 1, 1, 0
    return arr


SHAPES = [(0, 1, 1), (1, 3, 20), (513, 33, 257), (2049, 96, 32), (54368, 1536, 256), (3000, 256, 512), (100000, 1, 64)]


def test_workspace_sizes():
    from gotennet_amd import _lib
    lib = _lib.load()
    for sh in SHAPES:
        one = _descs([sh])
        assert lib.gn_weight_grad_workspace_mode(one, 1, 0) == lib.gn_weight_grad_workspace(one, 1), sh
        rows, nout, K = sh
        assert lib.gn_weight_grad_workspace_mode(one, 1, 2) >= nout * K + nout > 0, sh
    arr = _descs(SHAPES)
    assert lib.gn_weight_grad_workspace_mode(arr, len(SHAPES), 0) == lib.gn_weight_grad_workspace(arr, len(SHAPES))
    assert lib.gn_weight_grad_workspace_mode(arr, len(SHAPES), 2) == sum(
        lib.gn_weight_grad_workspace_mode(_descs([sh]), 1, 2) for sh in SHAPES)


def test_unknown_mode_is_a_bad_argument():
    """n = 0: the launcher returns before it touches a device."""
    from gotennet_amd import _lib
    lib = _lib.load()
    for mode in (1, 3, -1, 7):
        assert lib.gn_weight_grad_group_mode(None, 0, mode, None, 0, None) == _lib.GN_ERR_BAD_ARG, mode
    for mode in (0, 2):
        assert lib.gn_weight_grad_group_mode(None, 0, mode, None, 0, None) == 0, mode


# ---------------------------------------------------------------------------------------------------- arithmetic
def _block_exp(m):
    """Block exponent of a block maximum: |x| < 2^(e + 15), clamped like the kernel's."""
    _, ex = torch.frexp(m)                           # m = f 2^ex, f in [0.5, 1)
    return torch.where(m > 0, ex - 15, torch.full_like(ex, -120)).clamp(-120, 113)


def emulate_f16x2(dY, A, stage=32, block=32):
    """dY^T A in the f16x2 scheme with the products summed in fp64: the error of the split alone."""
    rows, nout = dY.shape
    K = A.shape[1]
    mY, mA = torch.zeros(nout // block), torch.zeros(K // block)
    out = torch.zeros(nout, K, dtype=torch.float64)
    for r0 in range(0, rows, stage):
        y, a = dY[r0:r0 + stage], A[r0:r0 + stage]
        mY = torch.maximum(mY, y.abs().reshape(-1, nout // block, block).amax((0, 2)))   # running maxima only grow
        mA = torch.maximum(mA, a.abs().reshape(-1, K // block, block).amax((0, 2)))
        eY, eA = _block_exp(mY).repeat_interleave(block), _block_exp(mA).repeat_interleave(block)
        ys, as_ = torch.ldexp(y, -eY), torch.ldexp(a, -eA)
        yh, ah = ys.half(), as_.half()
        yl, al = (ys - yh.float()).half(), (as_ - ah.float()).half()
        yh, yl, ah, al = yh.double(), yl.double(), ah.double(), al.double()
        term = yh.t() @ ah + yh.t() @ al + yl.t() @ ah
        out += torch.ldexp(term, (eY[:, None] + eA[None, :]))
    return out


@pytest.mark.parametrize("kind", ["randn", "row_scales", "col_scales"])
def test_emulated_split_error(kind):
    g = torch.Generator().manual_seed(3)
    rows, nout, K = 8192, 64, 64
    dY, A = torch.randn(rows, nout, generator=g), torch.randn(rows, K, generator=g)
    if kind == "row_scales":
        s = torch.ldexp(torch.ones(rows), torch.randint(-20, 21, (rows,), generator=g))[:, None]
        dY, A = dY * s, A * s
    elif kind == "col_scales":
        dY = dY * torch.ldexp(torch.ones(nout), torch.randint(-12, 13, (nout,), generator=g))
        A = A * torch.ldexp(torch.ones(K), torch.randint(-12, 13, (K,), generator=g))
    ref = dY.double().t() @ A.double()
    err = float((emulate_f16x2(dY, A) - ref).abs().max() / ref.abs().max())
    print(f"{kind}: {err:.3e}")
    assert err <= 1e-6, (kind, err)
