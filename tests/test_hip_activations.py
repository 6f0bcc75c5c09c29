"""GPU: gn_gate, gn_gate_backward and gn_edge_gate_backward called directly, and through them the twelve activation kinds and the
four gates one function at a time: a dense sweep of 2^16 points over [-30, 30] plus the special points (tests/norm_util.py
sweep_points), value and derivative held to the per-function bound, +-Inf to torch's NaN / signed limit.  The sweep is also where
the device library's expf, expm1f, log1pf, tanhf and erff are measured in ulp and held to the allowances of norm_util.LIBM_ULP."""
import math

import pytest
import torch

from tests import norm_util as U
from tests.norm_gpu import SENTINEL, Out
from tests.norm_gpu import bits as _bits, dev as _dev, launch as _launch, lib as _lib, stream as _stream

pytestmark = pytest.mark.gpu

R = U.ratio
WORST = {}
SWEEP = {}                                         # kind -> (g_pre, g_wg) of the sweep, shared by the tests below


def _note(entry, rs, tag):
    print(f"{tag}: " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))
    for k, v in rs.items():
        WORST[entry + "." + k] = max(WORST.get(entry + "." + k, 0.0), v)
    assert all(v <= 1.0 for v in rs.values()), (tag, rs)


def _edge_gate(g, pre, wg, k):
    lib, st = _lib(), _stream()
    n = pre.numel()
    d = [_dev(t) for t in (g, pre, wg)]
    out = _launch(lambda o: lib.gn_edge_gate_backward(d[0].data_ptr(), d[1].data_ptr(), k, d[2].data_ptr(), n, o["g_pre"], o["g_wg"], st),
                  dict(g_pre=(n, 1), g_wg=(n, 1)))
    return out["g_pre"][:, 0], out["g_wg"][:, 0]


def _gate(x, g, kind):
    lib, st = _lib(), _stream()
    n = x.numel()
    dx, dg = _dev(x), _dev(g)
    out = _launch(lambda o: lib.gn_gate(dx.data_ptr(), kind, n, o["y"], st), dict(y=(n, 1)))
    out.update(_launch(lambda o: lib.gn_gate_backward(dg.data_ptr(), dx.data_ptr(), kind, n, o["gx"], st), dict(gx=(n, 1))))
    return out["y"][:, 0], out["gx"][:, 0]


def _sweep(k):
    """act(pre) and act'(pre) over the sweep through the edge-gate window: g = wg = 1."""
    if k not in SWEEP:
        x = U.sweep_points()
        SWEEP[k] = _edge_gate(torch.ones_like(x), x, torch.ones_like(x), k)
    return SWEEP[k]


# ------------------------------------------------------------------------------------------------ the element-wise entry points
@pytest.mark.parametrize("kind", range(4))
def test_gates_within_bound(kind):
    for n in U.GATE_N:
        x, g, _ = U.gate_inputs(n)
        y, gx = _gate(x, g, kind)
        rv, rd = U.ref_value_and_slope(U.REF_GATE[kind], x)
        by = U.bound_of(U.gate(U.RE, U.RE.load(x), kind))
        bg = U.bound_of(U.RE.load(g) * U.dgate(U.RE, U.RE.load(x), kind))
        _note("gn_gate", {f"kind{kind}": R(y, rv, by)}, f"kind {kind} n={n}")
        _note("gn_gate_backward", {f"kind{kind}": R(gx, g.double() * rd, bg)}, f"kind {kind} n={n}")


@pytest.mark.parametrize("k", [-1] + list(U.KINDS), ids=["identity"] + U.ACT_NAMES)
def test_edge_gate_backward_within_bound(k):
    for i, n in enumerate(U.GATE_N):
        x, g, wg = U.gate_inputs(n, seed=17)
        g_pre, g_wg = _edge_gate(g, x, wg, k)
        if k < 0:
            rv, rd = x.double(), torch.ones(n, dtype=torch.float64)
        else:
            rv, rd = U.ref_value_and_slope(U.REF_ACT[k], x)
        bp, bw = U.edge_gate_bwd(U.RE, g, x, wg, k)
        _note("gn_edge_gate_backward", {"g_pre": R(g_pre, g.double() * rd * wg.double(), U.bound_of(bp)),
                                        "g_wg": R(g_wg, g.double() * rv, U.bound_of(bw))}, f"act {k} n={n}")


def test_zero_size_calls_touch_nothing():
    lib, st = _lib(), _stream()
    d = _dev(torch.randn(8))
    p = d.data_ptr()
    o = Out(8, 1, fill=SENTINEL)
    for kind in range(4):
        assert lib.gn_gate(p, kind, 0, o.ptr(), st) == 0 and lib.gn_gate_backward(p, p, kind, 0, o.ptr(), st) == 0
    for k in [-1] + list(U.KINDS):
        assert lib.gn_edge_gate_backward(p, p, k, p, 0, o.ptr(), o.ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool((o.t == SENTINEL).all())


def test_non_finite_stays_in_its_element():
    x, g, wg = U.gate_inputs(1028, seed=3)
    bad = x.clone()
    bad[100], bad[601] = math.nan, math.inf
    keep = torch.ones(1028, dtype=torch.bool)
    keep[100], keep[601] = False, False
    for kind in range(4):
        clean, dirty = _gate(x, g, kind), _gate(bad, g, kind)
        for a, b in zip(clean, dirty):
            assert torch.equal(_bits(a[keep]), _bits(b[keep])), kind
    for k in (-1, U.SILU, U.MISH, U.GELU):
        clean, dirty = _edge_gate(g, x, wg, k), _edge_gate(g, bad, wg, k)
        for a, b in zip(clean, dirty):
            assert torch.equal(_bits(a[keep]), _bits(b[keep])), k
        assert bool(torch.isnan(dirty[1][100])), k                            # g_wg = g act(pre)


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("k", U.KINDS, ids=U.ACT_NAMES)
def test_activation_sweep_within_bound(k):
    x = U.sweep_points()
    fin = torch.isfinite(x)
    d, a = _sweep(k)
    rv, rd = U.ref_value_and_slope(U.REF_ACT[k], x)
    xs = U.RE.load(x)
    ba, bd = U.bound_of(U.act(U.RE, xs, k)).expand_as(rv), U.bound_of(U.dact(U.RE, xs, k)).expand_as(rv)
    _note("activation", {f"{U.ACT_NAMES[k]}.act": R(a[fin], rv[fin], ba[fin]), f"{U.ACT_NAMES[k]}.dact": R(d[fin], rd[fin], bd[fin])},
          U.ACT_NAMES[k])
    assert U.same_class(a[~fin], rv[~fin]), (a[~fin].tolist(), rv[~fin].tolist())
    assert U.same_class(d[~fin], rd[~fin]), (d[~fin].tolist(), rd[~fin].tolist())


@pytest.mark.parametrize("kind", range(4))
def test_gate_sweep_within_bound(kind):
    x = U.sweep_points()
    fin = torch.isfinite(x)
    y, gx = _gate(x, torch.ones_like(x), kind)
    rv, rd = U.ref_value_and_slope(U.REF_GATE[kind], x)
    xs = U.RE.load(x)
    by = U.bound_of(U.gate(U.RE, xs, kind)).expand_as(rv)
    bg = U.bound_of(U.RE.load(torch.ones_like(x)) * U.dgate(U.RE, xs, kind)).expand_as(rv)
    _note("gate", {f"gate{kind}": R(y[fin], rv[fin], by[fin]), f"dgate{kind}": R(gx[fin], rd[fin], bg[fin])}, f"gate {kind}")
    assert U.same_class(y[~fin], rv[~fin]) and U.same_class(gx[~fin], rd[~fin])
    if kind:                                                                 # the same functions as the activation kinds: the same bits
        d, a = _sweep({1: U.SIGMOID, 2: U.TANH, 3: U.SILU}[kind])
        assert torch.equal(_bits(y[fin]), _bits(a[fin])) and torch.equal(_bits(gx[fin]), _bits(d[fin]))


def _ulps(got, ref):
    """|got - ref| in units of the last place of ref (fp32), over the results that are normal numbers."""
    ref = ref.double()
    live = torch.isfinite(ref) & (ref.abs() >= U.MIN_NORMAL)
    e = torch.frexp(ref[live].abs())[1] - 1                                  # floor(log2 |ref|)
    return float(((got.double()[live] - ref[live]).abs() / torch.exp2((e - 23).double())).max())


def test_libm_ulp_errors_are_inside_their_allowances():
    """expf = ELU'(x <= 0); expm1f = ELU(x <= 0); tanhf = tanh(x); log1pf = softplus(x <= 0) taken at the device's own expf(x);
    erff from GELU(x) = (0.5 x)(1 + erff(x / sqrt 2)) where 1 + erf <= 1 / 16: the sum is exact there and the one rounding of the
    product is below 1 / 16 of erf's last place, so erff's bits are recovered exactly."""
    x = U.sweep_points()
    x64 = x.double()
    neg = torch.isfinite(x) & (x <= 0)
    elu_d, elu_a = _sweep(U.ELU)
    got = {"expf": _ulps(elu_d[neg], torch.exp(x64[neg])), "expm1f": _ulps(elu_a[neg], torch.expm1(x64[neg])),
           "tanhf": _ulps(_sweep(U.TANH)[1][torch.isfinite(x)], torch.tanh(x64[torch.isfinite(x)]))}
    arg = elu_d[neg]                                                         # the device's expf(x): log1pf's actual argument
    live = arg >= U.MIN_NORMAL
    got["log1pf"] = _ulps(_sweep(U.SOFTPLUS)[1][neg][live], torch.log1p(arg[live].double()))
    a32 = (x * torch.tensor(U.SQRT1_2, dtype=torch.float32)).double()        # the fp32 product the kernel forms
    erf = torch.erf(a32)
    win = torch.isfinite(x) & (x < 0) & (1.0 + erf <= 1.0 / 16.0)
    units = _sweep(U.GELU)[1].double()[win] / (0.5 * x64[win]) * 2.0 ** 24   # (1 + erff) in units of 2^-24
    assert float((units - units.round()).abs().max()) < 0.25
    got["erff"] = float(((units.round() * 2.0 ** -24 - 1.0) - erf[win]).abs().max() * 2.0 ** 24)
    print("libm worst error in ulp: " + " ".join(f"{k}={v:.3f}" for k, v in got.items()) + f"   (erff over {int(win.sum())} points)")
    for name, v in got.items():
        recorded, allow = U.LIBM_ULP[name]
        assert v <= allow <= 4, (name, v, allow)
        assert allow == math.floor(v) + 1 and abs(v - recorded) < 5e-3, (name, v, U.LIBM_ULP[name])


def test_worst_ratios_per_entry_point():
    print("worst error / bound: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())))
    assert WORST and all(v <= 1.0 for v in WORST.values())
