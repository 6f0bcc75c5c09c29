"""Yardstick of the norm, gate, activation and head kernels: gn_layernorm, gn_layernorm_silu and their backwards
(csrc/gn_node.hip, gn_backward.hip), gn_layernorm_param_grad (gn_wgrad.hip), gn_tensor_norm and its backward, gn_gate,
gn_gate_backward, gn_edge_gate_backward (gn_options.hip, gn_highl.h), the twelve activation kinds (gn_common.h) and
gn_head_energy / gn_head_grad (gn_backward.hip).  CPU only: fp64 restatements, an a-priori per-element error bound, an fp32
emulation in the kernels' operation order, the case tables and the mutations that prove their power.

The contracts:
    LayerNorm     xh = (x - mean) / sqrt(var + eps), var biased;  y = act(xh gamma + beta)  (act absent: the bare affine form)
                  g = g_out act'(xh gamma + beta) gamma;  g_x = rstd (g - mean(g) - xh mean(g xh))
                  dgamma[c] = sum_n g_out act' xh,  dbeta[c] = sum_n g_out act'   (64-row chunks, then the chunks in order; N = 0: zeros)
    TensorLayerNorm per (atom, degree): s_f = |X_l[:, f]|, c_f = max(s_f, eps), n_f = (c_f - min c) / (max c - min c) (the
                  denominator 1 when max = min), Y = relu(n_f) X / c_f w_f.  Backward with torch's routing: max / min send their
                  gradient to the FIRST extremal channel, the clamp passes it where s >= eps, relu'(0) = 0, the norm's
                  subgradient at 0 is 0.
    gates         kind 0 identity | 1 sigmoid | 2 tanh | 3 SiLU;  gn_gate_backward: g gate'(x)
    edge gate     t' = t + act(pre) wg:  g_pre = g act'(pre) wg,  g_wg = g act(pre)   (act = -1: the identity)
    activations   torch.nn.functional's: softplus with threshold 20, shifted softplus = softplus - ln 2, erf-GELU, SELU's two
                  constants, leaky slope 0.01, ELU'(x <= 0) = e^x, relu'(0) = 0, leaky'(0) = 0.01
    head          y_n = (sum_k act(pre1[n, k]) W2[k] + b2) scale + shift + atomref[z_n];  E = agg_{n in mol} y_n + mol_shift,
                  agg = sum | mean (an empty molecule: 0);  atom_scale[n] = 1 | 1 / n_mol(n);  g_pre1 = scale atom_scale W2 act'

The restatement is fp64 torch (torch.nn.functional, the oracle's tensor_layernorm and atomwise_*) on the fp32 inputs; the
backwards are fp64 autograd.  A second, closed-form statement -- the kernels' expressions over the ``F64`` arithmetic -- is
proved equal to it by tests/test_norm_host.py; the emulation is the same transcript over ``F32``, the bound the same transcript
over ``RE``.

The bounds (u = U32 = 2^-24; the library is built without fast-math and with -ffp-contract=off).  A RUNNING ERROR pass: every
spelled fp32 operation adds u |result| + 2^-126 (a flushed subnormal) to the first-order propagation of its operands' errors,
as in tests/geometry_util.py; fmaf rounds once; max, min and the selects add nothing.  No constant is fitted.
  sums          the pass walks the kernel's own order -- a lane's serial partial sum over f = lane, lane + 64, ..., then the six
                butterfly steps (offsets 1 .. 32; the parameter-gradient statistics 32 .. 1) -- so a term meets at most F / 64 + 6
                additions, each charged on the magnitude of its partial sum.
  LayerNorm     the mean's error rides through x - mean and is multiplied by rstd: a constant row gets the large but honest
                bound ~ rstd u |x| (F / 64 + 7).  No row is exempt.
  TensorLayerNorm  the divisions by delta, c and c^2 are spelled in the transcript: their factors are carried, not estimated.
  fast SiLU     sigmoid_fast = v_rcp_f32(1 + v_exp_f32(-x log2 e)): 1 ulp for each instruction, the rounded product
                x log2 e gives 2^-24 |x log2 e| relative on the exponential (the model above fast_exp in gn_common.h).
  libm          expf, expm1f, log1pf, tanhf, erff carry LIBM_ULP ulp (k ulp <= 2 k u |f|) on top of sup |f'| e_arg.
  cancelling expressions (1 - t^2, softplus - ln 2, 1 + erf for x < 0, s (1 - s)) are bounded absolutely by construction.
A piecewise activation behind a COMPUTED argument (LayerNorm + activation) is only bounded where the argument cannot change
side: the case tables keep |v| >= 64 bound(v) for the kinked kinds (``KINKED``), asserted from the reference alone.  On direct
inputs (edge gate, head gradient) the kink is tested at exactly 0 and +- the smallest normal.
"""
import functools
import math

import torch
import torch.nn.functional as Fn

from oracle import gotennet_oracle as orc
from tests.gather_util import FLOOR, U32
from tests.geometry_util import f32c, ratio  # noqa: F401  (ratio: re-exported for the tests)

#: function -> (worst error measured on MI355X over the sweep of tests/test_hip_activations.py, in ulp; the allowance = the
#: next integer above it).  The allowance is what the bounds use; DESIGN.md section 2 carries the same table.
LIBM_ULP = {"expf": (0.775, 1), "expm1f": (0.831, 1), "log1pf": (0.539, 1), "tanhf": (1.094, 2), "erff": (0.652, 1)}
TINY = 1e-300
LOG2E = 1.44269504088896341
SQRT1_2 = 0.70710678118654752
INV_SQRT_2PI = 0.39894228040143268
LN2 = 0.69314718055994531
SELU_L, SELU_A = 1.0507009873554805, 1.6732632423543772
MIN_NORMAL = 2.0 ** -126
EPS_LN, EPS_TLN = 1e-5, 1e-12

SILU, SSP, RELU, TANH, SIGMOID, ELU, SELU, MISH, GELU, SOFTPLUS, LEAKY, NONE = range(12)     # GN_ACT_* of gotennet_hip.h
ACT_NAMES = ["silu", "ssp", "relu", "tanh", "sigmoid", "elu", "selu", "mish", "gelu", "softplus", "leaky", "none"]
KINDS = range(12)
KINKED = (RELU, ELU, SELU, LEAKY)                  # piecewise: the argument may not change side (RELU', LEAKY', SELU' jump)
MARGIN = 64.0


def ulp_allow(name):
    return LIBM_ULP[name][1]


# ------------------------------------------------------------------------------------------------ arithmetics
class _Plain:
    """A tensor of one dtype under the operations the kernels spell; one rounding per operation."""
    dtype = None
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = v

    def _w(self, v):
        return type(self)(v)

    def __add__(a, b):
        return a._w(a.v + b.v)

    def __sub__(a, b):
        return a._w(a.v - b.v)

    def __mul__(a, b):
        return a._w(a.v * b.v)

    def __truediv__(a, b):
        return a._w(a.v / b.v)

    def __neg__(a):
        return a._w(-a.v)

    def fma(a, b, c):                              # fmaf(a, b, c): the product is exact in fp64
        return a._w((a.v.double() * b.v.double() + c.v.double()).to(a.dtype))

    def sqrt(a):
        return a._w(torch.sqrt(a.v))

    def _fn(a, f):                                 # transcendental: taken in fp64, then rounded
        return a._w(f(a.v.double()).to(a.dtype))

    def exp(a):
        return a._fn(torch.exp)

    def expm1(a):
        return a._fn(torch.expm1)

    def log1p(a):
        return a._fn(torch.log1p)

    def tanh(a):
        return a._fn(torch.tanh)

    def erf(a):
        return a._fn(torch.erf)

    def exp2_hw(a):
        return a._fn(torch.exp2)

    def rcp_hw(a):
        return a._fn(torch.reciprocal)

    def maximum(a, b):
        return a._w(torch.maximum(a.v, b.v))

    def gt(a, k=0.0):
        return a.v > k

    def take(a, idx):                              # lanes / columns of the last axis
        return a._w(a.v[..., idx])

    def pick(a, rows, cols):
        return a._w(a.v[rows, cols])

    def col(a):
        return a._w(a.v[..., None])

    def row(a, n):
        return a._w(a.v[n])

    @classmethod
    def const(cls, k):
        return cls(torch.tensor(k if cls.dtype == torch.float64 else f32c(k), dtype=cls.dtype))

    @classmethod
    def load(cls, t):
        return cls(torch.as_tensor(t).to(cls.dtype))

    @classmethod
    def where(cls, m, a, b):
        return cls(torch.where(m, a.v, b.v))

    @classmethod
    def stack(cls, xs, dim=0):
        return cls(torch.stack([x.v for x in xs], dim))

    @classmethod
    def cat(cls, xs, dim=0):
        return cls(torch.cat([x.v for x in xs], dim))

    def value(a):
        return a.v


class F64(_Plain):
    """The closed-form restatement: exact literals, fp64 throughout."""
    dtype = torch.float64
    __slots__ = ()


class F32(_Plain):
    """The emulation: torch fp32 on the CPU in the kernels' literal operation order."""
    dtype = torch.float32
    __slots__ = ()


class RE:
    """(fp64 value, bound on |fp32 result - value|): the running-error pass."""
    __slots__ = ("v", "e")

    def __init__(self, v, e):
        self.v, self.e = v, e

    @staticmethod
    def _r(v, p, k=1.0):                           # k u |result| for the rounding (k = 2 ulp-count for a library function)
        return RE(v, p + k * U32 * (v.abs() + p) + FLOOR)

    def __add__(a, b):
        return RE._r(a.v + b.v, a.e + b.e)

    def __sub__(a, b):
        return RE._r(a.v - b.v, a.e + b.e)

    def __mul__(a, b):
        return RE._r(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)

    def __truediv__(a, b):
        v = a.v / b.v
        return RE._r(v, (a.e + v.abs() * b.e) / (b.v.abs() - b.e).clamp_min(TINY))

    def __neg__(a):
        return RE(-a.v, a.e)

    def fma(a, b, c):
        return RE._r(a.v * b.v + c.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e + c.e)

    def sqrt(a):
        v = torch.sqrt(a.v)
        return RE._r(v, torch.minimum(a.e / (torch.sqrt((a.v - a.e).clamp_min(0)) + v).clamp_min(TINY), torch.sqrt(a.e)))   # |dsqrt| <= sqrt|d|

    def _near(a):                                  # the point of [v - e, v + e] closest to 0: where |f'| of tanh, erf peaks
        return (a.v.abs() - a.e).clamp_min(0)

    def exp(a):
        v = torch.exp(a.v)
        return RE._r(v, v * torch.expm1(a.e), 2 * ulp_allow("expf"))

    def expm1(a):
        return RE._r(torch.expm1(a.v), torch.exp(a.v) * torch.expm1(a.e), 2 * ulp_allow("expm1f"))

    def log1p(a):                                  # arguments >= 0 here
        return RE._r(torch.log1p(a.v), a.e / (1.0 + a.v - a.e).clamp_min(TINY), 2 * ulp_allow("log1pf"))

    def tanh(a):
        return RE._r(torch.tanh(a.v), a.e * (1.0 - torch.tanh(a._near()) ** 2), 2 * ulp_allow("tanhf"))

    def erf(a):
        return RE._r(torch.erf(a.v), a.e * (2.0 / math.sqrt(math.pi)) * torch.exp(-a._near() ** 2), 2 * ulp_allow("erff"))

    def exp2_hw(a):                                # v_exp_f32: 1 ulp
        v = torch.exp2(a.v)
        return RE._r(v, v * torch.expm1(math.log(2.0) * a.e), 2.0)

    def rcp_hw(a):                                 # v_rcp_f32: 1 ulp
        v = 1.0 / a.v
        return RE._r(v, a.e / (a.v.abs() * (a.v.abs() - a.e).clamp_min(TINY)).clamp_min(TINY), 2.0)

    def maximum(a, b):                             # 1-Lipschitz in both arguments, no rounding
        return RE(torch.maximum(a.v, b.v), torch.maximum(a.e, b.e))

    def gt(a, k=0.0):
        return a.v > k

    def take(a, idx):
        return RE(a.v[..., idx], a.e[..., idx])

    def pick(a, rows, cols):
        return RE(a.v[rows, cols], a.e[rows, cols])

    def col(a):
        return RE(a.v[..., None], a.e[..., None])

    def row(a, n):
        return RE(a.v[n], a.e[n])

    @classmethod
    def const(cls, k):
        return cls(torch.tensor(float(k), dtype=torch.float64), torch.tensor(abs(f32c(k) - float(k)), dtype=torch.float64))

    @classmethod
    def load(cls, t):
        t = torch.as_tensor(t).double()
        return cls(t, torch.zeros(t.shape, dtype=torch.float64))

    @classmethod
    def where(cls, m, a, b):
        return cls(torch.where(m, a.v, b.v), torch.where(m, a.e, b.e))

    @classmethod
    def stack(cls, xs, dim=0):
        return cls(torch.stack([x.v for x in xs], dim), torch.stack([x.e.expand_as(x.v) for x in xs], dim))

    @classmethod
    def cat(cls, xs, dim=0):
        return cls(torch.cat([x.v for x in xs], dim), torch.cat([x.e.expand_as(x.v) for x in xs], dim))

    def value(a):
        return a.v


def bound_of(x):
    """The accumulated running error of an RE number, broadcast to its value's shape, + the underflow floor."""
    return x.e.expand_as(x.v) + FLOOR


# ------------------------------------------------------------------------------------------------ activations (gn_common.h)
def sigmoid_fast(ar, x):
    if ar is F64:
        return F64(torch.sigmoid(x.v))
    return (ar.const(1.0) + (ar.const(LOG2E) * (-x)).exp2_hw()).rcp_hw()


def sigmoid_lib(ar, x):
    return ar.const(1.0) / (ar.const(1.0) + (-x).exp())


def softplus_t(ar, x, mut=None):
    sp = x.exp().log1p()
    return sp if mut == "softplus_no_threshold" else ar.where(x.gt(20.0), x, sp)


def act(ar, x, k, mut=None):
    """act1(x, k) in its literal expression order."""
    c = ar.const
    if k == SILU:
        return x * sigmoid_fast(ar, x)
    if k == SSP:
        return softplus_t(ar, x, mut) if mut == "ssp_no_shift" else softplus_t(ar, x, mut) - c(LN2)
    if k == RELU:
        return x.maximum(c(0.0))
    if k == TANH:
        return x.tanh()
    if k == SIGMOID:
        return sigmoid_lib(ar, x)
    if k == ELU:
        return ar.where(x.gt(), x, x.expm1())
    if k == SELU:
        lam, al = (SELU_A, SELU_L) if mut == "selu_swapped" else (SELU_L, SELU_A)
        return c(lam) * ar.where(x.gt(), x, c(al) * x.expm1())
    if k == MISH:
        return x * softplus_t(ar, x, mut).tanh()
    if k == GELU:
        if mut == "gelu_tanh":
            inner = c(math.sqrt(2.0 / math.pi)) * (x + c(0.044715) * x * x * x)
            return c(0.5) * x * (c(1.0) + inner.tanh())
        return c(0.5) * x * (c(1.0) + (x * c(SQRT1_2)).erf())
    if k == SOFTPLUS:
        return softplus_t(ar, x, mut)
    if k == LEAKY:
        return ar.where(x.gt(), x, c(0.1 if mut == "leaky_slope" else 0.01) * x)
    assert k == NONE
    return x


def dact(ar, x, k, mut=None):
    """dact1(x, k) in its literal expression order."""
    c = ar.const
    one = c(1.0)
    if k == SILU:
        s = sigmoid_fast(ar, x)
        return s * (one + x * (one - s))
    if k in (SSP, SOFTPLUS):
        s = sigmoid_lib(ar, x)
        return s if mut == "softplus_no_threshold" else ar.where(x.gt(20.0), one, s)
    if k == RELU:
        return step(ar, x, 1.0, 0.0)
    if k == TANH:
        t = x.tanh()
        return one - t * t
    if k == SIGMOID:
        s = sigmoid_lib(ar, x)
        return s * (one - s)
    if k == ELU:
        return x.exp() if mut == "elu_prime_exp" else ar.where(x.gt(), one, x.exp())
    if k == SELU:
        lam, al = (SELU_A, SELU_L) if mut == "selu_swapped" else (SELU_L, SELU_A)
        return c(lam) * ar.where(x.gt(), one, c(al) * x.exp())
    if k == MISH:
        t, s = softplus_t(ar, x, mut).tanh(), sigmoid_lib(ar, x)
        return t if mut == "mish_second_term" else t + x * s * (one - t * t)
    if k == GELU:
        if mut == "gelu_tanh":
            k0 = math.sqrt(2.0 / math.pi)
            t = (c(k0) * (x + c(0.044715) * x * x * x)).tanh()
            return c(0.5) * (one + t) + c(0.5) * x * (one - t * t) * c(k0) * (one + c(3 * 0.044715) * x * x)
        return c(0.5) * (one + (x * c(SQRT1_2)).erf()) + x * c(INV_SQRT_2PI) * (c(-0.5) * x * x).exp()
    if k == LEAKY:
        return step(ar, x, 1.0, 0.1 if mut == "leaky_slope" else 0.01)
    assert k == NONE
    return ar.load(torch.ones_like(x.v))


def step(ar, x, hi, lo):
    """x > 0 ? hi : lo, the two literals rounded as the arithmetic rounds a literal."""
    m = x.gt()
    t = lambda k: torch.tensor(float(k), dtype=torch.float64)
    if ar is RE:
        return RE(torch.where(m, t(hi), t(lo)), torch.where(m, t(abs(f32c(hi) - hi)), t(abs(f32c(lo) - lo))))
    return ar.where(m, ar.const(hi), ar.const(lo))


def gate(ar, x, kind, mut=None):
    """gate1(x, kind)."""
    if mut == "gate_kinds_exchanged" and kind in (1, 2):
        kind = 3 - kind
    if kind == 1:
        return sigmoid_lib(ar, x)
    if kind == 2:
        return x.tanh()
    if kind == 3:
        return x * sigmoid_fast(ar, x)
    return x


def dgate(ar, x, kind, mut=None):
    if mut == "gate_kinds_exchanged" and kind in (1, 2):
        kind = 3 - kind
    one = ar.const(1.0)
    if kind == 1:
        s = sigmoid_lib(ar, x)
        return s * (one - s)
    if kind == 2:
        t = x.tanh()
        return one - t * t
    if kind == 3:
        return dact(ar, x, SILU)
    return ar.load(torch.ones_like(x.v))


#: the restatement proper: torch.nn.functional in fp64
REF_ACT = {SILU: Fn.silu, SSP: orc.shifted_softplus, RELU: Fn.relu, TANH: torch.tanh, SIGMOID: torch.sigmoid, ELU: Fn.elu,
           SELU: Fn.selu, MISH: Fn.mish, GELU: Fn.gelu, SOFTPLUS: Fn.softplus, LEAKY: Fn.leaky_relu, NONE: lambda x: x}
REF_GATE = {0: lambda x: x, 1: torch.sigmoid, 2: torch.tanh, 3: Fn.silu}
for _k, _name in enumerate(ACT_NAMES[:-1]):                                  # (kind 9 is the un-shifted torch softplus)
    assert _k == SOFTPLUS or REF_ACT[_k] is orc.activation_of({"ssp": "softplus", "leaky": "leakyrelu"}.get(_name, _name)), _name


def ref_value_and_slope(fn, x32):
    """fn and d fn / dx in fp64 on the fp32 points: torch's own forward and autograd."""
    with torch.enable_grad():
        x = x32.double().clone().requires_grad_(True)
        y = fn(x)
        if not y.requires_grad:
            return y.detach(), torch.zeros_like(y)
        (d,) = torch.autograd.grad(y.sum(), x)
    return y.detach(), d


def edge_gate_bwd(ar, g, pre, wg, k, mut=None):
    """edge_gate_bwd_kernel: -> (g_pre, g_wg)."""
    g, p, w = ar.load(g), ar.load(pre), ar.load(wg)
    if k < 0:
        return g * w, g * p
    return (g * dact(ar, p, k, mut)) * w, g * act(ar, p, k, mut)


def sweep_points(n_grid=1 << 16):
    """The dense grid over [-30, 30] and the special points; a multiple of 4 long, +-Inf last."""
    sp = [0.0, MIN_NORMAL, 1e-6, 19.99, 20.0, 20.01, 88.0, 100.0]
    x = torch.cat([torch.linspace(-30.0, 30.0, n_grid, dtype=torch.float64).float(),
                   torch.tensor(sp + [-v for v in sp], dtype=torch.float32)])
    inf = torch.tensor([math.inf, -math.inf, math.inf, -math.inf])
    pad = (-(x.numel() + 4)) % 4
    return torch.cat([x, torch.zeros(pad), inf]).contiguous()


def same_class(got, ref):
    """Where the reference is not finite the result is the same NaN / signed infinity; elsewhere it is finite."""
    got, ref = got.double(), ref.double()
    nf = ~torch.isfinite(ref)
    ok = torch.where(torch.isnan(ref), torch.isnan(got), got == ref)
    return bool(ok[nf].all()) and bool(torch.isfinite(got[~nf]).all())


# ------------------------------------------------------------------------------------------------ wave reductions
_LANES = torch.arange(64)
UP, DOWN = (1, 2, 4, 8, 16, 32), (32, 16, 8, 4, 2, 1)      # wave_sum (xor_add<1> .. <32>) | the __shfl_xor loop of gn_wgrad.hip


def lane_sum(ar, x, order=UP):
    """sum over the last axis as a wave does it: lane l adds f = l, l + 64, ... serially, then the xor butterfly."""
    F = x.v.shape[-1]
    zero = ar.load(torch.zeros(()))
    acc = None
    for t in range(-(-F // 64)):
        f = t * 64 + _LANES
        live = f < F
        xt = x.take(f.clamp(max=F - 1))
        acc = ar.where(live, xt, zero) if acc is None else ar.where(live, acc + xt, acc)      # 0.f + x is exact
    for off in order:
        acc = acc + acc.take(_LANES ^ off)
    return acc.take(0)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_stats(ar, x, eps, order=UP, mut=None):
    """-> (x - mean is recomputed by the callers) mean [N], rstd [N]."""
    F = x.v.shape[-1]
    Ff = ar.load(torch.tensor(float(F)))
    mean = lane_sum(ar, x, order) / Ff
    d = x - mean.col()
    var = lane_sum(ar, d * d, order) / (ar.load(torch.tensor(float(F - 1))) if mut == "unbiased_variance" else Ff)
    e = ar.load(torch.tensor(f32c(eps)))
    rstd = ar.const(1.0) / ((var.sqrt() + e) if mut == "eps_outside_root" else (var + e).sqrt())
    return mean, rstd


def ln_forward(ar, c, k=None, mut=None, want_arg=False):
    """layernorm_kernel<SILU>: k None: gn_layernorm, else gn_layernorm_silu with kind k."""
    x, gamma, beta = ar.load(c["x"]), ar.load(c["gamma"]), ar.load(c["beta"])
    mean, rstd = ln_stats(ar, x, c["eps"], UP, mut)
    v = (x - mean.col()) * rstd.col() * gamma + beta
    if want_arg:
        return v
    return v if k is None else act(ar, v, k)


def ln_backward(ar, c, k=None, mut=None):
    """layernorm_bwd_kernel<SILU>."""
    x, gamma, beta, go = ar.load(c["x"]), ar.load(c["gamma"]), ar.load(c["beta"]), ar.load(c["g"])
    F = x.v.shape[-1]
    Ff = ar.load(torch.tensor(float(F)))
    mean, rstd = ln_stats(ar, x, c["eps"], UP, mut)
    xh = (x - mean.col()) * rstd.col()
    if k is None:
        g = go * ar.const(1.0)
    else:
        g = go * dact(ar, xh if mut == "act_prime_at_xh" else xh * gamma + beta, k)
    if mut != "gamma_missing":
        g = g * gamma
    s1 = lane_sum(ar, g) / Ff
    s2 = lane_sum(ar, g * xh) / Ff
    r = g
    if mut != "mean_g_dropped":
        r = r - s1.col()
    else:
        r = r - ar.load(torch.zeros(()))
    if mut != "xh_term_dropped":
        r = r - xh * s2.col()
    return rstd.col() * r


def ln_reference(c, k=None):
    """fp64: torch.nn.functional.layer_norm (+ the activation) and autograd.  -> (y, g_x)."""
    F = c["x"].shape[1]
    with torch.enable_grad():
        x = c["x"].double().clone().requires_grad_(True)
        y = Fn.layer_norm(x, (F,), c["gamma"].double(), c["beta"].double(), f32c(c["eps"]))
        if k is not None:
            y = REF_ACT[k](y)
        (gx,) = torch.autograd.grad((y * c["g"].double()).sum(), x) if c["x"].numel() else (torch.zeros_like(x),)
    return y.detach(), gx


def ln_margin(c, k):
    """min |v| / bound(v) of the activation's argument over the case: the side of a kink is certain above 1."""
    v = ln_forward(RE, c, want_arg=True)
    return float((v.v.abs() / bound_of(v)).min()) if v.v.numel() else math.inf


LN_F = (1, 4, 48, 63, 64, 65, 96, 200, 256, 1024)
LN_N = (1, 3, 4, 5, 9)
ROW_PLAN = ("rand", "const0", "const1", "zerograd", "rand", "const1000", "mean1e4", "rand", "rand")
#: (F, N, act, first row kind): the twelve kinds over every width and row count, then the widths again under other kinds
LN_CASES = [(LN_F[i % 10], LN_N[i % 5], i, 0) for i in KINDS] + [
    (256, 9, RELU, 0), (200, 9, SELU, 0), (1024, 4, LEAKY, 5), (64, 9, SILU, 0), (65, 5, MISH, 5), (48, 3, GELU, 5),
    (63, 9, ELU, 0), (96, 4, TANH, 5), (1024, 9, SSP, 0), (256, 4, SILU, 5)]


def ln_id(n):
    F, N, k, sh = LN_CASES[n]
    return f"F{F}-N{N}-{ACT_NAMES[k]}-r{sh}"


def row_kinds(n):
    F, N, k, sh = LN_CASES[n]
    return [ROW_PLAN[(r + sh) % len(ROW_PLAN)] for r in range(N)]


@functools.lru_cache(maxsize=None)
def ln_case(n):
    F, N, k, sh = LN_CASES[n]
    g = torch.Generator().manual_seed(1000 + n)
    rn = lambda *s: torch.randn(*s, generator=g)
    kinds = row_kinds(n)
    x, go = rn(N, F), rn(N, F)
    for r, kind in enumerate(kinds):
        if kind.startswith("const"):
            x[r] = float(kind[5:])
        elif kind == "mean1e4":
            x[r] = 1e4 + rn(F)
        elif kind == "zerograd":
            go[r] = 0.0
    sign = torch.where(torch.rand(F, generator=g) < 0.5, -1.0, 1.0)
    dominant = k in KINKED and any(kind in ("const1000", "mean1e4") for kind in kinds)
    if dominant:                                   # the argument keeps beta's side whatever the row: |gamma| <= 0.04, |beta| in [1, 2]
        gamma = (torch.rand(F, generator=g) - 0.5) * 0.08
        beta = sign * (1.0 + torch.rand(F, generator=g))
    else:
        gamma = rn(F)
        beta = sign * (0.25 + torch.rand(F, generator=g))
    if F >= 4:
        gamma[::7] = 0.0
        gamma[1] = -gamma[1].abs() - 0.01
    return dict(F=F, N=N, act=k, eps=EPS_LN, kinds=kinds, dominant=dominant, id=ln_id(n), x=x.contiguous(), g=go.contiguous(),
                gamma=gamma.contiguous(), beta=beta.contiguous())


@functools.lru_cache(maxsize=None)
def ln_expected(n):
    """-> dict of (reference, bound) for y, ya (activated), gx, gxa of case n, computed once."""
    c = ln_case(n)
    k = c["act"]
    y, gx = ln_reference(c)
    ya, gxa = ln_reference(c, k)
    return dict(y=(y, bound_of(ln_forward(RE, c))), ya=(ya, bound_of(ln_forward(RE, c, k))),
                gx=(gx, bound_of(ln_backward(RE, c))), gxa=(gxa, bound_of(ln_backward(RE, c, k))))


# ------------------------------------------------------------------------------------------------ LayerNorm parameter gradients
LN_ROWS = 64
PG_N = (0, 1, 63, 64, 65, 130)
PG_C = (1, 48, 255, 256, 257, 300)
#: (N, C, act, dbeta NULL, beta NULL)
PG_CASES = [(0, 48, NONE, False, False), (1, 1, SILU, False, False), (63, 255, TANH, False, False), (64, 256, MISH, True, False),
            (65, 257, NONE, True, True), (130, 300, SILU, False, False), (130, 48, TANH, True, False), (0, 300, SILU, False, False)]


def pg_workspace(N, C):
    return 2 * (-(-N // LN_ROWS)) * C


@functools.lru_cache(maxsize=None)
def pg_case(n):
    N, C, k, no_dbeta, no_beta = PG_CASES[n]
    g = torch.Generator().manual_seed(2000 + n)
    rn = lambda *s: torch.randn(*s, generator=g).contiguous()
    x = rn(N, C)
    if N >= 63:
        x[5] = 3.0                                  # a constant row and an offset one among the rest
        x[7] = 50.0 + x[7]
    return dict(N=N, C=C, act=k, eps=EPS_LN, no_dbeta=no_dbeta, no_beta=no_beta, x=x, g=rn(N, C), gamma=rn(C), beta=rn(C),
                id=f"N{N}-C{C}-{ACT_NAMES[k]}{'-nodbeta' if no_dbeta else ''}{'-nobeta' if no_beta else ''}")


def pg_transcript(ar, c, mut=None):
    """ln_param_partial_kernel + ln_param_reduce_kernel.  -> (dgamma [C], dbeta [C])."""
    N, C, k = c["N"], c["C"], c["act"]
    zero = ar.load(torch.zeros(C))
    dgs, dbs = [], []
    x, go, gamma, beta = ar.load(c["x"]), ar.load(c["g"]), ar.load(c["gamma"]), ar.load(c["beta"])
    if N:
        mean, rstd = ln_stats(ar, x, c["eps"], DOWN)
    for r0 in range(0, N, LN_ROWS):
        dg, db = zero, zero
        for r in range(r0, min(r0 + LN_ROWS, N)):
            xr = x.row(r)
            xh = (xr - mean.row(r)) * rstd.row(r)
            gz = go.row(r)
            if k != NONE:
                gz = gz * dact(ar, xh * gamma + beta, k)
            dg = gz.fma(xr if mut == "dgamma_from_x" else xh, dg)
            db = db + gz
        dgs.append(dg)
        dbs.append(db)
    dg, db = zero, zero
    for a, b in zip(dgs, dbs):
        dg, db = dg + a, db + b
    return dg, db


def pg_reference(c):
    N, C, k = c["N"], c["C"], c["act"]
    if N == 0:
        return torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    with torch.enable_grad():
        gamma = c["gamma"].double().clone().requires_grad_(True)
        beta = c["beta"].double().clone().requires_grad_(True)
        y = REF_ACT[k](Fn.layer_norm(c["x"].double(), (C,), gamma, beta, f32c(c["eps"])))
        dg, db = torch.autograd.grad((y * c["g"].double()).sum(), (gamma, beta))
    return dg, db


# ------------------------------------------------------------------------------------------------ TensorLayerNorm
TN_F = (1, 4, 63, 64, 65, 200, 256)
TN_N = (1, 2, 3, 5)
TN_CASES = [(1, 1, 1), (2, 4, 2), (3, 63, 3), (4, 64, 5), (5, 65, 1), (6, 200, 2), (7, 256, 3), (8, 64, 5), (3, 200, 5), (2, 256, 3),
            (8, 1, 2), (1, 65, 5)]                  # (lmax, F, N)
BLOCK_PLAN = ("rand", "zero_channel", "tie_max2", "tiny_channel", "tie_min2", "eps_channel", "all_equal", "tie_max3", "tie_min3",
              "zero_and_tiny", "tie_both")
TIE_KINDS = tuple(k for k in BLOCK_PLAN if k.startswith("tie"))


def tn_dim(lmax):
    return (lmax + 1) ** 2 - 1


def tn_id(n):
    lmax, F, N = TN_CASES[n]
    return f"l{lmax}-F{F}-N{N}"


def _pyth(cnt, scale, variant):
    """A vector of norm exactly 5 scale (scale a power of two) over cnt components: (3, 4, 0 ..) and its rearrangements."""
    v = torch.zeros(cnt)
    a, b = [(0, 1), (2, 0), (1, 2), (0, 2)][variant % 4]
    v[a], v[b] = 3.0 * scale, (-4.0 if variant % 2 else 4.0) * scale
    return v


def tie_channels(F, m):
    """m channels in different lanes and, from F = 65 on, in different 64-strides (below: whatever F holds)."""
    want = [3, 70, 133][:m] if F > 133 else ([3, 64][:m] if m == 2 and F > 64 else [F // 7, F // 2, F - 1][:m])
    want = sorted(set(min(w, F - 1) for w in want))
    return want


@functools.lru_cache(maxsize=None)
def tn_case(n):
    lmax, F, N = TN_CASES[n]
    D = tn_dim(lmax)
    g = torch.Generator().manual_seed(3000 + n)
    X = torch.zeros(N, D, F)
    eps32 = f32c(EPS_TLN)
    plan = {}
    for a in range(N):
        for l in range(1, lmax + 1):
            kind = BLOCK_PLAN[(a * lmax + l - 1 + n) % len(BLOCK_PLAN)]
            cnt, off = 2 * l + 1, l * l - 1
            while True:                            # norms in [0.5, 1.5], the two largest and the two smallest 1e-4 apart
                blk = torch.randn(cnt, F, generator=g)
                blk = blk / blk.norm(dim=0, keepdim=True) * (0.5 + torch.rand(F, generator=g))
                srt = blk.double().norm(dim=0).sort()[0]
                if F < 2 or (float(srt[1] / srt[0]) > 1.001 and float(srt[-1] / srt[-2]) > 1.001):
                    break
            if kind in ("zero_channel", "zero_and_tiny"):
                blk[:, F // 3] = 0.0
            if kind in ("tiny_channel", "zero_and_tiny") and F > 1:
                blk[:, (F // 3 + 1) % F] = 1e-13
            if kind == "eps_channel":
                blk[:, F // 2] = 0.0
                blk[cnt // 2, F // 2] = eps32
            if kind == "all_equal":
                for f in range(F):
                    blk[:, f] = _pyth(cnt, 0.25, f)
            if kind in ("tie_max2", "tie_max3", "tie_both"):
                for i, f in enumerate(tie_channels(F, 3 if kind == "tie_max3" else 2)):
                    blk[:, f] = _pyth(cnt, 1.0, i)
            if kind in ("tie_min2", "tie_min3", "tie_both"):
                for i, f in enumerate(tie_channels(F, 3 if kind == "tie_min3" else 2)):
                    blk[:, (f + 1) % F] = _pyth(cnt, 2.0 ** -5, i + 1)
            X[a, off:off + cnt] = blk
            plan[(a, l)] = kind
    w = torch.randn(F, generator=g)
    if F >= 4:
        w[2] = 0.0
        w[3] = -w[3].abs() - 0.1
    return dict(lmax=lmax, F=F, N=N, D=D, eps=EPS_TLN, X=X.contiguous(), w=w.contiguous(), plan=plan, id=tn_id(n),
                g=torch.randn(N, D, F, generator=g).contiguous())


def _first_index(mask):
    """[.., F] bool -> [..] the first True index."""
    F = mask.shape[-1]
    return torch.where(mask, torch.arange(F), torch.full((), F)).min(-1)[0]


def tn_transcript(ar, c, backward=False, mut=None):
    """tensor_norm_kernel / tensor_norm_bwd_kernel over every (atom, degree) block.  -> Y or g_X [N, D, F] (and, for the backward,
    the routed channels amx, amn [N, lmax])."""
    lmax, F, N = c["lmax"], c["F"], c["N"]
    eps = ar.load(torch.tensor(f32c(c["eps"])))
    zero, one = ar.load(torch.zeros(())), ar.load(torch.ones(()))
    w = ar.load(c["w"])
    outs, route = [], []
    for l in range(1, lmax + 1):
        cnt, off = 2 * l + 1, l * l - 1
        x = [ar.load(c["X"][:, off + m]) for m in range(cnt)]                # cnt numbers [N, F]
        gy = [ar.load(c["g"][:, off + m]) for m in range(cnt)]
        q = ar.load(torch.zeros(N, F))
        for m in range(cnt):
            q = x[m].fma(x[m], q)
        s = q.sqrt()
        cc = s if mut == "eps_clamp_missing" else s.maximum(eps)
        cv = cc.v
        mxv, mnv = cv.max(-1, keepdim=True)[0], cv.min(-1, keepdim=True)[0]
        amx, amn = _first_index(cv == mxv), _first_index(cv == mnv)
        if mut == "last_extremal":
            amx, amn = F - 1 - _first_index((cv == mxv).flip(-1)), F - 1 - _first_index((cv == mnv).flip(-1))
        rows = torch.arange(N)
        mx, mn = cc.pick(rows, amx).col(), cc.pick(rows, amn).col()          # max / min: exact selections
        flat = (mx.v - mn.v) == 0
        delta = ar.where(flat & (mut != "flat_not_reset"), one, mx - mn)
        nf = (cc - mn) / delta
        rn = nf.maximum(zero)
        if not backward:
            outs.append(ar.stack([(rn * (x[m] / cc)) * w for m in range(cnt)], 1))
            continue
        G = ar.load(torch.zeros(N, F))
        for m in range(cnt):
            G = (gy[m] * w).fma(x[m], G)
        pos = (nf.v >= 0) if mut == "relu_mask_ge" else nf.gt()
        dn = ar.where(pos, G / cc, zero)
        s1, s2 = lane_sum(ar, dn).col(), lane_sum(ar, dn * (cc - mn)).col()
        d_delta = ar.where(flat, zero, (-s2) / (delta * delta))
        d_mx = d_delta
        d_mn = ((-s1) / delta + d_delta) if mut == "d_mn_sign" else ((-s1) / delta - d_delta)
        dc = (-rn) * G / (cc * cc) + dn / delta
        ch = torch.arange(F)[None, :]
        dc = ar.where(ch == amx[:, None], dc + d_mx, dc)
        dc = ar.where(ch == amn[:, None], dc + d_mn, dc)
        live = (s.v > 0) if mut == "clamp_mask_dropped" else ((s.v >= eps.v) & (s.v > 0))
        k = ar.where(live, dc / ar.where(s.v > 0, s, one), zero)
        outs.append(ar.stack([gy[m] * w * rn / cc + k * x[m] for m in range(cnt)], 1))
        route.append((amx, amn))
    out = ar.cat(outs, 1)
    if backward:
        return out, torch.stack([r[0] for r in route], 1), torch.stack([r[1] for r in route], 1)
    return out


def tn_reference(c):
    """fp64: the oracle's tensor_layernorm and autograd.  -> (Y, g_X)."""
    with torch.enable_grad():
        X = c["X"].double().clone().requires_grad_(True)
        Y = orc.tensor_layernorm(X, c["lmax"], c["w"].double(), f32c(c["eps"]))
        (gX,) = torch.autograd.grad((Y * c["g"].double()).sum(), X)
    return Y.detach(), gX


def tn_norm_gaps(c):
    """Per block: the relative gaps between the two largest and the two smallest clamped norms (fp64) -- 0 (a tie) or >= 1e-4."""
    gaps = []
    if c["F"] < 2:
        return gaps
    for l in range(1, c["lmax"] + 1):
        cnt, off = 2 * l + 1, l * l - 1
        cc = c["X"][:, off:off + cnt].double().norm(dim=1).clamp(min=f32c(c["eps"]))
        srt = cc.sort(-1)[0]
        gaps += ((srt[:, -1] - srt[:, -2]) / srt[:, -1]).tolist() + ((srt[:, 1] - srt[:, 0]) / srt[:, 1]).tolist()
    return gaps


@functools.lru_cache(maxsize=None)
def tn_expected(n):
    c = tn_case(n)
    Y, gX = tn_reference(c)
    gb, amx, amn = tn_transcript(RE, c, True)
    return dict(Y=(Y, bound_of(tn_transcript(RE, c))), gX=(gX, bound_of(gb)), amx=amx, amn=amn)


# ------------------------------------------------------------------------------------------------ gates
GATE_N = (0, 4, 1020, 1024, 1028, 4100)
SPECIAL = (0.0, MIN_NORMAL, -MIN_NORMAL, 1e-6, -1e-6, 19.99, 20.0, 20.01, -20.0, 88.0, -88.0, 100.0, -100.0)


@functools.lru_cache(maxsize=None)
def gate_inputs(n, seed=0):
    """x [n] (the special points first when they fit), g [n], wg [n]."""
    g = torch.Generator().manual_seed(4000 + n + seed)
    x = torch.randn(n, generator=g) * 3.0
    sp = torch.tensor(SPECIAL[:n] if n < len(SPECIAL) else SPECIAL)
    x[:sp.numel()] = sp
    return x.contiguous(), torch.randn(n, generator=g).contiguous(), torch.randn(n, generator=g).contiguous()


# ------------------------------------------------------------------------------------------------ energy head
HEAD_HD = (1, 32, 63, 64, 65, 200)
MOL_SIZES = (1, 15, 0, 16, 17, 64, 65, 70)
#: (Hd, molecule sizes, act, atomref, atom_scale): the twelve kinds, then the 1030-atom molecule
HEAD_CASES = [(HEAD_HD[i % 6], MOL_SIZES, i, i % 2 == 0, i % 3 != 0) for i in KINDS] + [(32, (3, 1030, 0), SILU, True, True),
                                                                                        (200, MOL_SIZES, GELU, False, False)]


def head_id(n):
    Hd, sizes, k, ref, asc = HEAD_CASES[n]
    return f"Hd{Hd}-A{sum(sizes)}-{ACT_NAMES[k]}{'-atomref' if ref else ''}{'-ascale' if asc else ''}"


@functools.lru_cache(maxsize=None)
def head_case(n):
    Hd, sizes, k, use_ref, use_asc = HEAD_CASES[n]
    A = sum(sizes)
    g = torch.Generator().manual_seed(5000 + n)
    rn = lambda *s: torch.randn(*s, generator=g).contiguous()
    pre1 = rn(A, Hd) * 1.5
    flat = pre1.view(-1)
    sp = torch.tensor([0.0, MIN_NORMAL, -MIN_NORMAL])                        # the kink on a direct input
    flat[:min(3, flat.numel())] = sp[:min(3, flat.numel())]
    mol_ptr = torch.zeros(len(sizes) + 1, dtype=torch.int32)
    mol_ptr[1:] = torch.tensor(sizes).cumsum(0).to(torch.int32)
    return dict(Hd=Hd, A=A, sizes=sizes, n_mol=len(sizes), act=k, use_ref=use_ref, use_asc=use_asc, pre1=pre1, W2=rn(Hd),
                b2=f32c(0.37), scale=f32c(1.7), shift=f32c(-0.21), mol_shift=f32c(2.5), atomref=rn(7) * 3.0,
                z=torch.randint(0, 7, (A,), generator=g).to(torch.int32), mol_ptr=mol_ptr, id=head_id(n))


def head_transcript(ar, c, mean, mut=None):
    """head_energy_kernel + head_grad_kernel.  -> dict(y [A], energy [n_mol], atom_scale [A], g_pre1 [A, Hd])."""
    k, A, Hd = c["act"], c["A"], c["Hd"]
    k32 = lambda v: ar.load(torch.tensor(v))
    pre, W2 = ar.load(c["pre1"]), ar.load(c["W2"])
    b2, scale, shift, mshift = k32(c["b2"]), k32(c["scale"]), k32(c["shift"]), k32(c["mol_shift"])
    s = lane_sum(ar, act(ar, pre, k) * W2) if A else ar.load(torch.zeros(0))
    y = ((s + b2 + shift) * scale) if mut == "shift_inside_scale" else ((s + b2) * scale + shift)
    if c["use_ref"] and mut != "atomref_omitted":
        y = y + ar.load(c["atomref"][c["z"].long()])
    if mut == "mol_shift_per_atom":
        y = y + mshift
    ptr = c["mol_ptr"].tolist()
    en, cnts = [], torch.ones(A)
    for b in range(c["n_mol"]):
        n0, n1 = ptr[b], ptr[b + 1]
        e = lane_sum(ar, y.take(slice(n0, n1))) if n1 > n0 else ar.load(torch.zeros(()))
        if mean and n1 > n0:
            e = e / k32(float(n1 - n0 + (1 if mut == "mean_wrong_count" else 0)))
            cnts[n0:n1] = float(n1 - n0)
        en.append(e if mut == "mol_shift_per_atom" else e + mshift)
    energy = ar.stack(en) if en else ar.load(torch.zeros(0))
    a_scale = (ar.const(1.0) / ar.load(cnts)) if mut != "atom_scale_not_inverse" else ar.load(cnts)
    sc = (scale * a_scale) if c["use_asc"] else ar.load(torch.full((A,), c["scale"]))
    g_pre1 = (sc.col() * W2) * dact(ar, pre, k)
    return dict(y=y, energy=energy, atom_scale=a_scale, g_pre1=g_pre1)


def head_reference(c, mean):
    """fp64.  The gradient is autograd of sum_mol E when atom_scale is passed, of scale-only (`sum` semantics) when it is NULL."""
    k, A = c["act"], c["A"]
    batch = torch.repeat_interleave(torch.arange(c["n_mol"]), torch.tensor(c["sizes"]))
    cnt = torch.tensor(c["sizes"], dtype=torch.float64)
    with torch.enable_grad():
        pre = c["pre1"].double().clone().requires_grad_(True)
        y = (REF_ACT[k](pre) @ c["W2"].double() + c["b2"]) * c["scale"] + c["shift"]
        if c["use_ref"]:
            y = y + c["atomref"].double()[c["z"].long()]
        agg = torch.zeros(c["n_mol"], dtype=torch.float64).index_add_(0, batch, y)
        if mean:
            agg = agg / cnt.clamp(min=1)
        energy = agg + c["mol_shift"]
        tot = energy.sum() if c["use_asc"] else y.sum()
        (gp,) = torch.autograd.grad(tot, pre)
    a_scale = (1.0 / cnt[batch]) if mean else torch.ones(A, dtype=torch.float64)
    return dict(y=y.detach(), energy=energy.detach(), atom_scale=a_scale, g_pre1=gp)


@functools.lru_cache(maxsize=None)
def head_expected(n, mean):
    c = head_case(n)
    ref, b = head_reference(c, mean), head_transcript(RE, c, mean)
    return {key: (ref[key], bound_of(b[key])) for key in ref}


#: mutation -> family.  Each is a mutation of the fp32 EMULATION: it must breach the bound on a case or break a named exact demand.
MUTATIONS = {
    "unbiased_variance": "ln", "eps_outside_root": "ln", "mean_g_dropped": "ln", "xh_term_dropped": "ln", "act_prime_at_xh": "ln",
    "gamma_missing": "ln", "dgamma_from_x": "pg",
    "last_extremal": "tn", "relu_mask_ge": "tn", "clamp_mask_dropped": "tn", "d_mn_sign": "tn", "flat_not_reset": "tn",
    "eps_clamp_missing": "tn",
    "ssp_no_shift": "act", "softplus_no_threshold": "act", "selu_swapped": "act", "gelu_tanh": "act", "mish_second_term": "act",
    "leaky_slope": "act", "elu_prime_exp": "act", "gate_kinds_exchanged": "gate",
    "shift_inside_scale": "head", "mean_wrong_count": "head", "atomref_omitted": "head", "atom_scale_not_inverse": "head",
    "mol_shift_per_atom": "head",
}
