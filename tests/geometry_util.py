"""Yardstick of the two ends of the force path: gn_edge_geometry (K1), gn_cosine_cutoff, gn_node_init (K2), gn_edge_init (K3)
and their backwards gn_node_init_backward, gn_edge_init_backward, gn_edge_geometry_backward, gn_pos_scatter (csrc/gn_edge.hip,
gn_backward.hip) with the `_images` entry points.  CPU only: an fp64 restatement of the contracts, an a-priori per-element
error bound, an fp32 emulation in the kernels' operation order, the case table and the mutations that prove its power.

The contracts, for edge e = (j -> i) with vector v, distance d (a SEPARATE input), cutoff c:
    loop(e) = j == i                      (index rule)      or      j == i and d == 0          (`_images`: a self-image is a real edge)
    u = v / |v|  (v itself on a loop);  rl = harmonics(u);  cut = 0.5 (cos(pi d / c) + 1) [d < c]
    phi = cut exp(-beta (exp(-alpha d) - mu)^2), alpha = 5 / c   |   sin(a d) / d   |   exp(-0.5 (d - o)^2 / w^2)          (basis 0 | 1 | 2)
    backward of  sum <G_rl, rl> + <G_phi, phi> + G_cut cut  to v (through u only) and to d; G_rl, G_cut are the fixed-order sums of
    n_rl / n_cut slices at stride E D / E; a loop row is exactly zero.
    g_pos[n] = sign (sum_{src = n} gv - sum_{dst = n} gv),  gv = g_vec + g_diff v / |v|  (the g_diff term dropped where g_diff == 0)
    K2: ctx[i, :F] = A_na[z_i];  ctx[i, F:] = sum_{e -> i, not loop} A_nbr[z_j] (fn[e] cut[e]);   K3: t[e] = (h_i + h_j) fe[e]
    K2 backward: g_fn[e] = g_m[i] A_nbr[z_j] cut[e] (0 on a loop);  g_cut[e] = sum_f g_m A_nbr fn, as max(1, F / 256) slices
    K3 backward: g_fe[e] = g_t[e] (h_i + h_j);  g_h[n] += sum_{dst = n} g_t fe + sum_{src = n} g_t fe

The restatement is fp64 torch on the fp32 inputs: the harmonics, the cutoff and the three bases are the oracle's functions, the
backward is fp64 autograd of the scalar above.  A second, closed-form statement (``transcript`` with the ``F64`` arithmetic)
follows the kernels' expressions; tests/test_geometry_host.py proves the two equal, and the mutations are mutations of it.

The bounds (u = U32 = 2^-24; the library is built without fast-math and with -ffp-contract=off: every rounding is one the source
spells).  No constant is fitted.  K1 and its backward are bounded by a RUNNING ERROR pass: the same transcript run on (value,
error) pairs (``RE``), where every operation adds u |result| to the first-order propagation of its operands' errors --
    a + b: ea + eb;   a b: |a| eb + |b| ea + ea eb;   a / b: (ea + |a / b| eb) / (|b| - eb);   sqrt a: ea / (sqrt(a - ea) + sqrt a)
-- division and sqrtf are correctly rounded (one u); a literal contributes |fp32(k) - k| (0 for 0.5, 2, 3, 4, 0.75); the raise
coefficients of degrees 5..8 are oracle.harmonic_raise_table rounded to fp32; expf carries the project's allowance of 2 ulp =
4 u (gather_util), sinf and cosf TRIG_ULP ulp on top of |f'| e_arg + e_arg^2 / 2.  The result is the accumulated error + 2^-126.
The bound is absolute and built from the magnitudes of the terms, so cancellation (the projection g_u - (g_u . u) u, the Bessel
derivative a cos(a d) / d - sin(a d) / d^2) is admitted by construction.
gn_pos_scatter: per edge the RE pass of gv (division, sqrt, the product and the add); per atom a lane adds its edges, six
  butterfly steps, the sign: (deg_in + deg_out + 3) u sum |gv|  +  sum e_gv.
K2: f = fn cut one product, the fma chain of a slot, the ns slot partials in order: (1 + chain(deg)) u sum |A fn cut|,
  chain(d) = ceil(d / ns) + ns + 1 (gather_util).  ctx[:, :F] is a copy.   K3: the add, the product: 2 u (|h_i| + |h_j|) |fe|.
K2 backward: g_fn = (g_m A) cut: 2 u |g_fn|;  g_cut: two products, hsum4 two adds, log2(w) butterfly steps, the slices added in
  fp64 by the test (or by the geometry backward, whose RE pass counts them): (5 + log2 w) u sum_f |g_m A fn|.
K3 backward: g_fe: 2 u |g_t| (|h_i| + |h_j|);  g_h: the fma chains over incoming and outgoing edges share one accumulator,
  the slot partials, the add into the old value: (ceil(din / ns) + ceil(dout / ns) + ns + 2) u (sum |g_t fe| + |g_h old|).
"""
import functools
import math

import numpy as np
import torch

from oracle import gotennet_oracle as orc
from tests.gather_util import FLOOR, U32, slots

EXP_ULP = 2                                        # expf: the project's allowance (gather_util: "expf 2 ulp (4 u)")
TRIG_ULP = 2                                       # sinf / cosf of the device library; measured by the GPU test of `cut`; may not exceed 4
PI32 = float(np.float32(math.pi))                  # 3.14159265358979323846f
TINY = 1e-300


def ndim(lmax):
    return (lmax + 1) ** 2 - 1


def f32c(k):
    return float(np.float32(k))


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
        return NotImplemented if isinstance(b, Dual) else a._w(a.v + b.v)

    def __sub__(a, b):
        return NotImplemented if isinstance(b, Dual) else a._w(a.v - b.v)

    def __mul__(a, b):
        return NotImplemented if isinstance(b, Dual) else a._w(a.v * b.v)

    def __truediv__(a, b):
        return a._w(a.v / b.v)

    def __neg__(a):
        return a._w(-a.v)

    def sqrt(a):
        return a._w(torch.sqrt(a.v))

    def _fn(a, f):                                 # transcendental: taken in fp64, then rounded
        return a._w(f(a.v.double()).to(a.dtype))

    def cos(a):
        return a._fn(torch.cos)

    def sin(a):
        return a._fn(torch.sin)

    def exp(a):
        return a._fn(torch.exp)

    @classmethod
    def const(cls, k):
        return cls(torch.tensor(k if cls.dtype == torch.float64 else f32c(k), dtype=cls.dtype))

    @classmethod
    def load(cls, t):
        return cls(t.to(cls.dtype))

    @classmethod
    def where(cls, m, a, b):
        return cls(torch.where(m, a.v, b.v))

    def value(a):
        return a.v


class F64(_Plain):
    """The closed-form restatement: exact literals (sqrt(3), not its fp32 rounding), fp64 throughout."""
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
    def _r(v, p):
        return RE(v, p + U32 * (v.abs() + p))

    def __add__(a, b):
        return NotImplemented if isinstance(b, Dual) else RE._r(a.v + b.v, a.e + b.e)

    def __sub__(a, b):
        return NotImplemented if isinstance(b, Dual) else RE._r(a.v - b.v, a.e + b.e)

    def __mul__(a, b):
        if isinstance(b, Dual):
            return NotImplemented
        return RE._r(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)

    def __truediv__(a, b):
        v = a.v / b.v
        return RE._r(v, (a.e + v.abs() * b.e) / (b.v.abs() - b.e).clamp_min(TINY))

    def __neg__(a):
        return RE(-a.v, a.e)

    def sqrt(a):
        v = torch.sqrt(a.v)
        return RE._r(v, a.e / (torch.sqrt((a.v - a.e).clamp_min(0)) + v).clamp_min(TINY))

    def _trig(a, v, dv):
        p = dv.abs() * a.e + 0.5 * a.e * a.e
        return RE(v, p + 2 * TRIG_ULP * U32 * (v.abs() + p))

    def cos(a):
        return a._trig(torch.cos(a.v), torch.sin(a.v))

    def sin(a):
        return a._trig(torch.sin(a.v), torch.cos(a.v))

    def exp(a):
        v = torch.exp(a.v)
        p = v * torch.expm1(a.e)
        return RE(v, p + 2 * EXP_ULP * U32 * (v + p))

    @classmethod
    def const(cls, k):
        return cls(torch.tensor(float(k), dtype=torch.float64), torch.tensor(abs(f32c(k) - float(k)), dtype=torch.float64))

    @classmethod
    def load(cls, t):
        return cls(t.double(), torch.zeros(t.shape, dtype=torch.float64))

    @classmethod
    def where(cls, m, a, b):
        return cls(torch.where(m, a.v, b.v), torch.where(m, a.e, b.e))

    def value(a):
        return a.v


class Dual:
    """Dual3 of gn_backward.hip: a value and its three partial derivatives, over any of the arithmetics above."""
    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v, self.d = v, d

    def __add__(a, b):
        return Dual(a.v + b.v, [p + q for p, q in zip(a.d, b.d)])

    def __sub__(a, b):
        return Dual(a.v - b.v, [p - q for p, q in zip(a.d, b.d)])

    def __neg__(a):
        return Dual(-a.v, [-p for p in a.d])

    def __mul__(a, b):
        if isinstance(b, Dual):
            return Dual(a.v * b.v, [a.v * q + p * b.v for p, q in zip(a.d, b.d)])
        return Dual(b * a.v, [b * p for p in a.d])

    __rmul__ = __mul__


# ------------------------------------------------------------------------------------------------ harmonics (gn_sh.h, gn_sh_high.h)
@functools.lru_cache(maxsize=None)
def raise_terms(l):
    """The non-zero (i, j, a, T) of degree l's raise table, in the generated header's order: j, then a, ascending."""
    T = orc.harmonic_raise_table(l)
    return [[(j, a, float(T[i, j, a])) for j in range(2 * l - 1) for a in range(3) if T[i, j, a] != 0] for i in range(2 * l + 1)]


def harmonics(ar, lmax, x, y, z, mut=None):
    """real_harmonics<LMAX, T> in its literal expression order, over plain numbers or Duals of the arithmetic ``ar``."""
    k = ar.const
    o = [x, y, z]
    if lmax >= 2:
        r3 = k(math.sqrt(3.0))
        y2 = y * y
        x2z2 = x * x + z * z
        o += [r3 * x * z, r3 * x * y, y2 - k(0.5) * x2z2, r3 * y * z, k(math.sqrt(3.0) / 2.0) * (z * z - x * x)]
    if lmax >= 3:
        a, b, c = k(math.sqrt(42) / 6), k(math.sqrt(7)), k(math.sqrt(168) / 8)
        hb = k(math.sqrt(7) / 2)
        s2 = o[3:8]
        o += [a * (s2[0] * z + s2[4] * x), b * s2[0] * y, c * (k(4.0) * y2 - x2z2) * x,
              hb * y * (k(2.0) * y2 - k(3.0) * x2z2), c * z * (k(4.0) * y2 - x2z2), b * s2[4] * y, a * (s2[4] * z - s2[0] * x)]
    if lmax >= 4:
        q = math.sqrt
        k0, k1, k2, k3, k4 = k(0.75 * q(2)), k(0.75), k(3 / 8 * q(6)), k(3 / 56 * q(14)), k(3 / 14 * q(21))
        k5, k6, k7, k8, k9, k10 = k(3 / 56 * q(210)), k(3 / 56 * q(42)), k(3 / 28 * q(105)), k(3 / 28 * q(70)), k(3 / 28 * q(42)), k(3 / 7 * q(7))
        s3 = o[8:15]
        o += [k0 * (s3[0] * z + s3[6] * x),
              k1 * s3[0] * y + k2 * s3[1] * z + k2 * s3[5] * x,
              -k3 * s3[0] * z + k4 * s3[1] * y + k5 * s3[2] * z + k5 * s3[4] * x + k3 * s3[6] * x,
              -k6 * s3[1] * z + k7 * s3[2] * y + k8 * s3[3] * x + k6 * s3[5] * x,
              -k9 * s3[2] * x + k10 * s3[3] * y - k9 * s3[4] * z,
              -k6 * s3[1] * x + k8 * s3[3] * z + k7 * s3[4] * y - k6 * s3[5] * z,
              -k3 * s3[0] * x - k5 * s3[2] * x + k5 * s3[4] * z + k4 * s3[5] * y - k3 * s3[6] * z,
              -k2 * s3[1] * x + k2 * s3[5] * z + k1 * s3[6] * y,
              k0 * (-s3[0] * x + s3[6] * z)]
    r = (x, y, z)
    for l in range(5, lmax + 1):
        s = o[l * l - 2 * l:l * l - 1]                                       # the degree below: rows (l-1)^2 - 1 .. l^2 - 2
        for i, terms in enumerate(raise_terms(l)):
            acc = None
            for n, (j, a, t) in enumerate(terms):
                if mut == "raise_coeff" and l == 6 and i == 4 and n == 1:
                    t *= 1.0 + 1e-4
                term = k(t) * (s[j] * r[a])
                acc = term if acc is None else acc + term
            if mut == "row_sign" and l == 5 and i == 3:
                acc = -acc
            o.append(acc)
    assert len(o) == ndim(lmax)
    return o


# ------------------------------------------------------------------------------------------------ self-loop rules (gn_common.h self_loop)
def loop_mask(c, rule=None):
    """rule "index": j == i;  "images": j == i and d == 0.  Default: the rule of the case's entry point."""
    rule = rule or ("images" if c["images"] else "index")
    same = c["src"] == c["dst"]
    return same if rule == "index" else same & (c["diff"] == 0)


# ------------------------------------------------------------------------------------------------ K1 and its backward: the transcript
def _cutoff_terms(ar, c, d):
    k = ar.const
    cutoff = k(c["cutoff"])
    arg = d * k(math.pi) / cutoff
    return arg, k(0.5) * (arg.cos() + k(1.0))


def k1_forward(ar, c, mut=None):
    """edge_sh_kernel + edge_rbf_kernel.  -> dict(rl [E, D], cut [E], phi [E, R]) of ``ar`` numbers."""
    k = ar.const
    E, R, basis, cutoff = c["E"], c["R"], c["basis"], c["cutoff"]
    loop = loop_mask(c)
    x, y, z = (ar.load(c["vec"][:, n]) for n in range(3))
    nrm = (x * x + y * y + z * z).sqrt()
    x, y, z = (ar.where(loop, p, p / nrm) for p in (x, y, z))
    rl = harmonics(ar, c["lmax"], x, y, z, mut)
    d = ar.load(c["diff"])
    inside = (c["diff"] <= cutoff) if mut == "cut_le" else (c["diff"] < cutoff)
    zero = ar.load(torch.zeros(E))
    cut = ar.where(inside, _cutoff_terms(ar, c, d)[1], zero)
    d2, p0, p1 = ar.load(c["diff"][:, None]), ar.load(c["p0"][None, :]), ar.load(c["p1"][None, :])
    if basis == 1:
        den = ar.where(c["diff"][:, None] == 0, ar.load(torch.ones(E, 1)), d2)
        phi = (d2 * p0).sin() / den
    elif basis == 2:
        q = d2 - p0
        phi = ((k(-0.5) / (p1 * p1)) * (q * q)).exp()
    else:
        c2 = ar.where(inside[:, None], _cutoff_terms(ar, c, d2)[1], ar.load(torch.zeros(E, 1)))
        u = (k(5.0 / cutoff) * (-d2)).exp() - p0
        phi = c2 * ((-p1) * (u * u)).exp()
    return dict(rl=rl, cut=cut, phi=phi)


def k1_backward(ar, c, mut=None):
    """edge_geometry_bwd_kernel.  -> dict(g_vec [3 x E], g_diff [E]) of ``ar`` numbers; loop rows are zero."""
    k = ar.const
    E, R, D, basis, cutoff = c["E"], c["R"], ndim(c["lmax"]), c["basis"], c["cutoff"]
    loop = loop_mask(c, "index" if mut == "loop_rule" else None)
    if mut == "loop_kept":
        loop = torch.zeros(E, dtype=torch.bool)
    zero = ar.load(torch.zeros(E))
    d = ar.load(c["diff"])
    gphi = [ar.load(c["g_phi"][:, r]) for r in range(R)]
    P0, P1 = [ar.load(c["p0"][r]) for r in range(R)], [ar.load(c["p1"][r]) for r in range(R)]
    gd = zero
    if basis == 1:
        for r in range(R):
            ad = P0[r] * d
            t = P0[r] * ad.cos() / d
            if mut != "bessel_second":
                t = t - ad.sin() / (d * d)
            gd = gd + gphi[r] * t
    elif basis == 2:
        for r in range(R):
            q = d - P0[r]
            c2 = k(-0.5) / (P1[r] * P1[r])
            gd = gd + gphi[r] * (c2 * (q * q)).exp() * (k(2.0) * c2 * q)
    inside = (c["diff"] <= cutoff) if mut == "cut_le" else (c["diff"] < cutoff)
    arg, cc = _cutoff_terms(ar, c, d)
    dc = (k(-0.5) if mut == "cut_pi" else k(-0.5) * (k(math.pi) / k(cutoff))) * arg.sin()
    s = zero
    if basis == 0:
        alpha = k(5.0 / cutoff)
        u = (alpha * (-d)).exp()
        for r in range(R):
            w = u - P0[r]
            G = ((-P1[r]) * (w * w)).exp()
            inner = k(2.0) * P1[r] * w if mut == "expnorm_chain" else k(2.0) * P1[r] * w * alpha * u
            s = s + gphi[r] * G * (dc + cc * inner)
    gc = zero
    for q in range(c["n_cut"] - (1 if mut == "cut_slice" else 0)):
        gc = gc + ar.load(c["g_cut"][q])
    g_diff = ar.where(inside, gd + (s + gc * dc), gd)
    x, y, z = (ar.load(c["vec"][:, n]) for n in range(3))
    nrm = (x * x + y * y + z * z).sqrt()
    u3 = [x / nrm, y / nrm, z / nrm]
    one, nul = ar.load(torch.ones(E)), zero
    seeds = ([one, nul, nul], [nul, one, nul], [nul, nul, one])
    o = harmonics(ar, c["lmax"], *(Dual(u3[n], seeds[n]) for n in range(3)), mut=mut)
    gsum = [zero] * D
    for q in range(c["n_rl"] - (1 if mut == "rl_slice" else 0)):
        gsum = [gsum[m] + ar.load(c["g_rl"][q, :, m]) for m in range(D)]
    gu = [zero, zero, zero]
    for m in range(D):
        gu = [gu[n] + gsum[m] * o[m].d[n] for n in range(3)]
    dotp = gu[0] * u3[0] + gu[1] * u3[1] + gu[2] * u3[2]
    den = nrm * nrm if mut == "inv_norm_sq" else nrm
    g_vec = [(gu[n] if mut == "no_projection" else gu[n] - dotp * u3[n]) / den for n in range(3)]
    return dict(g_vec=[ar.where(loop, zero, g) for g in g_vec], g_diff=ar.where(loop, zero, g_diff))


def _stack(x):
    return torch.stack([p.value() for p in x], -1) if isinstance(x, list) else x.value()


def values(out):
    return {key: _stack(x) for key, x in out.items()}


def bounds(out):
    """The accumulated running error of every element + the underflow floor."""
    e = lambda x: torch.stack([p.e for p in x], -1) if isinstance(x, list) else x.e
    return {key: e(x) + FLOOR for key, x in out.items()}


# ------------------------------------------------------------------------------------------------ the restatement proper: oracle + autograd
def basis_values(c, d):
    p0, p1 = c["p0"].double(), c["p1"].double()
    if c["basis"] == 1:
        return orc.bessel_basis(d, p0)
    if c["basis"] == 2:
        return orc.gaussian_rbf(d, p0, p1)
    return orc.expnorm_smearing(d, p0, p1, c["cutoff"])


def restate_forward(c):
    v, d = c["vec"].double(), c["diff"].double()
    loop = loop_mask(c)
    u = torch.where(loop[:, None], v, v / v.norm(dim=1, keepdim=True))
    return dict(rl=orc.real_harmonics(c["lmax"], u), cut=orc.cosine_cutoff(d, c["cutoff"]), phi=basis_values(c, d))


def restate_backward(c):
    """fp64 autograd of sum <G_rl, rl> + <G_phi, phi> + G_cut cut  to v (through u) and d, on the rows that are no loop."""
    E, D = c["E"], ndim(c["lmax"])
    keep = ~loop_mask(c)
    g_vec, g_diff = torch.zeros(E, 3, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    if int(keep.sum()) == 0:
        return dict(g_vec=g_vec, g_diff=g_diff)
    G_rl = c["g_rl"].double().sum(0) if c["n_rl"] else torch.zeros(E, D, dtype=torch.float64)
    G_cut = c["g_cut"].double().sum(0) if c["n_cut"] else torch.zeros(E, dtype=torch.float64)
    with torch.enable_grad():
        v = c["vec"].double()[keep].requires_grad_(True)
        d = c["diff"].double()[keep].requires_grad_(True)
        rl = orc.real_harmonics(c["lmax"], v / v.norm(dim=1, keepdim=True))
        sub = dict(c, diff=None)
        s = (G_rl[keep] * rl).sum() + (c["g_phi"].double()[keep] * basis_values(sub, d)).sum() \
            + (G_cut[keep] * orc.cosine_cutoff(d, c["cutoff"])).sum()
        gv, gd = torch.autograd.grad(s, (v, d))
    g_vec[keep], g_diff[keep] = gv, gd
    return dict(g_vec=g_vec, g_diff=g_diff)


# ------------------------------------------------------------------------------------------------ gn_pos_scatter
def csc_of(src, N):
    """colptr, perm of the by-source view: a stable sort on the CPU."""
    perm = torch.sort(src.long(), stable=True)[1]
    colptr = torch.zeros(N + 1, dtype=torch.int32)
    colptr[1:] = torch.bincount(src.long(), minlength=N).cumsum(0).to(torch.int32)
    return colptr, perm.to(torch.int32).contiguous()


def rowptr_of(dst, N):
    rp = torch.zeros(N + 1, dtype=torch.int32)
    rp[1:] = torch.bincount(dst.long(), minlength=N).cumsum(0).to(torch.int32)
    return rp


def check_graph(s):
    """What the by-target / by-source kernels index with; asserted before any launch."""
    N, E = s["N"], s["E"]
    rp, cp, perm, src, dst = (s[key].long() for key in ("rowptr", "colptr", "perm", "src", "dst"))
    for p in (rp, cp):
        assert p.numel() == N + 1 and int(p[0]) == 0 and int(p[-1]) == E and bool((p[1:] >= p[:-1]).all())
    assert perm.numel() == E and torch.equal(torch.sort(perm)[0], torch.arange(E))
    assert src.numel() == E and dst.numel() == E
    assert E == 0 or (0 <= int(src.min()) and int(src.max()) < N and 0 <= int(dst.min()) and int(dst.max()) < N)
    assert torch.equal(dst, torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1]))          # target-major
    assert torch.equal(src[perm], torch.repeat_interleave(torch.arange(N), cp[1:] - cp[:-1]))


def scatter_edge(ar, s):
    """The per-edge gv of pos_scatter_kernel's `add`: [3 x E] numbers."""
    x, y, z = (ar.load(s["vec"][:, n]) for n in range(3))
    gd = ar.load(s["g_diff"])
    q = gd / (x * x + y * y + z * z).sqrt()
    live = s["g_diff"] != 0
    return [ar.where(live, ar.load(s["g_vec"][:, n]) + q * p, ar.load(s["g_vec"][:, n])) for n, p in enumerate((x, y, z))]


def restate_scatter(s, mut=None):
    N, v = s["N"], s["vec"].double()
    gv = s["g_vec"].double().clone()
    live = s["g_diff"] != 0
    gv[live] += (s["g_diff"].double()[:, None] * v / v.norm(dim=1, keepdim=True))[live]
    out = torch.zeros(N, 3, dtype=torch.float64)
    src, dst = s["src"].long(), s["dst"].long()
    if mut == "scatter_sign":
        src, dst = dst, src
    if mut == "perm_identity":                                              # column n read through perm = identity
        cp = s["colptr"].long()
        src = torch.repeat_interleave(torch.arange(N), cp[1:] - cp[:-1])
    out.index_add_(0, src, gv)
    out.index_add_(0, dst, -gv)
    return s["sign"] * out


def bound_scatter(s):
    N = s["N"]
    r = scatter_edge(RE, s)
    mag, err = torch.stack([p.v.abs() for p in r], -1), torch.stack([p.e for p in r], -1)
    live = torch.isfinite(mag).all(1)                                        # (a zero-length row is held by the NaN test, not here)
    mag, err = torch.where(live[:, None], mag, torch.zeros(())), torch.where(live[:, None], err, torch.zeros(()))
    M, Er = torch.zeros(N, 3, dtype=torch.float64), torch.zeros(N, 3, dtype=torch.float64)
    for idx in (s["src"].long(), s["dst"].long()):
        M.index_add_(0, idx, mag)
        Er.index_add_(0, idx, err)
    deg = (torch.bincount(s["src"].long(), minlength=N) + torch.bincount(s["dst"].long(), minlength=N)).double()
    return Er + (deg[:, None] + 3) * U32 * M + FLOOR


def emulate_scatter(s):
    """pos_scatter_kernel in fp32: a lane adds its outgoing then its incoming edges, the xor butterfly 1, 2, .. 32, the sign."""
    N = s["N"]
    r = torch.stack([p.v for p in scatter_edge(F32, s)], -1).numpy()
    rp, cp, perm = s["rowptr"].tolist(), s["colptr"].tolist(), s["perm"].tolist()
    out = np.zeros((N, 3), dtype=np.float32)
    one, sign = np.float32(1.0), np.float32(s["sign"])
    for n in range(N):
        acc = np.zeros((64, 3), dtype=np.float32)
        for lane in range(64):
            for pp in range(cp[n] + lane, cp[n + 1], 64):
                acc[lane] = acc[lane] + one * r[perm[pp]]
            for e in range(rp[n] + lane, rp[n + 1], 64):
                acc[lane] = acc[lane] + (-one) * r[e]
        for off in (1, 2, 4, 8, 16, 32):
            acc = acc + acc[np.arange(64) ^ off]
        out[n] = sign * acc[0]
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------ error / bound
def ratio(got, ref, bound, mask=None):
    """max |got - ref| / bound over the (masked) elements; a non-finite element counts as a breach."""
    if got.numel() == 0:
        return 0.0
    r = (got.double() - ref.double()).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf))
    if mask is not None:
        r = r[mask.expand_as(r)] if mask.shape != r.shape else r[mask]
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ cases
def basis_params(basis, R, cutoff, hostile=False):
    """The default buffers of the three radial-basis modules; ``hostile``: trained values -- large betas, narrow widths."""
    if basis == 0:
        p0, p1 = orc.expnorm_params(cutoff, R)
        if hostile:
            p1 = p1 * 40.0 + torch.linspace(0.0, 500.0, R)
            p0 = (p0 + 0.03 * torch.sin(torch.arange(R).float())).clamp(0.0, 1.2)
    elif basis == 1:
        p0 = (torch.arange(1, R + 1) * math.pi / cutoff).float()
        if hostile:
            p0 = p0 * 1.37 + 0.11
        p1 = p0.clone()
    else:
        p0 = torch.linspace(0.0, cutoff, R)
        p1 = (torch.abs(p0[1] - p0[0]) if R > 1 else torch.tensor(0.5)) * torch.ones(R)
        if hostile:
            p1 = p1 * 0.05 + 0.01
    return p0.float().contiguous(), p1.float().contiguous()


def edge_set(E, cutoff, images, perturb, seed, N=9):
    """The special edges first (the whole set at E >= 40), random ones up to E.  -> vec [E, 3], diff [E], src, dst, tags."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    unit = lambda: torch.nn.functional.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0)
    vec, dset, tags = [], [], []
    cf = np.float32(cutoff)
    for a in range(3):                                                      # the six axis directions
        for sg in (1.0, -1.0):
            v = torch.zeros(3, dtype=torch.float64)
            v[a] = sg * (0.7 + 0.6 * a)
            vec.append(v); dset.append(None); tags.append("axis")
    for a in range(3):                                                      # 1e-4 off an axis
        for sg in (1.0, -1.0):
            v = torch.full((3,), 1e-4, dtype=torch.float64) * (1.1 + a)
            v[(a + 1) % 3] *= -0.5
            v[a] = sg * (1.3 + 0.4 * a)
            vec.append(v); dset.append(None); tags.append("near_axis")
    for L in np.linspace(0.05, float(cutoff) * 0.999, 8):                   # lengths from 0.05 to the cutoff
        vec.append(unit() * float(L)); dset.append(None); tags.append("length")
    vec.append(unit() * 0.5); dset.append(None); tags.append("half")        # d = 0.5: the Bessel note of DESIGN.md
    for dd, tag in ((cf, "at_cutoff"), (np.nextafter(cf, np.float32(0)), "below_cutoff"),
                    (np.nextafter(cf, np.float32(np.inf)), "above_cutoff"), (np.float32(1.5 * cutoff), "beyond")):
        vec.append(unit() * float(dd)); dset.append(float(dd)); tags.append(tag)
    vec.append(torch.zeros(3, dtype=torch.float64)); dset.append(0.0); tags.append("loop")
    if images:
        vec.append(unit() * 2.0); dset.append(None); tags.append("self_image")          # j == i, d > 0: a real edge
        vec.append(torch.zeros(3, dtype=torch.float64)); dset.append(0.0); tags.append("loop")
    while len(vec) < E:
        vec.append(unit() * float(0.3 + rnd(1) * (1.2 * cutoff - 0.3))); dset.append(None); tags.append("random")
    vec, dset, tags = vec[:E], dset[:E], tags[:E]
    v32 = torch.stack(vec).float() if E else torch.zeros(0, 3)
    diff = v32.norm(dim=1)                                                  # the fp32 norm of edge_vec
    if perturb:                                                             # an independent distance
        diff = diff * (1.0 + 2e-3 * (torch.rand(E, generator=g) - 0.5))
    src, dst = torch.zeros(E, dtype=torch.int32), torch.zeros(E, dtype=torch.int32)
    for e in range(E):
        if dset[e] is not None:
            diff[e] = dset[e]
        j = int(torch.randint(0, N, (1,), generator=g))
        src[e] = j
        dst[e] = j if tags[e] in ("loop", "self_image") else (j + 1 + int(torch.randint(0, N - 1, (1,), generator=g))) % N
    return v32.contiguous(), diff.float().contiguous(), src, dst, tags


def geo_case(lmax, E, R, basis, n_rl, n_cut, images=False, perturb=False, hostile=False, cutoff=5.0):
    return dict(lmax=lmax, E=E, R=R, basis=basis, n_rl=n_rl, n_cut=n_cut, images=images, perturb=perturb, hostile=hostile,
                cutoff=cutoff)


def geo_id(c):
    return (f"l{c['lmax']}-E{c['E']}-R{c['R']}-b{c['basis']}-rl{c['n_rl']}-cut{c['n_cut']}{'-img' if c['images'] else ''}"
            f"{'-pert' if c['perturb'] else ''}{'-hostile' if c['hostile'] else ''}-c{c['cutoff']}")


T_, F_ = True, False
GEO_CASES = [
    geo_case(1, 127, 20, 0, 1, 1),
    geo_case(1, 129, 20, 1, 2, 5, images=T_),
    geo_case(2, 128, 32, 0, 2, 4, perturb=T_),
    geo_case(2, 0, 20, 0, 1, 1),
    geo_case(3, 129, 7, 1, 3, 3, images=T_),
    geo_case(3, 1, 20, 0, 1, 1),
    geo_case(4, 257, 20, 2, 5, 5),
    geo_case(4, 129, 32, 2, 1, 3, images=T_, perturb=T_, cutoff=4.5),
    geo_case(5, 129, 1, 0, 0, 0, perturb=T_),
    geo_case(5, 127, 20, 2, 2, 4, hostile=T_),
    geo_case(6, 128, 32, 1, 1, 9, images=T_, perturb=T_),
    geo_case(6, 129, 20, 0, 1, 1, images=T_, hostile=T_, cutoff=4.5),
    geo_case(7, 127, 7, 2, 2, 1, hostile=T_),
    geo_case(7, 129, 32, 1, 3, 0, hostile=T_),
    geo_case(8, 257, 20, 0, 3, 4, images=T_),
    geo_case(8, 129, 7, 0, 5, 9, perturb=T_, hostile=T_),
]
for _dim, _vals in (("lmax", range(1, 9)), ("E", (0, 1, 127, 128, 129, 257)), ("R", (1, 7, 20, 32)), ("basis", (0, 1, 2)),
                    ("n_rl", (0, 1, 2, 3, 5)), ("n_cut", (0, 1, 3, 4, 5, 9))):
    assert {c[_dim] for c in GEO_CASES} == set(_vals), _dim


@functools.lru_cache(maxsize=None)
def _built(n):
    c = dict(GEO_CASES[n])
    E, R, D = c["E"], c["R"], ndim(c["lmax"])
    vec, diff, src, dst, tags = edge_set(E, c["cutoff"], c["images"], c["perturb"], seed=100 + n)
    p0, p1 = basis_params(c["basis"], R, c["cutoff"], c["hostile"])
    g = torch.Generator().manual_seed(7000 + n)
    rn = lambda *s: torch.randn(*s, generator=g).contiguous()
    c.update(vec=vec, diff=diff, src=src, dst=dst, tags=tags, p0=p0, p1=p1, id=geo_id(c),
             g_rl=rn(c["n_rl"], E, D), g_cut=rn(c["n_cut"], E), g_phi=rn(E, R))
    return c


def built(n, images=None):
    """Case n with its inputs (shared, never modified); ``images``: under the other entry point's loop rule."""
    c = _built(n)
    return c if images is None or images == c["images"] else dict(c, images=images)


@functools.lru_cache(maxsize=None)
def reference(n, images=None):
    """-> (forward restatement, backward restatement, forward bounds, backward bounds) of case n, computed once."""
    c = built(n, images)
    fr, br = restate_forward(c), restate_backward(c)
    fb, bb = bounds(k1_forward(RE, c)), bounds(k1_backward(RE, c))
    return fr, br, fb, bb


def tag_mask(c, *tags):
    return torch.tensor([t in tags for t in c["tags"]], dtype=torch.bool)


#: mutation -> the pass it changes ("fwd" | "bwd" | "scatter") and how a case rejects it ("bound" | "exact")
MUTATIONS = {
    "row_sign": "fwd", "raise_coeff": "fwd", "no_projection": "bwd", "inv_norm_sq": "bwd", "cut_pi": "bwd", "cut_le": "bwd",
    "expnorm_chain": "bwd", "bessel_second": "bwd", "cut_slice": "bwd", "rl_slice": "bwd", "loop_kept": "bwd",
    "loop_rule": "bwd", "scatter_sign": "scatter", "perm_identity": "scatter",
}


# ------------------------------------------------------------------------------------------------ scatter cases
def scatter_graph(N, seed, hub=False):
    """A target-major graph on N atoms: asymmetric, with isolated atoms (N >= 4), index self-loops, and with ``hub`` one
    atom of in-degree and out-degree 150 (parallel edges: more than two trips of the 64-lane stride)."""
    g = torch.Generator().manual_seed(seed)
    pairs = []
    live = max(1, N - 1) if N >= 4 else N                                   # the last atom of N >= 4 is isolated
    if N == 1:
        pairs = [(0, 0)] * 3
    else:
        for _ in range(4 * live):
            j = int(torch.randint(0, live, (1,), generator=g))
            i = int(torch.randint(0, live, (1,), generator=g))
            pairs.append((j, i))                                            # (i == j now and then: an index self-loop)
        pairs += [(0, 0), (1, 0), (1, 0), (1, 0)]                           # asymmetric: 1 -> 0 three times, never back
        pairs = [(j, i) for j, i in pairs if (j, i) != (0, 1)]
        if hub:
            h = live - 1
            pairs = [(j, i) for j, i in pairs if j != h and i != h]
            pairs += [((n % (live - 1)), h) for n in range(150)] + [(h, (n % (live - 1))) for n in range(150)]
    pairs.sort(key=lambda p: p[1])
    src = torch.tensor([p[0] for p in pairs], dtype=torch.int32)
    dst = torch.tensor([p[1] for p in pairs], dtype=torch.int32)
    return src, dst


@functools.lru_cache(maxsize=None)
def scatter_case(N, sign, hub=False):
    src, dst = scatter_graph(N, 40 + N, hub)
    E = src.numel()
    g = torch.Generator().manual_seed(900 + N)
    vec = (torch.randn(E, 3, generator=g) * 1.5).contiguous()
    g_vec, g_diff = torch.randn(E, 3, generator=g).contiguous(), torch.randn(E, generator=g).contiguous()
    loops = src == dst
    vec[loops] = 0.0                                                        # a zero-length vector with g_diff == 0: the term is dropped
    g_diff[loops] = 0.0
    g_vec[loops] = 0.0
    g_diff[::7] = 0.0                                                       # (and dropped on ordinary edges too)
    colptr, perm = csc_of(src, N)
    s = dict(N=N, E=E, sign=float(sign), src=src, dst=dst, rowptr=rowptr_of(dst, N), colptr=colptr, perm=perm, vec=vec,
             g_vec=g_vec, g_diff=g_diff, hub=hub, id=f"N{N}-sign{int(sign)}{'-hub' if hub else ''}")
    check_graph(s)
    return s


SCATTER_CASES = [(1, 1.0, False), (3, -1.0, False), (4, 1.0, False), (5, -1.0, True), (9, 1.0, True), (9, -1.0, False)]


# ------------------------------------------------------------------------------------------------ K2 / K3 and their backwards
INIT_F = (16, 64, 256, 512, 1024)
MAX_Z = 6


def wide(F):
    return max(1, F // 256)


def chain(deg, ns):
    return -(-deg // ns) + ns + 1


def init_graph(F, images, seed):
    """N = 8 targets with in-degrees 0, 1, ns - 1, ns, ns + 1, 70 (and two small ones), index self-loops among them; with
    ``images`` one of the self-loops of every target that has any carries d > 0 (a real edge).  Target-major."""
    ns = slots(F)
    degs = sorted({0, 1, max(ns - 1, 0), ns, ns + 1, 70})
    degs = (degs + [3, 2])[:8] if len(degs) < 8 else degs
    N = len(degs)
    g = torch.Generator().manual_seed(seed)
    src, dst = [], []
    for i, dg in enumerate(degs):
        for n in range(dg):
            j = i if (n % 5 == 1) else int(torch.randint(0, N, (1,), generator=g))
            src.append(j); dst.append(i)
    src, dst = torch.tensor(src, dtype=torch.int32), torch.tensor(dst, dtype=torch.int32)
    E = src.numel()
    diff = (0.5 + 4.0 * torch.rand(E, generator=g)).float()
    same = (src == dst).nonzero().flatten().tolist()
    for n, e in enumerate(same):
        if not (images and n % 2 == 0):
            diff[e] = 0.0
    return N, degs, src, dst, diff


@functools.lru_cache(maxsize=None)
def init_case(F, images=False, seed=0):
    N, degs, src, dst, diff = init_graph(F, images, 300 + F + seed)
    E, ldf = src.numel(), 2 * F + 4                                          # ldf > 2 F, a multiple of 4
    g = torch.Generator().manual_seed(500 + F + seed)
    rn = lambda *s: torch.randn(*s, generator=g).contiguous()
    feat = torch.full((E, ldf), math.nan)
    feat[:, :2 * F] = rn(E, 2 * F)
    colptr, perm = csc_of(src, N)
    d = dict(F=F, N=N, E=E, ldf=ldf, degs=degs, src=src, dst=dst, diff=diff, images=images, rowptr=rowptr_of(dst, N),
             colptr=colptr, perm=perm, z=torch.randint(0, MAX_Z, (N,), generator=g).to(torch.int32), feat=feat,
             cut=torch.rand(E, generator=g).contiguous(), A_na=rn(MAX_Z, F), A_nbr=rn(MAX_Z, F), h=rn(N, F),
             g_ctx=rn(N, 2 * F), g_t=rn(E, F), g_h0=rn(N, F), id=f"F{F}{'-img' if images else ''}")
    check_graph(d)
    assert set(degs) >= {0, 1, slots(F), slots(F) + 1, 70}
    return d


def restate_init(d):
    """fp64 K2, K3 and their backwards with per-element bounds.  -> (values, bounds), both dicts."""
    F, N, E = d["F"], d["N"], d["E"]
    ns, lw = slots(F), int(math.log2(min(F // 4, 64)))
    src, dst, z = d["src"].long(), d["dst"].long(), d["z"].long()
    keep = (~loop_mask(d)).double()[:, None]
    fn, fe, cut = d["feat"][:, :F].double(), d["feat"][:, F:2 * F].double(), d["cut"].double()[:, None]
    A, h = d["A_nbr"].double(), d["h"].double()
    din = torch.bincount(dst, minlength=N)
    dout = torch.bincount(src, minlength=N)
    val, bnd = {}, {}
    msg = A[z[src]] * fn * cut * keep
    val["ctx_m"] = torch.zeros(N, F, dtype=torch.float64).index_add_(0, dst, msg)
    mag = torch.zeros(N, F, dtype=torch.float64).index_add_(0, dst, msg.abs())
    ch = torch.tensor([chain(int(x), ns) for x in din], dtype=torch.float64)[:, None]
    bnd["ctx_m"] = (1 + ch) * U32 * mag + FLOOR
    val["ctx_a"] = d["A_na"].double()[z]
    hs = h[dst] + h[src]
    val["t"] = hs * fe
    bnd["t"] = 2 * U32 * (h[dst].abs() + h[src].abs()) * fe.abs() + FLOOR
    gm, gt = d["g_ctx"][:, F:].double(), d["g_t"].double()
    ga = gm[dst] * A[z[src]] * keep
    val["g_fn"] = ga * cut
    bnd["g_fn"] = 2 * U32 * val["g_fn"].abs() + FLOOR
    val["g_cut"] = (ga * fn).sum(1)
    bnd["g_cut"] = (5 + lw) * U32 * (ga * fn).abs().sum(1) + FLOOR
    val["g_fe"] = gt * hs
    bnd["g_fe"] = 2 * U32 * gt.abs() * (h[dst].abs() + h[src].abs()) + FLOOR
    prod = gt * fe
    val["g_h"] = d["g_h0"].double() + torch.zeros(N, F, dtype=torch.float64).index_add_(0, dst, prod).index_add_(0, src, prod)
    mag = d["g_h0"].double().abs() + torch.zeros(N, F, dtype=torch.float64).index_add_(0, dst, prod.abs()).index_add_(0, src, prod.abs())
    cnt = torch.tensor([-(-int(a) // ns) + -(-int(b) // ns) + ns + 2 for a, b in zip(din, dout)], dtype=torch.float64)[:, None]
    bnd["g_h"] = cnt * U32 * mag + FLOOR
    return val, bnd


def relabel_init(d, seed=1):
    """The same problem under a random permutation of the atoms, edges re-sorted target-major (stably).  -> (case, node map
    new -> old, edge map new -> old)."""
    g = torch.Generator().manual_seed(seed)
    N = d["N"]
    new_of_old = torch.randperm(N, generator=g)
    old_of_new = torch.argsort(new_of_old)
    src, dst = new_of_old[d["src"].long()], new_of_old[d["dst"].long()]
    emap = torch.sort(dst, stable=True)[1]
    out = dict(d, src=src[emap].to(torch.int32).contiguous(), dst=dst[emap].to(torch.int32).contiguous())
    for key in ("feat", "cut", "g_t", "diff"):
        out[key] = d[key][emap].contiguous()
    for key in ("z", "h", "g_ctx", "g_h0"):
        out[key] = d[key][old_of_new].contiguous()
    out["rowptr"] = rowptr_of(out["dst"], N)
    out["colptr"], out["perm"] = csc_of(out["src"], N)
    out["degs"] = torch.bincount(out["dst"].long(), minlength=N).tolist()
    check_graph(out)
    return out, old_of_new, emap
