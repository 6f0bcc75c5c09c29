"""Yardstick of the QM9 read-out kernels (csrc/gn_heads.hip: gn_geb_context, gn_geb_gate, gn_dipole_reduce, gn_ese_reduce and
their four backwards) and of the embedding gradients (csrc/gn_wgrad.hip: gn_embedding_grad, gn_embedding_grad_images).  CPU
only: fp64 restatements with autograd, the kernels' expressions spelled once over the three arithmetics of tests/norm_util.py
(``F64`` closed form, ``F32`` emulation, ``RE`` running-error bound), the case tables and the mutations.

The contracts:
    context       ctx [N, ldc] = [s (n_sin) | ||V_f||_2 over the 3 components (n_vout) | 0];  vmix [N*3, ldv] = [V | .. | W at w_off]
                  backward: g_s = g_ctx[:, :n_sin] (columns past n_sin untouched);  g_vmix[m, f] = g_ctx[n_sin + f] V[m, f] / ||V_f||,
                  exactly 0 where the norm is 0, 0 in [n_vout, w_off)
    gate          s_out[:, :n_sout] = sact(x[:, :n_sout]) (sact = -1: a copy), v_out[m, :n_vout] = x[:, n_sout + f] W[m, f]; the
                  columns past the widths are untouched
                  backward: g_x [N, ldgx] = [g_s_out sact'(s) | sum_m g_v_out[m] W[m] | 0];  g_vmix[m, w_off + f] = gate_f g_v_out[m, f],
                  0 in [w_off + n_vout, ldgv)
    dipole        d_b = sum_n (mu_n + pos_n c_n), c = scale q + shift when standardised; y = d or |d|; y_vec = sum_n mu_n; an empty
                  molecule: zeros.  backward: g_d = g_y d / |d| (exactly 0 where |d| = 0) or g_y; g_mu = g_d + g_yvec;
                  g_q = scale (g_d . pos) (scale only when standardised).  Column 0 of mu, q, g_mu, g_q is read / written.
    extent        m_n = mass[z_n] (0 outside [0, n_mass)), c_b = sum m pos / sum m (0 where sum m is not > 0), y_b = sum_n r_n^2 x_n
                  with r_n = sqrt(|pos_n - c_b|^2) squared again, as the reference writes it;  u_n = g_y[b] r_n^2
    embeddings    work[j] = sum over the out-edges e = (j -> i) of source j in ``perm`` order, self-loops skipped, of
                  fmaf(g_ctx[i, F + c], feat[e, c] cut[e], .);  dA_nbr[s] = sum_{j: z_j = s} work[j] and dA_na[s] = sum_{i: z_i = s}
                  g_ctx[i, :F] in ascending atom order; row 0 of dA_na is 0 (the padding index), row 0 of dA_nbr is not.  A self-loop:
                  src == dst, and, where edge_diff is given (_images), edge_diff == 0.  Plain stores: N = 0 writes zeros.

The bound is the running-error pass of tests/norm_util.py: u = 2^-24 per spelled operation (the library is built with
-ffp-contract=off; the one fmaf, in emb_source_kernel, rounds once) + 2^-126, sqrtf and the division correctly rounded, the sums
walked in the kernels' own order (``lane_sum``: atoms n0 + lane, + 64, .. per lane, then the wave butterfly; ``perm`` order;
ascending ``order[q]``).  No constant is fitted.  Elements the contract makes exact (the zero padding, the gradient at a zero
norm or a zero dipole, rows of absent species, row 0 of dA_na) carry the bound 0 and are compared for equality (``worst``).

A documented limit, not a case: a V column whose components are all below about 1e-23 squares to fp32 zero or subnormals
(a * a underflows), so the norm comes out 0 and the kernel returns the zero-norm gradient where fp64 has a finite one.  The
tables keep every non-zero column at ||V|| >= 2^-40.  A kinked sact is applied to a direct input, never to a computed one: its
side cannot change; the tables put the kink itself (0, +- the smallest normal) first and keep every other |x| above
MARGIN * 2^-126."""
import functools
import math

import torch

from tests.geometry_util import f32c
from tests.norm_util import F32, F64, LIBM_ULP, MARGIN, RE, REF_ACT  # noqa: F401  (re-exported for the tests)
from tests.norm_util import ACT_NAMES, KINKED, MIN_NORMAL, RELU, SILU, SSP, act, bound_of, dact, lane_sum, ratio

assert set(LIBM_ULP) >= {"expf", "log1pf"}        # the allowances silu / ssp lean on through RE
NAN = math.nan
V_FLOOR = 2.0 ** -40
_Z = lambda *s: torch.zeros(*s)


def worst(got, ref, bound):
    """max |got - ref| / bound over the elements with a bound; an element whose bound is 0 is exact: any difference is inf."""
    if ref.numel() == 0:
        return 0.0 if got.numel() == 0 else math.inf
    got, ref = got.double().reshape(ref.shape), ref.double()
    bound = bound.expand_as(ref)
    exact = bound == 0
    r = ratio(got, ref, bound, ~exact)
    if bool(exact.any()) and not torch.equal(got[exact], ref[exact]):
        return math.inf
    return r


def sqrt(ar, x):
    """sqrtf, correctly rounded as the device's is.  torch's fp32 square root on the CPU is not on every host (its vector
    path is off by an ulp on a fraction of a percent of arguments), so the emulation takes the fp64 root and rounds it: with 53
    bits >= 2 * 24 + 2 the second rounding cannot change the result."""
    return F32(x.v.double().sqrt().float()) if ar is F32 else x.sqrt()


def ld_of(width, mode):
    """A leading dimension: 0 the width itself, 1 one more, 2 rounded up to 32."""
    return width if mode == 0 else width + 1 if mode == 1 else -(-width // 32) * 32


def _poisoned(live, ld):
    """[.., w] -> [.., ld] with NaN in the columns the kernel must not read."""
    out = torch.full(live.shape[:-1] + (ld,), NAN)
    out[..., :live.shape[-1]] = live
    return out.contiguous()


# ------------------------------------------------------------------------------------------------ GatedEquivariantBlock
BLOCK_N = (0, 1, 5, 257)
BLOCK_W = ((1, 1, 1), (3, 2, 1), (64, 64, 64), (65, 33, 65), (200, 7, 96))       # (n_sin, n_sout, n_vout)
#: (N, widths, leading-dimension mode, w_off - n_vout, sact)
BLOCK_CASES = [(0, 1, 0, 0, -1), (1, 0, 0, 0, SILU), (5, 1, 1, 5, SSP), (5, 2, 2, 0, -1), (257, 3, 1, 5, RELU), (5, 3, 2, 5, SILU),
               (5, 4, 1, 0, SSP), (257, 0, 2, 5, SILU), (1, 4, 0, 5, RELU), (257, 1, 0, 0, SSP), (1, 2, 1, 5, RELU), (5, 4, 2, 5, -1)]
GV_SLACK = 3                                       # ldgv = w_off + n_vout + GV_SLACK: wider than the W half needs


def block_id(n):
    N, w, mode, extra, k = BLOCK_CASES[n]
    ns, no, nv = BLOCK_W[w]
    return f"N{N}-{ns}x{no}x{nv}-ld{mode}-w{nv + extra}-{'none' if k < 0 else ACT_NAMES[k]}"


@functools.lru_cache(maxsize=None)
def block_case(n):
    N, w, mode, extra, k = BLOCK_CASES[n]
    ns, no, nv = BLOCK_W[w]
    wo = nv + extra
    g = torch.Generator().manual_seed(7000 + n)
    rn = lambda *s: torch.randn(*s, generator=g)
    V, W = rn(N, 3, nv), rn(N, 3, nv)
    zero_col = torch.zeros(N, nv, dtype=torch.bool)
    for a in range(N):                             # exactly-zero columns and, beside them, one at 5 * 2^-40
        if a % 3 == 0:
            zero_col[a, (3 * a) % nv] = True
        if nv > 1:
            V[a, :, (3 * a + 1) % nv] = torch.tensor([3.0, -4.0, 0.0]) * V_FLOOR
    V = torch.where(zero_col[:, None, :], torch.zeros(()), V)
    vmix = torch.full((N, 3, ld_of(wo + nv, mode)), NAN)
    vmix[:, :, :nv], vmix[:, :, wo:wo + nv] = V, W
    x = rn(N, no + nv)
    if k in KINKED and x.numel() >= 3:
        x.view(-1)[:3] = torch.tensor([0.0, MIN_NORMAL, -MIN_NORMAL])
    return dict(N=N, n_sin=ns, n_sout=no, n_vout=nv, w_off=wo, sact=k, id=block_id(n), zero_col=zero_col,
                lds=ld_of(ns, mode), ldv=vmix.shape[-1], ldc=ld_of(ns + nv, mode), ldx=ld_of(no + nv, mode), ldso=ld_of(no, mode),
                ldo=ld_of(nv, mode), ldgs=ld_of(no, mode), ldgo=ld_of(nv, mode), ldgx=ld_of(no + nv, mode), ldgsin=ld_of(ns, mode),
                ldgv=wo + nv + GV_SLACK, s=_poisoned(rn(N, ns), ld_of(ns, mode)), vmix=vmix.contiguous(),
                x=_poisoned(x, ld_of(no + nv, mode)), g_s_out=_poisoned(rn(N, no), ld_of(no, mode)),
                g_v_out=_poisoned(rn(N, 3, nv), ld_of(nv, mode)), g_ctx=_poisoned(rn(N, ns + nv), ld_of(ns + nv, mode)))


def block_transcript(ar, c, mut=None):
    """geb_context_kernel, geb_gate_kernel and their backwards.  -> ctx [N, ldc], s_out [N, n_sout], v_out [N, 3 n_vout] (m-major),
    g_x [N, ldgx], g_s [N, n_sin], g_vmix [N, 3 ldgv] (m-major; the V half from the context backward, the W half from the gate's)."""
    N, ns, no, nv, wo, k = c["N"], c["n_sin"], c["n_sout"], c["n_vout"], c["w_off"], c["sact"]
    L = ar.load
    zero, one = L(_Z(())), L(torch.ones(()))
    pad = lambda w: L(torch.full((N, w), NAN if mut == "padding_unwritten" else 0.0))
    V = [L(c["vmix"][:, m, :nv]) for m in range(3)]
    W = [L(c["vmix"][:, m, wo:wo + nv]) for m in range(3)]
    Vn = W if mut == "v_from_w_half" else V
    q = Vn[0] * Vn[0] + Vn[1] * Vn[1]
    if mut != "norm_two_components":
        q = q + Vn[2] * Vn[2]
    nrm = sqrt(ar, q)
    ctx = ar.cat([L(c["s"][:, :ns]), nrm, pad(c["ldc"] - ns - nv)], 1)
    # the gate
    xs = L(c["x"][:, :no])
    gate = L(c["x"][:, :nv] if mut == "gate_column_f" else c["x"][:, no:no + nv])
    s_out = xs if k < 0 else act(ar, xs, k)
    gv = act(ar, gate, k) if (mut == "sact_on_gate" and k >= 0) else gate
    v_out = ar.cat([gv * W[m] for m in range(3)], 1)
    if mut == "mf_swapped":                        # element m n_vout + f computed from (m', f') = (e % 3, e / 3)
        e = torch.arange(3 * nv)
        v_out = gv.take(e // 3) * ar.cat(W, 1).take((e % 3) * nv + e // 3)
    # the gate's backward
    gso, G = L(c["g_s_out"][:, :no]), [L(c["g_v_out"][:, m, :nv]) for m in range(3)]
    gxs = gso if k < 0 else gso * dact(ar, act(ar, xs, k) if mut == "dact_at_activated" else xs, k)
    gxg = (G[0] * W[0] + G[1] * W[1]) + G[2] * W[2]
    g_x = ar.cat([gxs, gxg, pad(c["ldgx"] - no - nv)], 1)
    gW = [gate * G[m] for m in range(3)]
    # the context's backward
    gc = L(c["g_ctx"][:, ns:ns + nv])
    nz = nrm.gt()
    safe = ar.where(nz, nrm, one)
    if mut == "zero_over_zero":
        gV = [(gc * V[m]) / nrm for m in range(3)]
    else:
        gV = [ar.where(nz, (gc * V[m]) / safe, zero) for m in range(3)]
    g_vmix = ar.cat([t for m in range(3) for t in (gV[m], pad(wo - nv), gW[m], pad(c["ldgv"] - wo - nv))], 1)
    return dict(ctx=ctx, s_out=s_out, v_out=v_out, g_x=g_x, g_s=L(c["g_ctx"][:, :ns]), g_vmix=g_vmix)


def geb_halves(s, V, W, x_of_ctx, sact):
    """fp64 restatement of the block around whatever maps ctx to x.  -> ctx, x, s_out, v_out [N, 3, n_vout]."""
    ctx = torch.cat([s, torch.norm(V, dim=-2)], -1)
    x = x_of_ctx(ctx)
    nv = W.shape[-1]
    no = x.shape[-1] - nv
    s_out = x[:, :no] if sact is None or sact < 0 else REF_ACT[sact](x[:, :no])
    return ctx, x, s_out, x[:, no:].unsqueeze(-2) * W


def block_reference(c):
    """fp64 torch and autograd on the fp32 inputs, in the layout of ``block_transcript``; x is an input of its own (two GEMMs
    sit between the halves), so each half is differentiated against its own cotangent."""
    N, ns, no, nv, wo, k = c["N"], c["n_sin"], c["n_sout"], c["n_vout"], c["w_off"], c["sact"]
    z = lambda w: torch.zeros(N, w, dtype=torch.float64)
    with torch.enable_grad():
        s = c["s"][:, :ns].double().requires_grad_(True)
        V = c["vmix"][:, :, :nv].double().requires_grad_(True)
        W = c["vmix"][:, :, wo:wo + nv].double().requires_grad_(True)
        x = c["x"][:, :no + nv].double().requires_grad_(True)
        ctx, _, s_out, v_out = geb_halves(s, V, W, lambda _: x, k)
        g_s, g_V = torch.autograd.grad((ctx * c["g_ctx"][:, :ns + nv].double()).sum(), (s, V))
        g_x, g_W = torch.autograd.grad((s_out * c["g_s_out"][:, :no].double()).sum() + (v_out * c["g_v_out"][:, :, :nv].double()).sum(), (x, W))
    g_vmix = torch.cat([t for m in range(3) for t in (g_V[:, m], z(wo - nv), g_W[:, m], z(c["ldgv"] - wo - nv))], 1)
    return dict(ctx=torch.cat([ctx.detach(), z(c["ldc"] - ns - nv)], 1), s_out=s_out.detach(), v_out=v_out.detach().reshape(N, 3 * nv),
                g_x=torch.cat([g_x, z(c["ldgx"] - no - nv)], 1), g_s=g_s, g_vmix=g_vmix)


def block_exact(c):
    """name -> bool mask of the elements the contract makes exact (padding zeros, the zero-norm gradient)."""
    N, ns, no, nv, wo = c["N"], c["n_sin"], c["n_sout"], c["n_vout"], c["w_off"]
    ctx = torch.zeros(N, c["ldc"], dtype=torch.bool)
    ctx[:, ns + nv:] = True
    g_x = torch.zeros(N, c["ldgx"], dtype=torch.bool)
    g_x[:, no + nv:] = True
    gv = torch.zeros(N, 3, c["ldgv"], dtype=torch.bool)
    gv[:, :, nv:wo], gv[:, :, wo + nv:] = True, True
    gv[:, :, :nv] = c["zero_col"][:, None, :]
    return dict(ctx=ctx, g_x=g_x, g_vmix=gv.reshape(N, 3 * c["ldgv"]))


def _expected(ref, re, exact):
    out = {}
    for key, r in ref.items():
        b = bound_of(re[key]).expand_as(r).clone()
        if key in exact:
            b[exact[key].reshape(b.shape)] = 0.0
        out[key] = (r, b)
    return out


@functools.lru_cache(maxsize=None)
def block_expected(n):
    c = block_case(n)
    return _expected(block_reference(c), block_transcript(RE, c), block_exact(c))


# ------------------------------------------------------------------------------------------------ per-molecule reductions
MOL_A = (0, 1, 2, 63, 64, 65, 0, 128, 129, 200, 0)  # empty molecules first, in the middle and last; the strides take 1 .. 4 trips
MOL_B = (3,)
ZERO_MOL, FAR_MOL, MASSLESS_MOL = 2, 7, 4          # of MOL_A: the zero dipole | 30 A from the origin | every mass 0
SCALE = f32c(1.7)
#: (sizes, standardise, magnitude, y_vec and g_yvec present, (ldm, ldq, ldgm, ldgq), shift)
DIPOLE_CASES = [(MOL_A, 0, 0, True, (1, 3, 3, 1), 0.3), (MOL_A, 1, 0, False, (3, 1, 1, 3), 0.3), (MOL_A, 0, 1, True, (3, 3, 1, 1), 0.3),
                (MOL_A, 1, 1, False, (1, 1, 3, 3), 0.0), (MOL_B, 1, 1, True, (3, 3, 3, 3), 0.3), (MOL_A, 1, 1, True, (1, 3, 1, 3), 0.3),
                (MOL_B, 0, 0, False, (1, 1, 1, 1), 0.3)]
ESE_CASES = [MOL_A, MOL_B]
N_MASS = 10


def _mol_ptr(sizes):
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.int32)
    ptr[1:] = torch.tensor(sizes).cumsum(0).to(torch.int32)
    return ptr, torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def dipole_id(n):
    sizes, st, mag, yv, lds, shift = DIPOLE_CASES[n]
    return f"{'A' if sizes is MOL_A else 'B'}-st{st}-mag{mag}-{'yvec' if yv else 'noyvec'}-ld{''.join(map(str, lds))}-shift{shift}"


@functools.lru_cache(maxsize=None)
def dipole_case(n):
    sizes, st, mag, yv, (ldm, ldq, ldgm, ldgq), shift = DIPOLE_CASES[n]
    ptr, batch = _mol_ptr(sizes)
    N, n_mol = int(ptr[-1]), len(sizes)
    g = torch.Generator().manual_seed(8000 + n)
    rn = lambda *s: torch.randn(*s, generator=g)
    mu, q, pos = rn(N, 3), rn(N), rn(N, 3) * 2.0
    zero_mol = None
    if sizes is MOL_A:                             # mu = 0, q = 0 and shift = 0 (or, under a shift, pos = 0): d = 0 exactly
        zero_mol = ZERO_MOL
        a = slice(int(ptr[ZERO_MOL]), int(ptr[ZERO_MOL + 1]))
        mu[a], q[a] = 0.0, 0.0
        if st and shift != 0.0:
            pos[a] = 0.0
    return dict(sizes=sizes, N=N, n_mol=n_mol, mol_ptr=ptr, batch=batch, standardise=st, magnitude=mag, yvec=yv, ldm=ldm, ldq=ldq,
                ldgm=ldgm, ldgq=ldgq, scale=SCALE, shift=f32c(shift), zero_mol=zero_mol, id=dipole_id(n),
                mu=_poisoned(mu[:, :, None], ldm), q=_poisoned(q[:, None], ldq), pos=pos.contiguous(),
                g_y=rn(n_mol) if mag else rn(n_mol, 3), g_yvec=rn(n_mol, 3))


def _span(ptr, b, mut):
    n0, n1 = ptr[b], ptr[b + 1]
    if mut == "first_64_atoms":
        n1 = min(n1, n0 + 64)
    if mut == "mol_ptr_off_by_one":
        n1 = max(n0, n1 - 1)
    return slice(n0, n1)


def _mol_sums(ar, xT, ptr, mut):
    """xT [k, N] -> [n_mol, k]: each molecule's atoms summed as a wave sums them; an empty molecule: zeros."""
    k = xT.v.shape[0]
    out = []
    for b in range(len(ptr) - 1):
        sl = _span(ptr, b, mut)
        out.append(lane_sum(ar, xT.take(sl)) if sl.stop > sl.start else ar.load(_Z(k)))
    return ar.stack(out)


def dipole_transcript(ar, c, mut=None):
    """dipole_reduce_kernel and its backward.  -> y [n_mol, 3] | [n_mol], y_vec [n_mol, 3], g_mu [N, 3], g_q [N]."""
    L = ar.load
    st, mag, ptr, bidx = c["standardise"], c["magnitude"], c["mol_ptr"].tolist(), c["batch"]
    zero, one = L(_Z(())), L(torch.ones(()))
    scale, shift = L(torch.tensor(c["scale"])), L(torch.tensor(c["shift"]))
    muT, posT, q = L(c["mu"][:, :, 0].T), L(c["pos"].T), L(c["q"][:, 0])
    cq = q
    if st or mut == "scale_without_standardise":
        cq = scale * q
        if mut != "shift_dropped":
            cq = cq + shift
    d = _mol_sums(ar, muT + posT * cq, ptr, mut)
    y_vec = d if mut == "yvec_with_pos_q" else _mol_sums(ar, muT, ptr, mut)
    dk = [d.take(m) for m in range(3)]
    nrm = sqrt(ar, (dk[0] * dk[0] + dk[1] * dk[1]) + dk[2] * dk[2])
    gy = L(c["g_y"])
    if mag:
        nz = nrm.gt()
        safe = ar.where(nz, nrm, one)
        den = safe * safe if mut == "magnitude_grad_over_norm_squared" else safe
        if mut == "zero_over_zero":
            gd = (gy.col() * d) / nrm.col()
        else:
            gd = ar.where(nz[:, None], (gy.col() * d) / den.col(), zero)
    else:
        gd = gy
    g_mol = gd + L(c["g_yvec"]) if (c["yvec"] and mut != "g_mu_without_g_yvec") else gd
    gdn, pos = gd.row(bidx), L(c["pos"])
    s = (gdn.take(0) * pos.take(0) + gdn.take(1) * pos.take(1)) + gdn.take(2) * pos.take(2)
    g_q = scale * s if (st and mut != "g_q_without_scale") else s
    out = dict(y=nrm if mag else d, g_mu=g_mol.row(bidx), g_q=g_q)
    if c["yvec"]:
        out["y_vec"] = y_vec
    return out


def dipole_restatement(mu, q, pos, batch, n_mol, scale=None, shift=None, magnitude=False):
    """fp64: y [n_mol, 3] (or its norm [n_mol]) and y_vec [n_mol, 3] as the oracle's ``dipole`` ends."""
    c = q if scale is None else scale * q + shift
    seg = lambda v: torch.zeros((n_mol, 3), dtype=v.dtype).index_add_(0, batch, v)
    y = seg(mu + pos * c[:, None])
    return (torch.norm(y, dim=1) if magnitude else y), seg(mu)


def dipole_reference(c):
    with torch.enable_grad():
        mu = c["mu"][:, :, 0].double().requires_grad_(True)
        q = c["q"][:, 0].double().requires_grad_(True)
        st = c["standardise"]
        y, yv = dipole_restatement(mu, q, c["pos"].double(), c["batch"], c["n_mol"], c["scale"] if st else None,
                                   c["shift"] if st else None, bool(c["magnitude"]))
        loss = (y * c["g_y"].double()).sum() + ((yv * c["g_yvec"].double()).sum() if c["yvec"] else 0.0)
        g_mu, g_q = torch.autograd.grad(loss, (mu, q)) if c["N"] else (torch.zeros_like(mu), torch.zeros_like(q))
    out = dict(y=y.detach(), g_mu=g_mu, g_q=g_q)
    if c["yvec"]:
        out["y_vec"] = yv.detach()
    return out


def dipole_exact(c):
    """The zero-dipole molecule under ``magnitude``: g_d is exactly 0, so g_mu is g_yvec (or 0) and g_q is 0, exactly."""
    if not (c["magnitude"] and c["zero_mol"] is not None):
        return {}
    atoms = c["batch"] == c["zero_mol"]
    return dict(g_mu=atoms[:, None].expand(c["N"], 3), g_q=atoms)


@functools.lru_cache(maxsize=None)
def dipole_expected(n):
    c = dipole_case(n)
    return _expected(dipole_reference(c), dipole_transcript(RE, c), dipole_exact(c))


def dipole_margins(c):
    """A magnitude case: |d_b| / bound(|d_b|) of every molecule that is neither empty nor the zero one (from the reference and
    the bound alone)."""
    assert c["magnitude"]
    d = dipole_transcript(RE, c)["y"]
    keep = torch.tensor([s > 0 and b != c["zero_mol"] for b, s in enumerate(c["sizes"])])
    return (d.v / bound_of(d))[keep]


@functools.lru_cache(maxsize=None)
def ese_case(n):
    sizes = ESE_CASES[n]
    ptr, batch = _mol_ptr(sizes)
    N, n_mol = int(ptr[-1]), len(sizes)
    g = torch.Generator().manual_seed(9000 + n)
    rn = lambda *s: torch.randn(*s, generator=g)
    pos = rn(N, 3) * 2.0
    z = torch.randint(1, N_MASS, (N,), generator=g).to(torch.int32)
    mass = torch.rand(N_MASS, generator=g) * 30.0 + 1.0
    mass[0] = 0.0
    if sizes is MOL_A:
        pos[batch == FAR_MOL] += torch.tensor([30.0, -30.0, 30.0])
        a = torch.nonzero(batch == MASSLESS_MOL)[:, 0]
        z[a] = torch.where(a % 2 == 0, -1, N_MASS + 3).to(torch.int32)
        z[int(ptr[8]) + 5], z[int(ptr[8]) + 6], z[int(ptr[9]) + 70] = -2, N_MASS, 0        # massless atoms among massive ones
    return dict(sizes=sizes, N=N, n_mol=n_mol, mol_ptr=ptr, batch=batch, pos=pos.contiguous(), z=z, mass=mass, n_mass=N_MASS,
                x=rn(N), g_y=rn(n_mol), id="A" if sizes is MOL_A else "B")


def atom_mass(c, oob=0.0):
    z = c["z"].long()
    ok = (z >= 0) & (z < c["n_mass"])
    return torch.where(ok, c["mass"][z.clamp(0, c["n_mass"] - 1)], torch.full((), oob))


def ese_transcript(ar, c, mut=None):
    """ese_reduce_kernel and its backward.  -> y [n_mol], u [N]."""
    L = ar.load
    ptr, bidx = c["mol_ptr"].tolist(), c["batch"]
    zero, one = L(_Z(())), L(torch.ones(()))
    m = L(torch.ones(c["N"]) if mut == "unweighted_centroid" else atom_mass(c, 1.0 if mut == "out_of_range_mass_one" else 0.0))
    pos, posT = L(c["pos"]), L(c["pos"].T)
    ms = _mol_sums(ar, ar.stack([m]), ptr, mut).take(0)
    mp = _mol_sums(ar, m * posT, ptr, mut)
    has = ms.gt()
    cen = ar.where(has[:, None], mp / ar.where(has, ms, one).col(), zero)
    dl = pos - cen.row(bidx)
    r = sqrt(ar, (dl.take(0) * dl.take(0) + dl.take(1) * dl.take(1)) + dl.take(2) * dl.take(2))
    r2 = r if mut == "r_not_r_squared" else r * r
    y = _mol_sums(ar, ar.stack([r2 * L(c["x"])]), ptr, mut).take(0)
    return dict(y=y, u=L(c["g_y"]).row(bidx) * r2)


def ese_restatement(x, pos, mass, batch, n_mol):
    """fp64: the oracle's ``electronic_spatial_extent`` after its out-net, with c = 0 where a molecule has no mass (the oracle
    divides 0 by 0 there)."""
    seg = lambda v: torch.zeros((n_mol, v.shape[1]), dtype=v.dtype).index_add_(0, batch, v)
    ms = seg(mass[:, None])
    cen = torch.where(ms > 0, seg(mass[:, None] * pos) / torch.where(ms > 0, ms, torch.ones_like(ms)), torch.zeros_like(ms))
    return seg(torch.norm(pos - cen[batch], dim=1, keepdim=True) ** 2 * x[:, None])[:, 0]


def ese_reference(c):
    with torch.enable_grad():
        x = c["x"].double().requires_grad_(True)
        y = ese_restatement(x, c["pos"].double(), atom_mass(c).double(), c["batch"], c["n_mol"])
        (u,) = torch.autograd.grad((y * c["g_y"].double()).sum(), x)
    return dict(y=y.detach(), u=u)


@functools.lru_cache(maxsize=None)
def ese_expected(n):
    c = ese_case(n)
    return _expected(ese_reference(c), ese_transcript(RE, c), {})


# ------------------------------------------------------------------------------------------------ embedding gradients
EMB_F = (1, 48, 65, 256)
EMB_SPECIES = (1, 5, 100)
HUB_DEGREE = 300
#: (graph, F, ldf - 2 F, n_species, with edge_diff (the _images entry point))
EMB_CASES = [("hub", 48, 0, 5, False), ("hub", 65, 3, 100, True), ("hub", 256, 0, 1, False), ("small", 1, 3, 5, True),
             ("small", 256, 3, 100, False), ("empty", 48, 0, 5, False), ("empty", 1, 3, 1, True), ("one", 65, 0, 1, True),
             ("small", 48, 3, 1, False), ("hub", 1, 3, 5, True)]


def emb_id(n):
    gname, F, extra, nsp, img = EMB_CASES[n]
    return f"{gname}-F{F}-ldf{2 * F + extra}-sp{nsp}{'-images' if img else ''}"


def _graph(name, g):
    """-> N, src, dst, edge_diff (0 on the self-loops; > 0 on the self-PAIRS, an atom and its own periodic image)."""
    ri = lambda lo, hi, n: torch.randint(lo, hi, (n,), generator=g)
    if name == "empty":
        e = torch.zeros(0, dtype=torch.long)
        return 0, e, e, torch.zeros(0)
    if name == "one":
        return 1, torch.zeros(3, dtype=torch.long), torch.zeros(3, dtype=torch.long), torch.tensor([0.0, 2.5, 3.5])
    if name == "small":                            # atom 5: in-edges only; atom 6: nothing but a self-pair
        src = torch.tensor([0, 1, 2, 3, 4, 0, 0, 1, 3, 4, 2, 2, 6, 1, 1])
        dst = torch.tensor([0, 1, 2, 3, 4, 1, 5, 0, 5, 2, 4, 3, 6, 1, 2])
        diff = torch.rand(src.numel(), generator=g) * 3.0 + 0.5
        diff[:5] = 0.0                              # edges 12 and 13 stay self-pairs at a distance
        return 7, src, dst, diff
    N = 310                                        # hub: atom 0 has 300 out-edges; atoms 301 .. 309 have none; no loop on 200 ..
    loops = torch.arange(200)
    pairs = torch.arange(5, 26)
    rs, rd = ri(1, 151, 400), ri(0, 310, 400)
    src = torch.cat([torch.zeros(HUB_DEGREE, dtype=torch.long), loops, pairs, rs])
    dst = torch.cat([torch.arange(1, HUB_DEGREE + 1), loops, pairs, rd])
    diff = torch.rand(src.numel(), generator=g) * 3.0 + 0.5
    diff[HUB_DEGREE:HUB_DEGREE + 200] = 0.0
    diff[(src == dst) & (torch.arange(src.numel()) >= HUB_DEGREE + 221)] = 0.0               # a random edge that fell on j -> j
    return N, src, dst, diff


@functools.lru_cache(maxsize=None)
def emb_case(n):
    gname, F, extra, nsp, img = EMB_CASES[n]
    g = torch.Generator().manual_seed(10000 + n)
    N, src, dst, diff = _graph(gname, g)
    key = dst * max(N, 1) + src                    # the engine's edge order: by target, sources ascending (stable)
    o = torch.sort(key, stable=True)[1]
    src, dst, diff = src[o], dst[o], diff[o]
    E = src.numel()
    perm = torch.sort(src, stable=True)[1]
    colptr = torch.zeros(N + 1, dtype=torch.long)
    colptr[1:] = torch.bincount(src, minlength=N).cumsum(0)
    # species: 0 present, some absent (5: never 3; 100: most), one species for everything at n_species = 1
    z = torch.randint(0, nsp, (N,), generator=g)
    z = torch.where(z == 3, torch.full_like(z, 4 if nsp > 4 else 0), z)
    if N:
        z[N - 1], z[0] = min(1, nsp - 1), 0         # atom 0 (the hub; a source with kept edges) is of species 0
    zs, order = torch.sort(z, stable=True)
    sp_ptr = torch.searchsorted(zs, torch.arange(nsp + 1))
    rn = lambda *s: torch.randn(*s, generator=g)
    i32 = lambda t: t.to(torch.int32).contiguous()
    return dict(graph=gname, N=N, E=E, F=F, ldf=2 * F + extra, n_species=nsp, images=img, id=emb_id(n), src=src, dst=i32(dst), z=z,
                colptr=i32(colptr), perm=i32(perm), order=i32(order), sp_ptr=i32(sp_ptr), edge_diff=diff.contiguous(),
                g_ctx=rn(N, 2 * F).contiguous(), feat=_poisoned(rn(E, F), 2 * F + extra), cut=torch.rand(E, generator=g).contiguous())


def emb_loop(c, mut=None):
    """[E] bool: the edges the source kernel skips."""
    same = c["src"] == c["dst"].long()
    if mut == "self_loop_kept":
        return torch.zeros_like(same)
    if c["images"] and mut != "images_every_self_pair_skipped":
        return same & (c["edge_diff"] == 0)
    return same


def _ordered_sum(ar, X, start, count, index):
    """out[r] = X[index[start[r]]] + X[index[start[r] + 1]] + ..: ``count[r]`` rows of X, serially (0.f + x is exact)."""
    acc = ar.load(_Z(count.numel(), X.v.shape[1]))
    for t in range(int(count.max()) if count.numel() else 0):
        row = index[(start + t).clamp(max=index.numel() - 1)]
        live = (count > t)[:, None]
        acc = ar.where(live, X.row(row) if t == 0 else acc + X.row(row), acc)
    return acc


def emb_transcript(ar, c, mut=None):
    """emb_source_kernel, then emb_species_kernel twice.  -> work [N, F], dA_na, dA_nbr [n_species, F]."""
    N, E, F, nsp = c["N"], c["E"], c["F"], c["n_species"]
    L = ar.load
    zero = L(_Z(()))
    gc = L(c["g_ctx"])
    dst, perm, colptr = c["dst"].long(), c["perm"].long(), c["colptr"].long()
    P = L(_Z(N, F))
    if E:
        w = L(c["feat"][:, :F])
        if mut != "cut_dropped":
            w = w * L(c["cut"]).col()
        G = gc.take(slice(0, F) if mut == "g_ctx_column_c" else slice(F, 2 * F))
        loop, deg = emb_loop(c, mut), colptr[1:] - colptr[:-1]
        for t in range(int(deg.max())):
            qi = (colptr[:-1] + t).clamp(max=E - 1)
            e = qi if mut == "perm_ignored" else perm[qi]
            live = ((deg > t) & ~loop[e])[:, None]
            P = ar.where(live, G.row(dst[e]).fma(w.row(e), P), P)
    sp_ptr, order = c["sp_ptr"].long(), c["order"].long()
    cnt = sp_ptr[1:] - sp_ptr[:-1]
    row0 = (torch.arange(nsp) == 0)[:, None]
    na = _ordered_sum(ar, gc.take(slice(0, F)), sp_ptr[:-1], cnt, order)
    nbr = _ordered_sum(ar, P, sp_ptr[:-1], cnt, order)
    if mut != "a_na_row0_kept":
        na = ar.where(row0, zero, na)
    if mut == "a_nbr_row0_zeroed":
        nbr = ar.where(row0, zero, nbr)
    return dict(work=P, dA_na=na, dA_nbr=nbr)


def emb_restatement(g_ctx, feat, cut, src, dst, z, n_species, loop):
    """fp64, by autograd: ctx = [A_na[z] | m], m[i] = sum over the edges (j -> i) that are no self-loop of A_nbr[z_j] feat_e cut_e
    (``node_init`` of the oracle), L = sum g_ctx ctx.  -> work (dL/d of the gathered A_nbr rows), dL/dA_na (row 0 zeroed: A_na is
    an Embedding with padding_idx = 0, a rule the oracle's plain indexing does not know), dL/dA_nbr."""
    N, F = g_ctx.shape[0], g_ctx.shape[1] // 2
    with torch.enable_grad():
        A_na = torch.zeros(n_species, F, dtype=torch.float64, requires_grad=True)
        A_nbr = torch.zeros(n_species, F, dtype=torch.float64, requires_grad=True)
        h_src = A_nbr[z]
        keep = ~loop
        m = torch.zeros(N, F, dtype=torch.float64).index_add_(0, dst[keep], h_src[src[keep]] * feat[keep] * cut[keep, None])
        loss = (g_ctx * torch.cat([A_na[z], m], 1)).sum()
        got = torch.autograd.grad(loss, (h_src, A_na, A_nbr), allow_unused=True)      # (no kept edge: the A_nbr side is unused)
    work, d_na, d_nbr = (torch.zeros_like(t) if g is None else g for g, t in zip(got, (h_src, A_na, A_nbr)))
    d_na = d_na.clone()
    d_na[0] = 0.0
    return dict(work=work, dA_na=d_na, dA_nbr=d_nbr)


def emb_reference(c):
    F = c["F"]
    return emb_restatement(c["g_ctx"].double(), c["feat"][:, :F].double(), c["cut"].double(), c["src"], c["dst"].long(), c["z"],
                           c["n_species"], emb_loop(c))


def emb_exact(c):
    """Exact zeros: sources with no kept out-edge, species without atoms, row 0 of dA_na."""
    F, nsp = c["F"], c["n_species"]
    kept = torch.bincount(c["src"][~emb_loop(c)], minlength=c["N"]) > 0
    absent = torch.bincount(c["z"], minlength=nsp) == 0
    na = absent.clone()
    na[0] = True
    return dict(work=(~kept)[:, None].expand(c["N"], F), dA_na=na[:, None].expand(nsp, F), dA_nbr=absent[:, None].expand(nsp, F))


@functools.lru_cache(maxsize=None)
def emb_expected(n):
    c = emb_case(n)
    return _expected(emb_reference(c), emb_transcript(RE, c), emb_exact(c))


#: mutation -> family.  Each is a one-line change of the spelled kernel; at least one case of its family must reject it.
MUTATIONS = {
    "norm_two_components": "block", "v_from_w_half": "block", "gate_column_f": "block", "mf_swapped": "block", "sact_on_gate": "block",
    "dact_at_activated": "block", "padding_unwritten": "block", "zero_over_zero": "block+dipole",
    "first_64_atoms": "dipole+ese", "mol_ptr_off_by_one": "dipole+ese", "yvec_with_pos_q": "dipole", "shift_dropped": "dipole",
    "scale_without_standardise": "dipole", "g_q_without_scale": "dipole", "g_mu_without_g_yvec": "dipole",
    "magnitude_grad_over_norm_squared": "dipole",
    "unweighted_centroid": "ese", "r_not_r_squared": "ese", "out_of_range_mass_one": "ese",
    "self_loop_kept": "emb", "images_every_self_pair_skipped": "emb", "cut_dropped": "emb", "g_ctx_column_c": "emb",
    "perm_ignored": "emb", "a_nbr_row0_zeroed": "emb", "a_na_row0_kept": "emb",
}
FAMILY = dict(block=(BLOCK_CASES, block_case, block_expected, block_transcript),
              dipole=(DIPOLE_CASES, dipole_case, dipole_expected, dipole_transcript),
              ese=(ESE_CASES, ese_case, ese_expected, ese_transcript), emb=(EMB_CASES, emb_case, emb_expected, emb_transcript))


def ratios(got, ex):
    """{output: worst(got, reference, bound)} over the outputs of one case; ``got`` holds numbers of an arithmetic or tensors."""
    return {k: worst(got[k].v if hasattr(got[k], "v") else got[k], *ex[k]) for k in ex}
