"""Launch sequencer for the HIP hot path (forward, and the force backward).

Takes raw device tensors + packed weights and issues the C-ABI calls of
include/gotennet_hip.h on the current PyTorch-ROCm stream.  PyTorch is plumbing
here (device memory from the caching allocator, the stream, integer index
sorting for the CSC view); all floating-point arithmetic is in
libgotennet_hip.so.  Nothing in ``forward``/``backward`` synchronises with the
host, so a step can be captured in a hipGraph (torch.cuda.CUDAGraph).

Call order = the reference's op order in GotenNet.forward (gotennet.py:956-1010),
GATA.forward (366-450) and EQFF.forward (716-748); ``backward`` walks it in
reverse (what torch.autograd.grad does for the reference at outputs.py:365-375).
The backward's copies of activations are PRE-activation (SiLU' needs them); the forward applies SiLU once, in the
producing GEMM's epilogue.  Independent projections are issued as grouped launches (gn_gemm_group).
"""
from __future__ import annotations

import dataclasses
import os
from dataclasses import dataclass, field
from typing import Any, List, Optional

import torch

from . import _lib
from ._lib import call, ptr


@dataclass
class LayerWeights:
    Wn1: Optional[torch.Tensor] = None; bn1: Optional[torch.Tensor] = None   # [W_q; W_k; gamma_s.0; gamma_v.0]  [4F, F]
    Ws2: Optional[torch.Tensor] = None; bs2: Optional[torch.Tensor] = None   # gamma_s.1 [MF, F]
    Wv2: Optional[torch.Tensor] = None; bv2: Optional[torch.Tensor] = None   # gamma_v.1 [MF, F]
    We: Optional[torch.Tensor] = None; be: Optional[torch.Tensor] = None     # [W_re; W_rs] [(1+M)F, F]
    Wvu: Optional[torch.Tensor] = None              # EQFF (None in a stand-alone GATA pack, whose GATA operands above are None)
    Wm0: Optional[torch.Tensor] = None; bm0: Optional[torch.Tensor] = None
    Wm1: Optional[torch.Tensor] = None; bm1: Optional[torch.Tensor] = None
    Wt: Optional[torch.Tensor] = None; bt: Optional[torch.Tensor] = None   # gamma_t
    Wvq: Optional[torch.Tensor] = None
    Wvk: List[torch.Tensor] = field(default_factory=list)   # one per degree, or ONE shared weight (sep_htr=False)
    ln_w: Optional[torch.Tensor] = None; ln_b: Optional[torch.Tensor] = None   # optional nn.LayerNorm on h
    tln_w: Optional[torch.Tensor] = None                                       # optional TensorLayerNorm weight
    # composed edge update (edge_updates "mlp"/"mlpa"/"linw"/"linwa"/"ln"/"postln", gotennet.py:236-291)
    Wt0: Optional[torch.Tensor] = None; bt0: Optional[torch.Tensor] = None     # gamma_t hidden layer
    t_ln_w: Optional[torch.Tensor] = None; t_ln_b: Optional[torch.Tensor] = None   # its LayerNorm (edge_ln)
    Wedp: Optional[torch.Tensor] = None; bedp: Optional[torch.Tensor] = None   # W_edp
    w_ln_w: Optional[torch.Tensor] = None; w_ln_b: Optional[torch.Tensor] = None   # LayerNorm before / after W_edp
    T: dict = field(default_factory=dict)         # derived operands (``derived``): prefix views, transposes, concatenations


@dataclass
class PackedWeights:
    A_na: torch.Tensor; A_nbr: torch.Tensor
    Winit: torch.Tensor; binit: torch.Tensor      # [W_ndp; W_erp] [2F, R]
    Wa: torch.Tensor; ba: torch.Tensor; ln_w: torch.Tensor; ln_b: torch.Tensor
    Wb: torch.Tensor; bb: torch.Tensor
    rb0: torch.Tensor; rb1: torch.Tensor          # radial-basis parameter vectors (means/betas, freqs, offsets/widths)
    layers: List[LayerWeights] = field(default_factory=list)
    T: dict = field(default_factory=dict)         # derived operands (``derived``)
    emb_idx: Optional[torch.Tensor] = None        # model embedded in a power-of-two width (embed.py): real channel f sits at emb_idx[f]
    F_model: int = 0                              # ... and its real width (0: not embedded)


#: A/B and test switch: False runs the first interaction through the general kernels on the zero tensor
ZERO_X_FIRST = os.environ.get("GN_ZERO_X_FIRST", "1") != "0"
#: test switch: True withholds the head-sum workspace from gn_message_backward where the entry point allows it (monolithic
#: launches and every first interaction), which then runs the by-target / by-source kernel pair instead of the merged kernel
MSG_BWD_PAIR = False
#: A/B and test switch: False forms dL/dt of a layer with a plain edge update in two edge-sized launches (gt_a = gt + g_pre_t Wt^T
#: in ``_eqff_htr_backward``, then gt_b = gt_a + g_eproj We^T) instead of the one K-concatenated launch of ``_gata_backward``
DT_KCAT = True


def zero_X_in(cfg: "Config", li: int) -> bool:
    """Layer ``li`` of ``forward`` sees the all-zero X that forward itself creates (gotennet.py:992) and the kernels have
    the zero-X_in form (register-tiled SiLU kernels, lmax <= 4): every tensor-gate term of that layer is 0 * gate, so its
    blocks of the edge projection are neither computed nor read, and nothing consumes the gradient w.r.t. X_in."""
    return (ZERO_X_FIRST and li == 0 and cfg.lmax <= 4 and cfg.act == 0 and not cfg.steerable_norm and not cfg.sliced
            and cfg.aggr == 0 and not cfg.wide)


def derived(holder, key, build):
    """The operand ``key`` derived from the weights of ``holder`` (a LayerWeights or PackedWeights), kept in ``holder.T``: ONE
    object per pack (``split_weight`` caches the planes ON the tensor object), made by ``build()`` inside the call that first
    needs it (pipeline.InFlight fences only the first call of a kind per pack), never ahead of it (inference pays for no transposes)."""
    t = holder.T.get(key)
    if t is None:
        t = holder.T[key] = build()
    return t


def _T(holder, name: str, lo: int = 0, hi: Optional[int] = None) -> torch.Tensor:
    """Transposed copy of the operand ``name`` -- of its rows [lo, hi) -- ([in, out] -> the GEMM's [out', in'] layout for
    input-gradients).  (Fifty look-ups per one-molecule step: the hit does not go through ``derived``.)"""
    key = name if hi is None else (name, lo, hi)
    t = holder.T.get(key)
    return t if t is not None else derived(holder, key, lambda: getattr(holder, name)[lo:hi].t().contiguous())


def _rows(lw, name: str, n: int) -> torch.Tensor:
    """The first ``n`` rows of the operand ``name`` (a view): what a zero-X_in layer uses of [W_re; W_rs], gamma_s.1 and
    gamma_v.1 -- a prefix without the tensor-gate blocks (``_Call.cols``)."""
    return derived(lw, ("rows", name, n), lambda: getattr(lw, name)[:n])


@dataclass
class Config:
    F: int; L: int; R: int; H: int; lmax: int; M: int
    cutoff: float; eps: float
    scale_edge: bool; sep_dir: bool; sep_tensor: bool
    basis: int = 0            # gn_edge_geometry basis code: 0 expnorm, 1 Bessel, 2 Gaussian
    htr_mode: int = 0         # GN_HTR_* bits (sep_htr=False, "norej", gamma_w gate)
    layernorm: bool = False   # nn.LayerNorm on h at the GATA input (gotennet.py:397)
    steerable_norm: bool = False   # TensorLayerNorm on X at the GATA input (gotennet.py:398)
    composed_update: bool = False  # gamma_t 2-layer MLP and/or W_edp in gamma_w: sequenced by _edge_update_composed
    gate_kind: int = 0        # gamma_w's final element-wise gate: 0 none, 1 sigmoid, 2 tanh, 3 SiLU
    t_last_act: int = 3       # gamma_t's last layer: 3 = activated (with ``act``), 0 = linear ("mlp")
    lin_w: int = 0            # 0 no W_edp, 1 "linw", 2 "linwa" (SiLU before W_edp)
    lin_ln: int = 0           # 0 none, 1 "ln" (LayerNorm before W_edp), 2 "postln" (inside the W_edp Dense)
    act: int = 0              # GN_ACT_* kind of the ``activation`` argument (0 = SiLU / swish, the reference default)
    evec: int = 0             # evec_dim: width of EQ / EK / w (0 = F; != F needs W_edp to map back to F)
    emlp: int = 0             # emlp_dim: hidden width of the 2-layer gamma_t (0 = F)
    gemm_mode: str = ""       # projection arithmetic of THIS model ("f16x2" | "split" | "f32"; "" = engine.GEMM_MODE, the default)
    wgrad_mode: str = ""      # weight-gradient arithmetic of THIS model ("f32" | "f16x2"; "" = engine.WGRAD_MODE, the default)
    sliced: bool = False      # run lmax <= 4 on the degree-sliced kernel family too (GN_LMAX_SLICED in the lmax argument)
    aggr: int = 0             # the reference's `aggr` (gotennet.py:84,638): 0 "add", 1 "mean", 2 "max"
    Fc: int = 0               # width of the NodeInit LayerNorm intermediate when the model is embedded in a power-of-two F (embed.py; 0 = F)
    F_model: int = 0          # the model's real n_atom_basis when embedded (0 = F)
    fuse_eqff: Optional[bool] = None   # the node-local EQFF chain as ONE kernel each way where covered (eqff_fused_ok).  None =
                              # auto: on for systems of at most EQFF_FUSED_MAX_ATOMS atoms (launch-bound: -17 % on a one-molecule
                              # step, -2 % at 32 molecules), off above (a wash at the 128-molecule batch)
    attn_p: float = 0.0       # attention-dropout probability of THIS call (gotennet.py:513): > 0 only in the configuration a
                              # training-mode forward builds for itself (``GotenNet._dropout_call``); the module's own
                              # ``config()`` -- what the inference tools take -- always says 0

    @property
    def Fe(self) -> int:
        return self.evec or self.F

    @property
    def Fm(self) -> int:
        return self.emlp or self.F

    @property
    def D(self) -> int:
        return (self.lmax + 1) ** 2 - 1

    def degree_blocks(self, N: int, explicit: bool = False):
        """The row blocks of an [N, D, F] tensor that the weights ``lw.Wvk`` act on: -> [(index into Wvk, rows, rowmap)],
        rowmap = (cnt, D, off): one per degree l (cnt = 2l + 1 rows per atom from row off), or with ONE shared weight
        (sep_htr=False: ``htr_mode & 1``) every row -- the identity, which ``explicit`` writes (D, D, 0) as the X-products
        backward always has and else is the default (1, 1, 0): equivalent, historical, kept so no descriptor changes."""
        D = self.D
        if self.htr_mode & 1:
            return [(0, N * D, (D, D, 0) if explicit else (1, 1, 0))]
        blocks, off = [], 0
        for l in range(1, self.lmax + 1):
            blocks.append((l - 1, N * (2 * l + 1), (2 * l + 1, D, off)))
            off += 2 * l + 1
        return blocks

    @property
    def lmax_arg(self) -> int:
        """The ``lmax`` argument of the message / HTR entry points: GN_LMAX_SLICED rides in it."""
        return self.lmax | (_lib.LMAX_SLICED if self.sliced else 0)

    @property
    def wide(self) -> bool:
        """A slot (one edge row, F / 4 lanes) spans several waves: the input-gradient kernels are the degree-sliced family
        and the per-edge scalar gradients come as F / 256 partial slices per call."""
        return self.F > 256 or self.Fe > 256

    @property
    def lmax_arg_bwd(self) -> int:
        """... of the BACKWARD entry points: F > 256 runs the degree-sliced kernels there."""
        return self.lmax_arg | (_lib.LMAX_SLICED if self.wide else 0)

    @property
    def lmax_arg_msg_bwd(self) -> int:
        return self.lmax_arg_msg | (_lib.LMAX_SLICED if self.wide else 0)

    @property
    def lmax_arg_msg(self) -> int:
        """... of the two MESSAGE entry points, which also carry the aggregation (GN_LMAX_MEAN / GN_LMAX_MAX)."""
        return self.lmax_arg | {0: 0, 1: _lib.LMAX_MEAN, 2: _lib.LMAX_MAX}[self.aggr]


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """The current stream's handle.  (``torch.cuda.current_stream().cuda_stream`` builds a Stream object per call: 4 us, a
    hundred times per step -- a fifth of the host time of a one-molecule eager step.)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


#: DEFAULT projection arithmetic of a model that does not choose one (``GotenNet.gemm_mode = None``; env GN_GEMM_MODE
#: sets the default at import; every GPU parity test runs in all three).  The arithmetic and the activation kind of a
#: call are carried by ``Config`` (``cfg.gemm_mode``, ``cfg.act``) and bound per call by ``_Call`` -- there is no
#: per-call module state, so two models with different arithmetics can run from two threads.
#:   "f16x2" (default) -- every fp32 operand as two fp16 planes scaled by block exponents (A: per staging wave and
#:       32-column K-slab = 16 or 32 neighbouring rows of the workgroup tile, running maximum, accumulators rescaled when
#:       it grows; W: per tensor), THREE fp16 MFMAs per product, fp32 accumulate: <= 3e-7 of the output's max-norm vs an
#:       fp64 product.  Results depend on which rows share a group at the 1e-7 level (a molecule's energy moves by ~1e-6
#:       relative when its position in the batch, or the batch size, changes); identical inputs give identical bits.
#:   "split" -- three bf16 planes, six bf16 MFMAs per product: same error class, row-wise arithmetic independent of the
#:       batch layout (bit-exact batch independence), 14 % slower on the C2 step.
#:   "f32"   -- exact fp32 MFMA (v_mfma_f32_32x32x2_f32, bitwise an fmaf chain), 40 % slower.
GEMM_MODE = os.environ.get("GN_GEMM_MODE", "f16x2")
MODES = ("f16x2", "split", "f32")


#: projection arithmetic -> (single-product entry point, grouped entry point, weight packer, its size query, dtype)
_PLANE_MODES = {"split": ("gn_gemm_split", "gn_gemm_group_split", "gn_split_bf16x3", "gn_split_bf16x3_size", torch.bfloat16),
                "f16x2": ("gn_gemm_f16x2", "gn_gemm_group_f16x2", "gn_split_f16x2", "gn_split_f16x2_size", torch.float16)}


def resolve_mode(mode: Optional[str]) -> str:
    mode = mode or GEMM_MODE
    if mode not in MODES:
        raise ValueError(f"projection arithmetic {mode!r}: one of {MODES}")
    return mode


#: DEFAULT arithmetic of the weight gradients dW = dY^T A (``weight_grad_group``) of a module that does not choose one
#: (``wgrad_mode = None`` on GotenNet and the output heads; env GN_WGRAD_MODE sets the default at import).
#:   "f32" (default) -- exact fp32 MFMA (v_mfma_f32_32x32x2_f32), gn_weight_grad_group.
#:   "f16x2" -- both operands as two fp16 planes scaled by block exponents (one per 32-column block and side, running
#:       maximum along the rows), three fp16 MFMAs per product, fp32 accumulate (gn_weight_grad_group_mode, DESIGN
#:       section 7).  Opt-in; identical inputs give identical bits.
WGRAD_MODE = os.environ.get("GN_WGRAD_MODE", "f32")
WGRAD_MODES = ("f32", "f16x2")
_WGRAD_CODE = {"f32": _lib.WGRAD_F32, "f16x2": _lib.WGRAD_F16X2}


def resolve_wgrad_mode(mode: Optional[str]) -> str:
    mode = mode or WGRAD_MODE
    if mode not in WGRAD_MODES:
        raise ValueError(f"weight-gradient arithmetic {mode!r}: one of {WGRAD_MODES}")
    return mode


def split_weight(W: torch.Tensor, mode: Optional[str] = None) -> torch.Tensor:
    """Operand planes of a weight [N, K] for the arithmetic ``mode`` in MFMA-fragment-major order (gn_split_bf16x3: bf16
    hi/mid/lo; gn_split_f16x2: header + fp16 hi/lo), cached ON the tensor object per mode (the packed weights are
    long-lived; GotenNet.invalidate_packed() drops them with the pack)."""
    mode = resolve_mode(mode)
    key = "_gn_split_" + mode
    cached = getattr(W, key, None)
    if cached is not None and cached[0] == W._version and cached[1] == W.data_ptr():
        return cached[2]
    _, _, packer, sizer, dt = _PLANE_MODES[mode]
    N, K = W.shape
    planes = torch.empty(getattr(_lib.load(), sizer)(N, K), dtype=dt, device=W.device)
    call(packer, ptr(W.contiguous()), N, K, ptr(planes), _stream())
    setattr(W, key, (W._version, W.data_ptr(), planes))
    return planes


def gemm(A, lda, W, bias, C, ldc, rows, nout, K, act=(0, 0), rowmap=(1, 1, 0), res=None, gate=None,
         a_off=0, c_off=0, pre_out=None, pro=(0, 0, 0), a_pre=None, ldp=0, p_off=0, a_gate=None, ldg=0,
         dgate=None, g_off=0, kind=None, mode=None):
    """C = epi(pro(A) W^T + bias); ``kind``: GN_ACT_* of the activated columns / SiLU' gates / prologues (None = SiLU);
    ``mode``: projection arithmetic (None = the module default).  ``a_off`` / ``c_off`` / ``p_off`` / ``g_off``: float
    offsets of the first column.  ``dgate``: multiply the output by SiLU'(dgate) (same addressing as C)."""
    mode = resolve_mode(mode)
    name = "gn_gemm_ex"
    if mode in _PLANE_MODES:
        name, W = _PLANE_MODES[mode][0], split_weight(W, mode)
    call(name, A.data_ptr() + 4 * a_off, lda, ptr(W), ptr(bias), C.data_ptr() + 4 * c_off, ldc,
         rows, nout, K, act[0], act[1], rowmap[0], rowmap[1], rowmap[2], ptr(res),
         (dgate.data_ptr() + 4 * g_off) if dgate is not None else ptr(gate), 1 if dgate is not None else 0, ptr(pre_out),
         pro[0], pro[1], pro[2], (a_pre.data_ptr() + 4 * p_off) if a_pre is not None else None, ldp,
         ptr(a_gate), ldg, 0 if kind is None else kind, _stream())


def gemm_group(problems, mode=None, kind=None, form=0):
    """Several INDEPENDENT ``gemm(...)`` calls (a list of argument dicts) as ONE launch (gn_gemm_group, or
    gn_gemm_group_split / _f16x2 with the weights replaced by their cached planes).  ``form``: a GN_GEMM_FORM_* tile of the
    f16x2 slab kernel in place of the routed kernel (gn_gemm_group_f16x2_form: probes and tests)."""
    mode = resolve_mode(mode)
    if form and mode != "f16x2":
        raise ValueError("a named slab-kernel form is an f16x2 launch")
    kind = 0 if kind is None else kind
    problems = [q for q in problems if q is not None]
    split = mode in _PLANE_MODES
    for i0 in range(0, len(problems), 4):
        chunk = problems[i0:i0 + 4]
        arr = (_lib.GemmDesc * len(chunk))()
        for d, q in zip(arr, chunk):
            g = q.get                                # (a lambda around it was 39 Python calls per problem, 41 groups per step)
            act, rowmap, pro = g("act", (0, 0)), g("rowmap", (1, 1, 0)), g("pro", (0, 0, 0))
            dgate = g("dgate")
            d.A = q["A"].data_ptr() + 4 * g("a_off", 0); d.lda = q["lda"]
            d.W = ptr(split_weight(q["W"], mode) if split else q["W"]); d.bias = ptr(g("bias"))
            d.C = q["C"].data_ptr() + 4 * g("c_off", 0); d.ldc = q["ldc"]
            d.M, d.N, d.K = q["rows"], q["nout"], q["K"]
            d.act_lo, d.act_hi = act
            d.row_cnt, d.row_gstride, d.row_goff = rowmap
            d.res = ptr(g("res"))
            d.gate = (dgate.data_ptr() + 4 * g("g_off", 0)) if dgate is not None else ptr(g("gate"))
            d.gate_mode = 1 if dgate is not None else 0
            d.pre_out = ptr(g("pre_out"))
            d.pro_mode, d.pro_lo, d.pro_hi = pro
            a_pre = g("a_pre")
            d.a_pre = (a_pre.data_ptr() + 4 * g("p_off", 0)) if a_pre is not None else None
            d.ldp = g("ldp", 0)
            d.a_gate = ptr(g("a_gate")); d.ldg = g("ldg", 0)
            d.A2, d.A3, d.a_seg = ptr(g("A2")), ptr(g("A3")), g("a_seg", 0)
            d.act_kind = g("kind", kind)
            d.lda2 = g("lda2", 0)
        if form:
            call("gn_gemm_group_f16x2_form", arr, len(chunk), form, _stream())
            continue
        call(_PLANE_MODES[mode][1] if split else "gn_gemm_group", arr, len(chunk), _stream())


class _Call:
    """What ONE forward / backward / stand-alone layer call binds, evaluated once (a one-molecule eager step is host-bound):
    the projection launchers with the model's arithmetic and activation kind (``cfg.gemm_mode``, ``cfg.act``), the
    configuration, the graph, the stream, the sizes, the degree blocks and the gate columns ``cols[first]``."""
    __slots__ = ("mode", "act", "cfg", "g", "st", "N", "E", "F", "D", "Fe", "lde", "blocks", "cols", "key")

    def __init__(self, cfg: "Config", g: Optional["Graph"] = None, explicit_blocks: bool = False,
                 key: Optional[torch.Tensor] = None):
        self.key = key                             # attention dropout: this call's key, an int64 [2] device tensor (or None)
        self.mode, self.act, self.cfg, self.g, self.st = resolve_mode(cfg.gemm_mode), cfg.act, cfg, g, _stream()
        self.F, self.D, self.Fe, self.lde = cfg.F, cfg.D, cfg.Fe, (1 + cfg.M) * cfg.F
        # columns of (the edge projection [W_re; W_rs], gamma_s.1 / gamma_v.1) a layer computes: attention (edge only), scalar,
        # direction and tensor gates; cols[True]: a first interaction (X_in = 0) -- no tensor gates, a prefix
        n = cfg.lmax if cfg.sep_dir else 1
        self.cols = ((self.lde, cfg.M * cfg.F), ((2 + n) * cfg.F, (1 + n) * cfg.F))
        self.N, self.E = (g.N, g.E) if g is not None else (None, None)      # (no graph: the node-local EQFF layer)
        self.blocks = cfg.degree_blocks(g.N, explicit_blocks) if g is not None else None

    def gemm(self, *args, **kw):
        kw.setdefault("kind", self.act)
        kw.setdefault("mode", self.mode)
        return gemm(*args, **kw)

    def group(self, problems):
        return gemm_group(problems, mode=self.mode, kind=self.act)


def validate_edges(edge_index: torch.Tensor, n_atoms: int) -> int:
    """Bit 0: ``edge_index[1]`` is not non-decreasing (needs a stable sort by target); bit 1: an index is outside
    [0, n_atoms).  One tiny kernel + ONE host read of its flag (a stream synchronisation)."""
    flag = torch.zeros(1, dtype=torch.int32, device=edge_index.device)
    call("gn_check_edges", ptr(edge_index), edge_index.shape[1], n_atoms, ptr(flag), _stream())
    return int(flag.item())


def sorted_edges(edge_index, edge_diff, edge_vec, n_atoms: int):
    """Validate a caller-supplied edge list; returns it target-major (stable: the order inside a target row is kept)
    plus the permutation applied (None when it already was).  Raises on out-of-range indices."""
    if edge_index.shape[1] == 0:
        return edge_index, edge_diff, edge_vec, None
    bits = validate_edges(edge_index, n_atoms)
    if bits & 2:
        raise ValueError(f"edge_index holds indices outside [0, {n_atoms})")
    if not bits & 1:
        return edge_index, edge_diff, edge_vec, None
    order = torch.sort(edge_index[1], stable=True).indices
    return edge_index[:, order].contiguous(), edge_diff[order], edge_vec[order], order


class Graph:
    """CSR-by-target view of a target-sorted edge list + per-edge geometry (K1);
    ``csc()`` adds the by-source view the backward needs.  Topology (index arrays) and geometry (rl, phi, cut)
    are separate: ``set_geometry`` re-evaluates the geometry of a fixed edge list (static-topology steps that are
    replayed from a hipGraph, pipeline.CapturedStep)."""

    def __init__(self, cfg: Config, pw: PackedWeights, n_atoms: int, edge_index: torch.Tensor,
                 edge_diff: Optional[torch.Tensor] = None, edge_vec: Optional[torch.Tensor] = None,
                 self_images: bool = False):
        dev = edge_index.device
        E = edge_index.shape[1]
        self.N, self.E = n_atoms, E
        self.cfg, self.pw = cfg, pw
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.src = torch.empty(E, **i32)
        self.dst = torch.empty(E, **i32)
        self.rowptr = torch.empty(n_atoms + 1, **i32)
        call("gn_build_csr", ptr(edge_index), E, n_atoms, ptr(self.src), ptr(self.dst), ptr(self.rowptr), _stream())
        self.outdeg = None
        if cfg.scale_edge:
            self.outdeg = torch.zeros(n_atoms, **i32)
            call("gn_out_degree", ptr(self.src), E, ptr(self.outdeg), _stream())
        self.rl = torch.empty((E, cfg.D), **f32)
        self.phi = torch.empty((E, max(cfg.R, 0)), **f32)
        self.cut = torch.empty(E, **f32)
        self.perm = self.colptr = self.tgt_by_src = self._work = None      # (_work: ``refresh``'s scratch)
        self.edge_diff = self.edge_vec = None
        #: periodic list (graph.distance_pbc): int32 [E, 3] lattice shifts, the int64 batch vector and the fp32 [n_mol, 3, 3]
        #: cell (``set_periodic``); None for an isolated-molecule list
        self.shift = self.batch = self.cell = None
        #: the list may hold self-images (an atom's own periodic image: src == dst, edge_diff > 0; graph.distance_pbc with
        #: images="all"): the self-loop is then told by src == dst AND edge_diff == 0 (the gn_*_images entry points) instead
        #: of src == dst.  On a list without self-images the two rules agree, bit for bit.
        self.self_images = bool(self_images)
        if edge_vec is not None:
            self.set_geometry(edge_diff, edge_vec)

    def set_periodic(self, shift: torch.Tensor, batch: torch.Tensor, cell: torch.Tensor):
        """Make this a periodic list: ``shift`` int32 [E, 3] in the order of the (target-major) edge list, ``batch`` int64 [N],
        ``cell`` fp32 [n_mol, 3, 3] (rows = lattice vectors).  ``set_positions`` then uses gn_edge_vectors_pbc."""
        if tuple(shift.shape) != (self.E, 3) or batch.shape[0] != self.N or cell.dim() != 3 or tuple(cell.shape[1:]) != (3, 3):
            raise ValueError("set_periodic: shift [E, 3], batch [N] and cell [n_mol, 3, 3] expected")
        self.shift = shift.to(torch.int32).contiguous()
        self.batch = batch.to(torch.int64).contiguous()
        self.cell = cell.detach().to(torch.float32).contiguous()
        return self

    def set_geometry(self, edge_diff: torch.Tensor, edge_vec: torch.Tensor):
        """K1 on the current edge list: unit vectors, real harmonics, radial basis, cutoff."""
        cfg, pw = self.cfg, self.pw
        self.edge_diff, self.edge_vec = edge_diff, edge_vec
        call("gn_edge_geometry_images" if self.self_images else "gn_edge_geometry", ptr(edge_vec), ptr(edge_diff), ptr(self.src), ptr(self.dst), self.E,
             cfg.lmax, cfg.R, cfg.basis, ptr(pw.rb0), ptr(pw.rb1), float(cfg.cutoff),
             ptr(self.rl), ptr(self.phi), ptr(self.cut), _stream())

    def set_positions(self, pos: torch.Tensor, cell: Optional[torch.Tensor] = None):
        """Edge vectors of the fixed edge list for new positions (gn_edge_vectors; gn_edge_vectors_pbc with the stored shifts
        when the list is periodic, for ``cell`` -- fp32 contiguous [n_mol, 3, 3] -- or the graph's own), then the geometry."""
        if self.edge_vec is None:
            self.edge_vec = torch.empty((self.E, 3), dtype=torch.float32, device=pos.device)
            self.edge_diff = torch.empty(self.E, dtype=torch.float32, device=pos.device)
        if self.shift is not None:
            cell = self.cell if cell is None else cell
            if cell.dtype != torch.float32 or not cell.is_contiguous() or tuple(cell.shape) != tuple(self.cell.shape):
                raise ValueError(f"set_positions: cell must be contiguous fp32 {tuple(self.cell.shape)}")
            call("gn_edge_vectors_pbc", ptr(pos), ptr(self.src), ptr(self.dst), ptr(self.shift), ptr(cell), ptr(self.batch),
                 self.E, cell.shape[0], ptr(self.edge_vec), ptr(self.edge_diff), _stream())
        elif cell is not None:
            raise ValueError("set_positions: a cell was given but the graph has no shifts (set_periodic)")
        else:
            call("gn_edge_vectors", ptr(pos), ptr(self.src), ptr(self.dst), self.E, ptr(self.edge_vec), ptr(self.edge_diff),
                 _stream())
        self.set_geometry(self.edge_diff, self.edge_vec)

    def csc(self):
        """Edges grouped by source (stable order: gn_build_csc), no host sync."""
        if self.perm is None:
            i32 = dict(dtype=torch.int32, device=self.src.device)
            self.colptr, self.perm = torch.empty(self.N + 1, **i32), torch.empty(self.E, **i32)
            self.tgt_by_src = torch.empty(self.E, **i32)        # target of each by-source entry
            work = torch.empty(self.N + self.E, **i32)
            call("gn_build_csc", ptr(self.src), ptr(self.dst), self.E, self.N, ptr(self.colptr), ptr(self.perm),
                 ptr(self.tgt_by_src), ptr(work), _stream())
        return self.colptr, self.perm

    def refresh(self, edge_index: torch.Tensor):
        """Re-derive the topology IN PLACE from a new target-major ``edge_index`` of the same shape (gn_graph_refresh: what the
        constructor and ``csc()`` compute, into the buffers that exist; kernel launches only, no allocation after the first
        call, no host sync).  For a list of fixed capacity that is rebuilt on the device (``graph.rebuild_padded``); the geometry
        is the caller's next ``set_geometry``."""
        if (tuple(edge_index.shape) != (2, self.E) or edge_index.dtype != torch.int64 or not edge_index.is_contiguous()
                or edge_index.device != self.src.device):
            raise ValueError(f"refresh: a contiguous int64 [2, {self.E}] edge_index on the graph's device is expected")
        if self.perm is None or self._work is None:
            i32 = dict(dtype=torch.int32, device=self.src.device)
            self.colptr, self.perm = torch.empty(self.N + 1, **i32), torch.empty(self.E, **i32)
            self.tgt_by_src = torch.empty(self.E, **i32)
            self._work = torch.empty(self.N + self.E, **i32)
        call("gn_graph_refresh", ptr(edge_index), self.E, self.N, ptr(self.src), ptr(self.dst), ptr(self.rowptr),
             ptr(self.outdeg), ptr(self.colptr), ptr(self.perm), ptr(self.tgt_by_src), ptr(self._work), _stream())
        return self


@dataclass
class LayerTape:
    """What one layer of ``forward`` writes: a saving forward keeps one per layer (the tape), inference reuses one as scratch."""
    first: bool = False     # forward's ``zero_X_in`` decision, which backward reads: zero-X_in kernels; X_in, X_raw stay None
    h_in: torch.Tensor = None; X_in: torch.Tensor = None; t_in: torch.Tensor = None
    nproj: torch.Tensor = None; xs: torch.Tensor = None; vs: torch.Tensor = None
    eproj: torch.Tensor = None; attn: torch.Tensor = None
    attn_soft: torch.Tensor = None                 # attention dropout: the undropped weights (``attn`` holds the dropped ones)
    EQ: torch.Tensor = None; EK: torch.Tensor = None; w: torch.Tensor = None; pre_t: torch.Tensor = None
    w_raw: torch.Tensor = None; h_raw: torch.Tensor = None; X_raw: torch.Tensor = None
    upd: dict = None                               # intermediates of the composed edge update
    Xp: torch.Tensor = None; ctx: torch.Tensor = None; pre_g1: torch.Tensor = None; mm: torch.Tensor = None
    # parameter gradients only: X after the message stage (EQFF then updates X in place), the activated node projections
    # (columns 2F:4F: the inputs of gamma_s.1 / gamma_v.1) and act(pre_g1) (the input of gamma_m.1)
    X_msg: torch.Tensor = None; nact: torch.Tensor = None; g1act: torch.Tensor = None


@dataclass
class Tape:
    feat: torch.Tensor = None; y_pre: torch.Tensor = None; h0: torch.Tensor = None
    ctx0: torch.Tensor = None; y: torch.Tensor = None           # parameter gradients only: inputs of W_nrd_nru.{0,1}
    layers: List[LayerTape] = field(default_factory=list)
    key: torch.Tensor = None                                     # attention dropout: the key of the forward that wrote the tape


def draw_dropout_key(device, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """One attention-dropout key: int64 [2] = (seed, reserved) drawn ON the device with one ``torch.randint`` launch, from
    ``generator`` or the device's default generator (so ``torch.manual_seed`` makes a run reproducible).  No host read."""
    return torch.randint(0, 2 ** 63 - 1, (2,), dtype=torch.int64, device=device, generator=generator)


def attention_dropout_mask(key: torch.Tensor, layer: int, E: int, H: int, p: float) -> torch.Tensor:
    """The [E, H] multipliers (0 or 1 / (1 - p)) that layer ``layer`` of the call with ``key`` applied to its attention
    weights: the mask function of include/gotennet_hip.h, evaluated by gn_attn_dropout_mask.  Rows are the edges in the
    target-major order the engine runs on (a target-sorted edge list is in that order already)."""
    if not key.is_cuda or key.dtype != torch.int64 or key.numel() < 2 or not key.is_contiguous():
        raise ValueError("key: a contiguous int64 device tensor of two values (GotenNet.last_dropout_key)")
    m = torch.empty((E, H), dtype=torch.float32, device=key.device)
    with torch.cuda.device(key.device):
        call("gn_attn_dropout_mask", ptr(key), int(layer), float(p), E, H, ptr(m), _stream())
    return m


def check_backward_supported(cfg: Config) -> None:
    """Raise NotImplementedError -- BEFORE any launch -- for the configurations whose force path does not exist."""
    if cfg.wide and (cfg.F // 4) // cfg.H > 64:
        raise NotImplementedError(f"n_atom_basis={cfg.F_model or cfg.F} with {cfg.H} heads: the input-gradient kernels keep one "
                                  "attention head inside one wave (at most 256 channels per head)")


def check_param_grads_supported(cfg: Config) -> None:
    """Raise NotImplementedError -- BEFORE any launch -- for the configurations whose parameter gradients do not exist
    (``parameter_grads``): composed edge updates, widths that are not a power of two, and whatever has no force path."""
    if cfg.composed_update:
        raise NotImplementedError("parameter_grads: composed edge updates (edge_updates with 'mlp' / 'mlpa' / 'linw' / "
                                  "'linwa'; evec_dim != n_atom_basis needs one) have no parameter-gradient path")
    if cfg.F_model or cfg.F & (cfg.F - 1):
        raise NotImplementedError(f"parameter_grads: n_atom_basis={cfg.F_model or cfg.F} is not a power of two (the model "
                                  "runs embedded in a wider one); parameter gradients need a power-of-two width")
    check_backward_supported(cfg)


def param_grad_config(cfg: Config) -> Config:
    """The configuration a parameter-gradient forward / backward runs: the un-fused EQFF chain (the fused kernels never
    materialise g_m, dL/d pre_g1 or act(pre_g1))."""
    return dataclasses.replace(cfg, fuse_eqff=False)


def _norm_h(lw: LayerWeights, h: torch.Tensor, emb_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.LayerNorm on h at the GATA input (gotennet.py:397).  ``emb_idx`` (embedded model, embed.py): over the real
    channels -- gathered to a compact tensor for the kernel, scattered back into a zero-padded one."""
    x = h if emb_idx is None else h.index_select(1, emb_idx)
    y = torch.empty_like(x)
    call("gn_layernorm", ptr(x), ptr(lw.ln_w), ptr(lw.ln_b), 1e-5, x.shape[0], x.shape[1], ptr(y), _stream())
    return y if emb_idx is None else torch.zeros_like(h).index_copy_(1, emb_idx, y)


def _norm_X(lw: LayerWeights, X: torch.Tensor, lmax: int, emb_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """TensorLayerNorm on X at the GATA input (gotennet.py:398, layers.py:1497-1563); ``emb_idx`` as in ``_norm_h``."""
    x = X if emb_idx is None else X.index_select(2, emb_idx)
    y = torch.empty_like(x)
    call("gn_tensor_norm", ptr(x), ptr(lw.tln_w), 1e-12, x.shape[0], x.shape[2], lmax, ptr(y), _stream())
    return y if emb_idx is None else torch.zeros_like(X).index_copy_(2, emb_idx, y)


def _norm_h_backward(lw: LayerWeights, h_raw, g_y, g_x, emb_idx: Optional[torch.Tensor] = None):
    """g_x = dL/dh of ``_norm_h`` given g_y = dL/d of its output (embedded: compact -> kernel -> padded layout)."""
    x, gy, gx = h_raw, g_y, g_x
    if emb_idx is not None:                        # (named: alive until the launch)
        x, gy = h_raw.index_select(1, emb_idx), g_y.index_select(1, emb_idx)
        gx = torch.empty_like(gy)
    call("gn_layernorm_backward", ptr(x), ptr(lw.ln_w), 1e-5, ptr(gy), x.shape[0], x.shape[1], ptr(gx), _stream())
    if emb_idx is not None:
        g_x.zero_().index_copy_(1, emb_idx, gx)


def _norm_X_backward(lw: LayerWeights, X_raw, g_y, g_x, lmax: int, emb_idx: Optional[torch.Tensor] = None):
    """g_x = dL/dX of ``_norm_X`` given g_y = dL/d of its output."""
    x, gy, gx = X_raw, g_y, g_x
    if emb_idx is not None:
        x, gy = X_raw.index_select(2, emb_idx), g_y.index_select(2, emb_idx)
        gx = torch.empty_like(gy)
    call("gn_tensor_norm_backward", ptr(x), ptr(lw.tln_w), ptr(gy), 1e-12, x.shape[0], x.shape[2], lmax, ptr(gx), _stream())
    if emb_idx is not None:
        g_x.zero_().index_copy_(2, emb_idx, gx)


def gata_input_norms(cfg: Config, lw: LayerWeights, h: torch.Tensor, X: torch.Tensor):
    """The optional input norms of a GATA layer (gotennet.py:397-398) on their own: -> (h or LN(h), X or TLN(X))."""
    N = h.shape[0]
    return (_norm_h(lw, h) if cfg.layernorm and N else h), (_norm_X(lw, X, cfg.lmax) if cfg.steerable_norm and N else X)


def _htr_problems(p: _Call, lw: LayerWeights, X, EQ, EK):
    """EQ = X W_vq^T and the per-degree EK_l = X_l W_vk_l^T of the HTR edge weights (gotennet.py:561-611)."""
    F_, Fe, N = p.F, p.Fe, p.N
    return [dict(A=X, lda=F_, W=lw.Wvq, C=EQ, ldc=Fe, rows=N * p.D, nout=Fe, K=F_)] + [
        dict(A=X, lda=F_, W=lw.Wvk[k], C=EK, ldc=Fe, rows=rows, nout=Fe, K=F_, rowmap=rowmap)
        for k, rows, rowmap in p.blocks]


def _init_forward(p: _Call, pw: PackedWeights, z32, new, tape: Optional[Tape], pgrads: bool):
    """NodeInit and EdgeInit (gotennet.py:973-977): -> (h [N,F], t [E,F]); fills the init fields of ``tape``."""
    cfg, g, st, F_, R, N, E, gemm = p.cfg, p.g, p.st, p.F, p.cfg.R, p.N, p.E, p.gemm
    feat = new(E, 2 * F_)
    gemm(g.phi, R, pw.Winit, pw.binit, feat, 2 * F_, E, 2 * F_, R)
    ctx0 = new(N, 2 * F_)
    if g.self_images:
        call("gn_node_init_images", ptr(z32), ptr(g.rowptr), ptr(g.src), ptr(feat), 2 * F_, ptr(g.cut),
             ptr(pw.A_na), ptr(pw.A_nbr), N, F_, ptr(g.edge_diff), ptr(ctx0), st)
    else:
        call("gn_node_init", ptr(z32), ptr(g.rowptr), ptr(g.src), ptr(feat), 2 * F_, ptr(g.cut),
             ptr(pw.A_na), ptr(pw.A_nbr), N, F_, ptr(ctx0), st)
    Fc = cfg.Fc or F_                              # (an embedded model keeps this intermediate compact: LayerNorm over the real channels)
    y_pre = new(N, Fc)
    gemm(ctx0, 2 * F_, pw.Wa, pw.ba, y_pre, Fc, N, Fc, 2 * F_)
    y = new(N, Fc)
    call("gn_layernorm_silu", ptr(y_pre), ptr(pw.ln_w), ptr(pw.ln_b), 1e-5, N, Fc, ptr(y), cfg.act, st)
    h = new(N, F_)
    gemm(y, Fc, pw.Wb, pw.bb, h, F_, N, F_, Fc)
    t = new(E, F_)
    call("gn_edge_init", ptr(h), ptr(g.rowptr), ptr(g.src), feat.data_ptr() + 4 * F_, 2 * F_, N, F_, ptr(t), st)
    if tape is not None:
        tape.feat, tape.y_pre, tape.h0 = feat, y_pre, h
        if pgrads:
            tape.ctx0, tape.y = ctx0, y
    return h, t


def _layer_buffers(cfg: Config, N: int, E: int, new, last: bool, save: bool, pgrads: bool = False):
    """-> (LayerTape with the buffers one layer of ``forward`` writes, h2, X2, t2 for its outputs).  A saving forward makes
    them per layer; inference once (``last=False``: the widest set), the outputs ping-ponging against the inputs.  Pre-
    activation copies exist only when saving; ``nact`` / ``g1act`` are the caller's shared scratch unless ``pgrads``."""
    F_, D, M, Fe = cfg.F, cfg.D, cfg.M, cfg.Fe
    lt = LayerTape(xs=new(N, M * F_), vs=new(N, M * F_), eproj=new(E, (1 + M) * F_), attn=new(E, cfg.H),
                   Xp=new(N, D, F_), ctx=new(N, 2 * F_), mm=new(N, 2 * F_))
    if cfg.attn_p > 0:
        lt.attn_soft = new(E, cfg.H)
    if save:
        lt.nproj, lt.pre_g1 = new(N, 4 * F_), new(N, F_)
    if not last:
        lt.EQ, lt.EK, lt.w = new(N, D, Fe), new(N, D, Fe), new(E, Fe)
        if save:
            lt.pre_t = new(E, F_)
            lt.w_raw = new(E, Fe) if (cfg.htr_mode >> 2) else None
    if pgrads:                                     # activated copies: one per layer instead of the shared scratch
        lt.nact, lt.g1act = new(N, 4 * F_), new(N, F_)
    return lt, new(N, F_), new(N, D, F_), (None if last else new(E, F_))


def _gata_forward(p: _Call, lw: LayerWeights, lt: LayerTape, nact, h, X, t, h2, X2, li: int = 0):
    """GATA projections (gotennet.py:400-407) and message stage (452-559, 613-640, 426-427: scores + segment softmax,
    message, aggregate, residual) of one layer: writes h2, X2, ``nact`` and lt.xs, vs, eproj, attn -- and the pre-activation
    copy lt.nproj, where it is not None.  ``lt.first``: X is the zero tensor, no tensor-gate blocks.  With attention
    dropout (``cfg.attn_p > 0``) lt.attn holds the dropped weights of layer ``li`` under the call's key, lt.attn_soft the
    undropped ones."""
    cfg, g, st, F_, lde, N, E, first = p.cfg, p.g, p.st, p.F, p.lde, p.N, p.E, lt.first
    H, M, xs, vs, eproj, attn = cfg.H, cfg.M, lt.xs, lt.vs, lt.eproj, lt.attn
    ne, nv = p.cols[first]
    # The atom-sized node projection rides in the edge projection's launch (its 168 tiles fill the tail of the 5100-tile
    # grid).  SiLU of the two hidden blocks is applied ONCE by the epilogue (a SiLU prologue in the two products below would
    # redo it for each of their 4M column tiles); the pre-activation copy is what the backward needs.
    p.group([dict(A=t, lda=F_, W=_rows(lw, "We", ne) if first else lw.We, bias=lw.be, C=eproj, ldc=lde, rows=E, nout=ne, K=F_),
             dict(A=h, lda=F_, W=lw.Wn1, bias=lw.bn1, C=nact, ldc=4 * F_, rows=N, nout=4 * F_, K=F_,
                  act=(2 * F_, 4 * F_), pre_out=lt.nproj)])
    p.group([dict(A=nact, lda=4 * F_, W=_rows(lw, "Ws2", nv) if first else lw.Ws2, bias=lw.bs2, C=xs, ldc=M * F_, rows=N,
                  nout=nv, K=F_, a_off=2 * F_),
             dict(A=nact, lda=4 * F_, W=_rows(lw, "Wv2", nv) if first else lw.Wv2, bias=lw.bv2, C=vs, ldc=M * F_, rows=N,
                  nout=nv, K=F_, a_off=3 * F_)])
    # q | k are columns [0, 2F) of nact; t_attn (pre-activation) columns [0, F) of eproj, t_filter the rest
    if cfg.attn_p > 0:
        call("gn_attn_softmax_dropout", ptr(nact), nact.data_ptr() + 4 * F_, 4 * F_, ptr(eproj), lde,
             ptr(g.rowptr), ptr(g.src), ptr(g.outdeg), N, F_, H, ptr(lt.attn_soft), ptr(attn), ptr(p.key), li,
             float(cfg.attn_p), cfg.act, st)
    else:
        call("gn_attn_softmax", ptr(nact), nact.data_ptr() + 4 * F_, 4 * F_, ptr(eproj), lde,
             ptr(g.rowptr), ptr(g.src), ptr(g.outdeg), N, F_, H, ptr(attn), cfg.act, st)
    call("gn_message_aggregate", ptr(xs), ptr(vs), M * F_, eproj.data_ptr() + 4 * F_, lde,
         ptr(attn), ptr(g.rl), ptr(g.cut), ptr(g.rowptr), ptr(g.src), ptr(h), None if first else ptr(X), ptr(h2), ptr(X2),
         N, F_, H, cfg.lmax_arg_msg, int(cfg.sep_dir), int(cfg.sep_tensor), st)


def _eqff_htr_forward(p: _Call, lw: LayerWeights, lt: LayerTape, g1act, h, X, t, t2, save: bool, eq_fused: bool):
    """X-products, EQFF (gotennet.py:731-746: h, X updated in place) and HTR edge weights + edge update (561-611: t2, where
    the layer has one) of one layer, on the message stage's h, X."""
    cfg, g, st, F_, D, Fe, N, E = p.cfg, p.g, p.st, p.F, p.D, p.Fe, p.N, p.E
    last, Xp, ctx, mm = lw.Wt is None, lt.Xp, lt.ctx, lt.mm
    # every product of the updated X (X W_vu^T for EQFF; EQ and the per-degree EK_l for HTR) in one launch
    xprods = [dict(A=X, lda=F_, W=lw.Wvu, C=Xp, ldc=F_, rows=N * D, nout=F_, K=F_)]
    if not last:
        xprods += _htr_problems(p, lw, X, lt.EQ, lt.EK)
    p.group(xprods)
    # Where covered the EQFF chain after X_p is ONE kernel (context, both gamma_m layers, update); else: context kernel, the
    # first gamma_m layer riding in the launch of the edge-sized gamma_t product, the second layer, update kernel
    m0 = None
    if eq_fused:
        call("gn_eqff_fused_forward", ptr(Xp), ptr(split_weight(lw.Wm0, p.mode)), ptr(lw.bm0),
             ptr(split_weight(lw.Wm1, p.mode)), ptr(lw.bm1), float(cfg.eps), N, F_, D, ptr(h), ptr(X),
             ptr(ctx) if save else None, ptr(lt.pre_g1), ptr(mm) if save else None, 1 if p.mode == "split" else 2, st)
    else:
        call("gn_eqff_context", ptr(h), ptr(Xp), float(cfg.eps), N, F_, D, ptr(ctx), st)
        m0 = dict(A=ctx, lda=2 * F_, W=lw.Wm0, bias=lw.bm0, C=g1act, ldc=F_, rows=N, nout=F_, K=2 * F_, act=(0, F_),
                  pre_out=lt.pre_g1)
    if last:
        p.group([m0])
    else:
        call("gn_htr_edge", ptr(lt.EQ), ptr(lt.EK), ptr(g.rl), ptr(g.rowptr), ptr(g.src), N, Fe, cfg.lmax_arg, cfg.htr_mode,
             ptr(lt.w_raw), ptr(lt.w), st)
        if cfg.composed_update:
            upd = _edge_update_composed(cfg, lw, t, lt.w, t2, E, lt.pre_t)
            if save:
                lt.upd = upd
            p.group([m0])
        else:
            p.group([dict(A=t, lda=F_, W=lw.Wt, bias=lw.bt, C=t2, ldc=F_, rows=E, nout=F_, K=F_, act=(0, F_), res=t,
                          gate=lt.w, pre_out=lt.pre_t), m0])
    if not eq_fused:
        p.gemm(g1act, F_, lw.Wm1, lw.bm1, mm, 2 * F_, N, 2 * F_, F_)
        call("gn_eqff_update", ptr(mm), ptr(Xp), N, F_, D, ptr(h), ptr(X), st)


def forward(cfg: Config, pw: PackedWeights, z32: torch.Tensor, g: Graph, save: bool = False,
            trace: Optional[list] = None, pgrads: bool = False, key: Optional[torch.Tensor] = None):
    """-> (h [N,F], X [N,D,F], tape or None).  ``save`` keeps what ``backward`` needs; ``pgrads`` (with ``save``, and a
    ``param_grad_config``) also keeps the inputs of every projection for the parameter gradients;
    ``trace`` (tests only) collects per-layer clones of (h, X, t).  ``key``: the call's attention-dropout key
    (``draw_dropout_key``), required when ``cfg.attn_p > 0``; the tape keeps it next to both attention arrays."""
    F_, D, N, E = cfg.F, cfg.D, g.N, g.E
    if save:
        check_backward_supported(cfg)               # before any launch: a saving forward is only run for a backward
    if pgrads:
        check_param_grads_supported(cfg)
        if not save or cfg.fuse_eqff is not False:
            raise ValueError("internal: a parameter-gradient forward saves its tape and runs the un-fused EQFF chain")
    if cfg.attn_p > 0 and key is None:
        raise ValueError("internal: a forward with attention dropout needs the call's key (draw_dropout_key)")
    p = _Call(cfg, g, key=key)
    f32 = dict(dtype=torch.float32, device=z32.device)
    new = lambda *shape: torch.empty(shape, **f32)
    tape = Tape(key=key) if save else None
    h, t = _init_forward(p, pw, z32, new, tape, pgrads)
    # gotennet.py:992: X starts as the zero tensor.  Where the first interaction runs the zero-X_in kernels nothing ever reads
    # it (message stage and message backward get a null X_in): no fill launch
    X = new(N, D, F_) if (zero_X_in(cfg, 0) and pw.layers) else torch.zeros((N, D, F_), **f32)
    nact, g1act = new(N, 4 * F_), new(N, F_)       # activated copies (scratch, shared by all layers)
    eq_fused = eqff_fused_ok(cfg, N)
    if not save:                                   # inference: one set of work buffers, reused by every layer
        lt, h2, X2, t2 = _layer_buffers(cfg, N, E, new, last=False, save=False)

    for li, lw in enumerate(pw.layers):
        first = zero_X_in(cfg, li)                  # X is the zero tensor made above; the tape carries the decision
        h_raw, X_raw = h, X
        if cfg.layernorm:                          # gotennet.py:397-398: the layer (and its residuals) see the normalised values
            h = _norm_h(lw, h, pw.emb_idx)
        if cfg.steerable_norm:
            X = _norm_X(lw, X, cfg.lmax, pw.emb_idx)
        if save:                                   # every layer keeps its own activations
            lt, h2, X2, t2 = _layer_buffers(cfg, N, E, new, lw.Wt is None, True, pgrads)
            lt.h_in, lt.t_in, lt.h_raw = h, t, h_raw
            if not first:                          # (the uninitialised X of a zero-X_in layer never enters the tape)
                lt.X_in, lt.X_raw = X, X_raw
            tape.layers.append(lt)
            if pgrads:
                nact, g1act = lt.nact, lt.g1act
        lt.first = first
        _gata_forward(p, lw, lt, nact, h, X, t, h2, X2, li)
        h, h2 = h2, h
        X, X2 = X2, X
        if pgrads:
            lt.X_msg = X.clone()
        _eqff_htr_forward(p, lw, lt, g1act, h, X, t, t2, save, eq_fused)
        if lw.Wt is not None:
            t, t2 = t2, t
        if trace is not None:
            trace.append((h.clone(), X.clone(), t.clone()) if pw.emb_idx is None else
                         tuple(v.index_select(v.dim() - 1, pw.emb_idx) for v in (h, X, t)))
    if pw.emb_idx is not None:                     # embedded model: the real channels, in the model's own order
        h, X = h.index_select(1, pw.emb_idx), X.index_select(2, pw.emb_idx)
    return h, X, tape


def gata_layer(cfg: Config, lw: LayerWeights, g: "Graph", h: torch.Tensor, X: torch.Tensor, t: torch.Tensor,
               key: Optional[torch.Tensor] = None):
    """ONE GATA layer (gotennet.py:366-450) on its own, no backward: what ``GATA.forward`` of the mirror module runs
    when a caller composes layers directly.  Same kernels as ``forward`` (which additionally fuses the neighbouring EQFF
    launches into the grouped GEMMs).  ``g`` carries the CSR view, rl and the cosine cutoff.  With ``cfg.attn_p > 0``
    (a module in training mode) attention dropout is applied as layer 0 of ``key``.  -> (h', X', t')."""
    F_, D, M, Fe, N, E = cfg.F, cfg.D, cfg.M, cfg.Fe, g.N, g.E
    if cfg.attn_p > 0 and key is None:
        raise ValueError("internal: a layer with attention dropout needs the call's key (draw_dropout_key)")
    p = _Call(cfg, g, key=key)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=h.device)
    if cfg.layernorm:
        h = _norm_h(lw, h)
    if cfg.steerable_norm:
        X = _norm_X(lw, X, cfg.lmax)
    lt = LayerTape(xs=new(N, M * F_), vs=new(N, M * F_), eproj=new(E, p.lde), attn=new(E, cfg.H),
                   attn_soft=new(E, cfg.H) if cfg.attn_p > 0 else None)
    h2, X2 = new(N, F_), new(N, D, F_)
    _gata_forward(p, lw, lt, new(N, 4 * F_), h, X, t, h2, X2)
    if lw.Wt is None:
        return h2, X2, t
    EQ, EK, w, t2 = new(N, D, Fe), new(N, D, Fe), new(E, Fe), new(E, F_)
    p.group(_htr_problems(p, lw, X2, EQ, EK))
    call("gn_htr_edge", ptr(EQ), ptr(EK), ptr(g.rl), ptr(g.rowptr), ptr(g.src), N, Fe, cfg.lmax_arg, cfg.htr_mode, None, ptr(w),
         p.st)
    if cfg.composed_update:
        _edge_update_composed(cfg, lw, t, w, t2, E, None)
    else:
        p.gemm(t, F_, lw.Wt, lw.bt, t2, F_, E, F_, F_, act=(0, F_), res=t, gate=w)
    return h2, X2, t2


def eqff_layer(cfg: Config, lw: LayerWeights, h: torch.Tensor, X: torch.Tensor):
    """ONE EQFF block (gotennet.py:716-748) on its own, inference only (``EQFF.forward`` of the mirror module).
    Returns NEW tensors (h', X')."""
    F_, D, N = cfg.F, cfg.D, h.shape[0]
    p = _Call(cfg)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=h.device)
    Xp, ctx, g1, mm = new(N, D, F_), new(N, 2 * F_), new(N, F_), new(N, 2 * F_)
    p.gemm(X, F_, lw.Wvu, None, Xp, F_, N * D, F_, F_)
    call("gn_eqff_context", ptr(h), ptr(Xp), float(cfg.eps), N, F_, D, ptr(ctx), p.st)
    p.gemm(ctx, 2 * F_, lw.Wm0, lw.bm0, g1, F_, N, F_, 2 * F_, act=(0, F_))
    p.gemm(g1, F_, lw.Wm1, lw.bm1, mm, 2 * F_, N, 2 * F_, F_)
    h, X = h.clone(), X.clone()
    call("gn_eqff_update", ptr(mm), ptr(Xp), N, F_, D, ptr(h), ptr(X), p.st)
    return h, X

#: ``fuse_eqff = None`` (auto): fused up to this many atoms per call (measured crossover between 672 and 2688 atoms at F = 256)
EQFF_FUSED_MAX_ATOMS = 1024


def eqff_fused_ok(cfg: Config, n_atoms: Optional[int] = None) -> bool:
    """The EQFF chains run as one kernel each way (gn_eqff_fused_forward / _backward): F in {128, 256}, SiLU, a plane
    arithmetic; everything else keeps the launch sequence.  ``cfg.fuse_eqff`` None: decided by the system size."""
    mode = resolve_mode(cfg.gemm_mode)
    want = cfg.fuse_eqff if cfg.fuse_eqff is not None else (n_atoms is not None and n_atoms <= EQFF_FUSED_MAX_ATOMS)
    if not want or mode not in _PLANE_MODES:
        return False
    return bool(_lib.load().gn_eqff_fused_supported(cfg.F, cfg.act, 1 if mode == "split" else 2))


def _edge_update_composed(cfg: Config, lw: LayerWeights, t, w_raw, t2, E: int, pre_t):
    """t2 = t + gamma_t(t) * gamma_w(w) for the non-default variants (gotennet.py:236-291, 611):
    gamma_w = [LayerNorm "ln"] -> [SiLU "linwa"] -> W_edp "linw"/"linwa" [-> LayerNorm "postln"] -> [gate];
    gamma_t = Dense -> [LayerNorm edge_ln] -> SiLU -> Dense [-> SiLU unless "mlp"]  ("mlp"/"mlpa"), or the
    default SiLU(Dense).  Returns the intermediates the backward needs."""
    F_, Fe, Fm = cfg.F, cfg.Fe, cfg.Fm
    gemm = _Call(cfg).gemm
    new = lambda width=F_: torch.empty((E, width), dtype=torch.float32, device=t.device)
    st = _stream()
    u = dict(w_raw=w_raw)
    x = w_raw
    if cfg.lin_w:
        a_in = x
        if cfg.lin_ln == 1:
            a_in = new(Fe)
            call("gn_layernorm", ptr(x), ptr(lw.w_ln_w), ptr(lw.w_ln_b), 1e-5, E, Fe, ptr(a_in), st)
        lin = new()
        gemm(a_in, Fe, lw.Wedp, lw.bedp, lin, F_, E, F_, Fe, pro=(1, 0, Fe) if cfg.lin_w == 2 else (0, 0, 0))
        x = lin
        if cfg.lin_ln == 2:
            x = new()
            call("gn_layernorm", ptr(lin), ptr(lw.w_ln_w), ptr(lw.w_ln_b), 1e-5, E, F_, ptr(x), st)
        u.update(a_in=a_in, lin=lin)
    u["pre_gate"] = x
    if cfg.gate_kind:
        wg = new()
        call("gn_gate", ptr(x), cfg.gate_kind, E * F_, ptr(wg), st)
    else:
        wg = x
    u["wg"] = wg
    act = (0, F_) if cfg.t_last_act == 3 else (0, 0)
    if lw.Wt0 is not None:
        hid = new(Fm)
        gemm(t, F_, lw.Wt0, lw.bt0, hid, Fm, E, Fm, F_)
        u_in = hid
        if lw.t_ln_w is not None:
            u_in = new(Fm)
            call("gn_layernorm", ptr(hid), ptr(lw.t_ln_w), ptr(lw.t_ln_b), 1e-5, E, Fm, ptr(u_in), st)
        gemm(u_in, Fm, lw.Wt, lw.bt, t2, F_, E, F_, Fm, act=act, res=t, gate=wg, pre_out=pre_t, pro=(1, 0, Fm))
        u.update(hid=hid, u_in=u_in)
    else:
        gemm(t, F_, lw.Wt, lw.bt, t2, F_, E, F_, F_, act=act, res=t, gate=wg, pre_out=pre_t)
    return u


def _edge_update_composed_backward(cfg: Config, lw: LayerWeights, lt, gt, gt_a, E: int):
    """Input-gradients of _edge_update_composed: writes gt_a = gt + (d/dt through gamma_t) and returns dL/dw [E,F]."""
    F_, Fe, Fm = cfg.F, cfg.Fe, cfg.Fm
    gemm = _Call(cfg).gemm
    new = lambda width=F_: torch.empty((E, width), dtype=torch.float32, device=gt.device)
    st = _stream()
    u = lt.upd
    g_pre, g_wg = new(), new()
    call("gn_edge_gate_backward", ptr(gt), ptr(lt.pre_t), cfg.act if cfg.t_last_act else -1, ptr(u["wg"]), E * F_, ptr(g_pre), ptr(g_wg), st)
    if lw.Wt0 is not None:
        g_u = new(Fm)
        gemm(g_pre, F_, _T(lw, "Wt"), None, g_u, Fm, E, Fm, F_, dgate=u["u_in"])
        if lw.t_ln_w is not None:
            g_h = new(Fm)
            call("gn_layernorm_backward", ptr(u["hid"]), ptr(lw.t_ln_w), 1e-5, ptr(g_u), E, Fm, ptr(g_h), st)
            g_u = g_h
        gemm(g_u, Fm, _T(lw, "Wt0"), None, gt_a, F_, E, F_, Fm, res=gt)
    else:
        gemm(g_pre, F_, _T(lw, "Wt"), None, gt_a, F_, E, F_, F_, res=gt)
    gq = g_wg
    if cfg.gate_kind:
        g2 = new()
        call("gn_gate_backward", ptr(gq), ptr(u["pre_gate"]), cfg.gate_kind, E * F_, ptr(g2), st)
        gq = g2
    if cfg.lin_w:
        if cfg.lin_ln == 2:
            g2 = new()
            call("gn_layernorm_backward", ptr(u["lin"]), ptr(lw.w_ln_w), 1e-5, ptr(gq), E, F_, ptr(g2), st)
            gq = g2
        g3 = new(Fe)
        gemm(gq, F_, _T(lw, "Wedp"), None, g3, Fe, E, Fe, F_, dgate=u["a_in"] if cfg.lin_w == 2 else None)
        gq = g3
        if cfg.lin_ln == 1:
            g4 = new(Fe)
            call("gn_layernorm_backward", ptr(u["w_raw"]), ptr(lw.w_ln_w), 1e-5, ptr(gq), E, Fe, ptr(g4), st)
            gq = g4
    return gq


def weight_grad_group(problems, mode: Optional[str] = None):
    """Several independent weight gradients dW = dY^T A (+ db = sum_r dY) as one launch (gn_weight_grad_group).  A
    problem is a dict: dY, ldy, A, lda, dW (its rows [w_row, w_row + nout) are written), rows, nout, K; optional y_off,
    a_off (column offsets), db (with b_row), rowmap (cnt, gstride, goff).  ``mode``: the arithmetic (``WGRAD_MODES``;
    None = ``WGRAD_MODE``); anything but "f32" goes through gn_weight_grad_group_mode."""
    mode = resolve_wgrad_mode(mode)
    problems = [q for q in problems if q is not None]
    if not problems:
        return
    arr = (_lib.WgradDesc * len(problems))()
    for d, q in zip(arr, problems):
        g = q.get
        dW = q["dW"]
        d.dY, d.ldy, d.y_off = q["dY"].data_ptr(), q["ldy"], g("y_off", 0)
        d.A, d.lda, d.a_off = q["A"].data_ptr(), q["lda"], g("a_off", 0)
        d.dW, d.ldw = dW.data_ptr() + 4 * g("w_row", 0) * dW.shape[-1], dW.shape[-1]
        db = g("db")
        d.db = (db.data_ptr() + 4 * g("b_row", 0)) if db is not None else None
        d.rows, d.nout, d.K = q["rows"], q["nout"], q["K"]
        d.row_cnt, d.row_gstride, d.row_goff = g("rowmap", (1, 1, 0))
    lib, dev = _lib.load(), problems[0]["dW"].device
    if mode == "f32":
        work = torch.empty(max(1, lib.gn_weight_grad_workspace(arr, len(problems))), dtype=torch.float32, device=dev)
        call("gn_weight_grad_group", arr, len(problems), ptr(work), work.numel(), _stream())
        return
    code = _WGRAD_CODE[mode]
    work = torch.empty(max(1, lib.gn_weight_grad_workspace_mode(arr, len(problems), code)), dtype=torch.float32, device=dev)
    call("gn_weight_grad_group_mode", arr, len(problems), code, ptr(work), work.numel(), _stream())


def layernorm_param_grad(x, gamma, beta, g_out, act: int, dgamma, dbeta):
    """dgamma, dbeta of a LayerNorm over the last axis of x [N, C] (eps 1e-5) followed by the activation ``act``
    (GN_ACT_NONE: a bare nn.LayerNorm); g_out is the gradient at the activation's output."""
    N, C = x.shape
    work = torch.empty(max(1, _lib.load().gn_layernorm_param_grad_workspace(N, C)), dtype=torch.float32, device=x.device)
    call("gn_layernorm_param_grad", ptr(x), ptr(gamma), ptr(beta), 1e-5, ptr(g_out), N, C, act, ptr(work), ptr(dgamma),
         ptr(dbeta), _stream())


def empty_grads(pw: PackedWeights) -> PackedWeights:
    """Gradient storage in the layout of the pack (every trainable operand; buffers stay None).  The parameter-gradient
    backward writes every element."""
    e = lambda t: None if t is None else torch.empty_like(t)
    out = PackedWeights(A_na=e(pw.A_na), A_nbr=e(pw.A_nbr), Winit=e(pw.Winit), binit=e(pw.binit), Wa=e(pw.Wa), ba=e(pw.ba),
                        ln_w=e(pw.ln_w), ln_b=e(pw.ln_b), Wb=e(pw.Wb), bb=e(pw.bb), rb0=None, rb1=None)
    for lw in pw.layers:
        out.layers.append(LayerWeights(
            Wn1=e(lw.Wn1), bn1=e(lw.bn1), Ws2=e(lw.Ws2), bs2=e(lw.bs2), Wv2=e(lw.Wv2), bv2=e(lw.bv2), We=e(lw.We), be=e(lw.be),
            Wvu=e(lw.Wvu), Wm0=e(lw.Wm0), bm0=e(lw.bm0), Wm1=e(lw.Wm1), bm1=e(lw.bm1), Wt=e(lw.Wt), bt=e(lw.bt),
            Wvq=e(lw.Wvq), Wvk=[e(w) for w in lw.Wvk], ln_w=e(lw.ln_w), ln_b=e(lw.ln_b)))
    return out


def _partial_sum_layout(cfg: Config, pw: PackedWeights) -> dict:
    """The slices of the per-edge partial sums dL/drl [n_rl, E, D] and dL/dcut [n_cut, E]: every contributing kernel writes
    its own and gn_edge_geometry_backward adds them in index order, so the slice numbers are part of the bits:
      rl:   Wm per message backward (layer li: from ``msg_rl * li``), then Wh per HTR backward in layer order (``htr_rl[li]``);
      cut:  Wm * G per message backward (G degree groups; from ``msg_cut * li``), then Wm of the node-init backward (``init_cut``).
    Wm, Wh: partial slices per writing call (a slot wider than a wave writes one per 64-lane part: F / 256, Fe / 256)."""
    L = len(pw.layers)
    G = _lib.load().gn_message_backward_groups(cfg.lmax_arg_msg_bwd, int(cfg.sep_dir), int(cfg.sep_tensor), cfg.act)
    Wm, Wh = max(1, cfg.F // 256), max(1, cfg.Fe // 256)
    htr = [li for li, lw in enumerate(pw.layers) if lw.Wt is not None]
    return dict(G=G, msg_rl=Wm, msg_cut=Wm * G, init_cut=Wm * G * L, htr_rl={li: Wm * L + Wh * i for i, li in enumerate(htr)},
                n_rl=Wm * L + Wh * len(htr), n_cut=Wm * (G * L + 1))


@dataclass
class _BackwardWork:
    """Work buffers of ``backward``, reused by every layer, with the slice layout of the partial sums and the by-source
    view of the graph: made by ``_backward_work``, which says what each buffer holds."""
    gh: Any; gX: Any; gt: Any; colptr: Any; perm: Any; g_rl_parts: Any; g_cut_parts: Any; ga_parts: Any
    G: int; msg_rl: int; msg_cut: int; init_cut: int; htr_rl: dict; n_rl: int; n_cut: int
    gm: Any; gXp: Any; g_g1: Any; g_ctx: Any; gh1: Any; gX1: Any; gh2: Any; gX2: Any; gh_qk: Any; gEQ: Any; gEK: Any
    g_eproj: Any; g_s: Any; g_nproj: Any; g_x: Any; g_v: Any; gt_a: Any; gt_b: Any; g_pre_t: Any
    dt_kcat: bool = False                          # dL/dt = gt + [g_eproj | g_pre_t] [We | Wt]^T in ONE launch (``_dt_kcat``)


def _dt_kcat(cfg: Config) -> bool:
    """A layer with a plain edge update states dL/dt of its input ONCE, as a product over the concatenated K of g_eproj and
    g_pre_t (``_gata_backward``).  Not with ``composed_update`` (its gamma_t backward is a chain of its own), nor where the
    K-prefix of g_eproj is no whole number of K-slabs (the segment boundary of the projection kernels)."""
    n = cfg.lmax if cfg.sep_dir else 1
    return DT_KCAT and not cfg.composed_update and ((2 + n) * cfg.F) % 32 == 0 and ((1 + cfg.M) * cfg.F) % 32 == 0


def _backward_work(cfg: Config, pw: PackedWeights, g: Graph, f32: dict, gh, gX, eq_fused: bool) -> _BackwardWork:
    """The caller's adjoints brought into the engine's layout, and every work buffer (the ONE allocation site)."""
    F_, D, M, H, Fe, N, E = cfg.F, cfg.D, cfg.M, cfg.H, cfg.Fe, g.N, g.E
    new = lambda *shape: torch.empty(shape, **f32)
    if pw.emb_idx is not None:                     # embedded model: gradients arrive in the real layout
        gh = torch.zeros((N, F_), **f32).index_copy_(1, pw.emb_idx, gh.contiguous())
        if gX is not None:
            gX = torch.zeros((N, D, F_), **f32).index_copy_(2, pw.emb_idx, gX.contiguous())
    # dL/dX = None (an energy head reads h only): the un-fused EQFF backward takes a null pointer for it (no zero-filled
    # [N,D,F] tensor is made, written or read); the fused kernel wants the tensor
    if gX is None and eq_fused:
        gX = torch.zeros((N, D, F_), **f32)
    lay = _partial_sum_layout(cfg, pw)
    colptr, perm = g.csc()
    kcat = _dt_kcat(cfg)
    return _BackwardWork(
        # dL/d of the current layer's output h, X (None = 0), t (None = 0: nothing above the last layer reads t): rotate per layer
        gh=gh.contiguous(), gX=None if gX is None else gX.contiguous(), gt=None, colptr=colptr, perm=perm, **lay,
        g_rl_parts=new(lay["n_rl"], E, D), g_cut_parts=new(lay["n_cut"], E),
        # head sums of g_a: G partial slices (degree groups), or the merged kernel's one; aggr = "max": the per-message
        # gradient workspace of the routing kernel instead
        ga_parts=new(E, 1 + D, F_) if cfg.aggr == 2 else new(lay["G"], E, H),
        gm=new(N, 2 * F_), gXp=new(N, D, F_), g_g1=new(N, F_), g_ctx=new(N, 2 * F_),     # EQFF: dL/d mm, X_p, pre_g1, context
        gh1=new(N, F_), gX1=new(N, D, F_),             # dL/d of the message stage's output
        gh2=new(N, F_), gX2=new(N, D, F_), gh_qk=new(N, F_),     # dL/d of the layer's input (gh_qk: its q | k part)
        gEQ=new(N, D, Fe), gEK=new(N, D, Fe),          # HTR
        g_eproj=new(E, (1 + M) * F_), g_s=new(E, H), g_nproj=new(N, 4 * F_), g_x=new(N, M * F_), g_v=new(N, M * F_),   # message backward
        # dL/dt after the edge update (only where it is a tensor of its own) / of the layer input; dL/d pre_t
        gt_a=None if kcat else new(E, F_), gt_b=new(E, F_), g_pre_t=new(E, F_), dt_kcat=kcat)


def _eqff_htr_backward(p: _Call, lw: LayerWeights, lt: LayerTape, wb: _BackwardWork, li: int, eq_fused: bool, gw):
    """EQFF backward (reads gh, gX: writes gXp, gh1 -- and gm, g_g1, g_ctx un-fused); independent of it, the HTR + edge-update
    backward of a layer that has one (reads gt: writes gEQ, gEK, g_pre_t, gt_a, the layer's HTR slice of dL/drl); then the
    X-products' (gX1 = dL/dX at the message stage's output).  ``gw``: the layer's parameter-gradient storage or None.
    -> dL/dt at the layer's message stage (gt_a, or gt itself where t passes through unchanged -- and with ``wb.dt_kcat``,
    where the edge update's term g_pre_t Wt^T is left to the K-concatenated launch of ``_gata_backward``)."""
    cfg, g, st, F_, D, Fe, N, E = p.cfg, p.g, p.st, p.F, p.D, p.Fe, p.N, p.E
    gh, gX, gt = wb.gh, wb.gX, wb.gt
    m1 = None
    if eq_fused:                                   # one kernel
        call("gn_eqff_fused_backward", ptr(gh), ptr(gX), ptr(lt.mm), ptr(lt.Xp), ptr(lt.ctx), ptr(lt.pre_g1),
             ptr(split_weight(_T(lw, "Wm1"), p.mode)), ptr(split_weight(_T(lw, "Wm0"), p.mode)), N, F_, D,
             ptr(wb.gXp), ptr(wb.gh1), 1 if p.mode == "split" else 2, st)
    else:                                          # its first half here; the gamma_m.1 product rides below
        call("gn_eqff_backward_a", ptr(gh), ptr(gX), ptr(lt.mm), ptr(lt.Xp), N, F_, D, ptr(wb.gm), ptr(wb.gXp), st)
        m1 = dict(A=wb.gm, lda=2 * F_, W=_T(lw, "Wm1"), C=wb.g_g1, ldc=F_, rows=N, nout=F_, K=2 * F_,
                  dgate=lt.pre_g1)                 # * SiLU'(pre) in the epilogue
    if lw.Wt is None:
        p.group([m1])
        gt_in = gt                                 # no edge update in this layer: t passes through unchanged
    else:
        if gt is None:
            raise RuntimeError("internal: missing edge gradient")
        rl_slice = wb.g_rl_parts.data_ptr() + 4 * E * D * wb.htr_rl[li]
        if cfg.composed_update:                    # gt_a = gt + gamma_t backward; g_w = gamma_w backward
            g_w = _edge_update_composed_backward(cfg, lw, lt, gt, wb.gt_a, E)
            call("gn_htr_backward", ptr(g_w), None, None, None, ptr(lt.EQ), ptr(lt.EK), ptr(g.rl),
                 ptr(g.rowptr), ptr(g.src), ptr(g.tgt_by_src), ptr(wb.colptr), ptr(wb.perm), N, Fe, cfg.lmax_arg_bwd, cfg.htr_mode | 16,
                 ptr(wb.gEQ), ptr(wb.gEK), rl_slice, None, cfg.act, st)
            p.group([m1])
        else:
            call("gn_htr_backward", ptr(gt), ptr(lt.pre_t), ptr(lt.w), ptr(lt.w_raw), ptr(lt.EQ), ptr(lt.EK),
                 ptr(g.rl), ptr(g.rowptr), ptr(g.src), ptr(g.tgt_by_src), ptr(wb.colptr), ptr(wb.perm), N, Fe, cfg.lmax_arg_bwd,
                 cfg.htr_mode, ptr(wb.gEQ), ptr(wb.gEK), rl_slice, ptr(wb.g_pre_t), cfg.act, st)
            if wb.dt_kcat:                         # g_pre_t Wt^T joins g_eproj We^T in _gata_backward; gamma_m's product alone
                p.group([m1])
            else:
                # gt_a = gt + ((gt * w) * SiLU'(pre_t)) Wt; the atom-sized gamma_m product rides in its launch
                p.group([dict(A=wb.g_pre_t, lda=F_, W=_T(lw, "Wt"), C=wb.gt_a, ldc=F_, rows=E, nout=F_, K=F_, res=gt), m1])
        gt_in = gt if wb.dt_kcat else wb.gt_a
    if not eq_fused:                               # EQFF backward, second half
        p.gemm(wb.g_g1, F_, _T(lw, "Wm0"), None, wb.g_ctx, 2 * F_, N, 2 * F_, F_)
        call("gn_eqff_backward_b", ptr(wb.g_ctx), ptr(lt.ctx), ptr(lt.Xp), ptr(gh), N, F_, D, ptr(wb.gXp), ptr(wb.gh1), st)
    if gw is not None:
        _layer_weight_grads_eqff_htr(cfg, gw, lt, wb, N, E)
    # ---- gX1 = gX + gXp W_vu (+ gEQ W_vq + gEK_l W_vk_l)
    gX1, gXp = wb.gX1, wb.gXp
    if lw.Wt is None:
        p.gemm(gXp, F_, _T(lw, "Wvu"), None, gX1, F_, N * D, F_, F_, res=gX)
    elif Fe == F_:
        # one launch; per degree block: A = [gXp | gEQ | gEK] (K-segmented), W = [W_vu^T | W_vq^T | W_vk_l^T] along K
        wcat = lambda k: derived(lw, ("Xcat", k), lambda: torch.cat([_T(lw, "Wvu"), _T(lw, "Wvq"), lw.Wvk[k].t()], 1).contiguous())
        p.group([dict(A=gXp, A2=wb.gEQ, A3=wb.gEK, a_seg=F_, lda=F_, W=wcat(k), C=gX1, ldc=F_, rows=rows,
                      nout=F_, K=3 * F_, rowmap=rowmap, res=gX) for k, rows, rowmap in p.blocks])
    else:                                          # evec_dim != F: three chained products
        p.gemm(gXp, F_, _T(lw, "Wvu"), None, gX1, F_, N * D, F_, F_, res=gX)
        p.gemm(wb.gEQ, Fe, _T(lw, "Wvq"), None, gX1, F_, N * D, F_, Fe, res=gX1)
        for k, rows, rowmap in p.blocks:
            wkT = derived(lw, ("Wvk", k), lambda: lw.Wvk[k].t().contiguous())
            p.gemm(wb.gEK, Fe, wkT, None, gX1, F_, rows, F_, Fe, rowmap=rowmap, res=gX1)
    return gt_in


def _layer_weight_grads_eqff_htr(cfg: Config, gw: LayerWeights, lt: LayerTape, wb: _BackwardWork, N: int, E: int):
    """dL/d of gamma_m, W_vu and -- in a layer with an edge update -- gamma_t, W_vq, W_vk.  Reads gm, g_g1, gXp, g_pre_t,
    gEQ, gEK, which the next layer's ``_eqff_htr_backward`` overwrites: called as soon as this layer's has written them."""
    F_, D, Fe = cfg.F, cfg.D, cfg.Fe
    probs = [dict(dY=wb.gm, ldy=2 * F_, A=lt.g1act, lda=F_, dW=gw.Wm1, db=gw.bm1, rows=N, nout=2 * F_, K=F_),
             dict(dY=wb.g_g1, ldy=F_, A=lt.ctx, lda=2 * F_, dW=gw.Wm0, db=gw.bm0, rows=N, nout=F_, K=2 * F_),
             dict(dY=wb.gXp, ldy=F_, A=lt.X_msg, lda=F_, dW=gw.Wvu, rows=N * D, nout=F_, K=F_)]
    if gw.Wt is not None:
        probs += [dict(dY=wb.g_pre_t, ldy=F_, A=lt.t_in, lda=F_, dW=gw.Wt, db=gw.bt, rows=E, nout=F_, K=F_),
                  dict(dY=wb.gEQ, ldy=Fe, A=lt.X_msg, lda=F_, dW=gw.Wvq, rows=N * D, nout=Fe, K=F_)]
        probs += [dict(dY=wb.gEK, ldy=Fe, A=lt.X_msg, lda=F_, dW=gw.Wvk[k], rows=rows, nout=Fe, K=F_, rowmap=rowmap)
                  for k, rows, rowmap in cfg.degree_blocks(N)]
    weight_grad_group(probs, cfg.wgrad_mode)


def _gata_backward(p: _Call, lw: LayerWeights, lt: LayerTape, wb: _BackwardWork, li: int, gt_in, gw):
    """Message backward and the GATA projections' input-gradients: reads gh1, gX1 and ``gt_in`` (dL/dt at the message
    stage), writes gh2, gX2 (not for a zero-X_in layer), gt_b = dL/d of the layer's (normalised) input h, X, t and the
    final g_eproj, g_nproj, g_x, g_v.  ``gw``: the layer's parameter-gradient storage or None."""
    cfg, g, F_, D, lde, N, E, first, G = p.cfg, p.g, p.F, p.D, p.lde, p.N, p.E, lt.first, wb.G
    H, M = cfg.H, cfg.M
    if not first and lt.X_in is None:
        raise RuntimeError("internal: the tape of a general-path layer holds no X_in")
    if first and G > 1:                            # one launch instead of G degree groups: one g_cut slice is written
        wb.g_cut_parts[wb.msg_cut * li + 1:wb.msg_cut * li + G].zero_()   # (never with wide slots: zero_X_in excludes them)
    # (a layer that ran with attention dropout: lt.attn = the dropped weights, lt.attn_soft the softmax's own)
    drop = lt.attn_soft is not None
    call("gn_message_backward_dropout" if drop else "gn_message_backward", ptr(lt.xs), ptr(lt.vs), M * F_, ptr(lt.eproj),
         lde, ptr(lt.attn), *((ptr(lt.attn_soft),) if drop else ()),
         ptr(lt.nproj), 4 * F_, None if first else ptr(lt.X_in), ptr(g.rl), ptr(g.cut), ptr(g.outdeg),
         ptr(wb.gh1), ptr(wb.gX1), ptr(g.rowptr), ptr(g.src), ptr(g.tgt_by_src), ptr(wb.colptr), ptr(wb.perm),
         ptr(wb.g_eproj), ptr(wb.g_s), ptr(wb.g_nproj), 4 * F_, ptr(wb.g_x), ptr(wb.g_v), None if first else ptr(wb.gX2),
         wb.g_rl_parts.data_ptr() + 4 * E * D * wb.msg_rl * li, wb.g_cut_parts.data_ptr() + 4 * E * wb.msg_cut * li,
         None if (MSG_BWD_PAIR and (first or G == 1)) else ptr(wb.ga_parts), E,
         N, F_, H, cfg.lmax_arg_msg_bwd, int(cfg.sep_dir), int(cfg.sep_tensor), cfg.act, p.st)
    # the edge-sized W_e^T product leaves 0.7 of its last tile round idle: the two K-heavy atom-sized products
    # (g_x W_s2, g_v W_v2; 60 us as a launch of their own) ride there; W_n1^T needs their output and follows alone.
    # A zero-X_in layer: the tensor-gate columns of g_eproj, g_x, g_v were not written -- K-prefixes
    ke, kv = p.cols[first]
    g_nproj = wb.g_nproj
    if wb.dt_kcat and lw.Wt is not None:
        # dL/dt stated once: gt_b = gt + [g_eproj | g_pre_t] [We^T | Wt^T]^T, one product over the concatenated K (A2 = g_pre_t
        # has a leading dimension of its own); the message backward above never read the edge update's half
        wdt = derived(lw, ("dtcat", ke), lambda: torch.cat([_T(lw, "We", 0, ke), _T(lw, "Wt")], 1).contiguous())
        dt = dict(A=wb.g_eproj, lda=lde, A2=wb.g_pre_t, lda2=F_, a_seg=ke, W=wdt, C=wb.gt_b, ldc=F_, rows=E, nout=F_,
                  K=ke + F_, res=gt_in)
    else:
        dt = dict(A=wb.g_eproj, lda=lde, W=_T(lw, "We", 0, ke), C=wb.gt_b, ldc=F_, rows=E, nout=F_, K=ke, res=gt_in)
    p.group([dt,
             dict(A=wb.g_x, lda=M * F_, W=_T(lw, "Ws2", 0, kv), C=g_nproj, ldc=4 * F_, rows=N, nout=F_, K=kv, c_off=2 * F_,
                  dgate=lt.nproj, g_off=2 * F_),
             dict(A=wb.g_v, lda=M * F_, W=_T(lw, "Wv2", 0, kv), C=g_nproj, ldc=4 * F_, rows=N, nout=F_, K=kv, c_off=3 * F_,
                  dgate=lt.nproj, g_off=3 * F_),
             # the q | k half of the W_n1^T product needs only the message backward's g_q | g_k: it rides here
             # too and halves the K of the product that has to wait for the two riders above (33 -> 20 us)
             dict(A=g_nproj, lda=4 * F_, W=_T(lw, "Wn1", 0, 2 * F_), C=wb.gh_qk, ldc=F_, rows=N, nout=F_, K=2 * F_, res=wb.gh1)])
    p.gemm(g_nproj, 4 * F_, _T(lw, "Wn1", 2 * F_, 4 * F_), None, wb.gh2, F_, N, F_, 2 * F_, res=wb.gh_qk, a_off=2 * F_)
    if gw is not None:
        _layer_weight_grads_gata(p, gw, lt, wb)


def _layer_weight_grads_gata(p: _Call, gw: LayerWeights, lt: LayerTape, wb: _BackwardWork):
    """dL/d of the GATA projections [W_re; W_rs], W_n1, gamma_s.1, gamma_v.1.  Reads g_eproj, g_nproj, g_x, g_v, final
    at the end of ``_gata_backward`` and overwritten by the next layer's: called there."""
    F_, M, lde, N, E = p.F, p.cfg.M, p.lde, p.N, p.E
    ne, nv = p.cols[lt.first]
    weight_grad_group([
        dict(dY=wb.g_eproj, ldy=lde, A=lt.t_in, lda=F_, dW=gw.We, db=gw.be, rows=E, nout=ne, K=F_),
        dict(dY=wb.g_nproj, ldy=4 * F_, A=lt.h_in, lda=F_, dW=gw.Wn1, db=gw.bn1, rows=N, nout=4 * F_, K=F_),
        dict(dY=wb.g_x, ldy=M * F_, A=lt.nact, lda=4 * F_, a_off=2 * F_, dW=gw.Ws2, db=gw.bs2, rows=N, nout=nv, K=F_),
        dict(dY=wb.g_v, ldy=M * F_, A=lt.nact, lda=4 * F_, a_off=3 * F_, dW=gw.Wv2, db=gw.bv2, rows=N, nout=nv, K=F_)],
        p.cfg.wgrad_mode)
    if lt.first:                                   # a zero-X_in layer: the tensor-gate rows get exactly zero
        for t_, n in ((gw.We, ne), (gw.be, ne), (gw.Ws2, nv), (gw.bs2, nv), (gw.Wv2, nv), (gw.bv2, nv)):
            t_[n:].zero_()


def _init_backward(p: _Call, pw: PackedWeights, z32, tape: Tape, wb: _BackwardWork, new):
    """EdgeInit / NodeInit backward (layers.py:1658-1714): reads gt, gh (adds the EdgeInit part to gh in place), writes
    g_ctx and the node-init slice of dL/dcut.  -> (g_feat [E,2F], gy, gy1: dL/d of NodeInit's LayerNorm output and input)."""
    cfg, g, st, F_, N, E = p.cfg, p.g, p.st, p.F, p.N, p.E
    g_feat = new(E, 2 * F_)
    call("gn_edge_init_backward", ptr(wb.gt), ptr(tape.h0), ptr(tape.feat), 2 * F_, ptr(g.rowptr), ptr(g.src),
         ptr(wb.colptr), ptr(wb.perm), N, F_, ptr(g_feat), ptr(wb.gh), st)
    Fc = cfg.Fc or F_
    gy = new(N, Fc)
    p.gemm(wb.gh, F_, _T(pw, "Wb"), None, gy, Fc, N, Fc, F_)
    gy1 = new(N, Fc)
    call("gn_layernorm_silu_backward", ptr(tape.y_pre), ptr(pw.ln_w), ptr(pw.ln_b), 1e-5, ptr(gy), N, Fc, ptr(gy1), cfg.act, st)
    p.gemm(gy1, Fc, _T(pw, "Wa"), None, wb.g_ctx, 2 * F_, N, 2 * F_, Fc)
    if g.self_images:
        call("gn_node_init_backward_images", ptr(wb.g_ctx), ptr(z32), ptr(tape.feat), 2 * F_, ptr(g.cut), ptr(pw.A_nbr),
             ptr(g.rowptr), ptr(g.src), N, F_, ptr(g.edge_diff), ptr(g_feat),
             wb.g_cut_parts.data_ptr() + 4 * E * wb.init_cut, st)
    else:
        call("gn_node_init_backward", ptr(wb.g_ctx), ptr(z32), ptr(tape.feat), 2 * F_, ptr(g.cut), ptr(pw.A_nbr),
             ptr(g.rowptr), ptr(g.src), N, F_, ptr(g_feat), wb.g_cut_parts.data_ptr() + 4 * E * wb.init_cut, st)
    return g_feat, gy, gy1


def _init_weight_grads(cfg, pw: PackedWeights, gw: PackedWeights, z32, g: Graph, tape: Tape, wb: _BackwardWork, g_feat, gy, gy1, new):
    """dL/d of W_init, NodeInit's two layers and LayerNorm, and the embeddings A_na / A_nbr.  Reads gh, g_ctx and the
    results of ``_init_backward`` (all final by then); nothing after it overwrites them, it just follows."""
    F_, R, N, E, Fc = cfg.F, cfg.R, g.N, g.E, cfg.Fc or cfg.F
    layernorm_param_grad(tape.y_pre, pw.ln_w, pw.ln_b, gy, cfg.act, gw.ln_w, gw.ln_b)
    weight_grad_group([dict(dY=wb.gh, ldy=F_, A=tape.y, lda=Fc, dW=gw.Wb, db=gw.bb, rows=N, nout=F_, K=Fc),
                       dict(dY=gy1, ldy=Fc, A=tape.ctx0, lda=2 * F_, dW=gw.Wa, db=gw.ba, rows=N, nout=Fc, K=2 * F_),
                       dict(dY=g_feat, ldy=2 * F_, A=g.phi, lda=R, dW=gw.Winit, db=gw.binit, rows=E, nout=2 * F_, K=R)],
                      cfg.wgrad_mode)
    # species order of the atoms (integer plumbing): a stable argsort of z and the first sorted position of each species
    n_sp = pw.A_na.shape[0]
    zs, order = torch.sort(z32.long(), stable=True)
    sp_ptr = torch.searchsorted(zs, torch.arange(n_sp + 1, device=zs.device)).to(torch.int32)
    order = order.to(torch.int32)
    per_src = new(N, F_)                           # per-source sums of the A_nbr gradient (named: alive until the launch)
    if g.self_images:
        call("gn_embedding_grad_images", ptr(wb.g_ctx), ptr(tape.feat), 2 * F_, ptr(g.cut), ptr(g.dst), ptr(wb.colptr),
             ptr(wb.perm), ptr(order), ptr(sp_ptr), n_sp, N, F_, ptr(g.edge_diff), ptr(per_src), ptr(gw.A_na), ptr(gw.A_nbr),
             _stream())
    else:
        call("gn_embedding_grad", ptr(wb.g_ctx), ptr(tape.feat), 2 * F_, ptr(g.cut), ptr(g.dst), ptr(wb.colptr), ptr(wb.perm),
             ptr(order), ptr(sp_ptr), n_sp, N, F_, ptr(per_src), ptr(gw.A_na), ptr(gw.A_nbr), _stream())


def backward(cfg: Config, pw: PackedWeights, z32: torch.Tensor, g: Graph, tape: Tape,
             gh: torch.Tensor, gX: Optional[torch.Tensor], trace: Optional[list] = None,
             pgrads: Optional[PackedWeights] = None, geometry: bool = True):
    """Input-gradients of ``forward``: given dL/dh [N,F] and dL/dX [N,D,F] (or None = 0)
    returns (g_edge_vec [E,3], g_edge_diff [E]) in the CSR edge order of ``g``.

    ``pgrads`` (storage from ``empty_grads``; the tape of a ``pgrads`` forward): also writes dL/d of every packed weight
    into it.  ``geometry=False`` skips the edge-geometry backward (no position gradient wanted) and returns (None, None).

    ``trace`` (tests only) collects clones of the adjoints at every stage boundary, in the model's real channel layout, as
    dicts with a ``stage`` key: "layer" (dL/d of layer ``layer``'s output h, X, t; zeros where no gradient flows),
    "message" (dL/d of its message stage's output h, X: what EQFF and HTR read), "norm" (dL/d of its normalised inputs,
    with layernorm / steerable_norm only) and "init" (dL/dh0, dL/dt0, dL/dphi, dL/dX of the initial zero X, dL/d edge_vec,
    dL/d edge_diff).  An adjoint the backward never computes (dL/dX_in of a zero-X_in layer) is recorded as None."""
    snap = None
    if trace is not None:
        def snap(stage, li, **ts):
            sel = lambda k, v: (v.clone() if pw.emb_idx is None or k in ("phi", "vec", "diff") else
                                v.index_select(v.dim() - 1, pw.emb_idx))
            trace.append(dict(stage=stage, layer=li, **{k: None if v is None else sel(k, v) for k, v in ts.items()}))
    F_, R, D, N, E = cfg.F, cfg.R, cfg.D, g.N, g.E
    p = _Call(cfg, g, explicit_blocks=True)
    f32 = dict(dtype=torch.float32, device=z32.device)
    new = lambda *shape: torch.empty(shape, **f32)
    check_backward_supported(cfg)
    if pgrads is not None:
        check_param_grads_supported(cfg)
        if cfg.fuse_eqff is not False or tape.ctx0 is None:
            raise ValueError("internal: parameter gradients need the tape of a parameter-gradient forward")
    eq_fused = eqff_fused_ok(cfg, N)
    wb = _backward_work(cfg, pw, g, f32, gh, gX, eq_fused)
    gh_caller, gX_caller = wb.gh, wb.gX            # read-only: never enter the work-buffer rotation below

    for li in reversed(range(len(pw.layers))):
        lw, lt = pw.layers[li], tape.layers[li]
        gw = pgrads.layers[li] if pgrads is not None else None
        if snap is not None:
            snap("layer", li, h=wb.gh, X=wb.gX if wb.gX is not None else torch.zeros((N, D, F_), **f32),
                 t=wb.gt if wb.gt is not None else torch.zeros((E, F_), **f32))
        gt_in = _eqff_htr_backward(p, lw, lt, wb, li, eq_fused, gw)
        if snap is not None:
            snap("message", li, h=wb.gh1, X=wb.gX1)
        _gata_backward(p, lw, lt, wb, li, gt_in, gw)
        # the layer's input adjoints become the current ones; the caller's tensors leave the rotation
        wb.gh, wb.gh2 = wb.gh2, wb.gh
        wb.gX, wb.gX2 = wb.gX2, wb.gX
        if wb.gh2 is gh_caller:
            wb.gh2 = new(N, F_)
        if wb.gX2 is gX_caller:
            wb.gX2 = new(N, D, F_)
        wb.gt, wb.gt_b = wb.gt_b, (wb.gt if wb.gt is not None else new(E, F_))
        if snap is not None and (cfg.layernorm or cfg.steerable_norm):
            snap("norm", li, h=wb.gh, X=None if lt.first else wb.gX)
        # ---- optional input norms (gotennet.py:397-398): back to the un-normalised h / X
        if cfg.layernorm:
            if gw is not None:                     # gh: dL/d of the normalised h
                layernorm_param_grad(lt.h_raw, lw.ln_w, lw.ln_b, wb.gh, _lib.ACT_NONE, gw.ln_w, gw.ln_b)
            _norm_h_backward(lw, lt.h_raw, wb.gh, wb.gh2, pw.emb_idx)
            wb.gh, wb.gh2 = wb.gh2, wb.gh
        if cfg.steerable_norm:
            _norm_X_backward(lw, lt.X_raw, wb.gX, wb.gX2, cfg.lmax, pw.emb_idx)
            wb.gX, wb.gX2 = wb.gX2, wb.gX

    g_feat, gy, gy1 = _init_backward(p, pw, z32, tape, wb, new)
    if pgrads is not None:
        _init_weight_grads(cfg, pw, pgrads, z32, g, tape, wb, g_feat, gy, gy1, new)
        if not geometry:
            return None, None
    g_phi = new(E, R)
    p.gemm(g_feat, 2 * F_, _T(pw, "Winit"), None, g_phi, R, E, R, 2 * F_)
    g_vec, g_diff = new(E, 3), new(E)
    call("gn_edge_geometry_backward_images" if g.self_images else "gn_edge_geometry_backward", ptr(g.edge_vec), ptr(g.edge_diff), ptr(g.src), ptr(g.dst), E, cfg.lmax, R,
         cfg.basis, ptr(pw.rb0), ptr(pw.rb1), float(cfg.cutoff), ptr(wb.g_rl_parts), wb.n_rl, ptr(wb.g_cut_parts), wb.n_cut,
         ptr(g_phi), ptr(g_vec), ptr(g_diff), p.st)
    if snap is not None:
        snap("init", -1, h=wb.gh, t=wb.gt, phi=g_phi, X=None if tape.layers and tape.layers[0].first else wb.gX, vec=g_vec,
             diff=g_diff)
    return g_vec, g_diff


def pos_gradient(g: Graph, g_vec: torch.Tensor, g_diff: torch.Tensor, sign: float = 1.0) -> torch.Tensor:
    """sign * dL/dpos for edge_vec = pos[j] - pos[i], edge_diff = |edge_vec| (Distance, layers.py:1593-1600)."""
    colptr, perm = g.csc()
    out = torch.empty((g.N, 3), dtype=torch.float32, device=g_vec.device)
    call("gn_pos_scatter", ptr(g_vec), ptr(g_diff), ptr(g.edge_vec), ptr(g.rowptr), ptr(colptr), ptr(perm),
         g.N, float(sign), ptr(out), _stream())
    return out


def virial(g: Graph, g_vec: torch.Tensor, g_diff: torch.Tensor, mol_ptr: torch.Tensor, n_mol: int,
           volume: torch.Tensor) -> torch.Tensor:
    """[n_mol, 3, 3]: (1 / volume[m]) sum_{e in box m} r_e (x) dE/dr_e, dE/dr_e = g_vec + g_diff r / |r| = (1/V) dE/d(strain)
    (ASE's sign), as computed -- not symmetrised (gn_virial: fixed-order sums, bit-reproducible; an empty box gives zeros)."""
    out = torch.empty((n_mol, 3, 3), dtype=torch.float32, device=g.rowptr.device)
    call("gn_virial", ptr(g_vec), ptr(g_diff), ptr(g.edge_vec), ptr(g.rowptr), ptr(mol_ptr), n_mol, ptr(volume), ptr(out),
         _stream())
    return out
