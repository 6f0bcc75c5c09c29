"""Read-out heads on the MI355X path: Atomwise (energy / forces), Dipole, ElectronicSpatialExtentV2.

``Atomwise`` mirrors the reference head (gotennet/models/components/outputs.py:
323-376, with SchnetMLP layers.py:225-273) for its default shape on this path:
two Dense layers with SiLU, sum aggregation, optional mean/stddev/atomref and
``derivative`` (forces = -dE/dpos).  Parameters keep the reference's state_dict
keys (``out_net.1.out_net.{0,1}.{weight,bias}``, ``standardize.{mean,stddev}``,
``atomref.weight``).  The arithmetic runs in libgotennet_hip.so
(gn_gemm + gn_head_energy; gn_head_grad for the derivative).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import engine
from ._lib import GotenNetHipError, call, ptr
from .layers import Dense, activation_kind, resolve_activation, shifted_softplus


class _Identity(nn.Module):
    """Placeholder for the reference's ``GetItem('representation')`` at out_net.0 (no parameters)."""


class SchnetMLP(nn.Module):
    """Reference layers.py:225-273: ``n_layers - 1`` activated Dense layers and a linear output layer; ``n_hidden`` an
    int (every hidden layer), a list, or None (pyramid: each layer half the width of the one before)."""

    def __init__(self, n_in, n_out, n_hidden=None, n_layers=2, activation=shifted_softplus):
        super().__init__()
        if n_layers < 1:
            raise ValueError("n_layers >= 1")
        if n_hidden is None:
            neurons, c = [], n_in
            for _ in range(n_layers):
                neurons.append(c)
                c = c // 2
            neurons.append(n_out)
        else:
            hidden = [n_hidden] * (n_layers - 1) if isinstance(n_hidden, int) else list(n_hidden)
            neurons = [n_in] + hidden + [n_out]
        self.n_neurons = neurons
        layers = [Dense(neurons[i], neurons[i + 1], activation=activation) for i in range(n_layers - 1)]
        layers.append(Dense(neurons[-2], neurons[-1], activation=None))
        self.out_net = nn.Sequential(*layers)


class ScaleShift(nn.Module):
    def __init__(self, mean, stddev):
        super().__init__()
        self.register_buffer("mean", torch.as_tensor(mean, dtype=torch.float32).reshape(-1))
        self.register_buffer("stddev", torch.as_tensor(stddev, dtype=torch.float32).reshape(-1))


def molecule_ptr(batch: torch.Tensor, n_mol: int) -> torch.Tensor:
    """int32 [n_mol+1] offsets of each molecule in the batch vector -- index plumbing.  Precondition: ``batch`` is
    non-decreasing (each molecule's atoms contiguous: what a PyG ``Batch`` carries and ``radius_graph(batch=batch)`` assumes).
    An unsorted vector gives wrong per-molecule sums (in-bounds by construction, gn_graph.hip); ``EnergyForces(check_edges=True)``
    validates it."""
    out = torch.empty(n_mol + 1, dtype=torch.int32, device=batch.device)
    if batch.is_cuda and batch.dtype == torch.int64:           # one launch, no host read (torch.bincount synchronises)
        call("gn_molecule_ptr", ptr(batch.contiguous()), batch.shape[0], n_mol, ptr(out), engine._stream())
        return out
    cnt = torch.zeros(n_mol, dtype=torch.int32, device=batch.device)
    cnt.index_add_(0, batch, torch.ones_like(batch, dtype=torch.int32))
    out[0] = 0
    out[1:] = torch.cumsum(cnt, 0)
    return out


class Atomwise(nn.Module):
    def __init__(self, n_in: int, n_out: int = 1, aggregation_mode: Optional[str] = "sum", n_layers: int = 2,
                 n_hidden: Optional[int] = None, activation=shifted_softplus, property: str = "y",
                 contributions: Optional[str] = None, derivative: Optional[str] = None, negative_dr: bool = True,
                 create_graph: bool = True, mean=None, stddev=None, atomref=None, outnet=None,
                 return_vector: Optional[str] = None, standardize: bool = True):
        super().__init__()
        if n_out < 1 or outnet is not None or return_vector:
            raise NotImplementedError("accelerated Atomwise: the default out_net (SchnetMLP), no return_vector")
        #: ``n_out`` properties per atom (reference outputs.py:241, SchnetMLP(n_in, n_out, ...)): the last layer has n_out rows;
        #: each is one gn_head_energy launch on the shared hidden activations, the derivative is that of the SUM of the outputs
        #: (``grad_outputs=torch.ones_like(y)``, outputs.py:365-375)
        self.n_out = int(n_out)
        if aggregation_mode not in ("sum", "add", "mean", None):
            raise NotImplementedError(f"aggregation_mode={aggregation_mode!r}: 'sum', 'mean' or None on the accelerated path")
        self.aggregation_mode = aggregation_mode
        self.act_kind = activation_kind(activation)      # (reference default: shifted_softplus, outputs.py:246)
        activation = resolve_activation(activation)
        self.property, self.contributions, self.derivative = property, contributions, derivative
        self.negative_dr = negative_dr
        self.out_net = nn.Sequential(_Identity(), SchnetMLP(n_in, n_out, n_hidden, n_layers, activation))
        mean = torch.zeros(1) if mean is None else mean
        stddev = torch.ones(1) if stddev is None else stddev
        self.standardize = ScaleShift(mean, stddev) if standardize else nn.Identity()
        self.atomref = nn.Embedding.from_pretrained(atomref.type(torch.float32)) if atomref is not None else None
        #: True: with grad mode on and a parameter requiring grad, ``forward`` also returns d loss / d parameter for the
        #: out_net layers (first order; a backward with create_graph=True is refused)
        self.parameter_grads = False
        #: arithmetic of those weight gradients: None = ``engine.WGRAD_MODE`` (the default, "f32"), or "f32" / "f16x2"
        self.wgrad_mode: Optional[str] = None

    # ---- raw (non-autograd) pieces used by the fused pipeline -----------------------
    def invalidate_packed(self):
        """Drop the cached host scalars / transposed weight.  The cache notices updates through autograd's version
        counter and data_ptr; a write through ``param.data`` bumps neither -- call this after such a write."""
        self._cache = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_packed()
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._cache = None
        return out

    def _packed(self):
        """Host copies of the kernel's scalar arguments (a read-back per step would synchronise the stream, and is not
        allowed inside a hipGraph capture) and the transposed hidden-layer weights, rebuilt when any parameter changes."""
        layers = list(self.out_net[1].out_net)
        ts = [t for d in layers for t in (d.weight, d.bias)]
        if isinstance(self.standardize, ScaleShift):
            ts += [self.standardize.stddev, self.standardize.mean]
        key = tuple((t._version, t.data_ptr()) for t in ts)
        c = getattr(self, "_cache", None)
        if c is None or c["key"] != key:
            scale, shift = 1.0, 0.0
            if isinstance(self.standardize, ScaleShift):
                scale, shift = float(self.standardize.stddev[0]), float(self.standardize.mean[0])
            c = dict(key=key, scale=scale, shift=shift, b2=float(layers[-1].bias.detach().cpu()[0]),
                     w=[d.weight.detach() for d in layers], b=[d.bias.detach() for d in layers],
                     wt=[d.weight.detach().t().contiguous() for d in layers[:-1]])
            if getattr(self, "n_out", 1) > 1:        # per-output host scalars and weight rows (n_out launches share the hidden layers)
                n_out = self.n_out
                per = lambda t: [float(v) for v in t.detach().reshape(-1).cpu().expand(n_out).tolist()]
                sc_l, sh_l = [1.0] * n_out, [0.0] * n_out
                if isinstance(self.standardize, ScaleShift):
                    sc_l, sh_l = per(self.standardize.stddev), per(self.standardize.mean)
                w_last = layers[-1].weight.detach()
                c.update(scales=sc_l, shifts=sh_l, b2s=[float(v) for v in layers[-1].bias.detach().cpu().tolist()],
                         w_rows=[w_last[o].contiguous() for o in range(n_out)],
                         # d(sum of the outputs)/d(last hidden activation): sum_o stddev_o W_o
                         w_sum=(w_last * torch.tensor(sc_l, dtype=w_last.dtype, device=w_last.device).unsqueeze(1)).sum(0).contiguous(),
                         atomref_cols=([self.atomref.weight.detach()[:, o].contiguous() for o in range(n_out)]
                                       if self.atomref is not None else None))
            self._cache = c
        return layers, c

    def _weights(self):
        _, c = self._packed()
        return c["scale"], c["shift"]

    def energy_raw(self, h: torch.Tensor, z32: torch.Tensor, mol_ptr: torch.Tensor, n_mol: int, raw: bool = False,
                   mode: Optional[str] = None, acts: Optional[list] = None):
        """-> (energy [n_mol,1] (sum or mean over the molecule's atoms), y [N] per-atom contributions, tape).
        ``tape`` (pre-activations of the hidden layers + the aggregation's per-atom weights) goes to ``grad_h_raw``.
        ``raw``: y = the MLP output itself (no standardisation, no atomref) -- what ElectronicSpatialExtentV2 reads.
        ``acts``: a list that receives the activated output of every hidden layer (the parameter gradients read them)."""
        layers, c = self._packed()
        N = h.shape[0]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=h.device)
        x, pres = h, []
        hidden = layers[:-1]
        for k, d in enumerate(hidden):
            pre = new(N, d.out_features)
            if k + 1 < len(hidden):                  # activated output feeds the next layer; the pre-activation is kept
                xa = new(N, d.out_features)
                engine.gemm(x, d.in_features, c["w"][k], c["b"][k], xa, d.out_features, N, d.out_features, d.in_features,
                            act=(0, d.out_features), pre_out=pre, kind=self.act_kind, mode=mode)
                x = xa
            elif acts is not None:                   # ... and its activated copy for the last layer's weight gradient
                xa = new(N, d.out_features)
                engine.gemm(x, d.in_features, c["w"][k], c["b"][k], xa, d.out_features, N, d.out_features, d.in_features,
                            act=(0, d.out_features), pre_out=pre, kind=self.act_kind, mode=mode)
            else:                                    # last hidden layer: gn_head_energy applies the activation itself
                engine.gemm(x, d.in_features, c["w"][k], c["b"][k], pre, d.out_features, N, d.out_features, d.in_features,
                            kind=self.act_kind, mode=mode)
            if acts is not None:
                acts.append(xa)
            pres.append(pre)
        last_in = pres[-1] if pres else h.contiguous()
        act = self.act_kind if pres else 11          # GN_ACT_NONE: n_layers = 1, y = W h + b
        mean = self.aggregation_mode == "mean"
        atom_scale = new(N) if mean else None
        if getattr(self, "n_out", 1) > 1:
            # n_out properties: one launch per output row of the last layer on the shared hidden activations
            n_out = self.n_out
            y_t, e_t = new(n_out, N), new(n_out, n_mol)
            for o in range(n_out):
                call("gn_head_energy", ptr(last_in), ptr(c["w_rows"][o]), c["b2s"][o], 1.0 if raw else c["scales"][o],
                     0.0 if raw else c["shifts"][o], 0.0,
                     ptr(c["atomref_cols"][o]) if (c["atomref_cols"] is not None and not raw) else None, ptr(z32), ptr(mol_ptr),
                     n_mol, last_in.shape[1], ptr(y_t[o]), ptr(e_t[o]), int(mean), ptr(atom_scale), act, engine._stream())
            return e_t.t().contiguous(), y_t.t().contiguous(), (pres, last_in, atom_scale)
        y, e = new(N), new(n_mol, 1)
        call("gn_head_energy", ptr(last_in), ptr(c["w"][-1]), c["b2"], 1.0 if raw else c["scale"], 0.0 if raw else c["shift"],
             0.0 if raw else c.get("mol_shift", 0.0),
             ptr(self.atomref.weight.detach()) if (self.atomref is not None and not raw) else None, ptr(z32), ptr(mol_ptr),
             n_mol, last_in.shape[1], ptr(y), ptr(e), int(mean), ptr(atom_scale), act, engine._stream())
        return e, y, (pres, last_in, atom_scale)

    def grad_h_raw(self, tape, Fd: int, mode: Optional[str] = None, upstream: Optional[torch.Tensor] = None) -> torch.Tensor:
        """d(sum over molecules AND outputs of the aggregated property)/dh [N,F].  ``upstream`` [N, n_out] (n_out > 1 only): a
        per-atom, per-output weight of that sum (an autograd caller's ``grad_output`` spread to the atoms)."""
        layers, c = self._packed()
        pres, last_in, atom_scale = tape
        N, Hd = last_in.shape
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=last_in.device)
        g = new(N, Hd)
        act_last = self.act_kind if pres else 11
        if getattr(self, "n_out", 1) > 1 and upstream is not None:
            # sum_o upstream[n, o] stddev_o W_o act'(.): one launch per output with a per-atom scale, summed (linear from here on)
            part = new(N, Hd)
            for o in range(self.n_out):
                a_o = upstream[:, o].contiguous() if atom_scale is None else (upstream[:, o] * atom_scale).contiguous()
                call("gn_head_grad", ptr(last_in), ptr(c["w_rows"][o]), c["scales"][o], ptr(a_o), N, Hd,
                     ptr(g if o == 0 else part), act_last, engine._stream())
                if o:
                    g.add_(part)
        elif getattr(self, "n_out", 1) > 1:
            call("gn_head_grad", ptr(last_in), ptr(c["w_sum"]), 1.0, ptr(atom_scale), N, Hd, ptr(g), act_last, engine._stream())
        else:
            call("gn_head_grad", ptr(last_in), ptr(c["w"][-1]), c["scale"], ptr(atom_scale), N, Hd, ptr(g),
                 act_last, engine._stream())
        for k in range(len(pres) - 1, -1, -1):       # g is d/d(pre_k); through layer k's weight, then act'(pre_{k-1})
            d = layers[k]
            gi = new(N, d.in_features)
            engine.gemm(g, d.out_features, c["wt"][k], None, gi, d.in_features, N, d.in_features, d.out_features,
                        dgate=pres[k - 1] if k > 0 else None, kind=self.act_kind, mode=mode)
            g = gi
        return g

    def _per_atom_property(self, e: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """aggregation_mode=None: the property IS the per-atom contributions."""
        return y.reshape(-1, getattr(self, "n_out", 1)).clone()

    # ---- reference-style call --------------------------------------------------------
    def forward(self, inputs):
        """``inputs`` as in the reference: ``.z, .batch, .pos, .representation``.  With
        ``derivative`` set, ``inputs.pos`` must be the leaf the representation was computed
        from with requires_grad (goten_model.py:580-588)."""
        h = inputs["representation"] if isinstance(inputs, dict) else inputs.representation
        z = inputs["z"] if isinstance(inputs, dict) else inputs.z
        batch = inputs["batch"] if isinstance(inputs, dict) else inputs.batch
        pos = inputs["pos"] if isinstance(inputs, dict) else inputs.pos
        if not h.is_cuda:
            raise GotenNetHipError("gotennet_amd.outputs.Atomwise runs on a ROCm device only")
        n_mol = int(batch[-1].item()) + 1 if batch.numel() else 0
        params = list(self.parameters()) if (self.parameter_grads and torch.is_grad_enabled()) else []
        if any(p.requires_grad for p in params):
            y = _AtomwiseParamFn.apply(h, self, z.to(torch.int32), molecule_ptr(batch, n_mol), n_mol, *params)
        else:
            y = _AtomwiseFn.apply(h, self, z.to(torch.int32), molecule_ptr(batch, n_mol), n_mol)
        result = {self.property: y}                  # [n_mol,1], or the per-atom values [N,1] for aggregation_mode=None
        if self.contributions:
            result[self.contributions] = self._last_y.reshape(-1, getattr(self, "n_out", 1))
        if self.derivative:
            sign = -1.0 if self.negative_dr else 1.0
            from .gotennet import positions_only
            with positions_only(y):                  # parameter-gradient Functions on the way compute dL/dpos only
                (dy,) = torch.autograd.grad(outputs=y, inputs=[pos], grad_outputs=torch.ones_like(y), retain_graph=True)
            result[self.derivative] = sign * dy
        return result


class AtomwiseV3(Atomwise):
    """Reference ``AtomwiseV3`` (outputs.py:96-229) for ``n_out = 1`` with the default ``out_net``: like ``Atomwise`` but the
    per-atom values are only SCALED (``y_i = MLP(h_i) * stddev [+ atomref]``) and ``mean`` is added AFTER the aggregation
    (``y = agg(y_i) + mean``; with ``aggregation_mode=None`` per atom), and -- as in the reference -- the arithmetic reads the
    constructor's ``mean`` / ``stddev`` ATTRIBUTES, not the ``standardize`` buffers it also registers (those only carry
    the ``state_dict`` keys).  Same kernels: ``gn_head_energy`` with ``shift = 0`` and ``mol_shift = mean``."""

    def __init__(self, n_in: int, n_out: int = 1, aggregation_mode: Optional[str] = "sum", n_layers: int = 2,
                 n_hidden: Optional[int] = None, activation=shifted_softplus, property: str = "y",
                 contributions: Optional[str] = None, derivative: Optional[str] = None, negative_dr: bool = True,
                 create_graph: bool = True, mean=None, stddev=None, atomref=None, outnet=None,
                 return_vector: Optional[str] = None, standardize: bool = True):
        if n_out != 1:
            raise NotImplementedError("accelerated AtomwiseV3: n_out=1")
        mean = 0.0 if mean is None else mean
        stddev = 1.0 if stddev is None else stddev
        as_t = lambda v: v if isinstance(v, torch.Tensor) else torch.tensor([float(v)])
        super().__init__(n_in, n_out, aggregation_mode, n_layers, n_hidden, activation, property, contributions,
                         derivative, negative_dr, create_graph, as_t(mean), as_t(stddev), atomref, outnet, return_vector,
                         standardize)
        self.mean, self.stddev = mean, stddev

    def _packed(self):
        layers, c = super()._packed()
        f = lambda v: float(v.reshape(-1)[0]) if isinstance(v, torch.Tensor) else float(v)
        c = dict(c, scale=f(self.stddev), shift=0.0, mol_shift=f(self.mean))
        return layers, c

    def energy_raw(self, h, z32, mol_ptr, n_mol, raw: bool = False, mode: Optional[str] = None,
                   acts: Optional[list] = None):
        if self.aggregation_mode is None and not raw:        # y_n + mean per atom: every atom is its own segment
            N = h.shape[0]
            mol_ptr, n_mol = torch.arange(N + 1, dtype=torch.int32, device=h.device), N
        return super().energy_raw(h, z32, mol_ptr, n_mol, raw=raw, mode=mode, acts=acts)

    def _per_atom_property(self, e, y):
        return e.reshape(-1, 1)


class _AtomwiseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, head, z32, mol_ptr, n_mol):
        e, y, tape = head.energy_raw(h.detach().contiguous(), z32, mol_ptr, n_mol)
        head._last_y = y
        ctx.head, ctx.mol_ptr, ctx.n_mol, ctx.F, ctx.tape = head, mol_ptr, n_mol, h.shape[1], tape
        return head._per_atom_property(e, y) if head.aggregation_mode is None else e

    @staticmethod
    def backward(ctx, ge):
        if getattr(ctx.head, "n_out", 1) > 1:        # [n_mol or N, n_out] upstream: per-atom, per-output weights of the sum
            ge = ge.reshape(-1, ctx.head.n_out).to(torch.float32)
            if ctx.head.aggregation_mode is not None:
                mp = ctx.mol_ptr.long()
                ge = torch.repeat_interleave(ge, mp[1:] - mp[:-1], dim=0)
            return ctx.head.grad_h_raw(ctx.tape, ctx.F, upstream=ge.contiguous()), None, None, None, None
        gh = ctx.head.grad_h_raw(ctx.tape, ctx.F)
        if ctx.head.aggregation_mode is None:        # per-atom outputs: upstream gradient per atom
            return gh * ge.reshape(-1, 1), None, None, None, None
        # per-molecule upstream gradient (ones for energies -> forces): row scale by ge[molecule]
        mp = ctx.mol_ptr.long()
        per_atom = torch.repeat_interleave(ge.reshape(-1), mp[1:] - mp[:-1])
        return gh * per_atom.unsqueeze(1), None, None, None, None


class _AtomwiseParamFn(torch.autograd.Function):
    """h, *parameters -> the head's property, with parameter gradients (``Atomwise.parameter_grads``).  With u the per-atom
    upstream gradient of output o (for aggregation_mode="mean" including the mean's 1 / n) and a_k the activated output
    of hidden layer k (a_-1 = h): dW_last[o] = sum_i u_i^o scale_o a_last(i), and every earlier layer takes
    dW_k = g_k^T a_(k-1), db_k = sum_i g_k with g_k = dL/d pre_k."""

    @staticmethod
    def forward(ctx, h, head, z32, mol_ptr, n_mol, *params):
        acts = []
        ctx.gn_param_fn, ctx.gn_positions_only = True, False
        hd = h.detach().contiguous()
        layers, c = head._packed()
        e, y, tape = head.energy_raw(hd, z32, mol_ptr, n_mol, acts=acts)
        head._last_y = y
        ctx.state = (head, mol_ptr, hd, tape, acts, layers, c, params)
        return head._per_atom_property(e, y) if head.aggregation_mode is None else e

    @staticmethod
    def backward(ctx, ge):
        from .gotennet import refuse_second_order
        refuse_second_order("Atomwise.parameter_grads")
        head, mol_ptr, h, tape, acts, layers, c, params = ctx.state
        _, last_in, atom_scale = tape
        n_out = getattr(head, "n_out", 1)
        u = ge.reshape(-1, n_out).to(torch.float32)
        if head.aggregation_mode is not None and u.shape[0] != last_in.shape[0]:
            mp = mol_ptr.long()
            u = torch.repeat_interleave(u, mp[1:] - mp[:-1], dim=0)
        if atom_scale is not None:
            u = u * atom_scale.unsqueeze(1)
        scales = c["scales"] if n_out > 1 else [c["scale"]]
        weights = not ctx.gn_positions_only          # False inside positions_only(): dL/dh alone
        g, grads = _out_net_backward(head, h, tape, acts, layers, c, u, scales, weights)
        pg = [grads.get(id(p)) if (weights and ctx.needs_input_grad[5 + i]) else None for i, p in enumerate(params)]
        return (g if ctx.needs_input_grad[0] else None, None, None, None, None, *pg)


def _out_net_backward(head, h, tape, acts, layers, c, u, scales, weights: bool = True):
    """Backward of the head's out_net (SchnetMLP) from the per-atom upstream gradient ``u`` [N, n_out] of its RAW outputs
    times ``scales`` -> (dL/dh, {id(parameter): gradient}); the dict is empty without ``weights``.  Shared by
    ``_AtomwiseParamFn`` and ``_ESEParamFn``."""
    pres, last_in, _ = tape
    N, Hd = last_in.shape
    n_out = getattr(head, "n_out", 1)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=h.device)
    U = (u * torch.tensor(scales, dtype=torch.float32, device=h.device)).contiguous()
    grads = {id(d.weight): torch.empty_like(d.weight) for d in layers}
    grads.update({id(d.bias): torch.empty_like(d.bias) for d in layers})
    a_last = acts[-1] if acts else h
    probs = [dict(dY=U, ldy=n_out, A=a_last, lda=Hd, dW=grads[id(layers[-1].weight)], db=grads[id(layers[-1].bias)],
                  rows=N, nout=n_out, K=Hd)]
    # g = dL/d pre_last (dL/dh without hidden layers): sum_o u^o scale_o W_o act'(pre_last)
    act_last = head.act_kind if pres else 11
    g, part = new(N, Hd), new(N, Hd)
    for o in range(n_out):
        w_o = c["w_rows"][o] if n_out > 1 else c["w"][-1]
        call("gn_head_grad", ptr(last_in), ptr(w_o), scales[o], ptr(u[:, o].contiguous()), N, Hd,
             ptr(g if o == 0 else part), act_last, engine._stream())
        if o:
            g.add_(part)
    for k in range(len(pres) - 1, -1, -1):       # g = dL/d pre_k
        d = layers[k]
        probs.append(dict(dY=g, ldy=d.out_features, A=acts[k - 1] if k > 0 else h, lda=d.in_features,
                          dW=grads[id(d.weight)], db=grads[id(d.bias)], rows=N, nout=d.out_features, K=d.in_features))
        gi = new(N, d.in_features)
        engine.gemm(g, d.out_features, c["wt"][k], None, gi, d.in_features, N, d.in_features, d.out_features,
                    dgate=pres[k - 1] if k > 0 else None, kind=head.act_kind)
        g = gi
    if not weights:
        return g, {}
    engine.weight_grad_group(probs, getattr(head, "wgrad_mode", None))
    return g, grads


# ---------------------------------------------------------------------------------------------------------------------
# vector-representation read-outs of the QM9 task (reference models/tasks/QM9Task.py:168-187)
def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


class GatedEquivariantBlock(nn.Module):
    """Reference outputs.py:24-93 (state_dict keys ``mix_vectors.weight``, ``scalar_net.{0,1}.{weight,bias}``).
    ``forward(scalars [N, n_sin], vectors [N, 3, n_vin]) -> (s_out [N, n_sout], v_out [N, 3, n_vout])``; ``vectors`` may be
    the ``X[:, :3, :]`` view of the [N, D, F] vector representation (its gradient then has exact zeros in rows 3 and above).
    ``parameter_grads = True`` makes the block trainable (first order)."""

    def __init__(self, n_sin: int, n_vin: int, n_sout: int, n_vout: int, n_hidden: int, activation=F.silu,
                 sactivation=None):
        super().__init__()
        if n_vin % 4 or n_hidden % 4:
            raise NotImplementedError("GatedEquivariantBlock: n_vin and n_hidden must be multiples of 4 on the HIP path")
        self.n_sin, self.n_vin, self.n_sout, self.n_vout, self.n_hidden = n_sin, n_vin, n_sout, n_vout, n_hidden
        self.act_kind = activation_kind(activation)
        self.sact_kind = activation_kind(sactivation) if sactivation is not None else -1
        self.mix_vectors = Dense(n_vin, 2 * n_vout, activation=None, bias=False)
        self.scalar_net = nn.Sequential(Dense(n_sin + n_vout, n_hidden, activation=resolve_activation(activation)),
                                        Dense(n_hidden, n_sout + n_vout, activation=None))
        self.sactivation = resolve_activation(sactivation) if sactivation is not None else None
        #: True: with grad mode on and an input or parameter requiring grad, ``forward`` is differentiable (first order):
        #: dL/dscalars, dL/dvectors and d loss / d parameter; a backward with create_graph=True is refused
        self.parameter_grads = False
        #: arithmetic of the weight gradients: None = ``engine.WGRAD_MODE`` (the default, "f32"), or "f32" / "f16x2"
        self.wgrad_mode: Optional[str] = None

    def invalidate_packed(self):
        self._cache = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._cache = None
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._cache = None
        return out

    def _packed(self):
        """Weights padded to the GEMM's multiples of four (zero rows / columns): V block at column 0 and W block at column
        pad4(n_vout) of the mixing product; ctx columns and output rows padded likewise."""
        ts = [self.mix_vectors.weight, self.scalar_net[0].weight, self.scalar_net[0].bias,
              self.scalar_net[1].weight, self.scalar_net[1].bias]
        key = tuple((t._version, t.data_ptr()) for t in ts)
        c = getattr(self, "_cache", None)
        if c is None or c["key"] != key:
            nv, ns, no, nh = self.n_vout, self.n_sin, self.n_sout, self.n_hidden
            pv, kc, po = _pad4(nv), _pad4(ns + nv), _pad4(no + nv)
            dev = ts[0].device
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            wmix = z(2 * pv, self.n_vin)
            wmix[:nv], wmix[pv:pv + nv] = ts[0].detach()[:nv], ts[0].detach()[nv:]
            w0 = z(nh, kc)
            w0[:, :ns + nv] = ts[1].detach()
            w1, b1 = z(po, nh), z(po)
            w1[:no + nv], b1[:no + nv] = ts[3].detach(), ts[4].detach()
            c = dict(key=key, wmix=wmix, w0=w0, b0=ts[2].detach().contiguous(), w1=w1, b1=b1, pv=pv, kc=kc, po=po)
            self._cache = c
        return c

    def _packed_t(self):
        """``_packed()`` plus the transposed (padded) weights the backward's input-gradient products read."""
        c = self._packed()
        if "w1t" not in c:
            c.update(w1t=c["w1"].t().contiguous(), w0t=c["w0"].t().contiguous(), wmixt=c["wmix"].t().contiguous())
        return c

    def _run(self, c, scalars: torch.Tensor, vectors: torch.Tensor, save: bool = False):
        """The block's launches on detached fp32 inputs -> (s_out, v_out, saved); ``saved`` (``save``: what the backward
        reads, with the hidden layer's pre-activation as one more output of its product) is None otherwise."""
        N = scalars.shape[0]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=scalars.device)
        pv, kc, po, nh = c["pv"], c["kc"], c["po"], self.n_hidden
        vmix, ctx, hid, x = new(N * 3, 2 * pv), new(N, kc), new(N, nh), new(N, po)
        pre0 = new(N, nh) if save else None
        engine.gemm(vectors, self.n_vin, c["wmix"], None, vmix, 2 * pv, N * 3, 2 * pv, self.n_vin, kind=self.act_kind)
        call("gn_geb_context", ptr(scalars), scalars.stride(0), self.n_sin, ptr(vmix), 2 * pv, self.n_vout, N, ptr(ctx), kc,
             engine._stream())
        engine.gemm(ctx, kc, c["w0"], c["b0"], hid, nh, N, nh, kc, act=(0, nh), pre_out=pre0, kind=self.act_kind)
        engine.gemm(hid, nh, c["w1"], c["b1"], x, po, N, po, nh, kind=self.act_kind)
        s_out, v_out = new(N, self.n_sout), new(N, 3, self.n_vout)
        call("gn_geb_gate", ptr(x), po, self.n_sout, self.n_vout, ptr(vmix), 2 * pv, pv, N, self.sact_kind,
             ptr(s_out), self.n_sout, ptr(v_out), self.n_vout, engine._stream())
        return s_out, v_out, ((vectors, vmix, ctx, pre0, hid, x) if save else None)

    def _params(self):
        return [self.mix_vectors.weight, self.scalar_net[0].weight, self.scalar_net[0].bias,
                self.scalar_net[1].weight, self.scalar_net[1].bias]

    def forward(self, scalars: torch.Tensor, vectors: torch.Tensor):
        if not scalars.is_cuda:
            raise GotenNetHipError("gotennet_amd.outputs.GatedEquivariantBlock runs on a ROCm device only")
        if vectors.shape[1] != 3 or vectors.shape[2] != self.n_vin:
            raise ValueError(f"vectors must be [N, 3, {self.n_vin}]")
        if self.parameter_grads and torch.is_grad_enabled():
            params = self._params()
            if scalars.requires_grad or vectors.requires_grad or any(p.requires_grad for p in params):
                return _GatedBlockParamFn.apply(scalars, vectors, self, *params)
        # the X[:, :3, :] view of [N, D, F] is gathered into [N, 3, F] by a device copy (index plumbing: the GEMM's row map
        # addresses input AND output rows, and the mixing product's output is dense)
        vectors = vectors.detach().to(torch.float32).contiguous()
        scalars = scalars.detach().to(torch.float32)
        if scalars.stride(-1) != 1:
            scalars = scalars.contiguous()
        s_out, v_out, _ = self._run(self._packed(), scalars, vectors)
        return s_out, v_out


class _GatedBlockParamFn(torch.autograd.Function):
    """(scalars, vectors, *parameters) -> (s_out, v_out) with parameter gradients (``GatedEquivariantBlock.parameter_grads``).
    With the notation of the forward (vmix = [V | W], ctx = [s | ||V||], pre0 = ctx W0^T + b0, hid = act(pre0),
    x = hid W1^T + b1 = [s_raw | gate]): the gate adjoint gives g_x and the W half of g_vmix; dW1, db1 from (g_x, hid);
    g_pre0 = (g_x W1) act'(pre0); dW0, db0 from (g_pre0, ctx); g_ctx = g_pre0 W0; the context adjoint gives g_scalars and the
    V half of g_vmix; dWmix from (g_vmix, vectors) over the N * 3 rows; g_vectors = g_vmix Wmix."""

    @staticmethod
    def forward(ctx, scalars, vectors, blk, *params):
        vec = vectors.detach().to(torch.float32).contiguous()
        sc = scalars.detach().to(torch.float32)
        if sc.stride(-1) != 1:
            sc = sc.contiguous()
        c = blk._packed_t()
        s_out, v_out, saved = blk._run(c, sc, vec, save=True)
        ctx.state = (blk, c, saved)
        return s_out, v_out

    @staticmethod
    def backward(ctx, g_s_out, g_v_out):
        from .gotennet import refuse_second_order
        refuse_second_order("GatedEquivariantBlock.parameter_grads")
        blk, c, (vec, vmix, cx, pre0, hid, x) = ctx.state
        N = x.shape[0]
        nv, ns, no, nh, nin = blk.n_vout, blk.n_sin, blk.n_sout, blk.n_hidden, blk.n_vin
        pv, kc, po = c["pv"], c["kc"], c["po"]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        g_s_out, g_v_out = g_s_out.to(torch.float32).contiguous(), g_v_out.to(torch.float32).contiguous()
        need = ctx.needs_input_grad
        g_x, g_vmix = new(N, po), new(N * 3, 2 * pv)
        call("gn_geb_gate_backward", ptr(g_s_out), no, ptr(g_v_out), nv, ptr(x), po, no, nv, ptr(vmix), 2 * pv, pv, N,
             blk.sact_kind, ptr(g_x), po, ptr(g_vmix), 2 * pv, engine._stream())
        g_pre0, g_ctx, g_s = new(N, nh), new(N, kc), new(N, ns)
        engine.gemm(g_x, po, c["w1t"], None, g_pre0, nh, N, nh, po, dgate=pre0, kind=blk.act_kind)
        engine.gemm(g_pre0, nh, c["w0t"], None, g_ctx, kc, N, kc, nh, kind=blk.act_kind)
        call("gn_geb_context_backward", ptr(g_ctx), kc, ns, ptr(vmix), 2 * pv, nv, pv, N, ptr(g_s), ns, ptr(g_vmix), 2 * pv,
             engine._stream())
        g_vec = None
        if need[1]:
            g_vec = new(N, 3, nin)
            engine.gemm(g_vmix, 2 * pv, c["wmixt"], None, g_vec, nin, N * 3, nin, 2 * pv, kind=blk.act_kind)
        probs, pg = [], [None] * 5
        if need[3]:                                  # mix_vectors: the V rows, then the W rows
            pg[0] = new(2 * nv, nin)
            probs += [dict(dY=g_vmix, ldy=2 * pv, y_off=off, A=vec, lda=nin, dW=pg[0], w_row=row, rows=N * 3, nout=nv, K=nin)
                      for off, row in ((0, 0), (pv, nv))]
        if need[4] or need[5]:
            pg[1], pg[2] = new(nh, ns + nv), new(nh)
            probs.append(dict(dY=g_pre0, ldy=nh, A=cx, lda=kc, dW=pg[1], db=pg[2], rows=N, nout=nh, K=ns + nv))
        if need[6] or need[7]:
            pg[3], pg[4] = new(no + nv, nh), new(no + nv)
            probs.append(dict(dY=g_x, ldy=po, A=hid, lda=nh, dW=pg[3], db=pg[4], rows=N, nout=no + nv, K=nh))
        engine.weight_grad_group(probs, getattr(blk, "wgrad_mode", None))
        pg = [g if need[3 + i] else None for i, g in enumerate(pg)]
        return (g_s if need[0] else None, g_vec, None, *pg)


def _field(inputs, name):
    return inputs[name] if isinstance(inputs, dict) else getattr(inputs, name)


class Dipole(nn.Module):
    """Reference outputs.py:379-468: two GatedEquivariantBlocks on (h, X[:, :3]) -> atomic dipoles + charges,
    ``y = sum_atoms (mu_n + pos_n q_n)`` per molecule (its norm with ``predict_magnitude``).  ``mean`` / ``stddev`` are
    plain, untrained attributes like in the reference (not in the state_dict).  ``parameter_grads = True`` (forwarded to
    both blocks) trains it: a loss on ``y`` / ``y_vector`` reaches the blocks' parameters and (h, X), first order.  The QM9
    task takes no derivative: ``pos`` is data, and a ``pos`` that requires grad is refused in that mode."""

    def __init__(self, n_in: int, n_hidden: Optional[int] = None, activation=F.silu, property: str = "dipole",
                 predict_magnitude: bool = False, output_v: bool = True, mean=None, stddev=None):
        super().__init__()
        self.stddev, self.mean, self.output_v = stddev, mean, output_v
        n_hidden = n_in if n_hidden is None else n_hidden
        self.property, self.derivative, self.predict_magnitude = property, None, predict_magnitude
        self.equivariant_layers = nn.ModuleList([
            GatedEquivariantBlock(n_sin=n_in, n_vin=n_in, n_sout=n_hidden, n_vout=n_hidden, n_hidden=n_hidden,
                                  activation=activation, sactivation=activation),
            GatedEquivariantBlock(n_sin=n_hidden, n_vin=n_hidden, n_sout=1, n_vout=1, n_hidden=n_hidden,
                                  activation=activation)])
        self.requires_dr = self.requires_stress = False
        self.aggregation_mode = "sum"

    @property
    def parameter_grads(self) -> bool:
        return all(layer.parameter_grads for layer in self.equivariant_layers)

    @parameter_grads.setter
    def parameter_grads(self, on: bool):
        for layer in self.equivariant_layers:
            layer.parameter_grads = bool(on)

    @property
    def wgrad_mode(self) -> Optional[str]:
        """Weight-gradient arithmetic of both blocks (None = ``engine.WGRAD_MODE``); forwarded like ``parameter_grads``."""
        return self.equivariant_layers[0].wgrad_mode

    @wgrad_mode.setter
    def wgrad_mode(self, mode: Optional[str]):
        for layer in self.equivariant_layers:
            layer.wgrad_mode = mode

    def _reduce(self, l1, l0, pos, mp, n_mol):
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=l0.device)
        y = new(n_mol, 1) if self.predict_magnitude else new(n_mol, 3)
        y_vec = new(n_mol, 3, 1) if self.output_v else None
        call("gn_dipole_reduce", ptr(l1), 1, ptr(l0), 1, ptr(pos), ptr(mp), n_mol, *self._standardise(),
             int(self.predict_magnitude), ptr(y), ptr(y_vec), engine._stream())
        return y, y_vec

    def _standardise(self):
        """(scale, shift, standardise) of the charges, as the reduction kernels take them."""
        std = self.stddev is not None
        return (float(self.stddev) if std else 1.0, float(self.mean) if std else 0.0, int(std))

    def forward(self, inputs):
        pos, batch = _field(inputs, "pos"), _field(inputs, "batch")
        l0 = _field(inputs, "representation")
        l1 = _field(inputs, "vector_representation")[:, :3, :]
        train = self.parameter_grads and torch.is_grad_enabled() and (
            l0.requires_grad or l1.requires_grad or any(p.requires_grad for p in self.parameters()))
        if train and pos.requires_grad:              # before any launch
            raise NotImplementedError("Dipole.parameter_grads: `pos` requires grad, but the trained read-out takes no "
                                      "derivative with respect to positions (they are data here); detach them")
        for layer in self.equivariant_layers:
            l0, l1 = layer(l0, l1)
        n_mol = int(batch[-1].item()) + 1 if batch.numel() else 0
        mp = molecule_ptr(batch, n_mol)
        pos = pos.detach().to(torch.float32).contiguous()
        if train:
            y, y_vec = _DipoleReduceFn.apply(l1, l0, self, pos, mp, n_mol)
        else:
            y, y_vec = self._reduce(l1, l0, pos, mp, n_mol)
        result = {self.property: y}
        if self.output_v:
            result[self.property + "_vector"] = y_vec
        return result


class _DipoleReduceFn(torch.autograd.Function):
    """(mu [N, 3, 1], q [N, 1]) -> (y, y_vector): the per-molecule reduction of ``Dipole`` with its adjoint
    (gn_dipole_reduce_backward; the molecule's dipole is recomputed there in the forward's order)."""

    @staticmethod
    def forward(ctx, mu, q, head, pos, mp, n_mol):
        mu, q = mu.detach().contiguous(), q.detach().contiguous()
        y, y_vec = head._reduce(mu, q, pos, mp, n_mol)
        ctx.state = (head, mu, q, pos, mp, n_mol)
        return y, y_vec                              # (y_vec is None without ``output_v``)

    @staticmethod
    def backward(ctx, g_y, g_yvec):
        from .gotennet import refuse_second_order
        refuse_second_order("Dipole.parameter_grads")
        head, mu, q, pos, mp, n_mol = ctx.state
        g_mu, g_q = torch.empty_like(mu), torch.empty_like(q)
        g_y = g_y.to(torch.float32).contiguous()
        g_yvec = g_yvec.to(torch.float32).contiguous() if g_yvec is not None else None
        call("gn_dipole_reduce_backward", ptr(g_y), ptr(g_yvec), ptr(mu), 1, ptr(q), 1, ptr(pos), ptr(mp), n_mol,
             *head._standardise(), int(head.predict_magnitude), ptr(g_mu), 1, ptr(g_q), 1, engine._stream())
        return g_mu, g_q, None, None, None, None


#: standard atomic weights by atomic number (index 0: the dummy element, weight 1, as in ase.data.atomic_masses, which
#: the reference reads at outputs.py:513).  Elements up to Kr are built in; heavier ones come from the ``atomic_mass``
#: argument or from a reference checkpoint (the buffer is part of the state_dict).
_ATOMIC_MASS = [1.0, 1.008, 4.002602, 6.94, 9.0121831, 10.81, 12.011, 14.007, 15.999, 18.998403163, 20.1797,
                22.98976928, 24.305, 26.9815385, 28.085, 30.973761998, 32.06, 35.45, 39.948, 39.0983, 40.078,
                44.955908, 47.867, 50.9415, 51.9961, 54.938044, 55.845, 58.933194, 58.6934, 63.546, 65.38, 69.723,
                72.630, 74.921595, 78.971, 79.904, 83.798]


class ElectronicSpatialExtentV2(Atomwise):
    """Reference outputs.py:471-545: ``y = sum_atoms |pos_n - c|^2 x_n`` with ``x = out_net(h)`` (the raw MLP output:
    the reference does not standardise here) and ``c`` the mass-weighted centroid of the molecule.  ``parameter_grads =
    True`` trains the out_net (first order; ``pos`` is data and must not require grad then); ``contributions`` stay
    detached."""

    def __init__(self, n_in: int, n_layers: int = 2, n_hidden: Optional[int] = None, activation=shifted_softplus,
                 property: str = "y", contributions: Optional[str] = None, mean=None, stddev=None, outnet=None,
                 atomic_mass: Optional[torch.Tensor] = None):
        super().__init__(n_in, 1, "sum", n_layers, n_hidden, activation=activation, mean=mean, stddev=stddev,
                         outnet=outnet, property=property, contributions=contributions)
        if atomic_mass is None:
            atomic_mass = torch.zeros(119)
            atomic_mass[:len(_ATOMIC_MASS)] = torch.tensor(_ATOMIC_MASS)
        self.register_buffer("atomic_mass", torch.as_tensor(atomic_mass, dtype=torch.float32))

    def forward(self, inputs):
        h, z, batch, pos = (_field(inputs, k) for k in ("representation", "z", "batch", "pos"))
        if not h.is_cuda:
            raise GotenNetHipError("gotennet_amd.outputs.ElectronicSpatialExtentV2 runs on a ROCm device only")
        n_mol = int(batch[-1].item()) + 1 if batch.numel() else 0
        if z.numel():
            # the built-in table stops at Kr (the reference reads ase's full table): an element without a mass would
            # silently shift the mass-weighted centroid (and an all-massless molecule divides 0 by 0)
            zc = z.long().clamp(0, self.atomic_mass.numel() - 1)
            if bool(((self.atomic_mass[zc] <= 0) | (z.long() != zc)).any()):
                raise ValueError("ElectronicSpatialExtentV2: an atomic number has no entry in `atomic_mass` (built-in "
                                 "table: Z <= 36); pass atomic_mass= or load a reference checkpoint that carries it")
        params = list(self.parameters()) if (self.parameter_grads and torch.is_grad_enabled()) else []
        train = bool(params) and (h.requires_grad or any(p.requires_grad for p in params))
        if train and pos.requires_grad:              # before any launch
            raise NotImplementedError("ElectronicSpatialExtentV2.parameter_grads: `pos` requires grad, but the trained "
                                      "read-out takes no derivative with respect to positions (they are data here); "
                                      "detach them")
        mp, z32 = molecule_ptr(batch, n_mol), z.to(torch.int32)
        pos = pos.detach().to(torch.float32).contiguous()
        if train:
            y = _ESEParamFn.apply(h, self, z32, mp, n_mol, pos, *params)
            x = self._last_y
        else:
            y, x, _ = self._raw_forward(h.detach().contiguous(), z32, mp, n_mol, pos)
        result = {self.property: y}
        if self.contributions:
            result[self.contributions] = x.reshape(-1, 1)
        return result

    def _raw_forward(self, h, z32, mp, n_mol, pos, acts=None):
        """-> (y [n_mol, 1], x [N] the raw out_net output, the out_net's tape)."""
        _, x, tape = self.energy_raw(h, z32, mp, n_mol, raw=True, acts=acts)
        y = torch.empty((n_mol, 1), dtype=torch.float32, device=h.device)
        call("gn_ese_reduce", ptr(x), ptr(pos), ptr(z32), ptr(self.atomic_mass), self.atomic_mass.numel(), ptr(mp), n_mol,
             ptr(y), engine._stream())
        return y, x, tape


class _ESEParamFn(torch.autograd.Function):
    """h, *parameters -> ``ElectronicSpatialExtentV2``'s property with parameter gradients: gn_ese_reduce_backward spreads
    the molecule's upstream gradient to u_n = g_y[b] |pos_n - c_b|^2, the per-atom gradient of the raw out_net output;
    from there the out_net backward of ``_AtomwiseParamFn`` (scale 1, no atomref, no atom_scale)."""

    @staticmethod
    def forward(ctx, h, head, z32, mol_ptr, n_mol, pos, *params):
        acts = []
        hd = h.detach().contiguous()
        layers, c = head._packed()
        y, x, tape = head._raw_forward(hd, z32, mol_ptr, n_mol, pos, acts=acts)
        head._last_y = x
        ctx.state = (head, z32, mol_ptr, n_mol, pos, hd, tape, acts, layers, c, params)
        return y

    @staticmethod
    def backward(ctx, g_y):
        from .gotennet import refuse_second_order
        refuse_second_order("ElectronicSpatialExtentV2.parameter_grads")
        head, z32, mol_ptr, n_mol, pos, h, tape, acts, layers, c, params = ctx.state
        u = torch.empty((h.shape[0], 1), dtype=torch.float32, device=h.device)
        call("gn_ese_reduce_backward", ptr(g_y.to(torch.float32).contiguous()), ptr(pos), ptr(z32), ptr(head.atomic_mass),
             head.atomic_mass.numel(), ptr(mol_ptr), n_mol, ptr(u), engine._stream())
        g, grads = _out_net_backward(head, h, tape, acts, layers, c, u, [1.0])
        pg = [grads.get(id(p)) if ctx.needs_input_grad[6 + i] else None for i, p in enumerate(params)]
        return (g if ctx.needs_input_grad[0] else None, None, None, None, None, None, *pg)
