"""The SPAI-emitting GNN (``NodeEdgeProcessing``) with a HIP forward pass.

Parameter layout, module names and seeded initialisation follow the reference
(``neural_cg/nn/gnns.py:9-97``, ``neural_cg/nn/basic_layers.py:73-225``,
``neural_cg/utils/weight_init.py``), so ``state_dict()`` keys are the reference's and a
reference checkpoint's ``gnn.*`` tensors load directly.  The modules here are parameter
containers; the forward pass is ``lspcg_gnn_forward`` (csrc/lspcg_gnn.hip) and, with
``differentiable = True``, the parameter gradients come from ``lspcg_gnn_backward``
(csrc/lspcg_gnn_bwd.hip) through ``_GnnFn`` -- there is no torch compute path.

Packed weight blob (fp32, ``pack_weights``), each FeedForward as
``[W1 (16 x in) | b1 | W2 (16 x 16) | b2 | W3 (out x 16) | b3]``::

    node_enc | edge_enc | per MPLayer: [node LN γ,β (16) | node_mlp]
                                      [edge LN γ,β (48) | edge_mlp]
                                      [msg  LN γ,β (48) | msg_mlp ] | edge_dec
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import nn

from . import _lib
from .sparse import Context, _ptr


def _act(name: str):
    table = {"relu": nn.ReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "gelu": nn.GELU, "elu": nn.ELU,
             "leaky_relu": nn.LeakyReLU, "none": nn.Identity}
    return table[name.lower()]()


def _norm(name: str, channels: int):
    n = name.lower()
    if n == "none":
        return nn.Identity()
    if n in ("layer", "layernorm", "layer_norm"):
        return nn.LayerNorm(channels)
    if n in ("batch", "batchnorm", "batch_norm", "rms", "rmsnorm", "rms_norm"):
        return nn.RMSNorm(channels)
    raise ValueError(f"Normalization {name} not supported.")


class FeedForward(nn.Module):
    """Parameters of basic_layers.py:73-109 FeedForward."""

    def __init__(self, in_channels, out_channels, hidden_channels, num_layers, pre_norm="none", activation="gelu",
                 out_activation="none"):
        super().__init__()
        self.pre_norm = _norm(pre_norm, in_channels)
        self.lift = nn.Sequential(nn.Linear(in_channels, hidden_channels), _act(activation))
        self.body = nn.ModuleList()
        for _ in range(1, num_layers):
            self.body.append(nn.Sequential(nn.Linear(hidden_channels, hidden_channels), _act(activation)))
        self.proj = nn.Sequential(nn.Linear(hidden_channels, out_channels), _act(out_activation))
        self.activation = activation
        self.out_activation = out_activation

    def linears(self):
        return [self.lift[0]] + [b[0] for b in self.body] + [self.proj[0]]


class _MessageNormParams(nn.Module):
    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(1), requires_grad=False)

    def reset_parameters(self):
        self.scale.data.fill_(1.0)


class MPLayer(nn.Module):
    """Parameters of basic_layers.py:145-191 MPLayer."""

    def __init__(self, node_channels, edge_channels, node_residual, edge_residual, node_mlp, edge_mlp, msg_mlp,
                 aggr="add", msg_norm=True):
        super().__init__()
        if aggr != "add":
            raise NotImplementedError("only aggr='add' (config/gnn.yaml) is implemented")
        self.node_mlp = FeedForward(in_channels=node_channels, out_channels=node_channels, **node_mlp)
        self.edge_mlp = FeedForward(in_channels=2 * node_channels + edge_channels, out_channels=edge_channels,
                                    **edge_mlp)
        self.msg_mlp = FeedForward(in_channels=edge_channels + 2 * node_channels, out_channels=node_channels,
                                   **msg_mlp)
        self.node_residual = node_residual
        self.edge_residual = edge_residual
        if msg_norm:
            self.node_msg_norm = _MessageNormParams()


def _weight_init(m: nn.Module):
    if hasattr(m, "reset_parameters"):
        m.reset_parameters()


def default_gnn_config(features: int = 16, mlp_layers: int = 2, num_mp_layers: int = 4) -> dict:
    """config/gnn.yaml."""
    ff = lambda norm: {"pre_norm": norm, "hidden_channels": features, "num_layers": mlp_layers}
    return dict(node_encoder=ff("none"), edge_encoder=ff("none"), node_decoder=ff("none"), edge_decoder=ff("none"),
                num_mp_layers=num_mp_layers, node_residual=True, edge_residual=True, node_features=features,
                edge_features=features, node_mlp=ff("layer"), edge_mlp=ff("layer"), msg_mlp=ff("layer"),
                msg_norm=True, aggr="add")


class NodeEdgeProcessing(nn.Module):
    """gnns.py:9-97 -- forward runs on MI355X through ``lspcg_gnn_forward``."""

    def __init__(self, node_in_features, node_out_features, node_encoder, node_decoder, edge_in_features,
                 edge_out_features, edge_encoder, edge_decoder, num_mp_layers, node_features, edge_features,
                 node_residual, edge_residual, node_mlp, edge_mlp, msg_mlp, msg_norm, aggr="add"):
        super().__init__()
        self.node_enc = FeedForward(in_channels=node_in_features, out_channels=node_features, **node_encoder)
        if node_out_features is None:
            self.node_dec = nn.Identity()
        else:
            self.node_dec = FeedForward(in_channels=node_features, out_channels=node_out_features, **node_decoder)
        self.edge_enc = FeedForward(in_channels=edge_in_features, out_channels=edge_features, **edge_encoder)
        self.edge_dec = FeedForward(in_channels=edge_features + 2 * node_features, out_channels=edge_out_features,
                                    **edge_decoder)
        self.mp_layers = nn.ModuleList()
        for _ in range(num_mp_layers):
            self.mp_layers.append(MPLayer(node_features, edge_features, node_residual, edge_residual, node_mlp,
                                          edge_mlp, msg_mlp, aggr=aggr, msg_norm=msg_norm))
        self.apply(_weight_init)
        self.node_in_features = node_in_features
        self.edge_in_features = edge_in_features
        self.edge_out_features = edge_out_features
        self.hidden = node_features
        self.num_mp_layers = num_mp_layers
        self.node_residual = node_residual
        self.edge_residual = edge_residual
        self._check_supported(node_features, edge_features, node_encoder, edge_encoder, edge_decoder, node_mlp,
                              edge_mlp, msg_mlp)
        self._handle = None
        self._ctx = None
        self._packed_version = None
        self.flat = None  # the fp32 device blob all packed parameters are views of (flatten_parameters)
        self._graph = None  # (key, edge_index tensor) of the structure analysed by lspcg_gnn_set_graph
        self.differentiable = False  # True: forward builds the parameters' autograd graph (_GnnFn)

    @staticmethod
    def _check_supported(nf, ef, *ffs):
        if nf != 16 or ef != 16:
            raise NotImplementedError("the HIP GNN kernel is specialised for gnn_features = 16 (config/gnn.yaml)")
        for cfg in ffs:
            if cfg.get("num_layers", 2) != 2 or cfg.get("hidden_channels", 16) != 16:
                raise NotImplementedError("the HIP GNN kernel is specialised for gnn_mlp_layers = 2, hidden = 16")
            if cfg.get("activation", "gelu") != "gelu" or cfg.get("out_activation", "none") != "none":
                raise NotImplementedError("the HIP GNN kernel implements GELU hidden / identity output activations")

    # ---- packing
    def _packed_params(self):
        """``[(state_dict key, parameter)]`` in the order of the packed blob."""
        out = []

        def ff(prefix: str, m: FeedForward):
            for name, lin in [("lift.0", m.lift[0])] + [(f"body.{i}.0", b[0]) for i, b in enumerate(m.body)] + \
                    [("proj.0", m.proj[0])]:
                out.append((f"{prefix}.{name}.weight", lin.weight))
                out.append((f"{prefix}.{name}.bias", lin.bias))

        def ln(prefix: str, m: FeedForward):
            if not isinstance(m.pre_norm, nn.LayerNorm):
                raise NotImplementedError("MPLayer MLPs must use pre_norm 'layer' (config/gnn.yaml)")
            out.append((f"{prefix}.pre_norm.weight", m.pre_norm.weight))
            out.append((f"{prefix}.pre_norm.bias", m.pre_norm.bias))

        for name, enc in (("node_enc", self.node_enc), ("edge_enc", self.edge_enc)):
            if not isinstance(enc.pre_norm, nn.Identity):
                raise NotImplementedError("encoders must use pre_norm 'none' (config/gnn.yaml)")
            ff(name, enc)
        for i, mp in enumerate(self.mp_layers):
            for name, sub in (("node_mlp", mp.node_mlp), ("edge_mlp", mp.edge_mlp), ("msg_mlp", mp.msg_mlp)):
                ln(f"mp_layers.{i}.{name}", sub)
                ff(f"mp_layers.{i}.{name}", sub)
        if not isinstance(self.edge_dec.pre_norm, nn.Identity):
            raise NotImplementedError("edge decoder must use pre_norm 'none' (config/gnn.yaml)")
        ff("edge_dec", self.edge_dec)
        return out

    def pack_weights(self) -> torch.Tensor:
        """The fp32 weight blob on the host: one ``cat`` on the parameters' device, one copy.
        After ``flatten_parameters`` it is ``self.flat`` itself (on the device, no copy)."""
        if self.is_flat():
            return self.flat
        parts = [p.detach().reshape(-1).float() for _, p in self._packed_params()]
        return torch.cat(parts).cpu().contiguous()

    # ---- flat parameters (opt-in; the native optimizer writes them in place)
    def flatten_parameters(self, device="cuda") -> torch.Tensor:
        """Move the module to ``device`` and re-point every packed parameter's ``.data`` at a view of
        ONE fp32 device tensor in blob order (``self.flat``, returned).  From then on ``pack_weights``
        is free, ``lspcg_gnn_set_weights`` reads the device blob, ``lspcg_optim_step`` updates the
        live parameters in place and ``state_dict()`` is always current.  The values keep their bits.
        Anything that re-allocates a parameter (``.to(other device)``, ``.double()``) ends the flat
        state (``is_flat()`` turns False and the module packs as before)."""
        self.to(torch.device(device))
        packed = self._packed_params()
        flat = torch.cat([p.detach().reshape(-1).float() for _, p in packed]).contiguous()
        o = 0
        for _, p in packed:
            n = p.numel()
            p.data = flat[o:o + n].view(p.shape)
            o += n
        self.flat = flat
        self._packed_version = None
        return flat

    def is_flat(self) -> bool:
        """Every packed parameter still is its view of ``self.flat``."""
        flat = self.flat
        if flat is None:
            return False
        o, base = 0, flat.data_ptr()
        for _, p in self._packed_params():
            if p.dtype != torch.float32 or p.data_ptr() != base + 4 * o:
                return False
            o += p.numel()
        return o == flat.numel()

    def weights_updated_in_place(self):
        """``self.flat`` was written behind torch's version counters (``lspcg_optim_step``): hand the
        new values to the handle now (``lspcg_gnn_set_weights`` from the device blob; the workspace
        and the analysed graph stay) and mark them packed, so the next forward uploads nothing."""
        assert self.is_flat(), "weights_updated_in_place needs flatten_parameters()"
        if self._handle is None or self._ctx is not Context.get(self.flat.device):
            self._packed_version = None
            self._ensure_handle(self.flat.device)
            return
        _lib.call("lspcg_gnn_set_weights", self._handle, _ptr(self.flat), self.flat.numel())
        self._packed_version = self._version()

    def unpack_grads(self, blob: torch.Tensor) -> dict:
        """The inverse of ``pack_weights``: ``{state_dict key: tensor}`` views of a blob in its layout
        (the gradient blob of ``lspcg_gnn_backward``, or the weights themselves)."""
        out, o = {}, 0
        flat = blob.reshape(-1)
        for key, p in self._packed_params():
            n = p.numel()
            out[key] = flat[o:o + n].reshape(p.shape)
            o += n
        assert o == flat.numel(), (o, flat.numel())
        return out

    def _version(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _ensure_handle(self, device: torch.device):
        ctx = Context.get(device)
        if self._handle is not None and self._ctx is ctx and self._packed_version == self._version():
            return
        blob = self.pack_weights()
        if self._handle is not None and self._ctx is ctx:
            # only the values changed (an optimizer step): the handle, its workspace and the analysed
            # graph stay
            _lib.call("lspcg_gnn_set_weights", self._handle, blob.data_ptr(), blob.numel())
            self._packed_version = self._version()
            return
        self._free()
        self._graph = None
        desc = _lib.lspcg_gnn_desc(node_in=self.node_in_features, edge_in=self.edge_in_features, hidden=self.hidden,
                                   mlp_layers=2, num_mp_layers=self.num_mp_layers,
                                   edge_out=self.edge_out_features, node_residual=int(self.node_residual),
                                   edge_residual=int(self.edge_residual))
        h = C.c_void_p()
        _lib.call("lspcg_gnn_create", ctx.handle, C.byref(desc), blob.data_ptr(), blob.numel(), C.byref(h))
        self._handle, self._ctx, self._packed_version = h, ctx, self._version()

    def precision(self, device=None) -> dict:
        """Which GEMM kernels ``lspcg_gnn_create`` chose for the current weights:
        ``{"f32": False}`` = split-f16 MFMAs (the default), ``True`` = fp32 MFMAs (weights whose
        LayerNorm-fed hidden activations could pass f16's range, or LSPCG_GNN_F32=1), with the
        weights' hidden-activation bound that decided it (``lspcg_gnn_precision``)."""
        self._ensure_handle(torch.device(device) if device is not None else torch.device("cuda"))
        f32, hb = C.c_int(), C.c_double()
        _lib.call("lspcg_gnn_precision", self._handle, C.byref(f32), C.byref(hb))
        return {"f32": bool(f32.value), "hidden_bound": hb.value}

    def _free(self):
        if self._handle is not None and _lib._lib is not None:
            _lib._lib.lspcg_gnn_destroy(self._handle)
        self._handle = None

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        res = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._packed_version = None
        return res

    def invalidate_graph(self):
        """Forget the cached graph analysis and release the edge_index tensor it holds (the next
        forward re-analyses).  Needed after an in-place change of edge_index that torch's version
        counter does not see (.data, DLPack / CuPy views); also frees the held tensor."""
        self._graph = None

    def forward(self, node_attr: torch.Tensor, edge_index: torch.Tensor, edge_attr: torch.Tensor):
        """Returns ``(None, edge_out [E, b*b])``; the reference's node output is the identity
        node decoder of the final node state, which the hot path discards (workspace.py:93).
        With ``differentiable`` set, gradients enabled and a parameter that requires grad, the
        output carries the parameters' autograd graph (``_GnnFn``); its bits are the same."""
        if self.differentiable and torch.is_grad_enabled():
            if node_attr.requires_grad or edge_attr.requires_grad:
                raise NotImplementedError("gradients with respect to node_attr / edge_attr are not implemented")
            params = [p for _, p in self._packed_params()]
            if any(p.requires_grad for p in params):
                if not node_attr.is_cuda:
                    raise _lib.LspcgUnavailable("NodeEdgeProcessing.forward runs on the GPU only (HIP)")
                return None, _GnnFn.apply(self, node_attr, edge_index, edge_attr, *params)
        return None, self._forward_no_grad(node_attr, edge_index, edge_attr)[3]

    @torch.no_grad()
    def _forward_no_grad(self, node_attr: torch.Tensor, edge_index: torch.Tensor, edge_attr: torch.Tensor):
        """``(x, edge_index, edge_attr, out)``: the tensors the kernels saw, and the output."""
        if not node_attr.is_cuda:
            raise _lib.LspcgUnavailable("NodeEdgeProcessing.forward runs on the GPU only (HIP)")
        dev = node_attr.device
        self._ensure_handle(dev)
        x = node_attr.to(torch.float32).contiguous()
        ea = edge_attr.to(device=dev, dtype=torch.float32).contiguous()
        ei = edge_index.to(device=dev, dtype=torch.int64).contiguous()
        N, E = x.shape[0], ei.shape[1]
        assert x.shape[1] == self.node_in_features, (x.shape, self.node_in_features)
        assert ea.shape == (E, self.edge_in_features), (ea.shape, self.edge_in_features)
        out = torch.empty(E, self.edge_out_features, dtype=torch.float32, device=dev)
        self._set_graph(ei, N, E)
        _lib.call("lspcg_gnn_forward", self._handle, N, E, _ptr(x), _ptr(ei), _ptr(ea), _ptr(out))
        return x, ei, ea, out

    def _set_graph(self, ei: torch.Tensor, N: int, E: int):
        # the graph's CSC is analysed once per edge_index (the tensor is held, so its address cannot
        # be reused by another one while cached; an in-place torch op bumps its version -- writes
        # that bypass the version counter, through .data, DLPack or CuPy views, must be followed by
        # invalidate_graph(), as lspcg_gnn.h asks for lspcg_gnn_set_graph)
        key = (ei.data_ptr(), ei._version, N, E)
        if self._graph is None or self._graph[0] != key or self._graph[1].data_ptr() != ei.data_ptr():
            _lib.call("lspcg_gnn_set_graph", self._handle, N, E, _ptr(ei))
            self._graph = (key, ei)

    def _backward(self, x, ei, ea, grad_out: torch.Tensor) -> torch.Tensor:
        """The gradient blob (``pack_weights`` layout, fp32, on the device) for ``d loss / d out``."""
        self._ensure_handle(x.device)
        N, E = x.shape[0], ei.shape[1]
        self._set_graph(ei, N, E)
        go = grad_out.to(device=x.device, dtype=torch.float32).contiguous()
        assert go.shape == (E, self.edge_out_features), (tuple(go.shape), E, self.edge_out_features)
        gw = torch.empty(sum(p.numel() for _, p in self._packed_params()), dtype=torch.float32, device=x.device)
        _lib.call("lspcg_gnn_backward", self._handle, N, E, _ptr(x), _ptr(ei), _ptr(ea), _ptr(go), _ptr(gw))
        return gw


class _GnnFn(torch.autograd.Function):
    """``out = lspcg_gnn_forward(...)`` (the no-grad path's own call, so the same bits); backward
    runs ``lspcg_gnn_backward`` and hands every parameter its slice of the gradient blob."""

    @staticmethod
    def forward(ctx, gnn, node_attr, edge_index, edge_attr, *params):
        x, ei, ea, out = gnn._forward_no_grad(node_attr.detach(), edge_index, edge_attr.detach())
        ctx.gnn = gnn
        ctx.save_for_backward(x, ei, ea)
        ctx.version = gnn._version()
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gnn = ctx.gnn
        x, ei, ea = ctx.saved_tensors
        if gnn._version() != ctx.version:
            raise RuntimeError("a GNN parameter was modified in place between forward and backward")
        grads = gnn.unpack_grads(gnn._backward(x, ei, ea, g))
        outs = []
        for (key, p), need in zip(gnn._packed_params(), ctx.needs_input_grad[4:]):
            outs.append(grads[key].to(device=p.device, dtype=p.dtype) if need else None)
        return (None, None, None, None, *outs)


def build_gnn(node_in: int, edge_in: int, block_size: int, seed: Optional[int] = 0, differentiable: bool = False,
              **over) -> NodeEdgeProcessing:
    """Seeded construction with the reference's config (workspace.py:70-76, config/gnn.yaml).
    ``differentiable=True``: the forward is differentiable with respect to the parameters."""
    cfg = default_gnn_config()
    cfg.update(over)
    if seed is not None:
        torch.manual_seed(seed)
    gnn = NodeEdgeProcessing(node_in_features=node_in, node_out_features=None, edge_in_features=edge_in,
                             edge_out_features=block_size * block_size, **cfg)
    gnn.differentiable = bool(differentiable)
    return gnn


# ---------------------------------------------------------------------------
# GraphSpmv / AATPE / LLT (basic_layers.py:112-142, 228-275) on lspcg_graph_* (HIP)
# ---------------------------------------------------------------------------
class _GraphCache:
    """lspcg_graph handles keyed on the edge_index tensor (held, so its address cannot be reused
    by another tensor while cached), its in-place version, N and the block size."""

    def __init__(self, size: int = 8):
        self.size = size
        self.items = []  # [(key, edge_index tensor, handle)]

    def get(self, edge_index: torch.Tensor, N: int, bs: int) -> C.c_void_p:
        ctx = Context.get(edge_index.device)
        key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, N, bs, ctx.device)
        for i, (k, t, h) in enumerate(self.items):
            if k == key and t.data_ptr() == edge_index.data_ptr():
                self.items.append(self.items.pop(i))
                return h
        ei = edge_index.to(torch.int64).contiguous()
        h = C.c_void_p()
        _lib.call("lspcg_graph_create", ctx.handle, int(N), int(ei.shape[1]), int(bs), _ptr(ei), C.byref(h))
        self.items.append((key, edge_index, h))
        while len(self.items) > self.size:
            _, _, old = self.items.pop(0)
            if _lib._lib is not None:
                _lib._lib.lspcg_graph_destroy(old)
        return h


_GRAPHS = _GraphCache()


def _graph_args(X: torch.Tensor, edge_index: torch.Tensor, A: torch.Tensor, *opt):
    if not X.is_cuda:
        raise _lib.LspcgUnavailable("GraphSpmv / AATPE run on the GPU only (HIP)")
    if X.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"unsupported dtype {X.dtype}")
    N = X.shape[0]
    bs = X.shape[1] if X.ndim == 2 else 1
    assert A.shape[0] == edge_index.shape[1] and tuple(A.shape[1:]) in ((bs, bs),) + (((1,),) if bs == 1 else ()), \
        (tuple(A.shape), bs)
    dev = X.device
    x = X.contiguous()
    vals = A.to(device=dev, dtype=X.dtype).contiguous()
    out = []
    for o in opt:
        if o is None:
            out.append(None)
        else:
            o = o.to(device=dev, dtype=X.dtype).contiguous()
            assert o.numel() == N * bs, (tuple(o.shape), N, bs)
            out.append(o)
    return N, bs, x, vals, out, _lib.F32 if X.dtype == torch.float32 else _lib.F64


def _wants_grad(*tensors) -> bool:
    """The autograd path is taken only when gradients are enabled and X or the values ask for one;
    in every other case the modules below run exactly their no-grad code."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _opt(t):
    return _ptr(t) if t is not None else None


def _spmv(h, code, transpose, vals, x, m):
    y = torch.empty_like(x)
    _lib.call("lspcg_graph_spmv", h, _ptr(vals), code, int(transpose), _ptr(x), _opt(m), _ptr(y))
    return y


def _grad_vals(h, code, transpose, gy, x, vals):
    dv = torch.empty_like(vals)
    _lib.call("lspcg_graph_spmv_grad_vals", h, code, int(transpose), _ptr(gy), _ptr(x), _ptr(dv))
    return dv


class _GraphSpmvFn(torch.autograd.Function):
    """``y = m ⊙ (A x)`` (transpose: ``Aᵀ x``) with ``gx = Aᵀ (m ⊙ g)`` (``A (m ⊙ g)``) through
    lspcg_graph_spmv and ``dA_e = (m⊙g)_I ⊗ x_J`` (``x_I ⊗ (m⊙g)_J``) through
    lspcg_graph_spmv_grad_vals."""

    @staticmethod
    def forward(ctx, X, A, edge_index, mask, transpose):
        N, bs, x, vals, (m,), code = _graph_args(X.detach(), edge_index, A.detach(), mask)
        ei = edge_index.to(x.device)
        h = _GRAPHS.get(ei, N, bs)
        ctx.save_for_backward(x, vals, m)
        ctx.graph = (ei, N, bs)  # looked up again in backward: the cache may have dropped the handle by then
        ctx.code, ctx.transpose, ctx.a_like = code, bool(transpose), (A.shape, A.dtype, A.device)
        return _spmv(h, code, transpose, vals, x, m).reshape(X.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, vals, m = ctx.saved_tensors
        h = _GRAPHS.get(*ctx.graph)
        gm = g.reshape(x.shape).contiguous()
        if m is not None:
            gm = gm * m.reshape(x.shape)
        gx = dA = None
        if ctx.needs_input_grad[0]:
            gx = _spmv(h, ctx.code, not ctx.transpose, vals, gm, None).reshape(g.shape)
        if ctx.needs_input_grad[1]:
            shape, dtype, dev = ctx.a_like
            dA = _grad_vals(h, ctx.code, ctx.transpose, gm, x, vals).reshape(shape).to(device=dev, dtype=dtype)
        return gx, dA, None, None, None


class _AATPEFn(torch.autograd.Function):
    """``t = δ m (Lᵀ x) ; y = m (L t) + ε x δ``; ``t`` is saved.  With ``gm = m ⊙ g`` and
    ``gtm = δ m (Lᵀ gm)``: ``gx = L gtm + ε δ g`` and ``dL_e = gm_I ⊗ t_J + x_I ⊗ gtm_J``."""

    @staticmethod
    def forward(ctx, x, L, edge_index, mask, diag, epsilon):
        N, bs, xx, vals, (m, d), code = _graph_args(x.detach(), edge_index, L.detach(), mask, diag)
        ei = edge_index.to(xx.device)
        h = _GRAPHS.get(ei, N, bs)
        t = torch.empty_like(xx)
        y = torch.empty_like(xx)
        _lib.call("lspcg_graph_aatpe", h, _ptr(vals), code, float(epsilon), _ptr(xx), _opt(m), _opt(d), _ptr(t),
                  _ptr(y))
        ctx.save_for_backward(xx, vals, m, d, t)
        ctx.graph = (ei, N, bs)
        ctx.code, ctx.eps, ctx.l_like = code, float(epsilon), (L.shape, L.dtype, L.device)
        return y.reshape(x.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xx, vals, m, d, t = ctx.saved_tensors
        h = _GRAPHS.get(*ctx.graph)
        g = g.reshape(xx.shape).contiguous()
        gm = g if m is None else g * m.reshape(xx.shape)
        gtm = _spmv(h, ctx.code, True, vals, gm, m)
        if d is not None:
            gtm = gtm * d.reshape(xx.shape)
        gx = dL = None
        if ctx.needs_input_grad[0]:
            eg = ctx.eps * g
            gx = _spmv(h, ctx.code, False, vals, gtm, None) + (eg if d is None else eg * d.reshape(xx.shape))
        if ctx.needs_input_grad[1]:
            shape, dtype, dev = ctx.l_like
            dL = _grad_vals(h, ctx.code, False, gm, t, vals) + _grad_vals(h, ctx.code, True, gtm, xx, vals)
            dL = dL.reshape(shape).to(device=dev, dtype=dtype)
        return gx, dL, None, None, None, None


class GraphSpmv(nn.Module):
    """basic_layers.py:112-142: ``y_i = Σ_j A_ij x_j`` over the blocks of an edge list
    (``use_transpose``: ``y = Aᵀ x``), then ``y * mask``.  X is [N, b], A is [E, b, b].
    Differentiable with respect to X and A when either requires grad (``_GraphSpmvFn``)."""

    def __init__(self, use_transpose: bool = False):
        super().__init__()
        self.transpose = use_transpose

    def forward(self, X, edge_index, A, mask=None):
        if _wants_grad(X, A):
            if not X.is_cuda:
                raise _lib.LspcgUnavailable("GraphSpmv / AATPE run on the GPU only (HIP)")
            return _GraphSpmvFn.apply(X, A, edge_index, mask, self.transpose)
        return self._forward_no_grad(X, edge_index, A, mask)

    @torch.no_grad()
    def _forward_no_grad(self, X, edge_index, A, mask=None):
        N, bs, x, vals, (m,), code = _graph_args(X, edge_index, A, mask)
        h = _GRAPHS.get(edge_index.to(x.device), N, bs)
        y = torch.empty_like(x)
        _lib.call("lspcg_graph_spmv", h, _ptr(vals), code, int(self.transpose), _ptr(x),
                  _ptr(m) if m is not None else None, _ptr(y))
        return y


class AATPE(nn.Module):
    """basic_layers.py:228-261: ``y = ε x + A Aᵀ x`` (``diag``: ``ε diag x + A diag Aᵀ x``), the
    mask applied after each SpMV -- the ext_spai apply on the GNN's own edge-list output.
    Differentiable with respect to x and the values when either requires grad (``_AATPEFn``)."""

    def __init__(self, epsilon):
        super().__init__()
        self.epsilon = float(epsilon)
        self.spmv = GraphSpmv()
        self.spmv_t = GraphSpmv(use_transpose=True)

    def forward(self, x, edge_index, boo_values, mask=None, diag=None):
        if _wants_grad(x, boo_values):
            if not x.is_cuda:
                raise _lib.LspcgUnavailable("GraphSpmv / AATPE run on the GPU only (HIP)")
            if diag is not None:
                assert tuple(diag.shape) == tuple(x.shape), "diag must have AT_x's shape (basic_layers.py:253)"
            return _AATPEFn.apply(x, boo_values, edge_index, mask, diag, self.epsilon)
        return self._forward_no_grad(x, edge_index, boo_values, mask, diag)

    @torch.no_grad()
    def _forward_no_grad(self, x, edge_index, boo_values, mask=None, diag=None):
        N, bs, xx, vals, (m, d), code = _graph_args(x, edge_index, boo_values, mask, diag)
        if diag is not None:
            assert tuple(diag.shape) == tuple(x.shape), "diag must have AT_x's shape (basic_layers.py:253)"
        h = _GRAPHS.get(edge_index.to(xx.device), N, bs)
        t = torch.empty_like(xx)
        y = torch.empty_like(xx)
        _lib.call("lspcg_graph_aatpe", h, _ptr(vals), code, self.epsilon, _ptr(xx), _ptr(m) if m is not None else None,
                  _ptr(d) if d is not None else None, _ptr(t), _ptr(y))
        return y


class LLT(nn.Module):
    """basic_layers.py:264-275: ``L Lᵀ x`` with the mask after each SpMV (AATPE with ε = 0)."""

    def __init__(self):
        super().__init__()
        self._op = AATPE(0.0)

    def forward(self, x, edge_index, boo_values, mask=None):
        return self._op(x, edge_index, boo_values, mask)
