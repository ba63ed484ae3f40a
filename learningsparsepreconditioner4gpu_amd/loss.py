"""The SPAI training objective on the GPU (``neural_cg/loss.py``, ``config/loss.yaml``).

The reference's ``_shared_step`` (``workspace.py:96-112``, ``scaled_workspace.py:98-104``) is
``boo = gnn(...)``, ``d = AATPE(residual, edge_index, boo, mask[, inv_diag])``,
``loss = loss_fn(batch, d, boo)``.  Two forms of it live here:

* ``spai_loss(batch, boo, epsilon, diag, kind)``: the whole chain and its gradient with respect
  to ``boo`` in one ``lspcg_graph_spai_loss`` launch sequence (csrc/lspcg_graph.hip) -- five
  row-sum SpMVs, a fixed-order reduction in double and one per-edge outer-product kernel; no
  ``[E,b,b]`` message tensor, no atomics, the same bits every time.
* the modules ``RelativeL2Loss_ANorm`` / ``L2Loss_ANorm`` with the reference's call shape
  ``forward(batch, d, L_values)``: ``d`` goes through the differentiable ``GraphSpmv``
  (``nn.py``), the norms are torch ops, so ``d`` may come from any differentiable expression
  (``AATPE`` of ``nn.py``, or a user's own) and ``sqr_out=False`` is served too.

``batch`` is a ``data.GraphSample`` (``data.collate`` of several), or any object with
``residual, edge_index, mask, matrix_values, ptr``.  ``boo`` may come from the differentiable
``NodeEdgeProcessing`` (``nn.py``): ``d loss / d boo`` is then the input of ``lspcg_gnn_backward``
(``workspace.training_step``).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch
from torch import nn

from . import _lib
from .nn import _GRAPHS, GraphSpmv, _opt
from .sparse import _ptr

KINDS = {"relative": 0, "mse": 1}

# create_loss_item: the reference's names (loss.py:420-461), lower-cased
_NOT_NATIVE = ("relativel2loss_plainnorm", "proploss", "l1loss", "relproploss", "cosinesimilarityloss_plainnorm",
               "cosinesimilarityloss_anorm", "conjgradloss_plainnorm", "conjgradloss_anorm",
               "conjgradloss_anorm_norelative", "nifloss_norm")


def _graph_ptrs(batch, batch_less: bool) -> List[int]:
    n = int(batch.residual.shape[0])
    if batch_less or getattr(batch, "ptr", None) is None:
        return [0, n]
    return [int(v) for v in torch.as_tensor(batch.ptr).detach().cpu().tolist()]


def _spai_loss_launch(boo, r, edge_index, A, mask, diag, ptr, epsilon, kind, eps, want_grad):
    """One ``lspcg_graph_spai_loss`` call: ``(loss as a device double, d loss / d boo or None)``."""
    N = r.shape[0]
    bs = r.shape[1] if r.ndim == 2 else 1
    E = edge_index.shape[1]
    dt, dev = boo.dtype, r.device
    code = _lib.F32 if dt == torch.float32 else _lib.F64
    cast = lambda t: None if t is None else t.detach().to(device=dev, dtype=dt).contiguous()
    Lv, Av, rr, m, d = cast(boo), cast(A), cast(r), cast(mask), cast(diag)
    assert Lv.numel() == E * bs * bs and Av.numel() == E * bs * bs, (tuple(Lv.shape), tuple(Av.shape), E, bs)
    for o in (m, d):
        assert o is None or o.numel() == N * bs, (tuple(o.shape), N, bs)
    h = _GRAPHS.get(edge_index.to(dev), N, bs)
    hp = torch.as_tensor(ptr, dtype=torch.int64).cpu().contiguous()
    out = torch.empty((), dtype=torch.float64, device=dev)
    dL = torch.empty_like(Lv) if want_grad else None
    _lib.call("lspcg_graph_spai_loss", h, _ptr(Lv), _ptr(Av), code, float(epsilon), _ptr(rr), _opt(m), _opt(d),
              C.c_void_p(hp.data_ptr()), int(hp.numel() - 1), int(kind), float(eps), _ptr(out), _opt(dL))
    return out, dL


class _SpaiLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, boo, r, edge_index, A, mask, diag, ptr, epsilon, kind, eps):
        out, dL = _spai_loss_launch(boo, r, edge_index, A, mask, diag, ptr, epsilon, kind, eps,
                                    ctx.needs_input_grad[0])
        if dL is not None:
            ctx.save_for_backward(dL)
            ctx.like = (boo.shape, boo.device)
        return out.to(boo.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (dL,) = ctx.saved_tensors
        shape, dev = ctx.like
        return ((g.to(dL.dtype) * dL).reshape(shape).to(dev),) + (None,) * 9


def _check_spai_args(batch, boo, kind):
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    if batch.residual is None:
        raise ValueError("the batch has no residual (build the samples with is_inference=False)")
    if not batch.residual.is_cuda:
        raise _lib.LspcgUnavailable("spai_loss runs on the GPU only (HIP)")
    if boo.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"unsupported dtype {boo.dtype}")


def spai_loss_and_grad(batch, boo: torch.Tensor, epsilon: float, diag: Optional[torch.Tensor] = None,
                       kind: str = "relative", eps: float = 1e-6):
    """``spai_loss`` without autograd: ``(loss, d loss / d boo)`` straight from the one launch
    sequence -- the loss bits of ``spai_loss`` and the gradient bits its ``backward`` hands out for
    an upstream gradient of 1.  ``boo`` is treated as a constant; the loss stays on the device."""
    _check_spai_args(batch, boo, kind)
    with torch.no_grad():
        out, dL = _spai_loss_launch(boo, batch.residual, batch.edge_index, batch.matrix_values, batch.mask, diag,
                                    _graph_ptrs(batch, False), float(epsilon), KINDS[kind], float(eps), True)
        return out.to(boo.dtype), dL.reshape(boo.shape)


def spai_loss(batch, boo: torch.Tensor, epsilon: float, diag: Optional[torch.Tensor] = None, kind: str = "relative",
              eps: float = 1e-6) -> torch.Tensor:
    """``loss_fn(batch, AATPE(epsilon)(batch.residual, batch.edge_index, boo, batch.mask, diag), boo)``
    for ``RelativeL2Loss_ANorm`` (``kind="relative"``, ``sqr_out=True``) or ``L2Loss_ANorm``
    (``kind="mse"``), as a scalar tensor of ``boo``'s dtype.  When ``boo`` requires grad, the same
    launch sequence also leaves ``d loss / d boo``, which ``backward`` hands out."""
    _check_spai_args(batch, boo, kind)
    r = batch.residual
    return _SpaiLossFn.apply(boo, r, batch.edge_index, batch.matrix_values, batch.mask, diag,
                             _graph_ptrs(batch, False), float(epsilon), KINDS[kind], float(eps))


class NeuralCGLossBase(nn.Module):
    """loss.py:87-116: ``forward(batch, d, L_values)``; ``d`` is the preconditioner's output."""

    fused_kind: Optional[str] = None  # the spai_loss kind this module equals, if any

    def __init__(self, batch_less: bool, block_size: int):
        super().__init__()
        self.spmv = GraphSpmv()
        self.spmv_transpose = GraphSpmv(True)
        self.block_size = block_size
        self.batch_less = batch_less

    def _Ad(self, batch, d):
        return self.spmv(X=d, edge_index=batch.edge_index, A=batch.matrix_values.to(d.dtype), mask=batch.mask)

    def forward(self, batch, d, L_values):
        raise NotImplementedError()


class RelativeL2Loss_ANorm(NeuralCGLossBase):
    """loss.py:168-188: the mean over the graphs of ``‖A d − r‖² / (‖r‖² + eps)``
    (``sqr_out=False``: ``‖A d − r‖ / (‖r‖ + eps)``)."""

    def __init__(self, batch_less: bool, block_size: int, sqr_out: bool = True, eps: float = 1e-6):
        super().__init__(batch_less, block_size)
        self.sqr_out, self.eps = bool(sqr_out), float(eps)
        self.fused_kind = "relative" if self.sqr_out else None

    def forward(self, batch, d, L_values):
        ptrs = _graph_ptrs(batch, self.batch_less)
        Ad = self._Ad(batch, d)
        r = batch.residual.to(Ad.dtype)
        loss = 0.0
        for b, e in zip(ptrs[:-1], ptrs[1:]):
            gt = torch.linalg.norm(r[b:e].flatten())
            err = torch.linalg.norm((Ad[b:e] - r[b:e]).flatten())
            loss = loss + (err ** 2 / (gt ** 2 + self.eps) if self.sqr_out else err / (gt + self.eps))
        return loss / (len(ptrs) - 1)


class L2Loss_ANorm(NeuralCGLossBase):
    """loss.py:190-203: ``mse_loss(A d, r)`` over all elements (``sqr_out`` and ``eps`` are
    accepted and unused, as in the reference)."""

    fused_kind = "mse"

    def __init__(self, batch_less: bool, block_size: int, sqr_out: bool = True, eps: float = 1e-6):
        super().__init__(batch_less, block_size)
        self.sqr_out, self.eps = bool(sqr_out), float(eps)

    def forward(self, batch, d, L_values):
        Ad = self._Ad(batch, d)
        return torch.nn.functional.mse_loss(Ad, batch.residual.to(Ad.dtype).reshape(Ad.shape))


def create_loss_item(name: str, batch_less, block_size, **params) -> NeuralCGLossBase:
    """loss.py:420-461: the loss by its (case-insensitive) reference name.  The two A-norm L2
    losses are implemented; the reference's other names raise NotImplementedError."""
    key = name.lower()
    if key == "relativel2loss_anorm":
        return RelativeL2Loss_ANorm(batch_less=batch_less, block_size=block_size, **params)
    if key == "l2loss_anorm":
        return L2Loss_ANorm(batch_less=batch_less, block_size=block_size, **params)
    if key in _NOT_NATIVE:
        raise NotImplementedError(f"loss {name} of the reference is not implemented here "
                                  "(available: RelativeL2Loss_ANorm, L2Loss_ANorm)")
    raise ValueError(f"Unknown loss {name}")
