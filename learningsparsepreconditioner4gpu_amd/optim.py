"""Optimizers and learning-rate schedules of the training loop (``neural_cg/utils/optim.py``).

``create_optimizer`` / ``create_scheduler`` take the reference's names and keyword arguments
(``adam | adamw | sgd``; ``exp | cosine | cosine_warmup | onecycle | none``, the arguments of the
``torch.optim`` classes the reference builds).  Nothing here is a ``torch.optim`` object:

* ``NativeOptimizer`` keeps the moments ``m`` / ``v`` as two device tensors in the layout of the
  GNN's weight blob and steps with ONE ``lspcg_optim_step`` launch (csrc/lspcg_optim.hip: global
  gradient-norm clipping as ``clip_grad_norm_``, then torch's single-tensor SGD / Adam / AdamW
  update, in place on ``gnn.flat``), followed by ``lspcg_gnn_set_weights``.
* a ``Schedule`` is a host function ``lr(t)`` in closed form, ``t`` counting the scheduler steps
  taken so far (Lightning steps a scheduler once per epoch).  It agrees with the
  ``torch.optim.lr_scheduler`` class of the same name up to rounding.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional

import torch

from . import _lib
from .sparse import Context, _ptr

_OPT_DEFAULTS = {  # torch.optim's own defaults
    "adam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "adamw": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
    "sgd": dict(lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0),
}
# flags of torch.optim that change the update rule and are not implemented: accepted only when off
_OPT_OFF = {"amsgrad": False, "maximize": False, "nesterov": False, "dampening": 0.0, "capturable": False,
            "differentiable": False}
# flags that only pick torch's implementation of the same rule
_OPT_IGNORED = ("foreach", "fused")


class NativeOptimizer:
    """SGD / Adam / AdamW over a flat fp32 parameter blob, one HIP launch per step.

    ``clip_norm`` (Lightning's ``gradient_clip_val``; ``None`` or ``<= 0``: off) and ``accumulate``
    (Lightning's ``accumulate_grad_batches``: ``step`` sums that many gradient blobs, then steps
    once with ``grad_scale = 1 / accumulate``) belong to the step, so they live here."""

    def __init__(self, name: str, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 momentum: float = 0.0, clip_norm: Optional[float] = None, accumulate: int = 1,
                 grad_scale: Optional[float] = None):
        if int(accumulate) < 1:
            raise ValueError(f"accumulate must be >= 1, got {accumulate}")
        self.accumulate = int(accumulate)
        self._acc, self._acc_count = None, 0
        self.name = name
        self.lr = float(lr)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps, self.weight_decay, self.momentum = float(eps), float(weight_decay), float(momentum)
        self.clip_norm = 0.0 if clip_norm is None else float(clip_norm)
        self.grad_scale = 1.0 / self.accumulate if grad_scale is None else float(grad_scale)
        self.step_count = 0
        self.m: Optional[torch.Tensor] = None
        self.v: Optional[torch.Tensor] = None
        self.stats: Optional[torch.Tensor] = None  # device [4]: ‖grad‖ before clipping, coef, ‖w‖ before / after
        self._pending = None  # (m, v) of a loaded state, moved to the device by the first step

    # ---- the state
    @property
    def uses_m(self) -> bool:
        return self.name != "sgd" or self.momentum != 0.0

    @property
    def uses_v(self) -> bool:
        return self.name != "sgd"

    def _desc(self) -> "_lib.lspcg_optim_desc":
        return _lib.lspcg_optim_desc(kind=_lib.OPT_KIND[self.name], beta1=self.betas[0], beta2=self.betas[1],
                                     eps=self.eps, weight_decay=self.weight_decay, momentum=self.momentum,
                                     clip_norm=self.clip_norm, grad_scale=self.grad_scale)

    def _ensure_state(self, n: int, device: torch.device):
        if self._pending is not None:
            pm, pv = self._pending
            self.m = None if pm is None else pm.to(device=device, dtype=torch.float32).contiguous()
            self.v = None if pv is None else pv.to(device=device, dtype=torch.float32).contiguous()
            self._pending = None
        if self.uses_m and self.m is None:
            self.m = torch.zeros(n, dtype=torch.float32, device=device)
        if self.uses_v and self.v is None:
            self.v = torch.zeros(n, dtype=torch.float32, device=device)
        for t in (self.m, self.v):
            if t is not None and (t.numel() != n or t.device != device):
                raise ValueError(f"optimizer state has {t.numel()} entries on {t.device}, the parameters {n} on {device}")
        if self.stats is None or self.stats.device != device:
            self.stats = torch.zeros(4, dtype=torch.float64, device=device)

    def step_blob(self, w: torch.Tensor, grad: torch.Tensor, lr: Optional[float] = None):
        """One step on a flat fp32 device tensor ``w`` (in place) with the gradient ``grad``."""
        if not w.is_cuda:
            raise _lib.LspcgUnavailable("NativeOptimizer steps on the GPU only (HIP)")
        if w.dtype != torch.float32 or grad.dtype != torch.float32 or not w.is_contiguous() or not grad.is_contiguous():
            raise TypeError("NativeOptimizer needs contiguous fp32 tensors")
        if grad.numel() != w.numel() or grad.device != w.device:
            raise ValueError(f"gradient has {grad.numel()} entries on {grad.device}, the parameters {w.numel()} on {w.device}")
        n = w.numel()
        self._ensure_state(n, w.device)
        self.step_count += 1
        _lib.call("lspcg_optim_step", Context.get(w.device).handle, C.byref(self._desc()), n, self.step_count,
                  float(self.lr if lr is None else lr), _ptr(w), _ptr(grad),
                  None if self.m is None else _ptr(self.m), None if self.v is None else _ptr(self.v), _ptr(self.stats))

    def step(self, gnn, grad_blob: torch.Tensor, lr: Optional[float] = None) -> bool:
        """Clip, update ``gnn.flat`` in place (``lspcg_optim_step``) and hand the new weights to the
        GNN handle (``lspcg_gnn_set_weights``).  ``gnn`` is flattened on first use.  With
        ``accumulate`` > 1 the blob is only summed until that many have arrived; returns whether
        the weights were stepped."""
        if self.accumulate > 1:
            self._acc = grad_blob.clone() if self._acc is None else self._acc.add_(grad_blob)
            self._acc_count += 1
            if self._acc_count < self.accumulate:
                return False
            grad_blob = self._acc
        self._apply(gnn, grad_blob, lr)
        return True

    def flush(self, gnn, lr: Optional[float] = None) -> bool:
        """Step with the gradients summed so far, if any (Lightning steps on an epoch's last batch
        even if fewer than ``accumulate`` have arrived; the scale stays ``1 / accumulate``)."""
        if self._acc_count == 0:
            return False
        self._apply(gnn, self._acc, lr)
        return True

    def _apply(self, gnn, grad_blob, lr):
        if not gnn.is_flat():
            gnn.flatten_parameters(grad_blob.device)
        self.step_blob(gnn.flat, grad_blob, lr)
        gnn.weights_updated_in_place()
        self._acc, self._acc_count = None, 0

    def set_momentum(self, value: float):
        """β1 of Adam / AdamW, the momentum of SGD (what OneCycleLR's ``cycle_momentum`` drives)."""
        if self.name == "sgd":
            self.momentum = float(value)
        else:
            self.betas = (float(value), self.betas[1])

    def state_dict(self) -> dict:
        """Plain values and host tensors (a synchronising copy of ``m`` and ``v``)."""
        host = lambda t: None if t is None else t.detach().cpu().clone()
        m, v = (self.m, self.v) if self._pending is None else self._pending
        return {"kind": self.name, "step": int(self.step_count), "m": host(m), "v": host(v),
                "betas": list(self.betas), "momentum": self.momentum}

    def load_state_dict(self, sd: dict):
        if sd["kind"] != self.name:
            raise ValueError(f"optimizer state of kind {sd['kind']!r} does not fit {self.name!r}")
        self.step_count = int(sd["step"])
        self.m = self.v = None
        self._pending = (sd.get("m"), sd.get("v"))
        if sd.get("betas") is not None:
            self.betas = (float(sd["betas"][0]), float(sd["betas"][1]))
        if sd.get("momentum") is not None:
            self.momentum = float(sd["momentum"])


def create_optimizer(name: str, params: Optional[dict] = None, clip_norm: Optional[float] = None,
                     accumulate: int = 1) -> NativeOptimizer:
    """optim.py:4-12 ``create_optimizer`` (without the parameter list: the blob is handed to
    ``step``).  ``params`` are ``torch.optim.{Adam, AdamW, SGD}``'s keyword arguments with torch's
    defaults; ``amsgrad`` / ``maximize`` / ``nesterov`` / non-zero ``dampening`` raise."""
    if name not in _OPT_DEFAULTS:
        raise ValueError(f"Unknown optimizer {name}")
    kw = dict(_OPT_DEFAULTS[name])
    for k, val in dict(params or {}).items():
        if k in _OPT_IGNORED:
            continue
        if k in _OPT_OFF:
            if val != _OPT_OFF[k] and val is not None:
                raise NotImplementedError(f"optimizer option {k}={val!r} is not implemented by lspcg_optim_step")
            continue
        if k not in kw:
            raise TypeError(f"unexpected argument {k!r} for optimizer {name}")
        kw[k] = val
    kw.pop("dampening", None)
    for k in ("lr", "eps", "weight_decay", "momentum"):
        if k in kw and not float(kw[k]) >= 0.0:
            raise ValueError(f"Invalid {k}: {kw[k]}")
    return NativeOptimizer(name, clip_norm=clip_norm, accumulate=accumulate, **kw)


# ---------------------------------------------------------------------------
# schedules
# ---------------------------------------------------------------------------
class Schedule:
    """``lr(t)``: the learning rate after ``t`` scheduler steps (``t = 0``: the initial one);
    ``momentum(t)``: β1 / momentum where the schedule drives it (OneCycleLR), else ``None``."""

    def __init__(self, name: str, lr: Callable[[int], float], momentum: Optional[Callable[[int], float]] = None):
        self.name, self._lr, self._momentum = name, lr, momentum

    def lr(self, t: int) -> float:
        return float(self._lr(int(t)))

    def momentum(self, t: int) -> Optional[float]:
        return None if self._momentum is None else float(self._momentum(int(t)))

    __call__ = lr


def _anneal_cos(start, end, pct):
    return end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1)


def _anneal_linear(start, end, pct):
    return (end - start) * pct + start


def _onecycle(p: dict) -> Schedule:
    """torch.optim.lr_scheduler.OneCycleLR (already a closed form in torch)."""
    p = dict(p)
    max_lr = float(p.pop("max_lr"))
    total = p.pop("total_steps", None)
    epochs, spe = p.pop("epochs", None), p.pop("steps_per_epoch", None)
    if total is None:
        if epochs is None or spe is None:
            raise ValueError("You must define either total_steps OR (epochs AND steps_per_epoch)")
        total = int(epochs) * int(spe)
    total = int(total)
    if total <= 0:
        raise ValueError(f"Expected positive integer total_steps, but got {total}")
    pct_start = float(p.pop("pct_start", 0.3))
    strategy = p.pop("anneal_strategy", "cos")
    if strategy not in ("cos", "linear"):
        raise ValueError(f"anneal_strategy must be one of 'cos' or 'linear', instead got {strategy}")
    anneal = _anneal_cos if strategy == "cos" else _anneal_linear
    cycle_momentum = bool(p.pop("cycle_momentum", True))
    base_m, max_m = float(p.pop("base_momentum", 0.85)), float(p.pop("max_momentum", 0.95))
    div, final_div = float(p.pop("div_factor", 25.0)), float(p.pop("final_div_factor", 1e4))
    three = bool(p.pop("three_phase", False))
    p.pop("last_epoch", None)
    if p:
        raise TypeError(f"unexpected OneCycleLR arguments {sorted(p)}")
    initial, minimum = max_lr / div, max_lr / div / final_div
    if three:
        phases = [(float(pct_start * total) - 1, initial, max_lr, max_m, base_m),
                  (float(2 * pct_start * total) - 2, max_lr, initial, base_m, max_m),
                  (total - 1, initial, minimum, max_m, max_m)]
    else:
        phases = [(float(pct_start * total) - 1, initial, max_lr, max_m, base_m),
                  (total - 1, max_lr, minimum, base_m, max_m)]

    def at(t, lo, hi):
        if t > total:
            raise ValueError(f"Tried to step {t} times. The specified number of total steps is {total}")
        start = 0.0
        for i, ph in enumerate(phases):
            end = ph[0]
            if t <= end or i == len(phases) - 1:
                return anneal(ph[lo], ph[hi], (t - start) / (end - start))
            start = end

    return Schedule("onecycle", lambda t: at(t, 1, 2), (lambda t: at(t, 3, 4)) if cycle_momentum else None)


def create_scheduler(name: str, params: Optional[dict] = None, base_lr: float = 1e-3) -> Optional[Schedule]:
    """optim.py:14-26 ``create_scheduler``: ``exp`` (ExponentialLR: gamma), ``cosine``
    (CosineAnnealingLR: T_max, eta_min), ``cosine_warmup`` (CosineAnnealingWarmRestarts: T_0,
    T_mult, eta_min), ``onecycle`` (OneCycleLR) or ``none`` (returns None, like the reference).
    ``base_lr`` is the optimizer's ``lr`` (torch reads it from the optimizer it is given)."""
    p = dict(params or {})
    p.pop("last_epoch", None)
    base = float(base_lr)
    if name == "none":
        return None
    if name == "exp":
        gamma = float(p.pop("gamma"))
        fn = lambda t: base * gamma ** t
    elif name == "cosine":
        T, eta = int(p.pop("T_max")), float(p.pop("eta_min", 0.0))
        fn = lambda t: eta + (base - eta) * (1 + math.cos(math.pi * t / T)) / 2
    elif name == "cosine_warmup":
        T0, mult, eta = int(p.pop("T_0")), int(p.pop("T_mult", 1)), float(p.pop("eta_min", 0.0))
        if T0 <= 0 or mult < 1:
            raise ValueError(f"Expected positive integer T_0 and T_mult >= 1, got {T0}, {mult}")

        def fn(t):
            cur, Ti = t, T0
            while cur >= Ti:  # torch's own bookkeeping of T_cur / T_i, one restart at a time
                cur -= Ti
                Ti *= mult
            return eta + (base - eta) * (1 + math.cos(math.pi * cur / Ti)) / 2
    elif name == "onecycle":
        return _onecycle(p)
    else:
        raise ValueError(f"Unknown scheduler {name}")
    if p:
        raise TypeError(f"unexpected arguments {sorted(p)} for scheduler {name}")
    return Schedule(name, fn)


def _split_restated(n: int, train_ratio: float, seed: int = 42):
    """scikit-learn's ShuffleSplit behind ``train_test_split``, restated: ``RandomState(seed)
    .permutation(n)``, the validation set its first ``n - floor(train_ratio n)`` entries and the
    training set the rest."""
    import numpy as np

    n_train = int(math.floor(train_ratio * n))
    if n_train < 1 or n_train >= n:
        raise ValueError(f"train_size={train_ratio} leaves an empty training or validation set of {n} samples")
    perm = np.random.RandomState(seed).permutation(n)
    n_val = n - n_train
    return [int(i) for i in perm[n_val:]], [int(i) for i in perm[:n_val]]


def train_val_split(n: int, train_ratio: float, seed: int = 42):
    """datamodule.py:26: ``train_test_split(range(n), train_size=train_ratio, random_state=42,
    shuffle=True)`` -> ``(train indices, validation indices)``; without scikit-learn, its
    restatement ``_split_restated`` (the tests hold the two equal)."""
    try:
        from sklearn.model_selection import train_test_split
    except ImportError:
        return _split_restated(n, train_ratio, seed)
    tr, va = train_test_split(range(n), train_size=train_ratio, random_state=seed, shuffle=True)
    return [int(i) for i in tr], [int(i) for i in va]
