"""Inference workspace: GNN -> L in HBM, the hot half of ``SimpleTrainingWorkspace``.

Mirrors ``neural_cg/workspace.py`` (``forward`` :92-94, ``inference_step`` :195-205) and
``neural_cg/scaled_workspace.py`` (``inference_step`` :199-212) without Lightning: the
GNN runs as HIP kernels and L is assembled on the GPU with ``to_csr_cpu`` semantics
(``lspcg_assemble``), so nothing is copied back to the host.  ``dt`` has the reference's
meaning: wall time of the GNN forward until its result is available (the reference stops
the clock after ``.cpu()``, i.e. after a device sync).
"""
from __future__ import annotations

from time import time
from typing import Optional, Tuple, Union

import numpy as np
import scipy.sparse as sp
import torch

from .data import GraphSample
from .loss import create_loss_item, spai_loss, spai_loss_and_grad
from .nn import AATPE, NodeEdgeProcessing, build_gnn, default_gnn_config
from .sparse import DeviceMatrix, assemble


# ---- weights-only loading of Lightning checkpoints with OmegaConf hparams ------------------------
# The reference trains with Hydra: train.py:56-60 builds the workspace with ``**cfg`` (a DictConfig),
# and workspace.py:52 ``save_hyperparameters()`` stores those arguments, so ``hyper_parameters``
# holds omegaconf containers (``gnn``, ``optimizer``, ...).  torch's weights-only unpickler refuses
# their classes.  Instead of unpickling them (``weights_only=False`` would run whatever the file
# names), the names below are allowlisted to INERT stand-ins: plain attribute holders that only
# receive the pickled state (NEWOBJ = ``object.__new__``, BUILD = ``__dict__.update``), which
# ``_plain`` then folds into plain dicts / lists / values.  Nothing of omegaconf or lightning is
# imported or executed; any other global in the file is still refused.
class _OmegaContainer:
    """Stand-in for an omegaconf DictConfig / ListConfig: pickled state {_metadata, _parent, _content}."""


class _OmegaValueNode:
    """Stand-in for an omegaconf value node (AnyNode, StringNode, ...): state {_metadata, _parent, _val}."""


class _OmegaMetadata:
    """Stand-in for omegaconf.base.Metadata / ContainerMetadata (ignored by _plain)."""


class _AttributeDict:
    """Stand-in for Lightning's AttributeDict (a dict subclass): NEWOBJ makes a plain dict, which
    the unpickler's SETITEMS then fills."""

    def __new__(cls, *args):
        return {}


class _TypeRef:
    """Stand-in for a type object named in omegaconf metadata (typing.Any, builtins.dict, ...)."""

    def __init__(self, name: str):
        self.name = name


def _defaultdict_standin(*_args):  # collections.defaultdict(factory) in omegaconf's resolver cache
    return {}


_OMEGA_NODES = ("AnyNode", "StringNode", "IntegerNode", "FloatNode", "BooleanNode", "BytesNode", "PathNode")
_TYPE_NAMES = ("typing.Any", "typing.Dict", "typing.List", "typing.Optional", "typing.Union", "builtins.dict",
               "builtins.list", "builtins.str", "builtins.int", "builtins.float", "builtins.bool", "builtins.object",
               "builtins.NoneType", "builtins.bytes")


def _checkpoint_safe_globals():
    g = [(_OmegaContainer, "omegaconf.dictconfig.DictConfig"), (_OmegaContainer, "omegaconf.listconfig.ListConfig"),
         (_OmegaMetadata, "omegaconf.base.Metadata"), (_OmegaMetadata, "omegaconf.base.ContainerMetadata"),
         (_defaultdict_standin, "collections.defaultdict")]
    g += [(_OmegaValueNode, f"omegaconf.nodes.{n}") for n in _OMEGA_NODES]
    g += [(_AttributeDict, n) for n in ("lightning.fabric.utilities.data.AttributeDict",
                                        "lightning_fabric.utilities.data.AttributeDict",
                                        "pytorch_lightning.utilities.parsing.AttributeDict")]
    g += [(_TypeRef(n), n) for n in _TYPE_NAMES]
    return g


def _plain(o):
    """Fold the stand-ins into plain Python: containers by their ``_content``, nodes by their
    ``_val`` (``_parent`` back references and metadata are dropped)."""
    if isinstance(o, _OmegaContainer):
        c = o.__dict__.get("_content")
        if isinstance(c, dict):
            return {k: _plain(v) for k, v in c.items()}
        if isinstance(c, (list, tuple)):
            return [_plain(v) for v in c]
        return c  # None or a "???" / interpolation string
    if isinstance(o, _OmegaValueNode):
        return _plain(o.__dict__.get("_val"))
    if isinstance(o, dict):
        return {k: _plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return type(o)(_plain(v) for v in o)
    return o


def load_checkpoint_weights_only(path: str):
    """``torch.load(path, weights_only=True)`` with the OmegaConf / Lightning hparam classes
    allowlisted to inert stand-ins (above); returns the checkpoint with ``hyper_parameters``
    as plain dicts."""
    with torch.serialization.safe_globals(_checkpoint_safe_globals()):
        ck = torch.load(path, map_location="cpu", weights_only=True)
    if "hyper_parameters" in ck:
        ck["hyper_parameters"] = _plain(ck["hyper_parameters"])
    return ck


COND_KINDS = ("neural", "none", "diag", "ainv", "ichol")  # the columns of the reference's cond.py:83-89


class SimpleInferenceWorkspace:
    neural_precond = "ext_spai"  # the solver kind of this workspace's own preconditioner

    def __init__(self, node_features: int, edge_features: int, block_size: int = 1, epsilon: float = 3e-3,
                 gnn: Optional[dict] = None, seed: Optional[int] = 0, device: Union[str, torch.device] = "cuda",
                 loss_name: str = "RelativeL2Loss_ANorm", loss_params: Optional[dict] = None):
        self.block_size = block_size
        self.epsilon = float(epsilon)
        # workspace.py:60-67 (config/loss.yaml: batch_less false, RelativeL2Loss_ANorm); built on first
        # use, so a checkpoint trained with a loss that is not implemented here still serves inference
        self.loss_name = loss_name
        self.loss_params = dict(loss_params or {})
        self._loss_fn = None
        self.spai_preconditioner = AATPE(self.epsilon)
        cfg = default_gnn_config() if gnn is None else dict(gnn)
        if seed is not None:
            torch.manual_seed(seed)
        self.gnn = NodeEdgeProcessing(node_in_features=node_features, node_out_features=None,
                                      edge_in_features=edge_features, edge_out_features=block_size * block_size,
                                      **cfg)
        self.device = torch.device(device)
        self.node_features, self.edge_features, self.gnn_config = int(node_features), int(edge_features), cfg
        self.history: list = []  # one dict of metrics per epoch of fit()
        self.last_checkpoint: Optional[str] = None
        self.last_grad_blob: Optional[torch.Tensor] = None  # what fit_step handed to the optimizer last

    # ---- checkpoints (workspace.py:52 save_hyperparameters; infer.py:237 load_from_checkpoint)
    @classmethod
    def load_from_checkpoint(cls, path: str, device="cuda", trusted: bool = False) -> "SimpleInferenceWorkspace":
        """Load a Lightning checkpoint of the reference: ``hyper_parameters`` (block_size, epsilon,
        node_features, edge_features, gnn) and ``state_dict['gnn.*']``.  Loaded weights-only
        (``load_checkpoint_weights_only``: the reference's OmegaConf hparams come back as plain
        dicts through inert stand-ins) unless ``trusted=True`` (only for files you produced
        yourself, with omegaconf installed)."""
        ck = (torch.load(path, map_location="cpu", weights_only=False) if trusted
              else load_checkpoint_weights_only(path))
        hp = ck.get("hyper_parameters", {})
        gnn_cfg = hp.get("gnn")
        ws = cls(node_features=int(hp["node_features"]), edge_features=int(hp["edge_features"]),
                 block_size=int(hp.get("block_size", 1)), epsilon=float(hp.get("epsilon", 3e-3)),
                 gnn=None if gnn_cfg is None else {k: (dict(v) if hasattr(v, "items") else v)
                                                    for k, v in dict(gnn_cfg).items()},
                 seed=None, device=device, **cls._loss_hparams(hp))
        sd = {k[len("gnn."):]: v for k, v in ck["state_dict"].items() if k.startswith("gnn.")}
        ws.gnn.load_state_dict(sd, strict=True)
        return ws

    @staticmethod
    def _loss_hparams(hp: dict) -> dict:
        """``loss.name`` / ``loss.params`` of a reference checkpoint (config/loss.yaml), if stored."""
        loss = hp.get("loss")
        if not hasattr(loss, "get") or not loss.get("name"):
            return {}
        return {"loss_name": str(loss["name"]), "loss_params": dict(loss.get("params") or {})}

    def to(self, device) -> "SimpleInferenceWorkspace":
        self.device = torch.device(device)
        return self

    def eval(self) -> "SimpleInferenceWorkspace":
        return self

    # ---- workspace.py:92-94
    def forward(self, node_attr, edge_index, edge_attr) -> torch.Tensor:
        _, boo = self.gnn(node_attr, edge_index, edge_attr)
        return boo.reshape(-1, self.block_size, self.block_size)

    __call__ = forward

    @property
    def loss_fn(self):
        if self._loss_fn is None:
            self._loss_fn = create_loss_item(self.loss_name, batch_less=False, block_size=self.block_size,
                                             **self.loss_params)
        return self._loss_fn

    # ---- workspace.py:96-112 (scaled_workspace.py:98-104 passes diag = batch.inv_diag)
    def _step_diag(self, batch: GraphSample) -> Optional[torch.Tensor]:
        return None

    @torch.no_grad()
    def shared_step(self, batch: GraphSample) -> Tuple[torch.Tensor, torch.Tensor]:
        """``_shared_step`` without Lightning's logging: ``(boo, loss)`` of a (collated) batch built
        with ``is_inference=False`` -- the reference's ``Val/Loss`` / ``Test/Loss``.  The two A-norm
        L2 losses run as the fused ``spai_loss``; ``sqr_out=False`` composes AATPE and the module."""
        b = batch if batch.x.is_cuda else batch.to(self.device)
        boo = self.forward(b.x, b.edge_index, b.edge_attr)
        diag = self._step_diag(b)
        if self.loss_fn.fused_kind is not None:
            return boo, spai_loss(b, boo, self.epsilon, diag=diag, kind=self.loss_fn.fused_kind, eps=self.loss_fn.eps)
        d = self.spai_preconditioner(b.residual, b.edge_index, boo, mask=b.mask, diag=diag)
        return boo, self.loss_fn(b, d, boo)

    # ---- workspace.py:96-112, 178-180 (training_step = _shared_step with gradients)
    def parameters(self):
        """The GNN's parameters (``torch.optim.Adam(ws.parameters())``)."""
        return self.gnn.parameters()

    def training_step(self, batch: GraphSample) -> torch.Tensor:
        """The reference's ``training_step`` without Lightning: the loss of a (collated) batch built
        with ``is_inference=False``, differentiable with respect to the GNN's parameters --
        ``lspcg_gnn_forward``, the fused ``spai_loss`` (``sqr_out=False``: AATPE and the module) and,
        on ``loss.backward()``, ``lspcg_gnn_backward``.  Sets ``gnn.differentiable``."""
        self.gnn.differentiable = True
        b = batch if batch.x.is_cuda else batch.to(self.device)
        with torch.enable_grad():
            boo = self.forward(b.x, b.edge_index, b.edge_attr)
            diag = self._step_diag(b)
            if self.loss_fn.fused_kind is not None:
                return spai_loss(b, boo, self.epsilon, diag=diag, kind=self.loss_fn.fused_kind, eps=self.loss_fn.eps)
            d = self.spai_preconditioner(b.residual, b.edge_index, boo, mask=b.mask, diag=diag)
            return self.loss_fn(b, d, boo)

    # ---- training without autograd (train.py holds the loop)
    def fit_step(self, batch: GraphSample, optimizer, lr: Optional[float] = None) -> torch.Tensor:
        """One training step with no autograd graph: ``lspcg_gnn_forward``, the fused loss with its
        ``d loss / d boo`` (``spai_loss_and_grad``; ``sqr_out=False``: ``torch.autograd.grad`` through
        AATPE and the module), ``lspcg_gnn_backward`` and ``optimizer.step`` (``optim.NativeOptimizer``:
        accumulation if configured, ``lspcg_optim_step``, ``lspcg_gnn_set_weights``).  The loss and the
        gradient blob have ``training_step`` / ``backward``'s bits.  Returns the loss as a device
        scalar; nothing is read back."""
        b = batch if batch.x.is_cuda else batch.to(self.device)
        x, ei, ea, out = self.gnn._forward_no_grad(b.x, b.edge_index, b.edge_attr)
        boo = out.reshape(-1, self.block_size, self.block_size)
        diag = self._step_diag(b)
        if self.loss_fn.fused_kind is not None:
            loss, dL = spai_loss_and_grad(b, boo, self.epsilon, diag=diag, kind=self.loss_fn.fused_kind,
                                          eps=self.loss_fn.eps)
        else:
            leaf = boo.detach().requires_grad_(True)
            with torch.enable_grad():
                d = self.spai_preconditioner(b.residual, b.edge_index, leaf, mask=b.mask, diag=diag)
                loss = self.loss_fn(b, d, leaf)
            (dL,) = torch.autograd.grad(loss, leaf)
            loss = loss.detach()
        self.last_grad_blob = self.gnn._backward(x, ei, ea, dL.reshape(out.shape))
        optimizer.step(self.gnn, self.last_grad_blob, lr)
        return loss

    def fit(self, dataset, **kw):
        """The reference's ``trainer.fit`` without Lightning: see ``train.fit`` for the arguments."""
        from .train import fit

        return fit(self, dataset, **kw)

    def save_checkpoint(self, path, epoch: int = 0, global_step: int = 0, optimizer=None, hparams: Optional[dict] = None):
        """Write a checkpoint ``load_from_checkpoint`` reads weights-only: see ``train.save_checkpoint``."""
        from .train import save_checkpoint

        return save_checkpoint(self, path, epoch=epoch, global_step=global_step, optimizer=optimizer, hparams=hparams)

    def _assemble(self, sample: GraphSample, boo: torch.Tensor, block_output: Optional[bool],
                  out: Optional[DeviceMatrix] = None) -> DeviceMatrix:
        n = sample.num_nodes * self.block_size
        bo = (self.block_size > 1) if block_output is None else block_output
        return assemble(sample.edge_index, boo, n, sample.mask, dtype=torch.float64, block_output=bo, out=out)

    # ---- workspace.py:195-205
    def inference_step(self, sample: GraphSample, time_beg: Optional[float] = None, block_output: Optional[bool] = None,
                       return_scipy: bool = False) -> Tuple[Union[DeviceMatrix, sp.csr_matrix], float]:
        s = sample if sample.x.is_cuda else sample.to(self.device)
        # the reference's clock starts with no device work pending (its to_csr_cpu is synchronous);
        # here a previous call's assembly may still be queued
        torch.cuda.synchronize(s.x.device)
        time_beg = time()
        boo = self.forward(s.x, s.edge_index, s.edge_attr)
        torch.cuda.synchronize(boo.device)
        dt = time() - time_beg
        L = self._assemble(s, boo, block_output)
        return (L.to_scipy().tocsr() if return_scipy else L), dt

    def inference_step_batch(self, samples, block_output: Optional[bool] = None):
        """inference_step over a window of graphs as ONE GNN forward on their disjoint union (not in
        the reference, which runs one forward per sample, infer.py:280): node ids offset per graph,
        so the union keeps row-major sorted edges and every node aggregates exactly its own graph's
        messages in the same order -- each L equals the single forward's bit for bit.  Returns
        ``([L_k], dt)`` with dt the wall time of the one forward (the reference's clock)."""
        ss = [s if s.x.is_cuda else s.to(self.device) for s in samples]
        offs, off = [], 0
        for s in ss:
            offs.append(off)
            off += s.num_nodes
        x = torch.cat([s.x for s in ss])
        ei = torch.cat([s.edge_index + o for s, o in zip(ss, offs)], dim=1)
        ea = torch.cat([s.edge_attr for s in ss])
        torch.cuda.synchronize(x.device)
        time_beg = time()
        boo = self.forward(x, ei, ea)
        torch.cuda.synchronize(boo.device)
        dt = time() - time_beg
        Ls, e0 = [], 0
        for s in ss:
            E = s.edge_index.shape[1]
            Ls.append(self._assemble(s, boo[e0:e0 + E], block_output))
            e0 += E
        return Ls, dt

    def system_matrix(self, sample: GraphSample, block_output: Optional[bool] = None,
                      out: Optional[DeviceMatrix] = None) -> DeviceMatrix:
        """``to_csr_cpu(edge_index, matrix_values, n, mask)`` (infer.py:282) on the device.  ``out``: a
        matrix of the same pattern (an earlier sample of a fixed-topology dataset) to overwrite in place
        (``sparse.assemble(out=)``: ``LspcgError`` with ``ERR_FORMAT``, ``out`` unchanged, when the
        pattern differs)."""
        s = sample if sample.x.is_cuda else sample.to(self.device)
        return self._assemble(s, s.matrix_values, block_output, out=out)


    def live_solver(self, A, mask=None, node_features=None, dtype=np.float64, **sample_options) -> "LiveSolver":
        """The whole chain on a matrix that lives on the device (a simulation's ``DeviceMatrix``, or
        ``DeviceMatrix.from_device_csr``): its sample built on the device (``data.DeviceSampler``),
        ``system_matrix``, a solver of this workspace's preconditioner kind, ``inference_step`` and
        ``set_spai`` -- see :class:`LiveSolver`.  ``sample_options``: ``make_sample``'s keywords."""
        return LiveSolver(self, A, mask=mask, node_features=node_features, dtype=dtype, **sample_options)

    def condition_number(self, sample: GraphSample, kind: str = "neural", **kw):
        """κ(M⁻¹A) of ``sample``'s system under preconditioner ``kind`` -- the reference's ``cond.py``
        columns ``neural, none, diag, ainv, ichol`` -- from one PCG solve's scalars
        (``spectrum.condition_number``; ``**kw``: its ``start, seed, rtol, max_iter``).  ``neural`` is
        this workspace's own preconditioner on its inferred L; the baselines are the solvers
        ``get_cg_iter_time`` builds for ``none / diagonal / ainv / ic``.  AINV(0) and IC(0) factor
        scalar CSR only, so for them a block-3 sample's A is assembled as the scalar CSR of
        ``to_csr_cpu`` (what cond.py:110 hands its factorisations), not as BSR."""
        from . import spectrum
        from .linalg import PreconditionedConjugateGradient

        if kind not in COND_KINDS:
            raise ValueError(f"unknown kind {kind!r}; expected one of {COND_KINDS}")
        s = sample if sample.x.is_cuda else sample.to(self.device)
        scalar_only = kind in ("ainv", "ichol")
        A = self.system_matrix(s, block_output=False if scalar_only else None)
        method = {"neural": self.neural_precond, "none": "none", "diag": "diagonal", "ainv": "ainv", "ichol": "ic"}[kind]
        solver = PreconditionedConjugateGradient(A, device="cuda", preconditioner=method, dtype=np.float64)
        if kind == "neural":
            L, _ = self.inference_step(s)
            solver.set_spai(L, self.epsilon, block_size=L.block_size)
        return spectrum.condition_number(solver, **kw)


class LiveSolver:
    """A matrix on the device -> GNN input -> L -> PCG, with nothing of the matrix on the host.

    Fields: ``sampler`` (``data.DeviceSampler`` of ``A``), ``sample`` (its last ``GraphSample``),
    ``A_sys`` (``ws.system_matrix(sample)``: the scaled, masked system, as the reference's infer.py
    assembles it from a sample), ``L`` (the workspace's ``inference_step``) and ``solver``
    (``PreconditionedConjugateGradient(A_sys, preconditioner=ws.neural_precond)`` with L installed).

    After new values on the same pattern (``A.set_values(...)``, ``assemble(..., out=A)``),
    :meth:`refresh` runs ``sampler.sample()``, ``system_matrix(sample, out=A_sys)``,
    ``solver.update_matrix()``, ``inference_step`` and ``set_spai``: the sampler keeps its
    ``edge_index`` tensor, so the GNN's graph analysis is reused, and the solver keeps its views,
    ordering and graphs.  :meth:`solve` hands the solver ``matrix_scale * b`` and, where the fp32
    values of the assembled system leave the residual against the caller's own A above the bound,
    refines with that A, so x solves ``mask(A) x = b`` for the caller's unscaled A."""

    def __init__(self, ws: "SimpleInferenceWorkspace", A, mask=None, node_features=None, dtype=np.float64,
                 **sample_options):
        from .data import DeviceSampler
        from .linalg import PreconditionedConjugateGradient

        self.ws = ws
        self.sampler = DeviceSampler(A, mask=mask, node_features=node_features, **sample_options)
        if self.sampler.block_size != ws.block_size:
            raise ValueError(f"the matrix has block size {self.sampler.block_size}, the workspace {ws.block_size}")
        self.sample = self.sampler.sample()
        self.A_sys = ws.system_matrix(self.sample)
        self.solver = PreconditionedConjugateGradient(self.A_sys, device="cuda", preconditioner=ws.neural_precond,
                                                      dtype=dtype, ctx=self.A_sys.ctx)
        self.L, self.gnn_time = ws.inference_step(self.sample)
        self.solver.set_spai(self.L, ws.epsilon, block_size=self.L.block_size)
        self.graphs_kept: Optional[bool] = None  # of the last refresh's update_matrix
        self.last_solve: Optional[dict] = None   # of the last solve(): refinements, relative_residual, iters

    STEPS = ("sample", "system_matrix", "update_matrix", "inference_step", "set_spai")

    def refresh(self, node_features=None) -> dict:
        """New values of the sampler's matrix on this solver (see the class).  Returns, per step of
        ``STEPS`` and for ``"total"``, ``{"wall": s, "device": s}``: the host time spent in the call and
        the device time between events recorded around it (``total``: until the device has finished)."""
        ws, dev = self.ws, self.A_sys.ctx.torch_device
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(self.STEPS) + 1)]
        walls = []
        with torch.cuda.device(dev):
            torch.cuda.synchronize(dev)
            t_begin = t0 = time()
            marks[0].record()

            def done(k):
                nonlocal t0
                marks[k].record()
                t1 = time()
                walls.append(t1 - t0)
                t0 = t1

            self.sample = self.sampler.sample(node_features=node_features)
            done(1)
            ws.system_matrix(self.sample, out=self.A_sys)
            done(2)
            _, self.graphs_kept = self.solver.update_matrix()
            done(3)
            self.L, self.gnn_time = ws.inference_step(self.sample)
            done(4)
            self.solver.set_spai(self.L, ws.epsilon, block_size=self.L.block_size)
            done(5)
            torch.cuda.synchronize(dev)
            total = time() - t_begin
        out = {name: {"wall": walls[k], "device": marks[k].elapsed_time(marks[k + 1]) / 1e3}
               for k, name in enumerate(self.STEPS)}
        out["total"] = {"wall": total, "device": marks[0].elapsed_time(marks[-1]) / 1e3}
        return out

    def residual(self, b: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """``b - mask(A) x`` with the caller's own matrix (its values, not the sample's fp32 ones):
        ``mask(A) = M A M + (I - M)`` for the 0 / 1 mask M, one ``lspcg_spmv`` of the sampler's matrix."""
        A = self.sampler.A
        m = self.sampler.mask.reshape(-1).to(x.dtype)
        y = A.matvec((m * x).to(A.dtype)).to(x.dtype)
        return b - (m * y + (1.0 - m) * x)

    def solve(self, b: torch.Tensor, x: torch.Tensor, rtol: float = 1e-6, max_iter: int = 0, refine: int = 20, **kw):
        """x (in: the start, out: the solution) solves ``mask(A) x = b`` for the caller's unscaled A:
        ``|b - mask(A) x| <= rtol |b|``.

        The first step forwards to ``solver.solve`` with ``matrix_scale * b`` as the right-hand side
        (the assembled system is the scaled one; at masked unknowns, whose rows are the identity, the
        right-hand side is ``b`` itself).  That system carries the sample's fp32 ``matrix_values``, as the
        reference's does, so against A the solution has a residual floor of about 6e-8 times the
        condition number.  Where the true residual (:meth:`residual`) is above ``rtol |b|`` after the
        forward, up to ``refine`` steps of iterative refinement follow: the same solver on the scaled
        residual, to a tolerance that halves the distance to the bound (between ``rtol`` and 0.1), and
        ``x += d``.  A well-conditioned system takes no step and gets the plain forward's bits.  A step
        is guaranteed to gain only while 6e-8 times the condition number is below 1; past that it has
        gained in practice (heat_bunny, 3.4e8: a factor of about 4 per step), and ``converged`` says
        whether the bound was met.

        Returns ``(iterations of all solves, converged, device solve time s)`` -- converged is the
        true-residual bound -- and sets ``last_solve`` (``refinements``, ``relative_residual``, ``iters``
        and ``residuals`` per solve).  ``refine=0`` with ``**kw`` (``return_history`` ...) is the plain forward and returns
        what ``solver.solve`` returns."""
        dev, dt = self.A_sys.ctx.torch_device, self.solver.torch_dtype
        m = self.sampler.mask.reshape(-1).to(dt)
        w = m * self.sample.matrix_scale + (1.0 - m)  # matrix_scale on free unknowns, 1 on masked ones
        b = b.to(device=dev, dtype=dt)
        if refine <= 0:
            return self.solver.solve(b * w, x, rtol=rtol, max_iter=max_iter, **kw)
        if kw:
            raise ValueError(f"{sorted(kw)} belong to one solver.solve: pass refine=0 for the plain forward")
        from .sparse import dot

        it, conv, t = self.solver.solve(b * w, x, rtol=rtol, max_iter=max_iter)
        iters = [it]
        nb = float(np.sqrt(dot(b, b)))
        r = self.residual(b, x)
        nr = float(np.sqrt(dot(r, r)))
        hist = [nr / nb if nb else 0.0]
        while conv and nr > rtol * nb and len(iters) <= refine:
            d = torch.zeros_like(x)
            it, conv, ts = self.solver.solve(r * w, d, rtol=min(0.1, max(rtol, 0.5 * rtol * nb / nr)), max_iter=max_iter)
            x += d
            iters.append(it)
            t += ts
            r = self.residual(b, x)
            nr = float(np.sqrt(dot(r, r)))
            hist.append(nr / nb)
        self.last_solve = {"refinements": len(iters) - 1, "relative_residual": hist[-1], "iters": iters,
                           "residuals": hist}
        return sum(iters), bool(conv and nr <= rtol * nb), t


class ScaledInferenceWorkspace(SimpleInferenceWorkspace):
    """scaled_workspace.py:199-212: L <- L · diag(rsqrt(diag(A) + 1e-7)), solved with ext_spai_scaled."""

    neural_precond = "ext_spai_scaled"

    def _step_diag(self, batch: GraphSample) -> Optional[torch.Tensor]:
        assert batch.inv_diag is not None, "Relying on batch.inv_diag to maintain stability"
        return batch.inv_diag

    def inference_step(self, sample: GraphSample, time_beg: Optional[float] = None, block_output: Optional[bool] = None,
                       return_scipy: bool = False):
        s = sample if sample.x.is_cuda else sample.to(self.device)
        # the reference's clock starts with no device work pending (its to_csr_cpu is synchronous);
        # here a previous call's assembly may still be queued
        torch.cuda.synchronize(s.x.device)
        time_beg = time()
        boo = self.forward(s.x, s.edge_index, s.edge_attr)
        torch.cuda.synchronize(boo.device)
        dt = time() - time_beg
        L = self._assemble(s, boo, block_output)
        L.scale_columns_(s.rsqrt_diag.reshape(-1).to(torch.float64))
        return (L.to_scipy().tocsr() if return_scipy else L), dt

    def inference_step_batch(self, samples, block_output: Optional[bool] = None):
        """The window's one forward, every L_k then scaled by its own sample's columns as
        inference_step scales it (the same bits)."""
        ss = [s if s.x.is_cuda else s.to(self.device) for s in samples]
        Ls, dt = super().inference_step_batch(ss, block_output)
        for L, s in zip(Ls, ss):
            L.scale_columns_(s.rsqrt_diag.reshape(-1).to(torch.float64))
        return Ls, dt
