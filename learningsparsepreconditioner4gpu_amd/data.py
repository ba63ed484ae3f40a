"""GNN input samples (host-side input plumbing for the hot path).

``GraphSample`` carries the fields of the reference's PyG ``Data`` that the inference
path reads (``x, edge_index, edge_attr, mask, matrix_values, rsqrt_diag, ptr``);
``make_sample`` builds one inference sample of an in-memory matrix through
``dataset.make_data`` (the restatement of ``neural_cg/data.py:218-336``) -- or, for a matrix that
already lives in a ``DeviceMatrix``, on the device through ``lspcg_mat_sample`` (``DeviceSampler``:
no host copy of the matrix, no upload); ``collate`` forms the
disjoint union of several samples (the reference's PyG ``DataLoader`` batch) for ``loss.spai_loss``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import scipy.sparse as sp
import torch

from .problems import BlockGraph, to_block_graph


@dataclass
class GraphSample:
    x: torch.Tensor               # [N, F_in] fp32
    edge_index: torch.Tensor      # [2, E] int64, row-major sorted
    edge_attr: torch.Tensor       # [E, F_e] fp32
    mask: torch.Tensor            # [N, b] fp32
    matrix_values: Optional[torch.Tensor]  # [E, b, b] fp32 (scaled matrix)
    diagonal: Optional[torch.Tensor] = None
    inv_diag: Optional[torch.Tensor] = None
    rsqrt_diag: Optional[torch.Tensor] = None
    block_size: int = 1
    matrix_scale: float = 1.0
    ptr: torch.Tensor = field(default=None)
    gt: Optional[torch.Tensor] = None        # lhs / matrix_scale (training samples with a stored lhs)
    residual: Optional[torch.Tensor] = None  # rhs * mask (training samples)

    def __post_init__(self):
        if self.ptr is None:
            self.ptr = torch.tensor([0, self.x.shape[0]], dtype=torch.int64)

    @property
    def num_nodes(self) -> int:
        return int(self.x.shape[0])

    def to(self, device) -> "GraphSample":
        kw = {}
        for k, v in self.__dict__.items():
            kw[k] = v.to(device) if isinstance(v, torch.Tensor) and k != "ptr" else v
        return GraphSample(**kw)


_PER_ROW_FIELDS = ("x", "edge_attr", "mask", "matrix_values", "diagonal", "inv_diag", "rsqrt_diag", "gt", "residual")


def collate(samples: Sequence[GraphSample]) -> GraphSample:
    """The disjoint union of ``samples`` as one ``GraphSample`` (PyG's ``Batch.from_data_list``
    for the fields kept here): every per-node and per-edge field concatenated, each sample's node
    offset added to its ``edge_index``, and ``ptr`` (host int64) holding the node boundaries of
    the graphs -- a sample that is itself a batch contributes all of its graphs.  A field must be
    present in every sample or in none."""
    samples = list(samples)
    if not samples:
        raise ValueError("collate needs at least one sample")
    bs = samples[0].block_size
    if any(s.block_size != bs for s in samples):
        raise ValueError("collate: samples of different block_size")
    kw = {}
    for name in _PER_ROW_FIELDS:
        vals = [getattr(s, name) for s in samples]
        if all(v is None for v in vals):
            kw[name] = None
        elif any(v is None for v in vals):
            raise ValueError(f"collate: field {name!r} is missing from some samples")
        else:
            kw[name] = torch.cat(vals)
    eis, ptr, off = [], [0], 0
    for s in samples:
        eis.append(s.edge_index + off)
        ptr += [off + int(p) for p in s.ptr.tolist()[1:]]
        off += s.num_nodes
    scales = {float(s.matrix_scale) for s in samples}
    return GraphSample(edge_index=torch.cat(eis, dim=1), block_size=bs, ptr=torch.tensor(ptr, dtype=torch.int64),
                       matrix_scale=scales.pop() if len(scales) == 1 else float("nan"), **kw)


def _sample_codes(block_size: int, use_mask_as_node_feature: bool, use_edge_features_as_node_feature,
                  normalize_matrix, node_in: int):
    """The options of the device path as ``lspcg_sample_desc`` codes, checked before any native call:
    ``(normalize, flag, reduce, node_in, F_in)``."""
    from . import _lib

    norm = normalize_matrix
    if isinstance(norm, bool):  # make_data: True is "mean", False is "none"
        norm = "mean" if norm else "none"
    if not isinstance(norm, str) or norm not in _lib.NORM:
        raise ValueError(f"unknown normalize_matrix {normalize_matrix!r}; expected one of {tuple(_lib.NORM)}")
    if not isinstance(use_edge_features_as_node_feature, str) or use_edge_features_as_node_feature not in _lib.REDUCE:
        raise ValueError(f"unknown use_edge_features_as_node_feature {use_edge_features_as_node_feature!r}; "
                         f"expected one of {tuple(_lib.REDUCE)}")
    if block_size not in (1, 3):
        raise ValueError(f"block_size {block_size}: the device matrices are scalar CSR or BSR 3x3")
    if norm == "l1" and block_size != 1:
        # the reference's own l1 branch is wrong for b > 1 (dataset.make_data's note)
        raise ValueError("normalize_matrix='l1' is defined for block_size 1 only")
    flag = int(bool(use_mask_as_node_feature))
    red = _lib.REDUCE[use_edge_features_as_node_feature]
    f_in = int(node_in) + flag * block_size + (block_size * block_size if red else 0)
    if f_in == 0:
        raise ValueError("No node feature found.")
    return _lib.NORM[norm], flag, red, int(node_in), f_in


def _as_tensor(a) -> torch.Tensor:
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))  # (a copy: a may be read-only)


class DeviceSampler:
    """``make_sample`` for matrices of ONE pattern that live on the device: every field of the
    ``GraphSample`` is built by ``lspcg_mat_sample`` from the matrix's own arrays (no host copy of the
    matrix, no upload), into tensors that are allocated once.

    ``A``: a ``DeviceMatrix`` (scalar CSR or BSR 3x3, fp32 / fp64, rows sorted) -- or a scipy matrix,
    uploaded with ``block_size``.  ``mask`` ([N*b], numpy or tensor) and ``node_features`` ([N, k]) as
    for ``make_sample``; the options are ``make_sample``'s (``use_node_features_as_edge_feature`` is
    not offered).  ``sample()`` rebuilds the fields from the matrix's current values and always
    returns the same ``edge_index`` tensor (``lspcg_mat_edge_index`` runs once), so the GNN's graph
    analysis and the cached graph handles of that tensor are found again.  The returned samples share
    their tensors: one ``sample()`` overwrites what the one before returned."""

    def __init__(self, A, mask=None, node_features=None, block_size: Optional[int] = None,
                 use_mask_as_node_feature: bool = True, use_edge_features_as_node_feature: str = "disable",
                 normalize_matrix="mean", is_inference: bool = True):
        from . import _lib
        from .sparse import DeviceMatrix

        on_device = isinstance(A, DeviceMatrix)
        if on_device and block_size is not None and block_size != A.block_size:
            raise ValueError(f"block_size={block_size}, the matrix has {A.block_size}")
        bs = A.block_size if on_device else (1 if block_size is None else int(block_size))
        node_in = 0 if node_features is None else int(node_features.shape[1])
        norm, flag, red, node_in, f_in = _sample_codes(bs, use_mask_as_node_feature, use_edge_features_as_node_feature,
                                                       normalize_matrix, node_in)
        if not on_device:
            A = DeviceMatrix.from_scipy(A, dtype=np.float64, block_size=bs)
        if A.nnzb == 0 or A.n == 0:
            raise ValueError("an empty matrix has no sample")
        self.A = A
        self.block_size = bs
        self.is_inference = bool(is_inference)
        self._desc = _lib.lspcg_sample_desc(norm, flag, red, node_in)
        dev = A.ctx.torch_device
        N, E = A.n // bs, A.nnzb
        self.num_nodes = N
        f32 = dict(dtype=torch.float32, device=dev)
        self.edge_index = torch.empty((2, E), dtype=torch.int64, device=dev)
        _lib.call("lspcg_mat_edge_index", A.handle, self.edge_index.data_ptr())
        self.x = torch.empty((N, f_in), **f32)
        self.edge_attr = torch.empty((E, bs * bs), **f32)
        self.diagonal, self.inv_diag, self.rsqrt_diag = (torch.empty((N, bs), **f32) for _ in range(3))
        self._scale = torch.empty(1, dtype=torch.float64, device=dev)
        self._mask_in = None  # what the kernel reads: fp32 or fp64, [N*b]
        if mask is None:
            self.mask = torch.ones((N, bs), **f32)
        else:
            m = _as_tensor(mask).to(dev)
            if m.dtype not in (torch.float32, torch.float64):
                m = m.double()
            if m.numel() != N * bs:
                raise ValueError(f"mask has {m.numel()} entries, the matrix has {N * bs} rows")
            self._mask_in = m.reshape(-1).contiguous()
            self.mask = self._mask_in.to(torch.float32).reshape(N, bs)
        self._nf = self._features(node_features)

    def _features(self, node_features) -> Optional[torch.Tensor]:
        k = self._desc.node_in
        if node_features is None:
            if k:
                raise ValueError(f"this sampler was built with {k} node feature columns")
            return None
        nf = _as_tensor(node_features).to(device=self.x.device, dtype=torch.float32).contiguous()
        if tuple(nf.shape) != (self.num_nodes, k):
            raise ValueError(f"node_features is {tuple(nf.shape)}, expected {(self.num_nodes, k)}")
        return nf

    def sample(self, A=None, node_features=None) -> GraphSample:
        """The sample of ``A`` (default: the sampler's matrix, e.g. after ``set_values``) -- a matrix
        of another size, entry count or block size raises ``ValueError``; that the pattern is the
        same is the caller's statement -- with new ``node_features`` if given."""
        import ctypes as C

        from . import _lib

        if A is not None and A is not self.A:
            if (A.n, A.nnzb, A.block_size) != (self.A.n, self.A.nnzb, self.A.block_size):
                raise ValueError(f"the sampler was built for n={self.A.n}, nnzb={self.A.nnzb}, block size "
                                 f"{self.A.block_size}; got n={A.n}, nnzb={A.nnzb}, block size {A.block_size}")
            if A.ctx is not self.A.ctx:
                raise ValueError("the matrix belongs to another context")
            self.A = A
        if node_features is not None:
            self._nf = self._features(node_features)
        A = self.A
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        mcode = _lib.F64 if self._mask_in is not None and self._mask_in.dtype == torch.float64 else _lib.F32
        _lib.call("lspcg_mat_sample", A.ctx.handle, A.handle, C.byref(self._desc), ptr(self._mask_in), mcode,
                  ptr(self._nf), ptr(self.x), ptr(self.edge_attr), ptr(self.diagonal), ptr(self.inv_diag),
                  ptr(self.rsqrt_diag), ptr(self._scale))
        bs = self.block_size
        kw = {}
        if not self.is_inference:
            kw["residual"] = torch.randn(self.num_nodes, bs, dtype=torch.float32, device=self.x.device) * self.mask
        return GraphSample(x=self.x, edge_index=self.edge_index, edge_attr=self.edge_attr, mask=self.mask,
                           matrix_values=self.edge_attr.view(-1, bs, bs), diagonal=self.diagonal,
                           inv_diag=self.inv_diag, rsqrt_diag=self.rsqrt_diag, block_size=bs,
                           matrix_scale=float(self._scale.item()), **kw)  # the one 8-byte read-back


def make_sample(A, mask: Optional[np.ndarray] = None, node_features: Optional[np.ndarray] = None,
                block_size: int = 1, use_mask_as_node_feature: bool = True,
                use_edge_features_as_node_feature: str = "disable", normalize_matrix="mean",
                is_inference: bool = True) -> GraphSample:
    """make_data (data.py:218-336) for a sample of an in-memory matrix ``A`` (``is_inference=False``:
    a training sample with a random right-hand side drawn from torch's global generator): the
    block COO view of A (``FolderDataset.load``'s layout, data.py:471-572) fed to
    ``dataset.make_data`` -- the one restatement of make_data, golden-checked for every option.

    ``A`` may be a ``DeviceMatrix``: the sample is then built on A's device by ``lspcg_mat_sample``
    (``DeviceSampler``; same keyword arguments, ``block_size`` taken from the handle, ``mask`` /
    ``node_features`` numpy arrays or tensors) and its tensors live there."""
    from .dataset import RawData, make_data
    from .sparse import DeviceMatrix

    if isinstance(A, DeviceMatrix):
        return DeviceSampler(A, mask=mask, node_features=node_features,
                             use_mask_as_node_feature=use_mask_as_node_feature,
                             use_edge_features_as_node_feature=use_edge_features_as_node_feature,
                             normalize_matrix=normalize_matrix, is_inference=is_inference).sample()
    g: BlockGraph = to_block_graph(sp.csr_matrix(A), block_size)
    n_nodes = g.num_nodes
    if mask is None:
        mask = np.ones((n_nodes, block_size), dtype=np.float64)
    raw = RawData(block_values=g.block_values, diagonals=sp.csr_matrix(A).diagonal().reshape(-1, block_size),
                  edge_index=g.edge_index, node_features=None if node_features is None else np.asarray(node_features),
                  lhs=None, rhs=None, mask=np.asarray(mask, dtype=np.float64).reshape(n_nodes, block_size),
                  num_nodes=n_nodes, block_size=block_size)
    return make_data(raw, use_matrix_as_edge_feature=True, use_mask_as_node_feature=use_mask_as_node_feature,
                     use_node_features_as_edge_feature=False,
                     use_edge_features_as_node_feature=use_edge_features_as_node_feature, use_random_rhs=True,
                     normalize_matrix=normalize_matrix, is_inference=is_inference)
