"""GNN input samples (host-side input plumbing for the hot path).

``GraphSample`` carries the fields of the reference's PyG ``Data`` that the inference
path reads (``x, edge_index, edge_attr, mask, matrix_values, rsqrt_diag, ptr``);
``make_sample`` builds one inference sample of an in-memory matrix through
``dataset.make_data`` (the restatement of ``neural_cg/data.py:218-336``); ``collate`` forms the
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


def make_sample(A: sp.spmatrix, mask: Optional[np.ndarray] = None, node_features: Optional[np.ndarray] = None,
                block_size: int = 1, use_mask_as_node_feature: bool = True,
                use_edge_features_as_node_feature: str = "disable", normalize_matrix="mean",
                is_inference: bool = True) -> GraphSample:
    """make_data (data.py:218-336) for a sample of an in-memory matrix ``A`` (``is_inference=False``:
    a training sample with a random right-hand side drawn from torch's global generator): the
    block COO view of A (``FolderDataset.load``'s layout, data.py:471-572) fed to
    ``dataset.make_data`` -- the one restatement of make_data, golden-checked for every option."""
    from .dataset import RawData, make_data

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
