"""CPU: loss.create_loss_item's name handling, the GPU-only guards of the training objective and
data.collate's offsets and ptr (no compute calls -- there is no GPU here)."""
import types

import pytest
import torch


def test_create_loss_item_names():
    from learningsparsepreconditioner4gpu_amd.loss import L2Loss_ANorm, RelativeL2Loss_ANorm, create_loss_item

    a = create_loss_item("RelativeL2Loss_ANorm", batch_less=False, block_size=3)
    assert isinstance(a, RelativeL2Loss_ANorm) and a.block_size == 3 and a.sqr_out and a.eps == 1e-6
    assert a.fused_kind == "relative"
    b = create_loss_item("relativel2loss_anorm", False, 1, sqr_out=False, eps=1e-4)
    assert isinstance(b, RelativeL2Loss_ANorm) and not b.sqr_out and b.eps == 1e-4 and b.fused_kind is None
    c = create_loss_item("L2LOSS_ANORM", batch_less=True, block_size=1)
    assert isinstance(c, L2Loss_ANorm) and c.batch_less and c.fused_kind == "mse"
    for name in ("RelativeL2Loss_PlainNorm", "PropLoss", "L1Loss", "RelPropLoss", "CosineSimilarityLoss_PlainNorm",
                 "CosineSimilarityLoss_ANorm", "ConjGradLoss_PlainNorm", "ConjGradLoss_ANorm",
                 "ConjGradLoss_ANorm_NoRelative", "NifLoss_Norm"):
        with pytest.raises(NotImplementedError, match=name):
            create_loss_item(name, batch_less=False, block_size=1)
    with pytest.raises(ValueError, match="Unknown loss NoSuchLoss"):
        create_loss_item("NoSuchLoss", batch_less=False, block_size=1)


def test_cpu_tensors_raise_unavailable():
    from learningsparsepreconditioner4gpu_amd import _lib
    from learningsparsepreconditioner4gpu_amd.loss import create_loss_item, spai_loss
    from learningsparsepreconditioner4gpu_amd.nn import AATPE, GraphSpmv

    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    A = torch.randn(3, 1, 1)
    batch = types.SimpleNamespace(residual=torch.randn(3, 1), edge_index=ei, mask=torch.ones(3, 1), matrix_values=A,
                                  ptr=torch.tensor([0, 3]))
    boo = torch.randn(3, 1, 1, requires_grad=True)
    with pytest.raises(_lib.LspcgUnavailable):
        spai_loss(batch, boo, 3e-3)
    with pytest.raises(_lib.LspcgUnavailable):
        GraphSpmv()(batch.residual, ei, boo)
    with pytest.raises(_lib.LspcgUnavailable):
        AATPE(3e-3)(batch.residual, ei, boo, batch.mask)
    with pytest.raises(_lib.LspcgUnavailable):
        GraphSpmv()(batch.residual, ei, A)  # the no-grad path, as before
    with pytest.raises(_lib.LspcgUnavailable):
        create_loss_item("RelativeL2Loss_ANorm", False, 1)(batch, batch.residual, boo)
    with pytest.raises(ValueError, match="kind"):
        spai_loss(batch, boo, 3e-3, kind="cosine")


def _sample(n, e, seed, bs=1, training=True):
    from learningsparsepreconditioner4gpu_amd.data import GraphSample

    g = torch.Generator().manual_seed(seed)
    return GraphSample(x=torch.randn(n, 2, generator=g), edge_index=torch.randint(0, n, (2, e), generator=g),
                       edge_attr=torch.randn(e, bs * bs, generator=g), mask=torch.ones(n, bs),
                       matrix_values=torch.randn(e, bs, bs, generator=g), inv_diag=torch.rand(n, bs, generator=g),
                       block_size=bs, matrix_scale=2.0,
                       residual=torch.randn(n, bs, generator=g) if training else None)


def test_collate_offsets_and_ptr():
    from learningsparsepreconditioner4gpu_amd.data import collate

    a, b, c = _sample(4, 6, 1), _sample(1, 1, 2), _sample(7, 9, 3)
    u = collate([a, b, c])
    assert u.ptr.dtype == torch.int64 and u.ptr.tolist() == [0, 4, 5, 12]
    assert u.num_nodes == 12 and u.block_size == 1 and u.matrix_scale == 2.0
    assert torch.equal(u.edge_index, torch.cat([a.edge_index, b.edge_index + 4, c.edge_index + 5], dim=1))
    for name in ("x", "edge_attr", "mask", "matrix_values", "inv_diag", "residual"):
        assert torch.equal(getattr(u, name), torch.cat([getattr(s, name) for s in (a, b, c)])), name
    assert u.gt is None and u.diagonal is None
    # a batch is a sample: collating it again keeps every graph
    v = collate([u, a])
    assert v.ptr.tolist() == [0, 4, 5, 12, 16]
    assert torch.equal(v.edge_index[:, -6:], a.edge_index + 12)
    # the inputs are left alone
    assert a.ptr.tolist() == [0, 4] and int(a.edge_index.max()) < 4
    with pytest.raises(ValueError, match="residual"):
        collate([a, _sample(3, 2, 4, training=False)])
    with pytest.raises(ValueError, match="block_size"):
        collate([a, _sample(3, 2, 5, bs=3)])
    with pytest.raises(ValueError):
        collate([])


def test_workspace_loss_name():
    from learningsparsepreconditioner4gpu_amd.loss import L2Loss_ANorm, RelativeL2Loss_ANorm
    from learningsparsepreconditioner4gpu_amd.workspace import ScaledInferenceWorkspace, SimpleInferenceWorkspace

    ws = SimpleInferenceWorkspace(node_features=1, edge_features=1)
    assert ws.loss_name == "RelativeL2Loss_ANorm" and isinstance(ws.loss_fn, RelativeL2Loss_ANorm)
    ws = ScaledInferenceWorkspace(node_features=1, edge_features=1, loss_name="L2Loss_ANorm")
    assert isinstance(ws.loss_fn, L2Loss_ANorm)
    with pytest.raises(ValueError, match="Unknown loss"):
        SimpleInferenceWorkspace(node_features=1, edge_features=1, loss_name="nope").loss_fn
