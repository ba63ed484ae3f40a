"""CPU: the host side of the differentiable GNN -- unpack_grads is the inverse of pack_weights
under the reference's state_dict keys, the differentiable forward refuses CPU tensors, and the
workspaces expose training_step / parameters."""
import pytest
import torch


@pytest.mark.parametrize("node_in,edge_in,bs", [(1, 1, 1), (4, 9, 3), (20, 17, 2)])
def test_unpack_grads_inverts_pack_weights(node_in, edge_in, bs):
    from learningsparsepreconditioner4gpu_amd.nn import build_gnn

    gnn = build_gnn(node_in, edge_in, bs, seed=5)
    with torch.no_grad():  # LayerNorm affines off their defaults, so a swapped gamma / beta shows
        for p in gnn.parameters():
            if p.requires_grad:
                p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())))
    blob = gnn.pack_weights()
    assert blob.dtype == torch.float32 and blob.device.type == "cpu" and blob.ndim == 1
    got = gnn.unpack_grads(blob)
    sd = gnn.state_dict()
    want = {k: v for k, v in sd.items() if not k.endswith("node_msg_norm.scale")}
    assert set(got) == set(want)
    assert sum(v.numel() for v in got.values()) == blob.numel()
    for k, v in want.items():
        assert got[k].shape == v.shape and torch.equal(got[k], v), k
    assert all(k.endswith((".weight", ".bias")) for k in got)


def test_differentiable_forward_needs_the_gpu():
    from learningsparsepreconditioner4gpu_amd import _lib
    from learningsparsepreconditioner4gpu_amd.nn import build_gnn

    gnn = build_gnn(2, 1, 1, differentiable=True)
    assert gnn.differentiable and not build_gnn(2, 1, 1).differentiable
    x, ei, ea = torch.zeros(3, 2), torch.tensor([[0, 1], [1, 0]]), torch.zeros(2, 1)
    with pytest.raises(_lib.LspcgUnavailable):
        gnn(x, ei, ea)
    with pytest.raises(NotImplementedError):
        gnn(x, ei, ea.clone().requires_grad_())


def test_workspaces_expose_training_step_and_parameters():
    from learningsparsepreconditioner4gpu_amd.workspace import ScaledInferenceWorkspace, SimpleInferenceWorkspace

    for cls in (SimpleInferenceWorkspace, ScaledInferenceWorkspace):
        ws = cls(node_features=2, edge_features=1, device="cpu")
        assert callable(ws.training_step)
        params = list(ws.parameters())
        assert params and all(a is b for a, b in zip(params, ws.gnn.parameters()))
        torch.optim.Adam(ws.parameters())
