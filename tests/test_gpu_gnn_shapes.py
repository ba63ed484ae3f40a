"""HIP GNN forward and backward vs the fp64 oracle at the descriptors and graph shapes of
tests/_gnn_cases.py (tests/test_gnn_cases_host.py proves on the CPU that those inputs reach the
states they are built for).

Forward: ``spread_error(got, want64) <= max(1e-5, 4 r32)`` -- the error of every output column
relative to the column's own spread, ``r32`` the fp32 oracle's -- for the default (split-f16)
kernels and the fp32-MFMA kernels (LSPCG_GNN_F32=1), at the seeded weights and with every
Linear.weight times 3 (trained-like outputs, at which the aggregation shows in the output).
Backward: ``check_grads`` of tests/test_gpu_gnn_backward.py, its bound unchanged.

Every test prints its measured error, r32 and the bound.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _gnn_cases as C
from tests.test_gpu_gnn_backward import check_grads, cotangent, gpu_grads, oracle_grads

pytestmark = pytest.mark.gpu

KERNELS = ["f16", "f32"]  # the library's choice (split-f16 for these weights) / LSPCG_GNN_F32=1


def forward(monkeypatch, gname, desc, gain, kernels):
    """``(out, precision)`` of a fresh module on the graph's inputs."""
    if kernels == "f32":
        monkeypatch.setenv("LSPCG_GNN_F32", "1")  # read when the handle takes its weights
    else:
        monkeypatch.delenv("LSPCG_GNN_F32", raising=False)
    gnn = C.gpu_module(desc, gain)
    x, ei, ea = C.inputs(gname, desc[0], desc[1])
    with torch.no_grad():
        _, out = gnn(x.cuda(), ei.cuda(), ea.cuda())
    return out.cpu().numpy(), gnn.precision("cuda")


def check_forward(got, prec, gname, desc, gain, kernels):
    err, r32, bnd = C.forward_error(got, gname, desc, gain)
    print(f"FWD {gname} {C.desc_id(desc)} gain{gain} {kernels}: err {err:.3e} r32 {r32:.3e} bound {bnd:.3e} "
          f"f32 {prec['f32']} hidden_bound {prec['hidden_bound']:.4g}")
    assert np.isfinite(got).all()
    assert prec["f32"] == (kernels == "f32"), prec  # these weights stay on the split-f16 kernels by default
    assert err <= bnd, (err, r32, bnd)


GRID = [(g, d, gain) for g, d, gain in C.forward_combinations() if g.startswith("grid")]
STRUCT = [(g, d, gain) for g, d, gain in C.forward_combinations() if not g.startswith("grid")]
combo_id = lambda c: f"{c[0]}/{C.desc_id(c[1])}/gain{c[2]}"


# ---- 1. forward, descriptors ----------------------------------------------------------------------
@pytest.mark.parametrize("kernels", KERNELS)
@pytest.mark.parametrize("combo", GRID, ids=combo_id)
def test_forward_descriptors(gpu_ctx, monkeypatch, combo, kernels):
    """Measured on the MI355X: every case at gain 3 (and 1.5) is at most 0.29 of its bound; at gain 1
    the split-f16 kernels sit at 0.1 .. 0.94 of it and the fp32-MFMA kernels at 0.1 .. 0.75.

    This test found the fp32-MFMA decoder accumulating its four output MFMA steps onto the bias.  At
    the seeded weights the bias is the bulk of the output (max|want| 0.30, column spread 0.0087), so
    every step rounded at the bias's magnitude: grid/2-9-2-1/gain1-f32 gave 1.169e-05 against a bound
    of 1.081e-05, grid/4-9-3-1/gain1-f32 9.202e-06 against 1e-05.  With the bias added after the
    products (k_edge_dec<true, ...>) they give 6.291e-06 and 7.487e-06.  The split-f16 decoder still
    accumulates onto its bias (0.94 of the bound at grid/4-9-3-1/gain1); changing it changes every
    hashed output of test_gpu_gnn_bits.py."""
    gname, desc, gain = combo
    got, prec = forward(monkeypatch, gname, desc, gain, kernels)
    check_forward(got, prec, gname, desc, gain, kernels)


# ---- 2. forward, structure ------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", KERNELS)
@pytest.mark.parametrize("combo", STRUCT, ids=combo_id)
def test_forward_structure(gpu_ctx, monkeypatch, combo, kernels):
    gname, desc, gain = combo
    got, prec = forward(monkeypatch, gname, desc, gain, kernels)
    for state, node in C.named_nodes(gname):  # first: a failure names the node and its state
        rows = C.edges_at(gname, node)
        err, r32, bnd = C.forward_error(got, gname, desc, gain, rows)
        print(f"FWDNODE {gname} {C.desc_id(desc)} gain{gain} {kernels} node {node} ({state}; {len(rows)} edges): "
              f"err {err:.3e} r32 {r32:.3e} bound {bnd:.3e}")
        assert len(rows) > 0 and err <= bnd, f"{gname}: edges into / out of node {node} ({state}): {err} > {bnd}"
    check_forward(got, prec, gname, desc, gain, kernels)


# ---- 3. one handle across graphs ------------------------------------------------------------------
def test_one_handle_across_graphs(gpu_ctx, monkeypatch):
    """A large graph, N = 1, a one-workgroup graph and the large one again on one module: the
    workspace is kept (lspcg_gnn's capacities), the CSC re-analysed; every output has the bits of a
    fresh module's, and the handle stays."""
    monkeypatch.delenv("LSPCG_GNN_F32", raising=False)
    desc, gain = C.STRUCT_DESCRIPTORS[1], C.STRUCT_GAIN
    order = ["chunks", "one-node", "tile-edges[257]", "chunks-sym", "chunks"]
    dev = {g: tuple(t.cuda() for t in C.inputs(g, desc[0], desc[1])) for g in set(order)}
    fresh = {}
    for g in dev:
        with torch.no_grad():
            fresh[g] = C.gpu_module(desc, gain)(*dev[g])[1].clone()
    gnn = C.gpu_module(desc, gain)
    handle = None
    for g in order:
        with torch.no_grad():
            _, out = gnn(*dev[g])
        handle = gnn._handle.value if handle is None else handle
        err, r32, bnd = C.forward_error(out.cpu().numpy(), g, desc, gain)
        print(f"HANDLE {g}: err {err:.3e} r32 {r32:.3e} bound {bnd:.3e}")
        assert torch.equal(out, fresh[g]), g
        assert gnn._handle.value == handle
        assert err <= bnd, (g, err, bnd)


# ---- 4. backward ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grads_reference(gname, desc, gain):
    x, ei, ea = C.inputs(gname, desc[0], desc[1])
    G = cotangent(ei.shape[1], desc[2] ** 2)
    model = C.oracle(desc, gain)
    want = oracle_grads(model, x, ei, ea, G, torch.float64)
    g32 = oracle_grads(model, x, ei, ea, G, torch.float32)
    return G, want, g32


BACKWARD = [(g, d, gain) for g in ("grid", "grid-shuffled") for d in C.ADDED for gain in C.gains(d)] + \
           [(g, C.STRUCT_DESCRIPTORS[1], C.STRUCT_GAIN) for g in ("few-tiles", "first-empty", "one-node", "chunks",
                                                                  "chunks-sym")]


@pytest.mark.parametrize("combo", BACKWARD, ids=combo_id)
def test_backward(gpu_ctx, monkeypatch, combo):
    monkeypatch.delenv("LSPCG_GNN_F32", raising=False)
    gname, desc, gain = combo
    x, ei, ea = C.inputs(gname, desc[0], desc[1])
    G, want, g32 = grads_reference(gname, desc, gain)
    gnn = C.gpu_module(desc, gain, differentiable=True)
    with torch.no_grad():
        _, plain = gnn(x.cuda(), ei.cuda(), ea.cuda())
    out, got = gpu_grads(gnn, x, ei, ea, G)
    assert not plain.requires_grad and torch.equal(out, plain)  # the differentiable forward is the same call
    err, r32, bnd = C.forward_error(out.cpu().numpy(), gname, desc, gain)
    print(f"BWDFWD {combo_id(combo)}: err {err:.3e} r32 {r32:.3e} bound {bnd:.3e}")
    assert err <= bnd, (err, bnd)
    worst = check_grads(got, want, g32, combo_id(combo))
    print(f"BWD {combo_id(combo)}: worst relative gradient error {worst:.3e}")
