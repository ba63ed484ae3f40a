"""The GNN's forward output and packed gradient blob, pinned bit for bit.

``tests/golden/gnn_bits.json`` holds the sha256 of ``lspcg_gnn_forward``'s output and of
``lspcg_gnn_backward``'s gradient blob (cotangent: a seeded normal vector) for descriptors that
reach every branch of the packed-blob layout and of the fragment packer, with the precision the
library chose and the hidden bound it reports.  The hashes were recorded with this file's
``__main__`` block on the commit the fixture names; the Python API it drives (``build_gnn``,
forward, ``_backward``) is the same there, so a refactor of the layout / packer code has to
reproduce them exactly.  The ``out`` hashes of the four fp32 cases were recorded again when the
fp32-MFMA decoder began to add its bias after the products (``fp32_out_recorded_from``).

    python tests/test_gpu_gnn_bits.py --commit <sha> [--out tests/golden/gnn_bits.json]

Graph A: ``poisson2d_grid(9, 8)`` as a block graph (N = 72, row-major sorted and symmetric: the fast
CSC path).  Graph B: the same edges shuffled by a seeded permutation (the generic path: count /
scan / fill / sort, by-source slots in the backward).
"""
import functools
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from learningsparsepreconditioner4gpu_amd import problems as P  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = ROOT / "tests" / "golden" / "gnn_bits.json"
SEED = 11

# (node_in, edge_in, block size, layers, forced f32, scaled W2)
CASES = [
    (1, 1, 1, 4, False, False),    # the plain path
    (1, 1, 1, 4, True, False),     # ... on the fp32-MFMA kernels (LSPCG_GNN_F32=1)
    (4, 9, 3, 1, False, False),    # fused edge encoder, s1e = 3
    (2, 12, 2, 2, False, False),   # the last edge_in whose encoder is fused
    (2, 13, 1, 2, False, False),   # the first that is not
    (17, 17, 1, 1, False, False),  # k_enc<2>; edge_in > 16: no split-f16 encoder block
    (32, 16, 2, 1, True, False),
    (3, 5, 3, 0, False, False),    # no layers: the encoder is not fused, the decoder follows the encoders
    (1, 1, 1, 2, False, True),     # one W2 times 1e6: the library chooses fp32 through the hidden bound
]
ON_B = [CASES[0], CASES[2], CASES[8]]
RUNS = [("A", c) for c in CASES] + [("B", c) for c in ON_B]


def key(graph, case):
    ni, ei, bs, layers, f32, scaled = case
    return f"{graph}/{ni}-{ei}-{bs}-{layers}" + ("-f32" if f32 else "") + ("-w2e6" if scaled else "")


@functools.lru_cache(maxsize=None)
def edges(graph):
    ei = P.to_block_graph(P.poisson2d_grid(9, 8)[0], 1).edge_index
    perm = np.arange(ei.shape[1])
    if graph == "B":
        perm = np.random.default_rng(SEED).permutation(ei.shape[1])
    return torch.from_numpy(np.ascontiguousarray(ei[:, perm]).astype(np.int64)), perm


def inputs(graph, case):
    ni, ein, bs = case[:3]
    ei, perm = edges(graph)
    rng = np.random.default_rng(SEED + 1)
    x = rng.standard_normal((72, ni)).astype(np.float32)
    ea = rng.standard_normal((ei.shape[1], ein)).astype(np.float32)[perm]
    G = rng.standard_normal((ei.shape[1], bs * bs)).astype(np.float32)[perm]
    return torch.from_numpy(x).cuda(), ei.cuda(), torch.from_numpy(ea).cuda(), torch.from_numpy(G).cuda()


def module(case, seed=3):
    from learningsparsepreconditioner4gpu_amd.nn import build_gnn

    ni, ein, bs, layers, _, scaled = case
    gnn = build_gnn(ni, ein, bs, seed=seed, num_mp_layers=layers)
    if scaled:
        with torch.no_grad():
            gnn.mp_layers[0].msg_mlp.body[0][0].weight.mul_(1e6)
    return gnn


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def bits(gnn, graph, case):
    """The record of one run: hashes of the output and the gradient blob, f32, the hidden bound."""
    x, ei, ea, G = inputs(graph, case)
    with torch.no_grad():
        _, out = gnn(x, ei, ea)
    gw = gnn._backward(x, ei, ea, G)
    prec = gnn.precision("cuda")
    return {"out": sha(out), "grad": sha(gw), "f32": prec["f32"], "hidden_bound": float(prec["hidden_bound"]).hex()}


def run(graph, case):
    old = os.environ.pop("LSPCG_GNN_F32", None)
    if case[4]:
        os.environ["LSPCG_GNN_F32"] = "1"  # read when the handle takes its weights
    try:
        return bits(module(case), graph, case)
    finally:
        os.environ.pop("LSPCG_GNN_F32", None)
        if old is not None:
            os.environ["LSPCG_GNN_F32"] = old


def round_trip():
    """Weights X -> Y -> X on one handle: X chooses fp32, Y split-f16 (a larger fragment blob, so
    ``frag`` is regrown).  Returns the three records."""
    old = os.environ.pop("LSPCG_GNN_F32", None)
    try:
        case = CASES[8]
        gnn = module(case)
        X = {k: v.clone() for k, v in gnn.state_dict().items()}
        Y = module(case[:5] + (False,), seed=4).state_dict()
        first = bits(gnn, "A", case)
        handle = gnn._handle.value
        gnn.load_state_dict(Y)
        second = bits(gnn, "A", case)
        gnn.load_state_dict(X)
        third = bits(gnn, "A", case)
        assert gnn._handle.value == handle  # lspcg_gnn_set_weights, not a new handle
        return first, second, third
    finally:
        if old is not None:
            os.environ["LSPCG_GNN_F32"] = old


@functools.lru_cache(maxsize=None)
def fixture():
    return json.loads(FIXTURE.read_text())


@pytest.mark.parametrize("graph,case", RUNS, ids=[key(g, c) for g, c in RUNS])
def test_bits(gpu_ctx, graph, case):
    got, want = run(graph, case), fixture()["cases"][key(graph, case)]
    print(key(graph, case), got)
    assert got["f32"] == (case[4] or case[5])
    assert got == want


def test_set_weights_round_trip(gpu_ctx):
    first, second, third = round_trip()
    want = fixture()
    assert first["f32"] and not second["f32"]
    assert first == want["cases"][key("A", CASES[8])]
    assert second == want["round_trip_y"]
    assert third == first


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit this checkout is (written into the fixture)")
    ap.add_argument("--out", default=str(FIXTURE))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the recorder needs the MI355X"
    doc = {"recorded_from": args.commit, "cases": {key(g, c): run(g, c) for g, c in RUNS}}
    x, y, x2 = round_trip()
    assert x == doc["cases"][key("A", CASES[8])] and x2 == x, (x, x2)
    doc["round_trip_y"] = y
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))
