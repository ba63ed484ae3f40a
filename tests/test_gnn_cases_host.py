"""The inputs of tests/test_gpu_gnn_shapes.py, checked on the CPU (tests/_gnn_cases.py builds them).

Every cap here is a condition on the INPUTS: a structure graph reaches the work-split states it is
built for, every output column of the fp64 oracle has a spread the metric can divide by, the fp32
oracle is close enough that no bound exceeds 2e-5, and the output depends on the aggregation at
every named state (one incoming edge removed moves some other edge by 10 x the bound).  An input
that misses a cap gets another seed or size; the caps and the metric stay.

Gain used for the structure graphs: 3 (``STRUCT_GAIN``); every named state reaches 10 x the bound there.
"""
import numpy as np
import pytest

from tests import _gnn_cases as C

SPREAD_MIN = 1e-2  # of max|want|, per column
R32_MAX = 5e-6     # so that bound = max(1e-5, 4 r32) <= 2e-5
SENSITIVITY = 10   # times the bound

PROMISED = {
    "one-node": {"N=1", "NT=1", "one-node-workgroup", "fewer-than-4-tiles"},
    "few-tiles": {"NT=1", "NT=0", "NT=3", "fewer-than-4-tiles", "empty-workgroup", "empty-workgroup-in-the-middle",
                  "one-node-workgroup", "partial-last-tile", "k0-nonzero"},
    "first-empty": {"first-workgroup-empty", "empty-workgroup", "NT=0"},
    "tile-edges[63]": {"NT=4", "partial-last-tile"}, "tile-edges[64]": {"NT=4", "full-last-tile"},
    "tile-edges[65]": {"NT=5", "partial-last-tile"}, "tile-edges[127]": {"NT=8", "partial-last-tile"},
    "tile-edges[128]": {"NT=8", "full-last-tile"}, "tile-edges[129]": {"NT=9", "partial-last-tile"},
    "tile-edges[255]": {"NT=16", "partial-last-tile"}, "tile-edges[256]": {"NT=16", "full-last-tile"},
    "tile-edges[257]": {"NT=17", "partial-last-tile", "chunk-boundary-on-node-boundary"},
    "chunks": {"k0-nonzero", "range-crosses-k0+256", "range-ends-at-k0+512", "node-fills-a-chunk",
               "chunk-boundary-on-node-boundary"},
    "chunks-sym": {"k0-nonzero", "range-crosses-k0+256", "range-ends-at-k0+512", "node-fills-a-chunk",
                   "chunk-boundary-on-node-boundary"},
}


COMBOS = C.forward_combinations()
combo_id = lambda c: f"{c[0]}/{C.desc_id(c[1])}/gain{c[2]}"


def test_descriptor_grid_holds_every_hashed_descriptor():
    from tests.test_gpu_gnn_bits import CASES

    assert {c[:4] for c in CASES} <= {d[:4] for d in C.DESCRIPTORS}
    assert set(C.ADDED) <= set(C.DESCRIPTORS) and len(set(C.DESCRIPTORS)) == len(C.DESCRIPTORS)


@pytest.mark.parametrize("name", C.STRUCTURE)
def test_graph_states(name):
    ei, n = C.graph(name)
    assert ei.dtype == np.int64 and ei.shape[0] == 2 and ei.min() >= 0 and ei.max() < n
    got = C.states(ei, n)
    fast = C.is_fast_path(ei, n)
    print(f"{name}: N {n} E {ei.shape[1]} fast path {fast} states {sorted(got)}")
    assert PROMISED[name] <= got, sorted(PROMISED[name] - got)
    assert fast == (name in C.FAST_PATH)
    assert n <= 1000 and ei.shape[1] <= 4000


def test_graph_contents():
    """What the descriptions promise beyond the states."""
    ei, n = C.graph("few-tiles")
    indeg = np.bincount(ei[1], minlength=n)
    assert indeg[:256].sum() == 15 and indeg[256:512].sum() == 0 and indeg[512] == 33
    ei, n = C.graph("first-empty")
    indeg = np.bincount(ei[1], minlength=n)
    assert indeg[:256].sum() == 0 and indeg[256:].min() > 0
    for m in C.TILE_EDGES:
        ei, n = C.graph(f"tile-edges[{m}]")
        indeg = np.bincount(ei[1], minlength=n)
        assert ei.shape[1] == m and indeg.max() - indeg.min() <= 1
    assert sorted({m % 16 for m in C.TILE_EDGES}) == [0, 1, 15]
    for name in ("chunks", "chunks-sym"):
        ei, n = C.graph(name)
        ptr = C.csc_ptr(ei, n)
        k0 = int(ptr[256])
        rel = lambda i: (int(ptr[i]) - k0, int(ptr[i + 1]) - k0)
        assert k0 != 0
        a, b = rel(C.CHUNKS_CROSSING)
        assert a < 256 < b
        assert rel(C.CHUNKS_ENDS512)[1] == 512
        a, b = rel(C.CHUNKS_HUB)
        assert b - a == 600 and a % 256 != 0 and b % 256 != 0  # one whole chunk, parts of two others
        assert any(a <= c0 and c0 + 256 <= b for c0 in range(0, b, 256))
        for z in C.CHUNKS_ZEROS:
            assert ptr[z] == ptr[z + 1]
        assert C.CHUNKS_ZEROS[0] < C.CHUNKS_HUB < C.CHUNKS_ZEROS[1]
        assert np.bincount(ei[0], minlength=n)[C.CHUNKS_OUT_HUB] >= 600
        assert (ei[0] == ei[1]).sum() >= 3
        dup = ei.shape[1] - np.unique(ei, axis=1).shape[1]
        assert dup == (5 if name == "chunks" else 0)
    # sources are distinct per destination in the directed builder
    ei = C.from_in_degrees(np.array([3, 0, 5, 2, 4, 4]), 1)
    assert np.unique(ei, axis=1).shape[1] == ei.shape[1] == 18


@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_column_spread_and_fp32_oracle(combo):
    gname, desc, gain = combo
    want, r32, smin = C.reference(gname, desc, gain)
    print(f"{combo_id(combo)}: r32 {r32:.3e} bound {C.bound(r32):.3e} min column spread / max|want| {smin:.3e} "
          f"max|want| {np.abs(want).max():.3e}")
    assert np.isfinite(want).all()
    if want.shape[0] < 2:
        return  # one edge: no spread (C.forward_error compares it at the 1e-5 floor of its magnitude)
    assert smin >= SPREAD_MIN, smin
    assert r32 <= R32_MAX, r32


SENS = [(g, d, C.STRUCT_GAIN, state, node) for g, d, _ in COMBOS if g in C.STRUCTURE
        for state, node in C.named_nodes(g)]


@pytest.mark.parametrize("case", SENS, ids=lambda c: f"{c[0]}/{C.desc_id(c[1])}/node{c[4]}")
def test_sensitivity(case):
    """One incoming edge of the state's node removed in the fp64 oracle moves some other edge's
    output by at least 10 x the bound."""
    gname, desc, gain, state, node = case
    _, r32, _ = C.reference(gname, desc, gain)
    s = C.sensitivity(gname, desc, gain, node)
    print(f"{gname}/{C.desc_id(desc)}/gain{gain} node {node} ({state}): sensitivity {s:.3e} = "
          f"{s / C.bound(r32):.1f} x bound {C.bound(r32):.3e}")
    assert s >= SENSITIVITY * C.bound(r32), (s, C.bound(r32))
