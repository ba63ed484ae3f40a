"""Shared cases of the GNN forward / backward shape tests (no tests in this file).

``tests/test_gnn_cases_host.py`` (CPU) proves that the inputs built here reach the states they are
built for and that the fp64 oracle resolves them; ``tests/test_gpu_gnn_shapes.py`` runs the HIP
kernels on them.

Metric.  The GNN's output varies little from edge to edge at the seeded initialisation, so an error
relative to ``max(1, max|want|)`` accepts far more than the output carries.  ``spread_error`` scales
the error of output column c by the column's own spread ``max_e want - min_e want``.

Bound.  ``bound(r32) = max(1e-5, 4 r32)`` with ``r32`` the same metric for the oracle run in fp32 on
the CPU: the floor is the north star (BASELINE.json), the margin of 4 over the fp32 restatement is
the convention of ``check_grads`` and tests/test_gpu_loss.py.  The reference is always
``copy.deepcopy(oracle).double()``.

Weights.  At the seeded initialisation the output hardly depends on the aggregation (one of a hub's
600 incoming edges removed moves the other edges by 1e-5 .. 4e-5 of the spread); ``scaled(model, 3)``
gives trained-like O(10) outputs at which it does (3e-4 .. 5e-4).

Structure graphs.  ``k_mp_layer`` gives one workgroup 256 destination nodes and their CSC slots
``[k0, k1)``, walks them in 16-edge tiles (wave w: tiles w, w + 4, ...; prefetches clamped to
``k1 - 1``) and sums the messages per 256-slot chunk.  The graphs below are built from per-node
in-degree lists so that named states of that split occur; ``states`` names, from the CSC layout
alone, which of them a graph reaches.
"""
import copy
import functools

import numpy as np
import torch

from oracle import gnn as OG
from learningsparsepreconditioner4gpu_amd import problems as P
from tests.test_gpu_gnn_bits import CASES as BITS_CASES
from tests.test_gpu_gnn_bits import SEED as BITS_SEED

WG = 256     # destination nodes of one k_mp_layer workgroup
TILE = 16    # edges of one MFMA tile
CHUNK = 256  # CSC slots of one LDS chunk (CE)
SEED = 3     # of the oracle / GPU module pair

FLOOR = 1e-5


# ---- weights, metric, bound ---------------------------------------------------------------------
def scaled(model, gain):
    """Every 2-D ``Linear.weight`` of an oracle or GPU module times ``gain`` (in place)."""
    if gain != 1:
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, torch.nn.Linear):
                    m.weight.mul_(gain)
    return model


def column_spread(want64):
    w = np.asarray(want64, dtype=np.float64)
    w = w.reshape(w.shape[0], -1)
    return w.max(0) - w.min(0)


def spread_error(got, want64, rows=None):
    """max over the output columns c of ``max_e |got - want| / (max_e want - min_e want)``.
    ``rows``: the error is taken over these edges only (the spread is the whole column's)."""
    w = np.asarray(want64, dtype=np.float64)
    w = w.reshape(w.shape[0], -1)
    g = np.asarray(got, dtype=np.float64).reshape(w.shape)
    err = np.abs(g - w)
    if rows is not None:
        err = err[rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float((err.max(0) / column_spread(w)).max())


def bound(r32):
    return max(FLOOR, 4 * r32)


# ---- descriptors ----------------------------------------------------------------------------------
# (node_in, edge_in, block size, layers, residuals)
ADDED = [
    (1, 4, 1, 2, True), (1, 5, 2, 2, True), (3, 8, 2, 1, True), (2, 9, 2, 1, True),  # S1E steps 1 -> 2 -> 3
    (16, 1, 1, 1, True), (17, 1, 2, 1, True), (32, 32, 3, 2, True),  # encoder K steps; the backward's k_enc<2>
    (2, 6, 2, 2, False),  # residuals off
]
DESCRIPTORS = list(dict.fromkeys([c[:4] + (True,) for c in BITS_CASES])) + ADDED
STRUCT_DESCRIPTORS = [(1, 1, 1, 4, True), (2, 6, 2, 2, True)]
UNFUSED = (5, 17, 1, 2, True)  # on `chunks`: k_encode<true> gathers through perm
GAINS = (1, 3)


def gains(desc):
    """The gains a descriptor runs at on the N = 72 graphs.  Without residuals the seeded
    initialisation gives an almost constant output (over 7 module and 3 input seeds: smallest column
    spread 5e-4 .. 4e-3 of max|want|, fp32 oracle error 1.3e-5 .. 1.2e-4 of it), which no seed brings
    over the input caps of tests/test_gnn_cases_host.py; 1.5 is the lower gain for that descriptor
    (spread 9e-2, r32 1e-6)."""
    return GAINS if desc[4] else (1.5, 3)


STRUCT_GAIN = 3  # the gain at which every named state reaches 10 x the bound (test_gnn_cases_host.py)


def desc_id(d):
    return "-".join(str(v) for v in d[:4]) + ("" if d[4] else "-nores")


def oracle(desc, gain):
    ni, ein, bs, layers, res = desc
    return scaled(OG.build(ni, ein, bs, seed=SEED, num_mp_layers=layers, node_residual=res, edge_residual=res), gain)


def gpu_module(desc, gain, differentiable=False):
    from learningsparsepreconditioner4gpu_amd.nn import build_gnn

    ni, ein, bs, layers, res = desc
    return scaled(build_gnn(ni, ein, bs, seed=SEED, differentiable=differentiable, num_mp_layers=layers,
                            node_residual=res, edge_residual=res), gain)


# ---- graphs ---------------------------------------------------------------------------------------
def from_in_degrees(deg, seed, pool=None, forced=None, shuffle=True):
    """Directed edges ``[2, E]`` (row 0 the source): destination i receives ``deg[i]`` edges from
    distinct sources drawn from ``pool`` (default: every node); ``forced[i]`` are sources it must
    have.  Shuffled by the same generator."""
    rng = np.random.default_rng(seed)
    n = len(deg)
    pool = np.arange(n) if pool is None else np.asarray(pool)
    forced = forced or {}
    src, dst = [], []
    for i, d in enumerate(deg):
        if d == 0:
            continue
        must = np.asarray(forced.get(i, []), dtype=np.int64)
        assert len(must) <= d and len(set(must.tolist())) == len(must)
        rest = pool[~np.isin(pool, must)]
        s = np.concatenate([must, rng.choice(rest, d - len(must), replace=False)])
        src.append(s)
        dst.append(np.full(d, i, dtype=np.int64))
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    if shuffle:
        ei = ei[:, rng.permutation(ei.shape[1])]
    return ei


def symmetrised(ei):
    """Sorted row-major, duplicate free, with every edge's reverse: the fast CSC path."""
    return np.unique(np.concatenate([ei, ei[::-1]], axis=1), axis=1)


TILE_EDGES = (63, 64, 65, 127, 128, 129, 255, 256, 257)

# `chunks`: the in-degrees of the second workgroup's first nodes, in slot order relative to its k0
CHUNKS_N = 900
CHUNKS_WG2 = {256: 250, 257: 12, 258: 250, 259: 0, 260: 100, 261: 0, 262: 600, 263: 0}
CHUNKS_CROSSING, CHUNKS_ENDS512, CHUNKS_HUB, CHUNKS_OUT_HUB = 257, 258, 262, 700
CHUNKS_ZEROS = (261, 263)


def _chunks_directed():
    n = CHUNKS_N
    rng = np.random.default_rng(41)
    deg = np.ones(n, dtype=np.int64)
    deg[250:256] = 0  # k0 of the second workgroup = 250, no multiple of 16
    deg[256:512] = 0
    for i, d in CHUNKS_WG2.items():
        deg[i] = d
    outside = np.concatenate([np.arange(0, 256), np.arange(512, n)])  # no source in the second workgroup
    loops = (520, 640, 899)  # self loops
    # CHUNKS_OUT_HUB sends to 600 destinations outside the second workgroup (k_gather's by-source slots)
    has = outside[deg[outside] > 0]
    to = rng.choice(has[~np.isin(has, loops + (CHUNKS_OUT_HUB,))], 600, replace=False)
    forced = {int(i): [CHUNKS_OUT_HUB] for i in to}
    forced.update({i: [i] for i in loops})
    ei = from_in_degrees(deg, 42, pool=outside, forced=forced, shuffle=False)
    dup = np.flatnonzero(ei[1] >= 600)[[3, 70, 201, 250, 9]]  # five duplicated edges, into nodes past the hub
    ei = np.concatenate([ei, ei[:, dup]], axis=1)
    return ei[:, rng.permutation(ei.shape[1])]


@functools.lru_cache(maxsize=None)
def structure_graph(name):
    """``(edge_index [2, E] int64 numpy, N)`` of a structure graph version."""
    if name == "one-node":
        return np.zeros((2, 1), dtype=np.int64), 1
    if name == "few-tiles":
        deg = np.zeros(513, dtype=np.int64)
        deg[[3, 17, 40, 41, 100, 180, 255]] = [2, 1, 4, 3, 1, 2, 2]  # 15 edges: one partial tile
        deg[512] = 33  # three tiles (one wave idle); the last workgroup owns this node alone
        return from_in_degrees(deg, 5), 513
    if name == "first-empty":
        deg = np.zeros(300, dtype=np.int64)
        deg[256:] = 3 + (np.arange(44) % 5)
        # the nodes of the second workgroup also send to each other, so they have outgoing edges
        return from_in_degrees(deg, 6, pool=np.arange(200, 300)), 300
    if name.startswith("tile-edges["):
        m = int(name[len("tile-edges["):-1])
        deg = np.full(256, m // 256, dtype=np.int64)
        deg[:m % 256] += 1
        last = int(np.flatnonzero(deg)[-1])  # the destination of the last slot: it also sends to node 0
        return from_in_degrees(deg, 7 + m, forced={0: [last]}), 256
    if name == "chunks":
        return _chunks_directed(), CHUNKS_N
    if name == "chunks-sym":
        return symmetrised(_chunks_directed()), CHUNKS_N
    raise KeyError(name)


STRUCTURE = ["one-node", "few-tiles", "first-empty"] + [f"tile-edges[{m}]" for m in TILE_EDGES] + ["chunks", "chunks-sym"]
FAST_PATH = {"one-node", "chunks-sym", "grid"}  # strictly row-major sorted with a symmetric pattern


@functools.lru_cache(maxsize=None)
def graph(name):
    """Structure graphs and the two N = 72 graphs of tests/test_gpu_gnn_bits.py (``grid``: the fast
    path, ``grid-shuffled``: the generic one)."""
    if name in ("grid", "grid-shuffled"):
        ei = P.to_block_graph(P.poisson2d_grid(9, 8)[0], 1).edge_index.astype(np.int64)
        if name == "grid-shuffled":
            ei = ei[:, np.random.default_rng(BITS_SEED).permutation(ei.shape[1])]
        return np.ascontiguousarray(ei), 72
    return structure_graph(name)


def forward_combinations():
    """(graph, descriptor, gain) of every forward run of tests/test_gpu_gnn_shapes.py."""
    out = [(g, d, gain) for g in ("grid", "grid-shuffled") for d in DESCRIPTORS for gain in gains(d)]
    for g in STRUCTURE:
        out += [(g, d, STRUCT_GAIN) for d in STRUCT_DESCRIPTORS]
        if g.startswith("chunks"):
            out.append((g, UNFUSED, STRUCT_GAIN))
    return out


# ---- predicates on the CSC layout -----------------------------------------------------------------
def csc_ptr(ei, n):
    """``ptr`` by destination: node i owns the CSC slots ``[ptr[i], ptr[i + 1])``."""
    return np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=n))]).astype(np.int64)


def workgroups(ptr, n):
    """Per k_mp_layer workgroup: its nodes ``[n0, n1)``, slots ``[k0, k1)``, tile count NT and chunk ranges."""
    out = []
    for n0 in range(0, n, WG):
        n1 = min(n0 + WG, n)
        k0, k1 = int(ptr[n0]), int(ptr[n1])
        nt = (k1 - k0 + TILE - 1) // TILE
        chunks = [(k0 + c * CHUNK, min(k0 + (c + 1) * CHUNK, k1)) for c in range((nt + 15) // 16)]
        out.append(dict(n0=n0, n1=n1, k0=k0, k1=k1, NT=nt, chunks=chunks))
    return out


def is_fast_path(ei, n):
    """Strictly row-major sorted (so duplicate free) with a symmetric pattern: k_csc_rowstart / k_csc_sym."""
    key = ei[0] * n + ei[1]
    if not np.all(np.diff(key) > 0):
        return False
    return np.array_equal(np.sort(ei[1] * n + ei[0]), key)


def states(ei, n):
    """The names of the work-split states the graph reaches (see the module docstring)."""
    ptr = csc_ptr(ei, n)
    s = set()
    if n == 1:
        s.add("N=1")
    for g, w in enumerate(workgroups(ptr, n)):
        k0, k1, nt = w["k0"], w["k1"], w["NT"]
        s.add(f"NT={nt}")
        if k1 == k0:
            s.add("empty-workgroup")
            if g == 0:
                s.add("first-workgroup-empty")  # klast = -1
            elif k0 < ptr[-1]:
                s.add("empty-workgroup-in-the-middle")
        elif nt < 4:
            s.add("fewer-than-4-tiles")
        if k1 > k0 and (k1 - k0) % TILE:
            s.add("partial-last-tile")
        if k1 > k0 and (k1 - k0) % TILE == 0:
            s.add("full-last-tile")
        if w["n1"] - w["n0"] == 1:
            s.add("one-node-workgroup")
        if k0 != 0 and k1 > k0:
            s.add("k0-nonzero")
        for i in range(w["n0"], w["n1"]):
            a, b = int(ptr[i]), int(ptr[i + 1])
            if a == b:
                continue
            if a < k0 + 256 < b:
                s.add("range-crosses-k0+256")
            if b == k0 + 512:
                s.add("range-ends-at-k0+512")
            for c0, c1 in w["chunks"]:
                if a <= c0 and b >= c1 and c1 - c0 == CHUNK:
                    s.add("node-fills-a-chunk")
                if k0 < c0 == a or b == c1 < k1:
                    s.add("chunk-boundary-on-node-boundary")
    return s


# ---- inputs and references (built once, never modified) -------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(gname, ni, ein):
    """``(x [N, ni], edge_index, edge_attr [E, ein])`` as CPU tensors, seeded by the sizes."""
    ei, n = graph(gname)
    rng = np.random.default_rng([BITS_SEED + 1, ni, ein])
    x = rng.standard_normal((n, ni)).astype(np.float32)
    ea = rng.standard_normal((ei.shape[1], ein)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(ei.copy()), torch.from_numpy(ea)


def oracle_forward(model, x, ei, ea, dtype):
    m = copy.deepcopy(model).to(dtype)
    with torch.no_grad():
        return m(x.to(dtype), ei, ea.to(dtype))[1].double().numpy()


@functools.lru_cache(maxsize=None)
def reference(gname, desc, gain):
    """``(want64, r32, smin)``: the fp64 oracle's output, the fp32 oracle's spread error and the
    smallest column spread over ``max|want|``."""
    x, ei, ea = inputs(gname, desc[0], desc[1])
    model = oracle(desc, gain)
    want = oracle_forward(model, x, ei, ea, torch.float64)
    got32 = oracle_forward(model, x, ei, ea, torch.float32)
    want.setflags(write=False)
    if want.shape[0] < 2:
        return want, 0.0, float("nan")  # one edge: no spread; compared with the 1e-5 floor of its magnitude
    return want, spread_error(got32, want), float(column_spread(want).min() / np.abs(want).max())


def forward_error(got, gname, desc, gain, rows=None):
    """``(err, r32, bound)`` of a kernel output.  A one-edge graph has no spread: its error is taken
    relative to ``max|want|`` and r32 likewise."""
    want, r32, _ = reference(gname, desc, gain)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    if want.shape[0] < 2:
        x, ei, ea = inputs(gname, desc[0], desc[1])
        got32 = oracle_forward(oracle(desc, gain), x, ei, ea, torch.float32)
        scale = float(np.abs(want).max())
        r32 = float(np.abs(got32 - want).max()) / scale
        return float(np.abs(got - want).max()) / scale, r32, bound(r32)
    return spread_error(got, want, rows), r32, bound(r32)


def edges_at(gname, node):
    """The edges into and out of ``node`` (indices into edge_index's columns)."""
    ei, _ = graph(gname)
    return np.flatnonzero((ei[0] == node) | (ei[1] == node))


# The node that embodies each named state, per structure graph: (state, node).
def named_nodes(gname):
    ei, n = graph(gname)
    ptr = csc_ptr(ei, n)
    if gname == "few-tiles":
        return [("the one partial tile of the first workgroup (NT = 1)", 40),
                ("the lone node of the last workgroup (NT = 3, one wave idle)", 512)]
    if gname == "first-empty":
        return [("the first node with edges, after an empty first workgroup", 256),
                ("the last node", 299)]
    if gname.startswith("tile-edges"):
        return [("the destination of the last tile's last slot", int(np.flatnonzero(np.diff(ptr))[-1]))]
    if gname.startswith("chunks"):
        return [("range crosses k0 + 256", CHUNKS_CROSSING), ("range ends at k0 + 512", CHUNKS_ENDS512),
                ("600 incoming edges: fills a whole chunk, parts of two others", CHUNKS_HUB),
                ("600 outgoing edges", CHUNKS_OUT_HUB)]
    return []


def without_one_edge_into(gname, node):
    """The graph's inputs with the first incoming edge of ``node`` removed: (keep mask, removed edge)."""
    ei, _ = graph(gname)
    e = int(np.flatnonzero(ei[1] == node)[0])
    keep = np.ones(ei.shape[1], dtype=bool)
    keep[e] = False
    return keep, e


def sensitivity(gname, desc, gain, node):
    """How far the fp64 oracle's output on the OTHER edges moves, in the spread metric, when one
    incoming edge of ``node`` is removed."""
    want, _, _ = reference(gname, desc, gain)
    x, ei, ea = inputs(gname, desc[0], desc[1])
    keep, _ = without_one_edge_into(gname, node)
    k = torch.from_numpy(keep)
    moved = oracle_forward(oracle(desc, gain), x, ei[:, k], ea[k], torch.float64)
    w = want.reshape(want.shape[0], -1)[keep]
    return float((np.abs(moved.reshape(w.shape) - w).max(0) / column_spread(want)).max())
