"""Matrices at the edges of the jagged layouts SELL-64J (view kind 17) and SELL-64X (kind 18):
csrc/lspcg_sell.hpp kSellJag / kSellJagX.  Pure numpy / scipy, seeded, each built in well under a
second (CPU-side construction only); tests/test_jagged_cases_host.py asserts that every case has the
property it is named for, tests/test_gpu_jagged.py runs them on the device.

Every matrix is a scalar CSR with sorted rows, distinct columns per row and nonzero fp64 values; a
caller that needs fp32-representable values rounds them (f32_exact)."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

SLICE, TILE, XBLK, XMAX = 64, 256, 16, 256  # rows per slice / tile, x entries per staged block, blocks per tile
SWEEP_N = 64 * SLICE + 37
SIZES = (63, 64, 65, 255, 256, 257, 513)


def f32_exact(A: sp.csr_matrix) -> sp.csr_matrix:
    """The same stored arrays with every value rounded through fp32."""
    return sp.csr_matrix((A.data.astype(np.float32).astype(np.float64), A.indices.copy(), A.indptr.copy()),
                         shape=A.shape)


def stored_order(A: sp.csr_matrix, seed: int = 2) -> sp.csr_matrix:
    """Every third row in a shuffled stored order (for DeviceMatrix.from_scipy(keep_order=True))."""
    rng = np.random.default_rng(seed)
    idx, dat = A.indices.copy(), A.data.copy()
    for i in range(0, A.shape[0], 3):
        a, b = A.indptr[i], A.indptr[i + 1]
        p = a + rng.permutation(b - a)
        idx[a:b], dat[a:b] = A.indices[p], A.data[p]
    B = sp.csr_matrix((dat, idx, A.indptr.copy()), shape=A.shape)
    B.has_sorted_indices = False
    return B


def tile_blocks(A: sp.csr_matrix) -> np.ndarray:
    """Distinct 16-entry x blocks each 256-row tile reads (0 for a tile without entries)."""
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr)).astype(np.int64)
    key = np.unique((rows // TILE) * (1 << 32) + A.indices.astype(np.int64) // XBLK)
    return np.bincount(key >> 32, minlength=(n + TILE - 1) // TILE)


def group_counts(A: sp.csr_matrix) -> np.ndarray:
    """[slices, 16]: cnt_q, the rows of each 64-row slice that reach 4-entry group q."""
    n = A.shape[0]
    ns = (n + SLICE - 1) // SLICE
    g = np.zeros(ns * SLICE, dtype=np.int64)
    g[:n] = (np.diff(A.indptr) + 3) // 4
    return (g.reshape(ns, SLICE)[:, :, None] > np.arange(16)[None, None, :]).sum(axis=1)


def _csr_from_rows(n: int, cols_of_row, rng) -> sp.csr_matrix:
    """CSR from one sorted column array per row; values uniform in +-[0.25, 1.25)."""
    lens = np.array([len(c) for c in cols_of_row], dtype=np.int64)
    indptr = np.r_[0, np.cumsum(lens)].astype(np.int32)
    indices = (np.concatenate(cols_of_row) if lens.sum() else np.zeros(0)).astype(np.int32)
    data = (0.25 + rng.random(indices.size)) * rng.choice([-1.0, 1.0], indices.size)
    A = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    A.has_sorted_indices = True
    return A


def _near(rng, i: int, n: int, k: int, spread: int) -> np.ndarray:
    """k distinct sorted columns within +-spread of row i."""
    lo, hi = max(0, i - spread), min(n - 1, i + spread)
    return np.sort(lo + rng.choice(hi - lo + 1, size=k, replace=False))


def sweep_lengths(seed: int = 0) -> np.ndarray:
    """Row lengths of sweep(): slice s < 64 has its longest row, s % 64 + 1 entries, on lane (7 s) % 64
    and the others at random lengths 0..longest with at least one empty row -- except every 8th slice,
    whose rows are all equal; the 37-row tail slice has rows of 0..23 entries, the longest on the
    matrix's last row."""
    rng = np.random.default_rng(seed)
    lens = np.zeros(SWEEP_N, dtype=np.int64)
    for s in range(64):
        longest = s % 64 + 1
        if s % 8 == 0:
            lens[SLICE * s:SLICE * (s + 1)] = longest
            continue
        l = rng.integers(0, longest + 1, SLICE)
        lane = (7 * s) % 64
        l[(lane + 1 + int(rng.integers(0, 63))) % 64] = 0
        l[lane] = longest
        lens[SLICE * s:SLICE * (s + 1)] = l
    tail = rng.integers(0, 23, 37)
    tail[5] = 0
    tail[36] = 23
    lens[64 * SLICE:] = tail
    return lens


def sweep(spread: int, seed: int = 0) -> sp.csr_matrix:
    """n = 4133: every group count 1..16 as a slice's longest row, on 64 different lanes, slices whose
    64 rows all reach every group, empty rows; columns distinct and random within +-spread of the row.
    spread 1500: at most (256 + 3000) / 16 x blocks per tile (SELL-64X once its floor is lowered);
    spread 2200: a tile over the 256-block limit (stays SELL-64J)."""
    rng = np.random.default_rng(seed + 1000)
    lens = sweep_lengths(seed)
    return _csr_from_rows(SWEEP_N, [_near(rng, i, SWEEP_N, int(k), spread) for i, k in enumerate(lens)], rng)


def row65() -> sp.csr_matrix:
    """sweep(1500) with one more entry in a 64-entry row (the longest row of slice 63): 65 entries, more
    than the 16 groups a jagged slice counts."""
    A = sweep(1500)
    i = int(np.flatnonzero(np.diff(A.indptr) == 64)[-1])
    row = A.indices[A.indptr[i]:A.indptr[i + 1]]
    new = int(np.setdiff1d(np.arange(max(0, i - 1500), i), row)[-1])
    B = sp.lil_matrix(A)
    B[i, new] = 0.75
    B = sp.csr_matrix(B)
    B.sort_indices()
    assert B.nnz == A.nnz + 1
    return B


def limit(k: int, seed: int = 3) -> sp.csr_matrix:
    """n = 4133; tile 0 (rows 0..255) reads exactly k in {256, 257} distinct x blocks: row r holds
    column 16 r (blocks 0..255) and 0..20 more columns below 4000, row 100 one last entry at column
    4095 (k = 256: block 255 again) or 4101 (k = 257: block 256) -- the only difference between the two
    matrices.  The other tiles: ragged rows of 1..20 entries within +-300 of the row."""
    assert k in (XMAX, XMAX + 1)
    rng = np.random.default_rng(seed)
    n = SWEEP_N
    rows = []
    for r in range(n):
        m = int(rng.integers(0, 21))
        if r < TILE:
            c = np.union1d(rng.choice(4000, size=m, replace=False), [XBLK * r])
            if r == 100:
                c = np.r_[c, 4095 if k == XMAX else 4101]
        else:
            c = _near(rng, r, n, max(m, 1), 300)
        rows.append(c)
    return _csr_from_rows(n, rows, rng)


def sizes(n: int, seed: int = 4) -> sp.csr_matrix:
    """n rows around the slice and tile sizes: ragged rows of 0..20 entries, columns anywhere."""
    rng = np.random.default_rng(seed + n)
    lens = rng.integers(0, 21, n)
    lens[n // 2] = 20
    lens[n - 1] = 17  # the last row (of a partial slice) is a long one
    return _csr_from_rows(n, [np.sort(rng.choice(n, size=int(k), replace=False)) for k in lens], rng)


def holes(variant: str, seed: int = 5) -> sp.csr_matrix:
    """n = 1100 (n % 16 = 12): rows 256..511, a whole tile, and rows 576..639, a slice inside a live
    tile, are empty; the other rows have 0..20 entries.
    "last": columns within +-400 of the row, the largest is n - 1 (the last x block runs past n);
    "boundary": every column below 640 and the largest 639 (xn = 640, a block boundary well below n)."""
    assert variant in ("last", "boundary")
    rng = np.random.default_rng(seed)
    n = 1100
    rows = []
    for i in range(n):
        k = int(rng.integers(0, 21))
        if 256 <= i < 512 or 576 <= i < 640:
            k = 0
        if variant == "last":
            c = _near(rng, i, n, k, 400)
            if i == n - 7:
                c = np.union1d(c, [n - 1])
        else:
            c = np.sort(rng.choice(640, size=k, replace=False))
            if i == 1000:
                c = np.union1d(c, [639])
        rows.append(c)
    return _csr_from_rows(n, rows, rng)


def off16(far: int = 32767, seed: int = 6) -> sp.csr_matrix:
    """n = 40,000, ragged rows of 1..20 entries within +-300 of the row, plus one entry `far` columns
    above its slice's first row (row 100, slice base 64) and one 32767 below (row 39,990, base 39,936).
    far = 32767: 16-bit offsets still fit; 32768: they do not."""
    rng = np.random.default_rng(seed)
    n = 40000
    lens = rng.integers(1, 21, n)
    r = np.repeat(np.arange(n), lens)
    c = np.clip(r + rng.integers(-300, 301, r.size), 0, n - 1)
    r = np.r_[r, 100, 39990]
    c = np.r_[c, 64 + far, 39936 - 32767]
    key = np.unique(r.astype(np.int64) * n + c)  # sorted by (row, column), duplicates dropped
    r, c = key // n, key % n
    data = (0.25 + rng.random(key.size)) * rng.choice([-1.0, 1.0], key.size)
    A = sp.csr_matrix((data, c.astype(np.int32), np.r_[0, np.cumsum(np.bincount(r, minlength=n))].astype(np.int32)),
                      shape=(n, n))
    A.has_sorted_indices = True
    return A


def banded_spd(n: int, spread: int, seed: int = 0, shift: float = 1.0) -> sp.csr_matrix:
    """Symmetric, strictly diagonally dominant (SPD) band with irregular rows (3..30 entries within
    +-spread of the row), a_ii = sum_j |a_ij| + shift, values rounded through fp32: SELL-64 pads more
    than 1.15 x, a 256-row tile reads at most (256 + 2 spread) / 16 + 1 x blocks."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 15, n)
    rows = np.repeat(np.arange(n), lens)
    cols = rows + rng.integers(-spread, spread + 1, rows.size)
    keep = (cols >= 0) & (cols < n) & (cols != rows)
    B = sp.csr_matrix((rng.uniform(-1, 1, int(keep.sum())), (rows[keep], cols[keep])), shape=(n, n))
    B = sp.csr_matrix(B + B.T)
    B.data = B.data.astype(np.float32).astype(np.float64)
    A = sp.csr_matrix(B + sp.diags(np.asarray(abs(B).sum(axis=1)).ravel() + shift))
    A.sum_duplicates()
    A.sort_indices()
    A.data = A.data.astype(np.float32).astype(np.float64)
    return A


HUB_TARGETS = (61, 62, 63, 64)


def hub_rows(n: int):
    """The four hub rows of hub_spd(n): more than 2 x 300 rows apart, on lanes 1, 22, 43 and 63."""
    return [(k * n // 9) // SLICE * SLICE + lane for k, lane in ((1, 1), (3, 22), (5, 43), (7, 63))]


def hub_spd(n: int = 4500, exact32: bool = True, seed: int = 7) -> sp.csr_matrix:
    """Symmetric, strictly diagonally dominant system of irregular rows (3..30 entries within +-300 of
    the row) in which symmetric couplings bring four hub rows to exactly 61, 62, 63 and 64 entries (the
    diagonal included): the last four bytes of the 16-byte group-count register are in use.
    exact32: every value fp32-representable; else full fp64 values that fp32 cannot hold."""
    rng = np.random.default_rng(seed + n)
    lens = rng.integers(1, 15, n)
    rows = np.repeat(np.arange(n), lens)
    cols = rows + rng.integers(-300, 301, rows.size)
    keep = (cols >= 0) & (cols < n) & (cols != rows)
    S = sp.csr_matrix((np.ones(int(keep.sum())), (rows[keep], cols[keep])), shape=(n, n))
    S = sp.lil_matrix(((S + S.T) != 0).astype(np.float64))
    hubs = hub_rows(n)
    for h, target in zip(hubs, HUB_TARGETS):
        have = set(S.rows[h]) | {h}
        free = np.array([c for c in range(h - 300, h + 301) if c not in have])
        for c in rng.choice(free, size=target - len(have), replace=False):
            S[h, c] = 1.0
            S[c, h] = 1.0
    U = sp.triu(sp.csr_matrix(S), k=1).tocoo()
    v = rng.uniform(0.1, 1.0, U.nnz) * rng.choice([-1.0, 1.0], U.nnz)
    if exact32:
        v = v.astype(np.float32).astype(np.float64)
    B = sp.csr_matrix((v, (U.row, U.col)), shape=(n, n))
    B = sp.csr_matrix(B + B.T)
    d = np.asarray(abs(B).sum(axis=1)).ravel() + 1.0
    if exact32:  # rounded upwards by more than an fp32 ulp: the row stays strictly dominant
        d = (d * (1.0 + 2.0 ** -20)).astype(np.float32).astype(np.float64)
    else:
        d = d + rng.uniform(0.0, 1e-3, n)
    A = sp.csr_matrix(B + sp.diags(d))
    A.sum_duplicates()
    A.sort_indices()
    return A
