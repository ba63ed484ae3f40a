"""Shared small test systems (CPU-side construction only)."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from learningsparsepreconditioner4gpu_amd import problems as P


def spai_like(A: sp.csr_matrix, seed: int = 0, scale: float = 0.05) -> sp.csr_matrix:
    """A factor on A's pattern: D^{-1/2} plus small random off-diagonal entries."""
    rng = np.random.default_rng(seed)
    A = sp.csr_matrix(A)
    L = A.copy().astype(np.float64)
    d = A.diagonal()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    vals = rng.normal(size=A.nnz) * scale / np.sqrt(np.abs(d[rows]) + 1e-12)
    diag = rows == A.indices
    vals[diag] = 1.0 / np.sqrt(np.abs(d[rows[diag]]) + 1e-12)
    L.data = vals
    return L


def ragged_matrix(n: int = 3000, seed: int = 1) -> sp.csr_matrix:
    """Empty rows, a row longer than one SpMV chunk (5000 > 4096 entries), random lengths."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n):
        if i % 97 == 5:
            continue  # empty row
        k = rng.integers(1, 40)
        c = rng.choice(n, size=k, replace=False)
        rows += [i] * k
        cols += list(c)
    k = min(2500, n)
    rows += [7] * k  # long row (+ beyond chunk with the neighbours)
    cols += list(rng.choice(n, size=k, replace=False))
    A = sp.csr_matrix((rng.normal(size=len(rows)), (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    A.sort_indices()
    big = sp.csr_matrix((rng.normal(size=5000), (np.full(5000, 11), np.arange(5000) % n)), shape=(n, n))
    A = (A + big).tocsr()
    A.sort_indices()
    return A


# ---------------------------------------------------------------------------
# Factor-unit fixtures (tests/test_factor_host.py asserts their structure, tests/
# test_gpu_factor_shapes.py runs them): SPD M-matrices, off-diagonals in [-1, -0.1], each diagonal
# its row's absolute sum plus uniform(0.05, 1), so IC(0) and AINV(0) exist in fp32 and fp64.
# ---------------------------------------------------------------------------
RAGGED_COUNTS = (7, 8, 9, 15, 16, 17, 24, 25, 33, 63)  # lower off-diagonals of the designated rows
RAGGED_HUB = 3  # the column stored in >= 100 later rows
LEVEL_WIDTHS = (64, 65, 1, 256, 257, 63, 128)


def _m_matrix(n: int, rows, cols, vals, slack) -> sp.csr_matrix:
    """The symmetric M-matrix with the strictly lower entries (rows, cols, vals) and the diagonal
    slack above each row's absolute sum."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    assert (cols < rows).all()
    S = sp.csr_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=(n, n))
    assert S.nnz == rows.size, "duplicate entries in the lower pattern"
    S = S + S.T
    d = np.asarray(abs(S).sum(axis=1)).ravel() + np.asarray(slack)
    A = sp.csr_matrix(S + sp.diags(d))
    A.sort_indices()
    return A


def factor_ragged(n: int = 900, seed: int = 11, longest: int = 63) -> sp.csr_matrix:
    """Row i stores a prescribed number of distinct random columns < i: 0-5 in the background,
    RAGGED_COUNTS (the last one ``longest``) in ten designated rows (one short of, exactly and one
    past 1, 2 and 3 trsv batches of 8; 33; a 64-entry tril row, the AINV limit), and the hub column
    in every 7th other row, so the transposed factor has a row of more than 100 entries."""
    counts = list(RAGGED_COUNTS[:-1]) + [longest]
    designated = {n - 50 - 60 * (len(counts) - 1 - q): c for q, c in enumerate(counts)}  # ascending rows, >= 310
    rows, cols, vals, slack = [], [], [], []
    for i in range(n):
        rng = np.random.default_rng([seed, i])  # a stream per row: a longer row changes no other
        slack.append(rng.uniform(0.05, 1.0))
        k = min(int(rng.integers(0, 6)), i)
        hub = i not in designated and i > RAGGED_HUB and i % 7 == 3
        if i in designated:
            k = designated[i]
        elif hub:
            k = max(k, 1)
        if hub:
            others = np.delete(np.arange(i), RAGGED_HUB)
            c = [RAGGED_HUB] + rng.permutation(others)[:k - 1].tolist()
        else:
            c = rng.permutation(i)[:k].tolist()
        rows += [i] * k
        cols += c
        vals += (-rng.uniform(0.1, 1.0, size=k)).tolist()
    return _m_matrix(n, rows, cols, vals, slack)


def factor_ragged65() -> sp.csr_matrix:
    """factor_ragged with the longest row one entry longer: a 65-entry tril row, past the AINV limit."""
    return factor_ragged(longest=64)


def factor_levels(seed: int = 12) -> sp.csr_matrix:
    """Rows numbered level by level, the levels of tril(A) exactly LEVEL_WIDTHS wide (a full
    wave, one past it, a single row, a full 256-block, one past it, ...): each row of level l > 0
    stores 1-10 columns of level l - 1 and now and then one of an earlier level."""
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(LEVEL_WIDTHS)])
    n = int(start[-1])
    rows, cols = [], []
    for l in range(1, len(LEVEL_WIDTHS)):
        for i in range(start[l], start[l + 1]):
            k = min(int(rng.integers(1, 11)), LEVEL_WIDTHS[l - 1])
            c = (start[l - 1] + rng.choice(LEVEL_WIDTHS[l - 1], size=k, replace=False)).tolist()
            if l > 1 and rng.random() < 0.2:
                c.append(int(rng.integers(0, start[l - 1])))
            rows += [i] * len(c)
            cols += c
    return _m_matrix(n, rows, cols, -rng.uniform(0.1, 1.0, size=len(rows)), rng.uniform(0.05, 1.0, size=n))


def factor_chain(n: int = 1500) -> sp.csr_matrix:
    """Tridiagonal (-1, 2.5, -1): n levels of one row each, n wave-padded positions of 64."""
    A = sp.diags([-np.ones(n - 1), np.full(n, 2.5), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


def factor_one() -> sp.csr_matrix:
    return sp.csr_matrix(np.array([[2.5]]))


def factor_diagonal(n: int = 130, seed: int = 13) -> sp.csr_matrix:
    """No off-diagonal entry: a single level, empty AINV candidate lists."""
    return sp.csr_matrix(sp.diags(np.random.default_rng(seed).uniform(0.5, 3.0, size=n)))


def factor_grid_lower(nx: int = 300, ny: int = 300) -> sp.csr_matrix:
    """tril of the 5-point grid, for the triangular solves alone: nx + ny - 1 levels and more
    256-position blocks than the device has CUs."""
    L = sp.csr_matrix(sp.tril(P.poisson2d_grid(nx, ny)[0], format="csr"))
    L.sort_indices()
    return L


def reversed_upper(L: sp.csr_matrix) -> sp.csr_matrix:
    """J L Jᵀ (rows and columns reversed): upper triangular, the same level widths as L."""
    n = L.shape[0]
    C = sp.coo_matrix(L)
    U = sp.csr_matrix((C.data, (n - 1 - C.row, n - 1 - C.col)), shape=(n, n))
    U.sort_indices()
    return U


def sorted_transpose(L: sp.csr_matrix) -> sp.csr_matrix:
    U = sp.csr_matrix(sp.csr_matrix(L).T)
    U.sort_indices()
    return U


def solve_levels(T: sp.csr_matrix, lower: bool = True) -> np.ndarray:
    """lev[i] = 1 + max lev over row i's off-diagonal columns (0 without any), computed row by row
    in the order of the solve."""
    T = sp.csr_matrix(T)
    n = T.shape[0]
    lev = np.zeros(n, dtype=np.int64)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        c = T.indices[T.indptr[i]:T.indptr[i + 1]]
        c = c[c < i] if lower else c[c > i]
        if c.size:
            lev[i] = lev[c].max() + 1
    return lev


def trsv_blocks(widths) -> int:
    """256-position blocks of the sync-free solve: every level padded to whole wave64s."""
    return -(-sum(-(-int(w) // 64) * 64 for w in widths) // 256)


def factor_cases():
    """name -> SPD matrix, the systems the factorizations and solves run on."""
    return {"ragged": factor_ragged(), "levels": factor_levels(), "chain": factor_chain(), "one": factor_one(),
            "diagonal": factor_diagonal()}


def spd_cases():
    """(name, A, mask) small SPD systems covering the reference's configs."""
    out = []
    out.append(("synthetic-2048", P.generate_spd_sparse_matrix(2048, 2e-3, 1e-3, np.random.RandomState(3)), None))
    A, m, _ = P.poisson2d_grid(24, 20)
    out.append(("poisson2d-24x20", A, m))
    out.append(("kuhn-9", P.kuhn_laplacian(9), None))
    A, m, _ = P.heat_tet(7, 6, 5)
    out.append(("heat-tet", A, m))
    return out
