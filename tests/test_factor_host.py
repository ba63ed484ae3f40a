"""The factor unit's CPU side: the oracle in both precisions against the committed digests, and the
structure of the fixture matrices that tests/test_gpu_factor_shapes.py runs on the device.

``oracle/precond.py`` restates IC(0), AINV(0) and the two triangular solves with every operation
rounded to the working precision; ``tests/golden/factor_bits.json`` holds what the device produced
in fp32 and fp64.  The two agreeing bit for bit, here, without a GPU, is what lets the device tests
hold the fp32 kernels to the oracle with ``np.array_equal``, and it pins the fp64 default path to
its bits.  The structure assertions keep a later change to a generator from moving the device tests
back onto easy shapes (short rows, fewer blocks than CUs, smooth level widths)."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import _cases as K
from tests.test_gpu_factor_bits import RUNS, fixture, oracle_bits


def _tril_counts(A):
    """off-diagonal entries per row of tril(A)"""
    return np.diff(sp.csr_matrix(sp.tril(A, k=-1)).indptr)


def _triu_counts(A):
    return np.diff(sp.csr_matrix(sp.triu(A, k=1)).indptr)


def _widths(T, lower=True):
    return np.bincount(K.solve_levels(T, lower))


@pytest.mark.parametrize("name,dt", RUNS, ids=[f"{n}-{d}" for n, d in RUNS])
def test_oracle_reproduces_committed_digests(name, dt):
    got, want = oracle_bits(name, dt), fixture()["cases"][f"{name}/{dt}"]
    for key in ("ic0", "ainv0", "trsv_lower", "trsv_upper"):
        assert got[key] == want[key], (name, dt, key)
    assert set(got) == set(want)


@pytest.mark.parametrize("name", ["ragged", "ragged65", "levels"])
def test_fixtures_are_spd_m_matrices(name):
    A = {"ragged": K.factor_ragged, "ragged65": K.factor_ragged65, "levels": K.factor_levels}[name]()
    assert (abs(A - A.T)).nnz == 0 and A.has_sorted_indices
    off = sp.csr_matrix(A - sp.diags(A.diagonal()))
    off.eliminate_zeros()
    assert off.data.max() <= -0.1 and off.data.min() >= -1.0
    slack = A.diagonal() - np.asarray(abs(off).sum(axis=1)).ravel()
    assert slack.min() >= 0.05 - 1e-12 and slack.max() <= 1.0 + 1e-12  # strictly diagonally dominant


def test_ragged_structure():
    A = K.factor_ragged()
    assert A.shape == (900, 900)
    lo = _tril_counts(A)
    for c in K.RAGGED_COUNTS:  # 7 8 9 / 15 16 17 / 24 25 / 33 / 63: around 1, 2, 3 batches of 8, and the AINV limit
        assert (lo == c).any(), c
    assert lo.max() == 63  # a 64-entry tril row
    designated = np.isin(lo, K.RAGGED_COUNTS)
    assert lo[~designated].max() <= 5
    up = _triu_counts(A)
    assert up.max() >= 100 and up.argmax() == K.RAGGED_HUB
    w = _widths(sp.tril(A))
    print("ragged: levels", w.size, "widest", w.max())
    assert w.max() > 64 and w.size >= 10
    # the solve's arithmetic order is the stored order: many rows mix early and late levels
    wu = _widths(sp.triu(A), lower=False)
    assert K.trsv_blocks(w) > 1 and K.trsv_blocks(wu) > 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_ragged_bits_depend_on_the_batch_order(dtype):
    """The bitwise comparison on ``ragged`` can see a solve that sums a row's later batches of 8
    dependencies in another order: restated that way, the lower solve differs from the oracle in
    rows of more than 9 dependencies and in rows that depend on them, and in none before."""
    from oracle import precond as OP

    L = OP.ic0(K.factor_ragged(), dtype)
    r = np.random.default_rng(3).normal(size=L.shape[0]).astype(dtype)
    want = OP.trsv_lower(L, r, dtype)
    d = L.diagonal()
    inv = dtype(1) / d
    y = np.zeros_like(r)
    for i in range(L.shape[0]):
        cols = L.indices[L.indptr[i]:L.indptr[i + 1] - 1].tolist()
        vals = list(L.data[L.indptr[i]:L.indptr[i + 1] - 1])
        order = list(range(min(8, len(cols))))
        for kb in range(8, len(cols), 8):  # every batch after the first, backwards
            order += list(range(min(kb + 8, len(cols)) - 1, kb - 1, -1))
        s = r[i]
        for k in order:
            s = s - y[cols[k]] * (vals[k] * inv[cols[k]])
        y[i] = s
    got = (y / (d * inv)) * inv
    differs = np.flatnonzero(got != want)
    long_rows = np.flatnonzero(_tril_counts(L) > 9)
    print(np.dtype(dtype).name, "rows that differ", differs.size, "first", differs[:3], "first long row", long_rows[0])
    assert differs.size > 0 and differs[0] >= long_rows[0]
    assert np.isin(differs, long_rows).any()


def test_ragged65_structure():
    A, B = K.factor_ragged(), K.factor_ragged65()
    lo = _tril_counts(B)
    assert lo.max() == 64 and (lo == 64).sum() == 1  # the longest tril row has 65 entries
    r = int(lo.argmax())
    assert np.array_equal(np.delete(lo, r), np.delete(_tril_counts(A), r)) and _tril_counts(A)[r] == 63
    keep = np.delete(np.arange(900), r)
    D = sp.csr_matrix(sp.tril(B, k=-1) - sp.tril(A, k=-1))
    D.eliminate_zeros()
    assert D.nnz == 1 and D[keep].nnz == 0  # the same matrix but for that row's one more entry
    for c in K.RAGGED_COUNTS[:-1]:
        assert (lo == c).any(), c
    assert _triu_counts(B).max() >= 100


def test_levels_structure():
    A = K.factor_levels()
    L = sp.csr_matrix(sp.tril(A))
    assert np.array_equal(_widths(L), K.LEVEL_WIDTHS)
    assert np.array_equal(K.solve_levels(L), np.repeat(np.arange(len(K.LEVEL_WIDTHS)), K.LEVEL_WIDTHS))  # level by level
    lo = _tril_counts(A)
    assert lo.max() >= 10 and lo[64:].min() >= 1  # second trsv batch; no row past level 0 is free
    lev = K.solve_levels(L)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(L.indptr))
    assert (lev[rows] - lev[L.indices] >= 2).any()  # a dependency on an earlier level than the previous one
    U = K.reversed_upper(L)
    assert (sp.tril(U, k=-1)).nnz == 0 and U.has_sorted_indices
    assert np.array_equal(U.indices[U.indptr[:-1]], np.arange(U.shape[0]))  # the diagonal first in each row
    assert np.array_equal(_widths(U, lower=False), K.LEVEL_WIDTHS)
    assert np.array_equal(U.toarray(), L.toarray()[::-1, ::-1])


def test_chain_structure():
    A = K.factor_chain()
    assert A.shape == (1500, 1500)
    assert np.array_equal(A.diagonal(), np.full(1500, 2.5)) and np.array_equal(A.diagonal(-1), -np.ones(1499))
    assert A.nnz == 3 * 1500 - 2 and (abs(A - A.T)).nnz == 0
    w = _widths(sp.tril(A))
    assert w.size == 1500 and (w == 1).all()  # one row per level
    assert K.trsv_blocks(w) == 375 > 256  # more blocks than CUs: workgroups take a second block
    assert np.array_equal(_widths(sp.triu(A), lower=False), w)


def test_grid_structure():
    L = K.factor_grid_lower()
    assert L.shape == (90000, 90000) and sp.triu(L, k=1).nnz == 0 and (L.diagonal() > 0).all()
    w = _widths(L)
    print("grid: levels", w.size, "blocks", K.trsv_blocks(w))
    assert w.size == 599 and w.max() > 256
    assert K.trsv_blocks(w) > 256
    assert K.trsv_blocks(_widths(K.sorted_transpose(L), lower=False)) > 256


def test_degenerate_structure():
    one, dg = K.factor_one(), K.factor_diagonal()
    assert one.shape == (1, 1) and one[0, 0] == 2.5
    assert dg.shape == (130, 130) and dg.nnz == 130 and (dg.diagonal() > 0).all()
    assert _widths(dg).tolist() == [130]


def test_factor_cases_names():
    assert sorted(K.factor_cases()) == ["chain", "diagonal", "levels", "one", "ragged"]
