"""The factor unit off the grid: IC(0), AINV(0) and the sync-free triangular solve on the fixture
matrices of tests/_cases.py, in fp32 and fp64, against oracle/precond.py in the same precision,
bit for bit (tests/test_factor_host.py pins that oracle, in both precisions, to what the device
produced on the two grids, and asserts the structure these cases rely on):

* rows of 7 / 8 / 9, 15 / 16 / 17, 24 / 25, 33 and 63 dependencies, and a transposed row of more than
  100: partial, exactly full and several ``kTrsvBatch`` batches of ``k_trsv_syncfree``;
* 375 and 428 blocks of 256 positions, more than the device has CUs: workgroups take a second
  block from the dequeue counter;
* level widths 64, 65, 1, 256, 257, 63, 128 and 1,500 levels of one row: the wave padding;
* long and unlike lists in ``merge_sorted`` and the k-way merge of ``k_ainv_cand``, a 64-entry row
  (the AINV limit) and the refusal of a 65-entry one; n = 1 and a matrix without off-diagonals.

Every comparison is on the bits (the unsigned views of the values): no tolerance."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import linalg as O
from oracle import precond as OP
from tests import _cases as K

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f64": np.float64}
MATS = ["ragged", "levels", "chain", "one", "diagonal"]
# the triangular pairs the solves run on: the oracle's IC(0) factor of a matrix and its sorted
# transpose ("ic:<name>"), tril of the levels matrix with its reversal, tril of the 300 x 300 grid
# with its sorted transpose
TRI = ["ic:" + m for m in MATS + ["ragged65"]] + ["levels", "grid"]


@functools.lru_cache(maxsize=None)
def matrix(name):
    return K.factor_ragged65() if name == "ragged65" else K.factor_cases()[name]


@functools.lru_cache(maxsize=None)
def oracle_ic0(name, dt):
    return OP.ic0(matrix(name), DTYPES[dt])


@functools.lru_cache(maxsize=None)
def oracle_ainv(name, dt):
    return OP.ainv_spai_factor(matrix(name), DTYPES[dt])


@functools.lru_cache(maxsize=None)
def tri_pair(name, dt):
    """(lower matrix, upper matrix) in that precision"""
    if name.startswith("ic:"):
        L = oracle_ic0(name[3:], dt)
        return L, K.sorted_transpose(L)
    if name == "levels":
        L = sp.csr_matrix(sp.tril(matrix("levels")), dtype=DTYPES[dt])
        L.sort_indices()
        return L, K.reversed_upper(L)
    L = K.factor_grid_lower().astype(DTYPES[dt])
    return L, K.sorted_transpose(L)


def rhs(n, dt):
    r = np.random.default_rng(3).normal(size=n)
    r[5::37] = -0.0
    return r.astype(DTYPES[dt])


@functools.lru_cache(maxsize=None)
def oracle_solves(name, dt):
    L, U = tri_pair(name, dt)
    r = rhs(L.shape[0], dt)
    return OP.trsv_lower(L, r, DTYPES[dt]), OP.trsv_upper(U, r, DTYPES[dt])


def _dm(A, dt):
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    return DeviceMatrix.from_scipy(A, dtype=DTYPES[dt])


def assert_same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.flatnonzero(got.view(u) != want.view(u))
    assert bad.size == 0, (bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def assert_same_csr(G, W):
    assert G.shape == W.shape
    assert np.array_equal(G.indptr, W.indptr) and np.array_equal(G.indices, W.indices)
    assert_same_bits(G.data, W.data)


def _trsv(T, r, dt, lower):
    return _dm(T, dt).trsv(torch.from_numpy(r).cuda(), lower=lower).cpu().numpy()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", MATS)
def test_ic0_bitwise(gpu_ctx, name, dt):
    assert_same_csr(_dm(matrix(name), dt).ic0()[0].to_scipy(), oracle_ic0(name, dt))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", MATS)
def test_ainv0_bitwise(gpu_ctx, name, dt):
    """``ragged`` holds a 64-entry tril row: the longest the k-way merge accepts."""
    assert_same_csr(_dm(matrix(name), dt).ainv0()[0].to_scipy(), oracle_ainv(name, dt))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", TRI)
def test_trsv_bitwise(gpu_ctx, name, dt):
    L, U = tri_pair(name, dt)
    r = rhs(L.shape[0], dt)
    y, z = oracle_solves(name, dt)
    assert_same_bits(_trsv(L, r, dt, True), y)
    assert_same_bits(_trsv(U, r, dt, False), z)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_trsv_nonfinite_rhs(gpu_ctx, dt):
    """inf and NaN in early rows spread along the dependencies exactly as in the oracle, and the
    solve returns OK: a quiet NaN is a published value like any other, no row waits for it."""
    L, U = tri_pair("ic:ragged", dt)
    n = L.shape[0]
    for T, lower, at_inf, at_nan in ((L, True, 0, K.RAGGED_HUB), (U, False, n - 2, n - 4)):
        r = rhs(n, dt)
        r[at_inf], r[at_nan] = np.inf, np.nan
        with np.errstate(all="ignore"):
            want = (OP.trsv_lower if lower else OP.trsv_upper)(T, r, DTYPES[dt])
        got = _trsv(T, r, dt, lower)  # raises LspcgError unless lspcg_trsv returns OK
        nan = np.isnan(want)
        print(dt, "lower" if lower else "upper", "NaN", int(nan.sum()), "inf", int(np.isinf(want).sum()), "of", n)
        assert nan.sum() > 1 and np.isinf(want).any() and np.isfinite(want).any()  # it spreads, and not everywhere
        assert np.array_equal(np.isnan(got), nan)
        assert_same_bits(got[~nan], want[~nan])  # +-inf included


@pytest.mark.parametrize("dt", list(DTYPES))
def test_ainv_refuses_65_entry_row(gpu_ctx, dt):
    from learningsparsepreconditioner4gpu_amd import _lib

    dA = _dm(matrix("ragged65"), dt)
    with pytest.raises(_lib.LspcgError) as e:
        dA.ainv0()
    assert e.value.code == _lib.ERR_UNSUPPORTED
    # IC(0) has no such limit (its solves: test_trsv_bitwise[ic:ragged65])
    assert_same_csr(dA.ic0()[0].to_scipy(), oracle_ic0("ragged65", dt))


@pytest.mark.parametrize("method", ["ic", "ainv"])
@pytest.mark.parametrize("name", ["ragged", "chain"])
def test_pcg_counts_and_solution(gpu_ctx, name, method):
    """The captured-graph path of the two solves (with the solver's done word) on the new shapes:
    iteration counts equal to the oracle's, x within 1e-12 relative."""
    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient

    A = matrix(name)
    b = A @ np.ones(A.shape[0])
    ps = OP.ic_operator(oracle_ic0(name, "f64")) if method == "ic" else O.spai_operator(oracle_ainv(name, "f64"), 0.0)
    it_o, x_o, _ = O.pcg(A, b, ps, rtol=1e-8, dot="exact")
    solver = PreconditionedConjugateGradient(A, device="cuda", preconditioner=method)
    x = np.zeros_like(b)
    it = solver(b, x, rtol=1e-8)[0]
    err = np.linalg.norm(x - x_o) / np.linalg.norm(x_o)
    print(name, method, "iterations", it, "oracle", it_o, "relative error", err)
    assert it == it_o
    assert err <= 1e-12


@pytest.mark.parametrize("dt", list(DTYPES))
def test_trsv_twice_same_bits(gpu_ctx, dt):
    """Two solves on one DeviceMatrix: the dequeue counter starts from zero in each."""
    for T, lower, want in zip(tri_pair("ic:chain", dt), (True, False), oracle_solves("ic:chain", dt)):
        dT = _dm(T, dt)
        r = torch.from_numpy(rhs(T.shape[0], dt)).cuda()
        first = dT.trsv(r, lower=lower).cpu().numpy()
        second = dT.trsv(r, lower=lower).cpu().numpy()
        assert_same_bits(first, want)
        assert_same_bits(second, first)


def test_pcg_ic_twice_same_bits(gpu_ctx):
    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient

    A = matrix("ragged")
    b = A @ np.ones(A.shape[0])
    solver = PreconditionedConjugateGradient(A, device="cuda", preconditioner="ic")
    x1, x2 = np.zeros_like(b), np.zeros_like(b)
    it1 = solver(b, x1, rtol=1e-8)[0]
    it2 = solver(b, x2, rtol=1e-8)[0]
    assert it1 == it2 and it1 > 0
    assert_same_bits(x2, x1)
