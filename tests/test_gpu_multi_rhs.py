"""GPU parity of the multi-right-hand-side lockstep PCG (lspcg_solver_solve_multi,
PreconditionedConjugateGradient.solve_multi).

Every column must come out as the single ``solve`` on the same solver (and the oracle with
correctly rounded dots) returns it for that column alone: equal count and status, the history
within ``rtol=1e-12`` and the iterate within 1e-12 relative in fp64 (1e-5 in fp32) -- the bounds
of test_gpu_batch.py.  The K-vector kernels add each column's row sums in the single kernels' slot
order, so only the compensated dots' summation trees differ; the tests print how many columns
agree bit for bit.

Columns of a system (``_columns``): 0 ``A@1``; 1 a seeded normal vector; 2 zero (done at the init,
returns b); 3 ``A@sin(0.01 i)`` started from its exact solution (0 iterations while the others
run); 4.. ``A@`` seeded normal vectors scaled by 1, 10, 100, 1000.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import linalg as O
from tests import _cases
from learningsparsepreconditioner4gpu_amd import problems as P

pytestmark = pytest.mark.gpu

EPS = 3e-3


def _columns(A, k=8, dtype=np.float64):
    n = A.shape[0]
    i = np.arange(n, dtype=np.float64)
    B = np.zeros((n, 8))
    X0 = np.zeros((n, 8))
    B[:, 0] = A @ np.ones(n)
    B[:, 1] = np.random.default_rng(11).normal(size=n)
    X0[:, 3] = np.sin(0.01 * i)
    B[:, 3] = A @ X0[:, 3]
    for j in range(4, 8):
        B[:, j] = A @ (10.0 ** (j - 4) * np.random.default_rng(20 + j).normal(size=n))
    return np.ascontiguousarray(B[:, :k].astype(dtype)), np.ascontiguousarray(X0[:, :k].astype(dtype))


def _solver(A, L=None, eps=EPS, pre="ext_spai", dtype=np.float64, **kw):
    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient

    s = PreconditionedConjugateGradient(sp.csr_matrix(A).astype(dtype), device="cuda", preconditioner=pre, dtype=dtype,
                                        **kw)
    if L is not None:
        s.set_spai(sp.csr_matrix(L).astype(dtype), eps)
    return s


def _singles(s, B, X0, rtol, max_iter=0):
    """[(iters, converged, x, hist)] of the single solve of every column on solver ``s``."""
    out = []
    for j in range(B.shape[1]):
        b = torch.from_numpy(np.ascontiguousarray(B[:, j])).cuda()
        x = torch.from_numpy(np.ascontiguousarray(X0[:, j])).cuda()
        it, conv, _, h = s.solve(b, x, rtol=rtol, max_iter=max_iter, return_history=True)
        out.append((it, conv, x.cpu().numpy(), h))
    return out


def _multi(s, B, X0, rtol, max_iter=0):
    Bt = torch.from_numpy(B).cuda()
    Xt = torch.from_numpy(X0.copy()).cuda()
    res, t = s.solve_multi(Bt, Xt, rtol=rtol, max_iter=max_iter, return_history=True)
    assert t > 0 and len(res) == B.shape[1]
    return res, Xt.cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _check(res, X, refs, tol=1e-12, htol=1e-12, what=""):
    """Every column against its reference (iters, converged, x, hist); returns the bit-identical count."""
    same = 0
    for j, ((it, conv, h), (it1, conv1, x1, h1)) in enumerate(zip(res, refs)):
        print(f"{what} column {j}: multi {it} {conv}, reference {it1} {conv1}, iterate rel diff {_rel(X[:, j], x1):.3e}")
        assert (it, conv) == (it1, conv1), (what, j, it, it1)
        assert len(h) == len(h1)
        np.testing.assert_allclose(h, h1, rtol=htol, atol=0)
        assert _rel(X[:, j], x1) <= tol or (not np.linalg.norm(x1) and not np.linalg.norm(X[:, j]))
        same += int(np.array_equal(X[:, j], x1) and np.array_equal(h, h1))
    return same


SDIA_SYSTEMS = {
    "poisson7x9": lambda: P.poisson2d_grid(7, 9)[0],        # 63 rows: less than one slice
    "poisson40x33": lambda: P.poisson2d_grid(40, 33)[0],    # 1,320 rows: a partial tile
    "poisson64x64": lambda: P.poisson2d_grid(64, 64)[0],    # 4,096 rows: whole tiles
    "kuhn23": lambda: P.kuhn_laplacian(23),                 # 12,167 rows
}
_ORACLE = {}


def _oracle(name, A, L, B, X0):
    """The oracle's exact-dot solve of every column, computed once per system."""
    if name not in _ORACLE:
        out = []
        for j in range(B.shape[1]):
            it, x, h = O.pcg(sp.csr_matrix(A), B[:, j], O.spai_operator(sp.csr_matrix(L), EPS), rtol=1e-8,
                             x0=X0[:, j], dot="exact")
            out.append((it, True, x, np.asarray(h)))
        _ORACLE[name] = out
    return _ORACLE[name]


@pytest.mark.parametrize("name", list(SDIA_SYSTEMS))
def test_sdia_partial_slices_and_tiles(gpu_ctx, monkeypatch, name):
    """SELL-DIA views from less than one slice to many tiles, k = 2, 3, 4, 8 (Kp = 2, 4, 4, 8: one
    padding column at k = 3).  LSPCG_SMALL_N=0 gives the two small systems SELL-DIA views too (by
    default they are solved in one workgroup from SELL-64 copies), so all four run the same kernel."""
    monkeypatch.setenv("LSPCG_SMALL_N", "0")
    A = SDIA_SYSTEMS[name]()
    L = _cases.spai_like(A, seed=3)
    B, X0 = _columns(A)
    s = _solver(A, L)
    views = s.views
    assert [views[m]["columns"] for m in ("A", "L", "LT")] == ["sdia"] * 3, views
    singles = _singles(s, B, X0, 1e-8)
    oracle = _oracle(name, A, L, B, X0)
    counts = [r[0] for r in singles]
    print(f"{name}: single-solve counts {counts}")
    assert counts[2] == 0 and counts[3] == 0
    assert len(set(counts)) >= 3, counts  # the columns finish at different iterations
    same = total = 0
    for k in (2, 3, 4, 8):
        res, X = _multi(s, B[:, :k].copy(), X0[:, :k].copy(), 1e-8)
        same += _check(res, X, singles[:k], what=f"{name} k={k} vs single")
        _check(res, X, oracle[:k], what=f"{name} k={k} vs oracle")
        total += k
        assert not X[:, 2:3].any()  # the zero column returns b
    print(f"{name}: columns bit-identical to their single solves: {same}/{total}")


@pytest.mark.parametrize("name", ["poisson7x9", "poisson40x33"])
def test_small_systems_default_views(gpu_ctx, name):
    """By default systems of n <= 3072 get SELL-64 views and their single solve runs in one
    workgroup; solve_multi takes the five K-wide launches on the same views and must still equal it."""
    A = SDIA_SYSTEMS[name]()
    L = _cases.spai_like(A, seed=3)
    s = _solver(A, L)
    views = s.views
    assert [views[m]["columns"] for m in ("A", "L", "LT")] == ["sell16"] * 3, views
    B, X0 = _columns(A, 5)
    singles = _singles(s, B, X0, 1e-8)
    for k in (3, 5):
        res, X = _multi(s, B[:, :k].copy(), X0[:, :k].copy(), 1e-8)
        same = _check(res, X, singles[:k], what=f"{name} default views k={k}")
        print(f"{name} k={k}: columns bit-identical to their single solves: {same}/{k}")


def _rcm27():
    A, m = P.renumber(*P.kuhn_dirichlet(27), "rcm")
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def _rand33():
    A, m = P.renumber(*P.kuhn_dirichlet(33), "rand")
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


_SELL64 = {}


def _sell64_system(monkeypatch, make, want, max_iter):
    """The system's solver, its 8 columns and their single solves, built once per system."""
    if want not in _SELL64:
        monkeypatch.setenv("LSPCG_REORDER", "0")
        monkeypatch.setenv("LSPCG_SELLC", "0")
        A = make()
        s = _solver(A, _cases.spai_like(A, seed=4))
        B, X0 = _columns(A, 8)
        _SELL64[want] = (s, B, X0, _singles(s, B, X0, 1e-8, max_iter))
    return _SELL64[want]


@pytest.mark.parametrize("k", (2, 4, 8))
@pytest.mark.parametrize("make,want,max_iter", [(_rcm27, "sell16", 0), (_rand33, "sell32", 40)])
def test_sell64_views(gpu_ctx, monkeypatch, make, want, max_iter, k):
    """SELL-64 views with 16-bit offsets (an RCM ordering) and with int32 columns (a random
    numbering of 35,937 rows: offsets past the 16-bit range; bounded by max_iter = 40), k = 2, 4, 8:
    the K-vector SELL-64 kernel batches two 4-entry groups at K = 2 and one at K = 4, 8."""
    s, B, X0, singles = _sell64_system(monkeypatch, make, want, max_iter)
    views = s.views
    assert [views[m]["columns"] for m in ("A", "L", "LT")] == [want] * 3, views
    res, X = _multi(s, B[:, :k].copy(), X0[:, :k].copy(), 1e-8, max_iter)
    if max_iter:
        assert [r[0] for r in res][:4] == [40, 40, 0, 0][:k] and len(res[0][2]) == 41
    same = _check(res, X, singles[:k], what=f"{want} k={k}")
    print(f"{want} k={k}: columns bit-identical to their single solves: {same}/{k}")


@pytest.fixture(scope="module")
def poisson64():
    A = P.poisson2d_grid(64, 64)[0]
    return A, _cases.spai_like(A, seed=3)


def test_columns_are_independent(gpu_ctx, poisson64):
    """K identical columns give K bit-identical results; permuting the columns permutes the results
    bit for bit (no column's arithmetic depends on its lane or on its neighbours)."""
    A, L = poisson64
    s = _solver(A, L)
    B, X0 = _columns(A)
    Bs = np.ascontiguousarray(np.repeat(B[:, 1:2], 8, axis=1))
    res, X = _multi(s, Bs, np.zeros_like(Bs), 1e-8)
    for j in range(1, 8):
        assert res[j][:2] == res[0][:2]
        assert np.array_equal(res[j][2], res[0][2]) and np.array_equal(X[:, j], X[:, 0])
    res0, Xa = _multi(s, B, X0, 1e-8)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    res1, Xb = _multi(s, np.ascontiguousarray(B[:, perm]), np.ascontiguousarray(X0[:, perm]), 1e-8)
    for j, pj in enumerate(perm):
        assert res1[j][:2] == res0[pj][:2]
        assert np.array_equal(res1[j][2], res0[pj][2]) and np.array_equal(Xb[:, j], Xa[:, pj])


@pytest.mark.parametrize("max_iter", [1, 5, 37])
def test_stops(gpu_ctx, poisson64, max_iter):
    """max_iter stops inside and at the end of a captured chunk: the zero and exact-x0 columns
    converge, the others do not; status per column, LSPCG_NOT_CONVERGED for the call, histories of
    iters + 1 entries."""
    from learningsparsepreconditioner4gpu_amd import _lib

    A, L = poisson64
    s = _solver(A, L)
    B, X0 = _columns(A, 5)
    singles = _singles(s, B, X0, 1e-8, max_iter)
    res, X = _multi(s, B, X0, 1e-8, max_iter)
    assert [r[:2] for r in res] == [(max_iter, False), (max_iter, False), (0, True), (0, True), (max_iter, False)]
    for it, _, h in res:
        assert len(h) == it + 1
    _check(res, X, singles, what=f"max_iter={max_iter}")
    # the C call's own return value and status array
    Bt, Xt = torch.from_numpy(B).cuda(), torch.from_numpy(X0.copy()).cuda()
    it, stt, ms = (C.c_int64 * 5)(), (C.c_int32 * 5)(), C.c_double()
    rc = _lib.call("lspcg_solver_solve_multi", s.handle, 5, Bt.data_ptr(), Xt.data_ptr(), 1e-8, max_iter, it, stt,
                   None, C.byref(ms), allow_not_converged=True)
    assert rc == _lib.NOT_CONVERGED
    assert list(stt) == [_lib.NOT_CONVERGED, _lib.NOT_CONVERGED, _lib.OK, _lib.OK, _lib.NOT_CONVERGED]
    assert np.array_equal(Xt.cpu().numpy(), X)
    # all columns converging returns OK
    B2, X2 = Bt[:, 2:4].contiguous(), torch.from_numpy(np.ascontiguousarray(X0[:, 2:4])).cuda()
    rc = _lib.call("lspcg_solver_solve_multi", s.handle, 2, B2.data_ptr(), X2.data_ptr(), 1e-8, max_iter, it, stt,
                   None, C.byref(ms), allow_not_converged=True)
    assert rc == _lib.OK and list(stt)[:2] == [_lib.OK, _lib.OK]


def test_nonfinite_column_stops_alone(gpu_ctx, poisson64):
    """A column whose residual is not finite stops with the single solve's report (max_iter, not
    converged, NaN-filled history) while its neighbours converge as they do alone."""
    A, L = poisson64
    s = _solver(A, L)
    B, X0 = _columns(A, 3)
    B[5, 1] = np.inf
    singles = _singles(s, B, X0, 1e-8, 50)
    res, X = _multi(s, B, X0, 1e-8, 50)
    assert res[1][:2] == (50, False) and not res[0][1] and res[2][:2] == (0, True)
    for j in range(3):
        assert res[j][:2] == singles[j][:2]
        np.testing.assert_allclose(res[j][2], singles[j][3], rtol=1e-12, atol=0)  # NaN and inf entries compare equal
    assert _rel(X[:, 0], singles[0][2]) <= 1e-12
    assert np.array_equal(X[:, 1], singles[1][2]) and np.array_equal(X[:, 2], singles[2][2])


def test_reuse(gpu_ctx, poisson64):
    """A second solve_multi gives the same bits; after set_spai with another L the columns equal
    that L's single solves; a single solve gives the same bits before and after a solve_multi."""
    A, L = poisson64
    s = _solver(A, L)
    B, X0 = _columns(A, 4)
    before = _singles(s, B, X0, 1e-8)
    res0, Xa = _multi(s, B, X0, 1e-8)
    res1, Xb = _multi(s, B, X0, 1e-8)
    assert np.array_equal(Xa, Xb)
    for a, b in zip(res0, res1):
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2])
    after = _singles(s, B, X0, 1e-8)
    for a, b in zip(before, after):
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    _check(res0, Xa, before, what="first L")
    L2 = _cases.spai_like(A, seed=9, scale=0.03)
    s.set_spai(L2, 1e-3)
    singles2 = _singles(s, B, X0, 1e-8)
    assert [r[0] for r in singles2] != [r[0] for r in before]
    res2, Xc = _multi(s, B, X0, 1e-8)
    _check(res2, Xc, singles2, what="second L")


@pytest.mark.parametrize("pre", ["ext_spai_scaled", "ainv"])
def test_scaled_and_ainv(gpu_ctx, poisson64, pre):
    A, L = poisson64
    s = _solver(A, L if pre == "ext_spai_scaled" else None, pre=pre)
    B, X0 = _columns(A, 4)
    singles = _singles(s, B, X0, 1e-8)
    res, X = _multi(s, B, X0, 1e-8)
    assert max(r[0] for r in res) > 10
    same = _check(res, X, singles, what=pre)
    print(f"{pre}: columns bit-identical to their single solves: {same}/4")


@pytest.mark.parametrize("name", ["poisson64x64", "kuhn23"])
def test_fp32(gpu_ctx, name):
    A = SDIA_SYSTEMS[name]().astype(np.float32)
    L = _cases.spai_like(A, seed=3).astype(np.float32)
    s = _solver(A, L, dtype=np.float32)
    B, X0 = _columns(A, 4, dtype=np.float32)
    singles = _singles(s, B, X0, 1e-5)
    res, X = _multi(s, B, X0, 1e-5)
    for j, ((it, conv, h), (it1, conv1, x1, h1)) in enumerate(zip(res, singles)):
        print(f"{name} fp32 column {j}: multi {it} {conv}, single {it1} {conv1}, rel diff {_rel(X[:, j], x1):.3e}")
        assert (it, conv) == (it1, conv1)
        assert _rel(X[:, j], x1) <= 1e-5 or not np.linalg.norm(x1)
    # the oracle's fp32 scipy cg with correctly rounded dots: the same counts
    for j in (0, 1):
        it_o, x_o, _ = O.pcg(sp.csr_matrix(A), B[:, j], O.spai_operator(sp.csr_matrix(L), np.float32(EPS)), rtol=1e-5,
                             dot="exact", dtype=np.float32)
        assert res[j][0] == it_o
        assert _rel(X[:, j], x_o) <= 1e-5


def test_eleven_columns_in_groups(gpu_ctx, poisson64):
    """k = 11 through the Python grouping (8 + 3 columns)."""
    A, L = poisson64
    s = _solver(A, L)
    B8, X8 = _columns(A)
    B = np.ascontiguousarray(np.concatenate([B8, 0.5 * B8[:, :3]], axis=1))
    X0 = np.ascontiguousarray(np.concatenate([X8, 0.5 * X8[:, :3]], axis=1))
    singles = _singles(s, B, X0, 1e-8)
    res, X = _multi(s, B, X0, 1e-8)
    assert len(res) == 11
    _check(res, X, singles, what="k=11")


def test_refusals(gpu_ctx, poisson64):
    """Argument checks made before any launch: unsupported configurations and nrhs out of range."""
    from learningsparsepreconditioner4gpu_amd import _lib

    A, L = poisson64
    n = A.shape[0]
    Bt = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    Xt = torch.zeros_like(Bt)

    def refused(s, B=Bt, X=Xt):
        with pytest.raises(_lib.LspcgError) as e:
            s.solve_multi(B, X)
        assert e.value.code == _lib.ERR_UNSUPPORTED, e.value
        assert "solve_multi" in str(e.value)

    refused(_solver(A, pre="none"))
    refused(_solver(A, pre="diagonal"))
    refused(_solver(A, pre="ic"))
    refused(_solver(A, L, dot_order="openblas"))
    E = sp.csr_matrix(P.elasticity_box(5, 4, 4)[0])
    s3 = _solver(E, pre="ext_spai", block_size=3)
    s3.set_spai(_cases.spai_like(E, seed=1, scale=0.02), 1e-3, block_size=3)
    B3 = torch.zeros((E.shape[0], 2), dtype=torch.float64, device="cuda")
    refused(s3, B3, torch.zeros_like(B3))
    s = _solver(A, L)
    it, stt, ms = (C.c_int64 * 9)(), (C.c_int32 * 9)(), C.c_double()
    for nrhs in (0, 9):
        with pytest.raises(_lib.LspcgError) as e:
            _lib.call("lspcg_solver_solve_multi", s.handle, nrhs, Bt.data_ptr(), Xt.data_ptr(), 1e-8, 0, it, stt, None,
                      C.byref(ms))
        assert e.value.code == _lib.ERR_ARG
    with pytest.raises(ValueError):
        s.solve_multi(Bt, Xt[:, :1])
    with pytest.raises(ValueError):
        s.solve_multi(Bt.t(), Xt.t())
    with pytest.raises(TypeError):
        s.solve_multi(Bt.float(), Xt.float())
