"""GPU: new values of A on a live solver (lspcg_mat_set_values, lspcg_assemble_into,
lspcg_solver_update_matrix).  The standard is set_spai's (test_new_spai_on_the_same_solver_equals_a_fresh_solver):
the same kernels on the same values in the same order give the same bits, so every comparison
here is bit equality -- an updated solver against a solver created on the new matrix, an
in-place assembly against a fresh one, the refilled SpMV copy against scipy.

The matrices: A1, A2 = D A1 D with D = diag(1 + 0.5 u), u seeded uniform (the same pattern, SPD, no
new zeros, not fp32-exact) and A3 = A1 rounded through fp32 (the exactness transitions).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from learningsparsepreconditioner4gpu_amd import problems as P
from tests import _cases

pytestmark = pytest.mark.gpu

EPS = 1e-3
KINDS = ("none", "diagonal", "ext_spai", "ext_spai_scaled", "ic", "ainv")


def _csr(A):
    A = sp.csr_matrix(A).astype(np.float64)
    A.sort_indices()
    return A


def _scaled(A, seed=7):
    """D A D, D = diag(1 + 0.5 u): the stored arrays of A with new values."""
    A = _csr(A)
    d = 1.0 + 0.5 * np.random.default_rng(seed).uniform(size=A.shape[0])
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return sp.csr_matrix((d[rows] * A.data * d[A.indices], A.indices.copy(), A.indptr.copy()), shape=A.shape)


def _f32_exact_copy(A):
    A = _csr(A).copy()
    A.data = A.data.astype(np.float32).astype(np.float64)
    return A


def _is_f32_exact(A):
    return bool(np.all(A.data.astype(np.float32).astype(np.float64) == A.data))


def _band(n=3008, seed=21, blk=64, offs=(1, 2, 3, 5, 8, 13, 21, 27, 29, 30, 31)):
    """Block-diagonal M-matrix of circulant 64-row blocks, 23 entries in every row: more than 16
    offsets per slice (no SELL-DIA), equal row lengths (no SELL-64J), columns within 16 bits.  No
    dependency chain is longer than a block, so IC(0) and AINV(0) run a few dozen levels."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for o in offs:
        i = np.arange(n)
        j = (i // blk) * blk + (i + o) % blk
        rows.append(np.maximum(i, j))
        cols.append(np.minimum(i, j))
        vals.append(-rng.uniform(0.1, 1.0, size=n))
    return _cases._m_matrix(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals),
                            rng.uniform(0.05, 1.0, size=n))


# name -> (matrix, environment, block size, the A view's column storage the case is about)
SYSTEMS = {
    "sdia": (lambda: P.kuhn_laplacian(15), {}, 1, ("sdia",)),  # 3,375 rows: partial last slice, multi-kernel schedule
    "sell16": (_band, {}, 1, ("sell16",)),
    "sell16j": (lambda: P.delaunay_heat(4000)[0], {"LSPCG_REORDER": "0"}, 1, ("sell16j", "sell16x")),
    # the x-staged jagged layout, which exists from 2^18 rows: its floor lowered to reach it at 4,000
    "sell16x": (lambda: P.delaunay_heat(4000)[0], {"LSPCG_REORDER": "0", "LSPCG_SELLX_MIN_N": "0"}, 1, ("sell16x",)),
    "csr": (lambda: P.kuhn_laplacian(15), {"LSPCG_NO_SELL": "1"}, 1, ("csr",)),
    "small": (lambda: P.kuhn_laplacian(9), {}, 1, None),  # the one-workgroup solve
    "bsr3": (lambda: P.elasticity_box(6, 5, 5)[0], {"LSPCG_SMALL_N": "0"}, 3, None),
    "reorder": (lambda: P.kuhn_laplacian(30, 1e-2), {"LSPCG_REORDER": "1"}, 1, None),
}


@functools.lru_cache(maxsize=None)
def _matrices(name):
    """(A1, A2, A3) and their ext_spai factors, built once per system and never written to."""
    A1 = _csr(SYSTEMS[name][0]())
    As = (A1, _scaled(A1), _f32_exact_copy(A1))
    bs = SYSTEMS[name][2]
    Ls = []
    for k, A in enumerate(As):
        L = _cases.spai_like(A, seed=k)
        Ls.append(_csr(sp.bsr_matrix(L, blocksize=(3, 3))) if bs == 3 else L)
    assert not _is_f32_exact(As[1]) and _is_f32_exact(As[2])
    return As, tuple(Ls)


def _typed(A, dtype):
    # (scipy's astype keeps the stored order of sorted rows)
    return sp.csr_matrix((A.data.astype(dtype), A.indices, A.indptr), shape=A.shape)


def _solver(A, L, pre, dtype, bs=1, dot_order="compensated"):
    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient

    s = PreconditionedConjugateGradient(_typed(A, dtype), device="cuda", preconditioner=pre, dtype=dtype, block_size=bs,
                                        dot_order=dot_order)
    if pre.startswith("ext_spai"):
        s.set_spai(_typed(L, dtype), EPS, block_size=bs)
    return s


def _update(s, A, L, pre, dtype, bs=1):
    t, kept = s.update_matrix(_typed(A, dtype))
    assert t >= 0.0
    if pre.startswith("ext_spai"):
        s.set_spai(_typed(L, dtype), EPS, block_size=bs)
    return kept


def _run(s, b, dtype):
    x = torch.zeros_like(b)
    it, conv, _t, h = s.solve(b, x, rtol=1e-8 if dtype == np.float64 else 1e-5, return_history=True, max_iter=5000)
    return it, conv, x.cpu().numpy(), np.asarray(h)


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def _rhs(A, dtype):
    # (A @ ones is an eigenvector of the shifted Laplacians: one iteration)
    b = (A @ np.random.default_rng(11).normal(size=A.shape[0])).astype(dtype)
    return torch.as_tensor(b, device="cuda")


def _kept_expected(prev, new, dtype):
    """Graphs survive between matrices of equal fp32-exactness; an fp32 solver stores fp32 either way."""
    return True if dtype == np.float32 else _is_f32_exact(prev) == _is_f32_exact(new)


def _updated_equals_fresh(monkeypatch, name, pre, dtype, dot_order="compensated"):
    _mat, env, bs, want = SYSTEMS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    (A1, A2, A3), (L1, L2, L3) = _matrices(name)
    b = _rhs(A1, dtype)
    fresh = {}

    def fresh_run(k, A, L):
        if k not in fresh:
            fresh[k] = _run(_solver(A, L, pre, dtype, bs, dot_order), b, dtype)
        return fresh[k]

    s = _solver(A1, L1, pre, dtype, bs, dot_order)
    if want is not None:
        assert s.views["A"]["columns"] in want, s.views
    if name == "small":
        assert A1.shape[0] <= 2560
    if name == "reorder":
        assert s.reorder_info["applied"]
    r1 = _run(s, b, dtype)
    assert r1[0] > 1 and (r1[1] or dtype == np.float32)
    views = s.views
    # A2, solved twice (the first solve after an update, then a repeat on the kept graphs)
    kept = _update(s, A2, L2, pre, dtype, bs)
    assert kept == _kept_expected(A1, A2, dtype)
    f2 = fresh_run(2, A2, L2)
    assert not np.array_equal(f2[3], r1[3])  # another system
    assert _same(_run(s, b, dtype), f2)
    assert _same(_run(s, b, dtype), f2)
    # back to A1
    assert _update(s, A1, L1, pre, dtype, bs) == _kept_expected(A2, A1, dtype)
    assert _same(_run(s, b, dtype), r1)
    # to the fp32-exact matrix and back: the fp32 copy of the values comes and goes
    assert _update(s, A3, L3, pre, dtype, bs) == _kept_expected(A1, A3, dtype)
    assert _same(_run(s, b, dtype), fresh_run(3, A3, L3))
    assert _update(s, A2, L2, pre, dtype, bs) == _kept_expected(A3, A2, dtype)
    assert _same(_run(s, b, dtype), f2)
    assert s.views["A"]["columns"] == views["A"]["columns"]  # the pattern was never rebuilt into another kind
    if name == "reorder":
        assert s.reorder_info["applied"]
    return s, f2


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("pre", KINDS)
@pytest.mark.parametrize("name", ["sdia", "sell16", "sell16j", "sell16x", "csr", "small"])
def test_updated_solver_equals_fresh_solver(gpu_ctx, monkeypatch, name, pre, dtype):
    _updated_equals_fresh(monkeypatch, name, pre, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("pre", ["none", "diagonal", "ext_spai", "ext_spai_scaled"])
def test_updated_bsr3_solver_equals_fresh_solver(gpu_ctx, monkeypatch, pre, dtype):
    s, _ = _updated_equals_fresh(monkeypatch, "bsr3", pre, dtype)
    assert s.A.block_size == 3


@pytest.mark.parametrize("pre", ["none", "diagonal", "ext_spai", "ext_spai_scaled", "ainv"])
def test_updated_reordered_solver_equals_fresh_solver(gpu_ctx, monkeypatch, pre):
    _updated_equals_fresh(monkeypatch, "reorder", pre, np.float64)


@pytest.mark.parametrize("pre", ["none", "diagonal", "ext_spai", "ic"])
def test_updated_solver_equals_fresh_solver_in_parity_dot_order(gpu_ctx, monkeypatch, pre):
    _updated_equals_fresh(monkeypatch, "sdia", pre, np.float64, dot_order="openblas")


@pytest.mark.parametrize("pre", ["ext_spai", "ext_spai_scaled"])
def test_solve_multi_after_an_update(gpu_ctx, monkeypatch, pre):
    (A1, A2, _A3), (L1, L2, _L3) = _matrices("sdia")
    rng = np.random.default_rng(3)
    B = torch.as_tensor(rng.normal(size=(A1.shape[0], 3)), device="cuda").contiguous()

    def multi(s):
        X = torch.zeros_like(B)
        res, _t = s.solve_multi(B, X, rtol=1e-8, return_history=True)
        return res, X.cpu().numpy()

    s = _solver(A1, L1, pre, np.float64)
    first = multi(s)  # captures solve_multi's graphs on A1
    assert _update(s, A2, L2, pre, np.float64) == _kept_expected(A1, A2, np.float64)
    got = multi(s)
    ref = multi(_solver(A2, L2, pre, np.float64))
    assert not np.array_equal(got[1], first[1])
    assert np.array_equal(got[1], ref[1])
    for (it, conv, h), (it2, conv2, h2) in zip(got[0], ref[0]):
        assert it == it2 and conv and conv2 and np.array_equal(h, h2)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def _one_entry_more(A):
    B = sp.lil_matrix(A)
    i = A.shape[0] // 2
    free = np.setdiff1d(np.arange(A.shape[0]), A.indices[A.indptr[i]:A.indptr[i + 1]])
    B[i, free[0]] = 0.125
    return _csr(B)


def _one_entry_less(A):
    B = _csr(A).copy()
    i = A.shape[0] // 2
    p = B.indptr[i] + (0 if B.indices[B.indptr[i]] != i else 1)  # an off-diagonal entry of row i
    keep = np.ones(B.nnz, dtype=bool)
    keep[p] = False
    indptr = B.indptr.copy()
    indptr[i + 1:] -= 1
    return sp.csr_matrix((B.data[keep], B.indices[keep], indptr), shape=B.shape)


def _one_entry_moved(A):
    """The same row lengths and entry count, one column index another one."""
    B = _csr(A).copy()
    i = A.shape[0] // 2
    row = B.indices[B.indptr[i]:B.indptr[i + 1]]
    free = np.setdiff1d(np.arange(row[-1] + 1, A.shape[0]), row)
    B.indices[B.indptr[i + 1] - 1] = free[0]  # past the row's last column: the row stays sorted
    return B


def test_another_pattern_or_dtype_is_refused_and_the_solver_keeps_its_system(gpu_ctx):
    from learningsparsepreconditioner4gpu_amd import _lib

    (A1, A2, _A3), (L1, _L2, _L3) = _matrices("sdia")
    b = _rhs(A1, np.float64)
    s = _solver(A1, L1, "ext_spai", np.float64)
    r1 = _run(s, b, np.float64)
    before = s.A.to_scipy()
    for bad in (_one_entry_more(A2), _one_entry_less(A2), _one_entry_moved(A2)):
        with pytest.raises(_lib.LspcgError) as e:
            s.update_matrix(bad)
        assert e.value.code == _lib.ERR_FORMAT
    with pytest.raises(TypeError):
        s.update_matrix(_typed(A2, np.float32))
    after = s.A.to_scipy()
    assert np.array_equal(before.data, after.data) and np.array_equal(before.indices, after.indices)
    assert _same(_run(s, b, np.float64), r1)


def test_set_values_without_update_matrix_makes_the_solves_raise(gpu_ctx):
    (A1, A2, _A3), (L1, L2, _L3) = _matrices("sdia")
    b = _rhs(A1, np.float64)
    s = _solver(A1, L1, "ext_spai", np.float64)
    _run(s, b, np.float64)
    s.A.set_values(A2.data, indptr=A2.indptr.astype(np.int32), indices=A2.indices.astype(np.int32))
    x = torch.zeros_like(b)
    with pytest.raises(RuntimeError, match="update_matrix"):
        s.solve(b, x)
    with pytest.raises(RuntimeError, match="update_matrix"):
        s.solve_multi(torch.stack([b, b], 1).contiguous(), torch.zeros(b.numel(), 2, dtype=b.dtype, device="cuda"))
    with pytest.raises(RuntimeError, match="update_matrix"):
        s(b, x)
    t, kept = s.update_matrix()  # None: self.A was changed in place
    assert kept == _kept_expected(A1, A2, np.float64)
    s.set_spai(L2, EPS)
    assert _same(_run(s, b, np.float64), _run(_solver(A2, L2, "ext_spai", np.float64), b, np.float64))


# ---------------------------------------------------------------------------
# set_values on a matrix with a prepare_spmv copy
# ---------------------------------------------------------------------------
def _shuffled_kuhn():
    K = _csr(P.kuhn_laplacian(15))
    perm = np.random.default_rng(2).permutation(K.shape[0])
    return _csr(K[perm][:, perm])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", ["sdia", "sell16", "reordered"])
def test_set_values_refills_the_prepare_spmv_copy(gpu_ctx, monkeypatch, case, dtype):
    from learningsparsepreconditioner4gpu_amd import _lib
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    monkeypatch.setenv("LSPCG_REORDER", "1" if case == "reordered" else "0")
    A1 = {"sdia": lambda: _csr(P.kuhn_laplacian(15)), "sell16": _band, "reordered": _shuffled_kuhn}[case]()
    A2 = _typed(_scaled(A1), dtype)
    D = DeviceMatrix.from_scipy(_typed(A1, dtype), dtype=dtype)
    kind = D.prepare_spmv()
    assert kind == {"sdia": 1, "sell16": 16}.get(case, kind) and kind != 0
    assert D.spmv_reorder_info["applied"] == (case == "reordered")
    x = np.random.default_rng(1).normal(size=A1.shape[0]).astype(dtype)
    xt = torch.as_tensor(x, device="cuda")
    assert np.array_equal(D.matvec(xt).cpu().numpy(), _typed(A1, dtype) @ x)
    # another pattern: refused, nothing written (the copy still multiplies by A1)
    with pytest.raises(_lib.LspcgError) as e:
        D.set_values(A2.data, indices=_one_entry_moved(A1).indices.astype(np.int32))
    assert e.value.code == _lib.ERR_FORMAT
    assert np.array_equal(D.matvec(xt).cpu().numpy(), _typed(A1, dtype) @ x)
    # host arrays, then device tensors
    D.set_values(A2.data, indptr=A2.indptr.astype(np.int32), indices=A2.indices.astype(np.int32))
    assert np.array_equal(D.matvec(xt).cpu().numpy(), A2 @ x)
    assert D.spmv_reorder_info["applied"] == (case == "reordered")
    D.set_values(torch.as_tensor(_typed(A1, dtype).data, device="cuda"),
                 indptr=torch.as_tensor(A1.indptr.astype(np.int32), device="cuda"),
                 indices=torch.as_tensor(A1.indices.astype(np.int32), device="cuda"))
    assert np.array_equal(D.matvec(xt).cpu().numpy(), _typed(A1, dtype) @ x)
    D.set_values(A2.data)
    assert np.array_equal(D.to_scipy().data, A2.data)
    assert D.prepare_spmv() == kind
    assert np.array_equal(D.matvec(xt).cpu().numpy(), A2 @ x)


# ---------------------------------------------------------------------------
# assemble(out=)
# ---------------------------------------------------------------------------
def _edges(A, bs):
    """Row-major sorted block edges and blocks of A (scalar: [E], bs 3: [E, 3, 3])."""
    if bs == 1:
        C = _csr(A).tocoo()
        return torch.as_tensor(np.stack([C.row, C.col]).astype(np.int64)), torch.as_tensor(C.data)
    B = sp.bsr_matrix(_csr(A), blocksize=(bs, bs))
    B.sort_indices()
    rows = np.repeat(np.arange(B.shape[0] // bs), np.diff(B.indptr))
    return torch.as_tensor(np.stack([rows, B.indices]).astype(np.int64)), torch.as_tensor(B.data.copy())


def _arrays(D):
    M = D.to_scipy()
    return M.indptr.copy(), M.indices.copy(), M.data.copy()


def _same_arrays(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", ["scalar", "masked", "bsr3", "scalar-from-blocks"])
def test_assemble_into_equals_a_fresh_assemble(gpu_ctx, case):
    from learningsparsepreconditioner4gpu_amd import _lib
    from learningsparsepreconditioner4gpu_amd.sparse import assemble

    if case in ("scalar", "masked"):
        A, mask, _ = P.poisson2d_grid(24, 20)
        bs, block_output = 1, False
    else:
        A, mask, _ = P.elasticity_box(6, 5, 5)
        bs, block_output = 3, case == "bsr3"
    A = _csr(A)
    n = A.shape[0]
    ei, bl1 = _edges(A, bs)
    _, bl2 = _edges(_scaled(A), bs)
    m = None if case == "scalar" else torch.as_tensor(np.asarray(mask, dtype=np.float64).reshape(-1))
    if m is not None:
        assert 0 < int((m == 0).sum()) < n
    kw = dict(n=n, mask=m, dtype=torch.float64, block_output=block_output)
    out = assemble(ei, bl1, **kw)
    fresh1, fresh2 = _arrays(out), _arrays(assemble(ei, bl2, **kw))
    assert not np.array_equal(fresh1[2], fresh2[2])
    v0 = out.values_version
    assert assemble(ei, bl2, out=out, **kw) is out
    assert out.values_version == v0 + 1
    assert _same_arrays(_arrays(out), fresh2)
    # refusals leave `out` bit for bit as it was
    if m is not None:  # a mask that differs in one node
        m2 = m.clone()
        i = int(torch.nonzero(m2 != 0)[n // 3])
        m2[i] = 0.0
        if block_output:  # BSR output keeps the block pattern whatever the mask: the same pattern, written
            assemble(ei, bl1, out=out, **dict(kw, mask=m2))
            assert _same_arrays(_arrays(out), _arrays(assemble(ei, bl1, **dict(kw, mask=m2))))
            assemble(ei, bl2, out=out, **kw)
            v0 += 2
        else:
            with pytest.raises(_lib.LspcgError) as e:
                assemble(ei, bl1, out=out, **dict(kw, mask=m2))
            assert e.value.code == _lib.ERR_FORMAT
        assert _same_arrays(_arrays(out), fresh2)
    if not block_output:  # a value that became exactly 0: scalar output drops it
        bl0 = bl1.clone()
        kept = np.flatnonzero(np.isin(_edge_keys(ei, bs, bl0), _entry_keys(fresh1, n)))
        bl0.reshape(-1)[int(kept[len(kept) // 2])] = 0.0
        with pytest.raises(_lib.LspcgError) as e:
            assemble(ei, bl0, out=out, **kw)
        assert e.value.code == _lib.ERR_FORMAT
        assert _same_arrays(_arrays(out), fresh2)
    assert out.values_version == v0 + 1
    assemble(ei, bl1, out=out, **kw)
    assert _same_arrays(_arrays(out), fresh1)


def _edge_keys(ei, bs, blocks):
    """row * n_big + col of every scalar entry of the block edges, in the blocks' flat order; entries
    that are stored zeros get -1 (they are dropped anyway)."""
    r, c = ei[0].numpy(), ei[1].numpy()
    a = np.arange(bs)
    rows = (r[:, None, None] * bs + a[None, :, None]) + 0 * a[None, None, :]
    cols = (c[:, None, None] * bs + a[None, None, :]) + 0 * a[None, :, None]
    key = (rows.astype(np.int64) << 32) + cols
    key = key.reshape(-1)
    key[blocks.reshape(-1).numpy() == 0] = -1
    off = rows.reshape(-1) != cols.reshape(-1)  # keep off the diagonal: masked rows get their 1 there
    return np.where(off, key, -1)


def _entry_keys(arrays, n):
    indptr, indices, _ = arrays
    rows = np.repeat(np.arange(n), np.diff(indptr)).astype(np.int64)
    return (rows << 32) + indices


# ---------------------------------------------------------------------------
# IC(0): numeric-only refactorization
# ---------------------------------------------------------------------------
def _boosted(A):
    """The same pattern, strictly diagonally dominant: IC(0) exists whatever A's own values."""
    A = _csr(A).copy()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    diag = rows == A.indices
    off = np.bincount(rows[~diag], weights=np.abs(A.data[~diag]), minlength=A.shape[0])
    A.data[diag] = off[rows[diag]] + 1.0
    return A


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_ic_update_equals_fresh_on_the_spd_cases(gpu_ctx, case, dtype):
    """Starts on the diagonally boosted matrix of the case's pattern (IC(0) always exists there) and
    updates to the case's own A1 and A2: wherever a fresh "ic" solver exists the updated one gives its
    bits; where the fresh one breaks down (synthetic-2048 is no M-matrix) the update breaks down too,
    the solves then raise, and the next good update restores a fresh solver's bits."""
    from learningsparsepreconditioner4gpu_amd import _lib

    name, A, _mask = _cases.spd_cases()[case]
    A1 = _csr(A)
    A0, A2 = _boosted(A1), _scaled(A1)
    b = _rhs(A1, dtype)
    s = _solver(A0, None, "ic", dtype)
    r0 = _run(s, b, dtype)
    assert r0[1]
    prev, failed = A0, False
    for target in (A1, A2, A0):
        was, prev = prev, target  # (a broken-down update has installed the target's A side all the same)
        try:
            ref = _run(_solver(target, None, "ic", dtype), b, dtype)
        except _lib.LspcgError as e:
            assert e.code == _lib.ERR_BREAKDOWN, name
            with pytest.raises(_lib.LspcgError) as e2:
                s.update_matrix(_typed(target, dtype))
            assert e2.value.code == _lib.ERR_BREAKDOWN, name
            with pytest.raises(RuntimeError):
                s.solve(b, torch.zeros_like(b))
            failed = True
            continue
        t, kept = s.update_matrix(_typed(target, dtype))
        # (a failed update drops the graphs: the update after it keeps none)
        assert kept == (False if failed else _kept_expected(was, target, dtype)), name
        failed = False
        assert _same(_run(s, b, dtype), ref), name
    assert _same(_run(s, b, dtype), r0), name


def test_ic_breakdown_then_a_good_update(gpu_ctx):
    from learningsparsepreconditioner4gpu_amd import _lib

    (A1, A2, _A3), _ = _matrices("sdia")
    bad = A1.copy()
    rows = np.repeat(np.arange(A1.shape[0]), np.diff(A1.indptr))
    bad.data[rows == A1.indices] *= 0.01  # the same pattern, no longer positive definite
    b = _rhs(A1, np.float64)
    s = _solver(A1, None, "ic", np.float64)
    r1 = _run(s, b, np.float64)
    with pytest.raises(_lib.LspcgError) as e:
        s.update_matrix(bad)
    assert e.value.code == _lib.ERR_BREAKDOWN
    with pytest.raises(RuntimeError, match="update_matrix"):
        s.solve(b, torch.zeros_like(b))
    s.update_matrix(A2)
    assert _same(_run(s, b, np.float64), _run(_solver(A2, None, "ic", np.float64), b, np.float64))
    s.update_matrix(A1)
    assert _same(_run(s, b, np.float64), r1)


def test_ic_graphs_survive_other_work_on_the_default_stream(gpu_ctx):
    """Two solves of one "ic" solver with unrelated device work and a host read in between (what every
    update does on the context's stream): the second solve replays the first one's graphs and repeats
    its bits.  With the dequeue counter reset by a memset node inside the graph it came out NaN from
    the second triangular solve on; the reset now runs in the fill kernel."""
    (A1, _A2, _A3), _ = _matrices("sdia")
    b = _rhs(A1, np.float64)
    s = _solver(A1, None, "ic", np.float64)
    r1 = _run(s, b, np.float64)
    assert r1[1]
    assert float((b * 2.0).sum().item()) != 0.0
    assert _same(_run(s, b, np.float64), r1)


def _weak_diagonal(A, factor):
    """The same pattern with the diagonal scaled down: no longer positive definite, not fp32-exact."""
    B = _csr(A).copy()
    rows = np.repeat(np.arange(B.shape[0]), np.diff(B.indptr))
    B.data[rows == B.indices] *= factor
    return B


def test_failed_update_across_an_exactness_transition_drops_the_graphs(gpu_ctx):
    """fp32-exact A1 (graphs captured on the fp32 copy of its values) -> a matrix in full doubles
    whose IC(0) breaks down (the fp32 copy and the fp32 SELL values are gone before the
    factorization fails) -> a good matrix in full doubles.  Between the last two no view moves, yet
    the graphs of A1 hold freed arrays: the failed update has dropped them, the next one reports none
    kept, and the solve gives a fresh solver's bits."""
    from learningsparsepreconditioner4gpu_amd import _lib

    A1 = _csr(P.poisson2d_grid(24, 20)[0])
    bad, A2 = _weak_diagonal(A1, 0.0123), _scaled(A1)
    assert _is_f32_exact(A1) and not _is_f32_exact(bad) and not _is_f32_exact(A2)
    b = _rhs(A1, np.float64)
    s = _solver(A1, None, "ic", np.float64)
    assert s.views["A"]["value_bytes"] in (0, 4), s.views  # the compact copy is in use
    r1 = _run(s, b, np.float64)
    assert r1[1] and r1[0] > 4
    with pytest.raises(_lib.LspcgError) as e:
        s.update_matrix(bad)
    assert e.value.code == _lib.ERR_BREAKDOWN
    t, kept = s.update_matrix(A2)
    assert kept is False
    assert _same(_run(s, b, np.float64), _run(_solver(A2, None, "ic", np.float64), b, np.float64))
    t, kept = s.update_matrix(A2)  # after a successful update the flag follows the views again
    assert kept is True
    assert s.update_matrix(A1)[1] is False
    assert _same(_run(s, b, np.float64), r1)


def test_ainv_breakdown_in_an_update_makes_the_solves_raise(gpu_ctx):
    """AINV(0) of the new values is computed before the solver is touched: when it breaks down the
    solver stays behind its matrix and refuses to solve, and a good update restores a fresh solver's bits."""
    from learningsparsepreconditioner4gpu_amd import _lib

    (A1, A2, _A3), _ = _matrices("sdia")
    b = _rhs(A1, np.float64)
    s = _solver(A1, None, "ainv", np.float64)
    _run(s, b, np.float64)
    with pytest.raises(_lib.LspcgError) as e:
        s.update_matrix(_weak_diagonal(A1, 0.01))
    assert e.value.code == _lib.ERR_BREAKDOWN
    with pytest.raises(RuntimeError, match="update_matrix"):
        s.solve(b, torch.zeros_like(b))
    s.update_matrix(A2)
    assert _same(_run(s, b, np.float64), _run(_solver(A2, None, "ainv", np.float64), b, np.float64))


def test_update_matrix_leaves_the_callers_bsr_matrix_as_it_is(gpu_ctx):
    A = _csr(P.elasticity_box(4, 3, 3)[0])
    B = sp.bsr_matrix(_scaled(A), blocksize=(3, 3))
    # rows stored in descending block-column order
    for i in range(B.shape[0] // 3):
        sl = slice(B.indptr[i], B.indptr[i + 1])
        B.indices[sl], B.data[sl] = B.indices[sl][::-1].copy(), B.data[sl][::-1].copy()
    B.has_sorted_indices = False
    before = (B.indices.copy(), B.data.copy())
    s = _solver(A, None, "none", np.float64, bs=3)
    s.update_matrix(B)
    assert np.array_equal(B.indices, before[0]) and np.array_equal(B.data, before[1])
    b = _rhs(A, np.float64)
    assert _same(_run(s, b, np.float64), _run(_solver(_scaled(A), None, "none", np.float64, bs=3), b, np.float64))


def test_a_given_ic_factor_is_left_alone(gpu_ctx):
    """set_ic_factor's L does not follow A: after an update the solver applies the same factor to the
    new A, as a fresh solver with that factor does."""
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    (A1, A2, _A3), _ = _matrices("sdia")
    Lg = DeviceMatrix.from_scipy(A1).ic0()[0].to_scipy()
    b = _rhs(A1, np.float64)
    s = _solver(A1, None, "ic", np.float64)
    s.set_ic_factor(Lg)
    _run(s, b, np.float64)
    t, kept = s.update_matrix(A2)
    assert kept == _kept_expected(A1, A2, np.float64)
    f = _solver(A2, None, "ic", np.float64)
    f.set_ic_factor(Lg)
    assert _same(_run(s, b, np.float64), _run(f, b, np.float64))


# ---------------------------------------------------------------------------
# infer.run(reuse_solver=True)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True])
def test_infer_run_with_a_reused_solver_equals_the_default_path(gpu_ctx, tmp_path, scaled):
    from learningsparsepreconditioner4gpu_amd import infer
    from learningsparsepreconditioner4gpu_amd.dataset import FolderWriter
    from learningsparsepreconditioner4gpu_amd.workspace import ScaledInferenceWorkspace, SimpleInferenceWorkspace

    A, mask, feats = P.heat_tet(7, 6, 5)
    A = _csr(A)
    w = FolderWriter(str(tmp_path / "fixed"), block_size=1, is_fixed_topology=True, save_rhs=1, seed=5)
    w.write_topology(A)
    for k in range(3):
        w.append(A if k == 0 else _scaled(A, seed=10 + k), mask, np.asarray(feats, dtype=np.float64))
    samples = infer.folder_dataset(str(tmp_path / "fixed"), block_size=1, fixed_topology=True)
    assert len(samples) == 3
    cls = ScaledInferenceWorkspace if scaled else SimpleInferenceWorkspace
    ws = cls(node_features=samples[0].x.shape[1], edge_features=samples[0].edge_attr.shape[1], seed=0)
    x_ref, x_got = {}, {}
    ref = infer.run(samples, ws, rtol=1e-8, warmup=1, solutions=x_ref)
    got = infer.run(samples, ws, rtol=1e-8, warmup=1, reuse_solver=True, solutions=x_got)
    assert [r.index for r in got] == [r.index for r in ref] == [0, 1, 2]
    assert [r.iters for r in got] == [r.iters for r in ref]
    assert [r.converged for r in got] == [r.converged for r in ref] and all(r.iters > 1 for r in got)
    assert len({r.iters for r in ref}) > 1 or not torch.equal(x_ref[0], x_ref[1])  # three different systems
    for i in range(3):
        assert torch.equal(x_got[i], x_ref[i]), i
    with pytest.raises(ValueError):
        infer.run(samples, ws, reuse_solver=True, batch=2)
