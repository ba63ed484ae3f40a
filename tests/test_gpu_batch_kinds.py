"""GPU parity of the lockstep batch for every preconditioner kind but ext_spai (which
tests/test_gpu_batch.py holds): no preconditioner and Jacobi (three launches per lockstep
iteration, the per-system reduction inside the elementwise r update), ext_spai_scaled (five
launches with the divisions by diag(A)) and ainv (run as ext_spai with ε = 0).

Every system of a window must come out as ``PreconditionedConjugateGradient`` of the same kind
(and the CPU oracle with exact dots) returns it alone: the same iteration count and verdict, the
residual history within 1e-12 relative and the iterate within 1e-12 relative (fp64; 1e-5 fp32) --
the tolerances tests/test_gpu_batch.py holds the ext_spai batch to.  The shapes are that file's:
ragged sizes (tile padding), a system smaller than one tile (7 x 9), an exact multiple of 256
(64 x 64, also above the one-workgroup bound of 2,560 rows), and heat_tet(7, 6, 5), whose diagonal
varies (minimum 0.22), so a wrong d shows.  The Kuhn systems take a seeded random right-hand side:
A @ ones converges plain CG on them in 8 iterations.
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
KINDS = ("none", "diagonal", "ext_spai_scaled")


def _rhs(A, k, kuhn):
    if kuhn:
        return A @ np.random.default_rng(100 + k).normal(size=A.shape[0])
    return A @ np.ones(A.shape[0])


def _systems():
    """(A, L, b) of the seven systems of tests/test_gpu_batch.py."""
    As, kuhn = [], []
    for nx, ny in ((24, 20), (40, 33), (7, 9), (64, 64)):
        As.append(sp.csr_matrix(P.poisson2d_grid(nx, ny)[0]))
        kuhn.append(False)
    for m in (9, 23):
        As.append(sp.csr_matrix(P.kuhn_laplacian(m)))
        kuhn.append(True)
    As.append(sp.csr_matrix(P.heat_tet(7, 6, 5)[0]))
    kuhn.append(False)
    Ls = [_cases.spai_like(A, seed=k) for k, A in enumerate(As)]
    bs_ = [_rhs(A, k, kuhn[k]) for k, A in enumerate(As)]
    return As, Ls, bs_


@pytest.fixture(scope="module")
def systems():
    return _systems()


def _needs_L(kind):
    return kind in ("ext_spai", "ext_spai_scaled")


def _single(A, L, b, kind, rtol, max_iter=0, dtype=np.float64, bs=1, eps=EPS):
    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient

    s = PreconditionedConjugateGradient(A, device="cuda", preconditioner=kind, dtype=dtype, block_size=bs)
    if _needs_L(kind):
        s.set_spai(L, eps, block_size=bs)
    bt = torch.from_numpy(np.asarray(b).astype(dtype)).cuda()
    x = torch.zeros_like(bt)
    it, conv, _, h = s.solve(bt, x, rtol=rtol, max_iter=max_iter, return_history=True)
    return it, conv, x.cpu().numpy(), h


def _make(As, Ls, kind, dtype=np.float64, bsz=1, eps=EPS):
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient

    return BatchedConjugateGradient(As, Ls if _needs_L(kind) else None, eps, dtype=dtype, block_size=bsz,
                                    preconditioner=kind)


def _solve(B, bs_, rtol, max_iter=0, dtype=np.float64):
    bt = [torch.from_numpy(np.asarray(b).astype(dtype)).cuda() for b in bs_]
    xs = [torch.zeros_like(b) for b in bt]
    res, t = B.solve(bt, xs, rtol=rtol, max_iter=max_iter, return_history=True)
    assert t > 0
    return res, [x.cpu().numpy() for x in xs]


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _oracle_operator(kind, A, L):
    if kind == "none":
        return None
    if kind == "diagonal":
        return O.diagonal_operator(A)
    return O.spai_scaled_operator(A, sp.csr_matrix(L), EPS)


@pytest.fixture(scope="module")
def references(systems):
    """Per kind, each system's single solve and oracle solve (rtol 1e-8), computed once on first use."""
    As, Ls, bs_ = systems
    cache = {}

    def get(kind):
        if kind not in cache:
            single = [_single(A, L, b, kind, 1e-8) for A, L, b in zip(As, Ls, bs_)]
            oracle = [O.pcg(A, b, _oracle_operator(kind, A, L), rtol=1e-8, dot="exact") for A, L, b in zip(As, Ls, bs_)]
            cache[kind] = (single, oracle)
        return cache[kind]

    return get


@pytest.mark.parametrize("reduce", ["auto", "0", "1"])
@pytest.mark.parametrize("kind", KINDS)
def test_kind_matches_single_and_oracle(gpu_ctx, monkeypatch, systems, references, kind, reduce):
    """reduce: the window's reductions (auto / 0 = per-system last arrivers / 1 = consumer sums)."""
    if reduce != "auto":
        monkeypatch.setenv("LSPCG_BATCH_REDUCE", reduce)
    else:
        monkeypatch.delenv("LSPCG_BATCH_REDUCE", raising=False)
    As, Ls, bs_ = systems
    single, oracle = references(kind)
    res, xs = _solve(_make(As, Ls, kind), bs_, 1e-8)
    same_bits = 0
    for A, (it, conv, h), x, (it1, conv1, x1, h1), (it_o, x_o, h_o) in zip(As, res, xs, single, oracle):
        print(f"{kind} reduce={reduce} n={A.shape[0]}: batch {it} {conv}, single {it1} {conv1}, oracle {it_o}; "
              f"x vs single {_rel(x, x1):.2e}, vs oracle {_rel(x, x_o):.2e}")
        assert (it, conv) == (it1, conv1), (A.shape, it, it1)
        np.testing.assert_allclose(h, h1, rtol=1e-12, atol=0)
        assert _rel(x, x1) <= 1e-12
        same_bits += int(np.array_equal(x, x1))
        assert it == it_o
        np.testing.assert_allclose(h, h_o, rtol=1e-12, atol=0)
        assert _rel(x, x_o) <= 1e-12
    print(f"{kind}: batch iterates bit-identical to single solves: {same_bits}/{len(As)}")


@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("kind", KINDS)
def test_kind_small_systems_one_workgroup_each(gpu_ctx, monkeypatch, kind, small):
    """The window of tests/test_gpu_batch.py's small-mode test (every system <= 2,560 rows, one zero
    right-hand side, max_iter 0 and 12): one workgroup per system in one launch (small = 1) or the
    lockstep phases (LSPCG_BATCH_SMALL=0); each system matches its single solve."""
    monkeypatch.setenv("LSPCG_BATCH_SMALL", small)
    As = [sp.csr_matrix(P.poisson2d_grid(nx, ny)[0]) for nx, ny in ((24, 20), (40, 33), (7, 9), (45, 50))]
    As += [sp.csr_matrix(P.kuhn_laplacian(9)), sp.csr_matrix(P.kuhn_laplacian(13)), sp.csr_matrix(P.heat_tet(7, 6, 5)[0])]
    assert max(A.shape[0] for A in As) <= 2560
    Ls = [_cases.spai_like(A, seed=k) for k, A in enumerate(As)]
    bs_ = [_rhs(A, k, k in (4, 5)) for k, A in enumerate(As)]
    bs_[2] = np.zeros(As[2].shape[0])
    B = _make(As, Ls, kind)
    for max_iter in (0, 12):
        res, xs = _solve(B, bs_, 1e-9, max_iter=max_iter)
        assert res[2][0] == 0 and res[2][1] and not xs[2].any()
        for A, L, b, (it, conv, h), x in zip(As, Ls, bs_, res, xs):
            it1, conv1, x1, h1 = _single(A, L, b, kind, 1e-9, max_iter=max_iter)
            assert (it, conv) == (it1, conv1), (A.shape, it, it1)
            np.testing.assert_allclose(h, h1, rtol=1e-12, atol=0)
            assert _rel(x, x1) <= 1e-12 or not np.linalg.norm(x1)


@pytest.mark.parametrize("kind", KINDS)
def test_kind_fp32(gpu_ctx, systems, kind):
    As, Ls, bs_ = (v[:5] for v in systems)
    As = [A.astype(np.float32) for A in As]
    Ls = [L.astype(np.float32) for L in Ls]
    bs_ = [b.astype(np.float32) for b in bs_]
    res, xs = _solve(_make(As, Ls, kind, dtype=np.float32), bs_, 1e-5, dtype=np.float32)
    for A, L, b, (it, conv, h), x in zip(As, Ls, bs_, res, xs):
        it1, conv1, x1, h1 = _single(A, L, b, kind, 1e-5, dtype=np.float32)
        assert (it, conv) == (it1, conv1), (A.shape, it, it1)
        assert _rel(x.astype(np.float64), x1.astype(np.float64)) <= 1e-5


@pytest.mark.parametrize("reduce", ["0", "1"])
@pytest.mark.parametrize("kind", KINDS)
def test_kind_bsr3(gpu_ctx, monkeypatch, kind, reduce):
    """BSR 3 x 3: three elementwise tiles per SpMV row tile, so the r update's per-system reduction
    runs over more tiles than the SpMVs' (tickets and partials sized for that launch)."""
    monkeypatch.setenv("LSPCG_BATCH_REDUCE", reduce)
    eps = 1e-3
    As = [sp.csr_matrix(P.elasticity_box(*dims)[0]) for dims in ((9, 5, 5), (12, 6, 5), (5, 4, 4))]
    Ls = [_cases.spai_like(A, seed=k, scale=0.02) for k, A in enumerate(As)]
    bs_ = [A @ np.ones(A.shape[0]) for A in As]
    res, xs = _solve(_make(As, Ls, kind, bsz=3, eps=eps), bs_, 1e-8, max_iter=60)
    for A, L, b, (it, conv, h), x in zip(As, Ls, bs_, res, xs):
        it1, conv1, x1, h1 = _single(A, L, b, kind, 1e-8, max_iter=60, bs=3, eps=eps)
        assert (it, conv) == (it1, conv1)
        np.testing.assert_allclose(h, h1, rtol=1e-12, atol=0)
        assert _rel(x, x1) <= 1e-12


@pytest.mark.parametrize("kind", KINDS)
def test_kind_edge_cases_and_reuse(gpu_ctx, systems, references, kind):
    """A zero right-hand side (scipy returns b, 0 iterations), a max_iter = 15 stop per system, a
    second solve on the same handle with other right-hand sides, and the same bits from two solves
    of the same inputs."""
    As, Ls, bs2 = (v[:4] for v in systems)
    rng = np.random.default_rng(0)
    bs_ = [A @ rng.normal(size=A.shape[0]) for A in As]
    bs_[1] = np.zeros(As[1].shape[0])
    B = _make(As, Ls, kind)
    res, xs = _solve(B, bs_, 1e-10, max_iter=15)
    assert res[1][0] == 0 and res[1][1] and not xs[1].any()
    for k in (0, 2, 3):
        it1, conv1, x1, h1 = _single(As[k], Ls[k], bs_[k], kind, 1e-10, max_iter=15)
        assert (res[k][0], res[k][1]) == (it1, conv1)
        np.testing.assert_allclose(res[k][2], h1, rtol=1e-12, atol=0)
        assert _rel(xs[k], x1) <= 1e-12
    # reuse: new right-hand sides, default max_iter (each system's n); twice, for the bits
    single, _ = references(kind)
    res2, x2 = _solve(B, bs2, 1e-8)
    res3, x3 = _solve(B, bs2, 1e-8)
    for k in range(len(As)):
        it1, conv1, x1, _ = single[k]
        assert (res2[k][0], res2[k][1]) == (it1, conv1)
        assert _rel(x2[k], x1) <= 1e-12
        assert (res3[k][0], res3[k][1]) == (res2[k][0], res2[k][1])
        assert np.array_equal(res3[k][2], res2[k][2]) and np.array_equal(x3[k], x2[k])


def test_ainv_matches_single(gpu_ctx, systems):
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient, PreconditionedConjugateGradient

    As, _, bs_ = (v[:4] for v in systems)
    B = BatchedConjugateGradient(As, preconditioner="ainv")
    res, xs = _solve(B, bs_, 1e-8)
    for A, b, (it, conv, h), x in zip(As, bs_, res, xs):
        s = PreconditionedConjugateGradient(A, device="cuda", preconditioner="ainv")
        bt = torch.from_numpy(b).cuda()
        x1 = torch.zeros_like(bt)
        it1, conv1, _, h1 = s.solve(bt, x1, rtol=1e-8, return_history=True)
        assert (it, conv) == (it1, conv1)
        np.testing.assert_allclose(h, h1, rtol=1e-12, atol=0)
        assert _rel(x, x1.cpu().numpy()) <= 1e-12


def test_create_precond_arguments(gpu_ctx, systems):
    from learningsparsepreconditioner4gpu_amd import _lib
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient
    from learningsparsepreconditioner4gpu_amd.sparse import Context, DeviceMatrix

    As, Ls, _ = systems
    ctx = Context.get()
    Ad = [DeviceMatrix.from_scipy(A, ctx=ctx) for A in As[:2]]
    Ld = [DeviceMatrix.from_scipy(L, ctx=ctx) for L in Ls[:2]]
    ha = (C.c_void_p * 2)(*[M.handle.value for M in Ad])
    hl = (C.c_void_p * 2)(*[M.handle.value for M in Ld])

    def create(kind, L):
        h = C.c_void_p()
        try:
            _lib.call("lspcg_batch_create_precond", ctx.handle, 2, ha, L, _lib.PRECOND[kind], EPS, C.byref(h))
        except _lib.LspcgError as e:
            return e.code
        _lib.call("lspcg_batch_destroy", h)
        return _lib.OK

    assert create("ic", None) == _lib.ERR_UNSUPPORTED
    assert create("ic", hl) == _lib.ERR_UNSUPPORTED
    assert create("ext_spai", None) == _lib.ERR_ARG
    assert create("ext_spai_scaled", None) == _lib.ERR_ARG
    assert create("none", hl) == _lib.ERR_ARG
    assert create("diagonal", hl) == _lib.ERR_ARG
    assert create("diagonal", None) == _lib.OK
    assert create("ext_spai_scaled", hl) == _lib.OK
    with pytest.raises(TypeError):  # one dtype per batch, as today
        BatchedConjugateGradient([Ad[0], DeviceMatrix.from_scipy(As[1], dtype=np.float32, ctx=ctx)],
                                 preconditioner="diagonal")
    with pytest.raises(_lib.LspcgError):  # L of another size
        BatchedConjugateGradient(As[:2], [Ls[0], Ls[0]], EPS, preconditioner="ext_spai_scaled")


@pytest.fixture(scope="module")
def heat_window():
    from learningsparsepreconditioner4gpu_amd.infer import synthetic_dataset

    return synthetic_dataset("heat_batch8")


def _count_batch_solves(monkeypatch):
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient

    calls = []
    orig = BatchedConjugateGradient.solve

    def solve(self, *a, **kw):
        calls.append(self.preconditioner)
        return orig(self, *a, **kw)

    monkeypatch.setattr(BatchedConjugateGradient, "solve", solve)
    return calls


def _same_records(seq, bat, n):
    assert [r.index for r in bat] == list(range(n))
    for a, b in zip(seq, bat):
        assert a.converged and b.converged
        assert (a.iters, a.n, a.nnz) == (b.iters, b.n, b.nnz)
        assert abs(a.rel_res - b.rel_res) <= 1e-12 and b.rel_res <= 1e-8


def test_infer_scaled_workspace_batched_matches_sequential(gpu_ctx, monkeypatch, heat_window):
    from learningsparsepreconditioner4gpu_amd.infer import run
    from learningsparsepreconditioner4gpu_amd.workspace import ScaledInferenceWorkspace

    samples = heat_window
    ws = ScaledInferenceWorkspace(node_features=samples[0].x.shape[1], edge_features=1, seed=0)
    seq = run(samples, ws, rtol=1e-8, warmup=1)
    calls = _count_batch_solves(monkeypatch)
    for k in (3, 8):
        del calls[:]
        bat = run(samples, ws, rtol=1e-8, warmup=1, batch=k)
        assert calls and set(calls) == {"ext_spai_scaled"}  # not the silent one-at-a-time fall-back
        _same_records(seq, bat, len(samples))


@pytest.mark.parametrize("method", ["diagonal", "none"])
def test_infer_baseline_batched_matches_sequential(gpu_ctx, monkeypatch, heat_window, method):
    from learningsparsepreconditioner4gpu_amd.infer import run_baseline
    from learningsparsepreconditioner4gpu_amd.workspace import SimpleInferenceWorkspace

    samples = heat_window
    ws = SimpleInferenceWorkspace(node_features=samples[0].x.shape[1], edge_features=1, seed=0)
    seq = run_baseline(samples, ws, method, rtol=1e-8)
    calls = _count_batch_solves(monkeypatch)
    bat = run_baseline(samples, ws, method, rtol=1e-8, batch=8)
    assert calls and set(calls) == {method}
    _same_records(seq, bat, len(samples))


@pytest.fixture(scope="module")
def nonfinite_window():
    """An ordinary system, one whose alpha is not finite after iteration 0 (diag(+1, -1, ...), L = I,
    b = 1: p.Ap is exactly 0) and one whose right-hand side holds an inf (stops at k = 0), with each
    system's single solve per kind (max_iter 20), computed on first use."""
    As = [sp.csr_matrix(P.poisson2d_grid(24, 20)[0]),
          sp.diags(np.where(np.arange(600) % 2 == 0, 1.0, -1.0)).tocsr(),
          sp.csr_matrix(P.poisson2d_grid(40, 33)[0])]
    Ls = [_cases.spai_like(As[0], seed=0), sp.identity(600, format="csr"), _cases.spai_like(As[2], seed=2)]
    bs_ = [As[0] @ np.ones(As[0].shape[0]), np.ones(600), As[2] @ np.ones(As[2].shape[0])]
    bs_[2][5] = np.inf
    cache = {}

    def single(kind):
        if kind not in cache:
            cache[kind] = [_single(A, L, b, kind, 1e-8, max_iter=20, eps=1e-3) for A, L, b in zip(As, Ls, bs_)]
        return cache[kind]

    return As, Ls, bs_, single


@pytest.mark.parametrize("mode", ["last_arriver", "consumer_sums", "one_workgroup"])
@pytest.mark.parametrize("kind", ("none", "diagonal", "ext_spai", "ext_spai_scaled"))
def test_nonfinite_system_stops_alone(gpu_ctx, monkeypatch, nonfinite_window, kind, mode):
    """The non-finite stop (done == 3) in both lockstep reduction modes and in the window of
    one-workgroup solves: every system reports what its single solve reports (count, verdict,
    NaN-filled history), and the ordinary system beside the two stopped ones is not disturbed."""
    monkeypatch.delenv("LSPCG_BATCH_REDUCE", raising=False)
    if mode == "one_workgroup":
        monkeypatch.setenv("LSPCG_BATCH_SMALL", "1")
    else:
        monkeypatch.setenv("LSPCG_BATCH_SMALL", "0")
        monkeypatch.setenv("LSPCG_BATCH_REDUCE", "0" if mode == "last_arriver" else "1")
    As, Ls, bs_, single = nonfinite_window
    res, xs = _solve(_make(As, Ls, kind, eps=1e-3), bs_, 1e-8, max_iter=20)
    for k, ((it, conv, h), (it1, conv1, x1, h1)) in enumerate(zip(res, single(kind))):
        print(f"{kind} {mode} system {k}: batch {it} {conv} {h[:2]}, single {it1} {conv1} {h1[:2]}")
        assert (it, conv) == (it1, conv1), (k, it, it1)
        np.testing.assert_array_equal(h, h1)  # NaN and inf entries compare equal
    assert [r[:2] for r in res[1:]] == [(20, False), (20, False)]
    assert _rel(xs[0], single(kind)[0][2]) <= 1e-12
