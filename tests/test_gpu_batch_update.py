"""GPU: new values of A and L on a live lockstep batch (lspcg_batch_update,
BatchedConjugateGradient.update).  The standard is tests/test_gpu_update_matrix.py's: the same
kernels on the same values in the same order give the same bits, so an updated batch is compared
with a batch created on the resulting matrices by bit equality -- every system's count, verdict,
residual history and iterate.

The matrices are that file's: A1, A2 = D A1 D with D = diag(1 + 0.5 u), u seeded uniform (the same
pattern; not fp32-exact) and A3 = A1 rounded through fp32, each with its own `spai_like` factor.
D A D with d in [1, 1.5] of an SPD M-matrix is an SPD M-matrix, so CG converges and AINV(0) exists
on all three; every fresh run is asserted to converge in more than one iteration, so a frozen or
trivial solve cannot pass.  `graphs_kept` follows DESIGN.md §14's rule applied to the window: the
graphs survive between windows whose concatenated values are equally fp32-exact (always in fp32).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import linalg as O
from tests import _cases
from learningsparsepreconditioner4gpu_amd import problems as P

pytestmark = pytest.mark.gpu

EPS = 1e-3
MODES = {  # the three ways a window is run
    "one_workgroup": {},
    "consumer_sums": {"LSPCG_BATCH_SMALL": "0", "LSPCG_BATCH_REDUCE": "1"},
    "tickets": {"LSPCG_BATCH_SMALL": "0", "LSPCG_BATCH_REDUCE": "0"},
}


# ---- the helpers of tests/test_gpu_update_matrix.py ------------------------------------------
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


def _one_entry_more(A):
    B = sp.lil_matrix(A)
    i = A.shape[0] // 2
    free = np.setdiff1d(np.arange(A.shape[0]), A.indices[A.indptr[i]:A.indptr[i + 1]])
    B[i, free[0]] = 0.125
    return _csr(B)


def _one_entry_moved(A):
    """The same row lengths and entry count, one column index another one."""
    B = _csr(A).copy()
    i = A.shape[0] // 2
    row = B.indices[B.indptr[i]:B.indptr[i + 1]]
    free = np.setdiff1d(np.arange(row[-1] + 1, A.shape[0]), row)
    B.indices[B.indptr[i + 1] - 1] = free[0]  # past the row's last column: the row stays sorted
    return B


def _weak_diagonal(A, factor):
    """The same pattern with the diagonal scaled down: no longer positive definite."""
    B = _csr(A).copy()
    rows = np.repeat(np.arange(B.shape[0]), np.diff(B.indptr))
    B.data[rows == B.indices] *= factor
    return B


def _band(n=3008, seed=21, blk=64, offs=(1, 2, 3, 5, 8, 13, 21, 27, 29, 30, 31)):
    """Block-diagonal M-matrix of circulant 64-row blocks, 23 entries in every row: more than 16
    offsets per slice (no SELL-DIA), equal row lengths (no SELL-64J), columns within 16 bits."""
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


def _typed(A, dtype):
    return sp.csr_matrix((A.data.astype(dtype), A.indices, A.indptr), shape=A.shape)


# ---- windows ---------------------------------------------------------------------------------
WINDOWS = {
    # 480 rows (two 256-row tiles, the last partial), 63 (under one wave), 729, and a varying diagonal
    "small": (lambda: [P.poisson2d_grid(24, 20)[0], P.poisson2d_grid(7, 9)[0], P.kuhn_laplacian(9),
                       P.heat_tet(7, 6, 5)[0]], 1),
    # above the one-workgroup bound: SELL-DIA with a partial last slice, 16-bit SELL, a 5-point grid
    "large": (lambda: [P.kuhn_laplacian(15), _band(), P.poisson2d_grid(60, 50)[0]], 1),
    "bsr3": (lambda: [P.elasticity_box(5, 4, 4)[0], P.elasticity_box(9, 5, 5)[0], P.elasticity_box(12, 6, 5)[0]], 3),
}


@functools.lru_cache(maxsize=None)
def _window(name):
    """Per matrix set (0: A1, 1: A2, 2: A3) the window's matrices and factors, and the right-hand
    sides (of A1, seeded normal: A @ ones is an eigenvector of the shifted Laplacians); built once,
    never written to."""
    make, bs = WINDOWS[name]
    A1 = [_csr(A) for A in make()]
    sets = [A1, [_scaled(A, seed=7 + k) for k, A in enumerate(A1)], [_f32_exact_copy(A) for A in A1]]
    facs = []
    for s, As in enumerate(sets):
        Ls = [_cases.spai_like(A, seed=10 * s + k, scale=0.02 if bs == 3 else 0.05) for k, A in enumerate(As)]
        facs.append([_csr(sp.bsr_matrix(L, blocksize=(3, 3))) if bs == 3 else L for L in Ls])
    assert not any(_is_f32_exact(A) for A in sets[1]) and all(_is_f32_exact(A) for A in sets[2])
    bs_ = [A @ np.random.default_rng(100 + k).normal(size=A.shape[0]) for k, A in enumerate(A1)]
    return sets, facs, bs_, bs


def _needs_L(kind):
    return kind in ("ext_spai", "ext_spai_scaled")


def _make(As, Ls, kind, dtype, bsz=1, eps=EPS):
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient

    return BatchedConjugateGradient([_typed(A, dtype) for A in As],
                                    [_typed(L, dtype) for L in Ls] if _needs_L(kind) else None, eps, dtype=dtype,
                                    block_size=bsz, preconditioner=kind)


def _update(B, As, Ls, kind, dtype, **kw):
    t, kept = B.update(None if As is None else [None if A is None else _typed(A, dtype) for A in As],
                       [None if L is None else _typed(L, dtype) for L in Ls] if Ls is not None and _needs_L(kind)
                       else None, **kw)
    assert t >= 0.0
    return kept


def _run(B, bs_, dtype, coef=False, max_iter=0):
    """Per system (iters, converged, history, x[, rho, pi])."""
    bt = [torch.from_numpy(np.asarray(b).astype(dtype)).cuda() for b in bs_]
    xs = [torch.zeros_like(b) for b in bt]
    res, t = B.solve(bt, xs, rtol=1e-8 if dtype == np.float64 else 1e-5, return_history=True, return_coefficients=coef,
                     max_iter=max_iter)
    assert t > 0
    out = []
    for r, x in zip(res, xs):
        out.append((r[0], r[1], np.asarray(r[2]), x.cpu().numpy()) + (tuple(r[3]) if coef else ()))
    return out


def _same(a, b):
    return len(a) == len(b) and all(
        ra[0] == rb[0] and ra[1] == rb[1] and all(np.array_equal(u, v) for u, v in zip(ra[2:], rb[2:]))
        for ra, rb in zip(a, b))


def _kept_expected(prev, new, dtype):
    """§14's rule on the window: the block-diagonal values are fp32-exact when every system's are."""
    exact = lambda As: all(_is_f32_exact(A) for A in As)  # noqa: E731
    return True if dtype == np.float32 else exact(prev) == exact(new)


_FRESH = {}  # (window, kind, dtype, mode, matrix set, coef) -> a fresh batch's results, computed once


def _max_iter(name):
    """The elasticity window is no M-matrix window and its seeded factor no good preconditioner: as in
    tests/test_gpu_batch_kinds.py::test_kind_bsr3 its solves are compared over 60 iterations, converged or not."""
    return 60 if name == "bsr3" else 0


def _fresh(name, kind, dtype, mode, k, coef=False):
    key = (name, kind, np.dtype(dtype).name, mode, k, coef)
    if key not in _FRESH:
        sets, facs, bs_, bsz = _window(name)
        res = _run(_make(sets[k], facs[k], kind, dtype, bsz), bs_, dtype, coef, _max_iter(name))
        for j, r in enumerate(res):
            print(f"fresh {key} system {j}: {r[0]} iterations, converged {r[1]}")
            assert (r[1] or name == "bsr3") and r[0] > 1, (key, j, r[0], r[1])
        _FRESH[key] = res
    return _FRESH[key]


def _set_mode(monkeypatch, mode):
    for k in ("LSPCG_BATCH_SMALL", "LSPCG_BATCH_REDUCE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def _updated_equals_fresh(monkeypatch, name, kind, dtype, mode, coef=False):
    """A1 -> A2 (solved twice: the first solve after an update, then a repeat) -> A1 -> A3 -> A2 on
    every system; after each step the batch equals a fresh one on the same matrices."""
    _set_mode(monkeypatch, mode)
    sets, facs, bs_, bsz = _window(name)
    fresh = lambda k: _fresh(name, kind, dtype, mode, k, coef)  # noqa: E731
    B = _make(sets[0], facs[0], kind, dtype, bsz)
    mi = _max_iter(name)
    assert _same(_run(B, bs_, dtype, coef, mi), fresh(0))
    assert not _same(fresh(0), fresh(1))  # another window (A3 is A1 itself once both are stored in fp32)
    prev = 0
    for step, k in enumerate((1, 0, 2, 1)):
        kept = _update(B, sets[k], facs[k], kind, dtype)
        print(f"{name} {kind} {np.dtype(dtype).name} {mode}: set {prev} -> {k}, graphs_kept {kept}")
        assert kept == _kept_expected(sets[prev], sets[k], dtype), (prev, k)
        assert _same(_run(B, bs_, dtype, coef, mi), fresh(k)), (prev, k)
        if step == 0:
            assert _same(_run(B, bs_, dtype, coef, mi), fresh(k))
        prev = k
    return B


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["none", "diagonal", "ext_spai", "ext_spai_scaled", "ainv"])
def test_updated_batch_equals_fresh_batch(gpu_ctx, monkeypatch, kind, dtype, mode):
    assert max(A.shape[0] for A in _window("small")[0][0]) <= 2560
    B = _updated_equals_fresh(monkeypatch, "small", kind, dtype, mode)
    assert [M.n for M in B.A] == [480, 63, 729, B.A[3].n]


@pytest.mark.parametrize("kind", ["ext_spai", "diagonal"])
def test_updated_lockstep_batch_of_larger_systems_equals_fresh_batch(gpu_ctx, monkeypatch, kind):
    """Systems above the one-workgroup bound (lockstep by size, the default reductions), with every
    system's recorded (rho_k, pi_k) pairs among what is compared."""
    assert min(A.shape[0] for A in _window("large")[0][0]) > 2560
    _updated_equals_fresh(monkeypatch, "large", kind, np.float64, "one_workgroup", coef=True)


@pytest.mark.parametrize("reduce", ["0", "1"])
@pytest.mark.parametrize("kind", ["none", "diagonal", "ext_spai", "ext_spai_scaled"])
def test_updated_bsr3_batch_equals_fresh_batch(gpu_ctx, monkeypatch, kind, reduce):
    B = _updated_equals_fresh(monkeypatch, "bsr3", kind, np.float64, "consumer_sums" if reduce == "1" else "tickets")
    assert all(M.block_size == 3 for M in B.A)


# ---- partial updates -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one_workgroup", "consumer_sums"])
@pytest.mark.parametrize("kind", ["ext_spai", "ext_spai_scaled"])
def test_partial_updates_equal_fresh_batches(gpu_ctx, monkeypatch, kind, mode):
    _set_mode(monkeypatch, mode)
    sets, facs, bs_, _ = _window("small")
    dt = np.float64
    B = _make(sets[0], facs[0], kind, dt)
    r1 = _run(B, bs_, dt)
    # only system 1 of 4 gets a new A and L
    As = [sets[0][0], sets[1][1], sets[0][2], sets[0][3]]
    Ls = [facs[0][0], facs[1][1], facs[0][2], facs[0][3]]
    _update(B, [None, As[1], None, None], [None, Ls[1], None, None], kind, dt)
    got = _run(B, bs_, dt)
    assert _same(got, _run(_make(As, Ls, kind, dt), bs_, dt))
    assert _same(got[:1] + got[2:], r1[:1] + r1[2:]) and not _same(got[1:2], r1[1:2])
    assert B.A[0].n == 480 and B.A[1].to_scipy().data[0] == As[1].data[0]
    # every L, no A
    _update(B, None, facs[2], kind, dt)
    got = _run(B, bs_, dt)
    assert _same(got, _run(_make(As, facs[2], kind, dt), bs_, dt))
    # epsilon alone: the operator changes, so the histories do
    kept = _update(B, None, None, kind, dt, epsilon=2e-3)
    assert kept is False and B.epsilon == 2e-3
    got2 = _run(B, bs_, dt)
    assert _same(got2, _run(_make(As, facs[2], kind, dt, eps=2e-3), bs_, dt))
    assert all(not np.array_equal(a[2], b[2]) for a, b in zip(got, got2))


# ---- refusals --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one_workgroup", "tickets"])
def test_a_refused_update_leaves_the_batch_as_it_was(gpu_ctx, monkeypatch, mode):
    """System 2 of 4 comes with one column index moved (the same counts, so only the device check
    can see it), in A and separately in L: LSPCG_ERR_FORMAT, and the next solve repeats the solve
    before the call in all four systems -- systems 0 and 1 and every L were not written."""
    from learningsparsepreconditioner4gpu_amd import _lib

    _set_mode(monkeypatch, mode)
    sets, facs, bs_, _ = _window("small")
    dt = np.float64
    B = _make(sets[0], facs[0], "ext_spai", dt)
    before = _run(B, bs_, dt)
    handles = (list(B.A), list(B.L))

    def refused(As, Ls):
        with pytest.raises(_lib.LspcgError) as e:
            _update(B, As, Ls, "ext_spai", dt)
        assert e.value.code == _lib.ERR_FORMAT
        assert (list(B.A), list(B.L)) == handles
        assert _same(_run(B, bs_, dt), before)

    moved = lambda Ms: Ms[:2] + [_one_entry_moved(Ms[2])] + Ms[3:]  # noqa: E731
    refused(moved(sets[1]), facs[1])
    refused(sets[1], moved(facs[1]))
    refused(None, moved(facs[1]))
    refused(sets[1][:2] + [_one_entry_more(sets[1][2])] + sets[1][3:], facs[1])  # (found on the host)
    # a good update still works, on kept graphs
    assert _kept_expected(sets[0], sets[1], dt) is True
    assert _update(B, sets[1], facs[1], "ext_spai", dt) is True
    assert _same(_run(B, bs_, dt), _fresh("small", "ext_spai", dt, mode, 1))


def test_an_ainv_breakdown_in_an_update_leaves_the_batch_as_it_was(gpu_ctx, monkeypatch):
    from learningsparsepreconditioner4gpu_amd import _lib

    _set_mode(monkeypatch, "one_workgroup")
    sets, facs, bs_, _ = _window("small")
    dt = np.float64
    B = _make(sets[0], None, "ainv", dt)
    before = _run(B, bs_, dt)
    handles, setup = (list(B.A), list(B.L)), B.setup_time
    bad = sets[1][:2] + [_weak_diagonal(sets[0][2], 0.01)] + sets[1][3:]
    with pytest.raises(_lib.LspcgError) as e:
        _update(B, bad, None, "ainv", dt)
    assert e.value.code == _lib.ERR_BREAKDOWN
    assert (list(B.A), list(B.L)) == handles and B.setup_time == setup
    assert _same(_run(B, bs_, dt), before)
    _update(B, sets[1], None, "ainv", dt)
    assert B.setup_time > 0
    assert _same(_run(B, bs_, dt), _fresh("small", "ainv", dt, "one_workgroup", 1))


# ---- not only against the same code ------------------------------------------------------------
def test_updated_batch_matches_the_oracle(gpu_ctx, monkeypatch):
    """An updated ext_spai window against the oracle's exact-dot trajectory of A2 / L2: the count
    equal and x to 1e-12, the tolerances tests/test_gpu_batch.py holds a fresh batch to."""
    _set_mode(monkeypatch, "consumer_sums")
    sets, facs, bs_, _ = _window("small")
    B = _make(sets[0], facs[0], "ext_spai", np.float64)
    _run(B, bs_, np.float64)
    _update(B, sets[1], facs[1], "ext_spai", np.float64)
    for A, L, b, (it, conv, h, x) in zip(sets[1], facs[1], bs_, _run(B, bs_, np.float64)):
        it_o, x_o, h_o = O.pcg(A, b, O.spai_operator(sp.csr_matrix(L), EPS), rtol=1e-8, dot="exact")
        assert conv and it == it_o
        np.testing.assert_allclose(h, h_o, rtol=1e-12, atol=0)
        assert np.linalg.norm(x - x_o) <= 1e-12 * np.linalg.norm(x_o)


# ---- callers -----------------------------------------------------------------------------------
def _count_batches(monkeypatch):
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient

    made = []
    orig = BatchedConjugateGradient.__init__

    def init(self, *a, **kw):
        made.append(kw.get("preconditioner"))
        return orig(self, *a, **kw)

    monkeypatch.setattr(BatchedConjugateGradient, "__init__", init)
    return made


def test_validate_reuses_a_batch_across_windows_of_equal_patterns(gpu_ctx, monkeypatch):
    from learningsparsepreconditioner4gpu_amd.validate import get_pcg_iter_time_batch

    _set_mode(monkeypatch, "consumer_sums")
    sets, facs, bs_, _ = _window("small")
    # the same sizes and entry counts as window 1, another pattern in system 0: the kept batch refuses it
    perm = np.arange(480).reshape(24, 20).T.ravel()  # the grid numbered along its other axis
    other = _csr(sets[0][0][perm][:, perm])
    assert other.shape == sets[0][0].shape and other.nnz == sets[0][0].nnz
    assert not np.array_equal(other.indices, sets[0][0].indices)
    windows = [(sets[0], facs[0]), (sets[1], facs[1]),
               ([other] + sets[0][1:], [_cases.spai_like(other, seed=3)] + facs[0][1:])]
    gts = [b.copy() for b in bs_]

    def go(reuse):
        out = []
        for As, Ls in windows:
            infos = [{} for _ in As]
            kw = {} if reuse is None else {"reuse": reuse}
            res = get_pcg_iter_time_batch(As, gts, Ls, EPS, rtol=1e-8, infos=infos, **kw)
            out.append(([r[0] for r in res], [i["x"].cpu().numpy() for i in infos], [i["converged"] for i in infos]))
        return out

    ref = go(None)
    made = _count_batches(monkeypatch)
    kept = {}
    got = go(kept)
    assert len(made) == 2, made  # windows 1 and 2 share one batch, window 3 gets its own
    assert len(kept) == 1  # ... which replaced the kept one
    for (it, xs, conv), (it_r, xs_r, conv_r) in zip(got, ref):
        assert it == it_r and conv == conv_r and all(conv) and min(it) > 1
        assert all(np.array_equal(x, y) for x, y in zip(xs, xs_r))
    assert ref[0][0] != ref[1][0] or not np.array_equal(ref[0][1][0], ref[1][1][0])


@pytest.mark.parametrize("scaled", [False, True])
def test_infer_run_with_a_reused_batch_equals_the_default_path(gpu_ctx, monkeypatch, tmp_path, scaled):
    from learningsparsepreconditioner4gpu_amd import infer
    from learningsparsepreconditioner4gpu_amd.dataset import FolderWriter
    from learningsparsepreconditioner4gpu_amd.workspace import ScaledInferenceWorkspace, SimpleInferenceWorkspace

    A, mask, feats = P.heat_tet(7, 6, 5)
    A = _csr(A)
    w = FolderWriter(str(tmp_path / "fixed"), block_size=1, is_fixed_topology=True, save_rhs=1, seed=5)
    w.write_topology(A)
    for k in range(8):
        w.append(A if k == 0 else _scaled(A, seed=10 + k), mask, np.asarray(feats, dtype=np.float64))
    samples = infer.folder_dataset(str(tmp_path / "fixed"), block_size=1, fixed_topology=True)
    assert len(samples) == 8
    cls = ScaledInferenceWorkspace if scaled else SimpleInferenceWorkspace
    ws = cls(node_features=samples[0].x.shape[1], edge_features=samples[0].edge_attr.shape[1], seed=0)
    x_ref, x_got = {}, {}
    ref = infer.run(samples, ws, rtol=1e-8, warmup=1, batch=4, solutions=x_ref)
    made = _count_batches(monkeypatch)
    got = infer.run(samples, ws, rtol=1e-8, warmup=1, batch=4, reuse_batch=True, solutions=x_got)
    assert len(made) == 1, made  # two windows, one batch
    assert [r.index for r in got] == [r.index for r in ref] == list(range(8))
    assert [r.iters for r in got] == [r.iters for r in ref]
    assert [r.converged for r in got] == [r.converged for r in ref] and all(r.iters > 1 for r in got)
    assert [r.rel_res for r in got] == [r.rel_res for r in ref]
    assert not torch.equal(x_ref[0], x_ref[4])  # the windows hold different systems
    for i in range(8):
        assert torch.equal(x_got[i], x_ref[i]), i
    with pytest.raises(ValueError):
        infer.run(samples, ws, reuse_batch=True)
