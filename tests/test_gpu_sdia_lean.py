"""The SELL-DIA kernels' scalar addressing (csrc/lspcg_sell.hpp, kSdiaMax): vector windows loaded
unconditionally through range-checked loads, values at compile-time slot offsets behind one per-lane
base (surplus slots read on, into the array's zeroed tail), lane masks instead of row masks.

Everything here is bit for bit: against scipy's ``A @ x`` or against the same solve on the CSR views
(LSPCG_NO_SELL=1).  The cases are the ones where the new addressing could go wrong: windows that start
before row 0 or end past row n, masked slots over inf / nan / -0.0, a last slice whose surplus slots
run past the value array, graphs replayed after the values or the dot order changed, and offsets
nearly as large as the vector."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import _cases
from tests.test_gpu_sell import _dia_slots, _dm, _expected_kind, _offset_matrix, _sell_spmv, _v

pytestmark = pytest.mark.gpu

OFFS15 = [-4097, -4096, -65, -64, -63, -2, -1, 0, 1, 2, 63, 64, 65, 4096, 4097]
# (n, offsets): windows off both ends of the vector in nearly every slice; n no multiple of 64 or 256
WINDOWS = {"n4099": (4099, OFFS15), "n1500": (1500, [-1200, -1, 0, 1, 1200]), "n37": (37, [-30, -1, 0, 1, 30]),
           "n64": (64, [-30, -1, 0, 1, 30]), "n65": (65, [-30, -1, 0, 1, 30])}


@pytest.fixture(autouse=True)
def _given_numbering(monkeypatch):
    monkeypatch.setenv("LSPCG_REORDER", "0")


def _spd(A, exact32=True):
    """A symmetric, strictly diagonally dominant matrix on the (symmetric) pattern of A; values exact
    in fp32 (the solver then stores them as fp32) or not (fp64 values)."""
    S = sp.csr_matrix(A + A.T) * 0.5
    S.setdiag(0.0)
    S = sp.csr_matrix(S)
    S.setdiag(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)
    S = sp.csr_matrix(S)
    S.sort_indices()
    S.data = S.data.astype(np.float32).astype(np.float64)
    if not exact32:
        S.data = S.data * (1.0 + 2.0 ** -40)
    return S


def _solve(A, env, monkeypatch, L=None, eps=1e-3, max_iter=80):
    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = PreconditionedConjugateGradient(A, device="cuda", preconditioner="ext_spai")
    s.set_spai(_cases.spai_like(A) if L is None else L, eps)
    return s, _run(s, A, max_iter)


def _run(s, A, max_iter=80):
    n = A.shape[0]
    b = torch.from_numpy(A @ np.ones(n)).cuda()
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    it, conv, _, hist = s.solve(b, x, rtol=1e-9, max_iter=max_iter, return_history=True)
    return it, x.cpu().numpy(), hist


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _spmv_all(A, x, flags=(8, 9, 10, 11)):
    """fp64 SpMV (prepare_spmv + matvec) and the loop's kernels (flags 8-11: SELL-DIA under any
    padding, fp32 values, 16-bit hint)."""
    ref = A @ x
    assert np.all(np.isfinite(ref))
    Ad = _dm(A)
    assert Ad.prepare_spmv() == _expected_kind(A)
    xt = torch.from_numpy(x).cuda()
    assert np.array_equal(Ad.matvec(xt).cpu().numpy(), ref)
    for f in flags:
        assert np.array_equal(_sell_spmv(Ad, xt, f), ref), f


@pytest.mark.parametrize("case", list(WINDOWS))
def test_windows_off_both_ends_spmv(gpu_ctx, case):
    """(n = 37 and 65 store more than twice their entries as SELL-64 slots, so the analysis step's padding
    limit keeps every SELL view off prepare_spmv and the solver there; the SELL-DIA kernels run on them
    through flags 8-11, which build the view under any padding.)"""
    n, offs = WINDOWS[case]
    A = _offset_matrix(n, offs, 7)
    assert _dia_slots(A)[0] <= 16 and _expected_kind(A) == (17 if n in (37, 65) else 1)
    x = np.random.default_rng(11).normal(size=n)
    x[::13] = -0.0
    _spmv_all(A, x)


@pytest.mark.parametrize("case", list(WINDOWS))
def test_windows_off_both_ends_solve(gpu_ctx, case, monkeypatch):
    n, offs = WINDOWS[case]
    A = _spd(_offset_matrix(n, offs, 7))
    kind = _expected_kind(A)
    assert kind == (17 if n in (37, 65) else 1)
    _, ref = _solve(A, _v(no_sell="1", small="0"), monkeypatch)
    assert np.all(np.isfinite(ref[1]))
    for env in (_v(small="0"), _v(split="0", small="0"), _v(split="2", small="0")):
        s, out = _solve(A, env, monkeypatch)
        assert kind != 1 or all(v["columns"] == "sdia" for v in s.views.values()), s.views
        assert _same(ref, out), (case, env, ref[0], out[0])


def test_masked_slots_carry_nothing(gpu_ctx):
    """inf, nan and -0.0 in x exactly where only ABSENT slots read: none of them reaches a sum."""
    n, offs = 5003, [-40, -33, -17, -9, -3, -2, -1, 0, 1, 2, 3, 9, 17, 33, 40]
    A = _offset_matrix(n, offs, 3)
    rng = np.random.default_rng(4)
    keep = (rng.random(A.nnz) >= 0.3) & (A.indices % 97 != 5)  # ~30 % dropped, columns 5, 102, ... emptied
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    A = sp.csr_matrix((A.data[keep], (rows[keep], A.indices[keep])), shape=(n, n))
    A.sort_indices()
    assert _expected_kind(A) == 1
    # columns an absent slot reads: row i lacks offset o although its slice's dictionary has it
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    have = set(zip(rows.tolist(), (A.indices - rows).tolist()))
    absent = set()
    for s0 in range(0, n, 64):
        sl = slice(A.indptr[s0], A.indptr[min(s0 + 64, n)])
        dct = set((A.indices[sl] - rows[sl]).tolist())
        for i in range(s0, min(s0 + 64, n)):
            absent.update(i + o for o in dct if (i, o) not in have and 0 <= i + o < n)
    poison = np.array(sorted(absent - set(A.indices.tolist())))
    assert poison.size > 0
    x = rng.normal(size=n)
    x[poison] = np.resize([np.inf, np.nan, -0.0, -np.inf], poison.size)
    _spmv_all(A, x)


def _tail(slots, exact32=True):
    """n = 200 (4 slices): the last slice (rows 192..199) has 9 slots, or only its diagonal."""
    A = _offset_matrix(200, list(range(-4, 5)), 5).tolil()
    if slots == 1:
        for i in range(192, 200):
            for j in range(max(0, i - 4), min(200, i + 5)):
                if i != j:
                    A[i, j] = 0.0
                    A[j, i] = 0.0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    sl = slice(A.indptr[192], A.indptr[200])
    assert len(set((A.indices[sl] - np.repeat(np.arange(192, 200), np.diff(A.indptr[192:]))).tolist())) == slots
    return A


@pytest.mark.parametrize("slots", [9, 1])
def test_surplus_slots_at_the_end_spmv(gpu_ctx, slots):
    A = _tail(slots)
    x = np.random.default_rng(2).normal(size=200)
    _spmv_all(A, x, flags=(8, 9))  # fp64 and fp32 values


@pytest.mark.parametrize("exact32", [True, False])
@pytest.mark.parametrize("slots", [9, 1])
def test_surplus_slots_at_the_end_solve(gpu_ctx, slots, exact32, monkeypatch):
    A = _spd(_tail(slots), exact32)
    L = _cases.spai_like(A)
    if exact32:
        L.data = L.data.astype(np.float32).astype(np.float64)
    _, ref = _solve(A, _v(no_sell="1", small="0"), monkeypatch, L=L)
    s, out = _solve(A, _v(small="0"), monkeypatch, L=L)
    assert {v["columns"] for v in s.views.values()} == {"sdia"}
    assert {v["value_bytes"] for v in s.views.values()} == {4 if exact32 else 8}, s.views
    assert np.all(np.isfinite(ref[1])) and _same(ref, out)


def test_stale_graphs(gpu_ctx, monkeypatch):
    """A solver whose factor is replaced in place (other values, another epsilon) or whose dot order is
    switched and switched back gives what a fresh solver gives: no replay of a graph that holds an
    old pattern, value base or vector size."""
    n, offs = WINDOWS["n1500"]
    A = _spd(_offset_matrix(n, offs, 7))
    L1, L2 = _cases.spai_like(A, seed=0), _cases.spai_like(A, seed=1)
    env = _v(small="0")
    s, first = _solve(A, env, monkeypatch, L=L1)
    assert _same(first, _solve(A, env, monkeypatch, L=L1)[1])
    s.set_spai(L2, 1e-3)
    assert _same(_run(s, A), _solve(A, env, monkeypatch, L=L2)[1])
    s.set_spai(L2, 5e-2)
    assert _same(_run(s, A), _solve(A, env, monkeypatch, L=L2, eps=5e-2)[1])
    s.set_dot_order("openblas")
    f, _ = _solve(A, env, monkeypatch, L=L2, eps=5e-2)
    f.set_dot_order("openblas")
    assert _same(_run(s, A), _run(f, A))
    s.set_dot_order("compensated")
    assert _same(_run(s, A), _solve(A, env, monkeypatch, L=L2, eps=5e-2)[1])


def test_large_halo(gpu_ctx, monkeypatch):
    """Offsets nearly as large as the vector: whichever addressing the launch takes, scipy's bits, and
    the solver still runs on SELL-DIA views."""
    n = 150000
    A = _offset_matrix(n, [-120000, -1, 0, 1, 120000], 2)
    x = np.random.default_rng(8).normal(size=n)
    _spmv_all(A, x)
    S = _spd(A)
    _, ref = _solve(S, _v(no_sell="1", small="0"), monkeypatch, max_iter=30)
    s, out = _solve(S, _v(small="0"), monkeypatch, max_iter=30)
    assert all(v["columns"] == "sdia" for v in s.views.values()), s.views
    assert _same(ref, out)
