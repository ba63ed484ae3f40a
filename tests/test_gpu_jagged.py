"""GPU: the jagged layouts SELL-64J (view kind 17) and SELL-64X (kind 18, csrc/lspcg_sell.hpp
k_spmv_sellj) at their layout edges, on the matrices of tests/_jagged_cases.py (whose properties
tests/test_jagged_cases_host.py proves on the CPU).  LSPCG_SELLX_MIN_N=0 ("floor lowered") lets the
x-staged layout exist below its production floor of 2^18 rows.  Checked here:
  * the standalone SpMV's kind equals the rule mirror's and its bits equal scipy's csr_matvec on every
    case (fp64 / fp32, default and lowered floor, stored-order rows, -0.0 and inf in x), also through
    lspcg_spmv_sell_timed's flag bits 4 (SELL-64J) and 5 (SELL-64X);
  * the tile walk: the loop's reducing launches cap the grid at min(6 x CUs, 4096) workgroups, so only a
    system of more than 256 x cap rows sends a workgroup to a second tile (metadata reload, restart of the
    count register, LDS reuse behind a barrier) -- one such solve per layout against the CSR views;
  * solves on hub_spd (rows of 61..64 entries) for every preconditioner kind, fp64 and fp32 solvers,
    fp32-exact and full fp64 values, against the CSR views and the oracle's correctly-rounded-dot run;
  * the lockstep batch on jagged views against single solves and the oracle.
The solves also record whether the jagged runs equal the CSR runs bit for bit (printed tallies)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import linalg as O
from tests import _cases
from tests import _jagged_cases as J
from tests.test_gpu_sell import _expected_kind

pytestmark = pytest.mark.gpu

EPS = 3e-3
FLOORS = (("default", None, 262144), ("lowered", "0", 0))  # (name, LSPCG_SELLX_MIN_N, the mirror's xs_min_n)


@pytest.fixture(autouse=True)
def _given_numbering(monkeypatch):
    monkeypatch.setenv("LSPCG_REORDER", "0")
    monkeypatch.delenv("LSPCG_SELLX_MIN_N", raising=False)
    monkeypatch.delenv("LSPCG_NO_SELL", raising=False)


def _set_floor(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("LSPCG_SELLX_MIN_N", raising=False)
    else:
        monkeypatch.setenv("LSPCG_SELLX_MIN_N", value)


SPMV_CASES = {
    "sweep1500": lambda: J.sweep(1500),
    "sweep2200": lambda: J.sweep(2200),
    "sweep1500-stored-order": lambda: J.stored_order(J.sweep(1500)),
    "limit256": lambda: J.limit(256),
    "limit257": lambda: J.limit(257),
    "row65": J.row65,
    **{f"n{n}": functools.partial(J.sizes, n) for n in J.SIZES},
    "holes-last": lambda: J.holes("last"),
    "holes-boundary": lambda: J.holes("boundary"),
    "off16-32767": lambda: J.off16(32767),
    "off16-32768": lambda: J.off16(32768),
    "hub": lambda: J.hub_spd(4500, True),
    "hub-fp64-values": lambda: J.hub_spd(4500, False),
}
# the kinds the cases are about (default floor, floor lowered); None: whatever the rule mirror says
NAMED_KINDS = {"sweep1500": (17, 18), "sweep2200": (17, 17), "sweep1500-stored-order": (17, 18), "limit256": (17, 18),
               "limit257": (17, 17), "holes-last": (17, 18), "holes-boundary": (17, 18), "off16-32767": (17, 18),
               "hub": (17, 18), "hub-fp64-values": (17, 18), **{f"n{n}": (17, 18) for n in J.SIZES}}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's matrix, built once and never written to."""
    return SPMV_CASES[name]()


def _typed(A, dtype):
    # (scipy's astype sorts a row's entries: the copy is built from the stored arrays instead)
    return sp.csr_matrix((A.data.astype(dtype), A.indices, A.indptr), shape=A.shape)


def _x(n, dtype, seed=1):
    x = np.random.default_rng(seed).normal(size=n).astype(dtype)
    x[::17] = dtype(-0.0)
    x[-3:] = dtype(7.5)  # a tail block's entries
    return x


def _same_with_nonfinite(y, ref):
    return (np.array_equal(np.isnan(y), np.isnan(ref)) and np.array_equal(y[~np.isnan(y)], ref[~np.isnan(ref)])
            and np.array_equal(np.signbit(y[~np.isnan(y)]), np.signbit(ref[~np.isnan(ref)])))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(SPMV_CASES))
def test_jagged_spmv_kind_and_bits(gpu_ctx, monkeypatch, name, dtype):
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    A = _case(name)
    keep = name.endswith("stored-order")
    As = _typed(A, dtype)
    x = _x(A.shape[0], dtype)
    ref = As @ x  # (stored-order rows: scipy sums in that order, as the device does)
    xt = torch.as_tensor(x, device="cuda")
    for k, (floor, env, xs_min_n) in enumerate(FLOORS):
        _set_floor(monkeypatch, env)
        D = DeviceMatrix.from_scipy(As, dtype=dtype, keep_order=keep)
        kind = D.prepare_spmv()
        want = _expected_kind(A, dia=not keep, xs_min_n=xs_min_n)
        assert kind == want, (name, floor, kind, want)
        if name in NAMED_KINDS:
            assert kind == NAMED_KINDS[name][k], (name, floor, kind)
        else:
            assert kind not in (17, 18), (name, floor, kind)
        y = D.matvec(xt).cpu().numpy()
        assert np.array_equal(y, ref) and np.array_equal(np.signbit(y), np.signbit(ref)), (name, floor, kind)
        del D


def _sell_spmv(Ad, x, flags):
    from learningsparsepreconditioner4gpu_amd import _lib

    y = torch.full_like(x, float("nan"))
    ms = C.c_double()
    _lib.call("lspcg_spmv_sell_timed", Ad.ctx.handle, Ad.handle, int(flags), C.c_void_p(x.data_ptr()),
              C.c_void_p(y.data_ptr()), 1, 0, C.byref(ms))
    return y.cpu().numpy()


@pytest.mark.parametrize("name", list(SPMV_CASES))
def test_jagged_spmv_through_the_timed_entry(gpu_ctx, monkeypatch, name):
    """lspcg_spmv_sell_timed with flag bits 4 (SELL-64J) and 5 (SELL-64X, floor lowered) on top of bit
    1 (16-bit offsets), fp64 values (18, 50) and fp32 values (19, 51: on the fp32-exact copy)."""
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    A = _case(name)
    keep = name.endswith("stored-order")
    x = _x(A.shape[0], np.float64, seed=5)
    xt = torch.as_tensor(x, device="cuda")
    for M, flag_set in ((A, (18, 50)), (J.f32_exact(A), (19, 51))):
        ref = M @ x
        Ad = DeviceMatrix.from_scipy(M, keep_order=keep)
        for flags in flag_set:
            _set_floor(monkeypatch, "0" if flags & 32 else None)
            y = _sell_spmv(Ad, xt, flags)
            assert np.array_equal(y, ref) and np.array_equal(np.signbit(y), np.signbit(ref)), (name, flags)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("floor", ["default", "lowered"])
def test_jagged_spmv_skips_padding_with_inf(gpu_ctx, monkeypatch, floor, dtype):
    """sweep(1500) under kinds 17 and 18 with inf in x: at one column that the 64-entry row reads (that
    column's readers become +-inf, no other row changes), then at the entries a lane without an entry may gather instead (every
    slice's first row as a column, every tile's first staged entry): a padded lane that added 0 * inf
    would turn a finite row into NaN.  The NaN pattern and every other value equal scipy's."""
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    A = _case("sweep1500")
    n = A.shape[0]
    _set_floor(monkeypatch, dict((f[0], f[1]) for f in FLOORS)[floor])
    As = _typed(A, dtype)
    D = DeviceMatrix.from_scipy(As, dtype=dtype)
    assert D.prepare_spmv() == (17 if floor == "default" else 18)
    lens = np.diff(A.indptr)
    rows = np.repeat(np.arange(n), lens)
    # (every column of this matrix has a dozen readers or more: the 64-entry row's least-read column)
    long_row = int(np.flatnonzero(lens == 64)[0])
    own = A.indices[A.indptr[long_row]:A.indptr[long_row + 1]]
    c = int(own[np.argmin(np.bincount(A.indices, minlength=n)[own])])
    hit = np.unique(rows[A.indices == c])
    x1 = _x(n, dtype, seed=9)
    x1[c] = np.inf
    x2 = _x(n, dtype, seed=10)
    x2[::64] = np.inf  # the row a masked SELL-64J lane gathers: its slice's first
    first = np.minimum.reduceat(A.indices, A.indptr[:-1][lens > 0])  # the first column of each non-empty row
    tile_first = np.full((n + 255) // 256, n, dtype=np.int64)
    np.minimum.at(tile_first, np.flatnonzero(lens > 0) // 256, first)
    x2[(tile_first // 16) * 16] = -np.inf  # LDS entry 0 of each tile's staged blocks
    for k, x in enumerate((x1, x2)):
        with np.errstate(invalid="ignore"):
            ref = As @ x
        y = D.matvec(torch.as_tensor(x, device="cuda")).cpu().numpy()
        if k == 0:
            assert long_row in hit and np.array_equal(np.flatnonzero(~np.isfinite(ref)), hit) and np.all(np.isinf(ref[hit]))
        else:
            assert 0 < np.count_nonzero(np.isfinite(ref)) < n  # rows that read no inf stay finite
        assert _same_with_nonfinite(y, ref), (floor, k)


# ---- solves -------------------------------------------------------------------------------------
VIEWS = (("sell16j", {"LSPCG_SELLX_MIN_N": str(1 << 40)}), ("sell16x", {"LSPCG_SELLX_MIN_N": "0"}),
         ("csr", {"LSPCG_NO_SELL": "1"}))
MAX_ITER = 1000  # every system here converges within 50 iterations: a wrong kernel ends its solve quickly
_TALLY = {}


def _tally(group, same):
    """Counts, per group of tests, the fp64 jagged runs whose x and history equal the CSR run's bits."""
    t = _TALLY.setdefault(group, [0, 0])
    t[0] += int(same)
    t[1] += 1
    print(f"[{group}] jagged solves bit-identical to the CSR views' (x and history): {t[0]}/{t[1]} so far")


def _solver(A, L, pre, dtype):
    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient

    s = PreconditionedConjugateGradient(A, device="cuda", preconditioner=pre, dtype=dtype)
    if pre.startswith("ext_spai"):
        s.set_spai(L, EPS)
    return s


def _run(s, b, rtol, dtype):
    bt = torch.as_tensor(b, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    x = torch.zeros_like(bt)
    it, conv, _t, h = s.solve(bt, x, rtol=rtol, return_history=True, max_iter=MAX_ITER)
    return it, conv, x.cpu().numpy().astype(np.float64), np.asarray(h)


def _runs_on_every_view(monkeypatch, A, L, b, pre, dtype, rtol, value_bytes=None, views=VIEWS):
    runs = {}
    for name, env in views:
        for k in ("LSPCG_SELLX_MIN_N", "LSPCG_NO_SELL"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = _solver(A, L, pre, dtype)
        v = s.views
        assert v["A"]["columns"] == name, (name, v)
        if pre.startswith("ext_spai"):
            assert v["L"]["columns"] == name and v["LT"]["columns"] == name, (name, v)
        if value_bytes is not None and name != "csr":
            assert v["A"]["value_bytes"] == value_bytes, (name, v)
        runs[name] = _run(s, b, rtol, dtype)
        del s
    return runs


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _oracle_operator(A, L, pre, eps=EPS):
    return {"none": lambda: None, "diagonal": lambda: O.diagonal_operator(A), "ext_spai": lambda: O.spai_operator(L, eps),
            "ext_spai_scaled": lambda: O.spai_scaled_operator(A, L, eps)}[pre]()


@functools.lru_cache(maxsize=None)
def _hub(n, exact32):
    A = J.hub_spd(n, exact32)
    L = _cases.spai_like(A, seed=4)
    b = A @ np.random.default_rng(3).uniform(0, 1, n)
    return A, L, b


def _hub_solve(monkeypatch, pre, dtype, exact32):
    A, L, b = _hub(4500, exact32)
    assert A.shape[0] > 3072  # above the one-workgroup solve: the loop's kernels run
    f64 = dtype == np.float64
    rtol, tol = (1e-8, 1e-12) if f64 else (1e-5, 1e-5)
    if not f64:
        A, L = _typed(A, np.float32), _typed(L, np.float32)
        b = b.astype(np.float32)
    runs = _runs_on_every_view(monkeypatch, A, L, b, pre, dtype, rtol,
                               value_bytes=(4 if exact32 else 8) if f64 else None)
    it2, conv2, x2, h2 = runs["csr"]
    M = _oracle_operator(A, L, pre, EPS if f64 else np.float32(EPS))
    it_o, x_o, h_o = O.pcg(A, b, M, rtol=rtol, dot="exact", dtype=dtype)
    x_o, h_o = np.asarray(x_o, dtype=np.float64), np.asarray(h_o)
    for name in ("sell16j", "sell16x"):
        it, conv, x, h = runs[name]
        m = min(len(h), len(h2))
        print(f"{name} {pre} {np.dtype(dtype).name}: {it} iterations (csr {it2}, oracle {it_o}), x vs csr {_rel(x, x2):.2e}, "
              f"vs oracle {_rel(x, x_o):.2e}, history vs csr {np.max(np.abs(h[:m] - h2[:m]) / h2[:m]):.2e}")
        if f64:
            _tally("hub", np.array_equal(x, x2) and np.array_equal(h, h2))
        assert conv and conv2 and it == it2 == it_o, (name, it, it2, it_o)
        if f64:  # (every fp64 run measured bit-identical: the views change no bit of the default dot mode)
            assert np.array_equal(x, x2) and np.array_equal(h, h2), name
        assert _rel(x, x2) <= tol and _rel(x, x_o) <= tol, name
        np.testing.assert_allclose(h, h2, rtol=tol, atol=0)
        np.testing.assert_allclose(h, h_o[:len(h)], rtol=tol, atol=0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("pre", ["none", "diagonal", "ext_spai", "ext_spai_scaled"])
def test_hub_solve_equals_csr_and_oracle(gpu_ctx, monkeypatch, pre, dtype):
    """hub_spd (n = 4500, hub rows of 61..64 entries, fp32-exact values): SELL-64J, SELL-64X (floor
    lowered) and CSR views give the same count, which is the oracle's correctly-rounded-dot count; x
    and the history agree with both to 1e-12 (fp64 solver; with the CSR views' bit for bit) / 1e-5
    (fp32 solver)."""
    _hub_solve(monkeypatch, pre, dtype, True)


@pytest.mark.parametrize("pre", ["none", "ext_spai"])
def test_hub_solve_with_full_fp64_values(gpu_ctx, monkeypatch, pre):
    """The same with values fp32 cannot hold: the views store 8-byte values, so the loop's jagged
    kernels run with fp64 values (one workgroup per CU register budget)."""
    _hub_solve(monkeypatch, pre, np.float64, False)


# ---- the tile walk --------------------------------------------------------------------------------
# the oracle's correctly-rounded-dot counts (oracle.linalg.pcg, dot="exact", rtol 1e-10) of the system
# of a 256-CU device (cap 1536, n = 394,021), computed on the CPU: 12.7 s and 7.4 s, too long for here
WALK_ORACLE_COUNTS = {394021: {"none": 47, "ext_spai": 25}}
_WALK = {}


def _walk_system():
    if not _WALK:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        cap = min(6 * cus, 4096)
        n = 256 * (cap + 3) + 37
        A = J.banded_spd(n, 1500, seed=2)
        L = _cases.spai_like(A, seed=5)
        b = A @ np.random.default_rng(3).uniform(0, 1, n)
        _WALK["v"] = (cap, A, L, b)
    return _WALK["v"]


@pytest.mark.parametrize("pre", ["none", "ext_spai"])
def test_tile_walk_solve_equals_csr(gpu_ctx, monkeypatch, pre):
    """n = 256 (cap + 3) + 37 rows, cap = min(6 x CUs, 4096) the reducing launches' grid: four
    workgroups walk to a second tile (the last of them to the 37-row tail) and the others own one, the
    smallest shape that reaches the walk.  fp64 solver, A's values fp32-exact, L's not; SELL-64X (default
    floor: n > 2^18), SELL-64J (floor above n) and CSR views: the same count, x and history bit for
    bit, as in test_sell16x_solve_equals_csr_and_oracle.  The exact-dot oracle takes 7-13 s on this
    system, so it is not run here: the count is compared with the one it gave on the CPU
    (WALK_ORACLE_COUNTS) where the device has that system's size."""
    cap, A, L, b = _walk_system()
    n = A.shape[0]
    assert (n + 255) // 256 == cap + 4 and n > 262144
    runs = _runs_on_every_view(monkeypatch, A, L, b, pre, np.float64, 1e-10,
                               views=(("sell16x", {}),) + tuple(v for v in VIEWS if v[0] != "sell16x"))
    it2, conv2, x2, h2 = runs["csr"]
    for name in ("sell16x", "sell16j"):
        it, conv, x, h = runs[name]
        print(f"tile walk {name} {pre}: n {n}, {it} iterations (csr {it2}), x vs csr {_rel(x, x2):.2e}")
        _tally("tile walk", np.array_equal(x, x2) and np.array_equal(h, h2))
        assert conv and conv2 and it == it2, (name, it, it2)
        assert np.array_equal(x, x2) and np.array_equal(h, h2), name
    if n in WALK_ORACLE_COUNTS:
        assert it2 == WALK_ORACLE_COUNTS[n][pre], (it2, WALK_ORACLE_COUNTS[n][pre])
    tres = np.linalg.norm(b - A @ runs["sell16x"][2]) / np.linalg.norm(b)
    assert tres < 1e-9, tres


# ---- lockstep batch -------------------------------------------------------------------------------
BATCH_N = (4500, 4353, 4700)


@functools.lru_cache(maxsize=None)
def _batch_oracle():
    out = []
    for n in BATCH_N:
        A, L, b = _hub(n, True)
        out.append(O.pcg(A, b, O.spai_operator(L, EPS), rtol=1e-8, dot="exact"))
    return out


@pytest.mark.parametrize("name", ["sell16j", "sell16x"])
def test_batch_on_jagged_views_matches_single_and_oracle(gpu_ctx, monkeypatch, name):
    """Three hub_spd systems of different n (4353 = 17 x 256 + 1: 255 padding rows behind it) in one
    lockstep batch (one tile per workgroup: another grid shape of the jagged kernel) on SELL-64J and on
    SELL-64X views: per system the single solve's and the oracle's count, history and x within 1e-12."""
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient

    assert any(n % 256 == 1 for n in BATCH_N) and len(set(BATCH_N)) == 3
    for k, v in dict(VIEWS)[name].items():
        monkeypatch.setenv(k, v)
    systems = [_hub(n, True) for n in BATCH_N]
    B = BatchedConjugateGradient([s[0] for s in systems], [s[1] for s in systems], EPS)
    assert all(v["columns"] == name for v in B.views.values()), B.views
    bt = [torch.from_numpy(s[2]).cuda() for s in systems]
    xs = [torch.zeros_like(b) for b in bt]
    res, _t = B.solve(bt, xs, rtol=1e-8, return_history=True, max_iter=MAX_ITER)
    same_bits = 0
    for (A, L, b), (it, conv, h), xd, (it_o, x_o, h_o) in zip(systems, res, xs, _batch_oracle()):
        x = xd.cpu().numpy()
        s = _solver(A, L, "ext_spai", np.float64)
        assert s.views["A"]["columns"] == name, s.views
        it1, conv1, x1, h1 = _run(s, b, 1e-8, np.float64)
        assert (it, conv) == (it1, conv1) and conv, (A.shape, it, it1)
        np.testing.assert_allclose(h, h1, rtol=1e-12, atol=0)
        assert _rel(x, x1) <= 1e-12
        same_bits += int(np.array_equal(x, x1) and np.array_equal(h, h1))
        assert it == it_o
        np.testing.assert_allclose(h, h_o, rtol=1e-12, atol=0)
        assert _rel(x, x_o) <= 1e-12
    print(f"[batch {name}] systems bit-identical to their single solves (x and history): {same_bits}/{len(systems)}")
