"""GPU: the device phases of the row-partitioned PCG (csrc/lspcg_part.hip), rank by rank on the
virtual worlds of tests/_virtual_world.py -- every rank of a partitioned system in this process, the
halo exchange stood in for by device-to-device copies, no process spawned.

The cases (conditions pinned on the CPU by tests/test_part_world_host.py) reach what the whole
solves of tests/test_gpu_dist_pcg.py cannot at their sizes: launches of more than 64 workgroups
(the grouped reduction, gsz > 1, with a ragged last group), the staged-CSR branch of part_spmv (a
reordered copy attached, or SELL declined), SELL-64J and SELL-DIA under the own-row epilogues, a
part whose first row is r0 > 0, one-row ranks, and fp32 on more than one rank.

Every expected value is scipy / numpy in the vectors' dtype (stores: bit for bit),
oracle.linalg.exact_dot over the rows the launch reduced (dots: within 1 ulp of the exact value),
or dist_pcg.sum_groups of the gathered buffers (the device-side scalars: bit for bit).  The 1-ulp
bound is derived: the double-double sums carry an error of about n 2^-104 Σ|terms|, below 2^-69
relative under the conditioning cap 2^20 the CPU test asserts, so what is left is the one rounding
of collapsing s + c to a double (fp32 entries: their products are exact in double)."""
import numpy as np
import pytest

from oracle import linalg as O
from learningsparsepreconditioner4gpu_amd.dist_pcg import GROUPS, sum_groups
from tests import _virtual_world as V

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
SENT = -777.25  # exactly representable in fp32; no computed entry equals it
SEEN = {}       # (case, dtype name) -> layouts of the matrices a phase ran on


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _sent(dw, n, dtype=None):
    import torch

    return torch.full((max(int(n), 1),), SENT, dtype=dtype or dw.tdtype, device=dw.ctx.torch_device)


def _sent_red(dw, nd):
    """A reduction buffer [64][nd][2] of doubles, pre-filled (the call zeroes it)."""
    import torch

    return _sent(dw, GROUPS * nd * 2, torch.float64)


def _is_sent(a):
    return bool(np.all(np.asarray(a) == SENT))


def _within_ulp(got, exact):
    return abs(got - exact) <= np.spacing(abs(exact))


def _check_red(red, nd, grid, exact, what):
    """A reduction buffer [64][nd][2]: the totals within 1 ulp of the exact dots, the slots past the
    launch's groups exactly (+0.0, +0.0)."""
    red = np.asarray(red).reshape(GROUPS, nd, 2)
    ng = V.n_groups(grid)
    assert not _bits(red[ng:]).any(), (what, "slots past the groups", ng)
    tot = sum_groups(red.reshape(1, -1), nd)
    for j in range(nd):
        print(f"    {what}[{j}]: got {tot[j]!r} exact {exact[j]!r} diff/ulp "
              f"{abs(tot[j] - exact[j]) / np.spacing(abs(exact[j])):.3f}")
        assert _within_ulp(tot[j], exact[j]), (what, j, tot[j], exact[j])


def _run_phases(gpu_ctx, name, dtype):  # noqa: C901
    hw = V.case_world(name)
    T = np.dtype(dtype).type
    vin = V.inputs(hw.n, dtype)
    G = [V.as_dtype(M, dtype) for M in hw.mats]  # global A, L, LT in T
    ref_t = G[2] @ vin["r"]
    ref_s = G[1] @ vin["t"]
    ref_q = G[0] @ vin["p"]
    with V.open_world(hw, dtype, gpu_ctx) as dw:
        print(f"\n{name} {np.dtype(dtype).name}: split {hw.split}")
        for row in dw.layouts():
            print("    layout rank %d part %s %s: kind %d applied %s" % row)
        sends = []
        for dr in dw.ranks:
            hr, pl = dr.host, dr.host.plan
            no, ne = pl.n_own, pl.n_ext
            grid = V.spmv_grid(ne)
            # ---- pack
            r_ext = hr.ext(vin["r"])
            send = _sent(dw, pl.send_idx.size + 3)
            V.pack(dr, V.to_dev(dw, r_ext), send)
            send = send.cpu().numpy()
            ns = int(pl.send_idx.size)
            assert _same(send[:ns], r_ext[pl.send_idx]) and _is_sent(send[ns:]), (name, hr.rank, "pack")
            sends.append(send[:ns])
            t_ext, p_ext = hr.ext(vin["t"]), hr.ext(vin["p"])
            r_own, p_own = hr.own(vin["r"]), hr.own(vin["p"])
            d_r, d_t, d_p = (V.to_dev(dw, v) for v in (r_ext, t_ext, p_ext))
            for dp in dr.parts:
                hp = dp.host
                rows = slice(hp.r0, hp.n_own)
                tag = (name, hr.rank, hp.name)
                # ---- lt: t[r0:n_own] = (LT r)[order], everything else untouched
                t = _sent(dw, ne)
                V.lt(dp, d_r, t)
                t = t.cpu().numpy()
                assert _same(t[rows], ref_t[pl.order][rows]), tag + ("lt",)
                assert _is_sent(t[:hp.r0]) and _is_sent(t[hp.n_own:]), tag + ("lt wrote outside its rows",)
                # ---- l: z = s + T(eps) r, the groups of r·z and r·r; twice (same bits)
                for eps in (V.EPS, 0.0):
                    want = V.host_z(ref_s[pl.order][rows], r_own[rows], eps, dtype)
                    reds = []
                    for _ in range(2):
                        z, red = _sent(dw, no), _sent_red(dw, 2)
                        V.l(dp, d_t, d_r, eps, z, red)
                        z, red = z.cpu().numpy(), red.cpu().numpy()
                        assert _same(z[rows], want), tag + ("l", eps)
                        assert _is_sent(z[:hp.r0]) and _is_sent(z[hp.n_own:]), tag + ("l wrote outside its rows",)
                        reds.append(red)
                    assert _same(reds[0], reds[1]), tag + ("l: a second run changed the reduction's bits",)
                    exact = [O.exact_dot(r_own[rows], z[rows]), O.exact_dot(r_own[rows], r_own[rows])]
                    _check_red(reds[0], 2, grid, exact, f"rank {hr.rank} {hp.name} l eps={eps}")
                # ---- a: q = (A p)[order], the groups of p·q; twice
                reds = []
                for _ in range(2):
                    q, red = _sent(dw, no), _sent_red(dw, 1)
                    V.a(dp, d_p, q, red)
                    q, red = q.cpu().numpy(), red.cpu().numpy()
                    assert _same(q[rows], ref_q[pl.order][rows]), tag + ("a",)
                    assert _is_sent(q[:hp.r0]) and _is_sent(q[hp.n_own:]), tag + ("a wrote outside its rows",)
                    reds.append(red)
                assert _same(reds[0], reds[1]), tag + ("a: a second run changed the reduction's bits",)
                _check_red(reds[0], 1, grid, [O.exact_dot(p_own[rows], q[rows])], f"rank {hr.rank} {hp.name} a")
            # ---- norms (the main part; its grid follows n_own); twice
            reds = []
            for _ in range(2):
                red = _sent_red(dw, 2)
                V.norms(dr.main, d_r, d_p, red)
                reds.append(red.cpu().numpy())
            assert _same(reds[0], reds[1]), (name, hr.rank, "norms: a second run changed the bits")
            _check_red(reds[0], 2, max(1, -(-no // 256)), [O.exact_dot(r_own, r_own), O.exact_dot(p_own, p_own)],
                       f"rank {hr.rank} norms")
            # ---- update_p / update_xr over [0, n_own), the halo tail untouched
            z_own, q_own, x_own = hr.own(vin["z"]), hr.own(vin["q"]), hr.own(vin["x"])
            d_z, d_q = V.to_dev(dw, z_own), V.to_dev(dw, q_own)
            beta, alpha = 0.731, -1.37
            for first in (True, False):
                pb = V.to_dev(dw, p_ext)
                V.update_p(dr.main, d_z, pb, beta, first)
                pb = pb.cpu().numpy()
                want = z_own if first else ((p_own * T(beta)).astype(dtype) + z_own).astype(dtype)
                assert _same(pb[:no], want) and _same(pb[no:], p_ext[no:]), (name, hr.rank, "update_p", first)
            xb, rb = V.to_dev(dw, x_own), V.to_dev(dw, r_ext)
            V.update_xr(dr.main, alpha, d_p, d_q, xb, rb)
            xb, rb = xb.cpu().numpy(), rb.cpu().numpy()
            assert _same(xb, (x_own + (T(alpha) * p_own).astype(dtype)).astype(dtype)), (name, hr.rank, "update x")
            assert _same(rb[:no], (r_own - (T(alpha) * q_own).astype(dtype)).astype(dtype)), (name, hr.rank, "update r")
            assert _same(rb[no:], r_ext[no:]), (name, hr.rank, "update_xr touched the halo")
        # ---- across the world: what rank s sends to rank d is d's halo block owned by s, in order
        for d in hw.ranks:
            at = 0
            for s in hw.ranks:
                cnt = d.plan.recv_counts[s.rank]
                off = sum(s.plan.send_counts[:d.rank])
                assert _same(sends[s.rank][off:off + cnt], vin["r"][d.plan.halo[at:at + cnt]]), (name, s.rank, d.rank)
                at += cnt
        SEEN[(name, np.dtype(dtype).name)] = dw.layouts()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(V.CASES))
def test_phases_match_scipy_rank_by_rank(gpu_ctx, name, dtype):
    """pack, lt, l (eps = 3e-3 and 0), a, norms, update_p and update_xr on every rank and part of the
    case: stores bit for bit in T with the rows outside [r0, n_own) and the halo tail untouched (every
    output pre-filled with a sentinel), the group buffers within 1 ulp of the exact dots with the
    unused slots exactly zero, and a second run of each reducing phase giving the same bits (the
    last arriver of a group sums in block order; a ticket left unreset would show here)."""
    _run_phases(gpu_ctx, name, dtype)


def _T(dtype, v):
    return float(np.dtype(dtype).type(v))


def _sqrt(dtype, v):
    return float(np.sqrt(np.dtype(dtype).type(v)))


def _own_all(dw, name):
    return dw.host.to_global([dr.buf[name].cpu().numpy() for dr in dw.ranks])


def _progress_all(dw):
    st = [V.progress(dr.main) for dr in dw.ranks]
    assert all(_same(np.array(s[2:]), np.array(st[0][2:])) and s[:2] == st[0][:2] for s in st), st
    return st[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,precond", [(n, True) for n in V.CASES] + [("delaunay-w3", False)])
def test_device_recurrence_two_iterations(gpu_ctx, name, precond, dtype):
    """Two iterations enqueued by hand on the virtual world (state_init, norms, scalars(init); then lt,
    l, scalars(Z), update_p_dev, a, scalars(Q), update_xr_dev -- without L: scalars(Zcg) ... norms,
    scalars(R)), the halos exchanged between the phases and the reductions gathered with world *
    halves.  After the init, rr and atol of every rank are solve_host's recurrence, bit for bit; after
    each iteration p, x and r on every rank are the host expressions on the global scipy products,
    bit for bit, with beta and alpha from sum_groups of the gathered buffers."""
    hw = V.case_world(name, precond)
    T = np.dtype(dtype).type
    G = [V.as_dtype(M, dtype) for M in hw.mats]
    b = V.system(V.CASES[name].kind)[3].astype(dtype)
    rtol, hv = 1e-8, hw.halves
    with V.open_world(hw, dtype, gpu_ctx) as dw:
        V.init(dw, b, rtol, 1000)
        rr0, bb = (_T(dtype, v) for v in sum_groups(V.gathered_rows(dw, 2, 1), 2))
        k, done, rr, atol = _progress_all(dw)
        assert (k, done) == (0, 0)
        assert _same(np.array([rr, atol]), np.array([rr0, max(0.0, rtol * _sqrt(dtype, bb))]))
        x, r, p = np.zeros(hw.n, dtype), b.copy(), np.zeros(hw.n, dtype)
        rho_prev, rr_k = None, rr0
        for k in range(2):
            if precond:
                V.phase_lt(dw)
                V.phase_l(dw, V.EPS)
                rows = V.gathered_rows(dw, 2, hv)
                V.all_scalars(dw, 2, V.PHASE_Z, hv)
                z = V.host_z(G[1] @ (G[2] @ r), r, V.EPS, dtype)
                rho = _T(dtype, sum_groups(rows, 2)[0])
            else:
                V.all_scalars(dw, 0, V.PHASE_ZCG)
                z, rho = r, rr_k
            for dr in dw.ranks:
                V.update_p_dev(dr.main, dr.buf["z"] if precond else dr.buf["r"], dr.buf["p"])
            p = z.copy() if k == 0 else ((p * T(T(rho) / T(rho_prev))).astype(dtype) + z).astype(dtype)
            assert _same(_own_all(dw, "p"), p), (name, k, "p")
            V.phase_a(dw)
            rows = V.gathered_rows(dw, 1, hv)
            V.all_scalars(dw, 1, V.PHASE_Q, hv)
            q = G[0] @ p
            alpha = T(T(rho) / T(_T(dtype, sum_groups(rows, 1)[0])))
            for dr in dw.ranks:
                V.update_xr_dev(dr.main, dr.buf["p"], dr.buf["q"], dr.buf["x"], dr.buf["r"])
            x = (x + (alpha * p).astype(dtype)).astype(dtype)
            r = (r - (alpha * q).astype(dtype)).astype(dtype)
            assert _same(_own_all(dw, "x"), x) and _same(_own_all(dw, "r"), r), (name, k, "x, r")
            if not precond:
                for dr in dw.ranks:
                    V.norms(dr.main, dr.buf["r"], dr.buf["r"], dr.buf["red"])
                rr_k = _T(dtype, sum_groups(V.gathered_rows(dw, 2, 1), 2)[0])
                V.all_scalars(dw, 2, V.PHASE_R)
                assert _progress_all(dw)[2] == rr_k
            rho_prev = rho
            assert _progress_all(dw)[:2] == (k + 1, 0)
        # every rank's halo of p holds its owners' entries (the exchange put them there)
        for dr in dw.ranks:
            no = dr.host.plan.n_own
            assert _same(dr.buf["p"].cpu().numpy()[no:], p[dr.host.plan.halo])


def _snapshot(dw):
    out = []
    for dr in dw.ranks:
        out.append([dr.buf[n].cpu().numpy().copy() for n in ("p", "x", "r")] +
                   [np.array(V.progress(dr.main), dtype=np.float64)])
    return out


def _poke_after_stop(dw, code):
    """Once the state says done: one more update_p_dev, update_xr_dev and scalars of every phase that
    tests `done` (Z, Zcg, Q, R; phase 0 is the next solve's init) change nothing, bit for bit."""
    import torch

    hv = dw.host.halves
    for dr in dw.ranks:  # data an unguarded update would visibly use
        dr.buf["z"].copy_(torch.arange(1, dr.buf["z"].numel() + 1, device=dr.buf["z"].device).to(dw.tdtype))
        dr.buf["q"].copy_(dr.buf["z"] * 0.5)
        dr.buf["red"].fill_(3.0)
    before = _snapshot(dw)
    assert all(int(s[3][1]) == code for s in before), [s[3] for s in before]
    for dr in dw.ranks:
        V.update_p_dev(dr.main, dr.buf["z"], dr.buf["p"])
        V.update_xr_dev(dr.main, dr.buf["p"], dr.buf["q"], dr.buf["x"], dr.buf["r"])
    for nd, phase in ((2, V.PHASE_Z), (0, V.PHASE_ZCG), (1, V.PHASE_Q), (2, V.PHASE_R)):
        V.all_scalars(dw, nd, phase, hv if nd and phase != V.PHASE_R else 1)
    after = _snapshot(dw)
    for s0, s1 in zip(before, after):
        assert all(_same(u, v) for u, v in zip(s0, s1)), code


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stop_codes_and_frozen_state(gpu_ctx, dtype):
    """done == 4 for b = 0 after the init; done == 3 at scalars(Z) when one entry of one rank's r is
    NaN (data in a vector: nothing faults); done == 2 at the second top-of-loop test with max_iter
    = 1.  After each stop the state and the vectors are frozen.  World 2, split on."""
    name = "delaunay-big-small-split"
    hw = V.case_world(name)
    assert hw.split
    b = V.system("delaunay")[3].astype(dtype)
    with V.open_world(hw, dtype, gpu_ctx) as dw:
        # ‖b‖ = 0
        V.init(dw, np.zeros(hw.n, dtype), 1e-8, 1000)
        assert all(V.status(dr.main) == (0, 4) for dr in dw.ranks)
        _poke_after_stop(dw, 4)
        # a NaN in rank 1's residual
        V.init(dw, b, 1e-8, 1000)  # (sets r = b on every rank; redone below with the NaN in place)
        for dr in dw.ranks:
            V.state_init(dr.main, 1e-8, 1000)
        dw.ranks[1].buf["r"][5] = float("nan")
        for dr in dw.ranks:
            V.norms(dr.main, dr.buf["r"], dr.buf["r"], dr.buf["red"])
        V.all_scalars(dw, 2, V.PHASE_INIT)
        assert all(V.status(dr.main) == (0, 0) for dr in dw.ranks)
        V.phase_lt(dw)
        V.phase_l(dw, V.EPS)
        V.all_scalars(dw, 2, V.PHASE_Z, hw.halves)
        assert all(V.status(dr.main) == (0, 3) for dr in dw.ranks)
        _poke_after_stop(dw, 3)
        # max_iter = 1
        V.init(dw, b, 1e-8, 1)
        V.iteration(dw, V.EPS)
        assert all(V.status(dr.main) == (1, 0) for dr in dw.ranks)
        V.phase_lt(dw)
        V.phase_l(dw, V.EPS)
        V.all_scalars(dw, 2, V.PHASE_Z, hw.halves)
        assert all(V.status(dr.main) == (1, 2) for dr in dw.ranks)
        _poke_after_stop(dw, 2)


# ---- whole solves on the virtual world -------------------------------------------------------
SOLVE_RTOL = {np.float64: 1e-3, np.float32: 1e-3}
_ORACLE = {}


def _oracle(kind, dtype, precond):
    """oracle.linalg.pcg with correctly rounded dots, once per (system, dtype, preconditioner)."""
    key = (kind, np.dtype(dtype).name, precond)
    if key not in _ORACLE:
        A, L, _, b = V.system(kind)
        ps = O.spai_operator(V.as_dtype(L, dtype), V.EPS) if precond else None
        _ORACLE[key] = O.pcg(V.as_dtype(A, dtype), b.astype(dtype), ps, rtol=SOLVE_RTOL[dtype], dot="exact",
                             dtype=dtype)
    return _ORACLE[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,precond", [("delaunay-w3", True), ("delaunay-one-row", True), ("shuffled-w2", True),
                                          ("delaunay-w3", False)])
def test_virtual_world_solve_matches_oracle_and_single_gpu(gpu_ctx, name, precond, dtype):
    """ext_spai (L = spai_like(A), eps = 3e-3) or plain CG, b = A @ mask, on the virtual world with the
    device-side recurrence, against oracle.linalg.pcg(dot="exact") and the single-GPU solver, with
    the tolerances of tests/test_gpu_dist_pcg.py: equal counts, history to 1e-12, x to 1e-12 ‖x‖
    (fp32: equal counts, x to 1e-5), every rank reporting the same count and done.

    Choice of stop: all three solvers run to rtol = 1e-3 instead of 1e-8 (533 oracle iterations, 5 s
    of CPU, on this system): the counts are then a real comparison, not a shared iteration cap, and a
    test stays within a few seconds."""
    import torch

    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient

    hw = V.case_world(name, precond)
    kind = V.CASES[name].kind
    A, L, _, b = V.system(kind)
    rtol = SOLVE_RTOL[dtype]
    it_o, x_o, h_o = _oracle(kind, dtype, precond)
    assert 10 < it_o < 400, it_o
    with V.open_world(hw, dtype, gpu_ctx) as dw:
        st, x, hists = V.solve(dw, b, V.EPS, rtol, 1000, precond)  # (a wrong run ends at the cap, done == 2)
    assert all(s == (it_o, 1) for s in st), (st, it_o)
    assert all(_same(h, hists[0]) for h in hists)
    s = PreconditionedConjugateGradient(A, device="cuda", preconditioner="ext_spai" if precond else "none", dtype=dtype)
    if precond:
        s.set_spai(L, V.EPS)
    bt = torch.as_tensor(b.astype(dtype), device="cuda")
    xs = torch.zeros_like(bt)
    it_s, conv_s, _ = s.solve(bt, xs, rtol=rtol)
    assert conv_s and it_s == it_o, (it_s, it_o)
    xs = xs.cpu().numpy().astype(np.float64)
    x = x.astype(np.float64)
    x_o = np.asarray(x_o, dtype=np.float64)
    if dtype == np.float64:
        np.testing.assert_allclose(hists[0][:it_o + 1], h_o[:it_o + 1], rtol=1e-12, atol=0)
        assert np.linalg.norm(x - x_o) <= 1e-12 * np.linalg.norm(x_o)
        np.testing.assert_allclose(x, xs, rtol=0, atol=1e-12 * np.abs(x_o).max())
    else:
        assert np.linalg.norm(x - x_o) <= 1e-5 * np.linalg.norm(x_o)
        assert np.linalg.norm(x - xs) <= 1e-5 * np.linalg.norm(x_o)


def test_layouts_seen_over_the_module(gpu_ctx):
    """Over the cases the phase test ran (any not yet run in this session is run here), the own-row
    epilogues met SELL-DIA (kind 1), SELL-64J (17), the staged-CSR kernel with SELL declined (0) and
    with a reordered copy attached, and one of the coded / 16-bit / int32 SELL-64 layouts; the case
    table's expectations per case hold.  The layout is chosen on the device: if this fails, the
    input is to be replaced by one that takes the intended layout, not the assertion relaxed."""
    for name in V.CASES:
        if (name, "float64") not in SEEN:
            _run_phases(gpu_ctx, name, np.float64)
    kinds, applied = set(), False
    for (name, dt), rows in sorted(SEEN.items()):
        for rank, part, mat, kind, ap in rows:
            print(f"{name} {dt} rank {rank} part {part} {mat}: kind {kind} applied {ap}")
            kinds.add(kind if not ap else -1)
            applied |= ap
    by = {name: {(r[3], r[4]) for r in SEEN[(name, "float64")]} for name in V.CASES}
    assert by["chain-16384"] == {(1, False)} and by["chain-16385"] == {(1, False)}, by
    assert by["delaunay-w1"] == {(17, False)}, by
    assert by["ragged-w1"] == {(0, False)} and (0, False) in by["ragged-w2"], by
    assert (16, False) in by["regular-w2"], by
    assert all(ap for _, ap in by["shuffled-w1"]), by
    assert any(ap for _, ap in by["shuffled-w2"]), by
    assert {1, 17, 0} <= kinds and applied and kinds & {8, 16, 32}, kinds
