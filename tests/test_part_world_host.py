"""CPU: the virtual world of tests/_virtual_world.py and the conditions of its cases.

tests/test_gpu_part_phases.py runs the row-partitioned PCG's device phases (csrc/lspcg_part.hip) on
these cases to reach specific paths: the grouped reduction (more than 64 workgroups), the
staged-CSR branch (a reordered copy, or SELL declined), r0 > 0, one-row ranks.  Whether a case
reaches its path depends on sizes that are pure host arithmetic; they are pinned here so a GPU run
cannot pass by missing its target.  The numpy restatement of the phases on every rank must
reproduce the global scipy product bit for bit (the contract tests/test_dist_pcg.py states for
Poisson), and every dot the GPU tests compare to 1 ulp is well conditioned."""
import numpy as np
import pytest

from learningsparsepreconditioner4gpu_amd.dist_pcg import GROUPS
from tests import _virtual_world as V

DTYPES = [np.float64, np.float32]


def _mean_offset(M):
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    return float(np.abs(M.indices.astype(np.int64) - rows).mean())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(V.CASES))
def test_numpy_phases_reproduce_global_scipy_bits(name, dtype):
    """Every rank, every part, every matrix: rows [r0, n_own) of the part's extended matrix times
    the rank's extended vector are the global product's rows, bit for bit, and the parts of a rank
    cover each own row exactly once; the reverse gather returns the global vector."""
    hw = V.case_world(name)
    vin = V.inputs(hw.n, dtype)
    v = vin["p"]
    for k, M in enumerate(hw.mats):
        ref = V.as_dtype(M, dtype) @ v
        assert ref.dtype == dtype
        got = []
        for hr in hw.ranks:
            ve = hr.ext(v)
            assert ve.shape == (hr.plan.n_ext,)
            y = np.full(hr.plan.n_own, np.nan, dtype=dtype)
            seen = np.zeros(hr.plan.n_own, dtype=np.int64)
            for hp in hr.parts:
                assert hp.mats[k].shape == (hr.plan.n_ext,) * 2
                assert hp.mats[k][:hp.r0].nnz == 0 and hp.mats[k][hp.n_own:].nnz == 0
                y[hp.r0:hp.n_own] = V.host_spmv(hp, k, ve, dtype)
                seen[hp.r0:hp.n_own] += 1
            assert (seen == 1).all()
            assert np.array_equal(y, ref[hr.plan.order]), (name, k, hr.rank)
            got.append(y)
        assert np.array_equal(hw.to_global(got), ref)
    # the z expression in T, product rounded before the sum
    s, r = vin["t"], vin["r"]
    z = V.host_z(s, r, V.EPS, dtype)
    assert z.dtype == dtype
    prod = (np.asarray(r, dtype=np.float64) * float(np.dtype(dtype).type(V.EPS))).astype(dtype)
    assert np.array_equal(z, (s.astype(np.float64) + prod.astype(np.float64)).astype(dtype))


@pytest.mark.parametrize("name", [n for n in V.CASES if V.CASES[n].parts > 1 or len(V.CASES[n].bounds or ()) > 2])
def test_exchange_plan_of_the_world(name):
    """What rank s packs for rank d is d's halo block owned by s, in order (the copy V.exchange makes)."""
    hw = V.case_world(name)
    v = V.inputs(hw.n, np.float64)["r"]
    for d in hw.ranks:
        pd = d.plan
        at = 0
        for s in hw.ranks:
            cnt = pd.recv_counts[s.rank]
            off = sum(s.plan.send_counts[:d.rank])
            assert s.plan.send_counts[d.rank] == cnt
            sent = s.ext(v)[s.plan.send_idx[off:off + cnt]]
            assert np.array_equal(sent, v[pd.halo[at:at + cnt]])
            own = (pd.halo[at:at + cnt] >= hw.bounds[s.rank]) & (pd.halo[at:at + cnt] < hw.bounds[s.rank + 1])
            assert own.all()
            at += cnt
        assert at == len(pd.halo) and (d.rank != 0 or pd.recv_counts[0] == 0)


def test_case_table_conditions():
    W = {n: V.case_world(n) for n in V.CASES}
    # grouped ranks: more than 64 workgroups (gsz > 1), within the 1024 cap of a reducing grid
    for name, c in V.CASES.items():
        for hr in W[name].ranks:
            g = V.spmv_grid(hr.plan.n_ext)
            assert (g > GROUPS) == (hr.rank in c.grouped), (name, hr.rank, g)
            assert g <= 1024
    assert any(c.grouped for c in V.CASES.values())
    # the two chain sizes: all 64 slots without groups, and the first grid with groups (33 groups,
    # the last of one workgroup)
    a, b = W["chain-16384"].ranks[0].plan, W["chain-16385"].ranks[0].plan
    assert (a.n_ext, b.n_ext) == (16384, 16385)
    assert (V.spmv_grid(a.n_ext), V.n_groups(64)) == (64, 64)
    assert (V.spmv_grid(b.n_ext), V.n_groups(65), 65 - 2 * 32) == (65, 33, 1)
    # Delaunay: 20058 rows, grid 79; big-small: rank 0 has n_ext 18969, grid 75, n_int 17048
    d = W["delaunay-w1"]
    assert d.n == V.N_DEL and V.spmv_grid(d.n) == 79 and V.n_groups(79) == 40
    for name in ("delaunay-big-small-split", "delaunay-big-small-nosplit"):
        p0, p1 = (hr.plan for hr in W[name].ranks)
        assert (p0.n_ext, V.spmv_grid(p0.n_ext)) == (18969, 75)
        assert (p1.n_own, len(p1.halo)) == (2058, 952)
    assert W["delaunay-big-small-split"].ranks[0].plan.n_int == 17048
    assert W["delaunay-big-small-split"].split and not W["delaunay-big-small-nosplit"].split
    # three balanced ranks, the middle one with two neighbours and 1805 sent entries
    w3 = W["delaunay-w3"]
    assert w3.world == 3 and w3.split
    mid = w3.ranks[1].plan
    assert mid.recv_counts[0] > 0 and mid.recv_counts[2] > 0 and int(mid.send_idx.size) == 1805
    # the split cases have interior and boundary rows on every rank
    for name, hw in W.items():
        if hw.split:
            assert all(0 < hr.plan.n_int < hr.plan.n_own and len(hr.parts) == 2 for hr in hw.ranks), name
            assert all(hr.parts[1].r0 == hr.plan.n_int > 0 for hr in hw.ranks)
        else:
            assert all(len(hr.parts) == 1 and hr.parts[0].r0 == 0 for hr in hw.ranks), name
    assert sum(hw.split for hw in W.values()) >= 2
    # one-row ranks: the split was asked for and is turned off by all ranks together
    one = W["delaunay-one-row"]
    assert [hr.plan.n_own for hr in one.ranks] == [1, 16999, 1, 3057]
    assert [one.ranks[0].plan.n_ext, one.ranks[2].plan.n_ext] == [7, 14]
    assert one.requested_split and not one.split and V.spmv_grid(one.ranks[1].plan.n_ext) == 70
    assert any(hr.plan.n_int in (0, hr.plan.n_own) for hr in one.ranks)
    # shuffled: far from banded by the reordering rule (mean |col - row| > 4 n^(2/3), n >= 16384)
    for name in ("shuffled-w1", "shuffled-w2"):
        hr = W[name].ranks[0]
        n = hr.plan.n_ext
        assert n >= 16384
        for M in hr.local:
            assert _mean_offset(M) > 4 * n ** (2 / 3), (name, _mean_offset(M))
            # (the analysis also wants strictly increasing rows of at most 1024 entries)
            assert M.has_sorted_indices and np.diff(M.indptr).max() <= 1024
    A = W["shuffled-w1"].mats[0]
    assert _mean_offset(A) > 4 * A.shape[0] ** (2 / 3)
    assert _mean_offset(W["delaunay-w1"].mats[0]) < 4 * V.N_DEL ** (2 / 3)  # (the mesh's own numbering is not)
    # regular-w2: for A and L of every part, SELL-64 pads no more than 1.15 x nnz (no SELL-64J), some
    # 64-row slice has more than 16 distinct offsets (no SELL-DIA) and every column lies within
    # 32767 of its slice's first row (16-bit offsets): plain 16-bit columns, kind 16
    reg = W["regular-w2"]
    assert reg.split and (np.diff(reg.mats[0].indptr) == 8).all()
    for hr in reg.ranks:
        for hp in hr.parts:
            for M in hp.mats[:2]:
                lens = np.diff(M.indptr)
                pad = np.zeros(-(-lens.size // 64) * 64, dtype=np.int64)
                pad[:lens.size] = lens
                slots = 256 * ((pad.reshape(-1, 64).max(axis=1) + 3) // 4).sum()
                assert slots <= 1.15 * M.nnz, (hr.rank, hp.name, slots, M.nnz)
                rows = np.repeat(np.arange(M.shape[0]), lens)
                sl = rows // 64
                assert np.abs(M.indices.astype(np.int64) - sl * 64).max() <= 32767
                offs = np.unique(sl * (1 << 20) + (M.indices.astype(np.int64) - rows + (1 << 19)))
                assert np.bincount(offs >> 20).max() > 16
    # row lengths: SELL-64J takes no row beyond 64 entries; the ragged matrix has longer ones
    assert max(np.diff(M.indptr).max() for M in W["delaunay-w1"].mats) <= 64
    rag = W["ragged-w1"].mats[0]
    lens = np.sort(np.diff(rag.indptr))
    assert lens[-1] > 4096 and lens[-2] >= 2500 and lens[0] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(V.CASES))
def test_dots_are_well_conditioned(name, dtype):
    """Σ|a_i b_i| / |Σ a_i b_i| <= 2^20 for every dot the GPU phase tests compare with the exact one
    (r·z, r·r of part_l at both eps; p·q of part_a; a·a, b·b of part_norms), over the rows of each part:
    the double-double accumulation error, about n 2^-104 Σ|terms|, is then below 2^-69 relative and
    the 1-ulp bound there is the collapse's single rounding."""
    hw = V.case_world(name)
    vin = V.inputs(hw.n, dtype)
    cap = 2.0 ** 20
    for hr in hw.ranks:
        r, p = hr.own(vin["r"]), hr.own(vin["p"])
        assert V.dot_condition(r, r) <= cap and V.dot_condition(p, p) <= cap
        te, pe = hr.ext(vin["t"]), hr.ext(vin["p"])
        for hp in hr.parts:
            rows = slice(hp.r0, hp.n_own)
            q = V.host_spmv(hp, 0, pe, dtype)
            assert V.dot_condition(p[rows], q) <= cap, (name, hr.rank, hp.name, "pq")
            s = V.host_spmv(hp, 1, te, dtype)
            for eps in (V.EPS, 0.0):
                z = V.host_z(s, r[rows], eps, dtype)
                assert V.dot_condition(r[rows], z) <= cap, (name, hr.rank, hp.name, "rz", eps)
