"""A "virtual world" of the row-partitioned PCG (dist_pcg.py + csrc/lspcg_part.hip): every rank of
one partitioned system held in ONE process, so the device phases can be run and compared rank by
rank, on arbitrary ``bounds``, without ``torch.distributed`` and without a second process.

Host side (numpy / scipy only): ``make_world`` builds every rank's HaloPlan, extended local
matrices and, with the interior / boundary split, the two row_range halves, taking the split's
decision collectively exactly as ``DistributedPCG._setup`` does.  ``CASES`` / ``case_world`` are the
systems of tests/test_part_world_host.py (which pins their conditions on the CPU) and
tests/test_gpu_part_phases.py (which runs them).

Device side: ``open_world`` creates the parts as ``DistributedPCG._setup.make_part`` does and
destroys them in a ``finally``; thin wrappers call each ``lspcg_part_*`` phase on a rank;
``exchange`` stands in for the halo all-to-all with device-to-device copies and ``gather`` for the
all-gather of the reduction buffers; ``iteration`` / ``solve`` repeat ``DistributedPCG._iteration``
and ``solve`` over the ranks of the world."""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp

from learningsparsepreconditioner4gpu_amd import problems as P
from learningsparsepreconditioner4gpu_amd.dist_pcg import (GROUPS, HaloPlan, build_plan, local_matrix, partition_rows,
                                                          row_range)
from tests import _cases

EPS = 3e-3
PHASE_INIT, PHASE_Z, PHASE_ZCG, PHASE_Q, PHASE_R = 0, 1, 2, 3, 4  # lspcg_part.hip PartPhase
MAT_NAMES = ("A", "L", "LT")


# ---------------------------------------------------------------------------------------------
# host side
# ---------------------------------------------------------------------------------------------
def as_dtype(M: sp.csr_matrix, dtype) -> sp.csr_matrix:
    """M with its values in ``dtype``, built from the stored arrays (scipy's astype may reorder a
    row's entries; the extended matrices keep the global order on purpose)."""
    return sp.csr_matrix((M.data.astype(dtype), M.indices, M.indptr), shape=M.shape)


@dataclass
class HostPart:
    """One ``lspcg_part``: its matrices (A[, L, LT] over the extended numbering), the n_own it is
    created with, its first row (lspcg_part_set_rows) and the reduction half its dots go to."""
    name: str  # "all", "int" or "bnd"
    mats: List[sp.csr_matrix]
    n_own: int
    r0: int
    half: int


@dataclass
class HostRank:
    rank: int
    plan: HaloPlan
    local: List[sp.csr_matrix]  # local_matrix of every global matrix
    parts: List[HostPart]       # in launch order: interior (if split) then the main part

    @property
    def main(self) -> HostPart:
        """The part that also runs the elementwise phases, the pack and the state."""
        return self.parts[-1]

    def ext(self, v: np.ndarray) -> np.ndarray:
        """The rank's extended vector of a global one: own rows in plan.order, then the halo."""
        v = np.asarray(v)
        return np.concatenate([v[self.plan.order], v[self.plan.halo]])

    def own(self, v: np.ndarray) -> np.ndarray:
        return np.asarray(v)[self.plan.order]


@dataclass
class HostWorld:
    mats: List[sp.csr_matrix]  # global A[, L, LT]
    bounds: List[int]
    ranks: List[HostRank]
    split: bool                # the collective decision
    requested_split: bool

    @property
    def world(self) -> int:
        return len(self.ranks)

    @property
    def halves(self) -> int:
        return 2 if self.split else 1

    @property
    def n(self) -> int:
        return self.mats[0].shape[0]

    def to_global(self, own_rows: Sequence[np.ndarray]) -> np.ndarray:
        """The reverse gather: every rank's own rows (local order) back at their global places."""
        out = np.empty(self.n, dtype=np.asarray(own_rows[0]).dtype)
        for hr, v in zip(self.ranks, own_rows):
            out[hr.plan.order] = np.asarray(v)[:hr.plan.n_own]
        return out


def make_world(mats: Sequence[sp.csr_matrix], bounds: Sequence[int], split: bool) -> HostWorld:
    """The ranks of global ``mats`` = (A, L, LT) or (A,) (scipy CSR, sorted rows) over ``bounds``.
    ``split``: the own rows are numbered interior first (build_plan) and the split is kept only if
    EVERY rank has 0 < n_int < n_own -- DistributedPCG._setup's all_ranks_agree."""
    mats = [sp.csr_matrix(M) for M in mats]
    assert all(M.has_sorted_indices for M in mats)
    bounds = [int(b) for b in bounds]
    world = len(bounds) - 1
    split = bool(split) and world > 1
    plans = [build_plan(mats, bounds, r, split=split) for r in range(world)]
    on = split and all(0 < p.n_int < p.n_own for p in plans)
    ranks = []
    for r, p in enumerate(plans):
        local = [local_matrix(M, p) for M in mats]
        if on:
            parts = [HostPart("int", [row_range(M, 0, p.n_int) for M in local], p.n_int, 0, 0),
                     HostPart("bnd", [row_range(M, p.n_int, p.n_own) for M in local], p.n_own, p.n_int, 1)]
        else:
            parts = [HostPart("all", local, p.n_own, 0, 0)]
        ranks.append(HostRank(r, p, local, parts))
    return HostWorld(mats, bounds, ranks, on, split)


def n_groups(grid: int) -> int:
    """Group slots a reducing launch of ``grid`` workgroups fills (lspcg_part.hip part_gsz)."""
    gsz = -(-grid // GROUPS)
    return grid if gsz <= 1 else -(-grid // gsz)


def spmv_grid(n_ext: int) -> int:
    """Workgroups of a SELL or staged-CSR launch: one per 256 rows (below the 1024 cap)."""
    return -(-n_ext // 256)


# ---- the systems -----------------------------------------------------------------------------
def chain(n: int) -> sp.csr_matrix:
    A = sp.diags([-np.ones(n - 1), np.full(n, 2.5), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


def _with_factor(A) -> Tuple[sp.csr_matrix, sp.csr_matrix, sp.csr_matrix]:
    A = sp.csr_matrix(A)
    A.sort_indices()
    L = _cases.spai_like(A)
    L.sort_indices()
    return A, L, _cases.sorted_transpose(L)


@functools.lru_cache(maxsize=None)
def system(kind: str):
    """(A, L, LT, b) of a named system; b = A @ mask where the generator has a mask, else A @ 1."""
    if kind.startswith("chain"):
        A, L, LT = _with_factor(chain(int(kind[5:])))
        return A, L, LT, A @ np.ones(A.shape[0])
    if kind == "kuhn":  # the structured system of tests/test_gpu_dist_pcg.py
        A, mask = P.kuhn_dirichlet(17)
        A, L, LT = _with_factor(A)
        return A, L, LT, A @ np.asarray(mask, dtype=np.float64).ravel()
    if kind == "delaunay":
        A, mask, _ = P.delaunay_heat(20000)
        A, L, LT = _with_factor(A)
        return A, L, LT, A @ np.asarray(mask, dtype=np.float64).ravel()
    if kind == "shuffled":  # the Delaunay system in a random numbering: far from banded
        A, L, LT, b = system("delaunay")
        perm = np.random.default_rng(5).permutation(A.shape[0])
        out = []
        for M in (A, L, LT):
            Mp = sp.csr_matrix(M[perm][:, perm])
            Mp.sort_indices()
            out.append(Mp)
        return out[0], out[1], out[2], b[perm]
    if kind == "regular":  # 8 entries in every row at random offsets within +-1500: no padding, no diagonals
        n, rng = 6016, np.random.default_rng(9)
        cols = np.empty((n, 8), dtype=np.int64)
        for i in range(n):
            lo, hi = max(0, i - 1500), min(n, i + 1501)
            c = lo + rng.choice(hi - lo - 1, size=7, replace=False)
            cols[i] = np.sort(np.append(c + (c >= i), i))
        A = sp.csr_matrix((rng.normal(size=8 * n), cols.ravel(), np.arange(0, 8 * n + 1, 8)), shape=(n, n))
        A.setdiag(8.0 + rng.uniform(size=n))
        A, L, LT = _with_factor(A)
        return A, L, LT, A @ np.ones(n)
    if kind == "ragged":  # empty rows, a 5015- and a 2500-entry row; not SPD (the phases need none)
        A = _cases.ragged_matrix(17000)
        return A, A, A, A @ np.ones(A.shape[0])
    raise KeyError(kind)


@dataclass(frozen=True)
class Case:
    name: str
    kind: str
    bounds: Optional[Tuple[int, ...]]  # None: partition_rows(A.indptr, parts)
    split: bool
    parts: int = 1
    grouped: Tuple[int, ...] = ()      # ranks whose SpMV grid exceeds 64 workgroups (gsz > 1)


N_DEL = 20058  # rows of problems.delaunay_heat(20000)
CASES = {c.name: c for c in [
    Case("chain-16384", "chain16384", (0, 16384), False),
    Case("chain-16385", "chain16385", (0, 16385), False, grouped=(0,)),
    Case("delaunay-w1", "delaunay", (0, N_DEL), False, grouped=(0,)),
    Case("delaunay-big-small-split", "delaunay", (0, 18000, N_DEL), True, grouped=(0,)),
    Case("delaunay-big-small-nosplit", "delaunay", (0, 18000, N_DEL), False, grouped=(0,)),
    Case("delaunay-w3", "delaunay", None, True, parts=3),
    Case("delaunay-one-row", "delaunay", (0, 1, 17000, 17001, N_DEL), True, grouped=(1,)),
    Case("shuffled-w1", "shuffled", (0, N_DEL), False, grouped=(0,)),
    # (no interior-first numbering: rank 0's local rows stay sorted, which the reordering analysis needs)
    Case("shuffled-w2", "shuffled", (0, 18000, N_DEL), False, grouped=(0,)),
    Case("ragged-w1", "ragged", (0, 17000), False, grouped=(0,)),
    Case("ragged-w2", "ragged", None, True, parts=2, grouped=(0, 1)),
    # regular rows that are unsorted in local numbering (halo entries left of the own block, interior
    # rows first): SELL-DIA refuses them and the padding is too small for SELL-64J
    Case("chain-w2", "chain16385", (0, 8000, 16385), True),
    Case("kuhn-w2", "kuhn", None, True, parts=2),
    # rows of equal length at scattered offsets: SELL-DIA refuses them and SELL-64 pads nothing, so A and
    # L keep plain 16-bit columns (kind 16)
    Case("regular-w2", "regular", (0, 3008, 6016), True),
]}


@functools.lru_cache(maxsize=None)
def case_world(name: str, precond: bool = True) -> HostWorld:
    """The host world of a case (cached: the plans are built once per session and never changed)."""
    c = CASES[name]
    A, L, LT, _ = system(c.kind)
    bounds = list(c.bounds) if c.bounds is not None else partition_rows(A.indptr, c.parts)
    return make_world((A, L, LT) if precond else (A,), bounds, c.split)


def inputs(n: int, dtype, seed: int = 7) -> Dict[str, np.ndarray]:
    """Standard-normal global vectors r, t, p, q, x, z of a case, cast to ``dtype``."""
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal(n).astype(dtype) for k in ("r", "t", "p", "q", "x", "z")}


# ---- numpy restatement of the phases (the CPU test compares it with the global scipy products) --
def host_spmv(part: HostPart, which: int, v_ext: np.ndarray, dtype) -> np.ndarray:
    """Rows [r0, n_own) of the part's matrix ``which`` times the extended vector, in ``dtype``."""
    y = as_dtype(part.mats[which], dtype) @ np.asarray(v_ext, dtype=dtype)
    return y[part.r0:part.n_own]


def host_z(s: np.ndarray, r: np.ndarray, eps: float, dtype) -> np.ndarray:
    """z = s + T(eps) * r in T, the product rounded before the sum (no fused multiply-add)."""
    t = np.dtype(dtype).type
    return (s.astype(dtype) + (t(eps) * r.astype(dtype)).astype(dtype)).astype(dtype)


def dot_condition(a: np.ndarray, b: np.ndarray) -> float:
    """Σ|a_i b_i| / |Σ a_i b_i| in double (the products of fp32 entries are exact there)."""
    from oracle.linalg import exact_dot

    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = abs(exact_dot(a, b))
    return float(np.sum(np.abs(a * b)) / den) if den > 0 else float("inf")


# ---------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------
@dataclass
class DevPart:
    host: HostPart
    handle: C.c_void_p
    mats: list  # DeviceMatrix, kept alive while the part exists
    kinds: List[int]
    applied: List[bool]


@dataclass
class DevRank:
    host: HostRank
    parts: List[DevPart]
    buf: Dict[str, "object"] = field(default_factory=dict)  # name -> torch tensor

    @property
    def main(self) -> DevPart:
        return self.parts[-1]

    def part(self, name: str) -> DevPart:
        return next(p for p in self.parts if p.host.name == name)


@dataclass
class DevWorld:
    host: HostWorld
    dtype: np.dtype
    ranks: List[DevRank]
    ctx: object
    keep: list = field(default_factory=list)  # gathered buffers alive until the kernels that read them ran

    @property
    def tdtype(self):
        import torch

        return torch.float64 if self.dtype == np.float64 else torch.float32

    def layouts(self) -> List[Tuple[int, str, str, int, bool]]:
        """(rank, part, matrix, prepare_spmv kind, reordered copy attached) of every device matrix."""
        return [(dr.host.rank, dp.host.name, MAT_NAMES[k], dp.kinds[k], dp.applied[k])
                for dr in self.ranks for dp in dr.parts for k in range(len(dp.mats))]


def _lib():
    from learningsparsepreconditioner4gpu_amd import _lib as L

    return L


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@contextlib.contextmanager
def open_world(hw: HostWorld, dtype, ctx):
    """The world's parts on the device, created as DistributedPCG's make_part does; the vectors of
    every rank (r, t, p over n_ext; z, q, x over n_own; send; red = [half][64][nd][2]) zeroed."""
    import torch

    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    L = _lib()
    dtype = np.dtype(dtype)
    dw = DevWorld(hw, dtype, [], ctx)
    dev = ctx.torch_device
    try:
        for hr in hw.ranks:
            sidx = np.ascontiguousarray(hr.plan.send_idx, dtype=np.int32)
            dr = DevRank(hr, [])
            dw.ranks.append(dr)
            for hp in hr.parts:
                dm = [DeviceMatrix.from_scipy(M, dtype=dtype, ctx=ctx, keep_order=True) for M in hp.mats]
                kinds = [M.prepare_spmv() for M in dm]
                applied = [bool(M.spmv_reorder_info["applied"]) for M in dm]
                h = C.c_void_p()
                has_l = len(dm) == 3
                L.call("lspcg_part_create", ctx.handle, dm[0].handle, dm[1].handle if has_l else None,
                       dm[2].handle if has_l else None, hp.n_own, sidx.ctypes.data_as(C.c_void_p), int(sidx.size),
                       C.byref(h))
                dr.parts.append(DevPart(hp, h, dm, kinds, applied))
                if hp.r0:
                    L.call("lspcg_part_set_rows", h, int(hp.r0))
            ne, no = hr.plan.n_ext, hr.plan.n_own
            td = dw.tdtype
            for name in ("r", "t", "p"):
                dr.buf[name] = torch.zeros(ne, dtype=td, device=dev)
            for name in ("z", "q", "x"):
                dr.buf[name] = torch.zeros(max(no, 1), dtype=td, device=dev)
            dr.buf["send"] = torch.zeros(max(int(sidx.size), 1), dtype=td, device=dev)
            dr.buf["red"] = torch.zeros(2 * GROUPS * 2 * 2, dtype=torch.float64, device=dev)
        yield dw
    finally:
        ctx.synchronize()
        for dr in dw.ranks:
            for dp in dr.parts:
                if dp.handle is not None and dp.handle.value:
                    L._lib.lspcg_part_destroy(dp.handle)
                    dp.handle = None
            dr.parts.clear()
        dw.keep.clear()


def to_dev(dw: DevWorld, a: np.ndarray):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).to(dw.ctx.torch_device)


def red_half(dr: DevRank, nd: int, half: int):
    """Half ``half`` of the rank's reduction buffer for nd dots: [64][nd][2] doubles, halves adjacent."""
    return dr.buf["red"][half * GROUPS * nd * 2:(half + 1) * GROUPS * nd * 2]


# ---- one phase on one part --------------------------------------------------------------------
def pack(dr: DevRank, v, send):
    _lib().call("lspcg_part_pack", dr.main.handle, _ptr(v), _ptr(send))


def norms(dp: DevPart, a, b, red):
    _lib().call("lspcg_part_norms", dp.handle, _ptr(a), _ptr(b), _ptr(red))


def lt(dp: DevPart, r_ext, t_ext):
    _lib().call("lspcg_part_lt", dp.handle, _ptr(r_ext), _ptr(t_ext))


def l(dp: DevPart, t_ext, r, eps: float, z, red):  # noqa: E743
    _lib().call("lspcg_part_l", dp.handle, _ptr(t_ext), _ptr(r), float(eps), _ptr(z), _ptr(red))


def a(dp: DevPart, p_ext, q, red):
    _lib().call("lspcg_part_a", dp.handle, _ptr(p_ext), _ptr(q), _ptr(red))


def update_p(dp: DevPart, z, p_ext, beta: float, first: bool):
    _lib().call("lspcg_part_update_p", dp.handle, _ptr(z), _ptr(p_ext), float(beta), int(bool(first)))


def update_xr(dp: DevPart, alpha: float, p_ext, q, x, r_ext):
    _lib().call("lspcg_part_update_xr", dp.handle, float(alpha), _ptr(p_ext), _ptr(q), _ptr(x), _ptr(r_ext))


def state_init(dp: DevPart, rtol: float, max_iter: int, hist=None):
    _lib().call("lspcg_part_state_init", dp.handle, float(rtol), int(max_iter), _ptr(hist))


def scalars(dp: DevPart, gathered, world: int, phase: int):
    _lib().call("lspcg_part_scalars", dp.handle, _ptr(gathered), int(world), int(phase))


def update_p_dev(dp: DevPart, z, p_ext):
    _lib().call("lspcg_part_update_p_dev", dp.handle, _ptr(z), _ptr(p_ext))


def update_xr_dev(dp: DevPart, p_ext, q, x, r_ext):
    _lib().call("lspcg_part_update_xr_dev", dp.handle, _ptr(p_ext), _ptr(q), _ptr(x), _ptr(r_ext))


def status(dp: DevPart) -> Tuple[int, int]:
    it, done = C.c_int64(), C.c_int()
    _lib().call("lspcg_part_status", dp.handle, C.byref(it), C.byref(done))
    return it.value, done.value


def progress(dp: DevPart) -> Tuple[int, int, float, float]:
    it, done, rr, atol = C.c_int64(), C.c_int(), C.c_double(), C.c_double()
    _lib().call("lspcg_part_progress", dp.handle, C.byref(it), C.byref(done), C.byref(rr), C.byref(atol))
    return it.value, done.value, rr.value, atol.value


# ---- the world's exchanges --------------------------------------------------------------------
def exchange(dw: DevWorld, name: str):
    """The halo all-to-all of vector ``name``: every rank packs its send buffer, then each segment is
    copied device to device into the tail of its destination's extended vector."""
    if dw.host.world == 1:
        return
    for dr in dw.ranks:
        pack(dr, dr.buf[name], dr.buf["send"])
    for d in dw.ranks:
        pd = d.host.plan
        at = pd.n_own
        for s in dw.ranks:
            cnt = pd.recv_counts[s.host.rank]
            if cnt:
                off = sum(s.host.plan.send_counts[:d.host.rank])
                assert s.host.plan.send_counts[d.host.rank] == cnt
                d.buf[name][at:at + cnt].copy_(s.buf["send"][off:off + cnt])
            at += cnt
        assert at == pd.n_ext


def gather(dw: DevWorld, nd: int, halves: int):
    """Every rank's first ``halves`` reduction halves for nd dots, concatenated rank-major (as
    dist_pcg.gather_device): a device tensor of world * halves * 64 * nd * 2 doubles."""
    import torch

    return torch.cat([dr.buf["red"][:halves * GROUPS * nd * 2] for dr in dw.ranks])


def gathered_rows(dw: DevWorld, nd: int, halves: int) -> np.ndarray:
    """``gather`` on the host as [world, halves * 64 * nd * 2], dist_pcg.sum_groups' input."""
    return gather(dw, nd, halves).cpu().numpy().reshape(dw.host.world, -1)


def all_scalars(dw: DevWorld, nd: int, phase: int, halves: int = 1):
    """lspcg_part_scalars on every rank's main part from the gathered buffer."""
    g = gather(dw, nd, halves) if nd else None
    dw.keep.append(g)
    del dw.keep[:-8]
    for dr in dw.ranks:
        scalars(dr.main, g, dw.host.world * halves, phase)


def spmv_phase(dw: DevWorld, name: str, call):
    """One SpMV phase over the world as DistributedPCG._spmv runs it: the halo of ``name``
    exchanged, then ``call(rank, part, half)`` on the interior part (if split) and the main part."""
    exchange(dw, name)
    for dr in dw.ranks:
        for dp in dr.parts:
            call(dr, dp, dp.host.half)


def phase_lt(dw: DevWorld):
    spmv_phase(dw, "r", lambda dr, dp, h: lt(dp, dr.buf["r"], dr.buf["t"]))


def phase_l(dw: DevWorld, eps: float):
    spmv_phase(dw, "t", lambda dr, dp, h: l(dp, dr.buf["t"], dr.buf["r"], eps, dr.buf["z"], red_half(dr, 2, h)))


def phase_a(dw: DevWorld):
    spmv_phase(dw, "p", lambda dr, dp, h: a(dp, dr.buf["p"], dr.buf["q"], red_half(dr, 1, h)))


def init(dw: DevWorld, b_global: np.ndarray, rtol: float, max_iter: int, hists=None):
    """solve()'s start on every rank: x = 0, r = b, p = 0, the state, the norms and scalars(init)."""
    for k, dr in enumerate(dw.ranks):
        no = dr.host.plan.n_own
        for name in ("x", "r", "p"):
            dr.buf[name].zero_()
        dr.buf["r"][:no] = to_dev(dw, dr.host.own(b_global).astype(dw.dtype))
        state_init(dr.main, rtol, max_iter, hists[k] if hists is not None else None)
        norms(dr.main, dr.buf["r"], dr.buf["r"], dr.buf["red"])
    all_scalars(dw, 2, PHASE_INIT)


def iteration(dw: DevWorld, eps: float, precond: bool = True):
    """DistributedPCG._iteration over the ranks of the world (device-side recurrence)."""
    hv = dw.host.halves
    if precond:
        phase_lt(dw)
        phase_l(dw, eps)
        all_scalars(dw, 2, PHASE_Z, hv)
    else:
        all_scalars(dw, 0, PHASE_ZCG)
    for dr in dw.ranks:
        update_p_dev(dr.main, dr.buf["z"] if precond else dr.buf["r"], dr.buf["p"])
    phase_a(dw)
    all_scalars(dw, 1, PHASE_Q, hv)
    for dr in dw.ranks:
        update_xr_dev(dr.main, dr.buf["p"], dr.buf["q"], dr.buf["x"], dr.buf["r"])
    if not precond:
        for dr in dw.ranks:
            norms(dr.main, dr.buf["r"], dr.buf["r"], dr.buf["red"])
        all_scalars(dw, 2, PHASE_R)


def solve(dw: DevWorld, b_global: np.ndarray, eps: float, rtol: float, max_iter: int, precond: bool = True,
          chunk: int = 8):
    """DistributedPCG.solve over the virtual world, the status of rank 0 read every ``chunk``
    iterations.  Returns (per-rank (iter, done), x in global order, rank 0's history)."""
    import torch

    hists = [torch.full((max_iter + 2,), float("nan"), dtype=torch.float64, device=dw.ctx.torch_device)
             for _ in dw.ranks]
    init(dw, b_global, rtol, max_iter, hists)
    _, done = status(dw.ranks[0].main)
    while not done:
        for _ in range(chunk):
            iteration(dw, eps, precond)
        _, done = status(dw.ranks[0].main)
    st = [status(dr.main) for dr in dw.ranks]
    x = dw.host.to_global([dr.buf["x"].cpu().numpy() for dr in dw.ranks])
    return st, x, [h.cpu().numpy() for h in hists]
