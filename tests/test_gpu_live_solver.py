"""GPU: workspace.live_solver -- the chain matrix on the device -> sample -> A_sys, L -> PCG and its
refresh after new values -- against the existing device pipeline fed a host-built GraphSample.

The host sample's value fields are dataset.make_data's expressions evaluated with the scale the
device computed (tests/test_gpu_device_sample.py: the device's fields are those, bit for bit), so
every later step sees identical inputs and must give identical bits."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from learningsparsepreconditioner4gpu_amd import problems as P
from learningsparsepreconditioner4gpu_amd.data import make_sample
from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient
from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix
from learningsparsepreconditioner4gpu_amd.workspace import ScaledInferenceWorkspace, SimpleInferenceWorkspace

pytestmark = pytest.mark.gpu

RTOL = 1e-6
MAX_ITER = 10  # times n: CG in floating point may need more than n steps (the 240-unknown elasticity box does)
SEED = 3  # of the workspaces' random weights


@functools.lru_cache(maxsize=None)
def system(name):
    """``(A sorted scipy, mask [n] fp64, node_features or None, block size)``, never modified."""
    nf, bs = None, 1
    if name == "bunny":
        A, mask, nf = P.heat_bunny()
        nf = np.ascontiguousarray(nf, dtype=np.float32)
        nf.setflags(write=False)
    elif name == "poisson":
        A, mask, _ = P.poisson2d_grid(40, 33)
    else:
        A, mask, _ = P.elasticity_box(5, 4, 4)
        bs = 3
    A = sp.csr_matrix(A).astype(np.float64)
    A.sort_indices()
    if bs == 3:
        A = sp.bsr_matrix(A, blocksize=(3, 3))
        A.sort_indices()
    mask = np.ascontiguousarray(mask, dtype=np.float64).reshape(-1)
    assert mask.size == A.shape[0] and np.any(mask == 0) and set(np.unique(mask)) <= {0.0, 1.0}
    mask.setflags(write=False)
    return A, mask, nf, bs


def second_values(A):
    """A second coefficient field on the same pattern: D A D with a positive diagonal D (still SPD)."""
    d = 1.0 + 0.5 * np.random.default_rng(9).random(A.shape[0])
    A2 = sp.diags(d) @ sp.csr_matrix(A) @ sp.diags(d)
    A2 = sp.csr_matrix(A2)
    A2.sort_indices()
    if isinstance(A, sp.bsr_matrix):
        A2 = sp.bsr_matrix(A2, blocksize=A.blocksize)
        A2.sort_indices()
    assert np.array_equal(A2.indices, A.indices) and np.array_equal(A2.indptr, A.indptr)
    return A2


def workspace(cls, nf, bs):
    return cls(node_features=(0 if nf is None else nf.shape[1]) + bs, edge_features=bs * bs, block_size=bs, seed=SEED)


def host_sample_with_scale(A, mask, nf, bs, s):
    """make_sample's host sample with the value fields re-evaluated at the scale ``s``."""
    hs = make_sample(A, mask=mask, node_features=nf, block_size=bs)
    assert abs(hs.matrix_scale - s) <= 1e-14 * s
    E, N = A.indices.size, A.shape[0] // bs
    v = (s * A.data.astype(np.float64).reshape(-1)).astype(np.float32)
    d = sp.csr_matrix(A).diagonal().reshape(N, bs) * s
    hs.edge_attr = torch.from_numpy(v.reshape(E, bs * bs))
    hs.matrix_values = torch.from_numpy(v.reshape(E, bs, bs).copy())
    hs.diagonal = torch.from_numpy(d.astype(np.float32))
    hs.inv_diag = torch.from_numpy((1.0 / (d + 1e-7)).astype(np.float32))
    hs.rsqrt_diag = torch.from_numpy((1.0 / np.sqrt(d + 1e-7)).astype(np.float32))
    hs.matrix_scale = s
    return hs


def existing_pipeline(ws, hs):
    s = hs.to("cuda")
    A_sys = ws.system_matrix(s)
    solver = PreconditionedConjugateGradient(A_sys, device="cuda", preconditioner=ws.neural_precond, dtype=np.float64)
    L, _ = ws.inference_step(s)
    solver.set_spai(L, ws.epsilon, block_size=L.block_size)
    return A_sys, L, solver


def run(solver, rhs):
    x = torch.zeros_like(rhs)
    it, conv, _, hist = solver.solve(rhs.clone(), x, rtol=RTOL, max_iter=MAX_ITER * rhs.numel(), return_history=True)
    assert conv
    return it, hist, x.cpu().numpy()


def same_matrix(M1, M2, what):
    a, b = M1.to_scipy(), M2.to_scipy()
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices), what
    assert np.array_equal(a.data.view(np.int64), b.data.view(np.int64)), what


def same_run(r1, r2, what):
    assert r1[0] == r2[0], (what, r1[0], r2[0])
    assert np.array_equal(r1[1].view(np.int64), r2[1].view(np.int64)), what
    assert np.array_equal(r1[2].view(np.int64), r2[2].view(np.int64)), what


def masked(A, mask):
    M = sp.diags(mask)
    return sp.csr_matrix(M @ sp.csr_matrix(A) @ M + sp.diags(1.0 - mask))


CASES = [("bunny", SimpleInferenceWorkspace), ("poisson", SimpleInferenceWorkspace),
         ("poisson", ScaledInferenceWorkspace), ("elast", SimpleInferenceWorkspace)]
cases = pytest.mark.parametrize("name, cls", CASES, ids=[f"{n}-{c.__name__[:6].lower()}" for n, c in CASES])


def build(name, cls):
    A, mask, nf, bs = system(name)
    ws = workspace(cls, nf, bs)
    Ad = DeviceMatrix.from_scipy(A, dtype=np.float64, block_size=bs)
    b = torch.from_numpy(np.random.default_rng(1).standard_normal(A.shape[0]) * mask).cuda()
    return A, mask, nf, bs, ws, Ad, b, ws.live_solver(Ad, mask=mask, node_features=nf)


def relative_residual(M, x, b):
    x, b = x.cpu().numpy(), b.cpu().numpy()
    return float(np.linalg.norm(M @ x - b) / np.linalg.norm(b))


@cases
def test_construction_matches_the_existing_pipeline(gpu_ctx, name, cls):
    A, mask, nf, bs, ws, Ad, b, live = build(name, cls)
    assert live.solver.preconditioner == cls.neural_precond and live.A_sys.block_size == bs
    s = live.sample.matrix_scale
    A_ref, L_ref, solver_ref = existing_pipeline(ws, host_sample_with_scale(A, mask, nf, bs, s))
    same_matrix(live.A_sys, A_ref, "A_sys")
    same_matrix(live.L, L_ref, "L")
    same_run(run(live.solver, b * s), run(solver_ref, b * s), "construction")


@cases
def test_solve_solves_the_unscaled_masked_system(gpu_ctx, name, cls):
    """``live.solve(b, x)``: ``|mask(A) x - b| <= rtol |b| (1 + 1e-6)`` in fp64 on the host, with
    mask(A) = M A M + (I - M) of the caller's unscaled fp64 A.

    The solver's system is assembled from the sample's ``matrix_values``, which are fp32 as in the
    reference, so the forward alone solves mask(float32(scale * A)) x = scale * b.  On heat_bunny
    (condition 3.4e8) that leaves |mask(A) x - b| / |b| = 1.495e-02 after 1659 converged iterations,
    and an exact (sparse LU, fp64) host solve of the rounded system leaves 1.50e-02 too: the fp32
    rounding of the values (6e-8) times the condition number, not the solve.  ``solve`` therefore
    refines against the caller's matrix there.  The same host computation gives floors of 1.9e-8
    (poisson, condition 1.5e3) and 8.3e-8 (elasticity box, 1.4e2), below rtol: a system that needs
    no refinement gets the plain forward's bits."""
    A, mask, nf, bs, ws, Ad, b, live = build(name, cls)
    x = torch.zeros_like(b)
    it, conv = live.solve(b, x, rtol=RTOL, max_iter=MAX_ITER * b.numel())[:2]
    s = live.sample.matrix_scale
    res = relative_residual(masked(A, mask), x, b)
    info = live.last_solve
    print(f"{name} {cls.__name__}: {it} iterations {info['iters']}, {info['refinements']} refinements, "
          f"|mask(A) x - b| / |b| = {res:.3e} (device, per solve: {' '.join(f'{v:.2e}' for v in info['residuals'])})")
    assert conv and res <= RTOL * (1 + 1e-6)
    assert it == sum(info["iters"]) and len(info["iters"]) == info["refinements"] + 1
    assert info["relative_residual"] <= RTOL  # the device's own evaluation of the same residual
    forward = run(live.solver, b * s)
    if info["refinements"] == 0:
        assert forward[0] == it and np.array_equal(forward[2].view(np.int64), x.cpu().numpy().view(np.int64))
    else:  # the forward alone misses the bound, and each step gained on it
        assert relative_residual(masked(A, mask), torch.from_numpy(forward[2]), b) > RTOL
    x0 = torch.zeros_like(b)
    plain = live.solve(b, x0, rtol=RTOL, max_iter=MAX_ITER * b.numel(), refine=0, return_history=True)
    assert plain[0] == forward[0] and np.array_equal(plain[3].view(np.int64), forward[1].view(np.int64))
    with pytest.raises(ValueError, match="refine=0"):
        live.solve(b, x0, rtol=RTOL, return_history=True)


@cases
def test_refresh_matches_a_fresh_live_solver(gpu_ctx, name, cls):
    A, mask, nf, bs, ws, Ad, b, live = build(name, cls)
    s = live.sample.matrix_scale
    run(live.solver, b * s)  # the iteration graphs exist before the update
    A2 = second_values(A)
    key = ws.gnn._graph[0]
    ei_ptr = live.sample.edge_index.data_ptr()
    Ad.set_values(np.ascontiguousarray(A2.data, dtype=np.float64).reshape(-1))
    times = live.refresh()
    assert live.graphs_kept is True
    assert ws.gnn._graph[0] == key and live.sample.edge_index.data_ptr() == ei_ptr  # no new graph analysis
    assert set(times) == set(live.STEPS) | {"total"}
    assert all(t["wall"] >= 0 and t["device"] >= 0 for t in times.values())
    refreshed = run(live.solver, b * live.sample.matrix_scale)
    fresh = ws.live_solver(DeviceMatrix.from_scipy(A2, dtype=np.float64, block_size=bs), mask=mask, node_features=nf)
    assert fresh.sample.matrix_scale == live.sample.matrix_scale != s
    same_matrix(live.A_sys, fresh.A_sys, "A_sys after refresh")
    same_matrix(live.L, fresh.L, "L after refresh")
    same_run(refreshed, run(fresh.solver, b * fresh.sample.matrix_scale), "refresh")
