"""GPU: the PCG loop records its scalars ρ_k = r_k·z_k and π_k = p_k·q_k (``return_coefficients``),
and ``spectrum.condition_number`` turns them into λ_min, λ_max and κ of M⁻¹A.

Systems:
  a  Poisson 24x24, n = 576: the one-workgroup solve
  b  the same matrix with LSPCG_SMALL_N=0: the multi-kernel schedules
  c  kuhn_laplacian(17), n = 4913: above the one-workgroup bound without a switch
  d  elasticity_box(5, 4, 4), block size 3, ``spai_like(E, seed=1, scale=0.02)``, ε = 1e-3
The scalar systems' SPAI factors are ``_cases.spai_like(A, seed=1)``, ε = 1e-3.

Bounds: recorded scalars against the oracle's exact-dot trajectory to 1e-12, the constant
tests/test_gpu_traj.py holds ‖r_k‖ to against the same oracle.  ρ_0 and π_0 against ``lspcg_dot`` of
the device vectors to 4 ulp, not to the bit: both sides are compensated sums, each within an ulp or
two of the exact dot, summed in different trees (measured: equal bits in every case).  The estimate against the dense spectrum to max(1e-9, 10·e_host),
e_host the error of the fp64 numpy restatement of the same run (asserted <= 1e-10 first); fp32
solvers to the project's fp32 bound 1e-5.

Which kinds are estimate cases on system d (κ = 1.2e5 at n = 240) follows from that input condition,
measured on the host restatement alone: with max_iter = 4 n (CG in floating point needs 250 > n
iterations there) `none` and `ext_spai` reach e_host = 8.5e-12 and 9.4e-12 at rtol 1e-8; `diagonal`
and `ext_spai_scaled` reach rtol 1e-8 after 156 iterations with λ_min still 4.6e-9 and 4.8e-9 off
(a Ritz value converges like bound²/gap, and their bound is 7e-7 there), so they do not meet
e_host <= 1e-10 at that rtol; at rtol 1e-10 (165 iterations) they reach 1.3e-12 and 1.9e-12, and
that is the rtol their estimate cases run at, with the issue's bound and input condition unchanged.
The same condition on systems a and b:
`ainv` and `ic` converge in 62 and 38 iterations, too few for Lanczos to resolve λ_max -- the host
restatement is 2.4e-7 and 1.6e-4 off there (1.1e-9 and 1.6e-4 even at rtol 1e-12), and its
lmax_bound says so (2.7e-4, 6.6e-4).  They cannot meet the input condition at any rtol, so their
estimates are held to the host restatement's estimate of the same run instead
(test_estimate_of_a_short_run): the recorded scalars agree with the host's to 1e-12 (case 2's
bound), so T's entries agree to about 5e-12 relative, ‖δT‖ <= 3e-11·λ_max, and by Weyl's inequality
the extremes agree to 3e-11·κ relative; the bounds must still cover a tenth of the actual error."""
import csv
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import torch

from learningsparsepreconditioner4gpu_amd import problems as P
from oracle import linalg as O
from tests import _cases
from tests._spectrum import dense_extremes, numpy_cg

pytestmark = pytest.mark.gpu

EPS = 1e-3
KINDS = ("none", "diagonal", "ext_spai", "ext_spai_scaled", "ainv", "ic")
ULP = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def system(name):
    """(A, L, block size) of system a / b / c / d / p12 (a 12x12 Poisson grid, for the batch)."""
    if name in ("a", "b"):
        A = sp.csr_matrix(P.poisson2d_grid(24, 24)[0]).astype(np.float64)
    elif name == "p12":
        A = sp.csr_matrix(P.poisson2d_grid(12, 12)[0]).astype(np.float64)
    elif name == "c":
        A = sp.csr_matrix(P.kuhn_laplacian(17)).astype(np.float64)
    else:
        A = sp.csr_matrix(P.elasticity_box(5, 4, 4)[0]).astype(np.float64)
        A.sort_indices()
        return A, _cases.spai_like(A, seed=1, scale=0.02), 3
    A.sort_indices()
    return A, _cases.spai_like(A, seed=1), 1


@functools.lru_cache(maxsize=None)
def start(n, seed=0):
    return np.random.default_rng(seed).standard_normal(n)


def make_solver(name, kind, dtype=np.float64, dot_order="compensated", monkeypatch=None):
    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient

    if name == "b":
        monkeypatch.setenv("LSPCG_SMALL_N", "0")
    A, L, bs = system(name)
    s = PreconditionedConjugateGradient(A, device="cuda", preconditioner=kind, dtype=dtype, block_size=bs,
                                        dot_order=dot_order)
    if kind.startswith("ext_spai"):
        s.set_spai(L, EPS, block_size=bs)
    return s


def device_start(s):
    return torch.as_tensor(start(s.n)).to(device=s.ctx.torch_device, dtype=s.torch_dtype)


def host_operator(name, kind, solver=None):
    """(apply_m or None, C with M = C Cᵀ or None) on the host; ainv / ic take the factor the device built."""
    A, L, _ = system(name)
    n = A.shape[0]
    d = A.diagonal()
    if kind == "none":
        return None, None
    if kind == "diagonal":
        return O.diagonal_operator(A), np.diag(1.0 / np.sqrt(d))
    if kind == "ext_spai":
        return O.spai_operator(L, EPS), np.linalg.cholesky((L @ L.T).toarray() + EPS * np.eye(n))
    if kind == "ext_spai_scaled":
        M = (L @ sp.diags(1.0 / d) @ L.T).toarray() + EPS * np.diag(1.0 / d)
        return O.spai_scaled_operator(A, L, EPS), np.linalg.cholesky((M + M.T) / 2)
    if kind == "ainv":
        Z = sp.csr_matrix(solver.A.ainv0()[0].to_scipy())
        return O.spai_operator(Z, 0.0), Z.toarray()
    Lc = solver.A.ic0()[0].to_scipy().toarray()  # M = (Lc Lcᵀ)⁻¹ = C Cᵀ with C = Lc⁻ᵀ
    return (lambda r: sla.solve_triangular(Lc, sla.solve_triangular(Lc, r, lower=True), lower=True, trans="T"),
            sla.solve_triangular(Lc, np.eye(n), lower=True).T)


# ---- 1. recording changes nothing -----------------------------------------------------------
BLOCK3_KINDS = ("none", "diagonal", "ext_spai", "ext_spai_scaled")  # AINV(0) and IC(0) factor scalar CSR only
SAME_BITS = ([(n, k, np.float64, "compensated") for n in "abc" for k in KINDS]
             + [("d", k, np.float64, "compensated") for k in BLOCK3_KINDS]
             + [(n, k, np.float32, "compensated") for n in "ac" for k in KINDS]
             + [("c", k, np.float64, "openblas") for k in ("none", "ext_spai")])


@pytest.mark.parametrize("name,kind,dtype,dot_order", SAME_BITS,
                         ids=[f"{n}-{k}-{np.dtype(d).name}-{o}" for n, k, d, o in SAME_BITS])
def test_recording_leaves_the_solve_bit_identical(gpu_ctx, monkeypatch, name, kind, dtype, dot_order):
    s = make_solver(name, kind, dtype, dot_order, monkeypatch)
    b = device_start(s)
    rtol = 1e-8 if dtype == np.float64 else 1e-5
    x0, x1 = torch.zeros_like(b), torch.zeros_like(b)
    it0, c0, _, h0 = s.solve(b, x0, rtol, 0, return_history=True)
    it1, c1, _, h1, (rho, pi) = s.solve(b, x1, rtol, 0, return_history=True, return_coefficients=True)
    x2 = torch.zeros_like(b)
    it2, c2, _, h2 = s.solve(b, x2, rtol, 0, return_history=True)  # and the null case after a recording solve
    print(f"{name} {kind} {np.dtype(dtype).name} {dot_order}: iters {it0} {it1} {it2} converged {c0}")
    assert it0 == it1 == it2 and c0 == c1 == c2 and it0 > 0
    assert torch.equal(x0, x1) and torch.equal(x0, x2)
    assert np.array_equal(h0, h1, equal_nan=True) and np.array_equal(h0, h2, equal_nan=True)
    assert len(rho) == it1 and len(pi) == it1
    assert np.all(np.isfinite(rho)) and np.all(np.isfinite(pi)) and np.all(rho > 0) and np.all(pi > 0)


def test_recording_on_a_reordered_solver(gpu_ctx, monkeypatch):
    """LSPCG_REORDER=1: the loop runs on P A Pᵀ.  The same bits with and without recording, and the
    scalars of the unpermuted solver up to the dots' summation order (case 2's bound)."""
    plain = make_solver("c", "ext_spai")
    monkeypatch.setenv("LSPCG_REORDER", "1")
    s = make_solver("c", "ext_spai")
    assert s.reorder_info["applied"] and not plain.reorder_info["applied"]
    b = device_start(s)
    x0, x1 = torch.zeros_like(b), torch.zeros_like(b)
    it0, _, _, h0 = s.solve(b, x0, 1e-8, 0, return_history=True)
    it1, _, _, h1, (rho, pi) = s.solve(b, x1, 1e-8, 0, return_history=True, return_coefficients=True)
    assert it0 == it1 and torch.equal(x0, x1) and np.array_equal(h0, h1)
    it, _, _, (prho, ppi) = plain.solve(b, torch.zeros_like(b), 1e-8, 0, return_coefficients=True)
    assert it == it1 and len(rho) == it1
    e = max(np.max(np.abs(rho - prho) / prho), np.max(np.abs(pi - ppi) / ppi))
    print(f"reordered c ext_spai: {it1} iterations, scalars within {e:.2e} of the unpermuted solver's")
    assert e <= 1e-12


# ---- 2. the scalars are the recurrence's ------------------------------------------------------
FIRST_PAIR = [(n, k) for n in "abc" for k in KINDS] + [("d", k) for k in BLOCK3_KINDS]


@pytest.mark.parametrize("name,kind", FIRST_PAIR, ids=[f"{n}-{k}" for n, k in FIRST_PAIR])
def test_first_pair_is_the_device_dots(gpu_ctx, monkeypatch, name, kind):
    """max_iter = 1 from x0 = 0: r_0 = b, p_0 = z_0 = M⁻¹ b, q_0 = A p_0, recomputed with lspcg_spmv /
    lspcg_trsv / lspcg_dot on device vectors (for `none` from b alone)."""
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix, dot

    s = make_solver(name, kind, monkeypatch=monkeypatch)
    b = device_start(s)
    x = torch.zeros_like(b)
    it, _, _, (rho, pi) = s.solve(b, x, 1e-8, 1, return_coefficients=True)
    assert it == 1 and len(rho) == 1
    A, L, bs = system(name)
    if kind == "none":
        z = b
    elif kind == "diagonal":
        z = b / s.A.diagonal()
    elif kind == "ic":
        Lc = s.A.ic0()[0]
        z = Lc.T.trsv(Lc.trsv(b, lower=True), lower=False)
    else:
        Ld = s.A.ainv0()[0] if kind == "ainv" else DeviceMatrix.from_scipy(L, dtype=np.float64, block_size=bs, ctx=s.ctx)
        eps = 0.0 if kind == "ainv" else EPS
        t = Ld.T.matvec(b)
        if kind == "ext_spai_scaled":
            d = s.A.diagonal()
            z = Ld.matvec(t / d) + (eps * b) / d
        else:
            z = Ld.matvec(t) + eps * b
    want_rho, want_pi = dot(b, z), dot(z, s.A.matvec(z))
    print(f"{name} {kind}: rho {rho[0]!r} vs {want_rho!r}, pi {pi[0]!r} vs {want_pi!r}")
    assert abs(rho[0] - want_rho) <= 4 * ULP * abs(want_rho)
    assert abs(pi[0] - want_pi) <= 4 * ULP * abs(want_pi)


def oracle_scalars(A, b, psolve, rtol):
    """oracle.linalg.pcg's loop with the exact dot, keeping ρ_k and π_k."""
    d = O.exact_dot
    atol = rtol * np.sqrt(d(b, b))
    x, r = np.zeros_like(b), b.copy()
    rho, pi, p, rho_prev = [], [], None, None
    for k in range(b.size):
        if np.sqrt(d(r, r)) < atol:
            break
        z = psolve(r) if psolve is not None else r
        rho_cur = d(r, z)
        if k > 0:
            p *= rho_cur / rho_prev
            p += z
        else:
            p = z.copy()
        q = A @ p
        pq = d(p, q)
        alpha = rho_cur / pq
        x += alpha * p
        r -= alpha * q
        rho_prev = rho_cur
        rho.append(rho_cur)
        pi.append(pq)
    return np.array(rho), np.array(pi)


@functools.lru_cache(maxsize=None)
def oracle_run(name, kind):
    A, _, _ = system(name)
    psolve = host_operator(name, kind)[0]
    b = start(A.shape[0])
    rho, pi = oracle_scalars(A, b, psolve, 1e-8)
    assert len(rho) == O.pcg(A, b, psolve, rtol=1e-8, dot="exact")[0]  # the restatement is the oracle's loop
    return rho, pi


@pytest.mark.parametrize("kind", ["none", "diagonal", "ext_spai", "ext_spai_scaled"])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_scalars_follow_the_oracle_trajectory(gpu_ctx, monkeypatch, name, kind):
    s = make_solver(name, kind, monkeypatch=monkeypatch)
    b = device_start(s)
    it, conv, _, (rho, pi) = s.solve(b, torch.zeros_like(b), 1e-8, 0, return_coefficients=True)
    want_rho, want_pi = oracle_run("a" if name == "b" else name, kind)
    assert conv and it == len(want_rho) and len(rho) == it and len(pi) == it
    e_rho, e_pi = np.max(np.abs(rho - want_rho) / want_rho), np.max(np.abs(pi - want_pi) / want_pi)
    print(f"{name} {kind}: {it} iterations, rho within {e_rho:.2e}, pi within {e_pi:.2e}")
    assert e_rho <= 1e-12 and e_pi <= 1e-12


# ---- 3. the estimate --------------------------------------------------------------------------
ESTIMATE = ([(n, k, np.float64, 1e-8) for n in "ab" for k in ("none", "diagonal", "ext_spai", "ext_spai_scaled")]
            + [("d", "none", np.float64, 1e-8), ("d", "ext_spai", np.float64, 1e-8)]
            + [("d", "diagonal", np.float64, 1e-10), ("d", "ext_spai_scaled", np.float64, 1e-10)]  # module docstring
            + [("a", k, np.float32, 1e-8) for k in ("none", "diagonal", "ext_spai")])


@pytest.mark.parametrize("name,kind,dtype,rtol", ESTIMATE,
                         ids=[f"{n}-{k}-{np.dtype(d).name}-{r:g}" for n, k, d, r in ESTIMATE])
def test_estimate_matches_dense_spectrum(gpu_ctx, monkeypatch, name, kind, dtype, rtol):
    from learningsparsepreconditioner4gpu_amd import spectrum

    s = make_solver(name, kind, dtype, monkeypatch=monkeypatch)
    A, _, _ = system(name)
    apply_m, C = host_operator(name, kind, s)
    lo, hi = dense_extremes(A, C)
    n = A.shape[0]
    h_rho, h_pi = numpy_cg(A, start(n), apply_m, rtol=rtol, max_iter=4 * n)
    host = spectrum.estimate(h_rho, h_pi)
    e_host = max(abs(host.lmin - lo) / lo, abs(host.lmax - hi) / hi)
    est = spectrum.condition_number(s, rtol=rtol, max_iter=4 * n)
    e_lo, e_hi = abs(est.lmin - lo) / lo, abs(est.lmax - hi) / hi
    bound = max(1e-9 if dtype == np.float64 else 1e-5, 10 * e_host)
    print(f"{name} {kind} {np.dtype(dtype).name}: cond {hi / lo:.6e} est {est.cond:.6e} iters {est.iters} (host {host.iters}) "
          f"converged {est.converged} e_host {e_host:.2e} err {e_lo:.2e} {e_hi:.2e} bound {bound:.1e} "
          f"ritz bounds {est.lmin_bound:.2e} {est.lmax_bound:.2e}")
    assert e_host <= 1e-10
    assert e_lo <= bound and e_hi <= bound
    for b, err in ((est.lmin_bound, abs(est.lmin - lo)), (est.lmax_bound, abs(est.lmax - hi))):
        assert np.isfinite(b) and b >= 0 and b >= err / 10
    assert est.cond == est.lmax / est.lmin and len(est.rho) == est.iters == len(est.pi)
    assert est.lmin_bound == est.lmin_residual + est.rounding_floor and est.lmax_bound == est.lmax_residual + est.rounding_floor
    assert est.rounding_floor == 8 * float(np.finfo(dtype).eps) * est.lmax


@pytest.mark.parametrize("kind", ["ainv", "ic"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_estimate_of_a_short_run(gpu_ctx, monkeypatch, name, kind):
    """ainv / ic on the Poisson system (module docstring): against the host restatement's estimate of
    the same run to 3e-11·κ, and the bounds against the actual error from the dense spectrum."""
    from learningsparsepreconditioner4gpu_amd import spectrum

    s = make_solver(name, kind, monkeypatch=monkeypatch)
    A, _, _ = system(name)
    apply_m, C = host_operator(name, kind, s)
    lo, hi = dense_extremes(A, C)
    h_rho, h_pi = numpy_cg(A, start(A.shape[0]), apply_m, rtol=1e-8)
    host = spectrum.estimate(h_rho, h_pi)
    est = spectrum.condition_number(s, rtol=1e-8)
    tol = 3e-11 * hi / lo
    d_lo, d_hi = abs(est.lmin - host.lmin) / host.lmin, abs(est.lmax - host.lmax) / host.lmax
    print(f"{name} {kind}: cond {hi / lo:.6e} est {est.cond:.6e} host {host.cond:.6e} iters {est.iters} (host {host.iters}) "
          f"vs host {d_lo:.2e} {d_hi:.2e} tol {tol:.1e}; vs dense {abs(est.lmin - lo) / lo:.2e} {abs(est.lmax - hi) / hi:.2e} "
          f"ritz bounds {est.lmin_bound:.2e} {est.lmax_bound:.2e}")
    assert est.converged and est.iters == host.iters
    assert d_lo <= tol and d_hi <= tol
    assert lo * (1 - 1e-9) <= est.lmin and est.lmax <= hi * (1 + 1e-9)  # Ritz values lie inside the spectrum
    for b, err in ((est.lmin_bound, abs(est.lmin - lo)), (est.lmax_bound, abs(est.lmax - hi))):
        assert np.isfinite(b) and b >= 0 and b >= err / 10


# ---- 4. a truncated run says so ---------------------------------------------------------------
def test_truncated_run_says_so(gpu_ctx):
    from learningsparsepreconditioner4gpu_amd import spectrum

    s = make_solver("c", "none")
    full = spectrum.condition_number(s, rtol=1e-8)
    cut = spectrum.condition_number(s, rtol=1e-8, max_iter=full.iters // 4)
    print(f"full: {full.iters} iterations lmin {full.lmin!r} bound {full.lmin_bound:.2e}; "
          f"cut: {cut.iters} lmin {cut.lmin!r} bound {cut.lmin_bound:.2e}")
    assert full.converged is True and cut.converged is False and cut.iters == full.iters // 4
    assert cut.lmin > full.lmin
    assert cut.lmin_bound >= 100 * full.lmin_bound


# ---- 5. batch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [("a", "c", "p12"), ("a", "p12")], ids=["lockstep", "one-workgroup"])
@pytest.mark.parametrize("kind", ["none", "ext_spai"])
def test_batch_records_every_system(gpu_ctx, kind, window):
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient

    As = [system(n)[0] for n in window]
    Ls = [system(n)[1] for n in window] if kind == "ext_spai" else None
    B = BatchedConjugateGradient(As, Ls, EPS if Ls else 0.0, preconditioner=kind)
    dev = B.ctx.torch_device
    bs = [torch.as_tensor(start(A.shape[0])).to(dev) for A in As]
    x0 = [torch.zeros_like(b) for b in bs]
    x1 = [torch.zeros_like(b) for b in bs]
    r0, _ = B.solve(bs, x0, 1e-8, 0)
    r1, _ = B.solve(bs, x1, 1e-8, 0, return_coefficients=True)
    for j, n in enumerate(window):
        single = make_solver(n, kind)
        it, _, _, (rho, pi) = single.solve(bs[j], torch.zeros_like(bs[j]), 1e-8, 0, return_coefficients=True)
        it1, conv1, (brho, bpi) = r1[j]
        assert (it1, conv1) == r0[j] and torch.equal(x0[j], x1[j])
        assert it1 == it and len(brho) == it1 and len(bpi) == it1
        e = max(np.max(np.abs(brho - rho) / rho), np.max(np.abs(bpi - pi) / pi))
        print(f"{kind} {window} system {n}: {it1} iterations, scalars within {e:.2e} of the single solver's")
        assert e <= 1e-12
    assert len({r[0] for r in r1}) == len(window)  # every system its own length


# ---- 6. ordering ------------------------------------------------------------------------------
def test_ordering_on_the_kuhn_laplacian(gpu_ctx):
    """Jacobi does not worsen the Kuhn Laplacian (its diagonal differs only at the boundary).  The
    dense confirmation runs on kuhn_laplacian(8), n = 512: the family has no member of n = 576 (the
    dense spectrum of system c itself, n = 4913, gives 134,294 for none and 132,862 for diagonal)."""
    from learningsparsepreconditioner4gpu_amd import spectrum

    A8 = sp.csr_matrix(P.kuhn_laplacian(8))
    lo, hi = dense_extremes(A8)
    dlo, dhi = dense_extremes(A8, np.diag(1.0 / np.sqrt(A8.diagonal())))
    assert dhi / dlo <= hi / lo
    cond = {k: spectrum.condition_number(make_solver("c", k), rtol=1e-8).cond for k in ("none", "diagonal", "ext_spai")}
    print(cond)
    assert np.isfinite(cond["ext_spai"]) and cond["ext_spai"] >= 1
    assert cond["diagonal"] <= cond["none"]


# ---- 7. the command line ------------------------------------------------------------------------
def test_cond_cli_writes_both_tables(gpu_ctx, tmp_path):
    from learningsparsepreconditioner4gpu_amd import cond

    cond.main(["--dataset", "heat_batch8", "--out-dir", str(tmp_path), "--exp-name", "t", "--max-iter", "4000"])
    lines = (tmp_path / "cond_cond_t.csv").read_text().splitlines()
    assert lines[0] == "neural,none,diag,ainv,ichol"
    rows = [[float(v) for v in ln.split(",")] for ln in lines[1:]]
    assert len(rows) == 8 and all(len(r) == 5 for r in rows)
    assert all(np.isfinite(v) and v >= 1 for r in rows for v in r)
    with open(tmp_path / "cond_detail_t.csv") as f:
        detail = list(csv.DictReader(f))
    assert len(detail) == 40
    assert list(detail[0]) == ["index", "kind", "n", "iters", "converged", "lmin", "lmax", "lmin_bound", "lmax_bound"]


# ---- 8. training --------------------------------------------------------------------------------
def test_fit_logs_the_condition_number_on_request(gpu_ctx):
    from learningsparsepreconditioner4gpu_amd.infer import synthetic_dataset
    from learningsparsepreconditioner4gpu_amd.workspace import SimpleInferenceWorkspace

    samples = synthetic_dataset("heat_batch8", is_inference=False)
    s0 = samples[0]

    def run(**kw):
        ws = SimpleInferenceWorkspace(node_features=s0.x.shape[1], edge_features=s0.edge_attr.shape[1], seed=0)
        return ws.fit(samples, max_epochs=2, check_val_every_n_epoch=1, **kw)

    rows = run(val_cond=True)
    assert len(rows) == 2
    for r in rows:
        assert np.isfinite(r["Val/cuda_neural_cond"]) and r["Val/cuda_neural_cond"] >= 1
    assert all("Val/cuda_neural_cond" not in r for r in run())
