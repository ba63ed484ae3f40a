"""CPU: the host half of the condition-number estimate -- ``lspcg_cg_lanczos`` and
``lspcg_tridiag_extremes`` through ``spectrum.lanczos_matrix`` / ``spectrum.extremes`` -- on the
coefficients of an fp64 numpy CG written here, against scipy's tridiagonal eigenvalues and against
the dense spectrum of M·A.  No GPU: the two C functions never touch the device.

Systems (n = 576): the 24x24 five-point Poisson system, the same system under a random diagonal
scaling (κ = 1.1e4), and the scaled system with Jacobi and with an SPAI-like L Lᵀ + 3e-3·I."""
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

from learningsparsepreconditioner4gpu_amd import _lib
from learningsparsepreconditioner4gpu_amd import problems as P
from tests import _cases
from tests._spectrum import dense_extremes, numpy_cg
from tests.conftest import ROOT

ULP = np.finfo(np.float64).eps


def poisson():
    return sp.csr_matrix(P.poisson2d_grid(24, 24)[0]).astype(np.float64)


def scaled():
    A = poisson()
    s = np.exp(np.random.default_rng(5).uniform(-1.15, 1.15, A.shape[0]))
    return sp.csr_matrix(sp.diags(s) @ A @ sp.diags(s))


def cpu_cases():
    """name -> (A, apply_m or None, C with M = C Cᵀ or None)"""
    A0, A1 = poisson(), scaled()
    d = A1.diagonal()
    L = _cases.spai_like(A1, seed=1)
    LT = sp.csr_matrix(L.T)
    M = (L @ LT).toarray() + 3e-3 * np.eye(A1.shape[0])
    return {
        "poisson": (A0, None, None),
        "scaled": (A1, None, None),
        "scaled-jacobi": (A1, lambda r: r / d, np.diag(1.0 / np.sqrt(d))),
        "scaled-spai": (A1, lambda r: L @ (LT @ r) + 3e-3 * r, np.linalg.cholesky(M)),
    }


def start(n):
    return np.random.default_rng(0).standard_normal(n)


def against_scipy(rho, pi):
    from learningsparsepreconditioner4gpu_amd import spectrum

    diag, off = spectrum.lanczos_matrix(rho, pi)
    lmin, lmax = spectrum.extremes(diag, off)
    w = sla.eigvalsh_tridiagonal(diag, off) if diag.size > 1 else diag
    tol = 4 * ULP * abs(w[-1])
    print(f"m={diag.size} lmin {lmin!r} scipy {w[0]!r} lmax {lmax!r} scipy {w[-1]!r} tol {tol:.3e}")
    assert abs(lmin - w[0]) <= tol and abs(lmax - w[-1]) <= tol
    return diag, off


def test_lanczos_matrix_is_the_stated_one():
    from learningsparsepreconditioner4gpu_amd import spectrum

    rho, pi = np.array([2.0, 0.5, 0.125]), np.array([4.0, 3.0, 0.25])
    diag, off = spectrum.lanczos_matrix(rho, pi)
    assert np.array_equal(diag, [2.0, 3.0 / 0.5 + (0.5 / 2.0) * 2.0, 0.25 / 0.125 + (0.125 / 0.5) * 6.0])
    assert np.array_equal(off, [np.sqrt(0.5 / 2.0) * 2.0, np.sqrt(0.125 / 0.5) * 6.0])


@pytest.mark.parametrize("m", [1, 2, 77])
def test_extremes_match_scipy_on_poisson(m):
    A = poisson()
    rho, pi = numpy_cg(A, start(A.shape[0]), rtol=0.0, max_iter=m)
    assert rho.size == m
    against_scipy(rho, pi)


def test_extremes_match_scipy_on_clustered_spectrum():
    """Diagonal A with 5 distinct eigenvalues, run to 12 iterations: the Krylov space is exhausted
    after 5, so T has near-zero off-diagonals and repeated Ritz values."""
    lam = np.repeat([1.0, 2.0, 3.5, 7.0, 10.0], 10)
    rho, pi = numpy_cg(sp.diags(lam).tocsr(), start(lam.size), rtol=0.0, max_iter=12)
    assert rho.size == 12
    diag, off = against_scipy(rho, pi)
    assert np.min(np.abs(off)) < 1e-6
    from learningsparsepreconditioner4gpu_amd import spectrum

    lmin, lmax = spectrum.extremes(diag, off)
    assert abs(lmin - 1.0) <= 1e-12 and abs(lmax - 10.0) <= 1e-11


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
@pytest.mark.parametrize("which", ["rho", "pi"])
def test_breakdown_is_an_argument_error(which, bad):
    from learningsparsepreconditioner4gpu_amd import spectrum

    rho, pi = np.array([2.0, 0.5, 0.125]), np.array([4.0, 3.0, 0.25])
    (rho if which == "rho" else pi)[1] = bad
    with pytest.raises(_lib.LspcgError) as e:
        spectrum.lanczos_matrix(rho, pi)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.LspcgError) as e:
        spectrum.extremes([1.0, np.nan], [0.5])
    assert e.value.code == _lib.ERR_ARG


@pytest.mark.parametrize("name", ["poisson", "scaled", "scaled-jacobi", "scaled-spai"])
def test_estimate_matches_dense_spectrum(name):
    """λ_min and λ_max from T_m of a CG run to rtol 1e-8 against the dense spectrum of M·A:
    relative error <= 1e-10 (measured <= 2e-12)."""
    from learningsparsepreconditioner4gpu_amd import spectrum

    A, apply_m, C = cpu_cases()[name]
    rho, pi = numpy_cg(A, start(A.shape[0]), apply_m, rtol=1e-8)
    est = spectrum.estimate(rho, pi)
    lo, hi = dense_extremes(A, C)
    e_lo, e_hi = abs(est.lmin - lo) / lo, abs(est.lmax - hi) / hi
    print(f"{name}: m={rho.size} cond {hi / lo:.6e} est {est.cond:.6e} err lmin {e_lo:.2e} lmax {e_hi:.2e} "
          f"bounds {est.lmin_bound:.2e} {est.lmax_bound:.2e}")
    assert e_lo <= 1e-10 and e_hi <= 1e-10
    assert est.iters == rho.size and est.cond == est.lmax / est.lmin
    assert np.isfinite(est.lmin_bound) and np.isfinite(est.lmax_bound)


def test_truncated_run_is_visibly_worse():
    """Half the iterations: λ_min is off by orders of magnitude more, and lmin_bound says so."""
    from learningsparsepreconditioner4gpu_amd import spectrum

    A, _, _ = cpu_cases()["scaled"]
    rho, pi = numpy_cg(A, start(A.shape[0]), rtol=1e-8)
    full, half = spectrum.estimate(rho, pi), spectrum.estimate(rho[: rho.size // 2], pi[: rho.size // 2], converged=False)
    lo, _ = dense_extremes(A)
    print(f"full err {abs(full.lmin - lo) / lo:.2e} bound {full.lmin_bound:.2e}; "
          f"half err {abs(half.lmin - lo) / lo:.2e} bound {half.lmin_bound:.2e}")
    assert half.lmin > full.lmin and not half.converged
    assert half.lmin_bound > full.lmin_bound


def test_return_coefficients_is_unavailable_without_the_library(monkeypatch, tmp_path):
    """``solve(..., return_coefficients=True)`` on CPU tensors with no library to load raises
    ``LspcgUnavailable``, like ``solve``: it reaches the new entry point, never a host fallback.  (The
    solver object is made without its constructor, which would need the GPU.)"""
    import types

    import torch

    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", tmp_path / "absent.so")
    s = object.__new__(PreconditionedConjugateGradient)
    s.n, s.dtype, s.handle = 4, np.dtype(np.float64), None
    s.ctx = types.SimpleNamespace(torch_device=torch.device("cpu"))
    b = torch.ones(4, dtype=torch.float64)
    for kw in ({}, {"return_coefficients": True}):
        with pytest.raises(_lib.LspcgUnavailable):
            s.solve(b, torch.zeros_like(b), 1e-8, 0, **kw)


def test_cond_help_names_the_five_kinds():
    out = subprocess.run([sys.executable, "-m", "learningsparsepreconditioner4gpu_amd.cond", "--help"], cwd=ROOT,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    for kind in ("neural", "none", "diag", "ainv", "ichol"):
        assert kind in out.stdout
    assert "Kaporin" in out.stdout
