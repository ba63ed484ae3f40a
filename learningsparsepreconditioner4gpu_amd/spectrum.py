"""Extreme eigenvalues and condition number of the preconditioned system M⁻¹A, from the scalars of
one PCG solve (the quality measure of the reference's ``cond.py``, at any size).

The reference's ``cond.py:22-38`` forms ``M @ A`` densely on the host and takes its eigenvalues, which
stops at a few thousand unknowns.  Here the solver's own loop delivers the spectrum's ends: CG is the
Lanczos process on M⁻¹A, its ρ_k = r_k·z_k and π_k = p_k·q_k are the Lanczos coefficients
(``solve(..., return_coefficients=True)``), and the extreme eigenvalues of the tridiagonal T_m built
from them (``lspcg_cg_lanczos``) converge to λ_min and λ_max of M⁻¹A as the solve converges -- what
PETSc's ``KSPComputeExtremeSingularValues`` reads off its CG.  DESIGN.md "Condition number".

The estimate is only as good as the run is converged, so it carries its own evidence:
``lmin_bound`` / ``lmax_bound`` are the residual norms |T[m-2, m-1]·s_last| of the extreme Ritz pairs
of T_{m-1} -- some eigenvalue of M⁻¹A lies within that distance of the Ritz value -- plus the
rounding floor 8·eps·λ_max of the recorded scalars (the residual bound is exact arithmetic's; a
converged pair's goes to 1e-30 while T's entries carry a few eps each), and ``converged`` is the
solve's verdict.  The two parts are also reported on their own: ``lmin_residual`` /
``lmax_residual`` are the classical residual norms alone and ``rounding_floor`` the added term (in
fp32 it is about 1e-6·λ_max, which can exceed λ_min on an ill-conditioned system: read the residual
there).  A run cut short shows a large ``lmin_bound``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))


def lanczos_matrix(rho, pi) -> Tuple[np.ndarray, np.ndarray]:
    """``(diag, off)`` of the Lanczos tridiagonal T_m of M⁻¹A from the m recorded pairs
    (``lspcg_cg_lanczos``): diag[k] = π_k/ρ_k + (ρ_k/ρ_{k-1})·π_{k-1}/ρ_{k-1},
    off[k] = sqrt(ρ_{k+1}/ρ_k)·π_k/ρ_k.  A ρ or π that is not positive and finite (a breakdown, an
    operator that is not SPD) raises ``LspcgError`` with code ``ERR_ARG``."""
    rho, pi = _f64(rho), _f64(pi)
    if rho.size != pi.size:
        raise ValueError(f"rho has {rho.size} entries, pi has {pi.size}")
    m = rho.size
    coef = np.ascontiguousarray(np.stack([rho, pi], axis=1).reshape(-1)) if m else np.zeros(2)
    diag, off = np.empty(max(m, 1)), np.empty(max(m - 1, 1))
    _lib.call("lspcg_cg_lanczos", m, coef.ctypes.data_as(_lib.p_f64), diag.ctypes.data_as(_lib.p_f64),
              off.ctypes.data_as(_lib.p_f64))
    return diag[:m], off[: m - 1]


def extremes(diag, off) -> Tuple[float, float]:
    """``(lmin, lmax)`` of the symmetric tridiagonal (``lspcg_tridiag_extremes``: Sturm-count bisection
    of the Gershgorin interval, in double, down to adjacent doubles)."""
    diag, off = _f64(diag), _f64(off)
    if off.size != max(diag.size - 1, 0):
        raise ValueError(f"diag has {diag.size} entries, off has {off.size}")
    lo, hi = C.c_double(), C.c_double()
    offp = off if off.size else np.zeros(1)
    _lib.call("lspcg_tridiag_extremes", diag.size, diag.ctypes.data_as(_lib.p_f64), offp.ctypes.data_as(_lib.p_f64),
              C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def ritz_bounds(diag, off) -> Tuple[float, float]:
    """The classical Lanczos residual bounds of the extreme Ritz pairs (θ, s) of T_{m-1}, the leading
    block of T_m: |T[m-2, m-1]·s_last| for the smallest and the largest θ.  For each, an eigenvalue of
    M⁻¹A lies within that distance of θ.  ``inf`` for m < 2 (there is no T_{m-1})."""
    from scipy.linalg import eigh_tridiagonal

    diag, off = _f64(diag), _f64(off)
    m = diag.size
    if m < 2:
        return float("inf"), float("inf")
    d, e, beta = diag[: m - 1], off[: m - 2], abs(off[m - 2])
    if m == 2:
        return beta, beta
    out = []
    for j in (0, m - 2):
        _, s = eigh_tridiagonal(d, e, select="i", select_range=(j, j))
        out.append(float(beta * abs(s[-1, 0])))
    return out[0], out[1]


@dataclass
class SpectrumEstimate:
    lmin: float
    lmax: float
    cond: float
    iters: int
    converged: bool
    lmin_bound: float
    lmax_bound: float
    rho: np.ndarray
    pi: np.ndarray
    lmin_residual: float = 0.0   # the classical residual norm alone: lmin_bound = lmin_residual + rounding_floor
    lmax_residual: float = 0.0
    rounding_floor: float = 0.0  # 8·eps·λ_max of the type the scalars were rounded to


def estimate(rho, pi, converged: bool = True, eps: float = float(np.finfo(np.float64).eps)) -> SpectrumEstimate:
    """The estimate from recorded scalars alone (``condition_number`` without its solve).  ``eps``: the
    machine epsilon of the type the scalars were rounded to (the solver's dtype), for the bounds'
    rounding floor 8·eps·λ_max."""
    diag, off = lanczos_matrix(rho, pi)
    lmin, lmax = extremes(diag, off)
    floor = 8.0 * eps * abs(lmax)
    rmin, rmax = ritz_bounds(diag, off)
    return SpectrumEstimate(lmin=lmin, lmax=lmax, cond=lmax / lmin, iters=int(diag.size), converged=bool(converged),
                            lmin_bound=rmin + floor, lmax_bound=rmax + floor, rho=_f64(rho), pi=_f64(pi),
                            lmin_residual=rmin, lmax_residual=rmax, rounding_floor=floor)


def condition_number(solver, start=None, seed: int = 0, rtol: float = 1e-8, max_iter: int = 0) -> SpectrumEstimate:
    """κ(M⁻¹A) of a ``PreconditionedConjugateGradient`` (its preconditioner installed) from one solve
    of A x = start from x = 0 with ``return_coefficients=True``.

    ``start=None`` draws ``default_rng(seed).standard_normal(n)``.  The start must be random: Lanczos
    sees only the eigenvectors the start has a component in, and a constant vector (``rhs="mask"``)
    is orthogonal to most eigenvectors of a Laplacian and misses the extremes.  A run that stopped at
    ``max_iter`` still returns its estimate, with ``converged=False`` and the bounds to judge it by."""
    n = solver.n
    if start is None:
        start = np.random.default_rng(seed).standard_normal(n)
    dev, tdt = solver.ctx.torch_device, solver.torch_dtype
    b = torch.as_tensor(start).to(device=dev, dtype=tdt).contiguous().reshape(-1)
    x = torch.zeros_like(b)
    iters, conv, _, (rho, pi) = solver.solve(b, x, rtol, max_iter, return_coefficients=True)
    if iters < 1:
        raise ValueError("the solve completed no iteration (a zero start vector?): nothing to estimate from")
    return estimate(rho, pi, conv, eps=float(np.finfo(solver.dtype).eps))
