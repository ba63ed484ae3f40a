"""Helpers shared by the condition-number tests (CPU-side only)."""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla


def numpy_cg(A, b, apply_m=None, rtol=1e-8, max_iter=0):
    """scipy's cg loop in fp64 with np.dot, keeping ρ_k = r_k·z_k and π_k = p_k·q_k."""
    n = b.size
    max_iter = max_iter or n
    atol = rtol * np.linalg.norm(b)
    x, r = np.zeros(n), b.copy()
    rho, pi, p, rho_prev = [], [], None, None
    for k in range(max_iter):
        if np.linalg.norm(r) < atol:
            break
        z = apply_m(r) if apply_m is not None else r
        rho_k = float(np.dot(r, z))
        p = z.copy() if k == 0 else p * (rho_k / rho_prev) + z
        q = A @ p
        pi_k = float(np.dot(p, q))
        alpha = rho_k / pi_k
        x += alpha * p
        r = r - alpha * q
        rho_prev = rho_k
        rho.append(rho_k)
        pi.append(pi_k)
    return np.array(rho), np.array(pi)


def dense_extremes(A, C=None):
    """λ_min, λ_max of M·A with M = C Cᵀ: M·A is similar to the symmetric Cᵀ A C."""
    Ad = A.toarray()
    S = Ad if C is None else C.T @ Ad @ C
    w = sla.eigvalsh((S + S.T) / 2)
    return float(w[0]), float(w[-1])
