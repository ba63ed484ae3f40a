"""numpy restatement of the device FEM assembly (``lspcg_fem_*``): the same expressions in the same
order, so the device result can be pinned to the bit.

Per tet the expressions of ``problems.p1_laplacian_exact`` (edge vectors from vertex 0, the three
cross products, ``det`` summed left to right, ``g0 = -((g1 + g2) + g3)``) with ``vol = |det| / 6``;
per stored entry the sum of its contributions with ``np.add.at`` over contributions ordered by tet
(then by ``4 a + b``), which is sequential and therefore the kernel's order; the mass term of a
diagonal entry last.  The pattern holds every diagonal, used or not.
"""
import numpy as np
import scipy.sparse as sp


def tet_geometry(nodes, tets):
    """``(G [T,4,3], vol [T], det [T])``."""
    X = np.asarray(nodes, dtype=np.float64)[np.asarray(tets, dtype=np.int64)]
    a, b, c = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]
    cross = lambda u, v: np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                                   u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    bc, ca, ab = cross(b, c), cross(c, a), cross(a, b)
    det = (a[:, 0] * bc[:, 0] + a[:, 1] * bc[:, 1]) + a[:, 2] * bc[:, 2]
    g1, g2, g3 = bc / det[:, None], ca / det[:, None], ab / det[:, None]
    g0 = -((g1 + g2) + g3)
    return np.stack([g0, g1, g2, g3], 1), np.abs(det) / 6.0, det


def pattern(n, tets):
    """``(indptr, indices, slot [T,4,4])``: the canonical CSR of the 16 vertex pairs of every tet plus
    every diagonal, and the stored position of pair ``(a, b)`` of tet ``t``."""
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    r = np.repeat(tets, 4, axis=1).ravel()   # tets[t, a]
    c = np.tile(tets, (1, 4)).ravel()        # tets[t, b]
    keys = np.concatenate([r * n + c, np.arange(n, dtype=np.int64) * (n + 1)])
    uniq, inv = np.unique(keys, return_inverse=True)
    rows, cols = uniq // max(n, 1), uniq % max(n, 1)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    return np.cumsum(indptr).astype(np.int32), cols.astype(np.int32), inv[: r.size].reshape(-1, 4, 4)


def _diag_slots(indptr, indices):
    n = indptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    return np.flatnonzero(rows == indices)  # one per row, in row order


def lumped_mass(nodes, tets):
    _, vol, _ = tet_geometry(nodes, tets)
    m = np.zeros(np.asarray(nodes).shape[0])
    tets = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    # per vertex the order of its tets is what matters: (t, a) row-major is ascending t
    np.add.at(m, tets.ravel(), np.repeat(vol / 4.0, 4))
    return m


def heat(nodes, tets, kappa=None, density=0.0):
    """``K(kappa) + diag(density * lumped_mass)`` as scipy CSR (float64)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    n = nodes.shape[0]
    G, vol, _ = tet_geometry(nodes, tets)
    w = vol if kappa is None else vol * np.asarray(kappa, dtype=np.float64)
    K = ((G[:, :, None, 0] * G[:, None, :, 0] + G[:, :, None, 1] * G[:, None, :, 1])
         + G[:, :, None, 2] * G[:, None, :, 2]) * w[:, None, None]
    indptr, indices, slot = pattern(n, tets)
    vals = np.zeros(indices.size)
    np.add.at(vals, slot.ravel(), K.ravel())  # (t, a, b) row-major: ascending tet, then 4 a + b
    rho = np.broadcast_to(np.asarray(density, dtype=np.float64), (n,))
    d = _diag_slots(indptr, indices)
    vals[d] = vals[d] + rho * lumped_mass(nodes, tets)
    return sp.csr_matrix((vals, indices, indptr), shape=(n, n))


def elasticity(nodes, tets, young, poisson, mass_coef=0.0):
    """The 3x3-block linear-elastic operator as scipy BSR (float64, row-major blocks)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    n = nodes.shape[0]
    T = np.asarray(tets).reshape(-1, 4).shape[0]
    G, vol, _ = tet_geometry(nodes, tets)
    E = np.broadcast_to(np.asarray(young, dtype=np.float64), (T,))
    nu = np.broadcast_to(np.asarray(poisson, dtype=np.float64), (T,))
    lam = ((E * nu) / ((1.0 + nu) * (1.0 - 2.0 * nu)))[:, None, None, None, None]
    mu = (E / (2.0 * (1.0 + nu)))[:, None, None, None, None]
    ga, gb = G[:, :, None, :], G[:, None, :, :]  # [T,4,1,3], [T,1,4,3]
    gg = (ga[..., 0] * gb[..., 0] + ga[..., 1] * gb[..., 1]) + ga[..., 2] * gb[..., 2]  # [T,4,4]
    gai_gbj = ga[:, :, :, :, None] * gb[:, :, :, None, :]   # [t,a,b,i,j] = g_a,i g_b,j
    gaj_gbi = ga[:, :, :, None, :] * gb[:, :, :, :, None]   # [t,a,b,i,j] = g_a,j g_b,i
    Kt = (lam * gai_gbj + mu * (gaj_gbi + np.eye(3)[None, None, None] * gg[..., None, None])) \
        * vol[:, None, None, None, None]
    indptr, indices, slot = pattern(n, tets)
    vals = np.zeros((indices.size, 3, 3))
    np.add.at(vals, slot.ravel(), Kt.reshape(-1, 3, 3))
    d = _diag_slots(indptr, indices)
    mm = mass_coef * lumped_mass(nodes, tets)
    for q in range(3):
        vals[d, q, q] = vals[d, q, q] + mm
    return sp.bsr_matrix((vals, indices, indptr), shape=(3 * n, 3 * n), blocksize=(3, 3))
