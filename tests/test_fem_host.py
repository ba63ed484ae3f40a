"""CPU: the host side of fem.TetMesh -- argument checks made before any native call -- and the numpy
restatement of the device assembly (tests/_fem_ref.py) against the package's existing host routes.

The restatement is what tests/test_gpu_fem.py pins the device result to, bit for bit; here it is
itself held to the project's fp64 bound, 1e-12 of max |A|, against problems.p1_stiffness +
lumped_mass and against elasticity_box.  Measured on a Kuhn 5x4x3 grid, delaunay_tets(200) and
delaunay_tets(2000) with random kappa: within 3.9e-16 / 9.5e-16 / 3.5e-15 of p1_stiffness + the mass
term, within 3.5e-16 of lumped_mass, 4.4e-16 of elasticity_box, exactly symmetric, the host route's
pattern (570 / 2387 / 28662 entries) -- more than two orders of magnitude inside the bound.
"""
import functools
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from learningsparsepreconditioner4gpu_amd import _lib, fem
from learningsparsepreconditioner4gpu_amd import problems as P
from tests import _fem_ref as R

BOUND = 1e-12  # of max |A|: the project's fp64 bound


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "kuhn":
        nodes, tets = P.kuhn_tets(5, 4, 3)
    else:
        nodes, tets = P.delaunay_tets(int(name[8:]))
    nodes, tets = np.ascontiguousarray(nodes, dtype=np.float64), np.ascontiguousarray(tets, dtype=np.int64)
    kappa = np.random.default_rng(5).uniform(0.01, 1.0, size=tets.shape[0])
    for a in (nodes, tets, kappa):
        a.setflags(write=False)
    return nodes, tets, kappa


MESHES = [("kuhn", 570), ("delaunay200", 2387), ("delaunay2000", 28662)]


def rel(A, B):
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)
    return float(abs(A - B).max()) / float(abs(B).max())


@pytest.mark.parametrize("name, nnz", MESHES)
def test_restatement_matches_the_host_routes(name, nnz):
    nodes, tets, kappa = mesh(name)
    n = nodes.shape[0]
    rho = np.random.default_rng(6).uniform(1e-4, 5e-4, size=n)
    A = R.heat(nodes, tets, kappa, rho)
    K = P.p1_stiffness(nodes, tets, kappa)
    want = sp.csr_matrix(K + sp.diags(P.lumped_mass(nodes, tets) * rho))
    e_heat = rel(A, want)
    e_lap = rel(R.heat(nodes, tets, kappa), K)
    m, m_ref = R.lumped_mass(nodes, tets), P.lumped_mass(nodes, tets)
    e_mass = float(np.abs(m - m_ref).max() / np.abs(m_ref).max())
    print(f"{name}: heat {e_heat:.2e}, laplacian {e_lap:.2e}, mass {e_mass:.2e}, nnz {A.nnz}")
    assert e_heat <= BOUND and e_lap <= BOUND and e_mass <= BOUND
    # the pattern: canonical, every diagonal stored, the entries of the host route
    assert A.nnz == nnz and A.indptr.dtype == np.int32 and A.indices.dtype == np.int32
    assert A.has_canonical_format
    Kc = sp.csr_matrix(K)
    Kc.sort_indices()
    assert np.array_equal(A.indptr, Kc.indptr) and np.array_equal(A.indices, Kc.indices)
    # exactly symmetric
    At = sp.csr_matrix(A.T)
    At.sort_indices()
    assert np.array_equal(At.indices, A.indices) and np.array_equal(At.data, A.data)


@pytest.mark.parametrize("name, nnz", MESHES)
def test_restatement_under_a_permutation_of_the_tets(name, nnz):
    nodes, tets, kappa = mesh(name)
    p = np.random.default_rng(7).permutation(tets.shape[0])
    A, B = R.heat(nodes, tets, kappa, 2e-4), R.heat(nodes, tets[p], kappa[p], 2e-4)
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    assert rel(B, A) <= BOUND


def test_restatement_matches_elasticity_box():
    nx, ny, nz, E, nu, density, dt = 4, 3, 3, 3e6, 0.4, 1.0, 0.01
    want, _, nodes = P.elasticity_box(nx, ny, nz, E=E, nu=nu, density=density, dt=dt)
    _, tets = P.kuhn_tets(nx, ny, nz)
    A = R.elasticity(nodes, tets, E, nu, density / dt ** 2)
    assert A.blocksize == (3, 3) and A.shape == want.shape
    e = rel(A, want)
    print(f"elasticity box {nx}x{ny}x{nz}: {e:.2e}")
    assert e <= BOUND
    # symmetric in bits: block (i, j)[p][q] == block (j, i)[q][p]
    C = sp.csr_matrix(A)
    Ct = sp.csr_matrix(C.T)
    assert (C != Ct).nnz == 0


def test_restatement_edge_cases():
    # an unused vertex owns a stored 0 diagonal; one negatively oriented tet gives the same volume
    nodes = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5], [1, 1, 1]], dtype=np.float64)
    tets = np.array([[0, 1, 2, 3], [1, 2, 3, 5]])
    assert R.tet_geometry(nodes, tets)[2][0] > 0 > R.tet_geometry(nodes, tets[:, [0, 1, 3, 2]])[2][0]
    A = R.heat(nodes, tets, None, 1.0)
    assert A.indptr[5] - A.indptr[4] == 1 and A.indices[A.indptr[4]] == 4 and A.data[A.indptr[4]] == 0.0
    assert rel(A, P.p1_stiffness(nodes, tets) + sp.diags(P.lumped_mass(nodes, tets))) <= BOUND
    # T = 0: the diagonal only; N = 0: empty
    Z = R.heat(nodes, np.zeros((0, 4), dtype=np.int64), None, 1.0)
    assert Z.nnz == 6 and np.array_equal(Z.indices, np.arange(6)) and not Z.data.any()
    Z = R.heat(np.zeros((0, 3)), np.zeros((0, 4), dtype=np.int64))
    assert Z.shape == (0, 0) and Z.nnz == 0


# ---- fem.TetMesh: argument checks reach no native call ---------------------------------------

@pytest.fixture
def no_native(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError("native call before the arguments were checked")

    monkeypatch.setattr(_lib, "call", no_call)
    return types.SimpleNamespace(torch_device=torch.device("cpu"), handle=None)


@pytest.fixture
def stub(no_native):
    """A mesh without a native handle (no GPU here): N = 5, T = 2, on the CPU 'device'."""
    m = fem.TetMesh.__new__(fem.TetMesh)
    m.ctx, m.handle = no_native, None
    m.num_nodes, m.num_tets, m.nnz = 5, 2, 23
    return m


def test_construction_checks_arguments_first(no_native):
    nodes, tets = np.zeros((5, 3)), np.zeros((2, 4), dtype=np.int64)
    with pytest.raises(TypeError):
        fem.TetMesh([[0.0, 0.0, 0.0]], tets, ctx=no_native)  # a list
    with pytest.raises(TypeError):
        fem.TetMesh(nodes.astype(np.float32), tets, ctx=no_native)
    with pytest.raises(ValueError, match="expected"):
        fem.TetMesh(np.zeros((5, 2)), tets, ctx=no_native)
    with pytest.raises(ValueError, match="expected"):
        fem.TetMesh(np.zeros(15), tets, ctx=no_native)
    with pytest.raises(TypeError):
        fem.TetMesh(nodes, tets.astype(np.float64), ctx=no_native)
    with pytest.raises(TypeError):
        fem.TetMesh(nodes, tets.astype(np.int16), ctx=no_native)
    with pytest.raises(ValueError, match="expected"):
        fem.TetMesh(nodes, np.zeros((2, 3), dtype=np.int64), ctx=no_native)
    with pytest.raises(ValueError, match="int32 range"):
        fem.TetMesh(nodes, np.array([[0, 1, 2, 2 ** 31]]), ctx=no_native)
    with pytest.raises(ValueError, match="is on"):
        fem.TetMesh(torch.zeros((5, 3), dtype=torch.float64, device="meta"), tets, ctx=no_native)
    for good in (tets, tets.astype(np.int32), torch.from_numpy(tets)):
        with pytest.raises(AssertionError, match="native call"):
            fem.TetMesh(nodes, good, ctx=no_native)


def test_operators_check_arguments_first(stub):
    k, rho = torch.ones(2, dtype=torch.float64), torch.ones(5, dtype=torch.float64)
    with pytest.raises(TypeError):
        stub.heat(k.float())
    with pytest.raises(ValueError, match="expected"):
        stub.heat(torch.ones(3, dtype=torch.float64))  # per vertex, not per tet
    with pytest.raises(ValueError, match="expected"):
        stub.heat(k.reshape(2, 1))
    with pytest.raises(TypeError):
        stub.heat(k, density=rho.float())
    with pytest.raises(ValueError, match="expected"):
        stub.heat(k, density=k)
    with pytest.raises(TypeError):
        stub.heat(k, density=None)
    with pytest.raises(TypeError):
        stub.heat(k, density="1")
    with pytest.raises(ValueError, match="is on"):
        stub.heat(k.to("meta"))
    with pytest.raises(TypeError, match="DeviceMatrix"):
        stub.heat(k, rho, out=sp.identity(5, format="csr"))
    with pytest.raises(TypeError, match="DeviceMatrix"):
        stub.laplacian(out=np.zeros(23))
    with pytest.raises(TypeError):
        stub.elasticity(3e6, None)
    with pytest.raises(ValueError, match="expected"):
        stub.elasticity(rho, 0.4)  # per vertex
    with pytest.raises(TypeError):
        stub.elasticity(k, k.float())
    with pytest.raises(TypeError, match="mass_coef"):
        stub.elasticity(k, 0.4, mass_coef=rho)
    with pytest.raises(TypeError):
        stub.matrix(dtype=torch.float16)
    with pytest.raises(ValueError, match="block_size"):
        stub.matrix(block_size=2)
    with pytest.raises(TypeError):
        stub.set_nodes(np.zeros((5, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="expected"):
        stub.set_nodes(np.zeros((4, 3)))
    # well-formed arguments reach the native call (which the stub forbids)
    for call in (lambda: stub.heat(k, rho), lambda: stub.heat(None, 2e-4), lambda: stub.heat(k.numpy(), rho.numpy()),
                 lambda: stub.laplacian(), lambda: stub.elasticity(3e6, 0.4, 1e4), lambda: stub.elasticity(k, k),
                 lambda: stub.lumped_mass(), lambda: stub.pattern(), lambda: stub.set_nodes(np.zeros((5, 3)))):
        with pytest.raises(AssertionError, match="native call"):
            call()


def test_binding_lists_the_fem_entry_points():
    names = {n for n in _lib.SIGNATURES if n.startswith("lspcg_fem_")}
    assert names == {"lspcg_fem_" + s for s in ("create", "destroy", "set_nodes", "info", "pattern", "lumped_mass",
                                                "heat", "elasticity")}
