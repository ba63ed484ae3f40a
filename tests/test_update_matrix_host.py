"""Host side of "new values of A on a live solver": the three calls are declared, bound and exported,
the Python entry points exist, and argument errors are raised before any native call (no GPU)."""
import inspect
import re
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from learningsparsepreconditioner4gpu_amd import _lib, infer, sparse, workspace
from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient
from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

ROOT = Path(__file__).resolve().parents[1]
NEW = ("lspcg_mat_set_values", "lspcg_assemble_into", "lspcg_solver_update_matrix")


def test_the_three_calls_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lspcg.h").read_text(), flags=re.S)
    assert re.search(r"\bint lspcg_mat_set_values\(lspcg_mat\* A, const int32_t\* indptr, const int32_t\* indices,\s*"
                     r"const void\* vals,\s*int dtype\);", header)
    assert re.search(r"\bint lspcg_assemble_into\(lspcg_ctx\* ctx, int64_t nb, int64_t E, int bs, const int64_t\* "
                     r"edge_index,\s*const void\* blocks, int in_dtype, const void\* mask, int mask_dtype,\s*"
                     r"int out_block, lspcg_mat\* A\);", header)
    assert re.search(r"\bint lspcg_solver_update_matrix\(lspcg_solver\* s, double\* t_ms, int\* graphs_kept\);", header)
    for name, nargs in zip(NEW, (5, 11, 3)):
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs, name
    # lspcg_assemble's row without the output dtype, the handle by value instead of by reference
    _, base = _lib.SIGNATURES["lspcg_assemble"]
    _, into = _lib.SIGNATURES["lspcg_assemble_into"]
    assert into[:9] == base[:9] and into[9] == base[10] and into[10] is _lib.vp
    if not _lib.LIB_PATH.exists():
        pytest.fail(f"{_lib.LIB_PATH} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (lspcg_[a-z0-9_]+)$", out.stdout, flags=re.M))
    assert set(NEW) <= exported, set(NEW) - exported


def test_the_header_documents_the_breakdown_rule():
    header = (ROOT / "include" / "lspcg.h").read_text()
    doc = header[:header.index("int lspcg_solver_update_matrix(")]
    doc = doc[doc.rindex("/*"):]
    assert "LSPCG_ERR_BREAKDOWN" in doc and "graphs_kept" in doc


def test_python_entry_points_exist():
    assert list(inspect.signature(DeviceMatrix.set_values).parameters) == ["self", "vals", "indptr", "indices"]
    assert inspect.signature(sparse.assemble).parameters["out"].default is None
    assert list(inspect.signature(PreconditionedConjugateGradient.update_matrix).parameters) == ["self", "A_new"]
    assert inspect.signature(PreconditionedConjugateGradient.update_matrix).parameters["A_new"].default is None
    assert inspect.signature(workspace.SimpleInferenceWorkspace.system_matrix).parameters["out"].default is None
    assert inspect.signature(infer.run).parameters["reuse_solver"].default is False


@pytest.fixture
def no_native(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError("native call before the arguments were checked")

    monkeypatch.setattr(_lib, "call", no_call)


def _matrix(n=6, nnzb=10, bs=1, code=_lib.F64, values_version=0):
    """A DeviceMatrix without a native handle."""
    D = DeviceMatrix.__new__(DeviceMatrix)
    D.handle = None
    D.ctx = types.SimpleNamespace(torch_device=torch.device("cpu"))
    D.n, D.nnzb, D.block_size, D.dtype_code = n, nnzb, bs, code
    D.version, D.values_version = 0, values_version
    return D


def test_set_values_checks_arguments_first(no_native):
    D = _matrix()
    vals = np.zeros(10)
    with pytest.raises(TypeError):
        D.set_values(vals.astype(np.float32))
    with pytest.raises(TypeError):
        D.set_values(torch.zeros(10, dtype=torch.float32))
    with pytest.raises(ValueError, match="entries"):
        D.set_values(np.zeros(9))
    with pytest.raises(TypeError):
        D.set_values(vals, indptr=np.zeros(7, dtype=np.int64))
    with pytest.raises(TypeError):
        D.set_values(vals, indices=np.zeros(10, dtype=np.float64))
    # another entry count is another pattern: the error of the device comparison, nothing written
    for kw in (dict(indptr=np.zeros(8, dtype=np.int32)), dict(indices=np.zeros(11, dtype=np.int32))):
        with pytest.raises(_lib.LspcgError) as e:
            D.set_values(vals, **kw)
        assert e.value.code == _lib.ERR_FORMAT
    assert D.values_version == 0 and D.version == 0
    with pytest.raises(AssertionError, match="native call"):
        D.set_values(vals, indptr=np.zeros(7, dtype=np.int32), indices=np.zeros(10, dtype=np.int32))
    # BSR: nnzb * bs * bs values
    B = _matrix(n=6, nnzb=3, bs=3)
    with pytest.raises(ValueError, match="entries"):
        B.set_values(np.zeros(3))
    with pytest.raises(AssertionError, match="native call"):
        B.set_values(np.zeros((3, 3, 3)))


def test_assemble_out_checks_arguments_first(no_native):
    ei = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(TypeError, match="DeviceMatrix"):
        sparse.assemble(ei, torch.zeros(4), 6, out=sp.identity(6, format="csr"))
    with pytest.raises(ValueError, match="rows"):
        sparse.assemble(ei, torch.zeros(4), 9, out=_matrix(n=6))
    with pytest.raises(ValueError, match="block size"):
        sparse.assemble(ei, torch.zeros(4, 3, 3), 6, block_output=True, out=_matrix(n=6, bs=1))
    with pytest.raises(ValueError, match="block size"):
        sparse.assemble(ei, torch.zeros(4, 3, 3), 6, block_output=False, out=_matrix(n=6, bs=3))
    with pytest.raises(ValueError, match="context"):
        sparse.assemble(ei, torch.zeros(4), 6, out=_matrix(n=6), ctx=types.SimpleNamespace())


@pytest.fixture
def stub(no_native):
    """A solver object without a native handle on a matrix without one."""
    s = PreconditionedConjugateGradient.__new__(PreconditionedConjugateGradient)
    s.A = _matrix()
    s.n = 6
    s.dtype = np.dtype(np.float64)
    s.ctx = s.A.ctx
    s.handle = None
    s.preconditioner = "none"
    s.setup_time = 0.0
    s._A_values = 0
    s._L = None
    s._spai_key = None
    return s


def test_update_matrix_checks_arguments_first(stub):
    A = sp.csr_matrix((np.arange(1.0, 11.0), np.arange(10) % 6, np.array([0, 2, 4, 6, 8, 9, 10])), shape=(6, 6))
    with pytest.raises(TypeError, match="dtype"):
        stub.update_matrix(A.astype(np.float32))
    with pytest.raises(TypeError, match="dtype"):
        stub.update_matrix(_matrix(code=_lib.F32))
    with pytest.raises(TypeError, match="scipy"):
        stub.update_matrix(np.eye(6))
    more = sp.csr_matrix(A + sp.csr_matrix(([1.0], ([5], [0])), shape=(6, 6)))
    assert more.nnz == 11
    for bad in (more, sp.identity(7, format="csr"), _matrix(nnzb=11), _matrix(n=7), _matrix(bs=3, n=6, nnzb=10)):
        with pytest.raises(_lib.LspcgError) as e:
            stub.update_matrix(bad)
        assert e.value.code == _lib.ERR_FORMAT
    assert stub.A.values_version == 0
    with pytest.raises(AssertionError, match="native call"):
        stub.update_matrix(A)
    with pytest.raises(AssertionError, match="native call"):
        stub.update_matrix()  # None: self.A was changed in place


def test_solves_raise_when_the_matrix_changed_without_update_matrix(stub):
    b = torch.zeros(6, dtype=torch.float64)
    with pytest.raises(AssertionError, match="native call"):
        stub.solve(b, b.clone())  # current values: the arguments reach the native call
    stub.A.values_version += 1  # what set_values / assemble(out=) do
    with pytest.raises(RuntimeError, match="update_matrix"):
        stub.solve(b, b.clone())
    with pytest.raises(RuntimeError, match="update_matrix"):
        stub.solve_multi(torch.zeros((6, 2), dtype=torch.float64), torch.zeros((6, 2), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="update_matrix"):
        stub(b, b.clone())
    # the counter is not `version`: an in-place scaling as it runs today raises nothing new
    stub.A.values_version -= 1
    stub.A.version += 1
    with pytest.raises(AssertionError, match="native call"):
        stub.solve(b, b.clone())


def test_reuse_solver_is_one_solve_at_a_time(no_native):
    ws = types.SimpleNamespace(epsilon=1e-3)
    for kw in (dict(batch=2), dict(concurrency=2)):
        with pytest.raises(ValueError, match="reuse_solver"):
            infer.run([], ws, reuse_solver=True, **kw)
    with pytest.raises(SystemExit):
        infer.main(["--reuse-solver", "--dataset", "poisson_tiny8"])
