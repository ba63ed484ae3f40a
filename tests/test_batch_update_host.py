"""Host side of "new values of A and L on a live batch": lspcg_batch_update is declared, bound and
exported, the Python entry points exist, and argument errors are raised before any native call
(no GPU)."""
import ctypes as C
import inspect
import re
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from learningsparsepreconditioner4gpu_amd import _lib, infer, validate
from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient
from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

ROOT = Path(__file__).resolve().parents[1]


def test_the_call_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lspcg.h").read_text(), flags=re.S)
    assert re.search(r"\bint lspcg_batch_update\(lspcg_batch\* bt, const lspcg_mat\* const\* A, "
                     r"const lspcg_mat\* const\* L,\s*double epsilon, double\* t_ms, int\* graphs_kept\);", header)
    res, args = _lib.SIGNATURES["lspcg_batch_update"]
    assert len(args) == 6
    # the handle arrays and ε as lspcg_batch_create takes them
    _, create = _lib.SIGNATURES["lspcg_batch_create"]
    assert args[1:4] == create[2:5]
    if not _lib.LIB_PATH.exists():
        pytest.fail(f"{_lib.LIB_PATH} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (lspcg_[a-z0-9_]+)$", out.stdout, flags=re.M))
    assert "lspcg_batch_update" in exported


def test_the_header_documents_the_refusal_and_the_graph_rule():
    header = (ROOT / "include" / "lspcg.h").read_text()
    doc = header[:header.index("int lspcg_batch_update(")]
    doc = doc[doc.rindex("/*"):]
    words = " ".join(doc.replace("*", " ").split())
    assert "LSPCG_ERR_FORMAT" in words and "nothing has been written" in words and "graphs_kept" in words


def test_python_entry_points_exist():
    sig = inspect.signature(BatchedConjugateGradient.update)
    assert list(sig.parameters) == ["self", "As", "Ls", "epsilon"]
    assert all(sig.parameters[k].default is None for k in ("As", "Ls", "epsilon"))
    assert inspect.signature(infer.run).parameters["reuse_batch"].default is False
    assert inspect.signature(infer.run_baseline).parameters["reuse_batch"].default is False
    for f in (validate.get_pcg_iter_time_batch, validate.get_pcg_scaled_iter_time_batch, validate.get_cg_iter_time_batch):
        assert inspect.signature(f).parameters["reuse"].default is None


@pytest.fixture
def no_native(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError("native call before the arguments were checked")

    monkeypatch.setattr(_lib, "call", no_call)


def _matrix(n=6, nnzb=10, bs=1, code=_lib.F64):
    """A DeviceMatrix with a null native handle."""
    D = DeviceMatrix.__new__(DeviceMatrix)
    D.handle = C.c_void_p()
    D.ctx = types.SimpleNamespace(torch_device=torch.device("cpu"), handle=None)
    D.n, D.nnzb, D.block_size, D.dtype_code = n, nnzb, bs, code
    D.version, D.values_version = 0, 0
    return D


def _stub(kind, bs=1):
    """A batch of two systems (6 rows / 10 entries, 9 rows / 9 entries) without a native handle."""
    B = BatchedConjugateGradient.__new__(BatchedConjugateGradient)
    B.preconditioner = kind
    B.dtype = np.dtype(np.float64)
    B.A = [_matrix(bs=bs, n=6, nnzb=10), _matrix(bs=bs, n=9, nnzb=9)]
    B.L = ([_matrix(bs=bs, n=6, nnzb=10), _matrix(bs=bs, n=9, nnzb=9)] if kind in ("ext_spai", "ext_spai_scaled", "ainv")
           else None)
    B.ctx = B.A[0].ctx
    B.n = [6, 9]
    B.epsilon = 1e-3 if kind.startswith("ext_spai") else 0.0
    B.setup_time = 0.0
    B.handle = None
    return B


A0 = sp.csr_matrix((np.arange(1.0, 11.0), np.arange(10) % 6, np.array([0, 2, 4, 6, 8, 9, 10])), shape=(6, 6))
A1 = sp.identity(9, format="csr", dtype=np.float64)


@pytest.mark.parametrize("kind", ["ext_spai", "ext_spai_scaled"])
def test_update_checks_arguments_first(no_native, kind):
    B = _stub(kind)
    before = (list(B.A), list(B.L), B.epsilon)
    # list lengths, nothing to update
    with pytest.raises(ValueError, match="entries"):
        B.update([A0])
    with pytest.raises(ValueError, match="entries"):
        B.update(None, [A0, A1, A1])
    for args in ((), (None, None, None), ([None, None],), (None, [None, None]), (None, None, 1e-3)):
        with pytest.raises(ValueError, match="nothing to update"):
            B.update(*args)
    # dtype
    with pytest.raises(TypeError, match="dtype"):
        B.update([A0.astype(np.float32), None])
    with pytest.raises(TypeError, match="dtype"):
        B.update(None, [None, _matrix(n=9, nnzb=9, code=_lib.F32)])
    with pytest.raises(TypeError, match="scipy"):
        B.update([np.eye(6), None])
    # size, entry count, block size
    more = sp.csr_matrix(A0 + sp.csr_matrix(([1.0], ([5], [0])), shape=(6, 6)))
    assert more.nnz == 11
    for bad in (more, sp.identity(7, format="csr"), _matrix(nnzb=11), _matrix(n=7), _matrix(bs=3, n=6, nnzb=10)):
        for args in (([bad, None],), (None, [bad, None]), ([None, A1], [bad, None])):
            with pytest.raises(_lib.LspcgError) as e:
                B.update(*args)
            assert e.value.code == _lib.ERR_FORMAT
    with pytest.raises(_lib.LspcgError) as e:
        B.update([A1, A0])  # each fits the other system
    assert e.value.code == _lib.ERR_FORMAT
    assert (list(B.A), list(B.L), B.epsilon) == before
    # good arguments reach the native call
    for args in (([A0, A1],), ([None, A1], [A0, None]), (None, [_matrix(), None]), (None, None, 2e-3)):
        with pytest.raises(AssertionError, match="native call"):
            B.update(*args)
    assert (list(B.A), list(B.L), B.epsilon) == before


@pytest.mark.parametrize("kind", ["none", "diagonal", "ainv"])
def test_update_takes_no_factors_for_the_kinds_without_them(no_native, kind):
    B = _stub(kind)
    with pytest.raises(ValueError, match="takes no Ls"):
        B.update([A0, A1], [A0, A1])
    with pytest.raises(ValueError, match="takes no Ls"):
        B.update(None, [A0, A1])
    with pytest.raises(ValueError, match="nothing to update"):
        B.update()
    with pytest.raises(ValueError, match="nothing to update"):
        B.update(None, None, 5e-3)  # these kinds have no ε of their own
    with pytest.raises(_lib.LspcgError) as e:
        B.update([A0, sp.identity(8, format="csr")])
    assert e.value.code == _lib.ERR_FORMAT
    with pytest.raises(AssertionError, match="native call"):
        B.update([A0, None])


def test_update_checks_bsr_operands_first(no_native):
    B = _stub("diagonal", bs=3)
    B.A = [_matrix(bs=3, n=6, nnzb=2), _matrix(bs=3, n=9, nnzb=3)]
    blocks = sp.block_diag([np.full((3, 3), 2.0)] * 2, format="csr")
    with pytest.raises(_lib.LspcgError) as e:
        B.update([sp.block_diag([np.full((3, 3), 2.0)] * 3, format="csr"), None])  # 9 rows for the 6-row system
    assert e.value.code == _lib.ERR_FORMAT
    with pytest.raises(_lib.LspcgError) as e:
        B.update([None, sp.csr_matrix(np.ones((9, 9)))])  # 9 blocks for 3
    assert e.value.code == _lib.ERR_FORMAT
    with pytest.raises(AssertionError, match="native call"):
        B.update([blocks, None])


def test_reuse_batch_needs_a_batch(no_native):
    ws = types.SimpleNamespace(epsilon=1e-3)
    for kw in (dict(batch=1), dict(), dict(concurrency=2)):
        with pytest.raises(ValueError, match="reuse_batch"):
            infer.run([], ws, reuse_batch=True, **kw)
    with pytest.raises(ValueError, match="reuse_batch"):
        infer.run_baseline([], ws, "diagonal", reuse_batch=True, batch=1)
    with pytest.raises(SystemExit):
        infer.main(["--reuse-batch", "--dataset", "poisson_tiny8"])
