"""CPU: the host side of PreconditionedConjugateGradient.solve_multi -- the grouping of more than
eight right-hand sides and the argument checks made before any native call."""
import types

import numpy as np
import pytest
import torch

from learningsparsepreconditioner4gpu_amd import _lib
from learningsparsepreconditioner4gpu_amd import linalg
from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient, _rhs_groups


@pytest.mark.parametrize("k,want", [
    (1, [(0, 1)]),
    (3, [(0, 3)]),
    (8, [(0, 8)]),
    (9, [(0, 8), (8, 1)]),
    (11, [(0, 8), (8, 3)]),
    (16, [(0, 8), (8, 8)]),
])
def test_rhs_groups(k, want):
    got = _rhs_groups(k)
    assert got == want
    assert sum(nc for _, nc in got) == k and all(1 <= nc <= linalg.MULTI_RHS_MAX for _, nc in got)
    assert [c0 for c0, _ in got] == [sum(nc for _, nc in got[:i]) for i in range(len(got))]  # contiguous, in order


@pytest.mark.parametrize("k", [0, -3])
def test_rhs_groups_rejects_no_columns(k):
    with pytest.raises(ValueError):
        _rhs_groups(k)


def test_binding_matches_the_batch_reporting():
    """iters / status / res_hist have lspcg_batch_solve's types: per-column int64, int32, double*."""
    res, args = _lib.SIGNATURES["lspcg_solver_solve_multi"]
    bres, bargs = _lib.SIGNATURES["lspcg_batch_solve"]
    assert res is bres and len(args) == 10
    assert args[4:] == bargs[3:]  # rtol, max_iter, iters, status, res_hist, t_solve_ms


@pytest.fixture
def stub(monkeypatch):
    """A solver object without a native handle (no GPU here): n = 6, fp64, on the CPU 'device'; any
    native call fails the test."""
    s = PreconditionedConjugateGradient.__new__(PreconditionedConjugateGradient)
    s.n = 6
    s.dtype = np.dtype(np.float64)
    s.ctx = types.SimpleNamespace(torch_device=torch.device("cpu"))
    s.handle = None

    def no_call(*a, **k):
        raise AssertionError("native call before the arguments were checked")

    monkeypatch.setattr(_lib, "call", no_call)
    return s


def test_solve_multi_checks_arguments_first(stub):
    good = torch.zeros((6, 3), dtype=torch.float64)
    with pytest.raises(TypeError):
        stub.solve_multi(np.zeros((6, 3)), good)
    with pytest.raises(ValueError, match="expected"):
        stub.solve_multi(torch.zeros(6, dtype=torch.float64), good)  # a vector, not (n, k)
    with pytest.raises(ValueError, match="expected"):
        stub.solve_multi(torch.zeros((5, 3), dtype=torch.float64), good)  # wrong n
    with pytest.raises(ValueError, match="expected"):
        stub.solve_multi(torch.zeros((6, 0), dtype=torch.float64), torch.zeros((6, 0), dtype=torch.float64))
    with pytest.raises(TypeError):
        stub.solve_multi(good.float(), good)
    with pytest.raises(TypeError):
        stub.solve_multi(good, good.float())
    with pytest.raises(ValueError, match="contiguous"):
        stub.solve_multi(torch.zeros((3, 6), dtype=torch.float64).t(), good)  # column-major strides
    with pytest.raises(ValueError, match="contiguous"):
        stub.solve_multi(good, torch.zeros((6, 6), dtype=torch.float64)[:, ::2])
    with pytest.raises(ValueError, match="B is"):
        stub.solve_multi(good, torch.zeros((6, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="is on"):
        stub.solve_multi(good.to("meta"), good)
    # well-formed arguments reach the native call (which the stub forbids)
    with pytest.raises(AssertionError, match="native call"):
        stub.solve_multi(good, good.clone())
