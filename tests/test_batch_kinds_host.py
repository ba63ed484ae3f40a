"""Host-side contract of the lockstep batch's preconditioner kinds: the binding row, the argument
checks of ``BatchedConjugateGradient`` that must fail before any library call, and the drivers'
``batch`` keyword.  No GPU."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

from learningsparsepreconditioner4gpu_amd import _lib


def test_binding_table_has_create_precond():
    assert "lspcg_batch_create_precond" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["lspcg_batch_create_precond"]
    # lspcg_batch_create's row with the kind inserted before epsilon
    _, base = _lib.SIGNATURES["lspcg_batch_create"]
    assert len(args) == len(base) + 1 and args[:4] == base[:4] and args[5:] == base[4:]


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*_a, **_k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "call", refuse)


def test_batched_cg_rejects_kinds_before_any_library_call(no_library):
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient

    A = sp.identity(4, format="csr", dtype=np.float64)
    with pytest.raises(ValueError):
        BatchedConjugateGradient([A], preconditioner="ic")
    with pytest.raises(ValueError):
        BatchedConjugateGradient([A], [A], 1e-3, preconditioner="jacobi")
    with pytest.raises(ValueError):
        BatchedConjugateGradient([A], [A], 1e-3, preconditioner="none")
    with pytest.raises(ValueError):
        BatchedConjugateGradient([A], [A], preconditioner="diagonal")
    with pytest.raises(ValueError):  # the SPAI kinds need their factors
        BatchedConjugateGradient([A], preconditioner="ext_spai_scaled")


def test_drivers_accept_batch():
    from learningsparsepreconditioner4gpu_amd import infer, validate

    p = inspect.signature(infer.run_baseline).parameters
    assert "batch" in p and p["batch"].default == 1
    for name in ("get_pcg_scaled_iter_time_batch", "get_cg_iter_time_batch"):
        assert callable(getattr(validate, name))
    with pytest.raises(ValueError):  # ic has no lockstep form
        validate.get_cg_iter_time_batch([], [], "ic")
