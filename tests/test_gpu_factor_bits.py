"""The factor unit's outputs in fp32 and fp64, pinned bit for bit.

``tests/golden/factor_bits.json`` holds the sha256 of ``ic0()``, ``ainv0()`` (indptr, indices and
data bytes) and of ``trsv(lower=True)`` / ``trsv(lower=False)`` on the device's own IC(0) factor and
its sorted transpose, for the masked ``poisson2d_grid(16, 16)`` and ``kuhn_dirichlet(7)`` of
``test_gpu_precond._systems``.  The oracle reproduces every digest in both precisions
(``tests/test_factor_host.py``, on the CPU), so these are a second guard beside the comparisons with
the oracle in ``test_gpu_precond`` (fp64, grids) and ``test_gpu_factor_shapes`` (fp32 and fp64,
irregular matrices).  A few hundred
rows in tens of levels: the padded order spans several 256-position blocks, so several workgroups
of the sync-free solve wait on one another.

The hashes were recorded with this file's ``__main__`` block on the commit the fixture names; the
Python API it drives is the same there, so a refactor of the setup / dispatch code has to
reproduce them exactly.

    python tests/test_gpu_factor_bits.py --commit <sha> [--out tests/golden/factor_bits.json]
"""
import functools
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu

FIXTURE = ROOT / "tests" / "golden" / "factor_bits.json"
RUNS = [(name, dt) for name in ("poisson16", "kuhn7") for dt in ("f32", "f64")]
DTYPES = {"f32": np.float32, "f64": np.float64}


@functools.lru_cache(maxsize=None)
def systems():
    from tests.test_gpu_precond import _systems

    return _systems()


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def sha_csr(M):
    return sha(M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data)


def oracle_bits(name, dt="f64"):
    """The same record from oracle/precond.py in that precision (tests/test_factor_host.py holds
    it to the fixture in both, without a GPU)."""
    from oracle import precond as OP

    npdt = DTYPES[dt]
    A = systems()[name][0]
    L = OP.ic0(A, npdt)
    U = sp.csr_matrix(L.T)
    U.sort_indices()
    r = np.random.default_rng(3).normal(size=A.shape[0]).astype(npdt)
    y, z = OP.trsv_lower(L, r, npdt), OP.trsv_upper(U, r, npdt)
    assert L.data.dtype == npdt and y.dtype == npdt and z.dtype == npdt
    return {"ic0": sha_csr(L), "ainv0": sha_csr(OP.ainv_spai_factor(A, npdt)), "trsv_lower": sha(y), "trsv_upper": sha(z)}


def bits(name, dt):
    """The record of one system in one precision: the four digests."""
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    npdt = DTYPES[dt]
    A = systems()[name][0]
    dA = DeviceMatrix.from_scipy(A, dtype=npdt)
    L = dA.ic0()[0].to_scipy()
    Z = dA.ainv0()[0].to_scipy()
    assert L.data.dtype == npdt and Z.data.dtype == npdt
    U = sp.csr_matrix(L.T)
    U.sort_indices()
    r = torch.from_numpy(np.random.default_rng(3).normal(size=A.shape[0]).astype(npdt)).cuda()
    y = DeviceMatrix.from_scipy(L, dtype=npdt).trsv(r, lower=True).cpu().numpy()
    z = DeviceMatrix.from_scipy(U, dtype=npdt).trsv(r, lower=False).cpu().numpy()
    assert y.dtype == npdt and np.isfinite(y).all() and np.isfinite(z).all()
    return {"ic0": sha_csr(L), "ainv0": sha_csr(Z), "trsv_lower": sha(y), "trsv_upper": sha(z)}


@functools.lru_cache(maxsize=None)
def fixture():
    return json.loads(FIXTURE.read_text())


@pytest.mark.parametrize("name,dt", RUNS, ids=[f"{n}-{d}" for n, d in RUNS])
def test_bits(gpu_ctx, name, dt):
    got, want = bits(name, dt), fixture()["cases"][f"{name}/{dt}"]
    print(name, dt, got)
    assert got == want
    if dt == "f64":  # what test_gpu_precond's comparisons with the oracle imply
        assert want == oracle_bits(name)


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit this checkout is (written into the fixture)")
    ap.add_argument("--out", default=str(FIXTURE))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the recorder needs the MI355X"
    doc = {"recorded_from": args.commit, "cases": {f"{n}/{d}": bits(n, d) for n, d in RUNS}}
    for n in ("poisson16", "kuhn7"):
        assert doc["cases"][f"{n}/f64"] == oracle_bits(n), n
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))
