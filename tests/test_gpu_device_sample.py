"""GPU: lspcg_mat_edge_index / lspcg_mat_sample (data.make_sample of a DeviceMatrix, DeviceSampler)
against the host path, bit for bit.

References.  The host expressions of dataset.make_data evaluated with the scale the device wrote
(numpy's fp64 multiply, divide and sqrt and its fp64 -> fp32 conversion are correctly rounded, and so
are the device's), dataset._scatter on the device's own edge_attr, and make_data's own sample.  The
mean / frob scales are compared with math.fsum's within a relative 1e-14: three orders above what a
compensated sum and its two or three final roundings can cause, three orders below the fp32 rounding
unit that decides the outputs.  An fp32 matrix is compared with the host sample of its values widened
to fp64, which is what the device computes on.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from learningsparsepreconditioner4gpu_amd import _lib
from learningsparsepreconditioner4gpu_amd import problems as P
from learningsparsepreconditioner4gpu_amd.data import DeviceSampler, make_sample
from learningsparsepreconditioner4gpu_amd.dataset import _scatter

pytestmark = pytest.mark.gpu

UNREFERENCED = 37  # the column of `unsym` that no entry names
NORMS = ("mean", "frob", "l1", "none")
REDUCES = ("disable", "sum", "mean", "max", "min")
DIAG_FIELDS = ("diagonal", "inv_diag", "rsqrt_diag")


def _arrow(n=300):
    """Full first row and column plus the diagonal: rows and in-degrees longer than a wave."""
    rng = np.random.default_rng(11)
    A = sp.lil_matrix((n, n))
    A[0, :] = rng.standard_normal(n)
    A[:, 0] = rng.standard_normal((n, 1))
    A.setdiag(1.0 + rng.random(n))
    A = sp.csr_matrix(A)
    A.sort_indices()
    assert A.nnz == 3 * n - 2 and A.nnz % 4 != 0
    return A


def _unsym(n=70):
    """Rows 0 and n-1 empty, odd rows without a stored diagonal, column UNREFERENCED never named."""
    rng = np.random.default_rng(12)
    rows, cols, vals = [], [], []
    allowed = np.array([c for c in range(n) if c != UNREFERENCED])
    for i in range(1, n - 1):
        cs = set(rng.choice(allowed, size=int(rng.integers(2, 7)), replace=False).tolist()) - {i}
        for c in sorted(cs):
            rows.append(i), cols.append(c), vals.append(float(rng.standard_normal()))
        if i % 2 == 0 and i != UNREFERENCED:
            rows.append(i), cols.append(i), vals.append(1.0 + float(rng.random()))
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    assert A.indptr[1] == 0 and A.indptr[-1] == A.indptr[-2] and not np.any(A.indices == UNREFERENCED)
    assert np.all(A.diagonal()[1::2] == 0) and np.all(A.diagonal()[2:-1:2] > 0)
    return A


@functools.lru_cache(maxsize=None)
def matrix(name, dtype):
    """``(A fp64 scipy holding exactly the device's values, block size)``; sorted, never modified."""
    bs = 1
    if name == "poisson":
        A = P.poisson2d_grid(7, 9)[0]
    elif name == "kuhn23":
        A = P.kuhn_laplacian(23)
    elif name == "one":
        A = sp.csr_matrix(np.array([[2.5]]))
    elif name == "arrow":
        A = _arrow()
    elif name == "unsym":
        A = _unsym()
    else:
        A, bs = P.elasticity_box(5, 4, 4)[0], 3
    A = sp.csr_matrix(A)
    A.sort_indices()
    A = sp.csr_matrix(A.astype(dtype).astype(np.float64))  # the values the device holds, widened
    if bs == 3:
        A = sp.bsr_matrix(A, blocksize=(3, 3))
        A.sort_indices()
        assert np.any(A.data == 0.0)  # in-block zeros
    return A, bs


MATRICES = ("poisson", "kuhn23", "one", "arrow", "unsym", "elast")
DTYPES = (np.float64, np.float32)
CASES = [pytest.param(m, d, id=f"{m}-{np.dtype(d).name}") for m in MATRICES for d in DTYPES]


def test_the_matrices_are_what_the_cases_need():
    assert matrix("poisson", np.float64)[0].shape[0] == 63
    K = matrix("kuhn23", np.float64)[0]
    assert K.shape[0] == 12167 and K.nnz == 170083 and K.shape[0] % 256 != 0
    assert matrix("one", np.float64)[0].nnz == 1
    E = matrix("elast", np.float32)[0]
    assert E.blocksize == (3, 3) and E.shape[0] == 3 * 80


def device_matrix(name, dtype):
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    A, bs = matrix(name, dtype)
    return DeviceMatrix.from_scipy(A, dtype=dtype, block_size=bs)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(mask fp64 [N*b] of zeros and ones, node_features fp32 [N, 3]) of a matrix, seeded."""
    A, bs = matrix(name, np.float64)
    rng = np.random.default_rng(5)
    mask = (rng.random(A.shape[0]) > 0.2).astype(np.float64)
    if A.shape[0] > 1:
        mask[1] = 0.0
    nf = rng.standard_normal((A.shape[0] // bs, 3)).astype(np.float32)
    mask.setflags(write=False), nf.setflags(write=False)
    return mask, nf


@functools.lru_cache(maxsize=None)
def host_sample(name, dtype, norm):
    A, bs = matrix(name, dtype)
    return make_sample(A, block_size=bs, normalize_matrix=norm)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32).astype(np.int64)


def assert_same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} entries differ, first at {bad[:5]}"


@pytest.mark.parametrize("name, dtype", CASES)
def test_edge_index(gpu_ctx, name, dtype):
    A, bs = matrix(name, dtype)
    s = make_sample(device_matrix(name, dtype))
    want = P.to_block_graph(sp.csr_matrix(A), bs).edge_index
    assert s.edge_index.dtype == torch.int64 and s.edge_index.is_cuda
    assert np.array_equal(s.edge_index.cpu().numpy(), want)
    assert s.block_size == bs and s.num_nodes == A.shape[0] // bs and s.ptr.tolist() == [0, s.num_nodes]


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("name, dtype", CASES)
def test_scale_and_value_outputs(gpu_ctx, name, dtype, norm):
    A, bs = matrix(name, dtype)
    Ad = device_matrix(name, dtype)
    if norm == "l1" and bs == 3:
        with pytest.raises(ValueError, match="block_size 1 only"):
            make_sample(Ad, normalize_matrix=norm)
        return
    dev = make_sample(Ad, normalize_matrix=norm)
    host = host_sample(name, dtype, norm)
    s = dev.matrix_scale
    v = A.data.astype(np.float64).reshape(-1)
    # ---- scale
    if norm in ("l1", "none"):
        assert s == host.matrix_scale, (s, host.matrix_scale)
    else:
        want = (1.0 / (math.fsum(np.abs(v)) / float(v.size)) if norm == "mean"
                else 1.0 / math.sqrt(math.fsum(v * v)))
        rel = abs(s - want) / want
        print(f"{name} {np.dtype(dtype).name} {norm}: scale {s!r}, fsum {want!r}, rel {rel:.2e}, "
              f"numpy rel {abs(host.matrix_scale - want) / want:.2e}")
        assert rel <= 1e-14, (s, want, rel)
    # ---- the host expressions with the device's scale, bit for bit
    E, N = A.indices.size, A.shape[0] // bs
    assert dev.edge_attr.shape == (E, bs * bs) and dev.matrix_values.shape == (E, bs, bs)
    assert dev.matrix_values.data_ptr() == dev.edge_attr.data_ptr()
    assert_same_bits(dev.edge_attr, (s * v).astype(np.float32).reshape(E, bs * bs), "edge_attr")
    d = sp.csr_matrix(A).diagonal().reshape(N, bs) * s
    assert_same_bits(dev.diagonal, d.astype(np.float32), "diagonal")
    assert_same_bits(dev.inv_diag, (1.0 / (d + 1e-7)).astype(np.float32), "inv_diag")
    assert_same_bits(dev.rsqrt_diag, (1.0 / np.sqrt(d + 1e-7)).astype(np.float32), "rsqrt_diag")
    # ---- make_sample's own output: within one fp32 ulp
    differ = 0
    for f in ("edge_attr", "matrix_values") + DIAG_FIELDS:
        g, w = bits(getattr(dev, f)), bits(getattr(host, f))
        assert g.shape == w.shape, f
        differ += int(np.count_nonzero(g != w))
        assert np.abs(g - w).max() <= 1, f
    print(f"{name} {np.dtype(dtype).name} {norm}: {differ} values differ from the host sample's")
    assert torch.equal(dev.x.cpu(), host.x) and torch.equal(dev.mask.cpu(), host.mask)


@pytest.mark.parametrize("with_nf", (False, True), ids=("nonf", "nf3"))
@pytest.mark.parametrize("mask_kind", ("nomask", "mask32", "mask64"))
@pytest.mark.parametrize("name, dtype", CASES)
def test_x_columns(gpu_ctx, name, dtype, mask_kind, with_nf):
    A, bs = matrix(name, dtype)
    N = A.shape[0] // bs
    mask64, nf = inputs(name)
    mask = {"nomask": None, "mask32": mask64.astype(np.float32), "mask64": mask64}[mask_kind]
    Ad = device_matrix(name, dtype)
    k = 3 if with_nf else 0
    for reduce in REDUCES:
        s = make_sample(Ad, mask=None if mask is None else torch.from_numpy(mask.copy()),
                        node_features=nf if with_nf else None, use_edge_features_as_node_feature=reduce)
        x = s.x.cpu()
        assert x.shape == (N, k + bs + (bs * bs if reduce != "disable" else 0))
        if with_nf:
            assert_same_bits(x[:, :k], nf, "node_features columns")
        want_mask = np.ones((N, bs), np.float32) if mask is None else mask.astype(np.float32).reshape(N, bs)
        assert_same_bits(x[:, k:k + bs], want_mask, "mask columns")
        assert_same_bits(s.mask, want_mask, "mask")
        if reduce != "disable":
            want = _scatter(s.edge_index.cpu(), s.edge_attr.cpu(), N, reduce)
            assert_same_bits(x[:, k + bs:], want, f"reduce {reduce}")
            if name == "unsym":
                assert torch.all(x[UNREFERENCED, k + bs:] == 0)


@pytest.mark.parametrize("name, dtype", [("poisson", np.float64), ("kuhn23", np.float32), ("arrow", np.float64),
                                         ("elast", np.float64)])
def test_reuse(gpu_ctx, name, dtype):
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    A, bs = matrix(name, dtype)
    mask64, nf = inputs(name)
    opts = dict(mask=mask64, node_features=nf, use_edge_features_as_node_feature="mean", normalize_matrix="mean")
    Ad = device_matrix(name, dtype)
    sampler = DeviceSampler(Ad, **opts)
    fields = ("x", "edge_attr", "matrix_values", "mask") + DIAG_FIELDS
    first = sampler.sample()
    kept = {f: getattr(first, f).clone() for f in fields}
    scale1 = first.matrix_scale
    second = sampler.sample()
    assert second.matrix_scale == scale1
    for f in fields:
        assert_same_bits(getattr(second, f), kept[f], f"second call: {f}")
    # new values on the same pattern
    ei_ptr = sampler.edge_index.data_ptr()
    vals = (2.5 * A.data).astype(dtype)
    Ad.set_values(vals.reshape(-1))
    third = sampler.sample()
    assert third.edge_index is sampler.edge_index and third.edge_index.data_ptr() == ei_ptr
    A2 = A.copy()
    A2.data = vals.astype(np.float64)
    fresh = make_sample(DeviceMatrix.from_scipy(A2, dtype=dtype, block_size=bs), **opts)
    assert third.matrix_scale == fresh.matrix_scale and third.matrix_scale != scale1
    assert torch.equal(third.edge_index, fresh.edge_index)
    for f in fields:
        assert_same_bits(getattr(third, f), getattr(fresh, f), f"after set_values: {f}")
    # another size or entry count
    other = DeviceMatrix.from_scipy(sp.identity(A.shape[0] + 3, format="csr"), dtype=dtype)
    with pytest.raises(ValueError, match="the sampler was built for"):
        sampler.sample(A=other)


def test_training_sample_has_a_masked_residual(gpu_ctx):
    mask64, _ = inputs("poisson")
    torch.manual_seed(0)
    s = make_sample(device_matrix("poisson", np.float64), mask=mask64, is_inference=False)
    assert s.residual.is_cuda and s.residual.shape == (63, 1)
    assert torch.all(s.residual[s.mask == 0] == 0) and torch.any(s.residual != 0)


def _raw_sample(Ad, desc, n_x, with_nf=False):
    """lspcg_mat_sample on sentinel-filled outputs: (code, every output still the sentinel)."""
    dev = Ad.ctx.torch_device
    bs = Ad.block_size
    N, E = Ad.n // bs, max(Ad.nnzb, 1)
    outs = [torch.full((n,), -7.0, dtype=torch.float32, device=dev) for n in (n_x, E * bs * bs, Ad.n, Ad.n, Ad.n)]
    scale = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    nf = torch.zeros((N, 3), dtype=torch.float32, device=dev) if with_nf else None
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = _lib.load().lspcg_mat_sample(Ad.ctx.handle, Ad.handle, C.byref(desc), None, _lib.F32, p(nf),
                                      *[p(t) for t in outs], p(scale))
    torch.cuda.synchronize()
    return rc, all(bool(torch.all(t == -7.0)) for t in outs + [scale])


def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix

    D = _lib.lspcg_sample_desc
    ok = device_matrix("poisson", np.float64)
    empty = DeviceMatrix.from_scipy(sp.csr_matrix((4, 4)), dtype=np.float64)
    bsr = device_matrix("elast", np.float64)
    cases = [
        (empty, D(_lib.NORM["mean"], 1, 0, 0), False, _lib.ERR_ARG),         # E = 0
        (ok, D(_lib.NORM["mean"], 0, 0, 0), False, _lib.ERR_ARG),            # F_in = 0
        (ok, D(7, 1, 0, 0), False, _lib.ERR_ARG),                            # unknown normalize
        (ok, D(_lib.NORM["mean"], 1, 9, 0), False, _lib.ERR_ARG),            # unknown reduce
        (ok, D(_lib.NORM["mean"], 1, 0, 3), False, _lib.ERR_ARG),            # node_in > 0, no node_features
        (bsr, D(_lib.NORM["l1"], 1, 0, 0), False, _lib.ERR_UNSUPPORTED),     # l1 on BSR 3x3
    ]
    for Ad, desc, with_nf, code in cases:
        rc, untouched = _raw_sample(Ad, desc, n_x=Ad.n * 16, with_nf=with_nf)
        assert rc == code and untouched, (rc, code, untouched, _lib.last_error())
    rc, untouched = _raw_sample(ok, D(_lib.NORM["mean"], 1, 0, 0), n_x=ok.n)  # the same call, accepted
    assert rc == _lib.OK and not untouched
    with pytest.raises(ValueError, match="empty matrix"):
        make_sample(empty)
