"""The training objective on the GPU: lspcg_graph_spai_loss / lspcg_graph_spmv_grad_vals, the
autograd paths of GraphSpmv / AATPE, loss.py, data.collate and the workspaces' shared_step.

The reference here is an fp64 restatement of the reference project's chain with plain torch ops on
the CPU (``zeros.index_add(0, dst, bmm(blk, X[src]))``) and torch autograd for every gradient.

Bounds: fp64 inputs 1e-12 relative to the reference's max (the project's fp64 bound); fp32 inputs
``max(1e-5, 4 * e32)`` where e32 is the error of torch's own CPU fp32 autograd of the same
restatement against the fp64 one on the same inputs (1e-5 is the project's fp32 bound).
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 3e-3
N, E = 1501, 9000
PTR = [0, 300, 301, 365, 1501]


# ---- the fp64 CPU reference -------------------------------------------------------------------
def ref_spmv(X, ei, A, mask=None, transpose=False):
    src, dst = (ei[0], ei[1]) if transpose else (ei[1], ei[0])
    blk = A.transpose(1, 2) if transpose else A
    out = torch.zeros_like(X).index_add(0, dst, torch.bmm(blk, X[src].unsqueeze(-1)).squeeze(-1))
    return out if mask is None else out * mask


def ref_aatpe(x, ei, L, eps, mask=None, diag=None):
    t = ref_spmv(x, ei, L, mask, transpose=True)
    if diag is not None:
        t = t * diag
    y = ref_spmv(t, ei, L, mask)
    ex = eps * x
    return y + (ex * diag if diag is not None else ex)


def ref_loss_of_d(d, ei, A, r, mask, ptr, kind, leps=1e-6):
    q = ref_spmv(d, ei, A, mask)
    if kind == "mse":
        return ((q - r) ** 2).mean()
    loss = 0.0
    for b, e in zip(ptr[:-1], ptr[1:]):
        loss = loss + ((q[b:e] - r[b:e]) ** 2).sum() / ((r[b:e] ** 2).sum() + leps)
    return loss / (len(ptr) - 1)


def ref_loss(L, ei, A, r, mask, diag, ptr, kind, eps=EPS):
    return ref_loss_of_d(ref_aatpe(r, ei, L, eps, mask, diag), ei, A, r, mask, ptr, kind)


def ref_loss_and_grad(c, diag, kind, dtype=torch.float64):
    L = c.L.to(dtype).clone().requires_grad_(True)  # the cached inputs stay as they are
    loss = ref_loss(L, c.ei, c.A.to(dtype), c.r.to(dtype), c.mask.to(dtype), None if diag is None else diag.to(dtype),
                    c.ptr, kind)
    loss.backward()
    return loss.detach().double(), L.grad.double()


# ---- inputs (built once per (b, layout), never modified) ---------------------------------------
def _graph(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei[:, : e // 10] = ei[:, e // 2: e // 2 + e // 10]  # duplicated (row, col) pairs, as test_gpu_graph._graph
    return ei


@functools.lru_cache(maxsize=None)
def case(bs, layout="mixed"):
    """fp64 CPU inputs.  layouts: "mixed" (a one-node graph, boundaries off wave multiples),
    "masked" (graph 2 has every row masked: ‖r_g‖² = 0), "noedge" (graph 2 touches no edge)."""
    ei = _graph(N, E, 100 + bs)
    g = torch.Generator().manual_seed(17 + bs)
    if layout == "noedge":
        inside = (ei >= PTR[2]) & (ei < PTR[3])
        ei = torch.where(inside, ei + 100, ei)
    mask = (torch.rand(N, bs, generator=g) > 0.2).double()
    if layout == "masked":
        mask[PTR[2]:PTR[3]] = 0.0
    r = torch.randn(N, bs, generator=g, dtype=torch.float64) * mask
    L = 0.3 * torch.randn(E, bs, bs, generator=g, dtype=torch.float64)
    A = torch.randn(E, bs, bs, generator=g, dtype=torch.float64)
    diag = torch.rand(N, bs, generator=g, dtype=torch.float64) + 0.5
    return types.SimpleNamespace(bs=bs, ei=ei, mask=mask, r=r, L=L, A=A, diag=diag, ptr=list(PTR))


def gpu_batch(c, dtype):
    return types.SimpleNamespace(residual=c.r.to(dtype).cuda(), edge_index=c.ei.cuda(), mask=c.mask.to(dtype).cuda(),
                                 matrix_values=c.A.to(dtype).cuda(), ptr=torch.tensor(c.ptr, dtype=torch.int64))


def gpu_loss_and_grad(c, diag, kind, dtype, batch=None):
    from learningsparsepreconditioner4gpu_amd.loss import spai_loss

    batch = gpu_batch(c, dtype) if batch is None else batch
    boo = c.L.to(dtype).cuda().requires_grad_(True)
    loss = spai_loss(batch, boo, EPS, diag=None if diag is None else diag.to(dtype).cuda(), kind=kind)
    loss.backward()
    return loss.detach(), boo.grad


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def check(got, ref, dtype, ref32=None, what=""):
    """fp64: 1e-12; fp32: max(1e-5, 4 * e32) with e32 = torch's CPU fp32 error on the same inputs."""
    err = rel(got, ref)
    if dtype == torch.float64:
        bound = 1e-12
    else:
        e32 = rel(ref32, ref)
        bound = max(1e-5, 4 * e32)
        print(f"{what}: e32 {e32:.3e}")
    print(f"{what}: err {err:.3e} bound {bound:.3e}")
    assert np.isfinite(err) and err <= bound, (what, err, bound)


# ---- the fused loss and dL ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["relative", "mse"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("with_diag", [False, True])
@pytest.mark.parametrize("bs", [1, 3])
def test_spai_loss_and_grad(gpu_ctx, bs, with_diag, dtype, kind):
    c = case(bs)
    diag = c.diag if with_diag else None
    loss, dL = gpu_loss_and_grad(c, diag, kind, dtype)
    rl, rg = ref_loss_and_grad(c, diag, kind)
    l32, g32 = ref_loss_and_grad(c, diag, kind, torch.float32) if dtype == torch.float32 else (None, None)
    assert loss.dtype == dtype and dL.dtype == dtype and dL.shape == c.L.shape
    check(loss, rl, dtype, l32, "loss")
    check(dL, rg, dtype, g32, "dL")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("bs", [1, 3])
@pytest.mark.parametrize("layout", ["masked", "noedge"])
def test_spai_loss_degenerate_graphs(gpu_ctx, layout, bs, dtype):
    """A graph whose rows are all masked (‖r_g‖² = 0: its term is finite and the reference's) and
    a graph that no edge touches."""
    c = case(bs, layout)
    loss, dL = gpu_loss_and_grad(c, c.diag, "relative", dtype)
    rl, rg = ref_loss_and_grad(c, c.diag, "relative")
    l32, g32 = ref_loss_and_grad(c, c.diag, "relative", torch.float32) if dtype == torch.float32 else (None, None)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dL).all())
    check(loss, rl, dtype, l32, f"{layout} loss")
    check(dL, rg, dtype, g32, f"{layout} dL")


@pytest.mark.parametrize("kind", ["relative", "mse"])
@pytest.mark.parametrize("bs", [1, 3])
def test_directional_finite_difference(gpu_ctx, bs, kind):
    from learningsparsepreconditioner4gpu_amd.loss import spai_loss

    c = case(bs)
    batch = gpu_batch(c, torch.float64)
    diag = c.diag.cuda()
    _, dL = gpu_loss_and_grad(c, c.diag, kind, torch.float64, batch)
    V = torch.randn(c.L.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64).cuda()
    h = 1e-5
    L = c.L.cuda()
    with torch.no_grad():
        fd = (spai_loss(batch, L + h * V, EPS, diag=diag, kind=kind)
              - spai_loss(batch, L - h * V, EPS, diag=diag, kind=kind)) / (2 * h)
    dd = (dL * V).sum()
    err = float((fd - dd).abs() / dd.abs())
    print(f"fd {float(fd):.12e} <dL,V> {float(dd):.12e} rel {err:.3e}")
    assert err <= 1e-6, err


# ---- autograd modules -----------------------------------------------------------------------------
def _module_grads(fn, X, A, w):
    X = X.clone().requires_grad_(True)
    A = A.clone().requires_grad_(True)
    y = fn(X, A)
    (y * w).sum().backward()
    return y.detach(), X.grad, A.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("bs", [1, 3])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("transpose", [False, True])
def test_graph_spmv_autograd(gpu_ctx, transpose, with_mask, bs, dtype):
    from learningsparsepreconditioner4gpu_amd.nn import GraphSpmv

    c = case(bs)
    g = torch.Generator().manual_seed(23)
    X = torch.randn(N, bs, generator=g, dtype=torch.float64)
    w = torch.randn(N, bs, generator=g, dtype=torch.float64)
    mask = c.mask if with_mask else None
    ref = _module_grads(lambda x, a: ref_spmv(x, c.ei, a, mask, transpose), X, c.A, w)
    ref32 = (_module_grads(lambda x, a: ref_spmv(x, c.ei, a, None if mask is None else mask.float(), transpose),
                           X.float(), c.A.float(), w.float()) if dtype == torch.float32 else (None,) * 3)
    mod, ei, m = GraphSpmv(transpose), c.ei.cuda(), None if mask is None else mask.to(dtype).cuda()
    got = _module_grads(lambda x, a: mod(x, ei, a, m), X.to(dtype).cuda(), c.A.to(dtype).cuda(), w.to(dtype).cuda())
    for name, a, b, b32 in zip(("y", "gX", "gA"), got, ref, ref32):
        assert a.dtype == dtype
        check(a, b, dtype, b32, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("bs", [1, 3])
def test_aatpe_autograd(gpu_ctx, bs, dtype):
    from learningsparsepreconditioner4gpu_amd.nn import AATPE

    c = case(bs)
    g = torch.Generator().manual_seed(29)
    X = torch.randn(N, bs, generator=g, dtype=torch.float64)
    w = torch.randn(N, bs, generator=g, dtype=torch.float64)
    ref = _module_grads(lambda x, a: ref_aatpe(x, c.ei, a, EPS, c.mask, c.diag), X, c.L, w)
    ref32 = (_module_grads(lambda x, a: ref_aatpe(x, c.ei, a, EPS, c.mask.float(), c.diag.float()), X.float(),
                           c.L.float(), w.float()) if dtype == torch.float32 else (None,) * 3)
    mod, ei, m, d = AATPE(EPS), c.ei.cuda(), c.mask.to(dtype).cuda(), c.diag.to(dtype).cuda()
    got = _module_grads(lambda x, a: mod(x, ei, a, m, d), X.to(dtype).cuda(), c.L.to(dtype).cuda(), w.to(dtype).cuda())
    for name, a, b, b32 in zip(("y", "gX", "gL"), got, ref, ref32):
        check(a, b, dtype, b32, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ["relative", "mse"])
@pytest.mark.parametrize("bs", [1, 3])
def test_composed_equals_fused(gpu_ctx, bs, kind, dtype):
    """The loss module fed the differentiable AATPE's output = spai_loss (loss and dL)."""
    from learningsparsepreconditioner4gpu_amd.loss import create_loss_item
    from learningsparsepreconditioner4gpu_amd.nn import AATPE

    c = case(bs)
    batch = gpu_batch(c, dtype)
    fl, fg = gpu_loss_and_grad(c, c.diag, kind, dtype, batch)
    boo = c.L.to(dtype).cuda().requires_grad_(True)
    d = AATPE(EPS)(batch.residual, batch.edge_index, boo, mask=batch.mask, diag=c.diag.to(dtype).cuda())
    mod = create_loss_item("RelativeL2Loss_ANorm" if kind == "relative" else "L2Loss_ANorm", batch_less=False,
                           block_size=bs)
    cl = mod(batch, d, boo)
    cl.backward()
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    print(f"loss {rel(cl, fl):.3e} dL {rel(boo.grad, fg):.3e}")
    assert rel(cl, fl) <= tol and rel(boo.grad, fg) <= tol


def test_sqr_out_false_composes(gpu_ctx):
    """sqr_out=False has no fused form: the module path serves it (loss.py:22-25)."""
    from learningsparsepreconditioner4gpu_amd.loss import RelativeL2Loss_ANorm
    from learningsparsepreconditioner4gpu_amd.nn import AATPE

    c = case(1)
    batch = gpu_batch(c, torch.float64)
    boo = c.L.cuda().requires_grad_(True)
    d = AATPE(EPS)(batch.residual, batch.edge_index, boo, mask=batch.mask)
    loss = RelativeL2Loss_ANorm(False, 1, sqr_out=False)(batch, d, boo)
    loss.backward()
    L = c.L.clone().requires_grad_(True)
    q = ref_spmv(ref_aatpe(c.r, c.ei, L, EPS, c.mask), c.ei, c.A, c.mask)
    rl = sum(torch.linalg.norm(q[b:e] - c.r[b:e]) / (torch.linalg.norm(c.r[b:e]) + 1e-6)
             for b, e in zip(c.ptr[:-1], c.ptr[1:])) / (len(c.ptr) - 1)
    rl.backward()
    assert rel(loss, rl) <= 1e-12 and rel(boo.grad, L.grad) <= 1e-12


def test_deterministic(gpu_ctx):
    for bs, dtype in ((1, torch.float32), (3, torch.float64)):
        c = case(bs)
        batch = gpu_batch(c, dtype)
        l1, g1 = gpu_loss_and_grad(c, c.diag, "relative", dtype, batch)
        l2, g2 = gpu_loss_and_grad(c, c.diag, "relative", dtype, batch)
        assert torch.equal(l1, l2) and torch.equal(g1, g2)


# ---- the existing path is untouched ---------------------------------------------------------------
@pytest.mark.parametrize("bs", [1, 3])
def test_no_grad_path_unchanged(gpu_ctx, bs):
    from learningsparsepreconditioner4gpu_amd import _lib
    from learningsparsepreconditioner4gpu_amd.nn import _GRAPHS, AATPE, GraphSpmv
    from learningsparsepreconditioner4gpu_amd.sparse import _ptr

    c = case(bs)
    dt = torch.float32
    X, A, m, d, ei = c.r.to(dt).cuda(), c.L.to(dt).cuda(), c.mask.to(dt).cuda(), c.diag.to(dt).cuda(), c.ei.cuda()
    h = _GRAPHS.get(ei, N, bs)
    for transpose in (False, True):
        direct = torch.empty_like(X)
        _lib.call("lspcg_graph_spmv", h, _ptr(A), _lib.F32, int(transpose), _ptr(X), _ptr(m), _ptr(direct))
        y = GraphSpmv(transpose)(X, ei, A, m)
        assert not y.requires_grad and torch.equal(y, direct)
        with torch.no_grad():
            y = GraphSpmv(transpose)(X.clone().requires_grad_(True), ei, A.clone().requires_grad_(True), m)
        assert not y.requires_grad and torch.equal(y, direct)
    t, direct = torch.empty_like(X), torch.empty_like(X)
    _lib.call("lspcg_graph_aatpe", h, _ptr(A), _lib.F32, EPS, _ptr(X), _ptr(m), _ptr(d), _ptr(t), _ptr(direct))
    y = AATPE(EPS)(X, ei, A, m, d)
    assert not y.requires_grad and torch.equal(y, direct)
    with torch.no_grad():
        y = AATPE(EPS)(X.clone().requires_grad_(True), ei, A.clone().requires_grad_(True), m, d)
    assert not y.requires_grad and torch.equal(y, direct)
    # ... and the autograd path computes the same forward bits
    y = AATPE(EPS)(X, ei, A.clone().requires_grad_(True), m, d)
    assert y.requires_grad and torch.equal(y.detach(), direct)


# ---- the edge kernel's stride loop ----------------------------------------------------------------
def test_grid_stride_edges(gpu_ctx):
    """b = 1, fp32, one graph, E just past the edge kernel's launch-wide thread count (8192 x 256)."""
    n, e = 60000, 8192 * 256 + 1000
    g = torch.Generator().manual_seed(41)
    c = types.SimpleNamespace(bs=1, ei=_graph(n, e, 43), ptr=[0, n])
    c.mask = (torch.rand(n, 1, generator=g) > 0.2).double()
    c.r = torch.randn(n, 1, generator=g, dtype=torch.float64) * c.mask
    c.L = 0.1 * torch.randn(e, 1, 1, generator=g, dtype=torch.float64)
    c.A = 0.3 * torch.randn(e, 1, 1, generator=g, dtype=torch.float64)
    loss, dL = gpu_loss_and_grad(c, None, "relative", torch.float32)
    rl, rg = ref_loss_and_grad(c, None, "relative")
    l32, g32 = ref_loss_and_grad(c, None, "relative", torch.float32)
    check(loss, rl, torch.float32, l32, "loss")
    check(dL, rg, torch.float32, g32, "dL")
    check(dL[8192 * 256:], rg[8192 * 256:], torch.float32, g32[8192 * 256:], "dL past the first stride")


# ---- end to end: a torch MLP trained against the GPU loss -----------------------------------------
def _training_samples():
    import scipy.sparse as sp

    from learningsparsepreconditioner4gpu_amd import problems as P
    from learningsparsepreconditioner4gpu_amd.dataset import RawData, make_data

    A = sp.csr_matrix(P.kuhn_laplacian(5))
    g = P.to_block_graph(A, 1)
    n = g.num_nodes
    out = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        raw = RawData(block_values=g.block_values, diagonals=A.diagonal().reshape(-1, 1), edge_index=g.edge_index,
                      node_features=None, lhs=None, rhs=None, mask=np.ones((n, 1)), num_nodes=n, block_size=1)
        out.append(make_data(raw, is_inference=False))
    return out


def _sgd_losses(batch, loss_of_boo, steps=5, lr=0.01):
    torch.manual_seed(0)
    mlp = torch.nn.Sequential(torch.nn.Linear(batch.edge_attr.shape[1], 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))
    opt = torch.optim.SGD(mlp.parameters(), lr=lr)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = loss_of_boo(0.1 * mlp(batch.edge_attr).reshape(-1, 1, 1))  # small L: the loss is quartic in it
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    return losses


def test_end_to_end_sgd(gpu_ctx):
    from learningsparsepreconditioner4gpu_amd.data import collate
    from learningsparsepreconditioner4gpu_amd.loss import spai_loss

    batch = collate(_training_samples())
    ptr = batch.ptr.tolist()
    assert len(ptr) == 3
    dev = batch.to("cuda")
    gpu = _sgd_losses(batch, lambda boo: spai_loss(dev, boo.cuda(), EPS).cpu())
    r, A, m = batch.residual.double(), batch.matrix_values.double(), batch.mask.double()
    cpu = _sgd_losses(batch, lambda boo: ref_loss(boo.double(), batch.edge_index, A, r, m, None, ptr, "relative"))
    print("gpu", gpu, "cpu", cpu)
    for a, b in zip(gpu, cpu):
        assert abs(a - b) <= 1e-4 * abs(b), (gpu, cpu)
    assert gpu[5] < gpu[0]


# ---- collate and shared_step ----------------------------------------------------------------------
def test_collate_and_shared_step(gpu_ctx):
    from learningsparsepreconditioner4gpu_amd.data import collate
    from learningsparsepreconditioner4gpu_amd.loss import spai_loss
    from learningsparsepreconditioner4gpu_amd.workspace import ScaledInferenceWorkspace, SimpleInferenceWorkspace

    s1, s2 = _training_samples()
    batch = collate([s1, s2])
    ws = SimpleInferenceWorkspace(node_features=s1.x.shape[1], edge_features=s1.edge_attr.shape[1], epsilon=EPS)
    boo, loss = ws.shared_step(batch)
    assert boo.shape == (batch.edge_index.shape[1], 1, 1) and not loss.requires_grad
    parts = [float(ws.shared_step(s)[1]) for s in (s1, s2)]
    assert abs(float(loss) - sum(parts) / 2) <= 1e-5 * abs(float(loss)), (float(loss), parts)
    ptr = batch.ptr.tolist()
    ref = ref_loss(boo.double().cpu(), batch.edge_index, batch.matrix_values.double(), batch.residual.double(),
                   batch.mask.double(), None, ptr, "relative")
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    mse = SimpleInferenceWorkspace(node_features=s1.x.shape[1], edge_features=s1.edge_attr.shape[1], epsilon=EPS,
                                   loss_name="l2loss_anorm")
    ref = ref_loss(boo.double().cpu(), batch.edge_index, batch.matrix_values.double(), batch.residual.double(),
                   batch.mask.double(), None, ptr, "mse")
    assert abs(float(mse.shared_step(batch)[1]) - float(ref)) <= 1e-5 * abs(float(ref))
    # the scaled workspace passes inv_diag
    sws = ScaledInferenceWorkspace(node_features=s1.x.shape[1], edge_features=s1.edge_attr.shape[1], epsilon=EPS)
    sboo, sloss = sws.shared_step(batch)
    dev = batch.to("cuda")
    assert torch.equal(sboo, boo)  # same seed, same GNN
    assert torch.equal(sloss, spai_loss(dev, sboo, EPS, diag=dev.inv_diag))
    ref = ref_loss(sboo.double().cpu(), batch.edge_index, batch.matrix_values.double(), batch.residual.double(),
                   batch.mask.double(), batch.inv_diag.double(), ptr, "relative")
    assert abs(float(sloss) - float(ref)) <= 1e-5 * abs(float(ref))
    assert abs(float(sloss) - float(loss)) > 1e-3 * abs(float(loss))


# ---- C ABI ----------------------------------------------------------------------------------------
def test_abi_errors_and_empty(gpu_ctx):
    from learningsparsepreconditioner4gpu_amd import _lib
    from learningsparsepreconditioner4gpu_amd.nn import _GRAPHS
    from learningsparsepreconditioner4gpu_amd.sparse import _ptr

    c = case(1)
    dt = torch.float64
    L, A, r, m, ei = c.L.cuda(), c.A.cuda(), c.r.cuda(), c.mask.cuda(), c.ei.cuda()
    h = _GRAPHS.get(ei, N, 1)
    out = torch.zeros((), dtype=dt, device="cuda")
    dL = torch.empty_like(L)
    ptr = torch.tensor(c.ptr, dtype=torch.int64)

    def call(Lp=_ptr(L), dtype=_lib.F64, rp=_ptr(r), p=ptr, outp=_ptr(out), dLp=_ptr(dL)):
        _lib.call("lspcg_graph_spai_loss", h, Lp, _ptr(A), dtype, EPS, rp, _ptr(m), None, C.c_void_p(p.data_ptr()),
                  p.numel() - 1, 0, 1e-6, outp, dLp)

    call()  # the valid call, host ptr
    good = out.clone()
    call(p=ptr.cuda())  # a device ptr gives the same
    assert torch.equal(out, good)
    for kw, word in ((dict(rp=None), "NULL"), (dict(outp=None), "NULL"), (dict(dtype=7), "dtype"),
                     (dict(p=torch.tensor([0, 400, 300, N])), "non-decreasing"),
                     (dict(p=torch.tensor([0, 300, N - 1])), "non-decreasing"),
                     (dict(dLp=_ptr(L)), "alias")):
        with pytest.raises(_lib.LspcgError, match=word):
            call(**kw)
    with pytest.raises(_lib.LspcgError, match="NULL"):
        _lib.call("lspcg_graph_spmv_grad_vals", h, _lib.F64, 0, None, _ptr(r), _ptr(dL))
    with pytest.raises(_lib.LspcgError, match="dtype"):
        _lib.call("lspcg_graph_spmv_grad_vals", h, 5, 0, _ptr(r), _ptr(r), _ptr(dL))
    # N = 0: loss 0, nothing launched that indexes
    e0 = torch.zeros(2, 0, dtype=torch.int64, device="cuda")
    h0 = _GRAPHS.get(e0, 0, 1)
    z = torch.zeros(1, dtype=dt, device="cuda")
    out.fill_(7.0)
    p0 = torch.tensor([0, 0], dtype=torch.int64)
    _lib.call("lspcg_graph_spai_loss", h0, None, None, _lib.F64, EPS, _ptr(z), None, None, C.c_void_p(p0.data_ptr()),
              1, 0, 1e-6, _ptr(out), None)
    assert float(out) == 0.0
    # E = 0 with rows: L = A = 0, so q = 0 and every graph's term is ‖r_g‖² / (‖r_g‖² + eps)
    h1 = _GRAPHS.get(e0.clone(), 5, 1)
    r5 = torch.arange(1.0, 6.0, dtype=dt, device="cuda")
    p1 = torch.tensor([0, 2, 5], dtype=torch.int64)
    _lib.call("lspcg_graph_spai_loss", h1, None, None, _lib.F64, EPS, _ptr(r5), None, None, C.c_void_p(p1.data_ptr()),
              2, 0, 1e-6, _ptr(out), None)
    assert abs(float(out) - 0.5 * (5 / (5 + 1e-6) + 50 / (50 + 1e-6))) <= 1e-14
