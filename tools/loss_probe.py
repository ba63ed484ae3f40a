"""The fused training objective (loss.spai_loss -> lspcg_graph_spai_loss) against the same chain
composed from torch ops on the same GPU (index_add / bmm with torch autograd -- the stand-in for
the reference's PyG path), at kuhn101 (b = 1) and the C4 elasticity box (b = 3), fp32.

Timed with device events after a warm-up, one event pair per call, median and spread over the
repeats:  fused loss + gradient, fused forward only, torch loss + gradient, torch forward only.
GB/s are the byte model below (compulsory traffic: every array once per kernel that touches it)
over the fused medians.  Writes one JSON document (--out) and prints it.

    python tools/loss_probe.py --out profiles/loss_probe.json [--small]
"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from learningsparsepreconditioner4gpu_amd import problems as P  # noqa: E402
from learningsparsepreconditioner4gpu_amd.data import GraphSample  # noqa: E402
from learningsparsepreconditioner4gpu_amd.loss import spai_loss  # noqa: E402

EPS = 3e-3


def byte_model(N, E, b, s, grad):
    """Compulsory bytes of one call (mask given, no diag).  One row-sum SpMV reads perm + other
    (8 B per edge), the values, the row pointers, x and the mask, and writes y."""
    n = N * b
    spmv = E * (8 + b * b * s) + 4 * (N + 1) + 3 * n * s
    fwd = 3 * spmv + n * s + 2 * n * s  # + r in the second pass (ε r), q and r in the reduction
    if not grad:
        return fwd
    gq = 4 * n * s                                  # q, r, mask -> gq
    edge = E * (8 + b * b * s) + 4 * n * s          # both ends, dL out, gy / t / r / gtm gathered
    return fwd + gq + 2 * spmv + edge


def torch_spmv(X, ei, A, mask, transpose=False):
    src, dst = (ei[0], ei[1]) if transpose else (ei[1], ei[0])
    blk = A.transpose(1, 2) if transpose else A
    out = torch.zeros_like(X).index_add(0, dst, torch.bmm(blk, X[src].unsqueeze(-1)).squeeze(-1))
    return out * mask


def torch_loss(batch, L, ptr):
    r, ei, m = batch.residual, batch.edge_index, batch.mask
    t = torch_spmv(r, ei, L, m, True)
    d = torch_spmv(t, ei, L, m) + EPS * r
    q = torch_spmv(d, ei, batch.matrix_values, m)
    loss = 0.0
    for b, e in zip(ptr[:-1], ptr[1:]):
        loss = loss + ((q[b:e] - r[b:e]) ** 2).sum() / ((r[b:e] ** 2).sum() + 1e-6)
    return loss / (len(ptr) - 1)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "p90_ms": float(np.percentile(ms, 90)),
            "repeats": repeats}


def problem(name, small):
    if name == "kuhn101":
        A = P.kuhn_laplacian(11 if small else 101)
        b, mask = 1, np.ones((A.shape[0], 1))
    else:
        A, mask, _ = P.elasticity_box(*((12, 6, 6) if small else ()))
        b, mask = 3, np.asarray(mask, dtype=np.float64).reshape(-1, 3)
    g = P.to_block_graph(A, b)
    vals = g.block_values / np.mean(np.abs(g.block_values))  # make_data's "mean" normalisation
    gen = torch.Generator().manual_seed(0)
    m = torch.tensor(mask, dtype=torch.float32)
    N, E = g.num_nodes, g.edge_index.shape[1]
    s = GraphSample(x=m, edge_index=torch.tensor(g.edge_index), edge_attr=torch.zeros(E, 1), mask=m,
                    matrix_values=torch.tensor(vals, dtype=torch.float32).reshape(E, b, b), block_size=b,
                    residual=torch.randn(N, b, generator=gen) * m)
    boo = 0.05 * torch.randn(E, b, b, generator=gen)
    return s, boo, N, E, b


def run(name, small, warmup, repeats):
    batch, boo, N, E, b = problem(name, small)
    batch, boo = batch.to("cuda"), boo.cuda()
    ptr = batch.ptr.tolist()
    L = boo.clone().requires_grad_(True)

    def fused_grad():
        L.grad = None
        spai_loss(batch, L, EPS).backward()

    def fused_fwd():
        with torch.no_grad():
            spai_loss(batch, boo, EPS)

    def torch_grad():
        L.grad = None
        torch_loss(batch, L, ptr).backward()

    def torch_fwd():
        with torch.no_grad():
            torch_loss(batch, boo, ptr)

    # same results first (loss and gradient), then the times
    fused_grad()
    lf, gf = float(spai_loss(batch, boo, EPS)), L.grad.clone()
    torch_grad()
    lt, gt = float(torch_loss(batch, boo, ptr)), L.grad.clone()
    dl = abs(lf - lt) / abs(lt)
    dg = float((gf - gt).abs().max() / gt.abs().max())
    assert dl <= 1e-4 and dg <= 1e-4, (name, dl, dg)
    out = {"name": name, "N": N, "E": E, "block_size": b, "dtype": "fp32", "loss": lf, "loss_rel_diff_vs_torch": dl,
           "grad_rel_diff_vs_torch": dg}
    for key, fn in (("fused_loss_grad", fused_grad), ("fused_forward", fused_fwd), ("torch_loss_grad", torch_grad),
                    ("torch_forward", torch_fwd)):
        out[key] = timed(fn, warmup, repeats)
    for key, grad in (("fused_loss_grad", True), ("fused_forward", False)):
        nbytes = byte_model(N, E, b, 4, grad)
        out[key]["model_bytes"] = nbytes
        out[key]["model_GBps"] = nbytes / (out[key]["median_ms"] * 1e-3) / 1e9
    out["speedup_loss_grad"] = out["torch_loss_grad"]["median_ms"] / out["fused_loss_grad"]["median_ms"]
    out["speedup_forward"] = out["torch_forward"]["median_ms"] / out["fused_forward"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny meshes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loss_probe needs the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "small": args.small,
           "results": [run(n, args.small, args.warmup, args.repeats) for n in ("kuhn101", "c4_elasticity")]}
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
