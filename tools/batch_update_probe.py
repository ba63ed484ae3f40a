"""New values of A and L on a live lockstep batch against a fresh batch (measurement only, GPU box):
what a window's setup costs next to its solve, by either path.

    python tools/batch_update_probe.py [--out profiles/batch_update_probe.json] [--reps 5] [window:kind,kind ...]

Windows: heat_batch8 (infer.synthetic_dataset's C5 window), poisson8 (8 x Poisson 256^2) and bsr3 (the
BSR 3x3 elasticity window of tests/test_gpu_batch_kinds.py::test_kind_bsr3).  Every system has a
second matrix A2 = D A D on its pattern (D = diag(1 + 0.5 u)) and a factor of its own for each.
Per window and kind two sequences alternate in one process after a warm-up, `reps` times each:
  create  BatchedConjugateGradient on host matrices (upload, block-diagonal copies, views, tile maps;
          AINV(0) for ainv), then its first solve (which captures the graphs), then a repeat solve,
          then the release of the batch and its matrices (create_release_ms: a loop that creates a
          batch per window frees the one before; an update frees the matrices it replaces inside
          update_ms)
  update  BatchedConjugateGradient.update with the same host matrices on a batch that has solved the
          other set (upload, checks, value copy, refills; AINV(0) for ainv), then the first solve
          after it, then a repeat solve
Every figure is a host clock around work that ends in a device synchronise; the device times the
library reports (the update's events, the solves' events) stand beside it.  The sets alternate, so
every create and every update installs other values.  Passes: "f32_exact" rounds both sets through
fp32, as every matrix of the inference pipeline is, so the updates keep the graphs; "f64" keeps the
doubles of A2 against an fp32-exact A1 where A1 is exact, so an update may cross an exactness
transition.  Reported per figure: the median of the repeats with their minimum and maximum.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import scipy.sparse as sp
import torch

from learningsparsepreconditioner4gpu_amd import _lib
from learningsparsepreconditioner4gpu_amd import problems as P
from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient

DEFAULT = ["heat_batch8:ext_spai,ext_spai_scaled,diagonal,ainv", "poisson8:ext_spai,ext_spai_scaled,diagonal,ainv",
           "bsr3:ext_spai,ext_spai_scaled,diagonal,ainv"]
EPS = 3e-3


def csr(A):
    A = sp.csr_matrix(A).astype(np.float64)
    A.sort_indices()
    return A


def scaled(A, seed):
    d = 1.0 + 0.5 * np.random.default_rng(seed).uniform(size=A.shape[0])
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return sp.csr_matrix((d[rows] * A.data * d[A.indices], A.indices.copy(), A.indptr.copy()), shape=A.shape)


def factor(A, seed, scale, bs):
    """A factor on A's pattern (D^-1/2 plus small seeded off-diagonal entries), whole blocks for BSR."""
    rng = np.random.default_rng(seed)
    d = A.diagonal()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    vals = rng.normal(size=A.nnz) * scale / np.sqrt(np.abs(d[rows]) + 1e-12)
    diag = rows == A.indices
    vals[diag] = 1.0 / np.sqrt(np.abs(d[rows[diag]]) + 1e-12)
    L = sp.csr_matrix((vals, A.indices.copy(), A.indptr.copy()), shape=A.shape)
    return csr(sp.bsr_matrix(L, blocksize=(bs, bs))) if bs > 1 else L


def window(name):
    if name == "heat_batch8":  # infer.synthetic_dataset("heat_batch8")'s systems
        rng = np.random.default_rng(0)
        As = []
        for s in range(8):
            nv = int(rng.integers(400, 32000))
            k = max(4, int(round(nv ** (1 / 3))))
            As.append(P.heat_tet(k, k, max(4, nv // (k * k)), rho=float(rng.uniform(1e-4, 5e-4)), seed=s)[0])
        return [csr(A) for A in As], 1
    if name == "poisson8":
        return [csr(P.poisson2d_grid(256, 256, seed=k)[0]) for k in range(8)], 1
    if name == "bsr3":
        return [csr(P.elasticity_box(*dims)[0]) for dims in ((9, 5, 5), (12, 6, 5), (5, 4, 4))], 3
    raise KeyError(name)


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def probe(name, kinds, f32_exact, reps):
    A1, bs = window(name)
    sets = [A1, [scaled(A, 7 + k) for k, A in enumerate(A1)]]
    if f32_exact:
        for As in sets:
            for A in As:
                A.data = A.data.astype(np.float32).astype(np.float64)
    facs = [[factor(A, 10 * s + k, 0.02 if bs == 3 else 0.05, bs) for k, A in enumerate(As)] for s, As in enumerate(sets)]
    bvec = [torch.as_tensor(A @ np.random.default_rng(100 + k).normal(size=A.shape[0]), device="cuda")
            for k, A in enumerate(A1)]
    max_iter = 60 if bs == 3 else 0  # (test_kind_bsr3's bound)
    out = {}
    for kind in kinds:
        spai = kind in ("ext_spai", "ext_spai_scaled")

        def create(s):
            return BatchedConjugateGradient(sets[s], facs[s] if spai else None, EPS, block_size=bs, preconditioner=kind)

        def update(B, s):
            return B.update(sets[s], facs[s] if spai else None)

        def solve(B):
            xs = [torch.zeros_like(b) for b in bvec]
            res, t = B.solve(bvec, xs, rtol=1e-8, max_iter=max_iter)
            return [r[0] for r in res], t * 1e3

        try:
            B0 = create(0)  # (untimed: loads the kernels; its solves capture the graphs)
            solve(B0)
            update(B0, 1)
            solve(B0)
            update(B0, 0)
            solve(B0)
            col = {k: [] for k in ("create_ms", "create_release_ms", "create_first_solve_ms", "create_repeat_solve_ms",
                                   "create_first_solve_device_ms", "create_repeat_solve_device_ms", "update_ms",
                                   "update_device_ms", "update_first_solve_ms", "update_repeat_solve_ms",
                                   "update_first_solve_device_ms", "update_repeat_solve_device_ms")}
            kept, same_iters = [], True
            for r in range(reps):
                s = (r + 1) % 2
                t, Bf = clock(lambda: create(s))
                col["create_ms"].append(t)
                for tag in ("first", "repeat"):
                    t, (it_f, dev) = clock(lambda: solve(Bf))
                    col[f"create_{tag}_solve_ms"].append(t)
                    col[f"create_{tag}_solve_device_ms"].append(dev)
                hold = [Bf]
                del Bf
                t, _ = clock(hold.clear)  # the batch, its copies and the window's 2K matrix handles
                col["create_release_ms"].append(t)
                t, (dev, k) = clock(lambda: update(B0, s))
                col["update_ms"].append(t)
                col["update_device_ms"].append(dev * 1e3)
                kept.append(bool(k))
                for tag in ("first", "repeat"):
                    t, (it_u, dev) = clock(lambda: solve(B0))
                    col[f"update_{tag}_solve_ms"].append(t)
                    col[f"update_{tag}_solve_device_ms"].append(dev)
                same_iters = same_iters and it_u == it_f
            row = {k: stats(v) for k, v in col.items()}
            # a window's cost by either path: an update frees the previous window's matrices inside its
            # own clock, a create-per-window loop frees the previous batch as well (create_release_ms)
            row["create_total_ms"] = stats([a + b + c for a, b, c in zip(col["create_ms"], col["create_release_ms"],
                                                                         col["create_first_solve_ms"])])
            row["update_total_ms"] = stats([a + b for a, b in zip(col["update_ms"], col["update_first_solve_ms"])])
            row.update(graphs_kept=kept, iters=it_u, same_iters=same_iters, reps=reps, systems=len(A1),
                       rows=[int(A.shape[0]) for A in A1], block_size=bs)
            out[kind] = row
            del B0
        except _lib.LspcgError as e:  # a kind this window has no batch for: recorded, not hidden
            if e.code not in (_lib.ERR_BREAKDOWN, _lib.ERR_UNSUPPORTED, _lib.ERR_ARG):
                raise
            out[kind] = {"error": str(e)}
        print(json.dumps({"f32_exact" if f32_exact else "f64": {name: {kind: out[kind]}}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/batch_update_probe.json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", default="f32_exact,f64")
    ap.add_argument("items", nargs="*", default=DEFAULT)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5 (the medians are reported with their spread)")
    res = {}
    for mode in args.passes.split(","):
        res[mode] = {}
        for item in args.items:
            wl, _, kinds = item.partition(":")
            res[mode][wl] = probe(wl, kinds.split(",") if kinds else ["ext_spai"], mode == "f32_exact", args.reps)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
