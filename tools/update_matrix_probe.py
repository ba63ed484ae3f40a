"""New values of A on a live solver against a fresh solver (measurement only, GPU box): host clock
with the device drained, three repeats per path, both paths in one run.

    python tools/update_matrix_probe.py [--out profiles/update_matrix_probe.json] [workload:kind,kind ...]

Per workload and preconditioner kind, for a second matrix A2 = D A D on the first one's pattern
(D = diag(1 + 0.5 u)):
  fresh   DeviceMatrix.from_scipy(A2) + PreconditionedConjugateGradient (its set_ic / ainv0 included)
          [+ set_spai] (setup_ms), then the first solve (first_solve_ms)
  update  update_matrix(A2) on a solver that has solved A1 (host values through the checked
          set_values) [+ set_spai] (setup_ms), then the first solve, with the graphs_kept flag
  repeat  a further solve on the updated solver (three of them: the run's own spread)
  control a solver created on A2 and never updated, solved four times (never_updated_solves_ms): what
          a first solve and its repeats cost on a solver no update ever touched
The update path alternates between A2 and A1, so every update installs other values.  Two passes:
"f32_exact" rounds A2 through fp32, as every matrix of the inference pipeline is (a sample's
matrix_values are fp32), so A1 and A2 share the compact fp32 storage and the graphs survive; "f64"
keeps A2's full doubles, so every update crosses an fp32-exactness transition and drops them.
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
from learningsparsepreconditioner4gpu_amd.data import make_sample
from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient
from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix
from learningsparsepreconditioner4gpu_amd.workspace import SimpleInferenceWorkspace

# (IC(0) and AINV(0) factor scalar CSR only: the BSR 3x3 elasticity system has neither)
DEFAULT = ["kuhn101:ext_spai,diagonal,ic,ainv", "kuhn101rand:ext_spai,diagonal,ic,ainv",
           "delaunay27k:ext_spai,diagonal,ic,ainv", "bunny:ext_spai,diagonal,ic,ainv", "elasticity:ext_spai,diagonal"]
EPS = 3e-3


def scaled(A, seed=7):
    d = 1.0 + 0.5 * np.random.default_rng(seed).uniform(size=A.shape[0])
    out = A.copy()
    rows = np.repeat(np.arange(len(A.indptr) - 1), np.diff(A.indptr))
    if sp.isspmatrix_bsr(A):  # data[k, a, c] is entry (bs row_k + a, bs col_k + c)
        a = np.arange(A.blocksize[0])
        out.data = A.data * d[rows[:, None] * a.size + a][:, :, None] * d[A.indices[:, None] * a.size + a][:, None, :]
    else:
        out.data = d[rows] * A.data * d[A.indices]
    return out


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def probe(wl, kinds, f32_exact):
    A_raw, mask, feats, bs, e2n = P.workload(wl)
    smp = make_sample(A_raw, mask, node_features=feats, block_size=bs, use_edge_features_as_node_feature=e2n)
    d = smp.to("cuda")
    ws = SimpleInferenceWorkspace(node_features=smp.x.shape[1], edge_features=smp.edge_attr.shape[1], block_size=bs,
                                  seed=0)
    L, _ = ws.inference_step(d)
    A1 = ws.system_matrix(d).to_scipy()  # sorted CSR / BSR, as the solver's handle stores it
    A2 = scaled(A1)
    if f32_exact:
        A2.data = A2.data.astype(np.float32).astype(np.float64)
    n = A1.shape[0]
    b = torch.as_tensor(A1 @ np.random.default_rng(3).normal(size=n), device="cuda")
    out = {}
    for kind in kinds:
        def solve(s):
            x = torch.zeros_like(b)
            it, conv, _t = s.solve(b, x, rtol=1e-8)
            return it

        def fresh(M):
            s = PreconditionedConjugateGradient(DeviceMatrix.from_scipy(M, block_size=bs), device="cuda",
                                                preconditioner=kind, dtype=np.float64, block_size=bs)
            if kind == "ext_spai":
                s.set_spai(L, EPS, block_size=bs)
            return s

        def update(s, M):
            _t, kept = s.update_matrix(M)
            if kind == "ext_spai":
                s.set_spai(L, EPS, block_size=bs)
            return kept

        try:
            s0 = fresh(A1)  # (untimed: loads the kernels; its solve captures the graphs)
            solve(s0)
            rows = []
            for r in range(3):
                M = A2 if r % 2 == 0 else A1
                t_fs, sf = clock(lambda: fresh(M))
                t_f1, it_f = clock(lambda: solve(sf))
                del sf
                t_us, kept = clock(lambda: update(s0, M))
                t_u1, it_u = clock(lambda: solve(s0))
                rep = [clock(lambda: solve(s0))[0] for _ in range(3)]
                rows.append({"fresh": {"setup_ms": t_fs, "first_solve_ms": t_f1, "total_ms": t_fs + t_f1},
                             "update": {"setup_ms": t_us, "first_solve_ms": t_u1, "total_ms": t_us + t_u1,
                                        "graphs_kept": bool(kept)},
                             "repeat_solve_ms": rep, "iters_fresh": it_f, "iters_update": it_u})
            sc = fresh(A2)
            control = [clock(lambda: solve(sc))[0] for _ in range(4)]
            del sc
            out[kind] = {"rows": rows, "never_updated_solves_ms": control, "views": s0.views["A"]["columns"], "reorder": s0.reorder_info["applied"],
                         "n": n, "block_size": bs}
            del s0
        except _lib.LspcgError as e:  # a factorization that does not exist for this system: recorded, not hidden
            if e.code != _lib.ERR_BREAKDOWN:
                raise
            out[kind] = {"error": str(e)}
        print(json.dumps({"f32_exact" if f32_exact else "f64": {wl: {kind: out[kind]}}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/update_matrix_probe.json")
    ap.add_argument("items", nargs="*", default=DEFAULT)
    args = ap.parse_args()
    res = {"f32_exact": {}, "f64": {}}
    for mode in res:
        for item in args.items:
            wl, _, kinds = item.partition(":")
            res[mode][wl] = probe(wl, kinds.split(",") if kinds else ["ext_spai"], mode == "f32_exact")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
