"""Lockstep batch against one solve at a time for the preconditioner kinds beside ext_spai
(tools/batch_probe.py's protocol): the heat_batch8 and delaunay_batch8 windows (C5, the reference's
real sizes) solved as ONE ``BatchedConjugateGradient`` of kind none / diagonal / ext_spai_scaled /
ainv, and the same systems one after another through ``PreconditionedConjugateGradient`` in the
same process.  Per (window, kind): after a warm-up solve (graphs built, caches warm), the best of
``--repeat`` solves -- host wall time around the synchronised call(s) and the device time from the
calls' own t_solve_ms -- the iterations per system and the us per lockstep iteration.  Writes one
JSON document (default profiles/batch_kinds_probe.json) and prints each record as a line."""
import argparse
import json
import sys
import time

import numpy as np
import torch

KINDS = ("none", "diagonal", "ext_spai_scaled", "ainv")


def best_of(repeat, fn):
    wall = dev = out = None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o, d = fn()
        torch.cuda.synchronize()
        w = time.perf_counter() - t0
        if wall is None or w < wall:
            wall, dev, out = w, d, o
    return wall, dev, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="heat_batch8,delaunay_batch8")
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="profiles/batch_kinds_probe.json")
    args = ap.parse_args(argv)
    sys.path.insert(0, ".")
    from learningsparsepreconditioner4gpu_amd._lib import LspcgError
    from learningsparsepreconditioner4gpu_amd.infer import synthetic_dataset
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient, PreconditionedConjugateGradient
    from learningsparsepreconditioner4gpu_amd.workspace import ScaledInferenceWorkspace

    records = []
    for name in [s for s in args.sets.split(",") if s]:
        samples = [s.to("cuda") for s in synthetic_dataset(name)]
        s0 = samples[0]
        ws = ScaledInferenceWorkspace(node_features=s0.x.shape[1], edge_features=s0.edge_attr.shape[1], seed=0)
        As = [ws.system_matrix(s) for s in samples]
        Ls = [ws.inference_step(s)[0] for s in samples]
        bs = [A.matvec(s.mask.reshape(-1).to(torch.float64)) for A, s in zip(As, samples)]
        for kind in [k for k in args.kinds.split(",") if k]:
            spai = kind == "ext_spai_scaled"
            # one at a time: one solver per system, as get_cg_iter_time / get_pcg_scaled_iter_time hold them
            solvers = []
            try:
                for A, L in zip(As, Ls):
                    s = PreconditionedConjugateGradient(A, device="cuda", preconditioner=kind, dtype=np.float64)
                    if spai:
                        s.set_spai(L, ws.epsilon)
                    solvers.append(s)
            except LspcgError as e:  # AINV(0) breaks down on some systems: the single solver's row is NaN there
                rec = {"set": name, "kind": kind, "rtol": args.rtol, "systems": len(As), "error": str(e)}
                records.append(rec)
                print(json.dumps(rec), flush=True)
                continue

            def sequential():
                its, dev = [], 0.0
                for s, b in zip(solvers, bs):
                    it, _conv, t = s.solve(b, torch.zeros_like(b), rtol=args.rtol)
                    its.append(it)
                    dev += t
                return its, dev

            sequential()  # warm-up
            seq_wall, seq_dev, seq_its = best_of(args.repeat, sequential)

            B = BatchedConjugateGradient(As, Ls if spai else None, ws.epsilon, preconditioner=kind)

            def lockstep():
                res, t = B.solve(bs, [torch.zeros_like(b) for b in bs], rtol=args.rtol)
                return [r[0] for r in res], t

            lockstep()  # warm-up
            bat_wall, bat_dev, bat_its = best_of(args.repeat, lockstep)
            rec = {"set": name, "kind": kind, "rtol": args.rtol, "systems": len(As), "n": [A.n for A in As],
                   "iters": bat_its, "iters_equal_single": bat_its == seq_its,
                   "batch_wall_ms": bat_wall * 1e3, "batch_device_ms": bat_dev * 1e3,
                   "sequential_wall_ms": seq_wall * 1e3, "sequential_device_ms": seq_dev * 1e3,
                   "us_per_lockstep_iter": bat_dev * 1e6 / max(1, max(bat_its)),
                   "batch_wins_wall": bat_wall <= seq_wall}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del B, solvers
    with open(args.out, "w") as f:
        json.dump({"protocol": "warm-up solve, best of --repeat; wall = host time around the synchronised call(s), "
                               "device = the calls' own t_solve_ms", "repeat": args.repeat, "records": records}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
