"""Several right-hand sides of one system: ``solve_multi`` against its two alternatives.

For each system (default: Poisson 256^2, kuhn41, kuhn101 -- the bench's construction: the GNN's L,
eps 3e-3) and k = 2, 4, 8 right-hand sides at rtol 1e-8, three variants run in ONE process on the
same matrices:

  multi       ``PreconditionedConjugateGradient.solve_multi`` (one lockstep loop, k columns);
  sequential  k ``solve`` calls on the same solver, one after another (the baseline);
  batched     ``BatchedConjugateGradient`` over k copies of A and L (block-diagonal lockstep).

Every shape is warmed up first (graphs captured, caches warm); then the variants alternate,
``--repeat`` (>= 5) rounds.  Recorded per (system, k, variant): the median and min / max of the
device time (the calls' own t_solve_ms), the time per iteration per right-hand side (device time /
summed iteration counts) and the summed counts, which must be equal across the variants.
``multi_beats_sequential``: the multi median is below the sequential median by more than the
sequential runs' own min-max spread.  Writes one JSON document (default
profiles/multi_rhs_probe.json) and prints each record as a line."""
import argparse
import json
import statistics
import sys

import numpy as np
import torch


def build(name, epsilon):
    from learningsparsepreconditioner4gpu_amd import problems as P
    from learningsparsepreconditioner4gpu_amd.data import make_sample
    from learningsparsepreconditioner4gpu_amd.workspace import SimpleInferenceWorkspace

    A_raw, mask, feats, bs, e2n = P.workload(name)
    sample = make_sample(A_raw, mask, node_features=feats, block_size=bs, use_edge_features_as_node_feature=e2n)
    ws = SimpleInferenceWorkspace(node_features=sample.x.shape[1], edge_features=sample.edge_attr.shape[1],
                                  block_size=bs, epsilon=epsilon, seed=0)
    dev = sample.to("cuda")
    L, _ = ws.inference_step(dev)
    A = ws.system_matrix(dev)
    gt = dev.mask.reshape(-1).to(torch.float64)
    return A, L, gt


def rhs_block(A, gt, k):
    """(n, k): column 0 the bench's b = A @ mask, the others A @ seeded normal vectors."""
    g = torch.Generator(device="cpu").manual_seed(7)
    cols = [A.matvec(gt)]
    for _ in range(1, k):
        cols.append(A.matvec(torch.randn(A.n, generator=g, dtype=torch.float64).cuda()))
    return torch.stack(cols, dim=1).contiguous()


def stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="poisson256,kuhn41,kuhn101")
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--epsilon", type=float, default=3e-3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-batched", action="store_true", help="skip the BatchedConjugateGradient variant")
    ap.add_argument("--out", default="profiles/multi_rhs_probe.json")
    args = ap.parse_args(argv)
    sys.path.insert(0, ".")
    from learningsparsepreconditioner4gpu_amd.linalg import BatchedConjugateGradient, PreconditionedConjugateGradient

    records = []
    for name in [s for s in args.systems.split(",") if s]:
        A, L, gt = build(name, args.epsilon)
        solver = PreconditionedConjugateGradient(A, device="cuda", preconditioner="ext_spai", dtype=np.float64)
        solver.set_spai(L, args.epsilon, block_size=L.block_size)
        views = solver.views
        for k in [int(v) for v in args.ks.split(",") if v]:
            B = rhs_block(A, gt, k)
            bcols = [B[:, j].contiguous() for j in range(k)]

            def multi():
                res, t = solver.solve_multi(B, torch.zeros_like(B), rtol=args.rtol)
                return [r[0] for r in res], t

            def sequential():
                its, dev = [], 0.0
                for b in bcols:
                    it, _conv, t = solver.solve(b, torch.zeros_like(b), rtol=args.rtol)
                    its.append(it)
                    dev += t
                return its, dev

            variants = {"multi": multi, "sequential": sequential}
            batch = None
            if not args.no_batched:
                batch = BatchedConjugateGradient([A] * k, [L] * k, args.epsilon)

                def batched():
                    res, t = batch.solve(bcols, [torch.zeros_like(b) for b in bcols], rtol=args.rtol)
                    return [r[0] for r in res], t

                variants["batched"] = batched
            iters = {v: f()[0] for v, f in variants.items()}  # warm-up of every shape
            times = {v: [] for v in variants}
            for _ in range(max(5, args.repeat)):
                for v, f in variants.items():  # alternate
                    its, t = f()
                    assert its == iters[v], (name, k, v, its, iters[v])
                    times[v].append(t)
            seq = stats(times["sequential"])
            for v in variants:
                st = stats(times[v])
                rec = {"system": name, "n": A.n, "views": {m: views[m]["columns"] for m in views}, "k": k, "variant": v,
                       "rtol": args.rtol, "iters": iters[v], "iters_sum": int(sum(iters[v])),
                       "iters_equal_sequential": iters[v] == iters["sequential"], **st,
                       "us_per_iter_per_rhs": st["median_ms"] * 1e3 / max(1, sum(iters[v]))}
                if v == "multi":
                    rec["speedup_vs_sequential"] = seq["median_ms"] / st["median_ms"]
                    rec["multi_beats_sequential"] = st["median_ms"] < seq["median_ms"] - (seq["max_ms"] - seq["min_ms"])
                records.append(rec)
                print(json.dumps(rec), flush=True)
            del batch
        del solver
    with open(args.out, "w") as f:
        json.dump({"protocol": "one process; warm-up of every shape, then the variants alternate for `repeat` rounds; "
                               "times are the calls' own device times (t_solve_ms), summed over the k calls for "
                               "`sequential`", "repeat": max(5, args.repeat), "records": records}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
