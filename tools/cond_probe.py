"""What recording the PCG scalars costs, and one full-size condition-number estimate.

Three measurements, written as one JSON document (default profiles/cond_probe.json):

  null_case   ``ms_per_step`` of ``bench.py`` (kuhn101) on this tree and on the parent commit, taken
              from the bench's own JSON lines (``--branch-bench`` / ``--parent-bench`` files, one line
              per run, recorded in ONE session, the two trees alternating).  ``within_parent_spread``:
              this tree's median is not above the parent's by more than the parent's own max - min.
  recording   the same solve with and without ``return_coefficients`` in one process, alternating,
              ``--repeat`` rounds after a warm-up: kuhn101 (the bench's construction: the GNN's L,
              eps 3e-3, b = A @ mask) and a one-workgroup system (Poisson 30x30, n = 900, an SPAI-like
              L).  Median device time per iteration of either, and the difference.  No target: the
              recording is one 16-byte store per iteration.
  estimate    kappa(M^-1 A) of kuhn101 for ``neural`` (the bench's L), ``diag`` and ``none`` at rtol
              1e-8 (``workspace.condition_number``): iterations, both ends, both bounds.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def bench_lines(path):
    out = []
    for ln in Path(path).read_text().splitlines():
        ln = ln.strip()
        if ln.startswith("{") and '"ms_per_step"' in ln:
            out.append(json.loads(ln))
    return out


def null_case(branch_files, parent_files):
    b = [r["ms_per_step"] for f in branch_files for r in bench_lines(f)]
    p = [r["ms_per_step"] for f in parent_files for r in bench_lines(f)]
    if not b or not p:
        return None
    spread = max(p) - min(p)
    return {"branch_ms_per_step": b, "parent_ms_per_step": p, "branch_median": statistics.median(b),
            "parent_median": statistics.median(p), "parent_spread": spread,
            "within_parent_spread": statistics.median(b) <= statistics.median(p) + spread}


def recording(solver, b, repeat, rtol):
    x = torch.zeros_like(b)

    def run(rec):
        x.zero_()
        r = solver.solve(b, x, rtol, 0, return_coefficients=rec)
        return r[0], r[2]

    for rec in (False, True, False, True):
        run(rec)
    t = {False: [], True: []}
    its = set()
    for _ in range(repeat):
        for rec in (False, True):
            it, s = run(rec)
            its.add(it)
            t[rec].append(s)
    assert len(its) == 1, its
    it = its.pop()
    us = {k: statistics.median(v) / it * 1e6 for k, v in t.items()}
    return {"n": solver.n, "iters": it, "us_per_iter_plain": us[False], "us_per_iter_recording": us[True],
            "us_per_iter_difference": us[True] - us[False],
            "plain_min_max_us": [min(t[False]) / it * 1e6, max(t[False]) / it * 1e6],
            "recording_min_max_us": [min(t[True]) / it * 1e6, max(t[True]) / it * 1e6]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="kuhn101")
    ap.add_argument("--epsilon", type=float, default=3e-3)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--branch-bench", nargs="*", default=[])
    ap.add_argument("--parent-bench", nargs="*", default=[])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cond_probe.json"))
    args = ap.parse_args(argv)

    from learningsparsepreconditioner4gpu_amd import problems as P
    from learningsparsepreconditioner4gpu_amd.data import make_sample
    from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient
    from learningsparsepreconditioner4gpu_amd.workspace import SimpleInferenceWorkspace

    doc = {"workload": args.workload, "rtol": args.rtol, "device": torch.cuda.get_device_name(0),
           "null_case": null_case(args.branch_bench, args.parent_bench)}
    print(json.dumps({"null_case": doc["null_case"]}), flush=True)

    A_raw, mask, feats, bs, e2n = P.workload(args.workload)
    sample = make_sample(A_raw, mask, node_features=feats, block_size=bs, use_edge_features_as_node_feature=e2n)
    ws = SimpleInferenceWorkspace(node_features=sample.x.shape[1], edge_features=sample.edge_attr.shape[1],
                                  block_size=bs, epsilon=args.epsilon, seed=0)
    dev = sample.to("cuda")
    L, _ = ws.inference_step(dev)
    A = ws.system_matrix(dev)
    solver = PreconditionedConjugateGradient(A, device="cuda", preconditioner="ext_spai", dtype=np.float64)
    solver.set_spai(L, args.epsilon, block_size=L.block_size)
    big = recording(solver, A.matvec(dev.mask.reshape(-1).to(torch.float64)), args.repeat, args.rtol)

    A9 = P.poisson2d_grid(30, 30)[0].tocsr()
    d9 = A9.diagonal()
    L9 = A9.copy()
    rows = np.repeat(np.arange(A9.shape[0]), np.diff(A9.indptr))
    L9.data = np.where(rows == A9.indices, 1.0 / np.sqrt(d9[rows]),
                       np.random.default_rng(1).normal(size=A9.nnz) * 0.05 / np.sqrt(d9[rows]))
    s9 = PreconditionedConjugateGradient(A9, device="cuda", preconditioner="ext_spai", dtype=np.float64)
    s9.set_spai(L9, args.epsilon)
    b9 = torch.as_tensor(np.random.default_rng(0).standard_normal(A9.shape[0])).cuda()
    doc["recording"] = {args.workload: big, "poisson30_one_workgroup": recording(s9, b9, args.repeat, args.rtol)}
    print(json.dumps({"recording": doc["recording"]}), flush=True)

    doc["estimate"] = {}
    for kind in ("neural", "diag", "none"):
        e = ws.condition_number(dev, kind, rtol=args.rtol)
        doc["estimate"][kind] = {"n": A.n, "cond": e.cond, "lmin": e.lmin, "lmax": e.lmax, "iters": e.iters,
                                 "converged": e.converged, "lmin_bound": e.lmin_bound, "lmax_bound": e.lmax_bound}
        print(json.dumps({"estimate": {kind: doc["estimate"][kind]}}), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    return doc


if __name__ == "__main__":
    main()
