"""Condition-number study: κ(M⁻¹A) per sample for the preconditioners neural, none, diag, ainv, ichol
(``cond.py`` of the reference), estimated on the GPU from the scalars of one PCG solve each.

The reference's ``cond.py`` builds M·A densely on the host and calls ``eigvalsh`` (:22-38), which
ends at a few thousand unknowns.  Here every number comes from
``workspace.condition_number``: one solve of the sample's system with a random start, the loop's
ρ_k and π_k as Lanczos coefficients, the extreme Ritz values of their tridiagonal (spectrum.py,
DESIGN.md "Condition number").  Two CSVs are written into ``--out-dir``:

* ``cond_cond_{exp_name}.csv`` -- the reference's table (:83-89, :162-164): header
  ``neural,none,diag,ainv,ichol``, one row per sample, read by ``misc/plot_cond.py`` as it is;
* ``cond_detail_{exp_name}.csv`` -- ``index, kind, n, iters, converged, lmin, lmax, lmin_bound,
  lmax_bound``: what each number rests on (a row with ``converged`` False or a large ``lmin_bound``
  needs a larger ``--max-iter``).

Not here: the plots, and the reference's second table (Kaporin's number, mean/geometric mean of ALL
eigenvalues, :35-37) -- one Krylov run gives the ends of the spectrum, not every eigenvalue or
log det.  The reference's ``eigvalsh(M @ A)`` reads one triangle of a matrix that is not symmetric,
so its table is the spectrum of another matrix; this one reports the spectrum of M⁻¹A itself.

    python -m learningsparsepreconditioner4gpu_amd.cond --dataset heat_batch8 --checkpoint runs/heat/checkpoints/epoch=19.ckpt
"""
from __future__ import annotations

import argparse
import csv
from pathlib import Path

import numpy as np
import torch

from .workspace import COND_KINDS, ScaledInferenceWorkspace, SimpleInferenceWorkspace

DETAIL = ("index", "kind", "n", "iters", "converged", "lmin", "lmax", "lmin_bound", "lmax_bound")


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(
        description="Condition number of the preconditioned system per sample and preconditioner kind "
                    f"({', '.join(COND_KINDS)}), estimated from the PCG loop's own scalars on the GPU. "
                    "Writes cond_cond_{exp_name}.csv (the reference's table) and cond_detail_{exp_name}.csv. "
                    "No plots, and no Kaporin table: Kaporin's number needs every eigenvalue (or log det), "
                    "which one Krylov run does not give.")
    ap.add_argument("--dataset", default="heat_batch8", help="a stand-in set of infer.synthetic_dataset")
    ap.add_argument("--folder", default="", help="on-disk dataset (datagen folder format); overrides --dataset")
    ap.add_argument("--block-size", type=int, default=1)
    ap.add_argument("--workspace", default="simple", choices=["simple", "scaled"])
    ap.add_argument("--checkpoint", "--pretrained", dest="checkpoint", default="",
                    help="a checkpoint of the reference (Lightning) or of train.py; without one the GNN is untrained")
    ap.add_argument("--epsilon", type=float, default=3e-3)
    ap.add_argument("--exp-name", default=None)
    ap.add_argument("--out-dir", default="output")
    ap.add_argument("--rtol", type=float, default=1e-8, help="relative residual the estimating solve runs to")
    ap.add_argument("--max-iter", type=int, default=0, help="0: each system's n")
    ap.add_argument("--seed", type=int, default=0, help="sample i's start vector is default_rng(seed + i).standard_normal(n)")
    ap.add_argument("--kinds", default=",".join(COND_KINDS), help="comma list out of " + ",".join(COND_KINDS))
    ap.add_argument("--start", default="full", choices=["full", "masked"],
                    help="full: the random start as drawn -- masked rows of A are identity rows and the reference's "
                         "dense spectrum contains them; masked: start * mask, the operator the solver iterates on")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    kinds = [k for k in args.kinds.split(",") if k]
    for k in kinds:
        if k not in COND_KINDS:
            raise SystemExit(f"--kinds: unknown kind {k!r}; expected some of {COND_KINDS}")
    from .infer import folder_dataset, synthetic_dataset

    torch.cuda.set_device(0)
    samples = folder_dataset(args.folder, args.block_size) if args.folder else synthetic_dataset(args.dataset)
    cls = ScaledInferenceWorkspace if args.workspace == "scaled" else SimpleInferenceWorkspace
    if args.checkpoint:
        ws = cls.load_from_checkpoint(args.checkpoint)
    else:
        s0 = samples[0]
        ws = cls(node_features=s0.x.shape[1], edge_features=s0.edge_attr.shape[1], block_size=s0.block_size,
                 epsilon=args.epsilon, seed=0)
    table, detail = [], []
    for i, sample in enumerate(samples):
        s = sample.to(ws.device)
        n = s.num_nodes * ws.block_size
        start = np.random.default_rng(args.seed + i).standard_normal(n)
        if args.start == "masked":
            start = start * s.mask.detach().cpu().numpy().reshape(-1).astype(np.float64)
        row = {k: float("nan") for k in COND_KINDS}
        for k in kinds:
            est = ws.condition_number(s, k, start=start, rtol=args.rtol, max_iter=args.max_iter)
            row[k] = est.cond
            detail.append((i, k, n, est.iters, est.converged, est.lmin, est.lmax, est.lmin_bound, est.lmax_bound))
            print(f"sample {i} n={n} {k}: cond {est.cond:.6g} ({est.iters} iterations, converged {est.converged}, "
                  f"bounds {est.lmin_bound:.2e} / {est.lmax_bound:.2e})", flush=True)
        table.append(row)
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    exp = args.exp_name or (Path(args.folder).name if args.folder else args.dataset)
    with open(out / f"cond_cond_{exp}.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(COND_KINDS)
        for row in table:
            w.writerow([repr(row[k]) for k in COND_KINDS])
    with open(out / f"cond_detail_{exp}.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(DETAIL)
        w.writerows(detail)
    return table, detail


if __name__ == "__main__":
    main()
