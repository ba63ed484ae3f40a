"""What one training step costs, native optimizer against the per-parameter torch path.

Per batch, with device events after 5 warm-up steps, one event pair per step (the host work of a
step lies between the two records, so a pair spans it), median [min - p90] over 30 repeats:

  (a) fit_step: forward, fused loss + dL, backward, lspcg_optim_step, lspcg_gnn_set_weights
  (b) the path without the native optimizer: training_step + backward (autograd, unpack_grads) +
      clip_grad_norm_ + torch.optim.AdamW.step over the ~115 parameter tensors, then pack_weights +
      lspcg_gnn_set_weights at the next forward -- parameters on the device (b) and on the host (b_host)
  (c) forward + loss + backward alone (a without its optimizer step)
  (d) lspcg_optim_step alone
  (e) lspcg_gnn_set_weights alone from the device blob (its D2H copy, host fragment emit and H2D
      upload together; the emit is not separable from outside the library)

Batches: the collated heat_batch8 and four Poisson systems of 1,024 unknowns (the reference trains
on batches of 4).  The gate is (b) / (a) >= 1 on both.  Writes one JSON document (--out), prints it.

    python tools/train_step_probe.py --out profiles/train_step_probe.json [--small]
"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from learningsparsepreconditioner4gpu_amd import problems as P  # noqa: E402
from learningsparsepreconditioner4gpu_amd.data import collate, make_sample  # noqa: E402
from learningsparsepreconditioner4gpu_amd.infer import synthetic_dataset  # noqa: E402
from learningsparsepreconditioner4gpu_amd.loss import spai_loss_and_grad  # noqa: E402
from learningsparsepreconditioner4gpu_amd.optim import create_optimizer  # noqa: E402
from learningsparsepreconditioner4gpu_amd.workspace import SimpleInferenceWorkspace  # noqa: E402

OPT = {"lr": 1e-3, "weight_decay": 3e-3}
CLIP = 10.0


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


def batch(name, small):
    if name == "heat_batch8":
        samples = synthetic_dataset("heat_batch8", is_inference=False)
        return collate(samples[:2] if small else samples)
    out = []
    for seed in range(4):
        torch.manual_seed(seed)
        out.append(make_sample(*P.poisson2d_grid(32, 32, seed=seed)[:2], is_inference=False))
    return collate(out)


def run(name, small, warmup, repeats):
    b = batch(name, small).to("cuda")
    make = lambda: SimpleInferenceWorkspace(node_features=b.x.shape[1], edge_features=b.edge_attr.shape[1], seed=0)

    native = make()
    opt = create_optimizer("adamw", OPT, clip_norm=CLIP)

    def a_fit_step():
        native.fit_step(b, opt, OPT["lr"])

    def parent_step(ws, topt):
        def step():
            topt.zero_grad(set_to_none=True)
            ws.training_step(b).backward()
            torch.nn.utils.clip_grad_norm_(ws.parameters(), CLIP)
            topt.step()
        return step

    on_dev = make()
    on_dev.gnn.cuda()
    b_dev = parent_step(on_dev, torch.optim.AdamW(on_dev.parameters(), **OPT))
    on_host = make()
    b_host = parent_step(on_host, torch.optim.AdamW(on_host.parameters(), **OPT))

    alone = make()
    alone.gnn.flatten_parameters("cuda")

    def c_forward_backward():
        x, ei, ea, out = alone.gnn._forward_no_grad(b.x, b.edge_index, b.edge_attr)
        _, dL = spai_loss_and_grad(b, out.reshape(-1, 1, 1), alone.epsilon, kind="relative", eps=alone.loss_fn.eps)
        alone.gnn._backward(x, ei, ea, dL.reshape(out.shape))

    c_forward_backward()
    w = alone.gnn.flat.clone()
    g = torch.randn_like(w) * 1e-3
    kopt = create_optimizer("adamw", OPT, clip_norm=CLIP)

    def d_optim_step():
        kopt.step_blob(w, g, OPT["lr"])

    def e_set_weights():
        alone.gnn.weights_updated_in_place()

    res = {"name": name, "N": int(b.x.shape[0]), "E": int(b.edge_index.shape[1]), "graphs": int(b.ptr.numel() - 1),
           "parameters": int(w.numel()),
           "a_fit_step": timed(a_fit_step, warmup, repeats),
           "b_parent_step": timed(b_dev, warmup, repeats),
           "b_host_parent_step": timed(b_host, warmup, repeats),
           "c_forward_backward": timed(c_forward_backward, warmup, repeats),
           "d_optim_step": timed(d_optim_step, warmup, repeats),
           "e_set_weights": timed(e_set_weights, warmup, repeats)}
    med = lambda k: res[k]["median_ms"]
    res["ratio_b_over_a"] = med("b_parent_step") / med("a_fit_step")
    res["ratio_b_host_over_a"] = med("b_host_parent_step") / med("a_fit_step")
    res["optimizer_share_of_a"] = (med("a_fit_step") - med("c_forward_backward")) / med("a_fit_step")
    res["set_weights_share_of_a"] = med("e_set_weights") / med("a_fit_step")
    res["gate_b_over_a_ge_1"] = bool(res["ratio_b_over_a"] >= 1.0 and res["ratio_b_host_over_a"] >= 1.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal of the script on a smaller batch, not a measurement")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "train_step_probe needs the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "small": args.small, "optimizer": {"name": "adamw", **OPT},
           "gradient_clip_val": CLIP,
           "results": [run(n, args.small, args.warmup, args.repeats) for n in ("heat_batch8", "poisson1k_x4")]}
    doc["gate"] = all(r["gate_b_over_a_ge_1"] for r in doc["results"])
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
