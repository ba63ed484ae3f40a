"""The native GNN backward (lspcg_gnn_backward through NodeEdgeProcessing.differentiable) against
the same model composed from torch ops with torch autograd on the same GPU (oracle.gnn moved to
the device), at kuhn101 (N = 1,030,301, E = 15,210,901) and the collated heat_batch8 batch, fp32.

Both sides first agree on every parameter gradient within the test bound (1e-5 of the tensor's
largest entry); then, with device events after a warm-up, one event pair per call, median and
spread over the repeats:  native forward, native forward + backward, torch forward + backward.
The byte / flop model of the edge kernel is DESIGN.md section 11's.  Writes one JSON document
(--out) and prints it.

    python tools/gnn_backward_probe.py --out profiles/gnn_backward_probe.json [--small] [--only NAME]
"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from learningsparsepreconditioner4gpu_amd.data import collate  # noqa: E402
from learningsparsepreconditioner4gpu_amd.infer import synthetic_dataset  # noqa: E402
from learningsparsepreconditioner4gpu_amd.nn import build_gnn  # noqa: E402
from oracle import gnn as OG  # noqa: E402

LAYERS = 4
PEAK_F32_MFMA = 157.3e12  # MI355X fp32 matrix peak, flop/s
PEAK_HBM = 8.0e12         # MI355X HBM3E, B/s


def edge_kernel_model(E):
    """k_edge_layer<backward> per call: bytes (x[dst], x[src], e, da[dst], de in and out, dfd, dfs:
    8 rows of 64 B, and two 4-B indices per edge) and MFMA flops (two MLPs: forward 48x16 + 2 16x16,
    the same transposed, the same again for dW, plus the three bias products; 2 flop per MAC)."""
    macs_ff = 48 * 16 + 2 * 16 * 16
    flops = 2 * E * 2 * (3 * macs_ff + 3 * 16 * 16)
    return {"bytes": E * (8 * 64 + 8), "flops": flops}


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
        return synthetic_dataset("kuhn11" if small else "kuhn101")[0]
    samples = synthetic_dataset("heat_batch8")
    return collate(samples[:2] if small else samples)


def run(name, small, warmup, repeats):
    s = problem(name, small).to("cuda")
    N, E = s.x.shape[0], s.edge_index.shape[1]
    node_in, edge_in = s.x.shape[1], s.edge_attr.shape[1]
    gnn = build_gnn(node_in, edge_in, 1, seed=0, differentiable=True, num_mp_layers=LAYERS).cuda()
    ref = OG.build(node_in, edge_in, 1, seed=0, num_mp_layers=LAYERS).cuda()
    G = torch.randn(E, 1, generator=torch.Generator().manual_seed(5)).cuda()
    x, ei, ea = s.x, s.edge_index, s.edge_attr

    # oracle.gnn's MPLayer allocates its aggregation buffer on the CPU: the device version of the same line
    def mp_forward(mp, node_attr, edge_index, edge_attr):
        src, dst = edge_index[0], edge_index[1]
        feat = torch.cat([node_attr[dst], node_attr[src], edge_attr], dim=-1)
        msg = mp.msg_mlp(feat)
        aggr = torch.zeros(node_attr.shape[0], msg.shape[1], dtype=msg.dtype, device=msg.device).index_add_(0, dst, msg)
        node_new = mp.node_mlp(aggr)
        edge_new = mp.edge_mlp(feat)
        return (node_attr + node_new if mp.node_residual else node_new,
                edge_attr + edge_new if mp.edge_residual else edge_new)

    def torch_forward():
        xa, e = ref.node_enc(x), ref.edge_enc(ea)
        for mp in ref.mp_layers:
            xa, e = mp_forward(mp, xa, ei, e)
        return ref.edge_dec(torch.cat([e, xa[ei[0]], xa[ei[1]]], dim=-1))

    def native_fwd():
        with torch.no_grad():
            gnn(x, ei, ea)

    def native_grad():
        gnn.zero_grad(set_to_none=True)
        (gnn(x, ei, ea)[1] * G).sum().backward()

    def torch_grad():
        ref.zero_grad(set_to_none=True)
        (torch_forward() * G).sum().backward()

    # the test bound first: want = the same torch model in fp64 on the device, e32 = the error of its
    # fp32 run; every native gradient within max(1e-5, 4 e32 / max|want|) max|want|
    native_grad()
    got = {k: p.grad.double() for k, p in gnn.named_parameters() if p.grad is not None}
    torch_grad()
    g32 = {k: p.grad.double() for k, p in ref.named_parameters() if p.grad is not None}
    ref.zero_grad(set_to_none=True)
    ref.double()
    x, ea, G = x.double(), ea.double(), G.double()
    torch_grad()
    want = {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None}
    ref.zero_grad(set_to_none=True)
    ref.float()
    x, ea, G = x.float(), ea.float(), G.float()
    torch.cuda.empty_cache()
    worst = worst32 = 0.0
    worst_key = None
    for k, w in want.items():
        scale = float(w.abs().max())
        e32 = float((g32[k] - w).abs().max())
        err = float((got[k] - w).abs().max())
        if err / scale > worst:
            worst, worst_key = err / scale, k
        worst32 = max(worst32, e32 / scale)
        assert err <= max(1e-5, 4 * e32 / scale) * scale, (name, k, err, e32, scale)
    out = {"name": name, "N": N, "E": E, "layers": LAYERS, "dtype": "fp32", "native_grad_rel_err_vs_fp64": worst, "native_grad_worst_tensor": worst_key,
           "torch_fp32_grad_rel_err_vs_fp64": worst32,
           "native_forward": timed(native_fwd, warmup, repeats),
           "native_forward_backward": timed(native_grad, warmup, repeats),
           "torch_forward_backward": timed(torch_grad, warmup, max(3, repeats // 3) if E > 5e6 else repeats)}
    out["backward_over_forward"] = (out["native_forward_backward"]["median_ms"] - out["native_forward"]["median_ms"]) \
        / out["native_forward"]["median_ms"]
    out["speedup_vs_torch"] = out["torch_forward_backward"]["median_ms"] / out["native_forward_backward"]["median_ms"]
    out["edge_kernel_model"] = edge_kernel_model(E)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny problems (a rehearsal of the script, not a measurement)")
    ap.add_argument("--only", default=None, help="kuhn101 or heat_batch8")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gnn_backward_probe needs the GPU"
    names = [args.only] if args.only else ["heat_batch8", "kuhn101"]
    doc = {"device": torch.cuda.get_device_name(0), "small": args.small, "peak_f32_mfma": PEAK_F32_MFMA,
           "peak_hbm": PEAK_HBM, "results": [run(n, args.small, args.warmup, args.repeats) for n in names]}
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
