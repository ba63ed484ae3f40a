"""The GNN's input sample of a matrix that lives on the device: host route against device route
(measurement only, GPU box).

    python tools/device_sample_probe.py [--out profiles/device_sample_probe.json] [--rounds 5] [workload ...]

Per workload (default: kuhn101, elasticity, bunny, kuhn41) and option set (the workload's own, and the
same with use_edge_features_as_node_feature="sum", which needs the edges grouped by destination):
  host    DeviceMatrix.to_scipy() -> data.make_sample -> GraphSample.to("cuda")   (d2h / make / h2d split)
  cold    DeviceSampler(A).sample() on a handle that has never been sampled: edge_index and, for the
          reduce, the destination grouping are built
  steady  DeviceSampler.sample() again: wall (it ends with the 8-byte read-back of the scale) and
          device time between two events; bytes = what the kernels must move (values read twice,
          edge_attr written once, the per-node arrays; the reduce also gathers edge_attr through the
          permutation), next to lspcg_read_timed's rate for a plain read of that many bytes
  refresh LiveSolver.refresh() against the --reuse-solver sequence fed by a host sample (to_scipy,
          make_sample, .to("cuda"), system_matrix(out=), update_matrix, inference_step, set_spai),
          the matrix's values alternating between two coefficient fields
Every shape is warmed up once, the variants alternate inside a round, and each figure is the median
with min and max over the rounds.  Wall times are host clocks with the device drained before and after.
"""
import argparse
import ctypes as C
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
from learningsparsepreconditioner4gpu_amd.data import DeviceSampler, make_sample
from learningsparsepreconditioner4gpu_amd.linalg import PreconditionedConjugateGradient
from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix
from learningsparsepreconditioner4gpu_amd.workspace import SimpleInferenceWorkspace

DEFAULT = ["kuhn101", "elasticity", "bunny", "kuhn41"]


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stat(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "rounds": len(v)}


def sorted_host(A_raw, bs):
    A = sp.csr_matrix(A_raw).astype(np.float64)
    A.sort_indices()
    if bs > 1:
        A = sp.bsr_matrix(A, blocksize=(bs, bs))
        A.sort_indices()
    return A


def steady_bytes(Ad, f_in, reduce):
    bs, nb, E = Ad.block_size, Ad.n // Ad.block_size, Ad.nnzb
    ne = E * bs * bs
    b = 2 * ne * 8 + ne * 4                      # the values twice, edge_attr once
    b += nb * (2 * 4 + 8 * bs + 3 * 4 * bs)      # rowptr, the diagonal's search and block, three vectors
    b += nb * (f_in * 4 + 8 * bs)                # x, mask
    if reduce != "disable":
        b += ne * 4 + E * 4 + nb * 4             # edge_attr gathered through perm, the column pointer
    return b


def host_route(Ad, opts):
    t0, A = clock(Ad.to_scipy)
    t1, s = clock(lambda: make_sample(A, **opts))
    t2, d = clock(lambda: s.to("cuda"))
    return {"d2h": t0, "make_sample": t1, "h2d": t2, "total": t0 + t1 + t2}, d


def probe(wl, rounds):
    A_raw, mask, feats, bs, e2n = P.workload(wl)
    A = sorted_host(A_raw, bs)
    ctx = DeviceMatrix.from_scipy(A, dtype=np.float64, block_size=bs).ctx
    out = {"n": A.shape[0], "nnzb": int(A.indices.size), "block_size": bs}
    for reduce in dict.fromkeys([e2n, "sum"]):
        opts = dict(mask=mask, node_features=feats, use_edge_features_as_node_feature=reduce)
        hopts = dict(opts, block_size=bs)
        Ad = DeviceMatrix.from_scipy(A, dtype=np.float64, block_size=bs)
        sampler = DeviceSampler(Ad, **opts)
        sampler.sample(), host_route(Ad, hopts)  # warm-up of both routes at this shape
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        rows = {"host": [], "cold": [], "steady_wall": [], "steady_device": []}
        for _ in range(rounds):
            rows["host"].append(host_route(Ad, hopts)[0])
            new = DeviceMatrix.from_scipy(A, dtype=np.float64, block_size=bs)  # (untimed) a handle never sampled
            rows["cold"].append(clock(lambda: DeviceSampler(new, **opts).sample())[0])
            del new
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            sampler.sample()
            ev[1].record()
            torch.cuda.synchronize()
            rows["steady_wall"].append((time.perf_counter() - t0) * 1e3)
            rows["steady_device"].append(ev[0].elapsed_time(ev[1]))
        nbytes = steady_bytes(Ad, sampler.x.shape[1], reduce)
        ms = C.c_double()
        _lib.call("lspcg_read_timed", ctx.handle, int(nbytes) // 16 * 16, 10, 0, C.byref(ms))
        dev = stat(rows["steady_device"])
        out[f"reduce={reduce}"] = {
            "host_ms": {k: stat([r[k] for r in rows["host"]]) for k in rows["host"][0]},
            "device_cold_wall_ms": stat(rows["cold"]),
            "device_steady_wall_ms": stat(rows["steady_wall"]),
            "device_steady_device_ms": dev,
            "steady_bytes": nbytes,
            "steady_GBps": nbytes / dev["median"] / 1e6,
            "read_timed_ms": ms.value,
            "read_timed_GBps": nbytes / ms.value / 1e6,
        }
        print(json.dumps({wl: {f"reduce={reduce}": out[f"reduce={reduce}"]}}), flush=True)
        del sampler, Ad

    # ---- LiveSolver.refresh against the reuse-solver sequence fed by host samples
    opts = dict(mask=mask, node_features=feats, use_edge_features_as_node_feature=e2n)
    f_in = (0 if feats is None else feats.shape[1]) + bs + (bs * bs if e2n != "disable" else 0)
    ws = SimpleInferenceWorkspace(node_features=f_in, edge_features=bs * bs, block_size=bs, seed=0)
    d = 1.0 + 0.5 * np.random.default_rng(7).uniform(size=A.shape[0])
    A2 = sorted_host(sp.diags(d) @ sp.csr_matrix(A) @ sp.diags(d), bs)
    vals = [np.ascontiguousarray(M.data, dtype=np.float64).reshape(-1) for M in (A, A2)]
    Ad = DeviceMatrix.from_scipy(A, dtype=np.float64, block_size=bs)
    live = ws.live_solver(Ad, **opts)
    s0 = make_sample(A, block_size=bs, **opts).to("cuda")
    host_solver = PreconditionedConjugateGradient(ws.system_matrix(s0), device="cuda", preconditioner=ws.neural_precond,
                                                  dtype=np.float64)

    def host_refresh():
        s = host_route(Ad, dict(opts, block_size=bs))[1]
        ws.system_matrix(s, out=host_solver.A)
        host_solver.update_matrix()
        L, _ = ws.inference_step(s)
        host_solver.set_spai(L, ws.epsilon, block_size=L.block_size)

    Ad.set_values(vals[1])
    live.refresh(), host_refresh()  # warm-up
    rows = {"live_wall": [], "live_device": [], "host_wall": [], "steps": []}
    for r in range(rounds):
        Ad.set_values(vals[r % 2])
        t = live.refresh()
        rows["live_wall"].append(t["total"]["wall"] * 1e3)
        rows["live_device"].append(t["total"]["device"] * 1e3)
        rows["steps"].append({k: v["device"] * 1e3 for k, v in t.items()})
        rows["host_wall"].append(clock(host_refresh)[0])
    out["refresh"] = {"live_wall_ms": stat(rows["live_wall"]), "live_device_ms": stat(rows["live_device"]),
                      "live_steps_device_ms": {k: stat([s[k] for s in rows["steps"]]) for k in rows["steps"][0]},
                      "host_fed_wall_ms": stat(rows["host_wall"]), "graphs_kept": bool(live.graphs_kept)}
    print(json.dumps({wl: {"refresh": out["refresh"]}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/device_sample_probe.json")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("workloads", nargs="*", default=DEFAULT)
    args = ap.parse_args()
    res = {}
    for wl in args.workloads:
        res[wl] = probe(wl, args.rounds)
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
