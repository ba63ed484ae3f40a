"""Mesh + coefficients -> A: the host assembly of problems.py against fem.TetMesh on the device
(measurement only, GPU box).

    python tools/fem_probe.py [--out profiles/fem_probe.json] [--rounds 5] [mesh ...]

Per mesh (default: kuhn101, kuhn41, bunny, delaunay27000 for heat; elasticity = the C4 box):
  host     what a user of the package had before: problems.p1_stiffness + lumped_mass (heat) or
           problems.elasticity_box (elasticity) on the host, then DeviceMatrix.set_values (wall, split
           into assembly and upload)
  device   mesh.heat(kappa, rho, out=A) / mesh.elasticity(E, nu, c, out=A): wall and device time
           between two events; bytes = what the assembly must move at least (tets, nodes, gather map,
           run pointers, coefficients, heat's element matrices, the values written to scratch, set_values' pattern comparison and
           copy), next to lspcg_read_timed's rate for a plain read of that many bytes
  analysis fem.TetMesh(nodes, tets) from device tensors: the one-off pattern and gather map
  refresh  (heat) mesh.heat(out=A); live.refresh() against the host assembly + set_values +
           live.refresh() on a LiveSolver of a seeded workspace
Every device shape is warmed up once and each figure is the median with min and max over the rounds;
the host assembly runs once on a mesh above a million tets and at most three times above 100 k.  Wall times are host clocks
with the device drained before and after.
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

from learningsparsepreconditioner4gpu_amd import _lib, fem
from learningsparsepreconditioner4gpu_amd import problems as P
from learningsparsepreconditioner4gpu_amd.sparse import DeviceMatrix
from learningsparsepreconditioner4gpu_amd.workspace import SimpleInferenceWorkspace

DEFAULT = ["kuhn101", "kuhn41", "bunny", "delaunay27000", "elasticity"]
BOX = dict(nx=117, ny=30, nz=30, E=3e6, nu=0.4, density=1.0, dt=0.01)  # elasticity_box's defaults: config C4


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def timed(f):
    """(wall ms, device ms) of one call."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev[0].record()
    f()
    ev[1].record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, ev[0].elapsed_time(ev[1])


def stat(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "rounds": len(v)}


def mesh_of(name):
    if name.startswith("kuhn"):
        n = int(name[4:])
        return P.kuhn_tets(n, n, n)
    if name == "bunny":
        return P.bunny_tets()
    if name.startswith("delaunay"):
        return P.delaunay_tets(int(name[8:]))
    if name == "elasticity":
        nodes, tets = P.kuhn_tets(BOX["nx"], BOX["ny"], BOX["nz"])
        return nodes / float(max(BOX["ny"], BOX["nz"]) - 1), tets
    raise KeyError(name)


def device_bytes(N, T, nnz, bs, itemsize=8):
    v = nnz * bs * bs * itemsize
    b = 16 * T + 24 * N + 4 * (16 * T + N) + 4 * (nnz + 1)      # tets, nodes, gather map, run pointers
    b += 8 * T * (2 if bs == 3 else 1) + (8 * N if bs == 1 else 0)  # kappa | young, poisson; density
    if bs == 1:
        b += 2 * 8 * 17 * T                                      # heat: element matrices and vol / 4, written and read
    b += v                                                       # the values, written to the scratch
    b += 2 * (4 * (N + 1) + 4 * nnz) + 2 * v                     # set_values: pattern comparison, copy
    return b


def host_heat(nodes, tets, kappa, rho):
    K = P.p1_stiffness(nodes, tets, kappa)
    return P._canon(K + sp.diags(P.lumped_mass(nodes, tets) * rho))


def probe(name, rounds):
    nodes, tets = mesh_of(name)
    nodes, tets = np.ascontiguousarray(nodes, dtype=np.float64), np.ascontiguousarray(tets, dtype=np.int64)
    N, T = nodes.shape[0], tets.shape[0]
    elast = name == "elasticity"
    bs = 3 if elast else 1
    host_rounds = 1 if T > 1000000 else min(rounds, 3) if T > 100000 else rounds
    rng = np.random.default_rng(0)
    kappas = [rng.uniform(0.01, 1.0, size=T) for _ in range(2)]
    rho = rng.uniform(1e-4, 5e-4, size=N)
    nd, td = torch.as_tensor(nodes, device="cuda"), torch.as_tensor(tets, device="cuda")
    fem.TetMesh(nd, td)  # warm-up of the analysis at this shape
    ana = [clock(lambda: fem.TetMesh(nd, td))[0] for _ in range(rounds)]
    mesh = fem.TetMesh(nd, td)
    out = {"N": N, "T": T, "nnz": mesh.nnz, "block_size": bs, "analysis_wall_ms": stat(ana)}

    # ---- the device route
    if elast:
        E = torch.full((T,), BOX["E"], dtype=torch.float64, device="cuda")
        nu = torch.full((T,), BOX["nu"], dtype=torch.float64, device="cuda")
        coef = BOX["density"] / BOX["dt"] ** 2
        A = mesh.elasticity(E, nu, coef)
        assemble = lambda k: mesh.elasticity(E, nu, coef, out=A)
    else:
        kd = [torch.as_tensor(k, device="cuda") for k in kappas]
        rd = torch.as_tensor(rho, device="cuda")
        A = mesh.heat(kd[0], rd)
        assemble = lambda k: mesh.heat(kd[k], rd, out=A)
    assemble(1)
    rows = [timed(lambda: assemble(r % 2)) for r in range(rounds)]
    nbytes = device_bytes(N, T, mesh.nnz, bs)
    ms = C.c_double()
    _lib.call("lspcg_read_timed", A.ctx.handle, int(nbytes) // 16 * 16, 10, 0, C.byref(ms))
    dev = stat([r[1] for r in rows])
    out["device"] = {"wall_ms": stat([r[0] for r in rows]), "device_ms": dev, "bytes": nbytes,
                     "GBps": nbytes / dev["median"] / 1e6, "read_timed_ms": ms.value,
                     "read_timed_GBps": nbytes / ms.value / 1e6}
    print(json.dumps({name: {k: out[k] for k in ("N", "T", "nnz", "analysis_wall_ms", "device")}}), flush=True)

    # ---- the host route
    if elast:
        host = lambda k: sp.bsr_matrix(P.elasticity_box(**BOX)[0], blocksize=(3, 3))
    else:
        host = lambda k: host_heat(nodes, tets, kappas[k], rho)
    t0 = time.perf_counter()
    H = host(0)
    first = (time.perf_counter() - t0) * 1e3
    Ah = DeviceMatrix.from_scipy(H, block_size=bs)
    hrows = {"assemble": [first] if host_rounds == 1 else [], "set_values": [], "set_values_device": []}
    for r in range(host_rounds):
        if host_rounds > 1:
            t0 = time.perf_counter()
            H = host(r % 2)
            hrows["assemble"].append((time.perf_counter() - t0) * 1e3)
        vals = np.ascontiguousarray(H.data, dtype=np.float64).reshape(-1)
        w, d = timed(lambda: Ah.set_values(vals))
        hrows["set_values"].append(w)
        hrows["set_values_device"].append(d)
    out["host"] = {"assemble_wall_ms": stat(hrows["assemble"]), "set_values_wall_ms": stat(hrows["set_values"]),
                   "set_values_device_ms": stat(hrows["set_values_device"]), "nnzb": Ah.nnzb,
                   "total_wall_ms": stat(hrows["assemble"])["median"] + stat(hrows["set_values"])["median"]}
    assemble(0 if host_rounds == 1 else (host_rounds - 1) % 2)  # the coefficients H was assembled from
    out["host"]["device_vs_host_rel"] = float(abs(sp.csr_matrix(A.to_scipy()) - sp.csr_matrix(H)).max() / abs(H).max())
    print(json.dumps({name: {"host": out["host"]}}), flush=True)
    if elast:
        return out

    # ---- heat(out=A); refresh() against host values + set_values + refresh()
    mask = np.ones(N)
    mask[nodes[:, 0] <= nodes[:, 0].min()] = 0.0
    feats = np.ascontiguousarray(nodes / np.abs(nodes).max(), dtype=np.float32)
    ws = SimpleInferenceWorkspace(node_features=4, edge_features=1, block_size=1, seed=0)
    live = ws.live_solver(A, mask=mask, node_features=feats)
    live_h = ws.live_solver(Ah, mask=mask, node_features=feats)
    hvals = np.ascontiguousarray(H.data, dtype=np.float64).reshape(-1)
    assemble(0), live.refresh(), Ah.set_values(hvals), live_h.refresh()  # warm-up
    rr = {"device": [], "host_fed": [], "refresh_only": []}
    for r in range(rounds):
        rr["device"].append(clock(lambda: (assemble(r % 2), live.refresh()))[0])
        rr["host_fed"].append(clock(lambda: (Ah.set_values(hvals), live_h.refresh()))[0])
        rr["refresh_only"].append(live.refresh()["total"]["wall"] * 1e3)
    out["refresh"] = {"heat_and_refresh_wall_ms": stat(rr["device"]), "refresh_only_wall_ms": stat(rr["refresh_only"]),
                      "set_values_and_refresh_wall_ms": stat(rr["host_fed"]),
                      "host_fed_total_wall_ms": stat(rr["host_fed"])["median"] + out["host"]["assemble_wall_ms"]["median"],
                      "graphs_kept": bool(live.graphs_kept)}
    print(json.dumps({name: {"refresh": out["refresh"]}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fem_probe.json")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("meshes", nargs="*", default=DEFAULT)
    args = ap.parse_args()
    res = {}
    for name in args.meshes:
        res[name] = probe(name, args.rounds)
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
