#!/usr/bin/env python
"""Mesh extraction timing on one MI355X: the synthetic `hotdog` model (opaque density head, so threshold 10 cuts a surface) at R = 256 and 512.

    python tools/mesh_bench.py [--out profiles/mesh_bench.json]            # timings (device events + a synchronise), V and T
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_bench.py --kernels-only
    python tools/mesh_bench.py --stats DIR [--out ...]                     # add the MC kernels' bytes / kernel time from DIR's *_kernel_stats.csv
    python tools/mesh_bench.py --attributes [--out ...]                    # add the attribute and cleaning stages to the runs already in --out

Per R it reports the lattice evaluation (mesh.lattice), the marching-cubes call (mc_count, the one totals read, mc_emit) and the
device-to-host copy of the mesh separately, and the reference-shaped route: extract_fields' 128^3 chunks through model.density with a
.cpu() per chunk, then the numpy restatement of the kernels (tests/mc_ref.py) over 16 x-slabs in 16 threads (slab meshes not merged:
a lower bound on a CPU marching cubes' time).  Bytes of the MC kernels, per call, from shapes: count reads u (4 N) and writes the node
codes (2 N); vertex emit reads them (2 N), writes the vertex bases (4 N) and the vertices (12 V); triangle emit reads codes and bases
(6 N) and writes the triangles (12 T): 18 N + 12 V + 12 T, neighbour re-reads counted once (they hit the caches).

--attributes times, per R, the stages behind save_mesh's options on the device -- vertex normals (mc_vertex_normals from mc_emit's scratch), vertex
colours (the field forward at every vertex), components (mesh_components, no host read) and clean (components, filter at 8 triangles, compaction of the
vertices, the triangles and the normals, one host read) -- and beside them the host route they replace: copying the mesh to the host, scipy's
connected_components, and the numpy filter and compaction (tests/mesh_attr_ref.py's, on scipy's labels).
"""
import argparse
import csv
import glob
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec
THRESHOLD = 10.0
MC_KERNELS = ("k_mc_count", "k_mc_scan", "k_mc_verts", "k_mc_tris")


def model():
    from nerf_signature_amd import synthetic
    from nerf_signature_amd.network import NeRFNetwork
    m = NeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1, message_dim=32, n_views=1)
    synthetic.init_model(m, "hotdog", opaque=True)
    return m.cuda().eval()


def timed(fn, reps):
    """Median device time (ms) of fn() over reps calls, events around each call and a synchronise."""
    out, ts = None, []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), out


def reference_route(m, R, threads):
    """extract_fields with .cpu() per 128^3 chunk, then the CPU marching cubes over `threads` x-slabs (ms, ms)."""
    import mc_ref
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    S = 128
    X, Y, Z = (torch.linspace(float(lo[a]), float(hi[a]), R).split(S) for a in range(3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u = np.zeros([R, R, R], dtype=np.float32)
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    val = m.density(pts.cuda())["sigma"].reshape(len(xs), len(ys), len(zs)).detach().cpu().numpy()
                    u[xi * S:xi * S + len(xs), yi * S:yi * S + len(ys), zi * S:zi * S + len(zs)] = val
    t1 = time.perf_counter()
    cuts = np.linspace(0, R - 1, threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda s: mc_ref.marching_cubes(u[cuts[s]:cuts[s + 1] + 1], THRESHOLD), range(threads)))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, sum(len(p[1]) for p in parts)


def run(resolutions, reps, threads):
    from nerf_signature_amd import mesh
    m = model()
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    rec = {"model": "synthetic hotdog, opaque density head", "threshold": THRESHOLD, "device": torch.cuda.get_device_name(0), "runs": []}
    for R in resolutions:
        mesh.lattice(m, lo, hi, R)                    # warm-up: code objects, allocator
        lat_ms, u = timed(lambda: mesh.lattice(m, lo, hi, R), reps)
        mesh.marching_cubes(u, THRESHOLD)
        mc_ms, (v, t) = timed(lambda: mesh.marching_cubes(u, THRESHOLD), reps)
        copy_ms, _ = timed(lambda: (v.cpu(), t.cpu()), reps)
        N, V, T = R ** 3, v.shape[0], t.shape[0]
        ref_lat_ms, ref_mc_ms, ref_T = reference_route(m, R, threads)
        run_rec = {"R": R, "nodes": N, "V": V, "T": T, "lattice_ms": lat_ms, "mc_ms": mc_ms, "d2h_ms": copy_ms,
                   "mc_bytes": 18 * N + 12 * V + 12 * T, "reference_route": {"lattice_with_host_copies_ms": ref_lat_ms,
                   f"cpu_mc_{threads}_threads_ms": ref_mc_ms, "T_slabs": ref_T}}
        rec["runs"].append(run_rec)
        print(json.dumps(run_rec), flush=True)
    return rec


def host_route(v, t, n, min_triangles):
    """(copy ms, scipy components ms, numpy filter + compaction ms, components) of the same cleaning through the host."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hv, ht, hn = v.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy()
    t1 = time.perf_counter()
    V = len(hv)
    r, c = ht[:, [0, 1, 2]].reshape(-1), ht[:, [1, 2, 0]].reshape(-1)
    ncomp, lab = connected_components(coo_matrix((np.ones(r.size, np.int8), (r, c)), shape=(V, V)), directed=False)
    t2 = time.perf_counter()
    count = np.bincount(lab[ht[:, 0]], minlength=ncomp)
    keep = count >= max(min_triangles, 1)
    vkeep, tkeep = keep[lab], keep[lab[ht[:, 0]]]
    new_id = np.cumsum(vkeep) - 1
    out = hv[vkeep], new_id[ht[tkeep]].astype(np.int32), hn[vkeep]
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, int(ncomp), len(out[0]), len(out[1])


def attributes(resolutions, reps, min_triangles=8):
    """Per R: device times of normals, colours, components and clean, and the host route of the cleaning."""
    from nerf_signature_amd import mesh
    m = model()
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    out = {}
    for R in resolutions:
        u = mesh.lattice(m, lo, hi, R)
        scale = mesh.lattice_scale(lo, hi, R)
        v, t, scratch = mesh._march(u, THRESHOLD)
        n = mesh.vertex_normals(u, THRESHOLD, scratch, scale)                 # warm-ups: code objects, allocator
        x = mesh.world_vertices(v, lo, hi, R).float()
        mesh.vertex_colors(m, x, n)
        mesh.clean(v, t, min_triangles, attributes=(n,))
        normals_ms, _ = timed(lambda: mesh.vertex_normals(u, THRESHOLD, scratch, scale), reps)
        colours_ms, _ = timed(lambda: mesh.vertex_colors(m, x, n), reps)
        comp_ms, (labels, _) = timed(lambda: mesh._components(t, v.shape[0]), reps)
        clean_ms, (cv, ct, cn) = timed(lambda: mesh.clean(v, t, min_triangles, attributes=(n,)), reps)
        host = sorted(host_route(v, t, n, min_triangles) for _ in range(3))[1]
        rec = {"V": v.shape[0], "T": t.shape[0], "components": int(torch.unique(labels[t[:, 0].long()]).numel()), "min_triangles": min_triangles,
               "V_clean": cv.shape[0], "T_clean": ct.shape[0], "normals_ms": normals_ms, "colours_ms": colours_ms, "components_ms": comp_ms,
               "clean_ms": clean_ms, "host_route": {"d2h_ms": host[0], "scipy_components_ms": host[1], "numpy_filter_ms": host[2],
                                                      "components": host[3], "V_clean": host[4], "T_clean": host[5]}}
        out[R] = rec
        print(json.dumps(dict(rec, R=R)), flush=True)
    return out


def kernels_only(resolutions, reps):
    """What the profiled run executes: the lattice and the marching cubes, reps times per R."""
    from nerf_signature_amd import mesh
    m = model()
    for R in resolutions:
        u = mesh.lattice(m, m.aabb_infer[:3], m.aabb_infer[3:], R)
        for _ in range(reps):
            mesh.marching_cubes(u, THRESHOLD)
        torch.cuda.synchronize()


def add_stats(rec, d):
    """The MC kernels' calls and mean times from the *_kernel_stats.csv of a --kernels-only run under rocprofv3 (one R per run)."""
    f = sorted(glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True))[-1]
    rows = {k: r for r in csv.DictReader(open(f)) for k in MC_KERNELS if k + "(" in r["Name"]}
    rec["kernel_stats_file"] = os.path.relpath(f, ROOT)
    rec["mc_kernels"] = {k: {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3} for k, r in rows.items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--attributes", action="store_true", help="add the attribute and cleaning stages to the runs already in --out")
    ap.add_argument("--stats", help="directory of a rocprofv3 --kernel-trace --stats run of --kernels-only, one R per run: --resolutions R")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_bench needs a GPU")
    if a.kernels_only:
        kernels_only(a.resolutions, a.reps)
        return
    if a.attributes:
        rec = json.load(open(a.out))
        for R, r in attributes(a.resolutions, a.reps).items():
            next(x for x in rec["runs"] if x["R"] == R)["attributes"] = r
    elif a.stats:
        rec = json.load(open(a.out))
        if len(a.resolutions) != 1:
            sys.exit("--stats: give the one resolution the profiled run used")
        R = a.resolutions[0]
        run_rec = next(r for r in rec["runs"] if r["R"] == R)
        st = add_stats({}, a.stats)
        k_us = sum(v["avg_us"] for v in st["mc_kernels"].values())
        run_rec["mc_kernels"] = dict(st["mc_kernels"], total_us=k_us, bytes_per_s=run_rec["mc_bytes"] / (k_us * 1e-6),
                                     share_of_hbm_peak=run_rec["mc_bytes"] / (k_us * 1e-6) / HBM_PEAK, stats_file=st["kernel_stats_file"])
        print(json.dumps(run_rec["mc_kernels"]))
    else:
        rec = run(a.resolutions, a.reps, a.threads)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
