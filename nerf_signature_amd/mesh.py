"""Mesh extraction: marching cubes over the trained density field on the GPU (nerf/utils.py:174-204 and Trainer.save_mesh, :611-631).

The reference evaluates `model.density` on a 256^3 lattice in 128^3 chunks, copies every chunk to the host, runs mcubes.marching_cubes
on the CPU and exports a PLY through trimesh.  Here the lattice stays on the device and the marching cubes are HIP kernels
(csrc/mesh.hip, table csrc/mc_tables.h from mc_table.py); only the finished mesh is copied back.

    marching_cubes(u, threshold)                              -> vertices [V,3] fp32, triangles [T,3] int32 (device, lattice space)
    lattice(model, bound_min, bound_max, resolution, message) -> the fp32 [R,R,R] density lattice, bit-identical to extract_fields
    extract_geometry(bound_min, bound_max, resolution, threshold, query_func)   the reference's signature and return types
    save_mesh(model, path, resolution=256, threshold=10, message=None)          binary PLY over aabb_infer; returns (V, T)

The triangulation is this project's table ("Mesh extraction"), not mcubes': the same surface, closed and consistently
oriented, with its own choice in the ambiguous cases and its own triangle order.
"""
import math
import os

import numpy as np
import torch

from . import _native as nv
from . import fieldops as fo

MAX_NODES = 1 << 28          # mc_count's lattice limit (include/nerfsig.h)
LATTICE_CHUNK = 1 << 21      # points per field evaluation: the planes workspace is 136 B per point (hg_planes_bytes)
REFERENCE_CHUNK = 128        # extract_fields' S


def marching_cubes(u, threshold):
    """Marching cubes of the device lattice u[nx, ny, nz] (fp32, z fastest) at `threshold` (inside: u > threshold) -> (vertices float32 [V,3],
    triangles int32 [T,3]) on u's device, vertices in lattice space (the counterpart of mcubes.marching_cubes).  Output order: include/nerfsig.h."""
    if not isinstance(u, torch.Tensor) or not u.is_cuda:
        raise ValueError("marching_cubes: the lattice must be a tensor on the GPU (there is no CPU path)")
    if u.dtype != torch.float32:
        raise ValueError(f"marching_cubes: the lattice must be float32, got {u.dtype}")
    if u.dim() != 3:
        raise ValueError(f"marching_cubes: the lattice must be 3-D, got shape {tuple(u.shape)}")
    nx, ny, nz = (int(s) for s in u.shape)
    if min(nx, ny, nz) < 2:
        raise ValueError(f"marching_cubes: every lattice dimension must be at least 2, got {tuple(u.shape)}")
    if nx * ny * nz > MAX_NODES:
        raise ValueError(f"marching_cubes: {nx} x {ny} x {nz} nodes is above the limit of 2^28")
    thr = float(threshold)
    dev = u.device
    with torch.cuda.device(dev):
        u = u.contiguous()
        scratch = torch.empty(int(nv.fn("mc_scratch_bytes")(nx, ny, nz)), dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int32, device=dev)
        nv.call("mc_count", nv.ptr(u), nx, ny, nz, thr, nv.ptr(scratch), nv.ptr(totals), nv.stream())
        V, T = totals.tolist()
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        triangles = torch.empty(T, 3, dtype=torch.int32, device=dev)
        if V:
            nv.call("mc_emit", nv.ptr(u), nx, ny, nz, thr, nv.ptr(scratch), V, T, nv.ptr(vertices), nv.ptr(triangles), nv.stream())
    return vertices, triangles


def _axes(bound_min, bound_max, resolution):
    """extract_fields' three axes: torch.linspace on the CPU from the bounds as Python floats."""
    return [torch.linspace(float(bound_min[a]), float(bound_max[a]), resolution) for a in range(3)]


def _field_of(model, message):
    """(bound, base tables, codebook pre-sum or None, packed MLP weights) of density() for a NeRFNetwork or a CleanNeRFNetwork."""
    from .network import NeRFNetwork
    from .stage1 import CleanNeRFNetwork
    if isinstance(model, NeRFNetwork):
        _, _, S = model._select(message)             # the codebook only with a message, as density(x, message)
        return model.bound, model.encoder.tables(), S, model._packed()
    if isinstance(model, CleanNeRFNetwork):
        if message is not None:
            raise ValueError("the clean model has no codebook")
        return model.bound, model.encoder.tables(), None, fo.pack_weights(model.sigma_net.params, model.color_net.params)
    raise TypeError(f"lattice: expected a NeRFNetwork or a CleanNeRFNetwork, got {type(model).__name__}")


@torch.no_grad()
def lattice(model, bound_min, bound_max, resolution, message=None):
    """The fp32 density lattice [R,R,R] (z fastest) of `model` over [bound_min, bound_max]: bit-identical to the reference's
    extract_fields(bound_min, bound_max, R, lambda pts: model.density(pts, message)['sigma']).

    The axes are extract_fields' CPU linspace, uploaded once.  The points are evaluated by field_forward (sigma only) in chunks of about
    2 M, each at least fieldops.PLANES_MIN_POINTS (the route the reference's 128^3 chunks take) when the lattice has that many, and queried
    x fastest: hash-table rows of x-neighbours share cache lines.  Every point's density is independent of its neighbours, so neither the
    chunking nor the order changes a bit."""
    R = int(resolution)
    if R < 2:
        raise ValueError(f"lattice: resolution must be at least 2, got {R}")
    bound, tables, S, packed = _field_of(model, message)
    dev = packed.device
    ax = torch.stack(_axes(bound_min, bound_max, R)).to(dev)          # [3, R]
    total = R ** 3
    n_chunks = max(1, math.ceil(total / LATTICE_CHUNK))
    step = math.ceil(total / n_chunks)
    out = torch.empty(total, dtype=torch.float32, device=dev)       # (k, j, i): x fastest
    for s in range(0, total, step):
        idx = torch.arange(s, min(total, s + step), dtype=torch.int64, device=dev)
        pts = torch.stack([ax[0][idx % R], ax[1][(idx // R) % R], ax[2][idx // (R * R)]], dim=-1)
        sigma, _, _, _ = fo.field_forward(pts, None, bound, tables, S, packed, want_rgb=False, want_geo=False)
        out[s:s + idx.shape[0]] = sigma
    return out.view(R, R, R).permute(2, 1, 0).contiguous()


@torch.no_grad()
def query_lattice(bound_min, bound_max, resolution, query_func, device=None):
    """extract_fields with the lattice kept on the device: the same axes, 128^3 chunks and point order, any callable, no per-chunk host copy."""
    R = int(resolution)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    X, Y, Z = (a.to(dev).split(REFERENCE_CHUNK) for a in _axes(bound_min, bound_max, R))
    u = torch.empty(R, R, R, dtype=torch.float32, device=dev)
    S = REFERENCE_CHUNK
    for xi, xs in enumerate(X):
        for yi, ys in enumerate(Y):
            for zi, zs in enumerate(Z):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                val = query_func(pts).reshape(len(xs), len(ys), len(zs)).detach()
                u[xi * S:xi * S + len(xs), yi * S:yi * S + len(ys), zi * S:zi * S + len(zs)] = val.to(dev, torch.float32)
    return u


def _host(b):
    return b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)


def to_world(vertices, triangles, bound_min, bound_max, resolution):
    """Device lattice-space mesh -> (float64 world vertices [V,3], int64 triangles [T,3]) as numpy, by extract_geometry's own mapping."""
    v = vertices.cpu().numpy().astype(np.float64)
    t = triangles.cpu().numpy().astype(np.int64)
    b_max_np, b_min_np = _host(bound_max), _host(bound_min)
    return v / (resolution - 1.0) * (b_max_np - b_min_np)[None, :] + b_min_np[None, :], t


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func):
    """The reference's extract_geometry (nerf/utils.py:192): (float64 world vertices, int64 triangles) as numpy arrays.  The lattice is
    evaluated through query_func on the device (the bounds' device when they are GPU tensors) and marched on the GPU."""
    dev = bound_min.device if isinstance(bound_min, torch.Tensor) and bound_min.is_cuda else None
    u = query_lattice(bound_min, bound_max, resolution, query_func, device=dev)
    v, t = marching_cubes(u, threshold)
    return to_world(v, t, bound_min, bound_max, resolution)


def write_ply(path, vertices, triangles):
    """Binary little-endian PLY: double x, y, z per vertex; list uchar int vertex_indices per face."""
    vertices = np.ascontiguousarray(vertices, dtype="<f8").reshape(-1, 3)
    triangles = np.asarray(triangles).reshape(-1, 3)
    faces = np.empty(triangles.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"] = 3
    faces["v"] = triangles
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {vertices.shape[0]}\nproperty double x\nproperty double y\nproperty double z\n"
              f"element face {triangles.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vertices.tobytes())
        f.write(faces.tobytes())


def save_mesh(model, path, resolution=256, threshold=10, message=None):
    """Trainer.save_mesh (nerf/utils.py:611): the mesh of `model`'s density over aabb_infer, written to `path` as a binary PLY.
    Returns (vertex count, triangle count)."""
    bmin, bmax = model.aabb_infer[:3], model.aabb_infer[3:]
    u = lattice(model, bmin, bmax, resolution, message)
    v, t = marching_cubes(u, threshold)
    vertices, triangles = to_world(v, t, bmin, bmax, resolution)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    write_ply(path, vertices, triangles)
    return vertices.shape[0], triangles.shape[0]
