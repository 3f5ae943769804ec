"""Mesh extraction: marching cubes over the trained density field on the GPU (nerf/utils.py:174-204 and Trainer.save_mesh, :611-631).

The reference evaluates `model.density` on a 256^3 lattice in 128^3 chunks, copies every chunk to the host, runs mcubes.marching_cubes
on the CPU and exports a PLY through trimesh.  Here the lattice stays on the device and the marching cubes are HIP kernels
(csrc/mesh.hip, table csrc/mc_tables.h from mc_table.py); only the finished mesh is copied back.

    marching_cubes(u, threshold, normals=False)               -> vertices [V,3] fp32, triangles [T,3] int32 (device, lattice space)[, normals [V,3]]
    lattice(model, bound_min, bound_max, resolution, message) -> the fp32 [R,R,R] density lattice, bit-identical to extract_fields
    extract_geometry(bound_min, bound_max, resolution, threshold, query_func)   the reference's signature and return types
    save_mesh(model, path, resolution=256, threshold=10, message=None, ...)     binary PLY over aabb_infer; returns (V, T)

Opt-in mesh attributes and cleaning, all on the device ("Mesh attributes"):

    vertex_normals(u, threshold, scratch=None, scale=(1, 1, 1))   the normals of marching_cubes' vertices (mc_vertex_normals)
    vertex_colors(model, vertices_world, normals, message=None, directions=None)   the colour head seen against the normal (or along given directions), rgb [V,3] fp32
    occupied(model, bound_min, bound_max, resolution)             which lattice nodes lie in cells the model's occupancy bitfield marks, bool [R,R,R]
    read_ply(path)                                                what write_ply wrote, back (raster.render_mesh draws it: tools/mesh_view.py)
    components(triangles, n_vertices)                             labels [V] int32: the smallest vertex id of each component (mesh_components)
    clean(vertices, triangles, min_triangles=0, keep_largest=None, attributes=())   drop small components, stable compaction

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


def _check_lattice(u, who):
    if not isinstance(u, torch.Tensor) or not u.is_cuda:
        raise ValueError(f"{who}: the lattice must be a tensor on the GPU (there is no CPU path)")
    if u.dtype != torch.float32:
        raise ValueError(f"{who}: the lattice must be float32, got {u.dtype}")
    if u.dim() != 3:
        raise ValueError(f"{who}: the lattice must be 3-D, got shape {tuple(u.shape)}")
    nx, ny, nz = (int(s) for s in u.shape)
    if min(nx, ny, nz) < 2:
        raise ValueError(f"{who}: every lattice dimension must be at least 2, got {tuple(u.shape)}")
    if nx * ny * nz > MAX_NODES:
        raise ValueError(f"{who}: {nx} x {ny} x {nz} nodes is above the limit of 2^28")
    return nx, ny, nz


class McScratch:
    """What mc_emit leaves behind for vertex_normals: the (contiguous) lattice, the threshold, the scratch with the node codes and vertex bases, and V."""

    def __init__(self, u, threshold, buf, n_vertices):
        self.u, self.threshold, self.buf, self.n_vertices = u, threshold, buf, n_vertices


def _march(u, threshold, who="marching_cubes"):
    nx, ny, nz = _check_lattice(u, who)
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
    return vertices, triangles, McScratch(u, thr, scratch, V)


def marching_cubes(u, threshold, normals=False, scale=(1.0, 1.0, 1.0)):
    """Marching cubes of the device lattice u[nx, ny, nz] (fp32, z fastest) at `threshold` (inside: u > threshold) -> (vertices float32 [V,3],
    triangles int32 [T,3]) on u's device, vertices in lattice space (the counterpart of mcubes.marching_cubes).  Output order: include/nerfsig.h.
    normals=True: -> (vertices, triangles, normals float32 [V,3]), the vertex normals of vertex_normals(u, threshold, scale=scale) from the same scratch."""
    vertices, triangles, scratch = _march(u, threshold)
    if normals:
        return vertices, triangles, vertex_normals(scratch.u, threshold, scratch, scale)
    return vertices, triangles


def vertex_normals(u, threshold, scratch=None, scale=(1.0, 1.0, 1.0), gradients=False):
    """Unit normals float32 [V,3] of the vertices marching_cubes(u, threshold) returns, in their order: minus the lattice's finite-difference gradient,
    interpolated along the vertex's edge, scaled per axis and normalised, all in fp32 (include/nerfsig.h, mc_vertex_normals); (0, 0, 0) where the
    gradient is zero or not finite.  scratch: the McScratch of the marching-cubes call on this very lattice and threshold, or None to recompute it.
    scale: lattice steps per world unit along x, y, z -- (R - 1) / (bound_max - bound_min) for world-space normals (lattice_scale), ones for lattice
    space.  gradients=True: -> (normals, the scaled gradients before the division)."""
    nx, ny, nz = _check_lattice(u, "vertex_normals")
    thr = float(threshold)
    if scratch is None:
        scratch = _march(u, thr, "vertex_normals")[2]
    elif scratch.threshold != thr or tuple(scratch.u.shape) != (nx, ny, nz) or scratch.u.device != u.device:
        raise ValueError("vertex_normals: the scratch belongs to another lattice or threshold")
    sx, sy, sz = (float(x) for x in scale)
    dev, V = u.device, scratch.n_vertices
    with torch.cuda.device(dev):
        normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
        grads = torch.empty(V, 3, dtype=torch.float32, device=dev) if gradients else None
        nv.call("mc_vertex_normals", nv.ptr(scratch.u), nx, ny, nz, thr, nv.ptr(scratch.buf), V, sx, sy, sz, nv.ptr(normals) if V else None,
                nv.ptr(grads) if V else None, nv.stream())
    return (normals, grads) if gradients else normals


def lattice_scale(bound_min, bound_max, resolution):
    """vertex_normals' scale for world-space normals of an R^3 lattice over [bound_min, bound_max]: (R - 1) / (bound_max - bound_min) per axis."""
    lo, hi = _host(bound_min), _host(bound_max)
    return tuple((resolution - 1.0) / (float(hi[a]) - float(lo[a])) for a in range(3))


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
def occupied(model, bound_min, bound_max, resolution):
    """bool [R,R,R] on the model's device: which nodes of lattice()'s lattice lie in a cell the model's occupancy bitfield marks -- the only places a render of the
    model ever evaluates the field.  The cascade of a node is the smallest whose cube holds it (the marcher's rule for a position), the cell floor((p / extent + 1) / 2 *
    grid_size) clamped, the bit at its morton index (x -> bit 0).  `torch.where(occupied(...), lattice(...), -1)` is the density a render can see."""
    R, G, C = int(resolution), int(model.grid_size), int(model.cascade)
    dev = model.density_bitfield.device
    ax = torch.stack(_axes(bound_min, bound_max, R)).to(dev)
    p = torch.stack(torch.meshgrid(ax[0], ax[1], ax[2], indexing="ij"), dim=-1).reshape(-1, 3)
    linf = p.abs().amax(dim=-1).clamp_min(1e-6)
    cas = torch.ceil(torch.log2(linf)).clamp(0, C - 1).long()
    extent = torch.minimum(torch.pow(2.0, cas.float()), torch.tensor(float(model.bound), device=dev))
    cell = torch.floor((p / extent[:, None] + 1.0) * (0.5 * G)).long().clamp(0, G - 1)

    def spread(v):
        v = (v * 0x00010001) & 0xFF0000FF
        v = (v * 0x00000101) & 0x0F00F00F
        v = (v * 0x00000011) & 0xC30C30C3
        return (v * 0x00000005) & 0x49249249

    bit = cas * G ** 3 + (spread(cell[:, 0]) | (spread(cell[:, 1]) << 1) | (spread(cell[:, 2]) << 2))
    byte = model.density_bitfield[bit >> 3].long()
    return ((byte >> (bit & 7)) & 1).bool().view(R, R, R)


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


def world_vertices(vertices, bound_min, bound_max, resolution):
    """to_world's mapping on the device: float64 [V,3] world positions of lattice-space vertices (the same operations in the same order)."""
    dev = vertices.device
    lo = torch.as_tensor(_host(bound_min)).to(dev)
    hi = torch.as_tensor(_host(bound_max)).to(dev)
    steps = torch.full((1, 1), resolution - 1.0, dtype=torch.float64, device=dev)      # a tensor: a Python scalar divisor becomes a multiplication by its reciprocal
    return vertices.double() / steps * (hi - lo).double()[None, :] + lo.double()[None, :]


@torch.no_grad()
def vertex_colors(model, vertices_world, normals, message=None, directions=None):
    """rgb float32 [V,3] on the device: the model's colour head at every vertex, seen against the normal -- position float32(vertices_world), view
    direction -normal, (0, 0, 1) where the normal is zero.  Queried through field_forward as lattice() queries the density (NeRFNetwork with or without a
    message, CleanNeRFNetwork), in chunks of about 2 M vertices: up to one chunk the result is bit-equal to one model(x, d, message) call on these rows.
    directions: view directions [V,3] to use as they are instead of -normal (raster.view_directions: the mesh coloured as one camera sees the field);
    the normals are then not looked at and may be None."""
    bound, tables, S, packed = _field_of(model, message)
    dev = packed.device
    x = torch.as_tensor(vertices_world).to(dev, torch.float32).reshape(-1, 3).contiguous()
    if directions is not None:
        d = torch.as_tensor(directions).to(dev, torch.float32).reshape(-1, 3).contiguous()
        if d.shape != x.shape:
            raise ValueError(f"vertex_colors: {x.shape[0]} vertices with {d.shape[0]} directions")
    else:
        n = torch.as_tensor(normals).to(dev, torch.float32).reshape(-1, 3)
        if n.shape != x.shape:
            raise ValueError(f"vertex_colors: {x.shape[0]} vertices with {n.shape[0]} normals")
        zero = (n == 0).all(dim=-1, keepdim=True)
        d = torch.where(zero, torch.tensor([0.0, 0.0, 1.0], device=dev), -n).contiguous()
    V = x.shape[0]
    rgb = torch.empty(V, 3, dtype=torch.float32, device=dev)
    n_chunks = max(1, math.ceil(V / LATTICE_CHUNK))
    step = max(1, math.ceil(V / n_chunks))
    for s in range(0, V, step):
        _, c, _, _ = fo.field_forward(x[s:s + step], d[s:s + step], bound, tables, S, packed)
        rgb[s:s + step] = c
    return rgb


def quantize_colors(rgb):
    """The PLY's bytes of float colours: uint8(floor(clamp(c, 0, 1) * 255 + 0.5)) (numpy array or tensor, same kind back)."""
    if isinstance(rgb, torch.Tensor):
        return torch.floor(rgb.float().clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
    c = np.clip(np.asarray(rgb, np.float32), np.float32(0), np.float32(1))
    return np.floor(c * np.float32(255) + np.float32(0.5)).astype(np.uint8)


# ---- components and cleaning ------------------------------------------------------------------------------------------------------------------------------

CC_OK = 0xFFFFFFFF           # mesh_components' status word when every id was in range
MAX_ELEMENTS = 1 << 31       # mesh_components: V, T below 2^31


def _check_triangles(triangles, who):
    if not isinstance(triangles, torch.Tensor) or not triangles.is_cuda:
        raise ValueError(f"{who}: the triangles must be a tensor on the GPU (there is no CPU path)")
    if triangles.dtype != torch.int32 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"{who}: the triangles must be int32 [T,3], got {triangles.dtype} {tuple(triangles.shape)}")
    return triangles.contiguous()


def _components(triangles, V):
    """(labels [V] int32, status [1] int64 on the device: CC_OK or the first triangle with an id outside [0, V)); nothing is read back."""
    T = int(triangles.shape[0])
    if not 0 <= V < MAX_ELEMENTS or T >= MAX_ELEMENTS:
        raise ValueError(f"components: V={V}, T={T} out of range (each below 2^31)")
    dev = triangles.device
    with torch.cuda.device(dev):
        labels = torch.empty(V, dtype=torch.int32, device=dev)
        scratch = torch.empty(int(nv.fn("mesh_components_scratch_bytes")(V, T)), dtype=torch.uint8, device=dev)
        nv.call("mesh_components", nv.ptr(triangles) if T else None, T, V, nv.ptr(labels) if V else None, nv.ptr(scratch), nv.stream())
    return labels, scratch[:4].view(torch.int32).to(torch.int64) & CC_OK


def _refuse_bad_ids(status, V):
    if status != CC_OK:
        raise ValueError(f"components: triangle {status} has a vertex id outside [0, {V})")


def components(triangles, n_vertices):
    """Connected components of the mesh graph (vertices; the sides of every triangle): labels int32 [V] on the device, labels[v] = the smallest vertex id
    of v's component; a vertex in no triangle labels itself.  Any int32 [T,3] triangle list with ids in [0, V); an id outside raises ValueError."""
    triangles = _check_triangles(triangles, "components")
    labels, status = _components(triangles, int(n_vertices))
    _refuse_bad_ids(int(status.item()), int(n_vertices))
    return labels


def _kept(mask):
    """(running count of a bool mask, int64; a function n -> the indices of its n true entries in order, without a host read)."""
    run = torch.cumsum(mask, 0)
    return run, lambda n: torch.searchsorted(run, torch.arange(1, n + 1, dtype=run.dtype, device=run.device))


def clean(vertices, triangles, min_triangles=0, keep_largest=None, attributes=()):
    """Remove small components ("floaters") on the device -> (vertices, triangles, *attributes) compacted.  A component survives if it has at least
    min_triangles triangles and, with keep_largest=k, is among the k components of most triangles (ties: the smaller label first).  Surviving vertices
    and triangles keep their relative order, triangle ids are remapped, every tensor of `attributes` ([V, ...]) is compacted with the vertices, and
    vertices no surviving triangle uses are dropped.  One host read (the new sizes); the mesh is not copied to the host."""
    triangles = _check_triangles(triangles, "clean")
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    if keep_largest is not None and int(keep_largest) < 0 or int(min_triangles) < 0:
        raise ValueError("clean: min_triangles and keep_largest must not be negative")
    for a in attributes:
        if a.shape[0] != V or a.device != vertices.device:
            raise ValueError("clean: every attribute must have one row per vertex, on the vertices' device")
    dev = triangles.device
    labels, status = _components(triangles, V)
    with torch.cuda.device(dev):
        tri = triangles.long().clamp(0, max(V - 1, 0))                    # (ids out of range are refused below, before anything is returned)
        lab = labels.long()
        tlabel = lab[tri[:, 0]] if V else tri[:, 0]
        count = torch.zeros(V, dtype=torch.int64, device=dev).scatter_add_(0, tlabel, torch.ones_like(tlabel))       # triangles per component, at its label
        keep = count >= max(int(min_triangles), 1)
        if keep_largest is not None:
            order = torch.sort(count, descending=True, stable=True).indices[:int(keep_largest)]       # stable: equal counts stay in label order
            top = torch.zeros(V, dtype=torch.bool, device=dev)
            top[order] = True
            keep &= top
        used = torch.zeros(V, dtype=torch.bool, device=dev)
        used[tri.reshape(-1)] = True
        vkeep = keep[lab] & used
        tkeep = keep[tlabel]
        vrun, vidx = _kept(vkeep)
        trun, tidx = _kept(tkeep)
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        Vn, Tn, st = torch.cat([vrun[-1:] if V else zero, trun[-1:] if T else zero, status]).tolist()        # the one host read
        _refuse_bad_ids(st, V)
        vi, ti = vidx(Vn), tidx(Tn)
        new_id = (vrun - 1).to(torch.int32)
        out_t = new_id[triangles.index_select(0, ti).long()]
        return (vertices.index_select(0, vi), out_t) + tuple(a.index_select(0, vi) for a in attributes)


# ---- PLY ----------------------------------------------------------------------------------------------------------------------------------------------

def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Binary little-endian PLY: double x, y, z per vertex, then float nx, ny, nz when normals [V,3] are given, then uchar red, green, blue when
    colors are given (uint8 as they are, floats through quantize_colors); list uchar int vertex_indices per face."""
    vertices = np.ascontiguousarray(vertices, dtype="<f8").reshape(-1, 3)
    triangles = np.asarray(triangles).reshape(-1, 3)
    faces = np.empty(triangles.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"] = 3
    faces["v"] = triangles
    fields, props = [("p", "<f8", (3,))], "property double x\nproperty double y\nproperty double z\n"
    if normals is not None:
        fields.append(("n", "<f4", (3,)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        fields.append(("c", "u1", (3,)))
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    if len(fields) == 1:
        record = vertices
    else:
        record = np.empty(vertices.shape[0], dtype=fields)
        record["p"] = vertices
        if normals is not None:
            record["n"] = np.asarray(normals, dtype="<f4").reshape(vertices.shape[0], 3)
        if colors is not None:
            colors = np.asarray(colors)
            record["c"] = (colors if colors.dtype == np.uint8 else quantize_colors(colors)).reshape(vertices.shape[0], 3)
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {vertices.shape[0]}\n{props}"
              f"element face {triangles.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(record.tobytes())
        f.write(faces.tobytes())


_PLY_VERTEX = ["property double x", "property double y", "property double z"]
_PLY_NORMAL = ["property float nx", "property float ny", "property float nz"]
_PLY_COLOR = ["property uchar red", "property uchar green", "property uchar blue"]


def read_ply(path):
    """The binary PLY write_ply writes, back: {"vertices" float64 [V,3], "triangles" int32 [T,3], "normals" float32 [V,3] or None, "colors" uint8 [V,3] or None}
    as numpy arrays.  Exactly that layout is read -- little-endian binary, double positions, then optional float normals, then optional uchar colours, faces as
    `list uchar int vertex_indices` of three -- and any other is refused with the line or the size that differs."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"read_ply: {path} is not a PLY file (no 'ply' magic or no end_header)")
    lines = data[:end].decode("ascii", "replace").split("\n")[1:-1]
    lines = [" ".join(l.split()) for l in lines if l and not l.startswith(("comment", "obj_info"))]
    body = data[end + len(b"end_header\n"):]

    def expect(got, want):
        if got != want:
            raise ValueError(f"read_ply: unsupported layout: '{got}' where write_ply has '{want}'")

    def count(line, element):
        words = line.split()
        if len(words) != 3 or words[:2] != ["element", element] or not words[2].isdigit():
            raise ValueError(f"read_ply: unsupported layout: '{line}' where write_ply has 'element {element} <count>'")
        return int(words[2])

    if len(lines) < 7:
        raise ValueError(f"read_ply: unsupported layout: a header of {len(lines)} lines")
    expect(lines[0], "format binary_little_endian 1.0")
    V = count(lines[1], "vertex")
    T = count(lines[-2], "face")
    expect(lines[-1], "property list uchar int vertex_indices")
    props = lines[2:-2]
    expect(" / ".join(props[:3]), " / ".join(_PLY_VERTEX))
    rest = props[3:]
    fields = [("p", "<f8", (3,))]
    has_n = rest[:3] == _PLY_NORMAL
    if has_n:
        fields.append(("n", "<f4", (3,)))
        rest = rest[3:]
    has_c = rest[:3] == _PLY_COLOR
    if has_c:
        fields.append(("c", "u1", (3,)))
        rest = rest[3:]
    if rest:
        raise ValueError(f"read_ply: unsupported layout: '{rest[0]}' is no vertex property write_ply writes (double x y z, float nx ny nz, uchar red green blue, in that order)")
    vtype, ftype = np.dtype(fields), np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    want = V * vtype.itemsize + T * ftype.itemsize
    if len(body) != want:
        raise ValueError(f"read_ply: {len(body)} bytes after the header, {want} expected for {V} vertices and {T} triangles")
    rec = np.frombuffer(body, dtype=vtype, count=V)
    faces = np.frombuffer(body, dtype=ftype, count=T, offset=V * vtype.itemsize)
    if T and (faces["n"] != 3).any():
        raise ValueError(f"read_ply: face {int(np.flatnonzero(faces['n'] != 3)[0])} is not a triangle")
    return {"vertices": np.array(rec["p"], dtype=np.float64).reshape(V, 3), "triangles": np.array(faces["v"], dtype=np.int32).reshape(T, 3),
            "normals": np.array(rec["n"], dtype=np.float32).reshape(V, 3) if has_n else None, "colors": np.array(rec["c"], dtype=np.uint8).reshape(V, 3) if has_c else None}


def save_mesh(model, path, resolution=256, threshold=10, message=None, normals=False, colors=False, min_triangles=0, keep_largest=None):
    """Trainer.save_mesh (nerf/utils.py:611): the mesh of `model`'s density over aabb_infer, written to `path` as a binary PLY.
    Returns (vertex count, triangle count).  Opt-in, all computed on the device before the one copy of the finished mesh: normals=True writes world-space
    vertex normals; colors=True writes the colour head seen against the normal (normals are computed for it, written only with normals=True);
    min_triangles / keep_largest remove small components first (clean), and the counts returned are those after cleaning."""
    bmin, bmax = model.aabb_infer[:3], model.aabb_infer[3:]
    u = lattice(model, bmin, bmax, resolution, message)
    want_n = bool(normals or colors)
    v, t, *n = marching_cubes(u, threshold, normals=want_n, scale=lattice_scale(bmin, bmax, resolution))
    if min_triangles or keep_largest is not None:
        v, t, *n = clean(v, t, min_triangles, keep_largest, attributes=n)
    rgb = quantize_colors(vertex_colors(model, world_vertices(v, bmin, bmax, resolution), n[0], message)).cpu().numpy() if colors else None
    vertices, triangles = to_world(v, t, bmin, bmax, resolution)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    write_ply(path, vertices, triangles, normals=n[0].cpu().numpy() if normals else None, colors=rgb)
    return vertices.shape[0], triangles.shape[0]
