"""Vectorised numpy restatement of the marching cubes of csrc/mesh.hip, element for element: the same table (mc_table.py), the same
vertex and triangle order and the same fp32 formulas (include/nerfsig.h, mc_count / mc_emit).  Test support only."""
import numpy as np

from nerf_signature_amd import mc_table

_TAB = mc_table.table()
TRI_COUNT = np.array([len(t) for t in _TAB], np.int64)
MAX_TRIS = int(TRI_COUNT.max())
TRI_EDGES = np.full((256, MAX_TRIS, 3), -1, np.int64)
for _c, _t in enumerate(_TAB):
    if _t:
        TRI_EDGES[_c, :len(_t)] = _t
EDGE_CORNER = np.array([c for _, c in mc_table.EDGES], np.int64)
EDGE_AXIS = np.array([a for a, _ in mc_table.EDGES], np.int64)
CORNER_OFF = np.array(mc_table.CORNERS, np.int64)     # [8, 3]


def marching_cubes(u, threshold):
    """(vertices float32 [V,3] in lattice space, triangles int32 [T,3]) of u[nx,ny,nz] at `threshold` (inside: u > threshold)."""
    u = np.ascontiguousarray(u, dtype=np.float32)
    nx, ny, nz = u.shape
    thr = np.float32(threshold)
    inside = u > thr
    # crossing bits of every node's +x, +y, +z edges
    bits = np.zeros(u.shape, np.uint8)
    bits[:-1, :, :] |= (inside[:-1] != inside[1:]).astype(np.uint8)
    bits[:, :-1, :] |= (inside[:, :-1] != inside[:, 1:]).astype(np.uint8) << 1
    bits[:, :, :-1] |= (inside[:, :, :-1] != inside[:, :, 1:]).astype(np.uint8) << 2
    flat_bits = bits.reshape(-1).astype(np.int64)
    cnt = (flat_bits & 1) + ((flat_bits >> 1) & 1) + ((flat_bits >> 2) & 1)
    vbase = np.cumsum(cnt) - cnt

    # vertices: by node in C order, then axis
    keys = np.sort(np.concatenate([np.flatnonzero((flat_bits >> a) & 1) * 3 + a for a in range(3)]))
    node, axis = keys // 3, keys % 3
    i, j, k = np.unravel_index(node, u.shape)
    strides = np.array([ny * nz, nz, 1], np.int64)
    a = u.reshape(-1)[node]
    b = u.reshape(-1)[node + strides[axis]]
    with np.errstate(all="ignore"):
        t = (thr - a) / (b - a)
    t = np.where(np.isnan(t), np.float32(0.5), np.clip(t, np.float32(0), np.float32(1))).astype(np.float32)
    vertices = np.stack([i, j, k], axis=-1).astype(np.float32)
    vertices[np.arange(node.size), axis] += t

    # triangles: by cell in C order, then in table order
    cases = np.zeros((nx - 1, ny - 1, nz - 1), np.uint8)
    for c, (dx, dy, dz) in enumerate(mc_table.CORNERS):
        cases |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.uint8) << c
    cells = np.flatnonzero(cases)                               # C order over the (nx-1, ny-1, nz-1) cells
    cases = cases.reshape(-1)[cells].astype(np.int64)
    ci, cj, ck = np.unravel_index(cells, (nx - 1, ny - 1, nz - 1))
    n_tri = TRI_COUNT[cases]
    cell = np.repeat(np.arange(cases.size), n_tri)
    slot = np.arange(cell.size) - np.repeat(np.cumsum(n_tri) - n_tri, n_tri)
    edges = TRI_EDGES[cases[cell], slot]                        # [T, 3]
    base = (ci[cell] * ny + cj[cell]) * nz + ck[cell]
    off = CORNER_OFF[EDGE_CORNER[edges]]                        # [T, 3, 3]
    owner = base[:, None] + off[..., 0] * ny * nz + off[..., 1] * nz + off[..., 2]
    ax = EDGE_AXIS[edges]
    below = flat_bits[owner] & ((1 << ax) - 1)
    vid = vbase[owner] + (below & 1) + ((below >> 1) & 1)
    return vertices, vid.astype(np.int32).reshape(-1, 3)


def to_world(vertices, bound_min, bound_max, resolution):
    """extract_geometry's mapping (nerf/utils.py:200-203)."""
    b_max_np, b_min_np = np.asarray(bound_max), np.asarray(bound_min)
    return vertices.astype(np.float64) / (resolution - 1.0) * (b_max_np - b_min_np)[None, :] + b_min_np[None, :]


# ---- PLY ------------------------------------------------------------------------------------------------------------------------------------------------

def read_ply(path):
    """The binary little-endian PLY of write_ply: (float64 vertices [V,3], int64 faces [T,3])."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    V = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[-1])
    T = int(next(ln for ln in lines if ln.startswith("element face")).split()[-1])
    assert [ln for ln in lines if ln.startswith("property")] == ["property double x", "property double y", "property double z",
                                                                 "property list uchar int vertex_indices"]
    verts = np.frombuffer(data, "<f8", 3 * V, end).reshape(V, 3)
    faces = np.frombuffer(data, [("n", "u1"), ("v", "<i4", (3,))], T, end + 24 * V)
    assert (faces["n"] == 3).all() and len(data) == end + 24 * V + 13 * T
    return verts, faces["v"].astype(np.int64)


# ---- mesh checks ----------------------------------------------------------------------------------------------------------------------------------------

def directed_edges(tris):
    t = np.asarray(tris, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_oriented(tris):
    """Every directed edge has its reverse exactly once (and appears once itself): closed, 2-manifold along edges, consistently oriented."""
    d = directed_edges(tris)
    if d.size == 0:
        return True
    n = int(d.max()) + 1
    key = d[:, 0] * n + d[:, 1]
    rkey = d[:, 1] * n + d[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    if counts.max() != 1:
        return False
    return bool(np.isin(rkey, uniq).all())


def undirected_edge_counts(tris):
    d = np.sort(directed_edges(tris), axis=1)
    _, counts = np.unique(d[:, 0] * (int(d.max()) + 1) + d[:, 1], return_counts=True)
    return counts


def euler_characteristic(n_vertices, tris):
    return n_vertices - undirected_edge_counts(tris).size + len(tris)


def signed_volume(vertices, tris):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
