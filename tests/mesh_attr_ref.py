"""Numpy restatement of the mesh attributes and cleaning of csrc/mesh.hip and mesh.py: the vertex-normal formula in fp32, operation by
operation (include/nerfsig.h, mc_vertex_normals), in mc_ref's vertex order; connected components by a plain union-find; the component
filter and its stable compaction; a PLY reader for the attribute records and the PLY writer as it was before attributes existed.
Test support only."""
import numpy as np

F = np.float32


# ---- normals --------------------------------------------------------------------------------------------------------------------------------------------

def node_gradients(u):
    """[3, nx, ny, nz]: per axis (u[i+1] - u[i-1]) * 0.5 inside, u[1] - u[0] and u[n-1] - u[n-2] at the ends, in u's dtype."""
    g = np.empty((3,) + u.shape, u.dtype)
    half = u.dtype.type(0.5)
    with np.errstate(all="ignore"):
        for c in range(3):
            a = np.moveaxis(u, c, 0)
            o = np.moveaxis(g[c], c, 0)
            o[1:-1] = (a[2:] - a[:-2]) * half
            o[0] = a[1] - a[0]
            o[-1] = a[-1] - a[-2]
    return g


def crossings(u, threshold):
    """(node, axis) of every vertex in mc_emit's order: by node in C order, then by axis, one per owned crossing edge (as mc_ref.marching_cubes)."""
    inside = u > u.dtype.type(threshold)
    bits = np.zeros(u.shape, np.uint8)
    bits[:-1, :, :] |= (inside[:-1] != inside[1:]).astype(np.uint8)
    bits[:, :-1, :] |= (inside[:, :-1] != inside[:, 1:]).astype(np.uint8) << 1
    bits[:, :, :-1] |= (inside[:, :, :-1] != inside[:, :, 1:]).astype(np.uint8) << 2
    flat = bits.reshape(-1).astype(np.int64)
    keys = np.sort(np.concatenate([np.flatnonzero((flat >> a) & 1) * 3 + a for a in range(3)]))
    return keys // 3, keys % 3


def vertex_normals(u, threshold, scale=(1.0, 1.0, 1.0), dtype=np.float32):
    """(normals [V,3], scaled gradients [V,3]) of the vertices of mc_ref.marching_cubes(u, threshold), every operation rounded to `dtype` on its own
    (float32: the kernel's arithmetic; float64: the same formula without fp32 rounding, on the same lattice values)."""
    u = np.ascontiguousarray(u, dtype=np.float32).astype(dtype)
    T = u.dtype.type
    nx, ny, nz = u.shape
    thr = T(np.float32(threshold))
    node, axis = crossings(u, thr)
    strides = np.array([ny * nz, nz, 1], np.int64)
    other = node + strides[axis]
    flat = u.reshape(-1)
    a, b = flat[node], flat[other]
    with np.errstate(all="ignore"):
        t = (thr - a) / (b - a)
        t = np.where(np.isnan(t), T(0.5), np.clip(t, T(0), T(1))).astype(dtype)
        G = node_gradients(u).reshape(3, -1)
        g = np.empty((node.size, 3), dtype)
        for c in range(3):
            ga, gb = G[c][node], G[c][other]
            g[:, c] = (ga + t * (gb - ga)) * T(np.float32(scale[c]))
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = (length > 0) & (length < np.inf)
        n = np.where(ok[:, None], -g / length[:, None], T(0)).astype(dtype)
    return n, g


# ---- components -----------------------------------------------------------------------------------------------------------------------------------------

def components(triangles, n_vertices):
    """labels [V] int32: the smallest vertex id of each vertex's component, by a plain union-find over the three sides of every triangle."""
    parent = list(range(n_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(triangles, np.int64).reshape(-1, 3).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)        # the smaller id stays the root
    return np.array([find(v) for v in range(n_vertices)], np.int32).reshape(n_vertices)


def clean(vertices, triangles, min_triangles=0, keep_largest=None, attributes=()):
    """mesh.clean in numpy: (vertices, triangles, *attributes) with the small components removed, order kept, ids remapped."""
    vertices, triangles = np.asarray(vertices), np.asarray(triangles).reshape(-1, 3)
    V = vertices.shape[0]
    labels = components(triangles, V).astype(np.int64)
    tlabel = labels[triangles[:, 0]]
    count = np.bincount(tlabel, minlength=V)
    keep = count >= max(int(min_triangles), 1)
    if keep_largest is not None:
        order = np.lexsort((np.arange(V), -count))[:int(keep_largest)]      # most triangles first, ties to the smaller label
        top = np.zeros(V, bool)
        top[order] = True
        keep &= top
    used = np.zeros(V, bool)
    used[triangles.reshape(-1)] = True
    vkeep = keep[labels] & used
    tkeep = keep[tlabel]
    new_id = np.cumsum(vkeep) - 1
    out_t = new_id[triangles[tkeep]].astype(np.int32).reshape(-1, 3)
    return (vertices[vkeep], out_t) + tuple(np.asarray(a)[vkeep] for a in attributes)


# ---- PLY ------------------------------------------------------------------------------------------------------------------------------------------------

def write_ply_before_attributes(path, vertices, triangles):
    """mesh.write_ply as it was when it wrote geometry alone: the byte-for-byte yardstick of the default path."""
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


_PROPS = {"double": "<f8", "float": "<f4", "uchar": "u1"}


def read_ply(path):
    """The binary PLY of mesh.write_ply with any of its vertex records -> dict: 'vertices' float64 [V,3], 'faces' int64 [T,3], and
    'normals' float32 [V,3] / 'colors' uint8 [V,3] when the file has them."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    V = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[-1])
    T = int(next(ln for ln in lines if ln.startswith("element face")).split()[-1])
    props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
    assert props[-1] == ["list", "uchar", "int", "vertex_indices"]
    names = [p[1] for p in props[:-1]]
    assert names in (["x", "y", "z"], ["x", "y", "z", "nx", "ny", "nz"], ["x", "y", "z", "red", "green", "blue"],
                     ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]), names
    rec = np.dtype([(p[1], _PROPS[p[0]]) for p in props[:-1]])
    verts = np.frombuffer(data, rec, V, end)
    faces = np.frombuffer(data, [("n", "u1"), ("v", "<i4", (3,))], T, end + rec.itemsize * V)
    assert (faces["n"] == 3).all() and len(data) == end + rec.itemsize * V + 13 * T
    out = {"vertices": np.stack([verts[k] for k in "xyz"], -1), "faces": faces["v"].astype(np.int64)}
    assert out["vertices"].dtype == np.float64
    if "nx" in names:
        out["normals"] = np.stack([verts[k] for k in ("nx", "ny", "nz")], -1)
        assert out["normals"].dtype == np.float32
    if "red" in names:
        out["colors"] = np.stack([verts[k] for k in ("red", "green", "blue")], -1)
        assert out["colors"].dtype == np.uint8
    return out


def quantize_colors(rgb):
    """uint8(floor(clamp(c, 0, 1) * 255 + 0.5)) in fp32."""
    c = np.clip(np.asarray(rgb, np.float32), F(0), F(1))
    return np.floor(c * F(255) + F(0.5)).astype(np.uint8)


# ---- meshes the tests share -----------------------------------------------------------------------------------------------------------------------------

def ball(shape, centre, radius):
    """radius - distance to centre on a lattice, float32 (positive inside)."""
    g = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return (radius - np.sqrt(sum((x - c) ** 2 for x, c in zip(g, centre)))).astype(np.float32)


def two_spheres_and_specks():
    """A 40 x 36 x 32 lattice at threshold 0: a ball of radius 9, one of radius 5.5, one inside node far from both (a closed octahedron of 8
    triangles) and the corner node (0, 0, 0) inside (one open triangle)."""
    shape = (40, 36, 32)
    u = np.maximum(ball(shape, (13.2, 14.1, 15.3), 9.0), ball(shape, (30.4, 25.2, 16.6), 5.5))
    u[33, 6, 6] = 0.7
    u[0, 0, 0] = 0.4
    return u


def noise_lattice(n=33, seed=11, level=1.2):
    """Seeded noise with the border pushed outside: at `level` the inside nodes are sparse, so the mesh is hundreds of small closed components (the
    smallest, one inside node, an octahedron of 8 triangles).  Three corner nodes and one face node are inside on their own: open pieces of 1 and 4
    triangles, the only ones a filter at 8 triangles removes."""
    u = np.random.default_rng(seed).standard_normal((n, n, n)).astype(np.float32)
    u[[0, -1], :, :] = u[:, [0, -1], :] = u[:, :, [0, -1]] = -1.0
    u[0, 0, 0] = u[-1, -1, -1] = u[0, -1, 0] = u[0, n // 2, n // 2] = 2.0
    u[1, n // 2, n // 2] = -1.0
    return u, level
