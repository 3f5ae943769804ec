"""Small meshes for the rasteriser's tests, built in SCREEN space first: fixed-point coordinates on the 1/256 pixel grid and depths that are powers of two,
un-projected with the identity pose and power-of-two intrinsics, so that projection reproduces the coordinates exactly and snapping moves nothing."""
import numpy as np

IDENTITY = np.eye(4, dtype=np.float32)
INTR16 = (16.0, 16.0, 8.0, 8.0)      # for 16 x 16 images


def unproject(xy_fixed, z, intrinsics=INTR16):
    """Screen points (int, units of 1/256 pixel) at camera depths z -> float32 world positions under the identity pose; exact for power-of-two fx, fy and z."""
    fx, fy, cx, cy = intrinsics
    xy = np.asarray(xy_fixed, np.float64) / 256.0
    z = np.asarray(z, np.float64)
    p = np.stack([(xy[:, 0] - cx) / fx * z, (xy[:, 1] - cy) / fy * z, z], axis=1)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32)


def exact_mesh(seed=7, n_triangles=20):
    """About twenty random triangles over (and a little beyond) a 16 x 16 image: every triangle its own three vertices, coordinates anywhere on the 1/256 grid
    in [-3, 19) pixels, depths in {1, 2, 4}, random colours; triangle 3 is repeated as the last one, and one triangle has all corners on pixel centres.
    -> (xy int64 [V, 2], z float64 [V], vertices float32 [V, 3], triangles int32 [T, 3], colors float32 [V, 3])"""
    rng = np.random.RandomState(seed)
    T = n_triangles
    xy = rng.randint(-3 * 256, 19 * 256, size=(3 * T, 2)).astype(np.int64)
    xy[:3] = [[2 * 256 + 128, 1 * 256 + 128], [12 * 256 + 128, 1 * 256 + 128], [2 * 256 + 128, 11 * 256 + 128]]      # corners and two edges on pixel centres
    z = rng.choice([1.0, 2.0, 4.0], size=3 * T)
    z[2::3] = np.where((z[0::3] == z[1::3]) & (z[1::3] == z[2::3]), np.where(z[2::3] == 2.0, 4.0, 2.0), z[2::3])      # no flat triangle: two of one depth would tie wherever they overlap
    tris =np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    tris = np.concatenate([tris, tris[3:4]])
    colors = rng.rand(3 * T, 3).astype(np.float32)
    return xy, z, unproject(xy, z), tris, colors


def fan():
    """A closed fan of eight triangles about the pixel centre (8.5, 8.5), rim 16 pixels away along the axes and diagonals: it covers the whole 16 x 16 image,
    every spoke passes exactly through pixel centres, and the windings alternate."""
    h = np.array([8 * 256 + 128, 8 * 256 + 128])
    r = 16 * 256
    rim = [h + np.array(d) * r for d in ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))]
    xy = np.array([h] + rim, np.int64)
    tris = np.array([[0, 1 + k, 1 + (k + 1) % 8] if k % 2 == 0 else [0, 1 + (k + 1) % 8, 1 + k] for k in range(8)], np.int32)
    z = np.array([1.0] + [2.0, 4.0] * 4)
    return xy, z, unproject(xy, z), tris


def strip():
    """Six triangles zig-zagging between the rows y = 2.5 and y = 6.5 from x = 0.5 to x = 12.5: the outline and every shared edge pass through pixel centres.
    With the top-left rule the covered centres are exactly rows 2 .. 5, columns 0 .. 11."""
    xs = [0, 4, 8, 12]
    top = [[x * 256 + 128, 2 * 256 + 128] for x in xs]
    bot = [[x * 256 + 128, 6 * 256 + 128] for x in xs]
    xy = np.array(top + bot, np.int64)
    tris = []
    for k in range(3):
        tris += [[k, 4 + k, k + 1], [k + 1, 4 + k, 4 + k + 1]]
    z = np.array([1.0, 2.0, 1.0, 2.0, 2.0, 4.0, 2.0, 4.0])
    want = np.zeros((16, 16), np.int64)
    want[2:6, 0:12] = 1
    return xy, z, unproject(xy, z), np.array(tris, np.int32), want


def slanted_quad():
    """A quad over columns 2 .. 14, rows 4 .. 12 whose left side is at depth 1 with colour 0 and whose right side is at depth 4 with colour 1; the centre of
    pixel (8, 8) -- column, row -- lies at the middle of its width.  Perspective-correct colour there: (0.5 * 0.25) / (0.5 * 1 + 0.5 * 0.25) = 0.2; affine: 0.5."""
    xy = np.array([[2 * 256 + 128, 4 * 256], [14 * 256 + 128, 4 * 256], [14 * 256 + 128, 12 * 256], [2 * 256 + 128, 12 * 256]], np.int64)
    z = np.array([1.0, 4.0, 4.0, 1.0])
    colors = np.array([[0, 0, 0], [1, 1, 1], [1, 1, 1], [0, 0, 0]], np.float32)
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    return xy, z, unproject(xy, z), tris, colors
