"""Host restatement of the density-grid refresh entry points (include/nerfsig.h "The density-grid refresh on the device", csrc/gridrefresh.hip), numpy only.

Written from the header's text and from the reference's update_extra_state (oracle/field_ref.py restates it), not from the kernels.  Nearly all of it is exact:
the draws are integer functions of (seed, refresh count, cascade, draw), the occupied draw is an index into `flatnonzero(grid > 0)`, the EMA is one float32
multiply and one maximum (the library is built without contraction), the bitfield is a strict comparison, the mean sample count is an integer division of an
int64 total.  Two things are not: the probe points (float64 here from the same fp32 inputs; the tests carry the rounding count) and the mean density (float64
here in numpy's order; the device sums in double in another fixed order, so its float32 may sit one ulp away)."""
import numpy as np

from draw_ref import draw64, mix64, stream_key, unit24      # noqa: F401 (the tests read mix64 from here)

MASK32 = (1 << 32) - 1
_U = np.uint64


def stream(seed, it, cas, purpose):
    """The key of one (refresh count, cascade, purpose) stream: purpose 0 the uniform cells, 1 the occupied cells, 2 the jitter.  `it` is read as uint32."""
    return stream_key(seed, (int(it) & MASK32) * 64 + int(cas) * 8 + int(purpose))


def draw(key, i):
    """64 bits of draw i (array of indices) of the stream `key`."""
    return draw64(key, np.asarray(i, dtype=np.uint64))


def u01(bits):
    """The top 24 bits as a fraction: [0, 1) on the 2^-24 grid, exact in float32 and float64."""
    return unit24(np.asarray(bits, dtype=np.uint64) >> _U(40))


def _spread3(v):
    v = np.asarray(v, dtype=np.uint64) & _U(0x3FF)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> _U(b)) & _U(1)) << _U(3 * b)
    return out


def morton(x, y, z):
    """morton3D of 10-bit coordinates: bit b of x at bit 3b, of y at 3b + 1, of z at 3b + 2."""
    return (_spread3(x) | (_spread3(y) << _U(1)) | (_spread3(z) << _U(2))).astype(np.int64)


def uniform_cells(N, H, seed, it, cas):
    """(x, y, z) of the N uniform draws: bits 0.., 20.., 40.. of the draw, masked to the power-of-two grid."""
    b = draw(stream(seed, it, cas, 0), np.arange(N, dtype=np.uint64))
    m = _U(H - 1)
    return (b & m).astype(np.int64), ((b >> _U(20)) & m).astype(np.int64), ((b >> _U(40)) & m).astype(np.int64)


def draw_keys(grid_cas, N, H, seed, it, cas):
    """The key (z*H + y)*H + x of every draw i < 2N of rg_refresh_draw: [0, N) uniform over the grid, [N, 2N) uniform with repetition over the occupied cells
    (`grid_cas > 0`, morton order); a grid without an occupied cell draws cell 0."""
    from oracle import raymarch_ref as orm
    grid_cas = np.asarray(grid_cas, dtype=np.float32).reshape(-1)
    assert grid_cas.size == H ** 3 and H & (H - 1) == 0
    x, y, z = uniform_cells(N, H, seed, it, cas)
    occ = np.flatnonzero(grid_cas > 0)
    total = occ.size
    if total == 0:
        cell = np.zeros(N, np.int64)
    else:
        b = draw(stream(seed, it, cas, 1), np.arange(N, dtype=np.uint64))
        t = ((b >> _U(32)) * _U(total)) >> _U(32)      # (a 32-bit value times a count below 2^30: no wrap)
        cell = occ[t.astype(np.int64)]
    c = orm.morton3D_invert(cell.astype(np.int32)).astype(np.int64)
    x, y, z = np.concatenate([x, c[:, 0]]), np.concatenate([y, c[:, 1]]), np.concatenate([z, c[:, 2]])
    return (z * H + y) * H + x


def points(keys, ids, H, extent, half, seed, it, cas):
    """(xyz [n,3] float64, morton index [n]) of rg_refresh_points: centre (2c/(H-1) - 1)(extent - half) + jitter (2u - 1) half, u the exact 24-bit draw
    3*id + axis of the jitter stream.  extent and half are taken as the float32 values the entry point receives; everything after that is float64."""
    keys, ids = np.asarray(keys, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    e, h = float(np.float32(extent)), float(np.float32(half))
    c = np.stack([keys % H, (keys // H) % H, keys // (H * H)], axis=-1)
    key = stream(seed, it, cas, 2)
    j = _U(3) * ids.astype(np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :]
    u = u01(draw(key, j))
    xyz = (2.0 * c.astype(np.float64) / (H - 1) - 1.0) * (e - h) + (u * 2.0 - 1.0) * h
    return xyz, morton(c[:, 0], c[:, 1], c[:, 2])


def scatter(sigmas, cells, scale, n_cells):
    """fresh [n_cells] float32 of rg_refresh_begin + rg_refresh_scatter: -1 where nothing landed; a candidate sigma * scale (one float32 product) lands where the
    reference's `tmp >= 0` would hold (-0.0 lands, as +0) or where it is NaN (kept visible, and winning over every number); the largest candidate of a cell wins."""
    v = (np.asarray(sigmas, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    cells = np.asarray(cells, dtype=np.int64)
    fresh = np.full(n_cells, -1.0, np.float32)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        lands = v >= 0
    np.maximum.at(fresh, cells[lands], np.abs(v[lands]))
    fresh[cells[nan]] = np.nan
    return fresh


def finish(grid, fresh, decay, thresh, ring=None, window=0, steps=None):
    """rg_refresh_finish, i.e. oracle/field_ref.py::update_extra_state's tail: (grid float32, mean float64, bitfield uint8, mean_count or None).
    EMA in float32 where both sides are >= 0; mean of clamp(grid, 0) in float64; bitfield little-endian, strict `>` against min(float32(mean), thresh);
    mean_count = int(total / window) with an int64 total of column 0 of the ring rows (steps - window + i) mod 2^32 mod 16 (steps None: steps = window)."""
    grid = np.array(grid, dtype=np.float32).reshape(-1)
    fresh = np.asarray(fresh, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (grid >= 0) & (fresh >= 0)
        grid[valid] = np.maximum((grid[valid] * np.float32(decay)).astype(np.float32), fresh[valid])
        mean = float(np.maximum(grid, np.float32(0)).astype(np.float64).sum() / grid.size)
        level = min(np.float32(mean), np.float32(thresh))
    bits = np.packbits(grid > level, bitorder="little")
    mean_count = None
    if window > 0:
        steps = window if steps is None else int(steps)
        rows = [((steps - window + i) & MASK32) % 16 for i in range(window)]
        total = sum(int(np.asarray(ring)[r, 0]) for r in rows)
        mean_count = int(total / window)
    return grid, mean, bits, mean_count
