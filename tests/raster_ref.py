"""Host restatement of the mesh rasteriser, written from the text of include/nerfsig.h ("mesh rasteriser"), not from csrc/raster.hip.

    project(vertices, pose, intrinsics, near)          -> records int32 [V, 4]: x, y, the bits of iz, flag -- fp32, one numpy operation per rounding
    render(vertices, triangles, colors, pose, intrinsics, H, W, bg, near)   -> dict: records, image, depth, triangle, culled, bad, coverage

Coverage is decided on int64 edge functions at every pixel centre of the image for every triangle (no bounding box, no routes: a brute-force loop over the
triangles, numpy over the pixels), depth and colour in float64 in the header's association, the winner as a lexicographic minimum of (depth bits, index).
Meant for images up to 64 x 48 and a few thousand triangles.

The keyword mutants exist for tests/test_raster_cpu.py to show that each is caught: fill_rule=False (a centre on ANY edge is covered), tie="high" (equal depths
go to the higher index), affine=True (screen-affine colours), snap="trunc" (truncation instead of round-half-even)."""
import numpy as np

GUARD = np.float32(16384.0)
F = np.float32


def project(vertices, pose, intrinsics, near, snap="rint"):
    p = np.asarray(vertices, np.float32).reshape(-1, 3)
    P = np.asarray(pose, np.float32).reshape(4, 4)
    fx, fy, cx, cy = (F(v) for v in intrinsics)
    R, t = P[:3, :3], P[:3, 3]
    with np.errstate(all="ignore"):
        d = [p[:, k] - t[k] for k in range(3)]
        cam = [(R[0, c] * d[0] + R[1, c] * d[1]) + R[2, c] * d[2] for c in range(3)]
        Xc, Yc, Zc = cam
        u = fx * (Xc / Zc) + cx
        v = fy * (Yc / Zc) + cy
        iz = F(1.0) / Zc
        behind = ~(Zc >= F(near))
        outside = ~(np.abs(u) <= GUARD) | ~(np.abs(v) <= GUARD)
        flag = np.where(behind, 1, np.where(outside, 2, 0)).astype(np.int32)
        ok = flag == 0
        rnd = np.rint if snap == "rint" else np.trunc
        x = np.where(ok, rnd(np.where(ok, u, 0) * F(256.0)), 0).astype(np.int32)
        y = np.where(ok, rnd(np.where(ok, v, 0) * F(256.0)), 0).astype(np.int32)
        iz = np.where(ok, iz, F(0.0)).astype(np.float32)
    return np.stack([x, y, iz.view(np.int32), flag], axis=1)


def _owns(px, py, qx, qy):
    """The top-left rule for the directed edge p -> q of a triangle with A2 > 0."""
    dx, dy = qx - px, qy - py
    return dy < 0 or (dy == 0 and dx > 0)


def render(vertices, triangles, colors, pose, intrinsics, H, W, bg=1.0, near=0.05, fill_rule=True, tie="low", affine=False, snap="rint"):
    rec = project(vertices, pose, intrinsics, near, snap)
    V = rec.shape[0]
    tris = np.asarray(triangles, np.int64).reshape(-1, 3)[:None if V else 0]      # V = 0: rs_raster launches nothing, no triangle is looked at
    col = np.asarray(colors, np.float32).reshape(-1, 3).astype(np.float64)
    izf = rec[:, 2].copy().view(np.float32).astype(np.float64)
    X = (256 * np.arange(W, dtype=np.int64) + 128)[None, :].repeat(H, 0)
    Y = (256 * np.arange(H, dtype=np.int64) + 128)[:, None].repeat(W, 1)
    bits = np.full((H, W), 0xFFFFFFFF, np.int64)        # depth bits of the winner so far (above every float's)
    win = np.full((H, W), -1, np.int64)
    image = np.empty((H, W, 3), np.float32)
    image[:] = np.broadcast_to(np.asarray(bg, np.float32).reshape(-1), (3,))
    depth = np.full((H, W), np.inf, np.float32)
    coverage = np.zeros((H, W), np.int64)
    bad, n_near, n_guard = None, 0, 0
    for t, (a, b, c) in enumerate(tris.tolist()):
        if not (0 <= a < V and 0 <= b < V and 0 <= c < V):
            bad = t if bad is None else bad
            continue
        flags = (int(rec[a, 3]), int(rec[b, 3]), int(rec[c, 3]))
        if 1 in flags:
            n_near += 1
            continue
        if 2 in flags:
            n_guard += 1
            continue
        (xa, ya), (xb, yb), (xc, yc) = ((int(rec[k, 0]), int(rec[k, 1])) for k in (a, b, c))
        A2 = (xb - xa) * (yc - ya) - (yb - ya) * (xc - xa)
        if A2 == 0:
            continue
        if A2 < 0:
            b, c, xb, yb, xc, yc, A2 = c, b, xc, yc, xb, yb, -A2
        inside = np.ones((H, W), bool)
        E = []
        for (px, py, qx, qy) in ((xb, yb, xc, yc), (xc, yc, xa, ya), (xa, ya, xb, yb)):       # E_a, E_b, E_c
            e = (qx - px) * (Y - py) - (qy - py) * (X - px)
            inside &= (e > 0) | ((e == 0) if (not fill_rule or _owns(px, py, qx, qy)) else False)
            E.append(e)
        if not inside.any():
            continue
        coverage += inside
        bk = [e.astype(np.float64) / np.float64(A2) for e in E]
        iza, izb, izc = izf[a], izf[b], izf[c]
        with np.errstate(all="ignore"):
            q = (bk[0] * iza + bk[1] * izb) + bk[2] * izc
            z = (1.0 / q).astype(np.float32)
        zb = z.view(np.uint32).astype(np.int64)
        better = inside & ((zb < bits) | ((zb == bits) & ((t < win) if tie == "low" else (t > win)) & (win >= 0)))
        if not better.any():
            continue
        if affine:
            w = bk
            den = (bk[0] + bk[1]) + bk[2]
        else:
            w = [bk[0] * iza, bk[1] * izb, bk[2] * izc]
            den = q
        with np.errstate(all="ignore"):
            for ch in range(3):
                n = (w[0] * col[a, ch] + w[1] * col[b, ch]) + w[2] * col[c, ch]
                image[..., ch][better] = (n / den).astype(np.float32)[better]
        depth[better] = z[better]
        bits[better] = zb[better]
        win[better] = t
    return {"records": rec, "image": image, "depth": depth, "triangle": win.astype(np.int32), "culled": (n_near, n_guard), "bad": bad, "coverage": coverage}
