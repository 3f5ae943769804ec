"""Hard inputs for the occupancy walk: bitfields, rays, noises and the case list that tests/test_gpu_march_edges.py runs against the C oracle
and whose premises tests/test_march_scenes_cpu.py asserts with the oracle alone.  numpy only: no torch, no GPU.

Bitfields are morton-indexed and packed little-endian, as rm_packbits writes them: bit i of byte n is cell 8 n + i, cascade c starts at bit c H^3.
"""
import collections
import functools

import numpy as np

KINDS = ("dust", "half", "blocks", "shells", "specks", "parity", "empty", "full")
N_RAYS = 261          # ragged: 65 workgroups of four waves and one wave over
N_SPECIALS = 16


def _compact3(v):
    """every third bit of v, packed (the inverse of the morton spread)"""
    v = v & 0x49249249
    v = (v | (v >> 2)) & 0xC30C30C3
    v = (v | (v >> 4)) & 0x0F00F00F
    v = (v | (v >> 8)) & 0xFF0000FF
    v = (v | (v >> 16)) & 0x0000FFFF
    return v


def morton_coords(H):
    """[H^3, 3] cell coordinates of the morton indices 0 .. H^3 - 1"""
    idx = np.arange(H ** 3, dtype=np.int64)
    return np.stack([_compact3(idx), _compact3(idx >> 1), _compact3(idx >> 2)], -1)


@functools.lru_cache(maxsize=4)
def bitfield(kind, C, H, seed):
    """uint8 [C H^3 / 8] (read-only: shared between callers)"""
    cells, rng = H ** 3, np.random.RandomState(seed)
    if kind == "dust":
        bits = rng.rand(C, cells) < 0.03
    elif kind == "half":
        bits = rng.rand(C, cells) < 0.5
    elif kind == "blocks":       # 64 consecutive morton indices are one 4^3-cell block
        bits = np.repeat(rng.rand(C, cells // 64) < 0.3, 64, axis=1)
    elif kind == "shells":       # in units of the cascade's extent: the same pattern in every cascade
        centre = (2.0 * (morton_coords(H) + 0.5) / H - 1.0)
        radius = np.sqrt((centre * centre).sum(-1))
        one = np.zeros(cells, bool)
        for r in (0.3, 0.55, 0.8):
            one |= np.abs(radius - r) <= 2.0 / H
        bits = np.broadcast_to(one, (C, cells))
    elif kind == "specks":
        bits = np.zeros(C * cells, bool)
        bits[rng.choice(C * cells, 200, replace=False)] = True
    elif kind == "parity":
        bits = np.zeros((C, cells), bool)
        bits[0::2] = True
    elif kind == "empty":
        bits = np.zeros(C * cells, bool)
    elif kind == "full":
        bits = np.ones(C * cells, bool)
    else:
        raise ValueError(kind)
    out = np.packbits(np.ascontiguousarray(bits).reshape(-1), bitorder="little")
    assert out.shape[0] == C * cells // 8
    out.setflags(write=False)
    return out


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _ball(rng, n, radius):
    """n points uniform in the ball"""
    return _unit(rng.randn(n, 3)) * (radius * rng.rand(n, 1) ** (1.0 / 3.0))


def rays(n, bound, seed):
    """float32 o, d [n, 3], unit directions: n/3 origins inside 0.6 bound, the others on the sphere of radius 2.5 bound, each aimed at a uniform target
    inside 0.8 bound; the first N_SPECIALS rows are the fixed degenerate rays below."""
    rng = np.random.RandomState(seed)
    inside = n // 3
    o = np.concatenate([_ball(rng, inside, 0.6 * bound), _unit(rng.randn(n - inside, 3)) * 2.5 * bound])
    o = o[rng.permutation(n)]
    d = _unit(_ball(rng, n, 0.8 * bound) - o)
    o, d = o.astype(np.float32), d.astype(np.float32)
    b, far = np.float32(bound), np.float32(2.5 * bound)
    u = lambda *v: _unit(v).astype(np.float32)
    s3 = np.float32(1.0 / np.sqrt(3.0))
    nz = np.float32(-0.0)
    special = [
        # the six axis-parallel rays (two infinite reciprocals each)
        ((-far, 0.31 * b, -0.17 * b), (1, 0, 0)), ((far, -0.23 * b, 0.41 * b), (-1, 0, 0)),
        ((0.13 * b, -far, 0.37 * b), (0, 1, 0)), ((-0.29 * b, far, -0.11 * b), (0, -1, 0)),
        ((0.43 * b, 0.19 * b, -far), (0, 0, 1)), ((-0.07 * b, -0.33 * b, far), (0, 0, -1)),
        # one component -0.0: with that coordinate of the origin on a cell face (0 * -inf in the exit plane) and off it
        ((0.0, -far * 0.8, -far * 0.6), (nz,) + tuple(u(0.8, 0.6))), ((0.21 * b, 0.37 * b, far), (np.float32(0.6), nz, np.float32(-0.8))),
        # one component +0.0, likewise
        ((-far * 0.6, 0.0, far * 0.8), (np.float32(0.6), np.float32(0.0), np.float32(-0.8))), ((far * 0.8, far * 0.6, -0.37 * b), (np.float32(-0.8), np.float32(-0.6), np.float32(0.0))),
        # the diagonal through the origin: through cell corners at every H
        ((-far * s3, -far * s3, -far * s3), (s3, s3, s3)),
        # along +x in the planes y = 0 and z = 0: on cell faces at every H
        ((-far, 0.0, 0.0), (1, 0, 0)),
        # grazing the box face y = bound, and one float inside it
        ((-far, b, 0.1 * b), (1, 0, 0)), ((-far, np.nextafter(b, np.float32(0)), 0.1 * b), (1, 0, 0)),
        # misses the box
        ((3 * b, 3 * b, 3 * b), tuple(u(1, 0.2, 0.1))),
        # starts on a box face, pointing outward
        ((b, 0.1 * b, 0.2 * b), tuple(u(1, 0.3, 0.2))),
    ]
    assert len(special) == N_SPECIALS <= n
    for i, (so, sd) in enumerate(special):
        o[i], d[i] = np.array(so, np.float32), np.array(sd, np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def noises(n, seed):
    """uniform [0, 1); entry 0 is 0, entry 1 the largest float below 1"""
    v = np.random.RandomState(seed).rand(n).astype(np.float32)
    v = np.minimum(v, np.nextafter(np.float32(1), np.float32(0)))
    v[0], v[1] = 0.0, np.nextafter(np.float32(1), np.float32(0))
    return v


def dt_min_of(max_steps):
    """raymarching.cu:345 in fp32: fl(fl(2 fl(sqrt 3)) / max_steps)"""
    return np.float32(np.float32(2.0) * np.float32(1.7320508075688772)) / np.float32(max_steps)


def ties_in(max_steps, e):
    """frac(dt / 2^(e-23)) == 1/2 with the chunk's other preconditions: dt / ulp < 2^17, 64 dt <= 2^e (all exact in float64)"""
    q = float(dt_min_of(max_steps)) / 2.0 ** (e - 23)
    return q - np.floor(q) == 0.5 and q < 131072.0 and 64.0 * float(dt_min_of(max_steps)) <= 2.0 ** e


def tie_max_steps(lo_exp, hi_exp, limit=4096):
    """Smallest max_steps <= limit whose constant step ties (see ties_in) in a binade [2^e, 2^(e+1)), lo_exp <= e <= hi_exp: (max_steps, e)."""
    for max_steps in range(1, limit + 1):
        for e in range(lo_exp, hi_exp + 1):
            if ties_in(max_steps, e):
                return max_steps, e
    raise ValueError(f"no max_steps <= {limit} ties in binades {lo_exp} .. {hi_exp}")


# ------------------------------------------------------------------------------------------------------------------------ the case list
# claims: "alt" (a quarter of the rays have >= 8 gaps), "cap" (a ray with count == max_steps and one with 0 < count < max_steps), "capped" (a ray
# with count == max_steps; max_steps = 1 leaves no room for the other half of "cap"), "zero" (rays without samples), "tie" (a sampled ray overlaps
# the tie binade), "t0" (a sampled ray starts below 0.25), "lastcell" (C H^3 > 2^24 and a ray samples in the
# last cell of the last cascade, whose float bit index rounds up to C H^3, one past the bitfield: raymarching.cu:339,378), "twob" (a ray samples behind the second binade boundary of its first 64 steps: the closed-form
# chunk handles one boundary and must be refused there: `64 dt > t0`, which `dt / ulp(t0) >= 2^17` says as well).

Case = collections.namedtuple("Case", "name bound C H kind dt_gamma max_steps noise min_near seed claims tie_exp half_capacity")

TIE_1 = tie_max_steps(1, 1)       # rays of the bound-1 scenes run over [1.5, 3.5]
TIE_2 = tie_max_steps(2, 2)       # those of bound 2 over [3, 7]
_MULTI = ((2.0, 2), (1.5, 2), (4.0, 3), (16.0, 5))


def _alternates(kind, C, H, dt_gamma, max_steps):
    """Where a case claims alternation.  Eight gaps need nine separate runs of occupied steps on a ray, so the claim is made only where the scene can
    hold them: a constant step (a growing one merges runs), at least 64 samples, and enough independent cells on a ray's way -- a ray crosses about
    2 H cells of a cascade, so `half` needs H >= 32, `blocks` (H / 4 blocks a side, 30 % set) H >= 128, and 3 % `dust` H = 256 (or 128 with three
    cascades to cross) and the full 1024 samples.  `shells` is never claimed: a ray meets each of a cascade's three shells at most twice, six runs."""
    if dt_gamma != 0 or max_steps < 64:
        return False
    if kind == "half":
        return H >= 32
    if kind == "blocks":
        return H >= 128
    if kind == "dust":
        return max_steps >= 1024 and (H >= 256 or (H >= 128 and C >= 3))
    return False


def _case(bound, C, H, kind, dt_gamma, max_steps, noise, min_near, seed, tie_exp=None, cap=False, half_capacity=False, twob=False):
    claims = {"zero"}          # every ray set holds a ray that misses the box and one that starts on a face, pointing outward
    if _alternates(kind, C, H, dt_gamma, max_steps):
        claims.add("alt")
    if cap:
        claims.add("cap" if max_steps > 1 else "capped")
    if tie_exp is not None:
        claims.add("tie")
    if twob:
        claims.add("twob")
    if C * H ** 3 > 2 ** 24 and kind in ("full", "half", "blocks", "dust"):      # the diagonal ray leaves the box through its last cell
        claims.add("lastcell")
    if kind in ("half", "full", "blocks") and max_steps >= 64:      # origins inside the box start at min_near < 0.25
        claims.add("t0")
    g = {0.0: "0", 1 / 128: "128", 1 / 256: "256"}[dt_gamma]
    name = f"b{bound:g}-C{C}-H{H}-{kind}-g{g}-s{max_steps}-{'n' if noise else 'p'}-m{min_near:g}"
    return Case(name, float(bound), C, H, kind, float(dt_gamma), int(max_steps), bool(noise), float(min_near), seed, frozenset(claims), tie_exp, half_capacity)


def _build_cases():
    out, seed = [], 0
    hs = (8, 32, 128, 256)
    # (1) every instantiation (kOneCascade x kConstDt) meets every scene kind; H, bound, noise and min_near rotate
    for ki, kind in enumerate(KINDS):
        for inst in range(4):
            one, const = inst & 1, inst >> 1
            j = ki * 4 + inst
            bound, C = (1.0, 1) if one else _MULTI[(ki + inst // 2) % 4]
            H = hs[(ki + inst) % 4]
            if H == 256 and C > 2:
                H = 128          # keep the bitfield small
            dt_gamma = 0.0 if const else (1 / 128, 1 / 256)[ki % 2]
            out.append(_case(bound, C, H, kind, dt_gamma, 1024, j % 3 == 0, (0.05, 0.2)[j % 2], seed, half_capacity=(kind in ("half", "blocks", "shells") and inst == 2)))
            seed += 1
    # (2) every H with both cascade settings, constant step, on the gappy kinds
    for hi, H in enumerate(hs):
        for one in (True, False):
            bound, C = (1.0, 1) if one else ((2.0, 2), (1.5, 2), (4.0, 3), (2.0, 2))[hi]
            for kind in ("dust", "half", "blocks"):
                out.append(_case(bound, C, H, kind, 0.0, 1024, kind == "half", 0.05, seed, half_capacity=(kind == "dust" and H == 128)))
                seed += 1
    # (3) the tie: dt_min ties in [2, 4) (bound 1) and in [4, 8) (bound 2); chunks that start one binade lower meet the tie behind the boundary
    for H in (32, 128, 256):
        for kind, noise in (("dust", False), ("half", True), (("shells", "blocks")[H == 256], False)):
            out.append(_case(1.0, 1, H, kind, 0.0, TIE_1[0], noise, 0.05, seed, tie_exp=TIE_1[1]))
            seed += 1
    for H, kind, noise in ((128, "dust", False), (256, "half", False), (128, "blocks", True), (32, "full", False)):
        out.append(_case(2.0, 2, H, kind, 0.0, TIE_2[0], noise, 0.2, seed, tie_exp=TIE_2[1]))
        seed += 1
    # (4) the sample cap inside and at the end of a chunk: max_steps 64, 65, 7, 1 for all four instantiations.  The step is min(dt_min, dt_max) with
    # dt_max = 2 sqrt(3) 2^(C-1) / H, so H and the scene are chosen for chords that hold both more and fewer occupied steps than max_steps
    #            bound C    H  kind      dt_gamma  noise
    capped = {64: ((1.0, 1, 256, "half", 0.0, False), (1.0, 1, 256, "half", 1 / 128, True), (4.0, 3, 32, "half", 0.0, False), (2.0, 2, 128, "full", 1 / 128, True)),
              65: ((1.0, 1, 128, "full", 0.0, False), (1.0, 1, 256, "half", 1 / 256, True), (16.0, 5, 32, "blocks", 0.0, False), (1.5, 2, 128, "full", 1 / 128, False)),
              7: ((1.0, 1, 32, "half", 0.0, False), (1.0, 1, 32, "half", 1 / 128, True), (1.5, 2, 8, "blocks", 0.0, False), (16.0, 5, 8, "blocks", 1 / 128, False)),
              1: ((1.0, 1, 8, "half", 0.0, False), (1.0, 1, 8, "half", 1 / 128, True), (16.0, 5, 8, "blocks", 0.0, False), (1.5, 2, 8, "blocks", 1 / 128, False))}
    for max_steps, rows in capped.items():
        for k, (bound, C, H, kind, dt_gamma, noise) in enumerate(rows):
            out.append(_case(bound, C, H, kind, dt_gamma, max_steps, noise, 0.05, seed, cap=True, half_capacity=(max_steps == 65 and k == 2)))
            seed += 1
    out.append(_case(1.0, 1, 128, "full", 0.0, 1024, False, 0.2, seed, cap=True))
    seed += 1
    # the last cell of the last cascade occupied for certain, where the float bit index is one past the bitfield
    # (a growing step, so that the diagonal ray reaches the far corner within 1024 samples)
    out.append(_case(2.0, 2, 256, "full", 1 / 128, 1024, False, 0.2, seed))
    seed += 1
    # a step of 2 sqrt(3) / 64 from near ~ 1.6: 63 steps reach t = 5, across the binade boundaries 2 and 4
    out.append(_case(1.0, 1, 32, "half", 0.0, 64, False, 0.05, seed, twob=True))
    out.append(_case(1.0, 1, 32, "half", 0.0, 65, True, 0.2, seed + 1, twob=True))
    seed += 2
    # (5) the wide scenes with a growing step, and cascade choice under both dt_gamma
    for bound, C in ((4.0, 3), (16.0, 5)):
        for dt_gamma in (1 / 128, 1 / 256):
            for kind in ("parity", "shells", "half"):
                out.append(_case(bound, C, (32, 128)[kind != "half"], kind, dt_gamma, 1024, kind == "shells", 0.2, seed))
                seed += 1
    seen, unique = set(), []
    for c in out:           # the sections overlap in a few places: keep the first of two cases with the same parameters
        if c.name not in seen:
            seen.add(c.name)
            unique.append(c)
    return tuple(unique)


CASES = _build_cases()
# the eval burst runs on a cross-section (tests/test_march_scenes_cpu.py: every H, both cascade settings, both step rules, a tie and a cap case)
EVAL_CASES = tuple(CASES[i] for i in range(0, len(CASES), 7))


def inputs(case):
    """(bitfield, o, d, noises or None, aabb) of a case"""
    aabb = np.array([-case.bound] * 3 + [case.bound] * 3, np.float32)
    if case.kind == "slab":
        return (slab_bitfield(case.H),) + border_rays(case)[:3] + (aabb,)
    o, d = rays(N_RAYS, case.bound, 1000 + case.seed)
    return bitfield(case.kind, case.C, case.H, case.seed), o, d, (noises(N_RAYS, 2000 + case.seed) if case.noise else None), aabb


def gaps_per_ray(deltas, rays_table):
    """number of samples after a ray's first whose deltas[:, 1] exceeds deltas[:, 0] by more than half a step"""
    out = np.zeros(rays_table.shape[0], np.int64)
    for i, off, cnt in rays_table:
        if cnt > 1:
            dl = deltas[off + 1:off + cnt].astype(np.float64)
            out[i] = int((dl[:, 1] - dl[:, 0] > 0.5 * dl[:, 0]).sum())
    return out


def rays_behind_two_boundaries(case, ref):
    """Rays whose first chunk cannot be the closed form (near >= 0.25 but near < 64 dt) and that take a sample behind the second binade boundary above
    near within their first 63 steps.  Sample parameters are rebuilt from the oracle's deltas (float64 sums: a margin of one step stands in for the rounding)."""
    dt = float(dt_min_of(case.max_steps))
    assert case.dt_gamma == 0 and dt <= 2 * np.sqrt(3.0) * 2 ** (case.C - 1) / case.H
    out = []
    for i, off, cnt in ref.rays:
        near = float(ref.nears[i])
        if cnt == 0 or not 0.25 <= near < 64 * dt:
            continue
        second = 4.0 * 2.0 ** np.floor(np.log2(near))
        t = near + np.cumsum(ref.deltas[off:off + cnt, 1].astype(np.float64)) - dt        # where each sample was taken
        if ((t > second + dt) & (t < near + 62 * dt)).any():
            out.append(int(i))
    return out


def samples_in_last_cell(case, ref):
    """samples inside the cell (H-1, H-1, H-1) of the last cascade (its extent is min(2^(C-1), bound))"""
    extent = min(2.0 ** (case.C - 1), case.bound)
    live = ref.deltas[:, 0] > 0
    return int((live & (ref.xyzs.min(-1) >= extent * (1.0 - 2.0 / case.H)) & (ref.xyzs.max(-1) > extent / 2)).sum())


def octant_counts(d):
    """rays per direction-sign octant (a zero of either sign counts by its sign bit)"""
    code = (np.signbit(d[:, 0]).astype(int) << 2) | (np.signbit(d[:, 1]).astype(int) << 1) | np.signbit(d[:, 2]).astype(int)
    return np.bincount(code, minlength=8)


# ---- a step that lands exactly on a cell's exit, at the first index of a chunk
# The walk leaves an empty cell at the first parameter of its step sequence that is >= the cell's exit; the kernel carries that exit from one
# 64-step chunk to the next.  Equality is rare on random rays, so these rays are built for it: along +x from inside the box (near = min_near), the
# half space x >= 0.5 occupied and the rest empty, and the origin placed so that step 64 j of the sequence, T, gives x = 0.5 exactly.  Every
# quantity on the way is exact in fp32 (ox = 0.5 - T, t + ox inside the last empty cell, the exit t + (0.5 - x) = T), so the oracle's first sample
# is at x == 0.5; a walk that asks for > instead of >= at the chunk border loses it.

BORDER_X = 0.5


@functools.lru_cache(maxsize=1)
def slab_bitfield(H):
    out = np.packbits(morton_coords(H)[:, 0] >= H * (1 + BORDER_X) / 2, bitorder="little")
    out.setflags(write=False)
    return out


def border_chain(case, noise, steps):
    """step `steps` of the sequence t <- fl(t + dt) from t0 = fma(dt, noise, min_near), in fp32 (noise is dyadic: the product is exact in float64)"""
    dt = dt_min_of(case.max_steps)
    t = np.float32(np.float64(dt) * np.float64(noise) + np.float64(np.float32(case.min_near)))
    for _ in range(steps):
        t = np.float32(t + dt)
    return t


def border_rays(case):
    """(o, d, noises, chunk index j of each ray)"""
    rng = np.random.RandomState(case.seed)
    o, nz, js = [], [], []
    for j in (1, 2, 3, 4):
        for noise in (0.0, 0.25, 0.5, 0.75):
            for _ in range(4):
                T = border_chain(case, noise, 64 * j)
                ox = np.float32(BORDER_X - np.float64(T))
                assert np.float64(ox) == BORDER_X - np.float64(T)
                o.append((ox, np.float32(rng.uniform(-0.6, 0.6)), np.float32(rng.uniform(-0.6, 0.6))))
                nz.append(noise)
                js.append(j)
    o = np.array(o, np.float32)
    d = np.tile(np.array([1, 0, 0], np.float32), (o.shape[0], 1))
    return o, d, np.array(nz, np.float32), np.array(js)


BORDER = _case(1.0, 1, 32, "slab", 0.0, 1024, True, 0.2, 77)


Reference = collections.namedtuple("Reference", "nears fars xyzs dirs deltas rays counter")


@functools.lru_cache(maxsize=2)
def reference(case):
    """The C oracle's training march of a case, all rays kept, rows padded to the next multiple of 128 (computed once, shared, read-only)."""
    from oracle import raymarch_ref as orm
    bits, o, d, nz, aabb = inputs(case)
    with np.errstate(divide="ignore", invalid="ignore"):
        nears, fars = orm.near_far_from_aabb(o, d, aabb, case.min_near)
    counter = np.zeros(2, np.int32)
    x, dd, dl, table = orm.march_rays_train(o, d, case.bound, bits, case.C, case.H, nears, fars, counter, -1, case.noise, 128, True, case.dt_gamma,
                                            case.max_steps, noises=nz)
    out = Reference(nears, fars, np.ascontiguousarray(x), np.ascontiguousarray(dd), np.ascontiguousarray(dl), table, counter)
    for a in out:
        a.setflags(write=False)
    return out
