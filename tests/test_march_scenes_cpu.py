"""The premises of tests/test_gpu_march_edges.py, asserted with the C oracle alone: that the hard inputs its cases name are really in them.  Every
figure below comes from the inputs and from oracle/raymarch_ref.c, none from the kernels, so a green GPU run means the walk was compared on rays of all
eight sign octants, on alternating occupancy, at the sample cap, on the tie of the closed-form chunk and below t = 0.25 -- not on an easy scene."""
import numpy as np
import pytest

import march_scenes as ms

_IDS = [c.name for c in ms.CASES]


def test_generators_are_what_they_say():
    for C, H in ((1, 8), (2, 32)):
        cells = H ** 3
        unpack = lambda kind: np.unpackbits(ms.bitfield(kind, C, H, 5), bitorder="little").reshape(C, cells)
        assert ms.bitfield("dust", C, H, 5).shape == (C * cells // 8,) and ms.bitfield("dust", C, H, 5).dtype == np.uint8
        assert abs(unpack("dust").mean() - 0.03) < 0.01 and abs(unpack("half").mean() - 0.5) < 0.02
        blocks = unpack("blocks").reshape(C, cells // 64, 64)
        assert ((blocks.min(-1) == blocks.max(-1)).all()) and 0.2 < blocks.mean() < 0.4
        assert unpack("specks").sum() == 200 and unpack("empty").sum() == 0 and unpack("full").all()
        assert unpack("parity")[0::2].all() and not unpack("parity")[1::2].any()
        shells = unpack("shells")
        centre = 2.0 * (ms.morton_coords(H) + 0.5) / H - 1.0
        r = np.sqrt((centre ** 2).sum(-1))
        assert shells[0].any() and (np.abs(r[shells[0] == 1][:, None] - np.array([0.3, 0.55, 0.8])).min(-1) <= 2.0 / H).all()
    # morton order: cell (1, 0, 0) is index 1, (0, 1, 0) index 2, (0, 0, 1) index 4, as rm_morton3D and the oracle have it
    from oracle import raymarch_ref as orm
    np.testing.assert_array_equal(orm.morton3D(ms.morton_coords(8).astype(np.int32)), np.arange(512))
    o, d = ms.rays(ms.N_RAYS, 2.0, 3)
    assert o.dtype == d.dtype == np.float32 and o.shape == d.shape == (ms.N_RAYS, 3)
    np.testing.assert_allclose(np.sqrt((d.astype(np.float64) ** 2).sum(-1)), 1.0, atol=1e-6)
    r = np.sqrt((o[ms.N_SPECIALS:].astype(np.float64) ** 2).sum(-1))
    assert ((r <= 0.6 * 2.0 + 1e-6) | (np.abs(r - 5.0) < 1e-5)).all() and 60 < (r <= 1.2 + 1e-6).sum() <= ms.N_RAYS // 3
    assert (np.abs(d[:6]).max(-1) == 1).all() and (np.abs(d[:6]).sum(-1) == 1).all()                 # the six axis-parallel rays
    assert [int(np.signbit(d[i][d[i] == 0]).sum()) for i in (6, 7, 8, 9)] == [1, 1, 0, 0]           # -0.0, -0.0, +0.0, +0.0
    assert o[12, 1] == 2.0 and o[13, 1] == np.nextafter(np.float32(2), np.float32(0))
    z = ms.noises(ms.N_RAYS, 1)
    assert z[0] == 0 and z[1] == np.nextafter(np.float32(1), np.float32(0)) and (z >= 0).all() and (z < 1).all() and z.dtype == np.float32


def test_tie_search_finds_the_known_values():
    """the step 2 sqrt(3) / max_steps ties in [2, 4) for 514, in [1, 2) for 1028, in [4, 8) for 257 and 771, in [0.5, 1) for 653 -- and nowhere for 1024"""
    assert ms.tie_max_steps(1, 1) == (514, 1) and ms.tie_max_steps(2, 2) == (257, 2)
    assert ms.ties_in(1028, 0) and ms.ties_in(771, 2) and ms.ties_in(653, -1)
    assert not any(ms.ties_in(1024, e) for e in range(-2, 4))
    assert ms.TIE_1 == (514, 1) and ms.TIE_2 == (257, 2)
    found = sum(any(ms.ties_in(m, e) for e in range(-2, 4)) for m in range(1, 4097))
    assert found == 38


def test_case_list_covers_the_walk():
    """every template instantiation meets every scene kind, every H both cascade settings, and the list holds every parameter value of the grid"""
    seen = {(c.C == 1, c.dt_gamma == 0, c.kind) for c in ms.CASES}
    assert seen >= {(one, const, kind) for one in (True, False) for const in (True, False) for kind in ms.KINDS}
    assert {(c.H, c.C == 1) for c in ms.CASES} >= {(H, one) for H in (8, 32, 128, 256) for one in (True, False)}
    assert {(c.bound, c.C) for c in ms.CASES} == {(1.0, 1), (2.0, 2), (1.5, 2), (4.0, 3), (16.0, 5)}
    assert {c.dt_gamma for c in ms.CASES} == {0.0, 1 / 128, 1 / 256} and {c.min_near for c in ms.CASES} == {0.05, 0.2}
    assert {c.max_steps for c in ms.CASES} == {1024, ms.TIE_1[0], ms.TIE_2[0], 64, 65, 7, 1} and {c.noise for c in ms.CASES} == {True, False}
    assert any("lastcell" in c.claims and c.kind == "full" for c in ms.CASES)
    assert 90 <= len(ms.CASES) <= 110 and 4 <= sum(c.half_capacity for c in ms.CASES) <= 8
    for claim in ("alt", "cap", "capped", "zero", "tie", "t0", "twob", "lastcell"):
        assert any(claim in c.claims for c in ms.CASES), claim
    assert any({"alt", "tie"} <= c.claims for c in ms.CASES) and any({"alt", "cap"} <= c.claims for c in ms.CASES)
    # alternation is claimed wherever the rule written at march_scenes._alternates allows it, and at 64 samples only with `half` or `blocks`
    assert all(c.kind in ("half", "blocks") for c in ms.CASES if "alt" in c.claims and c.max_steps < 1024)
    # the eval cross-section: both cascade settings, both step rules, a tie and a cap
    ev = ms.EVAL_CASES
    assert {c.C == 1 for c in ev} == {True, False} and {c.dt_gamma == 0 for c in ev} == {True, False}
    assert any("tie" in c.claims for c in ev) and any("cap" in c.claims for c in ev) and any("alt" in c.claims for c in ev)
    assert len({c.H for c in ev}) == 4 and set(ev) <= set(ms.CASES)


def test_border_rays_step_exactly_onto_a_cell_exit_at_a_chunk_start():
    """ms.BORDER: step 64 j of every ray's sequence is the exit of its last empty cell and the oracle's first sample, at x == 0.5 exactly."""
    case = ms.BORDER
    bits, o, d, nz, _ = ms.inputs(case)
    js = ms.border_rays(case)[3]
    ref = ms.reference(case)
    dt = ms.dt_min_of(case.max_steps)
    assert float(dt) < 2 * np.sqrt(3.0) / case.H and o.shape[0] == 64 and not np.isnan(ref.xyzs).any()
    assert (ref.nears == np.float32(case.min_near)).all() and (ref.rays[:, 2] > 0).all()
    for i, off, cnt in ref.rays:
        T = ms.border_chain(case, nz[i], 64 * js[i])
        before = ms.border_chain(case, nz[i], 64 * js[i] - 1)
        assert np.float32(T + o[i, 0]) == ms.BORDER_X and np.float32(before + o[i, 0]) < ms.BORDER_X      # index 64 j is the first one at the exit
        x_cell = np.float32(before + o[i, 0])                                                      # the exit seen from the index before: exactly T
        assert np.float32(before + np.float32(ms.BORDER_X - x_cell)) == T
        assert ref.xyzs[off, 0] == ms.BORDER_X and ref.deltas[off, 0] == dt                        # the oracle samples there
        assert cnt == int(ref.rays[i, 2]) and abs(cnt - (1.0 - ms.BORDER_X) / float(dt)) <= 1.5      # and walks the occupied half to the box face


@pytest.mark.parametrize("case", ms.CASES, ids=_IDS)
def test_case_premises_hold_in_the_oracle(case):
    _, o, d, _, _ = ms.inputs(case)
    ref = ms.reference(case)
    n = ms.N_RAYS
    octants = ms.octant_counts(d)
    assert octants.min() >= n / 16, octants
    for a in (ref.xyzs, ref.dirs, ref.deltas):
        assert not np.isnan(a).any()
    cnt = ref.rays[:, 2]
    sampled = cnt > 0
    assert int(cnt.sum()) == int(ref.counter[0]) and int(ref.counter[1]) == n and cnt.max(initial=0) <= case.max_steps
    figures = [f"octants {octants.tolist()}"]
    if "alt" in case.claims:
        gappy = int((ms.gaps_per_ray(ref.deltas, ref.rays) >= 8).sum())
        figures.append(f"{gappy} rays with >= 8 gaps")
        assert gappy >= n / 4
    if "cap" in case.claims or "capped" in case.claims:
        capped, partial = int((cnt == case.max_steps).sum()), int((sampled & (cnt < case.max_steps)).sum())
        figures.append(f"{capped} capped rays, {partial} below the cap")
        assert capped >= 1 and (partial >= 1 or "cap" not in case.claims)
    if "zero" in case.claims:
        assert (~sampled).any()
    if "tie" in case.claims:
        e = case.tie_exp
        assert ms.ties_in(case.max_steps, e)
        # the tie is in the step the walk really takes: dt_min, not dt_max
        assert float(ms.dt_min_of(case.max_steps)) <= 2 * np.sqrt(3.0) * 2 ** (case.C - 1) / case.H and case.dt_gamma == 0
        inside = sampled & (ref.nears < 2.0 ** (e + 1)) & (ref.fars > 2.0 ** e)
        crossing = sampled & (ref.nears < 2.0 ** e) & (ref.fars > 2.0 ** e)          # chunks that enter the tie binade: the tie behind the boundary
        figures.append(f"{int(inside.sum())} sampled rays in the tie binade, {int(crossing.sum())} entering it")
        assert inside.any() and crossing.any()
    if "lastcell" in case.claims:
        last = ms.samples_in_last_cell(case, ref)
        figures.append(f"{last} samples in the last cell of the last cascade")
        assert case.C * case.H ** 3 > 2 ** 24 and (last >= 1 or case.kind != "full")      # the scene decides whether the cell is occupied; `full` says yes
    if "twob" in case.claims:
        two = ms.rays_behind_two_boundaries(case, ref)
        figures.append(f"{len(two)} rays sample behind a second binade boundary inside their first chunk")
        assert len(two) >= 1
    if "t0" in case.claims:
        low = int((sampled & (ref.nears < 0.25)).sum())
        figures.append(f"{low} sampled rays with near < 0.25")
        assert low >= 1
    print(f"\n{case.name}: " + "; ".join(figures))
