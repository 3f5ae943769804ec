"""The warm-up pass (hg_warm_tables, csrc/encode.hip) reads one table per XCD -- the finest its workgroups gather from -- and writes nothing.

The 16 base tables, the pre-summed codebook S and the sink word are bit-identical after the pass with S and without it (a clean model: another slot assignment),
and a field pass behind it gives what it gives without warming; a null sink, a null table list and a null table are refused."""
import ctypes

import numpy as np
import pytest
import torch

import closed_form as cf

pytestmark = pytest.mark.gpu

T = 1 << 19
M = 4099                         # points of the field pass: more than one workgroup, no multiple of the 32-point tile


@pytest.fixture(scope="module")
def scene():
    """Base tables, four codebook tables with their pre-sum, packed MLP weights, points and directions.  Computed once; the tests compare against clones."""
    from nerf_signature_amd import fieldops as fo
    base = [torch.from_numpy(cf.table(l)).cuda() for l in range(16)]
    cb = [torch.from_numpy(cf.table(100 + l, scale=0.05)).cuda() for l in range(4)]
    S = fo.codebook_presum([cb[1], cb[2]])
    packed = fo.pack_weights(torch.from_numpy(cf.mlp_params(3072, 1337)).cuda(), torch.from_numpy(cf.mlp_params(7168, 1338)).cuda())
    rng = np.random.RandomState(3)
    pts = torch.from_numpy((rng.rand(M, 3) * 2 - 1).astype(np.float32)).cuda()
    dirs = torch.from_numpy(cf.unit_dirs(M, seed=5)).cuda()
    torch.cuda.synchronize()
    return {"base": base, "cb": cb, "S": S, "packed": packed, "pts": pts, "dirs": dirs}


def _render(nv, sc):
    sigmas, rgbs = torch.full((M,), float("nan"), device="cuda"), torch.full((M, 3), float("nan"), device="cuda")
    nv.call("field_fwd", nv.ptr(sc["pts"]), nv.ptr(sc["dirs"]), M, 1.0, nv.ptr_array(sc["base"]), nv.ptr(sc["S"]), nv.ptr(sc["packed"]), nv.ptr(sigmas), nv.ptr(rgbs),
            None, None, None, 0, nv.stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sigmas).all()) and bool(torch.isfinite(rgbs).all())
    return sigmas, rgbs


def test_the_pass_only_reads_and_a_render_behind_it_is_unchanged(scene):
    from nerf_signature_amd import _native as nv
    snap = [t.clone() for t in scene["base"]] + [scene["S"].clone()]
    want = _render(nv, scene)
    sink = torch.zeros(1, dtype=torch.float32, device="cuda")
    tables = nv.ptr_array(scene["base"])
    for S in (scene["S"], None):      # (None: a clean model, no pre-sum)
        nv.call("hg_warm_tables", tables, nv.ptr(S), nv.ptr(sink), nv.stream())
        got = _render(nv, scene)
        assert all(torch.equal(a, b) for a, b in zip(snap, scene["base"] + [scene["S"]])) and float(sink) == 0.0, "the warm-up pass wrote"
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "the render changed"


def test_refusals(scene):
    from nerf_signature_amd import _native as nv
    sink = torch.zeros(1, dtype=torch.float32, device="cuda")
    tables = nv.ptr_array(scene["base"])

    def refused(message, *args):
        with pytest.raises(ValueError) as e:
            nv.call("hg_warm_tables", *args, nv.stream())
        assert str(e.value) == f"hg_warm_tables failed (code 1): hg_warm_tables: {message}"

    refused("sink is one writable float (never written)", tables, nv.ptr(scene["S"]), None)
    refused("null base table list", None, nv.ptr(scene["S"]), nv.ptr(sink))
    refused("base table 3 is null", (ctypes.c_void_p * 16)(*[None if l == 3 else t.data_ptr() for l, t in enumerate(scene["base"])]), nv.ptr(scene["S"]), nv.ptr(sink))
