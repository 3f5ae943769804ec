"""The multi-message entry points without a GPU: every refusal returns before a launch with its message, the byte-size queries, and the host helper that deals
K messages to launches of at most NSIG_MULTI_MAX_MESSAGES."""
import re

import pytest

MIB = 1 << 20


@pytest.fixture(scope="module")
def native():
    from nerf_signature_amd import build, _native
    build.build()
    return _native


def _refused(native, text, name, *args):
    with pytest.raises(ValueError, match=re.escape(text)):
        native.call(name, *args)


def test_presum_multi_refusals(native):
    d, odd = native._vp(256), native._vp(264)
    tabs = (native._vp * 128)(*([256] * 128))
    name = "hg_codebook_presum_multi"
    for args in ((None, d, 2, 32, d, None), (tabs, None, 2, 32, d, None), (tabs, d, 2, 32, None, None)):
        _refused(native, "hg_codebook_presum_multi: null pointer", name, *args)
    _refused(native, "hg_codebook_presum_multi: K=0 out of range [1,16]", name, tabs, d, 0, 32, d, None)
    _refused(native, "hg_codebook_presum_multi: K=17 out of range [1,16]", name, tabs, d, 17, 32, d, None)
    _refused(native, "hg_codebook_presum_multi: D=0 out of range [1,64]", name, tabs, d, 2, 0, d, None)
    _refused(native, "hg_codebook_presum_multi: D=65 out of range [1,64]", name, tabs, d, 2, 65, d, None)
    _refused(native, "hg_codebook_presum_multi: S_multi must be 16-byte aligned", name, tabs, d, 2, 32, odd, None)
    bad = (native._vp * 128)(*([256] * 5 + [264] + [256] * 122))
    _refused(native, "hg_codebook_presum_multi: table 5 is null or not 16-byte aligned", name, bad, d, 2, 32, d, None)
    hole = (native._vp * 128)(*([256] * 63 + [None] + [256] * 64))
    _refused(native, "hg_codebook_presum_multi: table 63 is null or not 16-byte aligned", name, hole, d, 2, 32, d, None)


def test_codebook_planes_multi_refusals(native):
    d = native._vp(256)
    name = "hg_encode_codebook_planes_multi"
    for args in ((None, 64, 1.0, d, 2, d, None), (d, 64, 1.0, None, 2, d, None), (d, 64, 1.0, d, 2, None, None)):
        _refused(native, "hg_encode_codebook_planes_multi: null pointer", name, *args)
    _refused(native, "hg_encode_codebook_planes_multi: K=0 out of range [1,16]", name, d, 64, 1.0, d, 0, d, None)
    _refused(native, "hg_encode_codebook_planes_multi: K=17 out of range [1,16]", name, d, 64, 1.0, d, 17, d, None)
    _refused(native, "hg_encode_codebook_planes_multi: bound must be positive", name, d, 64, 0.0, d, 2, d, None)
    _refused(native, "hg_encode_codebook_planes_multi: bound must be positive", name, d, 64, -1.0, d, 2, d, None)
    _refused(native, "hg_encode_codebook_planes_multi: S_multi must be 16-byte aligned", name, d, 64, 1.0, native._vp(264), 2, d, None)
    _refused(native, "hg_encode_codebook_planes_multi: cplanes must be 8-byte aligned", name, d, 64, 1.0, d, 2, native._vp(260), None)
    _refused(native, "hg_encode_codebook_planes_multi: M=134217729 too large", name, d, (1 << 27) + 1, 1.0, d, 2, d, None)


def test_field_fwd_multi_refusals(native):
    d = native._vp(256)
    name = "field_fwd_multi"
    ok = [d, 64, d, d, 0, d, 2, d, d, None]      # dirs, M, packed, planes, layout, cplanes, K, sigmas, rgbs, stream
    for i in (0, 2, 3, 5, 7, 8):
        args = list(ok)
        args[i] = None
        _refused(native, "field_fwd_multi: null pointer", name, *args)
    _refused(native, "field_fwd_multi: K=0 out of range [1,16]", name, d, 64, d, d, 0, d, 0, d, d, None)
    _refused(native, "field_fwd_multi: K=17 out of range [1,16]", name, d, 64, d, d, 0, d, 17, d, d, None)
    _refused(native, "field_fwd_multi: planes_layout must be NSIG_PLANES_F32 (0) or NSIG_PLANES_MIXED (1)", name, d, 64, d, d, 2, d, 2, d, d, None)
    _refused(native, "field_fwd_multi: packed must be 16-byte aligned", name, d, 64, native._vp(264), d, 0, d, 2, d, d, None)
    _refused(native, "field_fwd_multi: planes and cplanes must be 8-byte aligned", name, d, 64, d, native._vp(260), 0, d, 2, d, d, None)
    _refused(native, "field_fwd_multi: planes and cplanes must be 8-byte aligned", name, d, 64, d, d, 0, native._vp(260), 2, d, d, None)
    _refused(native, "field_fwd_multi: M=134217729 too large", name, d, (1 << 27) + 1, d, d, 0, d, 2, d, d, None)
    before = native.fn("mlp_get_precision")()
    native.set_mlp_precision("bf16x3")
    try:
        _refused(native, "field_fwd_multi: this plane set was written in the mixed (fp16) layout; the split-bf16 MLP needs hg_encode_planes", name,
                 d, 64, d, d, 1, d, 2, d, d, None)
    finally:
        native.call("mlp_set_precision", before)


def test_byte_size_queries(native):
    presum, planes, single = native.fn("hg_multi_presum_bytes"), native.fn("hg_multi_planes_bytes"), native.fn("hg_planes_bytes")
    for K in range(1, 17):
        assert presum(K) == K * 4 * MIB
    counts = (1, 31, 32, 33, 127, 128, 129, 1025, 4608 * 280)
    for M in counts:
        stride_bytes = single(M) // 17          # one float2 plane of a plane set of M points
        assert single(M) == 17 * stride_bytes and stride_bytes % (32 * 8) == 0 and stride_bytes >= 8 * M
        for K in range(1, 17):
            assert planes(M, K) == K * stride_bytes
            assert K == 1 or planes(M, K) > planes(M, K - 1)
    for K in (1, 3, 16):
        sizes = [planes(M, K) for M in counts]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]


def test_messages_are_dealt_in_order():
    from nerf_signature_amd import fieldops as fo
    assert fo.MULTI_MAX_MESSAGES == 16
    chunks = fo.message_chunks(200, 16)
    assert len(chunks) == 13 and [b - a for a, b in chunks] == [16] * 12 + [8]
    assert [i for a, b in chunks for i in range(a, b)] == list(range(200))
    assert fo.message_chunks(16, 16) == [(0, 16)] and fo.message_chunks(17, 16) == [(0, 16), (16, 17)] and fo.message_chunks(1, 16) == [(0, 1)]
    assert fo.message_chunks(0, 16) == []
    with pytest.raises(ValueError):
        fo.message_chunks(5, 0)


def test_header_constant_matches_the_host_constant():
    import os
    from nerf_signature_amd import fieldops as fo
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerfsig.h")).read()
    assert int(re.search(r"#define NSIG_MULTI_MAX_MESSAGES (\d+)", text).group(1)) == fo.MULTI_MAX_MESSAGES
