"""tests/draw_ref.py against known words.  The table was computed once with the four restatements draw_ref.py replaced (error_map_ref's numpy mix32 family,
orbit_ref's Python-int one, grid_refresh_ref's and tamper_ref's mix64), which agreed with each other on every entry; it is what keeps the host side of every
bit-exact draw test from drifting together with nothing to notice it."""
import numpy as np

import draw_ref as dr

SEEDS = [0, 1, 1 << 32, (1 << 64) - 1]
COUNTERS = [0, 1, (1 << 32) - 1]
STREAMS = [0, 1, 2, 3, 4, 5]
INDICES = [0, 1, (1 << 32) - 1]

# mix64(seed)
MIX64 = [0x0000000000000000, 0x5692161D100B05E5, 0xD820B7E910B0F93F, 0xB4D055FCF2CBBD7B]
# stream_key(seed, counter): [seed][counter]
KEYS = [
    [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0xBEEB67EAF1FC5E61],
    [0xE4D971771B652C20, 0xBEEB8DA1658EEC67, 0xC3FC3482A90CD79A],
    [0x219FC13D6BC5B015, 0x37AD5FDD5756BD3D, 0x7E14065B84AE508B],
    [0xDE0A564CBCD060C4, 0x738B10AF171367FF, 0x9011E6053017523E],
]
# draw64(KEYS[seed][counter], index): [seed][counter][index]
DRAW64 = [
    [
        [0x2FF145472E2746D6, 0x7B575A03C5870447, 0x6611ED784A7012E4],
        [0x26F3A00703FD88C5, 0x94BE694511DDC182, 0x4BA783B1DA35B46F],
        [0x72D12439417017B9, 0x0518CDFBAD49513D, 0xD18980E396F4E97C],
    ],
    [
        [0x6B07B7D0A7AFE795, 0xFE6E71628F888CED, 0xA1E916C0F38DB07B],
        [0xBB1D2681F3984480, 0xACD26DF696CAA62D, 0xD8F69B9E8CA43557],
        [0xB516B345CF9DA9B0, 0xDE9BFC22D925D020, 0xD90DEA9E87BB4734],
    ],
    [
        [0x5011D7E41485A44B, 0x051B53D0C98CE598, 0x3B8B77DEADCD8483],
        [0x171B138203AC0B64, 0xE1B64D454D4CAE61, 0x7693D6DC848778E0],
        [0xE7035A9C0683310C, 0x3862530403DB3C24, 0xE0F956DC11882973],
    ],
    [
        [0x1D65B6B06BE545B4, 0x9089F677D6A70CA6, 0x344BE259D8FE3196],
        [0xCA7AEF6B91C16587, 0x498DF726382683C5, 0x8BEBB6F9112FFE3D],
        [0xEDD40767A5F594BD, 0x579ADEC1236B96A7, 0x841BE5BEB8C3F366],
    ],
]
# mix32(counter)
MIX32 = [0x00000000, 0x514E28B7, 0x81F16F39]
# draw_base(seed, counter, stream): [seed][counter][stream]
BASES = [
    [
        [0x00000000, 0x4BC0FBEB, 0x5A3454BF, 0x963AE4B1, 0xAE68F829, 0xB04D2F1A],
        [0xAA3E5B61, 0x2FFDF3F7, 0x91FBD784, 0xF61896E8, 0x1CC2FACE, 0x5570CBEB],
        [0x3699BC7B, 0x90380935, 0x66720B19, 0x36104BB7, 0x7212269D, 0x23C54AB5],
    ],
    [
        [0x2FEF5C8F, 0x2D235D53, 0x4D164D50, 0x067696C3, 0x6ECB67A8, 0x7FDE15A9],
        [0x9941CD2D, 0x8A5B8510, 0x7CE6F933, 0x9CE80E45, 0x9ACE61EB, 0x08526F23],
        [0x3FB4E464, 0xC521797A, 0xAE4467EB, 0xBD5817E4, 0x51D00876, 0xA04379FC],
    ],
    [
        [0x514E28B7, 0xA49E0D39, 0xC3244901, 0xC9EDFA7E, 0xDE3887C7, 0xC74AFC5B],
        [0x6F0B28E6, 0xED1B3D55, 0xCA52FE21, 0xE804E4C6, 0x57FFDF90, 0xBB1C27A0],
        [0x907E88C1, 0x00755464, 0x7B744A3E, 0xEADDF32E, 0xD43D0E21, 0xD0FCFE4A],
    ],
    [
        [0xE210E9F0, 0xE012ADCA, 0x5DF77DD0, 0xE3D5D1BD, 0x8F05FD06, 0x2BAE05A0],
        [0xDA705282, 0xA15A2010, 0x5B0B3A7C, 0x7E784608, 0x1C94983A, 0x02C6F821],
        [0x4D80FE65, 0x69F7B640, 0xEE394A1B, 0x4914F2A2, 0x2DA3580A, 0x728DA2B6],
    ],
]
# draw_word(BASES[seed][counter][stream], index): [seed][counter][stream][index]
WORDS = [
    [
        [[0xE227D219, 0xA08696D0, 0x34972489], [0x48740548, 0xE4B5A295, 0x6B384A45], [0x91CE0D65, 0x66208F53, 0x455AE672],
         [0xC3F901C5, 0x45EBAF63, 0x0DA9F042], [0xB9688445, 0x7A4808F4, 0xAFBC90E3], [0x3A88FA82, 0x7CA1CE76, 0x85C1E4C8]],
        [[0xA8775073, 0xE7BAA853, 0x6E3DD3B3], [0xB4962814, 0x27F54A7B, 0x4FA2AEA1], [0x91317C81, 0xBBEA14DA, 0x7F426C1E],
         [0x4DD1249C, 0x738FDD44, 0x9FE934DA], [0x7D00E92F, 0xA68C7117, 0x7BF4C9F4], [0x6A01A6B3, 0x0556B288, 0x351AC19C]],
        [[0xC2C5153A, 0xD9F4ED26, 0x18ABC0FF], [0x4B6C3CFE, 0x91134937, 0x5D80A686], [0x36ACF155, 0x4E358E91, 0xCA4745C4],
         [0xF0365B52, 0x1843B48C, 0x44A286AD], [0x9BB1B5F4, 0xDDD2C94E, 0xEF04639D], [0xCE5E8D73, 0xA6505559, 0x8C492F59]],
    ],
    [
        [[0xEAFBA055, 0x89D3537E, 0xA02AB27B], [0xFD3D85AD, 0x025D29EA, 0x636D3F56], [0x893FAAC2, 0xC203811E, 0xF44AC122],
         [0x6B88B89F, 0x72987C70, 0x42846FBF], [0xF2A52A67, 0x31696D7E, 0x786A61DB], [0x7CC06EE2, 0x5068DC86, 0x0448F2E4]],
        [[0x9F5D075C, 0x5F818845, 0x2A85AC48], [0x194D4AE6, 0x38D7F634, 0x2E2825D7], [0xE7FC116B, 0x35CB30CF, 0x52C94272],
         [0x41BC0D46, 0xA311722E, 0xA8333E8C], [0xBAE43360, 0xFBECB0D4, 0x18C3AE90], [0x4292D232, 0x625B0BA1, 0xC9230865]],
        [[0xB7A6CB9B, 0x7CF91234, 0x15753163], [0x04640708, 0x71A58854, 0xEE723A6A], [0x16FBA07F, 0x08DD7E3F, 0x7E1ED812],
         [0xB0497D14, 0x05D6478E, 0xC2E263B2], [0x09C9F561, 0xAC47C0FC, 0x6AF469D4], [0xDC2089AF, 0xB2296185, 0x6E2C9BD9]],
    ],
    [
        [[0x298620AF, 0x356FD98B, 0x8ED5CC0B], [0x11A55E44, 0xD491C8EC, 0xBFD645FC], [0xD2CF6891, 0x15A2F573, 0x8FCDF0FB],
         [0x57A8052F, 0x525029FB, 0x601C1CEE], [0xDDA57399, 0x187A2453, 0xE4EADE1C], [0x9A5BE933, 0x597F1598, 0x4A193016]],
        [[0x2D0454AA, 0x9077126F, 0x736499B4], [0xCE18DB18, 0x864ABD2E, 0x2AB33D49], [0x042AFBF2, 0x4E019F4D, 0xD7C70D03],
         [0x9D009501, 0x5CC9CA80, 0x9F30EDAA], [0xAE7B6C4F, 0x7F969D94, 0x77550AEF], [0x69C91F41, 0x7B8F73A9, 0x3E5BE49D]],
        [[0xDD03809A, 0xDF122064, 0xBF9435C8], [0xCE8A6691, 0xC516CCFC, 0x07153E6E], [0x8ABA1E7B, 0x63224D8F, 0x568C2862],
         [0xDF067CB2, 0xEDE1A712, 0xEC2C8C00], [0x5583CA8D, 0xA3AEF472, 0x82A4E1B4], [0x8B3A917F, 0x447ED2CF, 0xE3605099]],
    ],
    [
        [[0x48DA3F0F, 0x7D4CD98F, 0xD24679A1], [0x9B93EFEC, 0x23C40DC1, 0x6D22C3F5], [0xB4B75D31, 0xB74E0E32, 0x493EFF99],
         [0xE64A4BB5, 0x18468304, 0x7170ECC5], [0x9352CD9B, 0x7E621217, 0x0B8816FC], [0x39812788, 0x3E57A08A, 0x43A585D7]],
        [[0x42F3BEB7, 0xFD0CB6F8, 0xB83705AC], [0xEA69DAA4, 0x0092214C, 0x0B3C0B3E], [0x9CF02A2A, 0x0FBAAE37, 0xE9844C84],
         [0x35FAA627, 0xA45875DE, 0xEE13E9B0], [0x6BF8D7B6, 0xDB471819, 0x376E2450], [0x3A0B625A, 0x1E264C02, 0xB8F53C28]],
        [[0x53BDB882, 0x2A3A9338, 0x38C9E19B], [0x2267FE9C, 0xD3435633, 0x62FB07F0], [0x8C7D7E8B, 0x31FE68AF, 0x396D9B52],
         [0x08E9163C, 0x388FC395, 0x6880CBB0], [0x706358B6, 0xEB5B05BD, 0x7689E3C7], [0xF6DC98CB, 0x9F821C4F, 0x741AA036]],
    ],
]


def test_family64_known_words():
    assert [dr.mix64(s) for s in SEEDS] == MIX64
    assert [[dr.stream_key(s, k) for k in COUNTERS] for s in SEEDS] == KEYS
    assert [[[dr.draw64(KEYS[a][b], i) for i in INDICES] for b in range(3)] for a in range(4)] == DRAW64


def test_family32_known_words():
    assert [dr.mix32(c) for c in COUNTERS] == MIX32
    assert [[[dr.draw_base(s, k, st) for st in STREAMS] for k in COUNTERS] for s in SEEDS] == BASES
    assert [[[[dr.draw_word(BASES[a][b][c], i) for i in INDICES] for c in range(6)] for b in range(3)] for a in range(4)] == WORDS


def test_arrays_and_ints_agree():
    """The array path computes what the scalar path computes, and returns uint64 arrays."""
    idx = np.array(INDICES, dtype=np.uint64)
    for a, s in enumerate(SEEDS):
        for b, k in enumerate(COUNTERS):
            got = dr.draw64(dr.stream_key(s, k), idx)
            assert got.dtype == np.uint64 and got.tolist() == DRAW64[a][b]
            assert dr.stream_key(s, np.array([k], dtype=np.uint64)).tolist() == [KEYS[a][b]]
            for c in STREAMS:
                got = dr.draw_word(dr.draw_base(s, k, c), idx)
                assert got.dtype == np.uint64 and got.tolist() == WORDS[a][b][c]
    assert dr.mix64(np.array(SEEDS, dtype=np.uint64)).tolist() == MIX64
    assert dr.mix32(np.array(COUNTERS, dtype=np.uint64)).tolist() == MIX32
    assert isinstance(dr.mix64(1), int) and isinstance(dr.draw_base(1, 1, 1), int) and isinstance(dr.draw_word(np.uint64(1), 1), int)


def test_unit24_grids():
    """[0, 1) and (0, 1] on the 2^-24 grid, exact in float32."""
    assert dr.unit24(0) == 0.0 and dr.unit24((1 << 24) - 1) == 1.0 - 2.0 ** -24
    assert dr.unit24_open0(0) == 2.0 ** -24 and dr.unit24_open0((1 << 24) - 1) == 1.0
    w = np.array([0, 1, 0x800000, 0xFFFFFF], dtype=np.uint64)
    for f in (dr.unit24, dr.unit24_open0):
        u = f(w)
        assert u.dtype == np.float64 and np.array_equal(u.astype(np.float32).astype(np.float64), u)
        assert u.tolist() == [f(int(x)) for x in w]
