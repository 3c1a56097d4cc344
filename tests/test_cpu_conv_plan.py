"""CPU-only: the convolution planner's size queries keep their values.

No kernel is launched: the library loads without a device (its CU count then falls back to 256,
the MI355X's).  Every distinct 3x3, pixel-pair-stem and 1x1 convolution of ResNet-18 and ResNet-50
at 224^2 with N = 64, and small odd shapes, for G in {1, 2, 12}: the split-K workspace bytes
(forward, input gradient), the stem's statistics rows and the two BatchNorm-statistics buffer
bounds, under the default switches, with the halo kernels off and with split-K off.

EXPECTED was recorded from the library as it stood before the kernel choice became a plan value
(conv_plan.h), by running measure() below against that build - not from the code under test.
"""
import ctypes

import pytest

GS = (1, 2, 12)
SETTINGS = ("default", "halo0", "splitk0")

# (N, H, W, C, K, R, S, stride_h, stride_w, pad_h, pad_w)
def _sq(N, H, W, C, K, R, st):
    return (N, H, W, C, K, R, R, st, st, R // 2, R // 2)


SHAPES = [
    # the 7x7/s2 stem at 224^2 as the 7x4 pixel-pair filter (conv.py _stem_geom: Hp 229, Wp/2 115)
    (64, 229, 115, 8, 64, 7, 4, 2, 1, 0, 0),
    # 3x3: ResNet-18 / ResNet-50
    _sq(64, 56, 56, 64, 64, 3, 1), _sq(64, 56, 56, 64, 128, 3, 2), _sq(64, 56, 56, 128, 128, 3, 2),
    _sq(64, 28, 28, 128, 128, 3, 1), _sq(64, 28, 28, 128, 256, 3, 2), _sq(64, 28, 28, 256, 256, 3, 2),
    _sq(64, 14, 14, 256, 256, 3, 1), _sq(64, 14, 14, 256, 512, 3, 2), _sq(64, 14, 14, 512, 512, 3, 2),
    _sq(64, 7, 7, 512, 512, 3, 1),
    # 1x1: ResNet-18's downsamples, ResNet-50's bottlenecks and downsamples
    _sq(64, 56, 56, 64, 128, 1, 2), _sq(64, 28, 28, 128, 256, 1, 2), _sq(64, 14, 14, 256, 512, 1, 2),
    _sq(64, 56, 56, 64, 64, 1, 1), _sq(64, 56, 56, 64, 256, 1, 1), _sq(64, 56, 56, 256, 64, 1, 1),
    _sq(64, 56, 56, 256, 128, 1, 1), _sq(64, 28, 28, 128, 512, 1, 1), _sq(64, 28, 28, 512, 128, 1, 1),
    _sq(64, 28, 28, 512, 256, 1, 1), _sq(64, 14, 14, 256, 1024, 1, 1), _sq(64, 14, 14, 1024, 256, 1, 1),
    _sq(64, 14, 14, 1024, 512, 1, 1), _sq(64, 7, 7, 512, 2048, 1, 1), _sq(64, 7, 7, 2048, 512, 1, 1),
    _sq(64, 56, 56, 256, 512, 1, 2), _sq(64, 28, 28, 512, 1024, 1, 2), _sq(64, 14, 14, 1024, 2048, 1, 2),
    # small odd cases: N = 3 at 37 x 30, and 1 x 3 x 62
    _sq(3, 37, 30, 64, 64, 3, 1), _sq(3, 37, 30, 128, 128, 3, 1), _sq(3, 37, 30, 64, 128, 3, 2),
    _sq(3, 37, 30, 64, 128, 1, 2), _sq(3, 37, 30, 256, 512, 3, 1),
    _sq(1, 3, 62, 64, 64, 3, 1), _sq(1, 3, 62, 128, 128, 3, 1), _sq(1, 3, 62, 64, 128, 3, 2),
    _sq(1, 3, 62, 64, 128, 1, 2), _sq(1, 3, 62, 256, 512, 3, 1),
]


def measure(L):
    """{setting: [(ws_fwd, ws_dgrad, stem_rows, fwd_floats, dgrad_floats) per (shape, G)]}; the
    gm_conv_desc queries are -1 for shapes only gm_conv_desc_hw describes (the stem)."""
    lib = L.load()
    saved = L.get_residency()
    out = {}
    try:
        L.set_residency(2, 1, 0)
        for setting in SETTINGS:
            try:
                if setting == "halo0":
                    L.check(lib.gm_conv_set_halo(0), "halo")
                if setting == "splitk0":
                    L.check(lib.gm_conv_set_splitk(0), "splitk")
                rows = []
                for s in SHAPES:
                    hw = L.ConvDescHW(*s)
                    N, H, W, C, K, R, S, sh, sw, ph, pw = s
                    sq = L.ConvDesc(N, H, W, C, K, R, S, sh, ph) if (R == S and sh == sw and ph == pw) else None
                    for G in GS:
                        row = [-1, -1, lib.gm_conv_stem_stats_rows(ctypes.byref(hw), G),
                               lib.gm_conv2d_fwd_bn_stats_floats(ctypes.byref(hw), G), -1]
                        if sq is not None:
                            row[0] = lib.gm_conv2d_splitk_ws_bytes_grouped(ctypes.byref(sq), G, 0)
                            row[1] = lib.gm_conv2d_splitk_ws_bytes_grouped(ctypes.byref(sq), G, 1)
                            row[4] = lib.gm_conv2d_dgrad_bn_stats_floats(ctypes.byref(sq), G)
                            if G == 1:
                                assert lib.gm_conv2d_splitk_ws_bytes(ctypes.byref(sq), 0) == row[0]
                                assert lib.gm_conv2d_splitk_ws_bytes(ctypes.byref(sq), 1) == row[1]
                        rows.append(tuple(row))
                out[setting] = rows
            finally:
                L.check(lib.gm_conv_set_halo(1), "halo")
                L.check(lib.gm_conv_set_splitk(384), "splitk")
    finally:
        L.set_residency(*saved)
    return out


EXPECTED = {
    "default": [
        (-1, -1, 512, 1605760, -1), (-1, -1, 256, 3211520, -1), (-1, -1, 64, 19269120, -1),
        (0, 0, 0, 401536, 401792), (0, 0, 0, 803072, 803584), (0, 0, 0, 4818432, 4821504),
        (0, 0, 0, 200960, 401792), (0, 0, 0, 401920, 803584), (0, 0, 0, 2411520, 4821504),
        (0, 0, 0, 200960, 803584), (0, 0, 0, 401920, 1607168), (0, 0, 0, 2411520, 9643008),
        (0, 0, 0, 200960, 201472), (0, 0, 0, 401920, 402944), (0, 0, 0, 2411520, 2417664),
        (0, 0, 0, 131584, 201472), (0, 0, 0, 263168, 402944), (0, 0, 0, 1579008, 2417664),
        (12910592, 0, 0, 131584, 402944), (0, 0, 0, 263168, 805888), (0, 0, 0, 1579008, 4835328),
        (12910592, 12910592, 0, 131584, 132608), (0, 0, 0, 263168, 265216), (0, 0, 0, 1579008, 1591296),
        (6619136, 0, 0, 263168, 132608), (13172736, 0, 0, 526336, 265216), (0, 0, 0, 3158016, 1591296),
        (6619136, 0, 0, 263168, 265216), (13172736, 0, 0, 526336, 530432), (0, 0, 0, 3158016, 3182592),
        (6619136, 6619136, 0, 263168, 265216), (13172736, 13172736, 0, 526336, 530432), (0, 0, 0, 3158016, 3182592),
        (0, 0, 0, 200960, 401792), (0, 0, 0, 401920, 803584), (0, 0, 0, 2411520, 4821504),
        (0, 0, 0, 131584, 201472), (0, 0, 0, 263168, 402944), (0, 0, 0, 1579008, 2417664),
        (0, 0, 0, 263168, 132608), (0, 0, 0, 526336, 265216), (0, 0, 0, 3158016, 1591296),
        (0, 0, 0, 401536, 401792), (0, 0, 0, 803072, 803584), (0, 0, 0, 4818432, 4821504),
        (0, 0, 0, 1606144, 401792), (0, 0, 0, 3212288, 803584), (0, 0, 0, 19273728, 4821504),
        (0, 0, 0, 401536, 1607168), (0, 0, 0, 803072, 3214336), (0, 0, 0, 4818432, 19286016),
        (0, 0, 0, 803072, 1607168), (0, 0, 0, 1606144, 3214336), (0, 0, 0, 9636864, 19286016),
        (0, 0, 0, 803840, 201472), (0, 0, 0, 1607680, 402944), (0, 0, 0, 9646080, 2417664),
        (0, 0, 0, 200960, 805888), (0, 0, 0, 401920, 1611776), (0, 0, 0, 2411520, 9670656),
        (0, 0, 0, 401920, 805888), (0, 0, 0, 803840, 1611776), (0, 0, 0, 4823040, 9670656),
        (0, 0, 0, 526336, 132608), (0, 0, 0, 1052672, 265216), (0, 0, 0, 6316032, 1591296),
        (0, 0, 0, 131584, 530432), (0, 0, 0, 263168, 1060864), (0, 0, 0, 1579008, 6365184),
        (0, 0, 0, 263168, 530432), (0, 0, 0, 526336, 1060864), (0, 0, 0, 3158016, 6365184),
        (0, 6619136, 0, 1052672, 265216), (0, 13172736, 0, 2105344, 530432), (0, 0, 0, 12632064, 3182592),
        (6619136, 0, 0, 263168, 1060864), (13172736, 0, 0, 526336, 2121728), (0, 0, 0, 3158016, 12730368),
        (0, 0, 0, 803840, 1607168), (0, 0, 0, 1607680, 3214336), (0, 0, 0, 9646080, 19286016),
        (0, 0, 0, 526336, 805888), (0, 0, 0, 1052672, 1611776), (0, 0, 0, 6316032, 9670656),
        (0, 13172736, 0, 1052672, 530432), (0, 0, 0, 2105344, 1060864), (0, 0, 0, 12632064, 6365184),
        (0, 0, 0, 32896, 33152), (0, 0, 0, 65792, 66304), (0, 0, 0, 394752, 397824),
        (0, 0, 0, 65792, 66304), (0, 0, 0, 131584, 132608), (0, 0, 0, 789504, 795648),
        (0, 0, 0, 65792, 33152), (0, 0, 0, 131584, 66304), (0, 0, 0, 789504, 397824),
        (0, 0, 0, 65792, 33152), (0, 0, 0, 131584, 66304), (0, 0, 0, 789504, 397824),
        (7143424, 3604480, 0, 263168, 132608), (14221312, 7143424, 0, 526336, 265216), (0, 0, 0, 3158016, 1591296),
        (0, 0, 0, 32896, 33152), (0, 0, 0, 65792, 66304), (0, 0, 0, 394752, 397824),
        (0, 0, 0, 65792, 66304), (0, 0, 0, 131584, 132608), (0, 0, 0, 789504, 795648),
        (0, 0, 0, 65792, 33152), (0, 0, 0, 131584, 66304), (0, 0, 0, 789504, 397824),
        (0, 0, 0, 65792, 33152), (0, 0, 0, 131584, 66304), (0, 0, 0, 789504, 397824),
        (589824, 327680, 0, 263168, 132608), (1114112, 589824, 0, 526336, 265216), (6356992, 3211264, 0, 3158016, 1591296),
    ],
}
# as recorded, gm_conv_set_halo(0) changed no value (the 256-pixel form alone has a workspace of
# its own) and gm_conv_set_splitk(0) zeroed every workspace and nothing else
EXPECTED["halo0"] = EXPECTED["default"]
EXPECTED["splitk0"] = [(min(r[0], 0), min(r[1], 0)) + r[2:] for r in EXPECTED["default"]]


@pytest.fixture(scope="module")
def measured():
    from greedy_multimodal_learning_amd import build, _lib as L
    build.build()
    return measure(L)


@pytest.mark.parametrize("setting", SETTINGS)
def test_size_queries_keep_their_values(measured, setting):
    got, want = measured[setting], EXPECTED[setting]
    assert len(got) == len(want) == len(SHAPES) * len(GS)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (setting, SHAPES[i // len(GS)], GS[i % len(GS)])


def test_table_exercises_the_planner():
    """The recorded table is not vacuous: it has split-K workspaces that the two switches change
    and the stem's rows."""
    d, h, s = (EXPECTED[k] for k in SETTINGS)
    assert any(r[0] > 0 for r in d) and any(r[1] > 0 for r in d) and any(r[2] > 0 for r in d)
    assert all(r[0] <= 0 and r[1] <= 0 for r in s)
    assert d != s
