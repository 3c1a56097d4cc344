"""CPU-only: the weight-gradient planner's size queries keep their values.

No kernel is launched: the library loads without a device (its CU count then falls back to 256,
the MI355X's).  The shapes of test_cpu_conv_plan.py for G in {1, 2, 12}: the scratch bytes of
gm_conv2d_wgrad_grouped_scratch (G x splits x slab x 4, so every kernel's split count), the
gm_conv_desc query at G = 1 and gm_conv2d_wgrad_stem_bn_ok, under the default switches, with
gm_conv_set_wgrad_loop at 0 (no dedicated 3x3 kernel), 14 (the halo kernel up to 512 channels, no
ring) and 16 (the ring alone), and with the stem kernel off.

EXPECTED was recorded from the library as it stood before the kernel choice became a plan value
(conv_wgrad_plan.h), by running measure() below against a build of that commit - not from the code
under test.
"""
import ctypes

import pytest

from test_cpu_conv_plan import GS, SHAPES

WGRAD_LOOP_DEFAULT = 22
# setting -> (gm_conv_set_wgrad_loop, gm_conv_set_wgrad_stem)
SETTINGS = {"default": (WGRAD_LOOP_DEFAULT, 1), "loop0": (0, 1), "loop14": (14, 1), "loop16": (16, 1),
            "stem0": (WGRAD_LOOP_DEFAULT, 0)}


def measure(L):
    """{setting: [(grouped_scratch, scratch, stem_bn_ok) per (shape, G)]}; the gm_conv_desc query
    is -1 for shapes only gm_conv_desc_hw describes (the stem) and for G > 1."""
    lib = L.load()
    out = {}
    try:
        for setting, (loop, stem) in SETTINGS.items():
            L.check(lib.gm_conv_set_wgrad_loop(loop), "wgrad_loop")
            L.check(lib.gm_conv_set_wgrad_stem(stem), "wgrad_stem")
            rows = []
            for s in SHAPES:
                hw = L.ConvDescHW(*s)
                N, H, W, C, K, R, S, sh, sw, ph, pw = s
                sq = L.ConvDesc(N, H, W, C, K, R, S, sh, ph) if (R == S and sh == sw and ph == pw) else None
                for G in GS:
                    row = [lib.gm_conv2d_wgrad_grouped_scratch(ctypes.byref(hw), G), -1,
                           lib.gm_conv2d_wgrad_stem_bn_ok(ctypes.byref(hw), G)]
                    if G == 1:
                        assert lib.gm_conv2d_wgrad_hw_scratch(ctypes.byref(hw)) == row[0]
                        if sq is not None:
                            row[1] = lib.gm_conv2d_wgrad_scratch(ctypes.byref(sq))
                    rows.append(tuple(row))
            out[setting] = rows
    finally:
        L.check(lib.gm_conv_set_wgrad_loop(WGRAD_LOOP_DEFAULT), "wgrad_loop")
        L.check(lib.gm_conv_set_wgrad_stem(1), "wgrad_stem")
    return out


EXPECTED = {
    "default": [
        (29360128, -1, 1), (29360128, -1, 1), (44040192, -1, 1), (18874368, 18874368, 0), (18874368, -1, 0),
        (17694720, -1, 0), (28901376, 28901376, 0), (28901376, -1, 0), (28311552, -1, 0), (33030144, 33030144, 0),
        (33030144, -1, 0), (28311552, -1, 0), (33030144, 33030144, 0), (33030144, -1, 0), (28311552, -1, 0),
        (25952256, 25952256, 0), (33030144, -1, 0), (28311552, -1, 0), (33030144, 33030144, 0), (33030144, -1, 0),
        (28311552, -1, 0), (33030144, 33030144, 0), (33030144, -1, 0), (28311552, -1, 0), (28311552, 28311552, 0),
        (28311552, -1, 0), (56623104, -1, 0), (28311552, 28311552, 0), (18874368, -1, 0), (113246208, -1, 0),
        (28311552, 28311552, 0), (18874368, -1, 0), (113246208, -1, 0), (3211264, 3211264, 0), (6422528, -1, 0),
        (16515072, -1, 0), (2883584, 2883584, 0), (5767168, -1, 0), (31457280, -1, 0), (3145728, 3145728, 0),
        (6291456, -1, 0), (31457280, -1, 0), (6422528, 6422528, 0), (7929856, -1, 0), (8257536, -1, 0),
        (15859712, 15859712, 0), (16515072, -1, 0), (16515072, -1, 0), (15859712, 15859712, 0), (16515072, -1, 0),
        (16515072, -1, 0), (31719424, 31719424, 0), (33030144, -1, 0), (33030144, -1, 0), (25690112, 25690112, 0),
        (31981568, -1, 0), (31457280, -1, 0), (25690112, 25690112, 0), (31981568, -1, 0), (31457280, -1, 0),
        (31981568, 31981568, 0), (33554432, -1, 0), (31457280, -1, 0), (23068672, 23068672, 0), (33554432, -1, 0),
        (25165824, -1, 0), (23068672, 23068672, 0), (33554432, -1, 0), (25165824, -1, 0), (33554432, 33554432, 0),
        (33554432, -1, 0), (25165824, -1, 0), (25165824, 25165824, 0), (33554432, -1, 0), (50331648, -1, 0),
        (25165824, 25165824, 0), (33554432, -1, 0), (50331648, -1, 0), (31981568, 31981568, 0), (33554432, -1, 0),
        (31457280, -1, 0), (33554432, 33554432, 0), (33554432, -1, 0), (25165824, -1, 0), (33554432, 33554432, 0),
        (16777216, -1, 0), (100663296, -1, 0), (8257536, 8257536, 0), (16515072, -1, 0), (17694720, -1, 0),
        (18874368, 18874368, 0), (18874368, -1, 0), (28311552, -1, 0), (294912, 294912, 0), (589824, -1, 0),
        (3538944, -1, 0), (32768, 32768, 0), (65536, -1, 0), (393216, -1, 0), (28311552, 28311552, 0),
        (28311552, -1, 0), (56623104, -1, 0), (442368, 442368, 0), (884736, -1, 0), (5308416, -1, 0),
        (1769472, 1769472, 0), (3538944, -1, 0), (14155776, -1, 0), (294912, 294912, 0), (589824, -1, 0),
        (3538944, -1, 0), (32768, 32768, 0), (65536, -1, 0), (393216, -1, 0), (4718592, 4718592, 0),
        (9437184, -1, 0), (56623104, -1, 0),
    ],
}
# the other settings as recorded: the rows (by index) that differ from the default table
_DIFF = {
    "loop0": {
        3: (15040512, 15040512, 0), 4: (15040512, -1, 0), 5: (14155776, -1, 0), 87: (884736, 884736, 0),
        88: (1769472, -1, 0), 89: (10616832, -1, 0), 90: (3538944, 3538944, 0), 91: (7077888, -1, 0),
        102: (147456, 147456, 0), 103: (294912, -1, 0), 104: (1769472, -1, 0), 105: (589824, 589824, 0),
        106: (1179648, -1, 0), 107: (7077888, -1, 0),
    },
    "loop14": {
        114: (14155776, 14155776, 0), 115: (18874368, -1, 0),
    },
    "stem0": {
        0: (14680064, -1, 0), 1: (14680064, -1, 0), 2: (14450688, -1, 0),
    },
}
# as recorded, bit 4 (the ring) changed no value: the query is the larger of the dedicated kernel's
# plan and k_conv_wgrad4's, and the ring, sized to half the CUs, never has more slabs than that
_DIFF["loop16"] = _DIFF["loop0"]
for _k, _d in _DIFF.items():
    EXPECTED[_k] = [_d.get(i, r) for i, r in enumerate(EXPECTED["default"])]


@pytest.fixture(scope="module")
def measured():
    from greedy_multimodal_learning_amd import build, _lib as L
    build.build()
    return measure(L)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_size_queries_keep_their_values(measured, setting):
    got, want = measured[setting], EXPECTED[setting]
    assert len(got) == len(want) == len(SHAPES) * len(GS)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (setting, SHAPES[i // len(GS)], GS[i % len(GS)])


def test_table_exercises_the_planner():
    """The recorded table is not vacuous: the settings do not all give one table, the stem's rows
    follow gm_conv_set_wgrad_stem, and 3x3 rows follow the halo bits of gm_conv_set_wgrad_loop
    (0 against the default and against 14).  Between 0 and 16 no row can differ - see above."""
    tables = [EXPECTED[k] for k in SETTINGS]
    assert any(t != tables[0] for t in tables[1:])
    stem = [i * len(GS) for i, s in enumerate(SHAPES) if s[5:7] == (7, 4)]
    assert stem and all(EXPECTED["default"][j] != EXPECTED["stem0"][j] for j in stem)
    assert all(EXPECTED["default"][j][2] == 1 and EXPECTED["stem0"][j][2] == 0 for j in stem)
    k3 = [i * len(GS) + g for i, s in enumerate(SHAPES) if s[5:7] == (3, 3) for g in range(len(GS))]
    for other in ("default", "loop14"):
        assert any(EXPECTED["loop0"][j] != EXPECTED[other][j] for j in k3)
    assert any(EXPECTED["default"][j] != EXPECTED["loop14"][j] for j in k3)
