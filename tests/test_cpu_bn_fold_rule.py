"""gm_bn_fold_blocks(M, C, rows, G): the host rule that sizes the folded BatchNorm finalize +
apply launch (workgroups per 64-channel slice and view group) or declines it (0: the entry
points then issue the two launches).  A pure host function: no device here.

The recorded values below were filled in from the library after its constants were set from
the per-shape table of tools/bn_fold_probe.py; the (M, C, rows, G) are
the shapes that probe recorded from the C2 step (ResNet-18, 2 views, B = 64) and, for
ResNet-50, from the C5 step (12 views, B = 32).  A change of the rule has to come with a new
table."""
import pytest


@pytest.fixture(scope="module")
def rule():
    from greedy_multimodal_learning_amd import build
    build.build()
    from greedy_multimodal_learning_amd import _lib as L
    return L.load().gm_bn_fold_blocks


def test_declines(rule):
    assert rule(0, 64, 1, 2) == 0, "M = 0"
    assert rule(-5, 64, 1, 2) == 0
    assert rule(3136, 512, 1024, 2) > 0, "the row limit itself still folds"
    assert rule(3136, 512, 1025, 2) == 0, "rows above the limit"
    assert rule(3136, 512, 100000, 2) == 0
    assert rule(3136, 512, 0, 2) == 0 and rule(3136, 512, 25, 0) == 0
    assert rule(3136, 32, 25, 2) == 0 and rule(3136, 96, 25, 2) == 0, "C a multiple of 64"
    assert rule(105, 128, 300, 2) == 0, "the rows' re-read would pass twice the slice's bytes"
    assert rule(1 << 25, 64, 25, 1) == 0, "32-bit vector offsets"
    assert rule(200704, 64, 128, 4) == 0, "more than 2^25 elements over the groups"


@pytest.mark.parametrize("M", [1, 2, 7, 105, 127, 128, 129, 1000, 3136, 12544, 50176, 200704])
@pytest.mark.parametrize("C", [64, 128, 512, 2048])
@pytest.mark.parametrize("rows", [1, 25, 98, 392, 1024])
@pytest.mark.parametrize("G", [1, 2, 3, 12])
def test_never_more_blocks_than_work_items(rule, M, C, rows, G):
    """A work item is one thread's four 16-B vectors of the slice's band (8 vectors per pixel):
    2 M of them per (slice, group).  Also: at most one block per 128-pixel chunk, and the
    re-read nb * rows * 512 B stays within twice the slice's x + y bytes."""
    nb = rule(M, C, rows, G)
    assert 0 <= nb <= (8 * M + 3) // 4
    assert nb <= (M + 127) // 128
    assert nb * rows * 512 <= 2 * M * 256


RECORDED = [  # M, C, rows, G, blocks
    # ResNet-18 at C2: layer 1, layer 2 (+ its downsample), layer 3 (+ ds), layer 4 (+ ds)
    (200704, 64, 128, 2, 128),
    (50176, 128, 392, 2, 64),
    (50176, 128, 784, 2, 64),
    (12544, 256, 98, 2, 32),
    (12544, 256, 196, 2, 32),
    (3136, 512, 25, 2, 13),
    (3136, 512, 49, 2, 13),
    # ResNet-50 at C5: the layer-1 shapes (all declined: 77 M and 308 M elements over the 12 views)
    (100352, 64, 21, 12, 0),
    (100352, 64, 1568, 12, 0),
    (100352, 256, 1568, 12, 0),
    # and the ResNet-50 shapes the rule folds, with the first it declines in layers 2 and 4
    (25088, 128, 196, 12, 0),
    (6272, 256, 98, 12, 5),
    (1568, 512, 25, 12, 2),
    (1568, 2048, 25, 12, 0),
]


@pytest.mark.parametrize("case", RECORDED, ids=lambda c: "x".join(map(str, c[:4])))
def test_recorded_trunk_shapes(rule, case):
    M, C, rows, G, nb = case
    assert rule(M, C, rows, G) == nb
