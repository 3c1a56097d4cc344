"""The BatchNorm regime harness (bnregimes.py) and the CPU-side conditions of
test_gpu_bn_regimes.py's cases: the inputs are what the table says, the ReLU rounding band is
(nearly) empty, every mutant of the reference violates its bound on at least 1 % of the checked
elements or channels, and an fp32 emulation of the kernels' apply formulas stays inside the bounds
at every shape the GPU module uses.  No GPU: these are conditions on the inputs and the bounds."""
import pytest
import torch

import bnregimes as R

STREAM_STANDIN = (1, 64, 1, 66000)   # the size class of the streaming rows (their M is found on the device)
SHAPES = R.EXACT_SHAPES + R.INEXACT_SHAPES + R.POOL_SHAPES + [STREAM_STANDIN]
ISSUE_SHAPES = [(16, 64, 56, 56), (64, 512, 7, 7)]   # where the old recipe hid two terms of dx
FORMS = [(False, False), (True, False), (True, True)]
ids = lambda s: "x".join(map(str, s))  # noqa: E731

_cases = {}


def case(shape, group=0):
    if (shape, group) not in _cases:
        _cases[shape, group] = R.build(shape, R.seed(shape, group), res=True)
    return _cases[shape, group]


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_inputs_follow_the_table(shape):
    c = case(shape)
    x, reg = c.x, c.reg
    assert sorted(set(reg.tolist())) == list(range(8))
    assert torch.equal(x, R.rne(x)) and torch.equal(c.dy, R.rne(c.dy)) and torch.equal(c.res, R.rne(c.res))
    assert bool((x[:, reg == 3] == 16).all())
    assert bool(((x[:, reg == 1] - 16).abs() <= 1).all()) and bool(((x[:, reg == 7] + 16).abs() <= 1).all())
    assert bool(((x[:, reg == 2] - 1).abs() <= 2 / 128).all())
    g = c.gamma
    assert bool((g[reg == 4] < 0).all()) and bool((g[reg == 5] == 0).all())
    assert bool((g[reg == 6] == 2.0 ** -10).all()) and bool((g[reg == 7] == 32).all())
    assert bool((c.beta.abs() >= 0.1).all())
    if c.C >= 16:
        b5 = c.beta[reg == 5]
        assert int((b5 > 0).sum()) == int((b5 < 0).sum())
    assert c.exact == (c.M <= R.EXACT_M)
    f = R.forward_ref(c, False, False)
    if c.M >= 64:
        r1 = (reg == 1) | (reg == 7)
        ratio = f.mean[r1].abs() * f.invstd[r1]
        assert 20 < float(ratio.min()) and float(ratio.max()) < 35          # |mean| / std ~ 26
        v2 = f.var[reg == 2]
        assert 0.5e-4 < float(v2.min()) and float(v2.max()) < 2.5e-4
        eps_moves = 1 - torch.sqrt(v2 / (v2 + R.EPS))
        assert 0.02 < float(eps_moves.min()) and float(eps_moves.max()) < 0.08    # eps: ~4 % of invstd
    assert bool((f.var[reg == 3] == 0).all())
    assert bool(((f.invstd[reg == 3] / R.EPS ** -0.5 - 1).abs() < 1e-15).all())


@pytest.mark.parametrize("shape", SHAPES + ISSUE_SHAPES, ids=ids)
def test_all_three_terms_of_dx_are_visible(shape):
    """Dropping mean(dz) or the projection term moves dx by tens of percent of max|dx| per
    channel group - at every size, the large maps of the streaming variants included."""
    c = case(shape)
    f = R.forward_ref(c, False, False)
    b = R.backward_ref(c, f)
    ordinary = c.reg == 0
    scale = float(b.dx[:, ordinary].abs().max())
    for term in ("mean", "proj"):
        moved = float((R.backward_ref(c, f, drop=(term,)).dx - b.dx)[:, ordinary].abs().max()) / scale
        assert moved > 0.1, (term, moved)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("group", [0, 1])
def test_relu_band_is_nearly_empty(shape, group):
    c = case(shape, group)
    for relu, res in FORMS[1:]:
        assert R.assert_band_small(R.forward_ref(c, relu, res), f"{shape} res={res}") <= R.MASK_BAND_CAP


# (1, 2048, 2, 2) is left out: four pixels a channel carry no statistics to speak of
@pytest.mark.parametrize("shape", [s for s in SHAPES + ISSUE_SHAPES if s[0] * s[2] * s[3] >= 64], ids=ids)
def test_mutants_violate_the_bounds(shape, capsys):
    c = case(shape)
    rates = R.assert_discriminates(c, what=str(shape))
    assert ("running_var_biased" in rates) == c.exact
    with capsys.disabled():
        print(f"\n  mutants {ids(shape)}: {R.fmt(rates)}")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_fp32_emulation_stays_inside_the_bounds(shape, capsys):
    """Coefficients rounded to fp32, fp32 multiply-add, one bf16 store: inside the bounds with
    K = 16 (the emulation's sums are exact) in all three forms."""
    c = case(shape)
    worst = {}
    for relu, res in FORMS:
        f = R.forward_ref(c, relu, res)
        y = R.emulate_forward(c, f, relu, res)
        wy, mask = R.check_forward(f, y, True, f"emulation {shape}")
        b = R.backward_ref(c, f, mask=mask)
        dx = R.emulate_backward(c, f, b, b.dres)
        w = R.check_backward(c, b, 16, True, f"emulation {shape}", dx=dx, dres=b.dres)
        worst[f"y{int(relu)}{int(res)}"] = wy
        worst[f"dx{int(relu)}{int(res)}"] = w["dx"]
    with capsys.disabled():
        print(f"\n  emulation {ids(shape)}: {R.fmt(worst)}")


def test_two_kernel_plan_and_chain():
    assert R.two_kernel_rows(693, 64) == (32, 32)          # one row per thread, 32 rows per pass
    assert R.two_kernel_rows(1568, 256) == (32, 32)
    assert R.two_kernel_rows(75, 8) == (256, 256)
    assert R.chain(32, 64) == 33 and R.chain(512, 64) == 48 and R.chain(256, 8) == 257


def test_pool_gather_scatters_to_the_selected_pixels():
    shape = (1, 8, 4, 4)
    c = R.build(shape, 1)
    idx = torch.full((1, 2, 2, 8), 4, dtype=torch.uint8)     # the window centre: pixel (2p, 2q)
    yp = torch.ones(1, 8, 2, 2)
    yp[0, :, 1, 1] = 0                                        # this window did not pass the ReLU
    dyp = torch.arange(1.0, 5.0).view(1, 1, 2, 2).expand(1, 8, 2, 2)
    g = R.nchw(R.pool_gather(c, dyp, yp, idx, 3, 2, 1), shape)
    want = torch.zeros(4, 4, dtype=torch.float64)
    want[0, 0], want[0, 2], want[2, 0] = 1, 2, 3
    for ch in range(8):
        assert torch.equal(g[0, ch], want)
