"""The max-pool kernels (csrc/maxpool.hip) at their edges, exactly: every window form prep()
accepts, NaN and -inf by the documented rule, the gradient bit for bit, and grids past the
16384 x 256 cap so that every grid-stride loop runs a second trip.

Small cases: against endsref.pool_scan (a numpy restatement of `v > max || isnan(v)`, shown equal
to torch's CPU max_pool2d in test_cpu_endsref.py) on inputs whose routed sums are exact integers:
y must equal the reference with NaN exactly where it has NaN, and dx must be torch.equal to the
exact sum (fp32) or to its one rounding (bf16).  Second-trip cases: against F.max_pool2d on the
device in fp32 with indices, the same function at a size numpy would take minutes for - on an
NCHW-contiguous copy: torch's device kernel for channels_last input reports index 0 for a window
of nothing but -inf (observed: 25 such windows, every index 0), where its CPU and NCHW kernels
and ours select the first in-bounds position."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import endsref as E
import exactint as X

pytestmark = pytest.mark.gpu
CL = torch.channels_last
BF16 = torch.bfloat16
CAP = 16384 * 256          # grid_for() in maxpool.hip: the vectors one trip of the loop covers
pid = lambda c: "x".join(map(str, c[0])) + "-k%ds%dp%d" % c[1]  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


_cases = {}


def case(shape, win):
    if (shape, win) not in _cases:
        c = E.pool_inputs(shape, win)
        e = E.pool_expected(c)
        E.assert_pool_discriminates(c, e)
        _cases[shape, win] = (c, e)
    return _cases[shape, win]


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape,win", E.POOL_CASES, ids=[pid(c) for c in E.POOL_CASES])
def test_pool_windows_nan_and_exact_gradient(dev, shape, win, dtype):
    from greedy_multimodal_learning_amd.pool import GMMaxPool2d
    c, e = case(shape, win)
    x = c.x.to(dev, dtype).contiguous(memory_format=CL).requires_grad_(True)
    y = GMMaxPool2d(*win)(x)
    y.backward(c.dy.to(dev, dtype).contiguous(memory_format=CL))
    got_y, got_dx = y.detach().float().cpu(), x.grad.float().cpu()
    assert y.dtype == dtype and x.grad.dtype == dtype
    assert E.same(got_y, e.y), f"y differs on {E.frac_differs(got_y, e.y):.4f} of the outputs"
    assert torch.equal(torch.isnan(got_y), torch.isnan(e.y))
    want = X.rne(e.dx) if dtype == BF16 else e.dx.float()
    assert torch.equal(got_dx, want), f"dx differs on {X.frac_ne(got_dx, want):.4f} of the inputs"
    assert bool((got_dx[e.terms == 0] == 0).all())       # unselected and uncovered pixels: exactly 0


# ---- second trips -----------------------------------------------------------------------------------

BIG = (4, 256, 129, 257)


def big_input(dev, seed):
    """The integer recipe at the size of the second trip, made on the device: bf16 [N, C, H, W]
    channels_last with 1 % NaN, 0.7 % -inf and two all -inf blocks."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randint(-2, 3, BIG, device=dev, generator=g).to(BF16)
    r = torch.rand(BIG, device=dev, generator=g)
    x[r < 0.01] = float("nan")
    x[(r >= 0.01) & (r < 0.017)] = float("-inf")
    del r
    x[0, 7, :4, :4] = float("-inf")
    x[3, 255, 60:66, 100:106] = float("-inf")
    return x.contiguous(memory_format=CL)


def big_dy(dev, shape, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    mag = torch.randint(0, 128, shape, device=dev, generator=g).float() * 2 + 1
    sign = torch.randint(0, 2, shape, device=dev, generator=g).float() * 2 - 1
    return (mag * sign).to(BF16).contiguous(memory_format=CL)


def same_dev(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("win", [(3, 1, 1), (3, 2, 1)], ids=["k3s1p1", "k3s2p1"])
def test_pool_second_trip(dev, win):
    """(3, 1, 1): the second trip of the 3 x 3 forward and of the generic backward; (3, 2, 1): of
    the 2 x 2-window backward (and the 3 x 3 forward's first trip at the stem's stride)."""
    from greedy_multimodal_learning_amd.pool import GMMaxPool2d
    N, C, H, W = BIG
    k, s, pad = win
    P, Q = E.pool_out(H, W, k, s, pad)
    assert N * H * W * C // 8 > CAP                        # the backward strides over the input
    if s == 1:
        assert N * P * Q * C // 8 > CAP                    # the forward over the output
    X.assert_exact_bound((-(-k // s)) ** 2, 255)
    x = big_input(dev, 10 + s)
    dy = big_dy(dev, (N, C, P, Q), 20 + s)
    xa = x.clone().requires_grad_(True)
    y = GMMaxPool2d(k, s, pad)(xa)
    y.backward(dy)
    xr = x.float().contiguous().requires_grad_(True)       # NCHW: see the module docstring
    yr, _ = F.max_pool2d(xr, k, s, pad, return_indices=True)
    yr.backward(dy.float().contiguous())
    assert bool(torch.isnan(yr).any()) and bool((yr == float("-inf")).any())
    assert same_dev(y.detach().float(), yr.detach())
    want = xr.grad.to(BF16)                                # exact integer sums, rounded once
    assert bool((xr.grad != want.float()).any())           # the rounding is under test
    assert torch.equal(xa.grad, want)


def test_bn_relu_pool_second_trip(dev):
    """gm_bn_relu_maxpool2d_fwd_grouped_bf16 at (3, 1, 1), two groups of (2, 256, 129, 257), with
    power-of-two scales and integer shifts: x * sc + sh is exact, so the fused multiply-add cannot
    differ from the reference; y and the selected raw x against the reference's argmax."""
    from greedy_multimodal_learning_amd import _lib as L
    G, (N, C, H, W) = 2, BIG
    Ng = N // G
    k, s, pad = 3, 1, 1
    P, Q = E.pool_out(H, W, k, s, pad)
    assert N * P * Q * C // 8 > CAP
    x = big_input(dev, 31)
    gen = torch.Generator().manual_seed(32)
    sc, sh = X.pow2_coefficients(G, C, gen)
    coef = torch.stack([sc, sh], 1).contiguous().to(dev)   # [G, 2, C]: group g reads coef + g * 2C
    y = torch.empty(N, C, P, Q, device=dev, dtype=BF16, memory_format=CL)
    idx = torch.empty(N, P, Q, C, device=dev, dtype=torch.uint8)
    xsel = torch.empty(N, P, Q, C, device=dev, dtype=BF16)
    d = L.PoolDesc(Ng, H, W, C, k, s, pad)
    L.check(L.load().gm_bn_relu_maxpool2d_fwd_grouped_bf16(ctypes.byref(d), G, x.data_ptr(), coef.data_ptr(),
                                                           y.data_ptr(), idx.data_ptr(), xsel.data_ptr(),
                                                           L.stream_of(dev)), "gm_bn_relu_maxpool2d_fwd_grouped_bf16")
    xf = x.float()
    scn = sc.to(dev).repeat_interleave(Ng, 0).view(N, C, 1, 1)
    shn = sh.to(dev).repeat_interleave(Ng, 0).view(N, C, 1, 1)
    z = torch.relu(xf * scn + shn).contiguous()            # exact; relu keeps NaN, as the kernel's
    fin = torch.isfinite(z)
    assert torch.equal(z[fin], z[fin].to(BF16).float())    # and a bf16 value: the store is exact too
    assert bool((sc[0] != sc[1]).any())                    # the groups differ
    yr, ir = F.max_pool2d(z, k, s, pad, return_indices=True)
    del z
    assert bool(torch.isnan(yr).any())
    assert same_dev(y.float(), yr)
    want_sel = torch.gather(xf.reshape(N, C, H * W), 2, ir.reshape(N, C, P * Q)).view(N, C, P, Q)
    assert same_dev(xsel.permute(0, 3, 1, 2).float(), want_sel)
    # the stored argmax is that pixel, window-relative (row * k + column)
    pp = torch.arange(P, device=dev).view(1, 1, P, 1) * s - pad
    qq = torch.arange(Q, device=dev).view(1, 1, 1, Q) * s - pad
    rel = (ir // W - pp) * k + (ir % W - qq)
    assert torch.equal(idx.permute(0, 3, 1, 2).long(), rel)
