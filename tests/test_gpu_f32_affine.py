"""gm_conv2d_f32_affine / conv.conv_f32_affine: the fp32 forward convolution with the eval-mode
BatchNorm, the residual add and the ReLU in its epilogue, for the exact-f32 MFMA (terms 0) and
the split-bf16 contraction (terms 3 / 6).

The reference is the unfused composition of the same build: conv.conv_f32(FWD, terms) followed
by bn.bn_fwd_infer with the same residual and relu.  The epilogue applies k_bn_apply's three
operations to the same accumulator (or the same fixed-order split sum), so the bar is
torch.equal - no tolerance.  The shapes are the smallest that reach every kernel form on a
256-CU device (see SHAPES).  BatchNorm state is randomised (gamma of both signs, beta, running
mean, running variance in [0.5, 2]) so a swapped or missing term shows; the coefficients come
from gm_bn_infer_coef.  One test is independent of the project's code: PyTorch in float64 on
the CPU, with test_gpu_f32_trunk.py's rule err <= max(4 * err(fp32 PyTorch on the CPU), 1e-5)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CL = torch.channels_last
EPS = 1e-5
TERMS = (0, 3, 6)

# name: (N, H, W, C, K, R, S, stride, pad), residual, relu
SHAPES = {
    # scalar operand loads, unsplit, partial k-tile (Kr = 147)
    "stem": ((2, 32, 32, 3, 64, 7, 7, 2, 3), False, True),
    # 36 k-tiles over 2 tiles: a split reduction, the affine sum kernel
    "l1_3x3_split": ((2, 8, 8, 64, 64, 3, 3, 1, 1), True, True),
    # unsplit, 16-byte loads, partial M tile (M = 32)
    "ds_1x1": ((2, 8, 8, 64, 128, 1, 1, 2, 0), False, False),
    # strided, odd extent, split, M = 75
    "s2_3x3_odd": ((3, 9, 9, 64, 128, 3, 3, 2, 1), False, True),
    # M = 32768: 2x2 tiles in the exact kernel, the split kernel's 2x1 tile (N <= 64)
    "tiles_2x1": ((2, 128, 128, 8, 16, 3, 3, 1, 1), True, True),
    # 2x2 tiles in both kernels
    "tiles_2x2": ((2, 128, 128, 8, 128, 3, 3, 1, 1), True, False),
    # the stem at an evaluation batch's extent (M = 32768): scalar loads with 2x2 / 2x1 tiles
    "stem_2x2": ((2, 256, 256, 3, 64, 7, 7, 2, 3), False, True),
    # 36 splits of a 512-wide output, M = 18: the affine sum's grid stride (9 blocks of 256) is no
    # multiple of N, so its column index does step between a thread's elements
    "l4_wide": ((2, 3, 3, 512, 512, 3, 3, 1, 1), True, True),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


_cache = {}


def _data(name):
    """Host operands of one shape (drawn once, never modified): x, w (NCHW / KCRS logical shapes),
    the residual and the BatchNorm state (gamma, beta, running_mean, running_var)."""
    if name in _cache:
        return _cache[name]
    (N, H, W, C, K, R, S, st, pad), _, _ = SHAPES[name]
    g = torch.Generator().manual_seed(sum(SHAPES[name][0]) + len(name))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5
    P, Q = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    res = torch.randn(N, K, P, Q, generator=g)
    sign = torch.randint(0, 2, (K,), generator=g).float() * 2 - 1
    gamma = (0.5 + torch.rand(K, generator=g)) * sign
    beta = 0.3 * torch.randn(K, generator=g)
    rm = 0.3 * torch.randn(K, generator=g)
    rv = 0.5 * 4 ** torch.rand(K, generator=g)  # [0.5, 2]
    _cache[name] = (x, w, res, (gamma, beta, rm, rv))
    return _cache[name]


def _coef(dev, bn):
    """[2][K] coefficients of one BatchNorm by gm_bn_infer_coef."""
    from greedy_multimodal_learning_amd import _lib as L
    K = bn[0].shape[0]
    coef = torch.empty(2 * K, device=dev, dtype=torch.float32)
    ent = L.BnCoefEntry(bn[0].data_ptr(), bn[1].data_ptr(), bn[2].data_ptr(), bn[3].data_ptr(), coef.data_ptr(), K,
                        EPS)
    table = torch.frombuffer(bytearray(bytes(L.arr(L.BnCoefEntry, [ent]))), dtype=torch.uint8).to(dev)
    L.check(L.load().gm_bn_infer_coef(table.data_ptr(), 1, K, L.stream_of(dev)), "gm_bn_infer_coef")
    torch.cuda.synchronize()
    return coef


def _on_device(dev, name, x=None):
    x0, w, res, bn = _data(name)
    x = x0 if x is None else x
    return (x.to(dev).contiguous(memory_format=CL), w.to(dev).contiguous(memory_format=CL),
            res.to(dev).contiguous(memory_format=CL), tuple(t.to(dev) for t in bn))


def _out(dev, name):
    (N, H, W, C, K, R, S, st, pad), _, _ = SHAPES[name]
    P, Q = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    return torch.empty(N, K, P, Q, device=dev, dtype=torch.float32, memory_format=CL)


def _desc(name):
    from greedy_multimodal_learning_amd import conv as G
    return G._desc(*SHAPES[name][0])


def _unfused(dev, name, terms, xd, wd, resd, bnd, residual, relu):
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import bn as B
    from greedy_multimodal_learning_amd import conv as G
    y = G.conv_f32(L.GM_CONV_FWD, _desc(name), x=xd, w=wd, out=_out(dev, name), terms=terms)
    return y, B.bn_fwd_infer(y, bnd[0], bnd[1], bnd[2], bnd[3], EPS, relu, resd if residual else None)


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_bit_identical_to_conv_then_batchnorm(dev, name, terms):
    from greedy_multimodal_learning_amd import conv as G
    _, residual, relu = SHAPES[name]
    xd, wd, resd, bnd = _on_device(dev, name)
    coef = _coef(dev, bnd)
    _, ref = _unfused(dev, name, terms, xd, wd, resd, bnd, residual, relu)
    out = G.conv_f32_affine(_desc(name), xd, wd, _out(dev, name).fill_(float("nan")), coef,
                            residual=resd if residual else None, relu=relu, terms=terms)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.1
    if relu:
        assert 0.05 < float((ref == 0).float().mean()) < 0.95  # the ReLU does cut
    assert torch.equal(out, ref)


@pytest.mark.parametrize("terms", TERMS)
def test_residual_may_be_the_output_buffer(dev, terms):
    from greedy_multimodal_learning_amd import conv as G
    name = "l1_3x3_split"
    xd, wd, resd, bnd = _on_device(dev, name)
    coef = _coef(dev, bnd)
    _, ref = _unfused(dev, name, terms, xd, wd, resd, bnd, True, True)
    buf = resd.clone(memory_format=torch.preserve_format)
    out = G.conv_f32_affine(_desc(name), xd, wd, buf, coef, residual=buf, relu=True, terms=terms)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(out, ref)


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("name", ["stem", "l1_3x3_split", "ds_1x1"])
def test_identity_epilogue_is_the_plain_convolution(dev, name, terms):
    """sc = 1, sh = 0, no residual, no ReLU: the accumulator and the split sum on their own."""
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import conv as G
    xd, wd, _, _ = _on_device(dev, name)
    K = SHAPES[name][0][4]
    coef = torch.cat([torch.ones(K), torch.zeros(K)]).to(dev)
    ref = G.conv_f32(L.GM_CONV_FWD, _desc(name), x=xd, w=wd, out=_out(dev, name), terms=terms)
    out = G.conv_f32_affine(_desc(name), xd, wd, _out(dev, name).fill_(float("nan")), coef, terms=terms)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("terms", TERMS)
def test_nan_propagates_as_in_the_composition(dev, terms):
    from greedy_multimodal_learning_amd import conv as G
    name = "l1_3x3_split"
    x = _data(name)[0].clone()
    x[1, 17, 3, 4] = float("nan")
    xd, wd, resd, bnd = _on_device(dev, name, x)
    coef = _coef(dev, bnd)
    _, ref = _unfused(dev, name, terms, xd, wd, resd, bnd, True, True)
    out = G.conv_f32_affine(_desc(name), xd, wd, _out(dev, name), coef, residual=resd, relu=True, terms=terms)
    nan_ref, nan_out = torch.isnan(ref), torch.isnan(out)
    assert 0 < int(nan_ref.sum()) < ref.numel()  # the ReLU did not hide it, and it stays local
    assert torch.equal(nan_ref, nan_out)
    assert torch.equal(out[~nan_out], ref[~nan_ref])


def _err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / float(b.abs().max())


def _torch_cpu(name, dtype):
    (N, H, W, C, K, R, S, st, pad), residual, relu = SHAPES[name]
    x, w, res, bn = (_data(name)[i] for i in range(4))
    c = lambda t: t.to(dtype)  # noqa: E731
    y = F.conv2d(c(x), c(w), stride=st, padding=pad)
    y = F.batch_norm(y, c(bn[2]), c(bn[3]), c(bn[0]), c(bn[1]), training=False, eps=EPS)
    if residual:
        y = y + c(res)
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("terms", [0, 6])
@pytest.mark.parametrize("name", ["l1_3x3_split", "stem"])
def test_against_float64_pytorch_on_the_cpu(dev, name, terms):
    from greedy_multimodal_learning_amd import conv as G
    _, residual, relu = SHAPES[name]
    xd, wd, resd, bnd = _on_device(dev, name)
    out = G.conv_f32_affine(_desc(name), xd, wd, _out(dev, name), _coef(dev, bnd),
                            residual=resd if residual else None, relu=relu, terms=terms)
    ref64 = _torch_cpu(name, torch.float64)
    e, e32 = _err(out, ref64), _err(_torch_cpu(name, torch.float32), ref64)
    print(f"{name} terms {terms}: fused {e:.3e}, fp32 PyTorch on the CPU {e32:.3e}")
    assert e <= max(4 * e32, 1e-5)


@pytest.mark.parametrize("mode,terms", [(1, 0), (2, 6), (0, 4)])
def test_refusals_launch_nothing(dev, mode, terms):
    from greedy_multimodal_learning_amd import _lib as L
    name = "l1_3x3_split"
    xd, wd, _, bnd = _on_device(dev, name)
    coef = _coef(dev, bnd)
    out = _out(dev, name).fill_(7.0)
    scratch = torch.empty(1 << 20, device=dev, dtype=torch.uint8)
    p = L.ConvF32(mode, _desc(name), xd.data_ptr(), wd.data_ptr(), xd.data_ptr(), out.data_ptr(), 0, 0, 0)
    with pytest.raises(L.GreedyMMLError, match="mode" if mode else "terms"):
        L.check(L.load().gm_conv2d_f32_affine(ctypes.byref(p), terms, coef.data_ptr(), 0, 1, scratch.data_ptr(),
                                              scratch.numel(), L.stream_of(dev)), "gm_conv2d_f32_affine")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    if not mode:  # the Python entry passes the refusal on
        from greedy_multimodal_learning_amd import conv as G
        with pytest.raises(L.GreedyMMLError, match="terms"):
            G.conv_f32_affine(_desc(name), xd, wd, out, coef, terms=terms)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
