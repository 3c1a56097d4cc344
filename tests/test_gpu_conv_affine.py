"""The evaluation epilogue of the grouped bf16 forward convolution (vtrunk.vconv_affine over
gm_conv2d_fwd_grouped_affine_bf16): y = act(conv * sc + sh (+ residual)), one rounding.

Reference: on the bf16-rounded x and w, F.conv2d -> * sc + sh -> + residual -> ReLU in fp32
torch.  The bar is test_gpu_conv.py's: 1e-2 of the reference's max (every product is exact in
fp32; what differs is the fp32 summation order and the one bf16 rounding of the output, 2^-8).
Every shape runs G = 2 view groups with different weights and different coefficients; the
coefficients have both signs and magnitudes in [0.25, 4] (a negative sc catches a ReLU applied
before the affine), sh is the negative median of each channel's scaled output (about half the
outputs are clipped) and the residual is as large as the scaled output (it flips signs).

gm_bn_infer_coef: the same inputs through gm_bn_fwd_infer_bf16 and through an apply with the
table launch's coefficients are bit-identical."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

G = 2
# N, C, H, W, K, k, stride; the kernel the default plan picks
SHAPES = [
    ((3, 64, 56, 56, 64, 3, 1), "k_conv_rw"),
    ((2, 64, 9, 7, 64, 3, 1), "k_conv_rw, ragged tile"),
    ((2, 128, 14, 14, 128, 3, 1), "k_conv_h9"),
    ((3, 128, 13, 11, 128, 3, 1), "k_conv_h9, M not a multiple of 128"),
    ((3, 64, 20, 20, 128, 3, 2), "k_conv_igemm_ut, strided"),
    ((8, 512, 7, 7, 512, 3, 1), "split-K"),
    ((4, 64, 28, 28, 128, 1, 2), "1x1/s2: declined, the apply behind the plain forward"),
]
CASES = [(res, relu) for res in (True, False) for relu in (True, False)]
_IDS = ["x".join(map(str, s)) for s, _ in SHAPES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


_cache = {}


def _problem(shape, dev):
    """Inputs and the four fp32 references of a shape, made once and shared (never modified)."""
    if shape in _cache:
        return _cache[shape]
    N, C, H, W, K, k, st = shape
    pad = k // 2
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(G * N, C, H, W, generator=g).bfloat16()
    w = (torch.randn(G, K, C, k, k, generator=g) / (C * k * k) ** 0.5).bfloat16()
    # fp32 on the CPU from the bf16-rounded values (as test_gpu_conv.py)
    conv = torch.cat([F.conv2d(x[i * N:(i + 1) * N].float(), w[i].float(), stride=st, padding=pad) for i in range(G)])
    P, Q = conv.shape[2:]
    mag = 0.25 * 16 ** torch.rand(G, K, generator=g)          # [0.25, 4], log-uniform
    sc = mag * (torch.randint(0, 2, (G, K), generator=g) * 2 - 1)
    scaled = conv.view(G, N, K, P, Q) * sc.view(G, 1, K, 1, 1)
    sh = -scaled.permute(0, 2, 1, 3, 4).reshape(G, K, -1).median(dim=2).values   # about half clipped
    z = (scaled + sh.view(G, 1, K, 1, 1)).view(G * N, K, P, Q)
    res = (torch.randn(G * N, K, P, Q, generator=g) * float(z.std())).bfloat16()
    area = torch.zeros(G, 4 * K)
    area[:, 2 * K:3 * K] = sc
    area[:, 3 * K:] = sh
    area = area.to(dev)
    refs = {}
    for r, a in CASES:
        t = z + res.float() if r else z
        refs[(r, a)] = (torch.relu(t) if a else t).to(dev)
    res = res.to(dev)
    CL = torch.channels_last
    # the library's weight layout: [G][K][R][S][C]
    wb = w.to(dev).permute(0, 1, 3, 4, 2).contiguous()
    out = dict(x=x.to(dev).contiguous(memory_format=CL), wb=wb, area=area, res=res.contiguous(memory_format=CL),
               refs=refs, geom=(K, k, k, st, pad), N=N)
    _cache[shape] = out
    return out


def _run(p, res, relu):
    from greedy_multimodal_learning_amd import vtrunk
    K, R, S, st, pad = p["geom"]
    wb = p["wb"]
    return vtrunk.vconv_affine(p["x"], G, wb[0], wb[0].numel(), K, R, S, st, pad, p["area"],
                               p["res"] if res else None, relu)


def _check(y, ref, what):
    assert y.dtype == torch.bfloat16 and y.shape == ref.shape
    scale = float(ref.abs().max())
    err = float((y.float() - ref).abs().max())
    print(f"{what}: max err {err:.4g} of max {scale:.4g} ({err / scale:.3g}; bar 1e-2)")
    assert err <= 1e-2 * scale, what


def _desc(shape):
    from greedy_multimodal_learning_amd import _lib as L
    N, C, H, W, K, k, st = shape
    return L.ConvDescHW(N, H, W, C, K, k, k, st, st, k // 2, k // 2)


@pytest.mark.parametrize("shape,path", SHAPES, ids=_IDS)
def test_affine_epilogue_matches_fp32(dev, shape, path):
    from greedy_multimodal_learning_amd import _lib as L
    lib = L.load()
    p = _problem(shape, dev)
    N, C, H, W, K, k, st = shape
    ok = lib.gm_conv2d_fwd_affine_ok(ctypes.byref(_desc(shape)), G)
    assert ok == (0 if k == 1 else 1), path
    if path == "split-K":  # the plan really splits (as test_gpu_conv.py's turnstile test asks)
        d = L.ConvDesc(N, H, W, C, K, k, k, st, k // 2)
        assert lib.gm_conv2d_splitk_ws_bytes_grouped(ctypes.byref(d), G, 0) > 0
    for res, relu in CASES:
        y = _run(p, res, relu)
        ref = p["refs"][(res, relu)]
        if relu:  # the case really clips: about half the outputs
            frac = float((ref == 0).float().mean())
            assert 0.2 < frac < 0.8, (path, frac)
        _check(y, ref, f"{path} residual={res} relu={relu}")


@pytest.mark.parametrize("shape,path", SHAPES[:6], ids=_IDS[:6])
def test_affine_epilogue_on_the_other_kernels(dev, shape, path):
    """gm_conv_set_rw(0) / gm_conv_set_h9(0): the layer-1 and halo shapes on the lean kernel
    (k_conv_igemm_ut, split-K included), same bar."""
    from greedy_multimodal_learning_amd import _lib as L
    lib = L.load()
    p = _problem(shape, dev)
    try:
        L.check(lib.gm_conv_set_rw(0), "rw")
        L.check(lib.gm_conv_set_h9(0), "h9")
        assert lib.gm_conv2d_fwd_affine_ok(ctypes.byref(_desc(shape)), G) == 1
        for res, relu in CASES:
            _check(_run(p, res, relu), p["refs"][(res, relu)], f"{path} (rw 0, h9 0) residual={res} relu={relu}")
    finally:
        L.check(lib.gm_conv_set_rw(1), "rw")
        L.check(lib.gm_conv_set_h9(1), "h9")


@pytest.mark.parametrize("shape,path", [SHAPES[1], SHAPES[3], SHAPES[4], SHAPES[6]],
                         ids=[_IDS[1], _IDS[3], _IDS[4], _IDS[6]])
def test_nan_input_reaches_the_output_through_the_relu(dev, shape, path):
    """A NaN in x: every output whose window covers it is NaN with the ReLU on (relu_nan), every
    other output is what it was."""
    p = _problem(shape, dev)
    N, C, H, W, K, k, st = shape
    x = p["x"].clone(memory_format=torch.channels_last)
    b, c, h, w = N + 1, C // 2, H // 2, W // 2   # an image of the second view group
    x[b, c, h, w] = float("nan")
    q = dict(p, x=x)
    for res in (False, True):
        y = _run(q, res, True).float()
        clean = _run(p, res, True).float()
        hit = torch.zeros_like(y, dtype=torch.bool)
        pad = k // 2
        for ho in range(y.shape[2]):
            for wo in range(y.shape[3]):
                if abs(ho * st - h) <= pad and abs(wo * st - w) <= pad:
                    hit[b, :, ho, wo] = True
        assert hit.any()
        assert torch.isnan(y[hit]).all(), path
        assert torch.equal(y[~hit], clean[~hit]), path


@pytest.mark.parametrize("C", [64, 512])
def test_infer_coef_table_is_bit_identical_to_bn_fwd_infer(dev, C):
    """Two BatchNorms in one gm_bn_infer_coef launch; an apply with its coefficients against
    gm_bn_fwd_infer_bf16 on the same input: torch.equal."""
    from greedy_multimodal_learning_amd import _lib as L
    lib = L.load()
    st = L.stream_of(dev)
    g = torch.Generator().manual_seed(C)
    M = 3 * 5 * 7
    x = torch.randn(2, M, C, generator=g).bfloat16().to(dev)
    gamma = (torch.randn(2, C, generator=g) + torch.sign(torch.randn(2, C, generator=g))).to(dev)
    beta = torch.randn(2, C, generator=g).to(dev)
    rm = torch.randn(2, C, generator=g).to(dev)
    rv = (0.1 * 100 ** torch.rand(2, C, generator=g)).to(dev)   # [0.1, 10]
    assert (gamma > 0).any() and (gamma < 0).any() and float(rv.min()) >= 0.1 and float(rv.max()) <= 10
    eps = (1e-5, 1e-3)
    area = torch.zeros(2, 4 * C, device=dev)
    ents = [L.BnCoefEntry(gamma[i].data_ptr(), beta[i].data_ptr(), rm[i].data_ptr(), rv[i].data_ptr(),
                          area[i].data_ptr() + 8 * C, C, eps[i]) for i in range(2)]
    tab = torch.frombuffer(bytearray(bytes(L.arr(L.BnCoefEntry, ents))), dtype=torch.uint8).to(dev)
    L.check(lib.gm_bn_infer_coef(tab.data_ptr(), 2, C, st), "gm_bn_infer_coef")
    for relu in (0, 1):
        for i in range(2):
            want = torch.empty_like(x[i])
            need = lib.gm_bn_scratch(M, C)
            scratch = torch.zeros(max(need, 16), device=dev, dtype=torch.uint8)
            sm = torch.empty(2, C, device=dev)
            pw = L.BnFwd(M, C, relu, x[i].data_ptr(), 0, want.data_ptr(), gamma[i].data_ptr(), beta[i].data_ptr(),
                         rm[i].data_ptr(), rv[i].data_ptr(), 0.1, eps[i], sm[0].data_ptr(), sm[1].data_ptr(), 0, 0, 0)
            L.check(lib.gm_bn_fwd_infer_bf16(ctypes.byref(pw), scratch.data_ptr(), scratch.numel(), st), "infer")
            got = torch.empty_like(x[i])
            a = area[i].data_ptr()
            pg = L.BnFwd(M, C, relu, x[i].data_ptr(), 0, got.data_ptr(), a, a, 0, 0, 0.0, 0.0, a, a, 0, 0, 0)
            L.check(lib.gm_bn_fwd_apply_grouped_bf16(L.arr(L.BnFwd, [pg]), 1, a, 1, st), "apply")
            torch.cuda.synchronize()
            assert torch.equal(got, want), (C, relu, i)
    # and the coefficients are the formula's (fp64, rounded once)
    sc = gamma.double() / torch.sqrt(rv.double() + torch.tensor(eps, device=dev, dtype=torch.float64)[:, None])
    sh = beta.double() - rm.double() * sc
    assert torch.allclose(area[:, 2 * C:3 * C], sc.float(), rtol=1e-6, atol=0)
    assert torch.allclose(area[:, 3 * C:], sh.float(), rtol=1e-6, atol=1e-6)
