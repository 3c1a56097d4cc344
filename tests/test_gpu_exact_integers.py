"""The bf16 convolution, weight-gradient and GEMM kernels pinned bit for bit with integer operands.

Every other test of these kernels compares against fp32 PyTorch on randn inputs at 1e-2 of the
tensor's max (2e-3 for the fp32 weight gradient); that bar cannot see a truncating store, a second
rounding in an epilogue, a bf16 split-K hand-off or one missing (channel, tap) product.  With
small integer operands (exactint.py) every partial sum is an integer below 2^24, the fp32
accumulation is exact in any order, and the only inexact step left is the ONE bf16 rounding of the
output: a correct kernel equals the exact reference rounded once, torch.equal.  The fp32 outputs
(weight gradients, the fp32 trunk, gm_gemm_f32) equal the exact reference itself.

Before a case touches the GPU its reference is checked on the CPU: the 2^24 bound (validity), fp32
== fp64 at the smallest shape of each family, and - for the rounding cases - that a truncating
store, a double rounding and a bf16 half-K partial each change >= 1 % of the expected elements
(non-vacuity; exactint.assert_discriminates).  Which kernel a row reaches is established as the
neighbouring tests do: the knob that forces it, a size query, or the grad_fn.

Statistics (section 7 of the module): with ternary operands y is an exact bf16 integer and the
sums are exact fp32 integers under any partition; the finalize is fp64, so running_mean /
running_var (momentum 1) may differ from the float64 batch statistics by the final rounding to
fp32 and a couple of fp32 operations of the blend: the bar is 8 fp32 ulps = 2^-21 = 4.77e-7
relative.  Observed on the MI355X, epilogue path and single-launch BatchNorm alike (max over the
channels, both view groups, mean and variance): k_conv_rw 5.40e-8, k_conv_h9 5.66e-8, strided lean
5.71e-8 and 5.67e-8 (64 x 64 tiles), split-K 5.82e-8, k_gemm_ring 5.33e-8 - the final rounding
to fp32 alone (2^-24 = 5.96e-8).

Measured on the CPU references (printed by the cases): at (8,512,7,7,512,3,3,1,1) with |x| <= 4,
|w| <= 2, 13.0 % of the outputs are not bf16 numbers, 11.7 % are exact ties, truncation != RNE on
6.4 %, a bf16 half-K partial changes 3.4 %; at (8,256,14,14,512,3,3,2,1) 6.3 % / 6.2 % / 3.1 % /
1.1 % (its input gradient, |dy| <= 8: 12.2 % / 10.7 % / 6.1 % / 3.2 %); double != single rounding
on 7.6-20.5 % of the fused-addend cases and 6.6-19.5 % of the evaluation-epilogue cases.
"""
import ctypes
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

import exactint as E

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
WGRAD_LOOP_DEFAULT = 22   # gm_conv_set_wgrad_loop's default (conv_wgrad_plan.h WgradKnobs::loop)
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


_DEFAULTS = dict(rw=1, h9=1, halo=1, stem=1, gemm1x1=2, wgrad_loop=WGRAD_LOOP_DEFAULT, wgrad_staging=2,
                 wgrad_stem=1)
_SETTERS = dict(rw="gm_conv_set_rw", h9="gm_conv_set_h9", halo="gm_conv_set_halo", stem="gm_conv_set_stem",
                gemm1x1="gm_conv_set_1x1_gemm", wgrad_loop="gm_conv_set_wgrad_loop",
                wgrad_staging="gm_conv_set_wgrad_staging", wgrad_stem="gm_conv_set_wgrad_stem")


@contextmanager
def knobs(**kw):
    """Set planner switches for the block; every one is back at its default afterwards."""
    from greedy_multimodal_learning_amd import _lib as L
    lib = L.load()
    try:
        for k, v in kw.items():
            L.check(getattr(lib, _SETTERS[k])(v), _SETTERS[k])
        yield
    finally:
        for k in kw:
            getattr(lib, _SETTERS[k])(_DEFAULTS[k])


def _cl(t, dev, dtype=BF):
    return t.to(dtype).to(dev).contiguous(memory_format=CL)


def _eq(got, want_bf16_valued, what):
    """got (bf16, device) == the expected bf16 values (an fp32 CPU tensor holding bf16 numbers)."""
    g = got.detach().float().cpu()
    assert g.shape == want_bf16_valued.shape, what
    bad = g != want_bf16_valued
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, max |diff| "
                                 f"{float((g - want_bf16_valued).abs().max())}")


# ---- 2. forward and input gradient on every planned kernel form --------------------------------
# (shape (N,C,H,W,K,R,S,stride,pad), knobs, operand magnitudes, what the row reaches and how that is known)
# Magnitudes (max |x|, max |w|[, max |dy|]): E.WIDE on the split-K rows, as the issue sets; wider on the shorter
# reductions (M8 below 2304 products, M16 on the 1x1 rows) so that on EVERY row at least 1 % of y and of dx are
# not bf16 numbers (asserted in conv_case): each row pins the store's rounding, not the products alone.
# The unsplit 128x128 lean tiles: pick_tile (conv_plan.h) takes them once Nout >= 128 and
# pixels / 128 * (Nout / 128) >= kTileBias / 4 = 256, i.e. from 32768 output pixels at Nout = 128; 3x3 / s1 with
# C = 64 keeps the forward off the halo kernels (C >= 128) and off k_conv_rw (Nout = 64), and
# gm_conv2d_splitk_ws_bytes == 0 says the tiles are not split.  Its input gradient contracts over 128 channels on
# a 3x3 / s1 same-size grid, so it is a halo shape: k_conv_h9 with BN = 64.
# The lean 128x64 tiles: small_tile takes them from pixels / 128 * ceil(Nout / 64) >= 768, i.e. 98304 pixels at
# Nout = 64 (below 128 output channels neither 128x128 nor split-K applies); gm_conv_set_rw(0) keeps the layer-1
# shape off k_conv_rw.  Forward and input gradient are the same problem there (C = K = 64).
M8, M16 = (8, 4), (16, 8)
FWD_ROWS = [
    ((2, 64, 9, 7, 64, 3, 3, 1, 1), {}, M8, "k_conv_rw ragged tile (default plan)"),
    ((3, 64, 20, 20, 64, 3, 3, 1, 1), {}, M8, "k_conv_rw (default plan)"),
    ((2, 64, 9, 7, 64, 3, 3, 1, 1), dict(rw=0), M8, "layer-1 shape on the lean kernel, 64x64 (gm_conv_set_rw(0))"),
    ((3, 64, 20, 20, 64, 3, 3, 1, 1), dict(rw=0), M8, "layer-1 shape on the lean kernel, 64x64 (gm_conv_set_rw(0))"),
    ((32, 64, 56, 56, 64, 3, 3, 1, 1), dict(rw=0), M8,
     "lean 128x64 tiles (gm_conv_set_rw(0); small_tile: 100352 pixels >= 98304)"),
    ((3, 128, 13, 11, 128, 3, 3, 1, 1), {}, M8, "k_conv_h9, M not a multiple of 128 (default plan)"),
    ((3, 128, 13, 11, 128, 3, 3, 1, 1), dict(h9=0), M8, "k_conv_halo<128> (gm_conv_set_h9(0))"),
    ((3, 128, 9, 11, 256, 3, 3, 1, 1), dict(halo=2), M8, "gm_conv_set_halo(2); below 192 tiles the plan keeps "
                                                           "the 128-pixel form"),
    ((32, 128, 28, 28, 256, 3, 3, 1, 1), dict(halo=2), M8,
     "k_conv_halo<256>: halo256_plan takes 196 >= 192 tiles of 256 x 128 (forward; the input gradient, 98 tiles, "
     "keeps the 128-pixel form); no size query tells the forms apart"),
    ((2, 64, 9, 11, 128, 3, 3, 2, 1), {}, M8 + (16,), "lean 64x64 tiles, strided (small_tile)"),
    ((3, 64, 20, 20, 128, 3, 3, 2, 1), {}, M8 + (16,), "lean 64x64 tiles, strided"),
    ((5, 128, 7, 7, 256, 1, 1, 2, 0), {}, M16,
     "1x1/s2 on the lean kernel (this entry routes only 1x1/s1 to k_gemm_ring): one parity class, the pixels it "
     "does not cover zeroed"),
    ((8, 64, 64, 64, 128, 3, 3, 1, 1), {}, M8,
     "forward: lean unsplit 128x128 tiles (pick_tile: 32768 pixels; ws_bytes == 0); input gradient: k_conv_h9"),
    ((8, 512, 7, 7, 512, 3, 3, 1, 1), {}, E.WIDE, "split-K turnstile (ws_bytes > 0), rounding case"),
    ((8, 256, 14, 14, 512, 3, 3, 2, 1), {}, E.WIDE + (8,), "split-K turnstile, strided (ws_bytes > 0), rounding case; "
     "|dy| <= 8: the input gradient's parity classes sum 1-4 taps only"),
    ((4, 256, 14, 14, 64, 1, 1, 1, 0), {}, M16, "1x1/s1 on k_gemm_ring (route_1x1), ragged M"),
    ((4, 64, 28, 28, 256, 1, 1, 1, 0), {}, M16, "1x1/s1 on k_gemm_ring (route_1x1)"),
]
SPLITK = {(8, 512, 7, 7, 512, 3, 3, 1, 1), (8, 256, 14, 14, 512, 3, 3, 2, 1)}
UNSPLIT_128 = (8, 64, 64, 64, 128, 3, 3, 1, 1)

_conv_cache = {}


def conv_case(shape, mags=E.WIDE, rounding=False, check64=False):
    """Operands and the exact fp32 CPU references of a shape, made once and never modified; the
    validity and (rounding=True) non-vacuity conditions asserted on the reference."""
    key = (shape, mags, rounding)
    if key in _conv_cache:
        return _conv_cache[key]
    N, C, H, W, K, R, S, st, pad = shape
    x, w, dy = E.conv_operands(shape, mags[:2], mag_dy=mags[2] if len(mags) > 2 else None)
    if check64:
        E.assert_fp32_is_exact(x, w, dy, st, pad)
    ref = E.conv_refs(x, w, dy, st, pad, want=("y", "dx"))
    case = dict(x=x, w=w, dy=dy, y=ref["y"], dx=ref["dx"])
    case["census"] = dict(y=E.bf16_census(ref["y"]), dx=E.bf16_census(ref["dx"]))
    for k, cen in case["census"].items():   # every row pins the store's rounding
        assert cen["inexact"] >= 0.01 and cen["trunc_ne_rne"] >= 0.005, (shape, k, cen)
    if rounding:
        h = C // 2   # the half-K partial a split hands on: the first half of the channels
        half_y = F.conv2d(x[:, :h], w[:, :h], stride=st, padding=pad)
        hk = K // 2
        half_dx = torch.nn.grad.conv2d_input(x.shape, w[:hk], dy[:, :hk], stride=st, padding=pad)
        case["fractions"] = dict(y=E.assert_discriminates(ref["y"], half=half_y, what=f"{_ids(shape)} y"),
                                 dx=E.assert_discriminates(ref["dx"], half=half_dx, what=f"{_ids(shape)} dx"))
        print(f"{_ids(shape)}: census {case['census']} wrong-reference fractions {case['fractions']}")
    _conv_cache[key] = case
    return case


@pytest.mark.parametrize("shape,kn,mags,path", FWD_ROWS,
                         ids=[f"{_ids(r[0])}-{'_'.join(r[1]) or 'default'}" for r in FWD_ROWS])
def test_fwd_dgrad_bit_exact(dev, shape, kn, mags, path):
    """y == bf16(exact conv) and dx == bf16(exact input gradient), torch.equal, on every row."""
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import conv as G
    N, C, H, W, K, R, S, st, pad = shape
    c = conv_case(shape, mags, rounding=shape in SPLITK, check64=shape == FWD_ROWS[0][0])
    lib = L.load()
    d = G._desc(N, H, W, C, K, R, S, st, pad)
    with knobs(**kn):
        nb = [lib.gm_conv2d_splitk_ws_bytes(ctypes.byref(d), dgrad) for dgrad in (0, 1)]
        if shape in SPLITK:   # the forward splits; the 3x3/s1 input gradient too (the strided one's parity
            assert nb[0] > 0, path   # classes have too few k-tiles to split)
            assert nb[1] > 0 or st == 2, path
        if shape == UNSPLIT_128:
            assert nb == [0, 0], path
        xd, wd, dyd = _cl(c["x"], dev), _cl(c["w"], dev), _cl(c["dy"], dev)
        y = G.conv_fwd(xd, wd, st, pad)
        dx = G.conv_dgrad(dyd, wd, H, W, st, pad)
        torch.cuda.synchronize()
        assert L.device_faults(clear=True) == 0
    _eq(y, E.rne(c["y"]), f"y, {path}")
    _eq(dx, E.rne(c["dx"]), f"dx, {path}")


GROUPED_1X1 = [  # shape, (gm_conv_set_1x1_gemm mode on k_gemm_ring, the mode on the im2col kernel)
    ((4, 256, 14, 14, 64, 1, 1, 1, 0), (1, 0)),    # ragged M
    ((4, 64, 28, 28, 256, 1, 1, 1, 0), (1, 0)),
    ((5, 128, 7, 7, 256, 1, 1, 2, 0), (2, 1)),     # the downsample: rows gathered (forward) / scattered (dgrad)
    ((1, 64, 15, 13, 128, 1, 1, 2, 0), (2, 1)),    # odd map, 15 x 13 -> 8 x 7
]


@pytest.mark.parametrize("ring", [True, False], ids=["k_gemm_ring", "im2col"])
@pytest.mark.parametrize("shape,modes", GROUPED_1X1, ids=[_ids(r[0]) for r in GROUPED_1X1])
def test_grouped_1x1_fwd_dgrad_bit_exact(dev, shape, modes, ring):
    """The view-grouped entries' 1x1 routing (k_gemm_ring: plain NT GEMM at stride 1, gathered A rows / scattered
    output rows at stride 2; gm_conv2d_fwd_affine_ok == 0 says the route is taken) and the im2col kernel under the
    other gm_conv_set_1x1_gemm mode, two view groups: y, dx == the exact result rounded once; the pixels a
    stride-2 input gradient does not cover are zero."""
    from greedy_multimodal_learning_amd import _lib as L
    lib = L.load()
    N, C, H, W, K, R, S, st, pad = shape
    G = 2
    mags = (16, 8)   # 64-256 products: wider operands so that outputs pass 256
    cs = [E.conv_operands(shape, mags, seed=i) for i in range(G)]
    refs = [E.conv_refs(x, w, dy, st, pad, want=("y", "dx")) for x, w, dy in cs]
    assert E.bf16_census(refs[0]["y"])["inexact"] > 0.01
    P, Q = E.out_hw(H, W, R, S, st, pad)
    x = torch.cat([c[0] for c in cs]).permute(0, 2, 3, 1).contiguous().to(BF).to(dev)
    dy = torch.cat([c[2] for c in cs]).permute(0, 2, 3, 1).contiguous().to(BF).to(dev)
    w = torch.stack([c[1].reshape(K, C) for c in cs]).to(BF).to(dev)     # [G][K][C]
    wt = w.transpose(1, 2).contiguous()                                   # [G][C][K]
    dh = L.ConvDescHW(N, H, W, C, K, 1, 1, st, st, 0, 0)
    dd = L.ConvDesc(N, H, W, C, K, 1, 1, st, 0)
    stt = L.stream_of(dev)
    with knobs(gemm1x1=modes[0 if ring else 1]):
        if ring:
            assert lib.gm_conv2d_fwd_affine_ok(ctypes.byref(dh), G) == 0
        y = torch.full((G * N, P, Q, K), 7.0, device=dev, dtype=BF)
        L.check(lib.gm_conv2d_fwd_grouped_bf16(ctypes.byref(dh), G, x.data_ptr(), w.data_ptr(), K * C, y.data_ptr(),
                                               0, 0, stt), "fwd")
        dx = torch.full((G * N, H, W, C), 7.0, device=dev, dtype=BF)
        L.check(lib.gm_conv2d_dgrad_grouped_bf16(ctypes.byref(dd), G, dy.data_ptr(), wt.data_ptr(), C * K,
                                                 dx.data_ptr(), 0, 0, 0, stt), "dgrad")
        torch.cuda.synchronize()
    _eq(y, E.rne(torch.cat([r["y"] for r in refs]).permute(0, 2, 3, 1)), "y")
    _eq(dx, E.rne(torch.cat([r["dx"] for r in refs]).permute(0, 2, 3, 1)), "dx")


STEM_SHAPES = [(3, 3, 37, 30, 64, 7, 7, 2, 3), (2, 4, 16, 18, 32, 5, 5, 2, 2)]


@pytest.mark.parametrize("stem", [1, 0], ids=["pair_stem", "im2col_fallback"])
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_ids)
def test_stem_bit_exact(dev, shape, stem):
    """The pixel-pair stem (the "Stem" grad_fn; k_conv_stem where it takes the shape, the im2col kernel
    under gm_conv_set_stem(0)): y == bf16(exact conv); its fp32 weight gradient == the exact one."""
    from greedy_multimodal_learning_amd.conv import GMConv2d
    N, C, H, W, K, R, S, st, pad = shape
    mags = (8, 8)   # 147 / 100 products: wider operands so that outputs pass 256
    x, w, dy = E.conv_operands(shape, mags)
    if shape == STEM_SHAPES[1]:
        E.assert_fp32_is_exact(x, w, dy, st, pad)
    ref = E.conv_refs(x, w, dy, st, pad, want=("y", "dw"))
    assert E.bf16_census(ref["y"])["inexact"] > 0.01
    m = GMConv2d(C, K, (R, S), stride=st, padding=pad, bias=False).to(dev)
    with torch.no_grad():
        m.weight.copy_(w)
    m = m.to(memory_format=CL)
    assert m.uses_pair_stem()
    with knobs(stem=stem):
        y = m(_cl(x, dev))
        assert y.grad_fn is not None and "Stem" in type(y.grad_fn).__name__
        y.backward(_cl(dy, dev))
        torch.cuda.synchronize()
    _eq(y, E.rne(ref["y"]), "stem y")
    assert m.weight.grad.dtype == torch.float32
    assert torch.equal(m.weight.grad.cpu(), ref["dw"]), "stem dw"


# ---- 3. fused input-gradient epilogues -----------------------------------------------------------
# dx = bf16(dgrad + addend), ONE rounding.  Magnitudes per row so that the contraction alone passes 256 often
# (the double rounding must differ in >= 1 % of the elements: asserted on the reference).
ADDEND_ROWS = [  # shape, (max |dy|, max |w|), max |addend|
    ((3, 64, 20, 20, 64, 3, 3, 1, 1), (8, 4), 300),      # k_conv_rw
    ((3, 128, 13, 11, 128, 3, 3, 1, 1), (8, 4), 300),    # k_conv_h9
    ((3, 64, 20, 20, 128, 3, 3, 2, 1), (16, 8), 300),    # strided: parity classes of 1-4 taps
    ((5, 128, 7, 7, 256, 1, 1, 2, 0), (16, 8), 300),     # 1x1/s2: the uncovered pixels take the addend
    ((8, 512, 7, 7, 512, 3, 3, 1, 1), E.WIDE, 300),      # split-K
]


def _addend_case(shape, mags, amag, seed=1):
    """dy, w, the integer addend and the exact dgrad (+ addend) of one view group, made once; the
    double rounding asserted to differ on the pixels the dgrad covers."""
    key = ("add", shape, seed)
    if key in _conv_cache:
        return _conv_cache[key]
    N, C, H, W, K, R, S, st, pad = shape
    x, w, dy = E.conv_operands(shape, (mags[0], mags[1]), seed=seed)
    g = torch.Generator().manual_seed(seed + 7 + sum(shape))
    add = E.rne(E.ints((N, C, H, W), amag, g))   # a bf16 tensor on the device: integers bf16 holds
    E.assert_exact_bound(K * R * S + 1, max(mags[0], amag), mags[1])
    dgrad = torch.nn.grad.conv2d_input(x.shape, w, dy, stride=st, padding=pad)
    total = dgrad + add
    step = st if R == 1 else 1   # a 1x1/s2 input gradient covers the even pixels only
    fr = E.assert_discriminates(total[:, :, ::step, ::step], addend=add[:, :, ::step, ::step],
                                what=f"{_ids(shape)} dx + addend")
    print(f"{_ids(shape)} addend (seed {seed}): census {E.bf16_census(total)} wrong-reference fractions {fr}")
    _conv_cache[key] = dict(w=w, dy=dy, add=add, dgrad=dgrad, total=total, fractions=fr)
    return _conv_cache[key]


@pytest.mark.parametrize("shape,mags,amag", ADDEND_ROWS, ids=[_ids(r[0]) for r in ADDEND_ROWS])
def test_dgrad_plain_addend_one_rounding(dev, shape, mags, amag):
    """conv_dgrad_t(addend=, inplace=): dx == bf16(exact dgrad + addend), out of place and in place."""
    from greedy_multimodal_learning_amd import conv as G
    N, C, H, W, K, R, S, st, pad = shape
    c = _addend_case(shape, mags, amag)
    wt = _cl(c["w"].permute(1, 0, 2, 3), dev)
    dyd, add = _cl(c["dy"], dev), _cl(c["add"], dev)
    want = E.rne(c["total"])
    _eq(G.conv_dgrad_t(dyd, wt, H, W, st, pad, addend=add), want, "dx + addend")
    buf = add.clone(memory_format=torch.preserve_format)
    out = G.conv_dgrad_t(dyd, wt, H, W, st, pad, addend=buf, inplace=True)
    assert out.data_ptr() == buf.data_ptr()
    _eq(out, want, "dx + addend in place")
    _eq(G.conv_dgrad_t(dyd, wt, H, W, st, pad), E.rne(c["dgrad"]), "dx")


MASKED_ROWS = ADDEND_ROWS + [((4, 256, 14, 14, 64, 1, 1, 1, 0), (16, 8), 300)]   # + k_gemm_ring 1x1/s1


@pytest.mark.parametrize("shape,mags,amag", MASKED_ROWS, ids=[_ids(r[0]) for r in MASKED_ROWS])
def test_dgrad_masked_addend_one_rounding(dev, shape, mags, amag):
    """gm_conv2d_dgrad_grouped_masked_bf16 over two view groups: dx == bf16(exact dgrad + (mask bit ?
    addend : 0)), one rounding, per element; and the grouped plain-addend entry alike."""
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import vtrunk
    lib = L.load()
    N, C, H, W, K, R, S, st, pad = shape
    G = 2
    P, Q = E.out_hw(H, W, R, S, st, pad)
    cs = [_addend_case(shape, mags, amag), _addend_case(shape, mags, amag, seed=2)]
    dy = torch.cat([c["dy"] for c in cs]).permute(0, 2, 3, 1).contiguous().to(BF).to(dev)        # [G*N,P,Q,K]
    add = torch.cat([c["add"] for c in cs]).permute(0, 2, 3, 1).contiguous()                      # [G*N,H,W,C]
    wt = torch.stack([c["w"].permute(1, 2, 3, 0) for c in cs]).contiguous().to(BF).to(dev)        # [G][C][R][S][K]
    gm = torch.Generator().manual_seed(sum(shape))
    mask = torch.randint(0, 256, (add.numel() // 8,), generator=gm, dtype=torch.uint8)
    bits = ((mask.to(torch.int32)[:, None] >> torch.arange(8)) & 1).reshape(add.shape).bool()
    dgrad = torch.cat([c["dgrad"] for c in cs]).permute(0, 2, 3, 1)
    want_m = E.rne(dgrad + torch.where(bits, add, torch.zeros(())))
    want_p = E.rne(dgrad + add)
    assert E.frac_ne(want_m, want_p) > 0.1   # the mask does decide
    d = L.ConvDesc(N, H, W, C, K, R, S, st, pad)
    ws, nb = vtrunk._splitk_g(dev, d, G, True)
    stt = L.stream_of(dev)
    addd, maskd = add.to(BF).to(dev), mask.to(dev)
    dxm = torch.full((G * N, H, W, C), 7.0, device=dev, dtype=BF)
    L.check(lib.gm_conv2d_dgrad_grouped_masked_bf16(ctypes.byref(d), G, dy.data_ptr(), wt.data_ptr(), wt[0].numel(),
                                                    dxm.data_ptr(), addd.data_ptr(), maskd.data_ptr(), ws, nb, stt),
            "dgrad masked")
    dxp = torch.full((G * N, H, W, C), 7.0, device=dev, dtype=BF)
    L.check(lib.gm_conv2d_dgrad_grouped_bf16(ctypes.byref(d), G, dy.data_ptr(), wt.data_ptr(), wt[0].numel(),
                                             dxp.data_ptr(), addd.data_ptr(), ws, nb, stt), "dgrad + addend")
    torch.cuda.synchronize()
    assert L.device_faults(clear=True) == 0
    _eq(dxm, want_m, "masked addend")
    _eq(dxp, want_p, "grouped plain addend")


# ---- 4. the evaluation epilogue (vtrunk.vconv_affine, G = 2) -------------------------------------
AFFINE_SHAPES = [  # N, C, H, W, K, k, stride (test_gpu_conv_affine.py's), operand magnitudes
    ((3, 64, 56, 56, 64, 3, 1), (8, 4)), ((2, 64, 9, 7, 64, 3, 1), (8, 4)), ((2, 128, 14, 14, 128, 3, 1), (8, 4)),
    ((3, 128, 13, 11, 128, 3, 1), (8, 4)), ((3, 64, 20, 20, 128, 3, 2), (8, 4)), ((8, 512, 7, 7, 512, 3, 1), E.WIDE),
    ((4, 64, 28, 28, 128, 1, 2), (16, 16)),   # declined: 64 products, wider operands so the conv alone passes 256
]
AFF_CASES = [(res, relu) for res in (True, False) for relu in (True, False)]
_aff_cache = {}


def _affine_case(shape, mags, dev):
    key = (shape, str(dev))   # (the CPU-side conditions are also run without a device: test_cpu_exactint.py)
    if key in _aff_cache:
        return _aff_cache[key]
    G = 2
    N, C, H, W, K, k, st = shape
    pad = k // 2
    E.assert_exact_bound(C * k * k, mags[0], mags[1], 4)   # acc * sc (|sc| <= 4), then + sh + residual below
    g = torch.Generator().manual_seed(sum(shape))
    x = E.ints((G * N, C, H, W), mags[0], g)
    w = E.ints((G, K, C, k, k), mags[1], g)
    conv = torch.cat([F.conv2d(x[i * N:(i + 1) * N], w[i], stride=st, padding=pad) for i in range(G)])
    P, Q = conv.shape[2:]
    sc, sh = E.pow2_coefficients(G, K, g)
    res = E.rne(E.ints((G * N, K, P, Q), 200, g))
    assert float(conv.abs().max()) * 4 + 8 + 200 < E.LIMIT / 4   # multiples of 1/4 below 2^22: exact in fp32
    scv = sc.view(G, 1, K, 1, 1).double()
    shv = sh.view(G, 1, K, 1, 1).double()
    z = (conv.double().view(G, N, K, P, Q) * scv + shv).view(G * N, K, P, Q)
    assert torch.equal(z.float().double(), z)   # the affine result is an fp32 number
    one, two = {}, {}
    for r, a in AFF_CASES:
        t = z + res.double() if r else z
        one[(r, a)] = E.rne(torch.relu(t) if a else t)
        # the declined path's contract: the plain forward stores bf16(conv), the apply rounds again
        c16 = E.rne(conv).double().view(G, N, K, P, Q)
        t2 = (c16 * scv + shv).view(G * N, K, P, Q)
        t2 = t2 + res.double() if r else t2
        two[(r, a)] = E.rne(torch.relu(t2) if a else t2)
    frac = E.frac_ne(one[(True, False)], two[(True, False)])
    cen = E.bf16_census((z + res.double()).float())
    print(f"affine {_ids(shape)}: census {cen} double != single rounding {frac:.4f}")
    assert frac >= 0.01, frac   # one rounding and two are told apart (|x| <= 8, |w| <= 4 below 512 channels)
    assert cen["trunc_ne_rne"] >= 0.01
    area = torch.zeros(G, 4 * K)
    area[:, 2 * K:3 * K] = sc
    area[:, 3 * K:] = sh
    out = dict(x=_cl(x, dev), wb=w.permute(0, 1, 3, 4, 2).contiguous().to(BF).to(dev), area=area.to(dev),
               res=_cl(res, dev), one=one, two=two, geom=(K, k, k, st, pad))
    _aff_cache[key] = out
    return out


def _affine_run(p, res, relu):
    from greedy_multimodal_learning_amd import vtrunk
    K, R, S, st, pad = p["geom"]
    wb = p["wb"]
    return vtrunk.vconv_affine(p["x"], 2, wb[0], wb[0].numel(), K, R, S, st, pad, p["area"],
                               p["res"] if res else None, relu)


_AFF_PARAMS = [(s, m, False) for s, m in AFFINE_SHAPES] + [(s, m, True) for s, m in AFFINE_SHAPES if s[5] != 1]


@pytest.mark.parametrize("shape,mags,other", _AFF_PARAMS,
                         ids=[f"{_ids(s)}-{'rw0_h90' if o else 'default_plan'}" for s, _, o in _AFF_PARAMS])
def test_affine_epilogue_rounds_once(dev, shape, mags, other):
    """y == bf16(act(conv * sc + sh (+ residual))) rounded ONCE (sc = +-2^e, integer sh and residual: the fp32
    epilogue is exact in whatever order it is evaluated), on the default plan's kernels and, with
    gm_conv_set_rw(0) / gm_conv_set_h9(0), on the lean kernel.  The declined 1x1 shape (plain forward, then the
    coefficient-only apply) is held to ITS contract: two roundings, against a reference built that way."""
    from greedy_multimodal_learning_amd import _lib as L
    lib = L.load()
    N, C, H, W, K, k, st = shape
    p = _affine_case(shape, mags, dev)
    d = L.ConvDescHW(N, H, W, C, K, k, k, st, st, k // 2, k // 2)
    with knobs(**(dict(rw=0, h9=0) if other else {})):
        assert lib.gm_conv2d_fwd_affine_ok(ctypes.byref(d), 2) == (0 if k == 1 else 1)
        if shape[:5] == (8, 512, 7, 7, 512):
            dd = L.ConvDesc(N, H, W, C, K, k, k, st, k // 2)
            assert lib.gm_conv2d_splitk_ws_bytes_grouped(ctypes.byref(dd), 2, 0) > 0
        for res, relu in AFF_CASES:
            y = _affine_run(p, res, relu)
            _eq(y, (p["two"] if k == 1 else p["one"])[(res, relu)], f"{_ids(shape)} residual={res} relu={relu}")


# ---- 5. weight gradients: fp32 out, torch.equal to the exact reference -----------------------------
# (N, C, H, W, K, R, stride, pad), knobs: the kernel they force (as the neighbouring tests do)
# Slabs: k_conv_wgrad4's plan (conv_wgrad_plan.h plan_wgrad4()) splits the 64-pixel steps over workgroups only from 16
# steps (>= 8 per split); "direct" rows write the gradient from one workgroup per tile, "split" rows through
# partial slabs and the fixed-order sum.  gm_conv_set_wgrad_staging picks the kernel's operand staging (its WR
# template argument): 1 registers, 0 LDS-DMA; the default (2) takes registers for 1x1 filters only.
# gm_conv_set_1x1_gemm plays no part in a weight gradient: every 1x1 one runs on k_conv_wgrad4.
_W4 = [  # shape, what
    ((2, 64, 9, 7, 64, 3, 1, 1), "3x3, direct (2 steps)"),
    ((3, 64, 20, 20, 128, 3, 2, 1), "3x3 strided, direct (5 steps)"),
    ((5, 256, 14, 14, 256, 3, 1, 1), "3x3, split in 2 slabs (16 steps), ragged batch"),
    ((4, 256, 14, 14, 64, 1, 1, 0), "1x1/s1, direct (13 steps)"),
    ((1, 64, 5, 3, 128, 1, 1, 0), "1x1/s1, M = 15, direct"),
    ((16, 64, 28, 28, 256, 1, 1, 0), "1x1/s1, split in 22 slabs (196 steps)"),
    ((7, 256, 14, 14, 512, 1, 2, 0), "1x1/s2, direct (6 steps), ragged batch"),
    ((16, 128, 28, 28, 256, 1, 2, 0), "1x1/s2, split in 6 slabs (49 steps)"),
]
WGRAD_ROWS = [(s, dict(wgrad_loop=0, wgrad_staging=wr), f"k_conv_wgrad4 {what}, {name} staging")
              for s, what in _W4 for wr, name in ((1, "register"), (0, "LDS-DMA"))] + [
    ((2, 64, 9, 7, 64, 3, 1, 1), dict(wgrad_loop=2), "k_wgrad_halo64 PP = 64"),
    ((2, 128, 5, 9, 128, 3, 1, 1), dict(wgrad_loop=6), "k_wgrad_halo64 PP = 32"),
    ((2, 256, 5, 9, 256, 3, 1, 1), dict(wgrad_loop=14), "k_wgrad_halo64 PP = 16"),
    ((3, 512, 7, 7, 512, 3, 1, 1), dict(wgrad_loop=14), "k_wgrad_halo64 PP = 16, layer 4"),
    ((3, 256, 14, 14, 256, 3, 1, 1), dict(wgrad_loop=16), "k_wgrad_ring"),
    ((5, 128, 9, 11, 128, 3, 2, 1), dict(wgrad_loop=16), "k_wgrad_ring strided, ragged M"),
    ((2, 32, 7, 5, 128, 3, 1, 1), dict(wgrad_loop=16), "k_wgrad_ring, C = 32"),
    # a cropped gradient (c_real < C, a fourth element) under the default knobs: the shape's dedicated kernel
    # must not take it - k_conv_wgrad4 without its direct form, then k_wgrad_reduce
    ((2, 64, 9, 7, 64, 3, 1, 1), {}, "halo64-eligible, c_real 61: k_conv_wgrad4, 1 slab, k_wgrad_reduce", 61),
    ((5, 256, 14, 14, 256, 3, 1, 1), {}, "ring-eligible, c_real 250: k_conv_wgrad4, 2 slabs, k_wgrad_reduce", 250),
]


def _wgrad_id(r):
    return f"{_ids(r[0])}-{'_'.join(f'{k}{v}' for k, v in r[1].items())}" + (f"c_real{r[3]}" if len(r) > 3 else "")


@pytest.mark.parametrize("shape,kn,path,c_real", [r if len(r) > 3 else r + (r[0][1],) for r in WGRAD_ROWS],
                         ids=[_wgrad_id(r) for r in WGRAD_ROWS])
def test_wgrad_bit_exact(dev, shape, kn, path, c_real):
    """gm_conv2d_wgrad_grouped_bf16 over two view groups, plain and accumulating onto an integer base:
    the fp32 gradient == the exact one (a bf16 partial, a lost or doubled slab changes an integer).
    c_real < C: the gradient of the first c_real input channels, groups K*R*R*c_real floats apart, with
    every channel of x non-zero (a wrong crop changes an integer) and nothing written past the last group."""
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import conv as CV
    lib = L.load()
    N, C, H, W, K, R, st, pad = shape
    G = 2
    P, Q = E.out_hw(H, W, R, R, st, pad)
    mx, md, base = 4, 4, 1000.0
    E.assert_exact_bound(N * P * Q, mx, md)
    assert N * P * Q * mx * md + base < E.LIMIT
    g = torch.Generator().manual_seed(sum(shape))
    x = E.ints((G * N, H, W, C), mx, g)
    dy = E.ints((G * N, P, Q, K), md, g)
    if c_real < C:
        x[x == 0] = mx
    refs = []
    for gi in range(G):
        xr, gr = x[gi * N:(gi + 1) * N].permute(0, 3, 1, 2), dy[gi * N:(gi + 1) * N].permute(0, 3, 1, 2)
        ref = torch.nn.grad.conv2d_weight(xr, (K, C, R, R), gr, stride=st, padding=pad)
        if shape == WGRAD_ROWS[0][0] and gi == 0:
            assert torch.equal(torch.nn.grad.conv2d_weight(xr.double(), (K, C, R, R), gr.double(), stride=st,
                                                           padding=pad), ref.double())
        assert float(ref.abs().max()) > 8
        refs.append(ref.permute(0, 2, 3, 1)[..., :c_real])   # KRSC, the first c_real input channels
    xd, dyd = x.to(BF).to(dev), dy.to(BF).to(dev)
    d = CV._desc_hw(N, H, W, C, K, R, R, st, st, pad, pad)
    outs = []
    with knobs(**kn):
        need = lib.gm_conv2d_wgrad_grouped_scratch(ctypes.byref(d), G)
        scr = torch.empty(max(need, 16), device=dev, dtype=torch.uint8)
        for acc in (0, 1):
            n = K * R * R * c_real
            dw = torch.full((G * n + 64,), base, device=dev, dtype=torch.float32)
            L.check(lib.gm_conv2d_wgrad_grouped_bf16(ctypes.byref(d), G, dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(),
                                                      n, c_real, acc, scr.data_ptr(), need, L.stream_of(dev)),
                    "wgrad")
            assert torch.equal(dw[G * n:].cpu(), torch.full((64,), base)), f"{path}: written past the gradient"
            outs.append(dw[:G * n].view(G, K, R, R, c_real))
        torch.cuda.synchronize()
    for gi in range(G):
        assert torch.equal(outs[0][gi].cpu(), refs[gi]), f"{path}: group {gi} plain"
        assert torch.equal(outs[1][gi].cpu(), refs[gi] + base), f"{path}: group {gi} accumulating"


def test_wgrad_stem_bit_exact(dev):
    """k_wgrad_stem (gm_conv_set_wgrad_stem(1)) and k_conv_wgrad4 (0) on the pixel-pair view, two view
    groups, B = 3, 64 x 64, plain and accumulating onto an integer base: both == the exact weight gradient of the
    pair-view convolution (+ the base)."""
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import conv as CV
    lib = L.load()
    B, G, H, W, K, R = 3, 2, 64, 64, 64, 7
    P, Q, Sp, Hp, Wp = CV._stem_geom(H, W, R, R, 3)
    E.assert_exact_bound(B * P * Q, 4, 4)
    g = torch.Generator().manual_seed(B + G + H + W)
    xp = torch.empty(G * B, Hp, Wp // 2, 8, device=dev, dtype=BF)
    for v in range(G):
        CV.stem_pack(E.ints((B, 3, H, W), 4, g).to(dev), E.ints((K, 3, R, R), 1, g).to(dev), 3,
                     xp=xp[v * B:(v + 1) * B], wp=torch.empty(K, R, Sp, 8, device=dev, dtype=BF))
    dy = E.ints((G * B, P, Q, K), 4, g)
    dyd = dy.to(BF).to(dev)
    d = CV._desc_hw(B, Hp, Wp // 2, 8, K, R, Sp, 2, 1, 0, 0)
    n = K * R * Sp * 8
    xph = xp.float().cpu()
    refs = [torch.nn.grad.conv2d_weight(xph[v * B:(v + 1) * B].permute(0, 3, 1, 2), (K, 8, R, Sp),
                                        dy[v * B:(v + 1) * B].permute(0, 3, 1, 2), stride=(2, 1)).permute(0, 2, 3, 1)
            for v in range(G)]
    base = 1000.0
    assert B * P * Q * 4 * 4 + base < E.LIMIT
    for on in (1, 0):
        outs = []
        with knobs(wgrad_stem=on):
            need = lib.gm_conv2d_wgrad_grouped_scratch(ctypes.byref(d), G)
            scr = torch.empty(max(need, 16), device=dev, dtype=torch.uint8)
            for acc in (0, 1):   # plain over stale content, and accumulating onto an integer base
                dw = torch.full((G, K, R, Sp, 8), base, device=dev)
                L.check(lib.gm_conv2d_wgrad_grouped_bf16(ctypes.byref(d), G, dyd.data_ptr(), xp.data_ptr(),
                                                          dw.data_ptr(), n, 8, acc, scr.data_ptr(), need,
                                                          L.stream_of(dev)), "wgrad")
                outs.append(dw)
            torch.cuda.synchronize()
        for v in range(G):
            assert torch.equal(outs[0][v].cpu(), refs[v]), (on, v, "plain")
            assert torch.equal(outs[1][v].cpu(), refs[v] + base), (on, v, "accumulating")


# ---- 6. fp32 trunk kernels -------------------------------------------------------------------------
F32_SHAPES = [  # one per tile form of test_gpu_f32_split.py's list (N, C, H, W, K, R, S, stride, pad)
    (1, 3, 37, 30, 64, 7, 7, 2, 3),        # stem, element loads, ragged
    (2, 64, 16, 16, 128, 3, 3, 2, 1),      # strided dgrad
    (3, 128, 9, 11, 256, 3, 3, 2, 1),      # ragged strided
    (16, 64, 56, 56, 64, 3, 3, 1, 1),      # 128 x 64 tiles, long split weight-gradient reduction
    (2, 6, 7, 5, 12, 3, 3, 1, 1),          # C % 4 != 0: element path everywhere
    (32, 128, 56, 56, 128, 1, 1, 1, 0),    # 128 x 128 tiles, 16-byte loads
    (16, 66, 64, 64, 130, 1, 1, 1, 0),     # 128 x 128 tiles, element loads
]
_f32_cache = {}


def _f32_case(shape):
    if shape not in _f32_cache:
        N, C, H, W, K, R, S, st, pad = shape
        x, w, dy = E.conv_operands(shape, (8, 8))
        if shape == F32_SHAPES[4]:
            E.assert_fp32_is_exact(x, w, dy, st, pad)
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = F.conv2d(xr, wr, stride=st, padding=pad)
        y.backward(dy)
        _f32_cache[shape] = (x, w, dy, y.detach(), xr.grad, wr.grad)
    return _f32_cache[shape]


@pytest.mark.parametrize("terms", [0, 3, 6])
@pytest.mark.parametrize("shape", F32_SHAPES, ids=_ids)
def test_f32_trunk_small_integers_bit_exact(dev, shape, terms):
    """The exact-f32 MFMA kernel (terms 0) and the split-bf16 contraction (integers split exactly:
    m = l = 0): fwd, dgrad and wgrad == the exact reference, on every tile form."""
    from greedy_multimodal_learning_amd.conv import GMConv2d
    N, C, H, W, K, R, S, st, pad = shape
    x, w, dy, yr, dxr, dwr = _f32_case(shape)
    m = GMConv2d(C, K, (R, S), stride=st, padding=pad, bias=False).to(dev)
    m.f32_terms = terms
    with torch.no_grad():
        m.weight.copy_(w)
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    assert y.dtype == torch.float32 and "ConvF32" in type(y.grad_fn).__name__
    y.backward(dy.to(dev))
    assert torch.equal(y.detach().cpu(), yr), "y"
    assert torch.equal(xd.grad.cpu(), dxr), "dx"
    assert torch.equal(m.weight.grad.cpu(), dwr), "dw"


F32_AFFINE = {  # test_gpu_f32_affine.py's forms: (N, H, W, C, K, R, S, stride, pad), residual, relu
    "stem": ((2, 32, 32, 3, 64, 7, 7, 2, 3), False, True),
    "l1_3x3_split": ((2, 8, 8, 64, 64, 3, 3, 1, 1), True, True),
    "s2_3x3_odd": ((3, 9, 9, 64, 128, 3, 3, 2, 1), False, True),
    "tiles_2x2": ((2, 128, 128, 8, 128, 3, 3, 1, 1), True, False),
    "l4_wide": ((2, 3, 3, 512, 512, 3, 3, 1, 1), True, True),
}


@pytest.mark.parametrize("terms", [0, 3, 6])
@pytest.mark.parametrize("name", list(F32_AFFINE))
def test_f32_affine_bit_exact(dev, name, terms):
    """conv_f32_affine with sc = +-2^e, integer sh and residual: == the float64 composition."""
    from greedy_multimodal_learning_amd import conv as G
    (N, H, W, C, K, R, S, st, pad), residual, relu = F32_AFFINE[name]
    x, w, _ = E.conv_operands((N, C, H, W, K, R, S, st, pad), (8, 8))
    g = torch.Generator().manual_seed(len(name))
    sc, sh = E.pow2_coefficients(1, K, g)
    conv = F.conv2d(x, w, stride=st, padding=pad)
    res = E.ints(conv.shape, 200, g)
    assert float(conv.abs().max()) * 4 + 208 < E.LIMIT / 4
    ref = conv.double() * sc.view(1, K, 1, 1).double() + sh.view(1, K, 1, 1).double()
    if residual:
        ref = ref + res.double()
    if relu:
        ref = torch.relu(ref)
        assert 0.05 < float((ref == 0).float().mean()) < 0.95
    assert torch.equal(ref.float().double(), ref)
    coef = torch.cat([sc[0], sh[0]]).to(dev)
    P, Q = conv.shape[2:]
    out = torch.full((N, K, P, Q), float("nan"), device=dev).contiguous(memory_format=CL)
    G.conv_f32_affine(G._desc(N, H, W, C, K, R, S, st, pad), _cl(x, dev, torch.float32), _cl(w, dev, torch.float32),
                      out, coef, residual=_cl(res, dev, torch.float32) if residual else None, relu=relu, terms=terms)
    assert torch.equal(out.cpu(), ref.float())


# ---- 7. statistics rows from the convolution epilogues -------------------------------------------
STATS_ROWS = [  # N per view, C, H, W, K, R, S, stride, pad: ternary operands
    ((3, 64, 20, 20, 64, 3, 3, 1, 1), "k_conv_rw"),
    ((3, 128, 13, 11, 128, 3, 3, 1, 1), "k_conv_h9"),
    ((3, 64, 20, 20, 128, 3, 3, 2, 1), "k_conv_igemm_ut, strided"),
    ((2, 64, 9, 11, 128, 3, 3, 2, 1), "k_conv_igemm_ut, strided, ragged 64 x 64 tiles"),
    ((8, 512, 7, 7, 512, 3, 3, 1, 1), "split-K"),
    ((4, 256, 14, 14, 64, 1, 1, 1, 0), "k_gemm_ring, ragged M"),
]
STATS_BAR = 2.0 ** -21   # 8 fp32 ulps


@pytest.mark.parametrize("shape,path", STATS_ROWS, ids=[_ids(r[0]) for r in STATS_ROWS])
def test_epilogue_statistics_exact(dev, shape, path):
    """vconv(stats=) -> vbn and the single-launch BatchNorm on the same ternary inputs, momentum 1:
    y is the exact integer convolution, running_mean / running_var are the float64 batch mean and
    unbiased variance within 2^-21 relative (a missing, doubled or stale partial row is a wrong
    integer sum, orders of magnitude above the bar)."""
    from greedy_multimodal_learning_amd.bn import GMBatchNorm2d
    from greedy_multimodal_learning_amd.conv import GMConv2d
    from greedy_multimodal_learning_amd.vtrunk import vbn, vconv
    N, C, H, W, K, R, S, st, pad = shape
    G = 2
    g = torch.Generator().manual_seed(sum(shape))
    x = E.ints((G * N, C, H, W), 1, g)
    ws = [E.ints((K, C, R, S), 1, g) for _ in range(G)]
    E.assert_exact_bound(C * R * S, 1, 1)
    ys = [F.conv2d(x[i * N:(i + 1) * N], ws[i], stride=st, padding=pad) for i in range(G)]
    convs = []
    for i in range(G):
        m = GMConv2d(C, K, (R, S), stride=st, padding=pad, bias=False).to(dev)
        with torch.no_grad():
            m.weight.copy_(ws[i])
        convs.append(m.to(memory_format=CL))
    means, varis = [], []
    for y in ys:   # narrow operands: y exact in bf16, the sums exact in fp32 under any partition
        assert float(y.abs().max()) <= 256
        flat = y.double().permute(1, 0, 2, 3).reshape(K, -1)
        assert float((flat * flat).sum(1).max()) < E.LIMIT
        means.append(flat.mean(1))
        varis.append(flat.var(1, unbiased=True))
    worst = {}
    for kind in ("epilogue", "single_launch"):
        bns = [GMBatchNorm2d(K, momentum=1.0).to(dev).train() for _ in range(G)]
        stats = {} if kind == "epilogue" else None
        xs = _cl(x, dev).requires_grad_(True)
        y0 = vconv(xs, convs, stats=stats)
        if kind == "epilogue":
            assert "part" in stats and stats["rows"] >= 1, path
            if path == "split-K":   # the grouped plan really splits
                from greedy_multimodal_learning_amd import _lib as L
                dd = L.ConvDesc(N, H, W, C, K, R, S, st, pad)
                assert L.load().gm_conv2d_splitk_ws_bytes_grouped(ctypes.byref(dd), G, 0) > 0
        vbn(y0, bns, relu=True, stats=stats)
        torch.cuda.synchronize()
        _eq(y0, torch.cat(ys), f"{path}: y")
        errs = []
        for i in range(G):
            assert int(bns[i].num_batches_tracked) == 1
            errs.append(E.ulps_rel(bns[i].running_mean, means[i]))
            errs.append(E.ulps_rel(bns[i].running_var, varis[i]))
        worst[kind] = max(errs)
        print(f"{path} {kind}: max relative error of running_mean / running_var {worst[kind]:.3e} "
              f"(bar {STATS_BAR:.3e})")
    for kind, e in worst.items():
        assert e <= STATS_BAR, (path, kind, e)


# ---- 8. gm_gemm_f32 --------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (3, 5, 7), (64, 512, 1024), (64, 128, 256),
                                   (256, 512, 64), (17, 33, 129), (1, 300, 64), (512, 1024, 64)])
@pytest.mark.parametrize("act", [0, 1])
def test_gemm_f32_bit_exact(dev, M, N, K, act):
    from greedy_multimodal_learning_amd import ops
    E.assert_exact_bound(K + 1, 8, 8)
    g = torch.Generator().manual_seed(M * 1000 + N + K)
    x, w, b = E.ints((M, K), 8, g), E.ints((N, K), 8, g), E.ints((N,), 8, g)
    y = ops.linear(x.to(dev), w.to(dev), b.to(dev), act=act).cpu()
    ref = x.double() @ w.double().T + b.double()
    if act == 1:
        ref = ref.clamp_min(0)
    assert torch.equal(y.double(), ref)


def test_gemm_segments_ones_mask_accumulate_bit_exact(dev):
    from greedy_multimodal_learning_amd import ops
    from greedy_multimodal_learning_amd.ops import ONES, Op
    g = torch.Generator().manual_seed(3)
    B, C1, C2, N = 5, 24, 40, 36
    a1, a2, w = E.ints((B, C1), 8, g), E.ints((C2,), 8, g), E.ints((N, C1 + C2), 8, g)
    mask = (E.ints((B, N), 4, g) > 0).float()
    c0 = E.ints((B, N), 100, g)
    A1, A2, W, MK, Cd = (t.to(dev).contiguous() for t in (a1, a2, w, mask, c0))
    ops.gemm([dict(M=B, N=N, segs=[(C1, Op(A1, C1, 1), Op(W, 1, C1 + C2)),
                                   (C2, Op(A2, 0, 1), Op(W, 1, C1 + C2, off=C1))],
                   C=Cd, ld_c=N, mask=MK, ld_mask=N, accumulate=1)], dev)
    ref = c0.double() + (a1.double() @ w[:, :C1].double().T + a2.double()[None] @ w[:, C1:].double().T) * mask.double()
    assert torch.equal(Cd.cpu().double(), ref)
    out = torch.empty(1, N, device=dev)
    ops.gemm([dict(M=1, N=N, segs=[(B, ONES, Op(MK, N, 1))], C=out, ld_c=N)], dev)
    assert torch.equal(out.cpu()[0], mask.sum(0))


@pytest.mark.parametrize("M,N,K,acc", [(300, 5000, 32, 0), (1000, 1027, 100, 1)])
def test_gemm_outer_product_bit_exact(dev, M, N, K, acc):
    """k_gemm_outer (form 1) and k_gemm_f32 on its shapes (form bit 9): == fp64."""
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import ops
    from greedy_multimodal_learning_amd.ops import Op
    g = torch.Generator().manual_seed(M + N + K)
    dz, sq = E.ints((K, M), 8, g), E.ints((K, N), 8, g)
    c0 = E.ints((M, N), 100, g) if acc else torch.zeros(M, N)
    ref = c0.double() + dz.double().T @ sq.double()
    try:
        for form in (1, 1 | 512):
            L.check(L.load().gm_gemm_set_form(form), "gemm form")
            C = c0.to(dev).contiguous()
            ops.gemm([dict(M=M, N=N, segs=[(K, Op(dz.to(dev), 1, M), Op(sq.to(dev), N, 1))], C=C, ld_c=N,
                           accumulate=acc)], dev)
            assert torch.equal(C.cpu().double(), ref), form
    finally:
        L.check(L.load().gm_gemm_set_form(1), "gemm form")
