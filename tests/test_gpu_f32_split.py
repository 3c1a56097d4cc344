"""Split-bf16 contraction of the fp32 trunk convolutions (gm_conv2d_f32_split, bf16x3 /
bf16x6 on the bf16 MFMA) against PyTorch in float64 on the CPU.

bf16x6 keeps every cross term down to 2^-24 and is held to the exact-f32 kernel's own
bounds.  bf16x3 drops terms of ~2^-16; its floor is computed here, per shape, as the same
three-term contraction evaluated on the CPU from the split parts (fp32 F.conv2d of hh + hm +
mh) against float64: the GPU may be off by at most twice that (summation order), and must
beat the single-term (hh only) error by 50x, so a lost cross term fails both.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import spec
from helpers import close
from oracle import weights

pytestmark = pytest.mark.gpu
CL = torch.channels_last
tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731

SHAPES = [  # N, C, H, W, K, R, S, stride, pad   (the list of test_gpu_f32_trunk.py)
    (2, 3, 64, 64, 64, 7, 7, 2, 3),      # RGB stem, element-load path
    (1, 3, 37, 30, 64, 7, 7, 2, 3),      # stem, ragged
    (2, 64, 16, 16, 64, 3, 3, 1, 1),     # layer1
    (2, 64, 16, 16, 128, 3, 3, 2, 1),    # layer2 entry (strided dgrad)
    (2, 64, 16, 16, 128, 1, 1, 2, 0),    # downsample
    (3, 128, 9, 11, 256, 3, 3, 2, 1),    # ragged strided
    (2, 256, 4, 4, 512, 3, 3, 2, 1),
    (4, 512, 2, 2, 512, 3, 3, 1, 1),     # layer4 at 64x64 input
    (16, 64, 56, 56, 64, 3, 3, 1, 1),    # 128x128 tiles, long wgrad reduction (split)
    (2, 6, 7, 5, 12, 3, 3, 1, 1),        # C % 4 != 0: element path everywhere
    (1, 8, 5, 5, 20, 1, 1, 1, 0),
]
# The planner takes 128 x 128 tiles once ceil(M/128) * ceil(N/128) reaches the CU count (256), and
# this kernel narrows them to 128 x 64 where N <= 64, which is what the 16x64x56x56 row above gets.
# These reach the 128 x 128 form itself (60 KB LDS image, four chunks per thread, the 4-deep
# register transpose of dgrad's weights) in fwd AND dgrad, 1x1 so the float64 reference stays cheap:
BIG = [
    (32, 128, 56, 56, 128, 1, 1, 1, 0),  # 16-byte loads: M = 100352, N = 128 -> 784 tiles both passes
    (16, 66, 64, 64, 130, 1, 1, 1, 0),   # element loads (C, K % 4 != 0): M = 65536; fwd N = 130 -> 1024
                                         # tiles, dgrad N = 66 (> 64: not narrowed) -> 512 tiles
]
SHAPES = SHAPES + BIG
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)


def _hm(t):
    """The two leading bf16 parts of an fp32 tensor, as fp32."""
    h = t.bfloat16().float()
    return h, (t - h).bfloat16().float()


def _conv3(x, w, stride, pad):
    """The three-term contraction (hh + hm + mh) of a forward convolution in fp32 on the CPU."""
    (xh, xm), (wh, wm) = _hm(x), _hm(w)
    c = lambda a, b: F.conv2d(a, b, stride=stride, padding=pad)  # noqa: E731
    return c(xm, wh) + c(xh, wm) + c(xh, wh)


_data_cache = {}


def _data(shape):
    """Inputs, the float64 results and the CPU three-term / single-term errors of one shape
    (computed once, shared by both term counts, never modified)."""
    if shape in _data_cache:
        return _data_cache[shape]
    N, C, H, W, K, R, S, st, pad = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5
    P, Q = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    gy = torch.randn(N, K, P, Q, generator=g)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, stride=st, padding=pad)
    yr.backward(gy.double())
    ref = (yr.detach(), xr.grad, wr.grad)
    (xh, xm), (wh, wm), (gh, gm) = _hm(x), _hm(w), _hm(gy)
    ci = lambda wt, gt: conv2d_input(x.shape, wt, gt, stride=st, padding=pad)  # noqa: E731
    cw = lambda xt, gt: conv2d_weight(xt, w.shape, gt, stride=st, padding=pad)  # noqa: E731
    three = (_conv3(x, w, st, pad), ci(wm, gh) + ci(wh, gm) + ci(wh, gh), cw(xm, gh) + cw(xh, gm) + cw(xh, gh))
    one = (F.conv2d(xh, wh, stride=st, padding=pad), ci(wh, gh), cw(xh, gh))
    floors = [(_err(a, r), _err(b, r)) for a, b, r in zip(three, one, ref)]
    _data_cache[shape] = (x, w, gy, ref, floors)
    return _data_cache[shape]


def _run_module(dev, shape, terms, x, w, gy):
    from greedy_multimodal_learning_amd.conv import GMConv2d
    N, C, H, W, K, R, S, st, pad = shape
    m = GMConv2d(C, K, (R, S), stride=st, padding=pad, bias=False).to(dev)
    m.f32_terms = terms
    with torch.no_grad():
        m.weight.copy_(w)
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    assert y.dtype == torch.float32 and y.is_contiguous(memory_format=CL)
    assert "ConvF32" in type(y.grad_fn).__name__
    y.backward(gy.to(dev))
    assert m.weight.grad.dtype == torch.float32
    return y, xd.grad, m.weight.grad


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_bf16x6_fwd_dgrad_wgrad_vs_fp64(dev, shape):
    """terms = 6 under the exact-f32 kernel's bounds (a dropped term lands at ~5e-6)."""
    x, w, gy, ref, _ = _data(shape)
    y, dx, dw = _run_module(dev, shape, 6, x, w, gy)
    e = [_err(y, ref[0]), _err(dx, ref[1]), _err(dw, ref[2])]
    print(f"bf16x6 {_ids(shape)}: y {e[0]:.2e} dx {e[1]:.2e} dw {e[2]:.2e}")
    assert e[0] < 2e-6
    assert e[1] < 2e-6
    assert e[2] < 5e-6


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_bf16x3_fwd_dgrad_wgrad_vs_cpu_floor(dev, shape):
    """terms = 3: within 2x of the CPU three-term floor and 50x under the single-term error."""
    x, w, gy, ref, floors = _data(shape)
    outs = _run_module(dev, shape, 3, x, w, gy)
    rows = []
    for name, o, r, (f3, f1) in zip(("y", "dx", "dw"), outs, ref, floors):
        e = _err(o, r)
        rows.append((name, e, f3, f1))
        print(f"bf16x3 {_ids(shape)} {name}: gpu {e:.2e}  cpu three-term {f3:.2e}  cpu single-term {f1:.2e}")
    for name, e, f3, f1 in rows:
        assert e <= 2 * f3, (name, e, f3)
        assert e <= f1 / 50, (name, e, f1)


@pytest.mark.parametrize("shape", [(8, 64, 28, 28, 128, 3, 3, 2, 1)] + BIG, ids=_ids)
@pytest.mark.parametrize("terms", [3, 6])
def test_split_deterministic_accumulate_and_addend(dev, terms, shape):
    """Bit-identical reruns (split reductions summed in a fixed order); wgrad accumulate
    adds into the buffer; the dgrad addend (gradient join) is folded in.  At the exact
    kernel's test shape and at the two shapes that run on 128 x 128 tiles."""
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import conv as G
    N, C, H, W, K, R, S, st, pad = shape
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, C, H, W, device=dev, generator=gen).contiguous(memory_format=CL)
    w = torch.randn(K, C, R, S, device=dev, generator=gen).contiguous(memory_format=CL)
    P, Q = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    dy = torch.randn(N, K, P, Q, device=dev, generator=gen).contiguous(memory_format=CL)
    add = torch.randn(N, C, H, W, device=dev, generator=gen).contiguous(memory_format=CL)
    d = G._desc(N, H, W, C, K, R, S, st, pad)
    outs = []
    for _ in range(2):
        y = torch.empty(N, K, P, Q, device=dev).contiguous(memory_format=CL)
        dx = torch.empty(N, C, H, W, device=dev).contiguous(memory_format=CL)
        dxa = torch.empty_like(dx)
        dw = torch.empty(K, C, R, S, device=dev).contiguous(memory_format=CL)
        G.conv_f32(L.GM_CONV_FWD, d, x=x, w=w, out=y, terms=terms)
        G.conv_f32(L.GM_CONV_DGRAD, d, w=w, dy=dy, out=dx, terms=terms)
        G.conv_f32(L.GM_CONV_DGRAD, d, w=w, dy=dy, out=dxa, addend=add, terms=terms)
        G.conv_f32(L.GM_CONV_WGRAD, d, x=x, dy=dy, out=dw, terms=terms)
        outs.append((y, dx, dxa, dw.clone()))
        G.conv_f32(L.GM_CONV_WGRAD, d, x=x, dy=dy, out=dw, accumulate=True, terms=terms)
        torch.testing.assert_close(dw, 2 * outs[-1][3], rtol=1e-6, atol=1e-6)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    torch.testing.assert_close(outs[0][2], outs[0][1] + add, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("terms", [3, 6])
def test_split_scale_invariance(dev, terms):
    """Inputs scaled by 2^-40 / 2^40 with inversely scaled weights: no part of the split
    underflows or overflows in the working range, so the relative error stays put."""
    shape = (2, 64, 16, 16, 64, 3, 3, 1, 1)
    N, C, H, W, K, R, S, st, pad = shape
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5
    gy = torch.randn(N, K, H, W, generator=g)
    errs = {}
    for e2 in (0, -40, 40):
        s = 2.0 ** e2
        xs, ws = x * s, w / s  # exact: powers of two
        xr, wr = xs.double().requires_grad_(True), ws.double().requires_grad_(True)
        F.conv2d(xr, wr, stride=st, padding=pad).backward(gy.double())
        y, dx, dw = _run_module(dev, shape, terms, xs, ws, gy)
        yr = F.conv2d(xs.double(), ws.double(), stride=st, padding=pad)
        errs[e2] = (_err(y, yr), _err(dx, xr.grad), _err(dw, wr.grad))
        print(f"terms {terms} scale 2^{e2}: y {errs[e2][0]:.2e} dx {errs[e2][1]:.2e} dw {errs[e2][2]:.2e}")
    for e2 in (-40, 40):
        for a, b in zip(errs[e2], errs[0]):
            assert a <= 2 * b, (e2, errs)


@pytest.mark.parametrize("terms", [3, 6])
@pytest.mark.parametrize("shape,ones", [((1, 8, 5, 5, 20, 1, 1, 1, 0), False), ((2, 6, 7, 5, 12, 3, 3, 1, 1), True)],
                         ids=["1x1", "3x3-ones"])
def test_split_small_integers_bit_exact(dev, terms, shape, ones):
    """Small integers split exactly (m = l = 0) and every partial sum is an integer below
    2^24, so zero padding and ragged tiles must come out bit-exact in every mode."""
    N, C, H, W, K, R, S, st, pad = shape
    g = torch.Generator().manual_seed(3)
    x = torch.ones(N, C, H, W) if ones else torch.randint(-8, 9, (N, C, H, W), generator=g).float()
    w = torch.randint(-8, 9, (K, C, R, S), generator=g).float()
    P, Q = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    gy = torch.randint(-8, 9, (N, K, P, Q), generator=g).float()
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, stride=st, padding=pad)
    yr.backward(gy.double())
    y, dx, dw = _run_module(dev, shape, terms, x, w, gy)
    assert torch.equal(y.cpu(), yr.detach().float())
    assert torch.equal(dx.cpu(), xr.grad.float())
    assert torch.equal(dw.cpu(), wr.grad.float())


def _set_terms(net, terms):
    from greedy_multimodal_learning_amd.conv import GMConv2d
    n = 0
    for m in net.modules():
        if isinstance(m, GMConv2d):
            m.f32_terms = terms
            n += 1
    assert n > 0
    return net


def _trunk(dev, terms):
    from greedy_multimodal_learning_amd.resnet import resnet18
    from oracle.resnet_ref import resnet18 as resnet18_ref
    torch.manual_seed(0)
    ref = resnet18_ref(num_classes=40).double()
    r32 = resnet18_ref(num_classes=40)
    r32.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    net = resnet18(num_classes=40)
    net.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    net = _set_terms(net.to(dev), terms)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 64, 64, generator=g)
    return ref, r32, net, x, g


def test_resnet18_trunk_bf16x6_vs_fp64(dev):
    """test_resnet18_trunk_f32_vs_fp64's own assertions (envelopes of the fp32 CPU oracle)
    with every convolution on the six-term contraction."""
    ref, r32, net, x, g = _trunk(dev, 6)
    out, o32, out_ref = net(x.to(dev)), r32(x), ref(x.double())
    print(f"bf16x6 trunk logits vs fp64: gpu {_err(out, out_ref):.2e}  cpu fp32 {_err(o32, out_ref):.2e}")
    assert _err(out, out_ref) < max(4 * _err(o32, out_ref), 1e-5)
    gy = torch.randn(out_ref.shape, generator=g)
    out.backward(gy.to(dev))
    o32.backward(gy)
    out_ref.backward(gy.double())
    rp, p32 = dict(ref.named_parameters()), dict(r32.named_parameters())
    e_hip = np.array([_err(p.grad, rp[n].grad) for n, p in net.named_parameters()])
    e_32 = np.array([_err(p32[n].grad, rp[n].grad) for n, _ in net.named_parameters()])
    assert np.sqrt((e_hip ** 2).mean()) <= max(3 * np.sqrt((e_32 ** 2).mean()), 1e-4), (e_hip, e_32)
    assert e_hip.max() <= max(10 * e_32.max(), 1e-4)
    assert np.median(e_hip) < 1e-2


def test_resnet18_trunk_bf16x3_vs_cpu_emulation(dev):
    """terms = 3: the logits error against fp64 is at most 3x that of the CPU emulation (the
    oracle's net with every conv forward replaced by the three-term split F.conv2d); the
    margin is for summation order and for ReLU / BatchNorm amplification."""
    ref, r32, net, x, _ = _trunk(dev, 3)
    for m in r32.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.forward = lambda t, m=m: _conv3(t, m.weight, m.stride, m.padding)
    with torch.no_grad():
        out, emu, out_ref = net(x.to(dev)), r32(x), ref(x.double())
    e_gpu, e_emu = _err(out, out_ref), _err(emu, out_ref)
    print(f"bf16x3 trunk logits vs fp64: gpu {e_gpu:.2e}  cpu emulation {e_emu:.2e}")
    assert e_gpu <= 3 * e_emu, (e_gpu, e_emu)


@pytest.mark.parametrize("case", [spec.MODEL_CASES[0], [c for c in spec.MODEL_CASES if c.get("cur")][0]],
                         ids=lambda c: c["id"])
def test_model_bf16x6_vs_reference(golden, dev, case):
    """The logits / loss / scale / squeeze checks of test_model_vs_reference at the case's
    own tolerance, and the fp64 envelope, with f32_terms = 6 on every convolution."""
    from greedy_multimodal_learning_amd.losses import blend_loss
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    from oracle import model_ref
    fix = golden["model"]
    p = case["id"] + "/"
    tol = case.get("gpu_tol", 1e-4)
    m = MMTM_MVCNN(saving_mmtm_scales=True, saving_mmtm_squeeze_array=True)
    weights.apply_to_module(m, seed=spec.SEED_MODEL)
    m = _set_terms(m.to(dev), 6)
    m.train(True)
    x, y = spec.model_inputs(case)
    kw = dict(curation_mode=case.get("cur", False), caring_modality=case.get("caring", None))
    mean, outs, scales, sqs = m(tt(x).to(dev), **kw)
    loss = blend_loss(outs, tt(y).to(dev))
    close(fix, p + "logits", mean.detach().cpu(), rtol=tol, atol=tol)
    close(fix, p + "logits0", outs[0].detach().cpu(), rtol=tol, atol=tol)
    close(fix, p + "logits1", outs[1].detach().cpu(), rtol=tol, atol=tol)
    assert abs(float(loss.detach()) - float(fix[p + "loss"])) < tol * abs(float(fix[p + "loss"]))
    for i in range(3):
        close(fix, p + f"scale{i}_v", scales[i][0], rtol=tol, atol=10 * tol)
        close(fix, p + f"scale{i}_s", scales[i][1], rtol=tol, atol=10 * tol)
        close(fix, p + f"sq{i}_v", sqs[i][0], rtol=tol, atol=10 * tol)
        close(fix, p + f"sq{i}_s", sqs[i][1], rtol=tol, atol=10 * tol)
    o = weights.apply_to_module(model_ref.MMTM_MVCNN_Ref(), seed=spec.SEED_MODEL).double()
    o.train(True)
    with torch.no_grad():
        mean64 = o(tt(x).double(), **kw)[0]
    sc64 = np.abs(mean64.numpy()).max()
    e_ref = (np.abs(fix[p + "logits"] - mean64.numpy()) / sc64).max()
    e_gpu = (np.abs(mean.detach().cpu().double().numpy() - mean64.numpy()) / sc64).max()
    print(f"{case['id']} bf16x6: logits vs fp64 (scale-relative) gpu {e_gpu:.2e} reference {e_ref:.2e}")
    assert e_gpu <= max(4 * e_ref, tol), (e_gpu, e_ref)


def _engine_run(dev, mode, graphs, x, y, steps=2):
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    m = MMTM_MVCNN()
    weights.apply_to_module(m, seed=spec.SEED_MODEL)
    m = m.to(dev)
    st = BalancedStep(m, lr=0.05, compute_dtype=torch.float32, f32_contraction=mode, graphs=graphs)
    losses = [float(st(x, y)) for _ in range(steps)]
    torch.cuda.synchronize()
    return m, st, losses


def test_engine_bf16x6_graphs_equal_eager_and_fp64_loss(dev):
    """BalancedStep(fp32, f32_contraction='bf16x6', graphs=True) at B=4, 64x64: two replayed
    steps equal two eager steps bit for bit; the loss of the step after the first update is
    as close to the float64 oracle's (one SGD step in float64) as the exact mode's, within
    max(4 e_exact, 1e-5)."""
    from oracle import gating_ref, model_ref
    lr = 0.05
    g = torch.Generator().manual_seed(21)
    x = torch.randn(4, 2, 3, 64, 64, generator=g)
    y = torch.randint(0, 40, (4,), generator=g)
    xd, yd = x.to(dev), y.to(dev)
    m_e, _, l_e = _engine_run(dev, "bf16x6", False, xd, yd)
    m_g, st_g, l_g = _engine_run(dev, "bf16x6", True, xd, yd)
    assert st_g._graphs and not st_g.capture_failures, st_g.capture_failures
    assert l_e == l_g
    se, sg = m_e.state_dict(), m_g.state_dict()
    for k in se:
        assert torch.equal(se[k], sg[k]), k
    _, _, l_x = _engine_run(dev, "exact", True, xd, yd)
    o = weights.apply_to_module(model_ref.MMTM_MVCNN_Ref(), seed=spec.SEED_MODEL).double()
    o.train(True)
    l64 = []
    for _ in range(2):
        for q in o.parameters():
            q.grad = None
        loss = gating_ref.blend_loss(o(x.double(), curation_mode=False, caring_modality=None)[1], y)
        loss.backward()
        l64.append(float(loss.detach()))
        with torch.no_grad():
            for q in o.parameters():
                if q.grad is not None:
                    q -= lr * q.grad
    for i in range(2):
        e_exact, e_6 = abs(l_x[i] - l64[i]), abs(l_g[i] - l64[i])
        print(f"step {i + 1} loss {l64[i]:.7f}: |exact - fp64| {e_exact:.2e}  |bf16x6 - fp64| {e_6:.2e}")
        assert e_6 <= max(4 * e_exact, 1e-5), (i, e_6, e_exact)
