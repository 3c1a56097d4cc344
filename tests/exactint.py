"""Integer operands for bit-exact kernel tests (tests/test_gpu_exact_integers.py).

With small integer operands every product and every partial sum of a contraction is an
integer below 2^24, so an fp32 accumulation is exact in ANY order - across tiles, k-steps,
split-K hand-offs and split sums - and a CPU fp32 reference is exact too.  What is left of a
bf16 kernel's arithmetic is the one rounding of its output store: a correct kernel equals
reference.to(bfloat16) bit for bit.

Everything here runs on the CPU.  The helpers assert, on the reference, what makes such a
comparison valid (the 2^24 bound) and what makes it non-vacuous (the wrong roundings a kernel
could commit do change the expected tensor, see wrong_references / assert_discriminates).

"wide" operands (|x| <= 4, |w| <= 2, or larger where a short reduction needs it): outputs pass
256, so many are not bf16 numbers and the store's rounding is under test.  "narrow" operands
(ternary): the outputs stay <= 256 and are exact in bf16 as well.
"""
import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
LIMIT = 1 << 24       # integers up to here are exact in fp32
WIDE = (4, 2)         # max |activation or gradient|, max |weight|
NARROW = (1, 1)


def ints(shape, mag, gen):
    """fp32 tensor of integers drawn uniformly from [-mag, mag]."""
    return torch.randint(-mag, mag + 1, tuple(shape), generator=gen).float()


def assert_exact_bound(terms, *mags):
    """terms products of operands bounded by mags stay below 2^24 in every partial sum."""
    bound = terms
    for m in mags:
        bound *= int(m)
    assert bound < LIMIT, f"{terms} products of magnitudes {mags}: {bound} >= 2^24, fp32 sums not exact"
    return bound


def rne(t):
    """fp32 / fp64 -> bf16, round to nearest even (torch's conversion), as fp32."""
    return t.float().to(BF16).float()


def trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits (the wrong store), as fp32."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def frac_ne(a, b):
    return float((a != b).float().mean())


def out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def conv_operands(shape, mags=WIDE, seed=0, mag_dy=None):
    """x [N,C,H,W], w [K,C,R,S], dy [N,K,P,Q]: integer fp32 tensors (|x| <= mags[0], |w| <= mags[1],
    |dy| <= mag_dy or mags[0]) of a (N, C, H, W, K, R, S, stride, pad) shape, after asserting the
    2^24 bounds of the forward, the input gradient and the weight gradient."""
    N, C, H, W, K, R, S, st, pad = shape
    P, Q = out_hw(H, W, R, S, st, pad)
    md = mags[0] if mag_dy is None else mag_dy
    assert_exact_bound(C * R * S, mags[0], mags[1])       # forward
    assert_exact_bound(K * R * S, md, mags[1])            # input gradient
    assert_exact_bound(N * P * Q, mags[0], md)            # weight gradient
    g = torch.Generator().manual_seed(seed + sum(shape))
    return ints((N, C, H, W), mags[0], g), ints((K, C, R, S), mags[1], g), ints((N, K, P, Q), md, g)


def conv_refs(x, w, dy, stride, pad, dtype=torch.float32, want=("y", "dx", "dw")):
    """The exact forward / input gradient / weight gradient on the CPU in `dtype`."""
    out = {}
    x, w, dy = x.to(dtype), w.to(dtype), dy.to(dtype)
    if "y" in want:
        out["y"] = F.conv2d(x, w, stride=stride, padding=pad)
    if "dx" in want:
        out["dx"] = torch.nn.grad.conv2d_input(x.shape, w, dy, stride=stride, padding=pad)
    if "dw" in want:
        out["dw"] = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=stride, padding=pad)
    return out


def assert_fp32_is_exact(x, w, dy, stride, pad):
    """fp32 == fp64 on the CPU (run at the smallest shape of a family; the bound covers the rest)."""
    a = conv_refs(x, w, dy, stride, pad, torch.float32)
    b = conv_refs(x, w, dy, stride, pad, torch.float64)
    for k in a:
        assert torch.equal(a[k].double(), b[k]), f"fp32 CPU reference of {k} is not exact"
        assert float(b[k].abs().max()) < LIMIT


def bf16_census(ref):
    """Fractions of a reference tensor: not representable in bf16, exact ties, truncation != RNE."""
    r = ref.float()
    up = rne(r)
    lo = trunc(r)
    inexact = up != r
    # a tie: the value sits midway between its two bf16 neighbours (lo and lo + one bf16 ulp)
    hi = (lo.contiguous().view(torch.int32) + 65536).view(torch.float32)
    tie = inexact & ((r - lo).abs() == (hi - r).abs())
    return dict(inexact=float(inexact.float().mean()), ties=float(tie.float().mean()),
                trunc_ne_rne=frac_ne(lo, up))


def wrong_references(ref, half=None, addend=None):
    """The wrong results a subtly broken bf16 kernel would give, from the exact fp32 `ref`
    (addend included when there is one): name -> bf16-valued fp32 tensor.
      truncated      : the store drops the low bits instead of rounding to nearest even
      double_rounded : the contraction rounded to bf16, then the addend added and rounded again
      half_k_bf16    : one half of the reduction (`half`, exact) handed on as bf16, not fp32"""
    out = {"truncated": trunc(ref)}
    if addend is not None:
        out["double_rounded"] = rne(rne(ref - addend) + addend)
    if half is not None:
        out["half_k_bf16"] = rne(rne(half) + (ref - half))
    return out


def assert_discriminates(ref, half=None, addend=None, floor=0.01, what=""):
    """Each wrong reference differs from the true one in at least `floor` of the elements - a
    condition on the inputs (ranges, seeds), checked before anything runs on the GPU.  Returns the
    measured fractions."""
    true = rne(ref)
    fr = {k: frac_ne(v, true) for k, v in wrong_references(ref, half, addend).items()}
    for k, f in fr.items():
        assert f >= floor, f"{what}: the {k} reference differs in only {f:.4f} of the elements"
    return fr


def pow2_coefficients(G, K, gen):
    """sc = +-2^e, e in {-2..2}, both signs; integer sh in [-8, 8]: fp32 [G, K] each."""
    e = torch.randint(-2, 3, (G, K), generator=gen).float()
    sign = torch.randint(0, 2, (G, K), generator=gen).float() * 2 - 1
    sc = sign * torch.pow(torch.tensor(2.0), e)
    assert bool((sc > 0).any()) and bool((sc < 0).any())
    return sc, ints((G, K), 8, gen)


def ulps_rel(got, ref64):
    """max |got - ref| / |ref| over the elements (ref in float64; 0 must be met exactly)."""
    got, ref64 = got.detach().double().cpu(), ref64.double()
    zero = ref64 == 0
    assert bool((got[zero] == 0).all())
    d = (got - ref64).abs()[~zero] / ref64.abs()[~zero]
    return float(d.max()) if d.numel() else 0.0
