"""References, operand recipes, bounds, mutants and launch plans for the MMTM site kernels
(csrc/mmtm_kernels.hip: k_rowreduce_nchw, k_colreduce_nhwc + k_reduce_partials, k_channel_scale,
k_running_avg, k_running_avg_dev) and the gate's three MMTM kernels (csrc/gate.hip: k_select_scale,
k_mask_rows, k_mask_rows2).  Used by tests/test_cpu_mmtmref.py (every condition below, no GPU) and
tests/test_gpu_mmtm_forms.py.  Everything here runs on the CPU.

Exact tier.  Operands on which every intermediate is exact in fp32 under any summation order and any
fma contraction, so a correct kernel equals the fp64 value, rounded once where it stores bf16:

  squeeze / squeeze backward   x, dy nonzero integers |v| <= 3 (a dropped or doubled element always
                               moves the sum), scale a power of two, e = k / 16 with 1 <= k <= 15:
                               out = scale * S * k (16 - k) / 256 with S the integer sum, and
                               max|S| * 64 < 2^24 is asserted per case (k (16 - k) <= 64).
  channel scale                x = m / 16 with 1 <= |m| <= 255 (a bf16 number), s = j / 1024 with
                               0 <= j <= 1024, a = n / 8 with |n| <= 64, alpha = 1/4:
                               y = (m j + 512 n) / 2^14, numerator below 2^24.  Channels c % 4 == 1
                               hold planted ties: odd m in [87, 169], s = 1.5, a = 0, so 3 m is an odd
                               9-bit integer, exactly half-way between two bf16 numbers.
  running averages             e and the old averages multiples of 2^-8 in [0, 1], B and step + 1
                               powers of two.

Bounded tier.  N(0, 1) activations, sigmoid scales, scale = alpha = 1 / HW, against fp64 with
u = 2^-24 and gamma_n = n u / (1 - n u):

  reduce        gamma_{HW+3} |scale| |e (1 - e)| sum_i |t_i|        (any summation order)
  scale         3 u (|x s| + |alpha a|), plus half a bf16 ulp of the reference in bf16
  running avg   gamma_{B+4} (|m| + |ra_old|)

Mutants are applied to the expected value; each must change (exact tier) or violate the bound on
(bounded tier) at least FLOOR of the checked outputs, or the case / mutant pair is in NOT_CHECKED.

Launch plans.  nhwc_plan restates red_setup (mmtm_kernels.hip:461-516), colreduce_instance the
dispatch of spatial_reduce_impl (:575-586), row_width the width loop of red_setup (:484-489),
scale_plan the choice of channel_scale_impl (:624-638, :665-684).
"""
import functools
import types
import zlib

import numpy as np
import torch

import exactint as X
from bnregimes import FLOOR

BF16 = torch.bfloat16
DT = {"bf16": BF16, "f32": torch.float32}
ES = {"bf16": 2, "f32": 4}
U = 2.0 ** -24
NCHW, NHWC = "nchw", "nhwc"


def gamma(n):
    return n * U / (1.0 - n * U)


def rha(t):
    """fp32 -> bf16 rounding halves away from zero (a wrong store), as fp32."""
    b = t.float().contiguous().view(torch.int32)
    return ((b + 0x8000) & -65536).view(torch.float32)


def half_ulp_bf16(ref):
    """Half a bf16 ulp at |ref| (fp64 tensor)."""
    _, ex = torch.frexp(ref.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(ref), ex - 9)


def used(err, bound):
    """The largest fraction of a bound that is used (inf for a non-finite error)."""
    err, bound = err.double(), bound.double()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(err), r, torch.full_like(err, float("inf")))
    return float(r.max())


def violation_rate(err, bound):
    return float((~(err.double() <= bound.double())).double().mean())


def same(a, b):
    """Equal with NaN exactly where the other has NaN."""
    a, b = a.double(), b.double()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def frac_ne(a, b):
    a, b = a.double(), b.double()
    return float((~((a == b) | (torch.isnan(a) & torch.isnan(b)))).double().mean())


# ---- launch plans -----------------------------------------------------------------------------------

RED_WGS = 128                       # red_wgs()
FORMS = [(256, 4), (256, 8), (256, 16), (1024, 4), (1024, 8), (-256, 4), (-256, 8), (-1024, 4)]
DEFAULT_FORM = (-256, 4)


def colreduce_instance(dtype, bwd, form):
    """(U, NTH, NT) of the k_colreduce_nhwc instantiation a form selects."""
    threads, unroll = form
    nt, nth = threads < 0, abs(threads)
    wide = nth == 1024
    if dtype == "bf16" and not bwd and nt:
        return (4, 1024, True) if wide else ((8, 256, True) if unroll >= 8 else (4, 256, True))
    if dtype == "f32":
        return (4, 1024, False) if wide else ((8, 256, False) if unroll >= 8 else (4, 256, False))
    if wide:
        return (8 if unroll >= 8 else 4, 1024, False)
    return (16 if unroll >= 16 else 8 if unroll >= 8 else 4, 256, False)


def nhwc_plan(C, HW, B, es, nth=256):
    """The host plan of one NHWC problem: channel slabs, threads per pixel, pixels per iteration,
    splits, pixels per thread (min, max over the pixel lanes) in a full and in the last split, the
    second-level reduction's R, the idle lanes and the partials' bytes."""
    assert (C * es) % 16 == 0 and (C * es <= 4096 or (C * es) % 4096 == 0)
    cw = C if C * es <= 4096 else 4096 // es
    ncs = C // cw
    tpp = cw * es // 16
    ppi = nth // tpp
    S = -(-(RED_WGS // 2) // B)
    maxS = (HW + 2 * ppi - 1) // (2 * ppi)
    S = max(1, min(S, maxS))
    hw_per = -(-HW // S)
    S = -(-HW // hw_per)
    last = HW - (S - 1) * hw_per
    ppt = lambda n: (n // ppi, -(-n // ppi))  # noqa: E731
    return types.SimpleNamespace(cw=cw, ncs=ncs, tpp=tpp, ppi=ppi, S=S, hw_per=hw_per, last=last,
                                 ppt_full=ppt(hw_per), ppt_last=ppt(last), R=nth // cw if cw <= nth else 1,
                                 idle=nth - tpp * ppi, scratch=B * S * C * 4 if S > 1 else 0)


def trips(n, unroll):
    """Trips of the U-pixel loop, the four-pixel loop (U > 4) and the one-pixel tail for n pixels."""
    main, r = divmod(n, unroll)
    four = r // 4 if unroll > 4 else 0
    return main, four, r - 4 * four


def depth_label(n, unroll):
    main, four, tail = trips(n, unroll)
    if n == 0:
        return "0"
    if n <= 3:
        return "1-3"
    if n == unroll:
        return "U"
    if (main, four) == (1, 1) and tail:
        return "U+4+t"
    if (main, four) == (2, 0) and tail:
        return "2U+t"
    return "other"


def depth_hws(unroll, ppi):
    """Pixel counts (S = 1) whose threads get 0-1, 2-3, exactly U, U + 4 + a tail (U > 4) and
    2U + a tail pixels."""
    hws = [ppi - 3, 3 * ppi - 5, unroll * ppi]
    if unroll > 4:
        hws.append((unroll + 5) * ppi + 5)
    hws.append((2 * unroll + 1) * ppi + 5)
    return hws


def depth_labels(hw, unroll, ppi):
    return {depth_label(n, unroll) for n in range(hw // ppi, -(-hw // ppi) + 1)}


def row_width(probs, es):
    """Vector bytes of a k_rowreduce_nchw launch: probs = [(HW, x address % 16, dy address % 16 or None)]."""
    vb = 16
    for hw, xa, da in probs:
        while vb > es and ((hw * es) % vb or xa % vb or (da is not None and da % vb)):
            vb >>= 1
    return vb


def row_trips(hw, es, vb):
    return -(-(hw * es // vb) // 64)


def scale_plan(probs, B, es, layout, add):
    """(elements per thread, form) of a k_channel_scale launch; probs: dicts with C, HW and the
    optional x_off / s_off / a_off (elements) and ld_s / ld_a as the launch gets them."""
    n = 16 // es
    rowconst = True
    for p in probs:
        numel = B * p["C"] * p["HW"]
        if (p.get("x_off", 0) * es) % 16 or numel % n:
            n = 1
        if layout == NHWC and (p["C"] % n or (p.get("s_off", 0) * 4) % 16 or p["ld_s"] % 4 or
                               (add and ((p.get("a_off", 0) * 4) % 16 or p["ld_a"] % 4))):
            n = 1
        if layout == NCHW and p["HW"] % n:
            rowconst = False
    if n == 1:
        return 1, "one"
    return n, "vec" if layout == NHWC or rowconst else "lookup"


# ---- squeeze and squeeze backward: cases --------------------------------------------------------------

RED_SCALE = 2.0 ** -5


def _p(C, HW, **kw):
    return dict(C=C, HW=HW, **kw)


# k_rowreduce_nchw: name -> (dtype, B, problems, vector bytes (or forward, backward), lane-loop trips of problem 0).  x_off / dy_off:
# the tensor starts that many elements into a 256-byte aligned buffer; e0: the e row is broadcast (ld_e = 0)
ROW_CASES = {
    "bf16-w16": ("bf16", 3, [_p(5, 8)], 16, 1),
    "bf16-w8": ("bf16", 3, [_p(5, 4, e0=True)], 8, 1),
    "bf16-w4": ("bf16", 3, [_p(5, 6)], 4, 1),
    "bf16-w2": ("bf16", 3, [_p(5, 7)], 2, 1),
    "bf16-w8-base": ("bf16", 3, [_p(5, 8, x_off=4)], 8, 1),
    "bf16-w4-base": ("bf16", 3, [_p(5, 8, x_off=2, dy_off=8)], 4, 1),
    "bf16-w8-dy": ("bf16", 3, [_p(5, 8, dy_off=4)], (16, 8), 1),
    "bf16-w2-base": ("bf16", 3, [_p(5, 8, x_off=1, e0=True)], 2, 1),
    "bf16-w2-trips": ("bf16", 2, [_p(3, 169)], 2, 3),
    "bf16-2prob": ("bf16", 3, [_p(5, 8), _p(3, 12, e0=True)], 8, 1),
    "bf16-4prob": ("bf16", 2, [_p(5, 16), _p(3, 12), _p(7, 6, e0=True), _p(2, 40)], 4, 1),
    "f32-w16": ("f32", 3, [_p(5, 4)], 16, 1),
    "f32-w8": ("f32", 3, [_p(5, 6, e0=True)], 8, 1),
    "f32-w4": ("f32", 3, [_p(5, 7)], 4, 1),
    "f32-w8-base": ("f32", 3, [_p(5, 8, x_off=2)], 8, 1),
    "f32-w4-base": ("f32", 3, [_p(5, 8, x_off=1, dy_off=4, e0=True)], 4, 1),
    "f32-w8-dy": ("f32", 3, [_p(5, 8, dy_off=2)], (16, 8), 1),
    "f32-w4-trips": ("f32", 2, [_p(3, 169)], 4, 3),
    "f32-3prob": ("f32", 2, [_p(5, 8), _p(3, 6), _p(4, 20, e0=True)], 8, 1),
}


def row_case_wanted(name, bwd):
    w = ROW_CASES[name][3]
    return w[int(bwd)] if isinstance(w, tuple) else w


def row_case_width(name, bwd):
    dtype, B, probs, _, _ = ROW_CASES[name]
    es = ES[dtype]
    return row_width([(p["HW"], p.get("x_off", 0) * es % 16, p.get("dy_off", 0) * es % 16 if bwd else None)
                      for p in probs], es)


# k_colreduce_nhwc: name -> (B, problems per dtype, what the case is there to reach).  Every case runs
# under every form; the depth cases (pixels per thread at S = 1) are made per form by depth_case().
COL_CASES = {
    "split11": (1, {"bf16": [_p(64, 700)], "f32": [_p(64, 700)]}, "S > 1, last split shorter"),
    "split22": (3, {"bf16": [_p(128, 784, e0=True)], "f32": [_p(128, 784, e0=True)]}, "S > 1, last split shorter"),
    "idle24": (2, {"bf16": [_p(24, 300)], "f32": [_p(12, 300)]}, "idle lanes, R = 10 / 21"),
    "idle40": (2, {"bf16": [_p(40, 77)], "f32": [_p(40, 77)]}, "idle lanes, R = 6"),
    "slab1": (2, {"bf16": [_p(2048, 7)], "f32": [_p(1024, 7)]}, "one 4096-byte slab: R = 1"),
    "slab2": (2, {"bf16": [_p(4096, 6), _p(4096, 9, e0=True)], "f32": [_p(2048, 6), _p(2048, 9, e0=True)]},
              "two slabs"),
    "mixedS": (1, {"bf16": [_p(64, 700), _p(128, 8)], "f32": [_p(64, 700), _p(64, 8)]}, "S > 1 with S == 1"),
    "four": (2, {"bf16": [_p(64, 700), _p(128, 8, e0=True), _p(24, 50), _p(2048, 5)],
                 "f32": [_p(64, 700), _p(64, 8, e0=True), _p(12, 50), _p(1024, 5)]}, "four shapes"),
}
DEPTH_C = {"bf16": 128, "f32": 64}      # 16 threads per pixel
DEPTH_B = 64                            # S = 1 from here up


def depth_case(dtype, bwd, form):
    """Two launches of S = 1 problems (B = 64) whose pixel counts reach every loop class of the
    instantiation the form selects: [[problem, ...], [problem, ...]] and the labels they reach."""
    unroll, nth, _ = colreduce_instance(dtype, bwd, form)
    C = DEPTH_C[dtype]
    ppi = nth // (C * ES[dtype] // 16)
    hws = depth_hws(unroll, ppi)
    labels = set()
    for hw in hws:
        assert nhwc_plan(C, hw, DEPTH_B, ES[dtype], nth).S == 1
        labels |= depth_labels(hw, unroll, ppi)
    return [[_p(C, hw) for hw in hws[:3]], [_p(C, hw) for hw in hws[3:]]], labels


def depth_labels_wanted(unroll):
    return {"0", "1-3", "U", "2U+t"} | ({"U+4+t"} if unroll > 4 else set())


# ---- squeeze and squeeze backward: operands and expected values -------------------------------------------

def _nonzero_ints(shape, mag, g):
    m = torch.randint(1, mag + 1, shape, generator=g, dtype=torch.int8)
    return m * (torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1)


def reduce_operands(B, C, HW, seed):
    """x, dy int8 [B, C, HW] (nonzero, |v| <= 3) and k int64 [B, C] with e = k / 16."""
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(B=B, C=C, HW=HW, x=_nonzero_ints((B, C, HW), 3, g), dy=_nonzero_ints((B, C, HW), 3, g),
                                 k=torch.randint(1, 16, (B, C), generator=g))


def reduce_sum(o, bwd, drop=None):
    """The integer sum per (b, c): int64 [B, C].  drop: pixel indices left out (a mutant)."""
    t = o.x.short() * o.dy.short() if bwd else o.x.short()
    s = t.sum(-1, dtype=torch.int64)
    if drop is not None:
        s = s - t[:, :, drop].sum(-1, dtype=torch.int64)
    return s


def reduce_expected(o, bwd, e0=False, with_e=None, scale=RED_SCALE, drop=None, e_plain=False):
    """fp64 [B, C]: scale * S * e (1 - e) (backward; e row 0 broadcast with e0) or scale * S."""
    with_e = bwd if with_e is None else with_e
    s = reduce_sum(o, bwd, drop)
    assert int(s.abs().max()) * 64 < X.LIMIT, "exact tier: |sum| * bits(e (1 - e)) reaches 2^24"
    out = s.double() * scale
    if with_e:
        k = (o.k[:1] if e0 else o.k).double()
        out = out * (k / 16 if e_plain else k * (16 - k) / 256)
    return out


def split_last_pixels(HW, plan):
    return [min(HW, (s + 1) * plan.hw_per) - 1 for s in range(plan.S)]


def reduce_mutants(o, bwd, e0, layout, es):
    """name -> the fp64 expected value a wrong kernel would give."""
    drop = split_last_pixels(o.HW, nhwc_plan(o.C, o.HW, o.B, es)) if layout == NHWC else [o.HW - 1]
    out = {"drop_last": reduce_expected(o, bwd, e0, drop=drop), "no_scale": reduce_expected(o, bwd, e0, scale=1.0)}
    if bwd:
        out["e_plain"] = reduce_expected(o, bwd, e0, e_plain=True)
    return out


def reduce_bounded(B, C, HW, dtype, bwd, seed):
    """Realistic operands (as the dtype holds them), the fp64 reference and its bound: x, dy fp32
    tensors [B, C, HW] holding dtype values, e [B, C], scale, ref, bound."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, HW, generator=g).to(DT[dtype]).float()
    dy = torch.randn(B, C, HW, generator=g).to(DT[dtype]).float()
    e = torch.sigmoid(torch.randn(B, C, generator=g))
    scale = 1.0 / HW
    t = x.double() * dy.double() if bwd else x.double()
    f = (e.double() * (1 - e.double())) if bwd else torch.ones(B, C, dtype=torch.float64)
    ref = scale * t.sum(-1) * f
    bound = gamma(HW + 3) * scale * f.abs() * t.abs().sum(-1)
    return types.SimpleNamespace(x=x, dy=dy, e=e, scale=scale, ref=ref, bound=bound, bwd=bwd)


def reduce_fp32_emulation(c, reverse=False):
    """The bounded reference's own operands summed sequentially in fp32 (forward or reverse pixel
    order) with the kernel's epilogue in fp32: fp64 tensor [B, C] of fp32 values."""
    t = (c.x.numpy() * c.dy.numpy()).astype(np.float32) if c.bwd else c.x.numpy()
    t = t[:, :, ::-1] if reverse else t
    s = np.cumsum(t, axis=-1, dtype=np.float32)[:, :, -1]
    s = (s * np.float32(c.scale)).astype(np.float32)
    e = c.e.numpy().astype(np.float32)
    if c.bwd:
        s = (s * ((np.float32(1) - e) * e).astype(np.float32)).astype(np.float32)
    return torch.from_numpy(s.astype(np.float64))


# ---- channel scale -------------------------------------------------------------------------------------------

ALPHA = 0.25

# name -> (layout, B, problems).  pad_s: ld_s = C + pad_s; s0: ld_s = 0 (row 0 broadcast)
SCALE_CASES = {
    "nchw-vec": (NCHW, 3, [_p(5, 16)]),
    "nchw-one": (NCHW, 3, [_p(5, 7)]),
    "nchw-lookup": (NCHW, 2, [_p(4, 9)]),
    "nchw-bcast": (NCHW, 3, [_p(5, 16, s0=True)]),
    "nchw-offs": (NCHW, 3, [_p(5, 16, s_off=1, a_off=3, pad_s=2)]),
    "nchw-xoff": (NCHW, 3, [_p(5, 16, x_off=1)]),
    "nchw-3prob": (NCHW, 2, [_p(4, 16), _p(6, 8), _p(3, 24, s0=True)]),
    "nchw-4prob-lookup": (NCHW, 2, [_p(4, 9), _p(2, 16), _p(8, 3), _p(4, 6)]),
    "nhwc-vec": (NHWC, 3, [_p(16, 5)]),
    "nhwc-one": (NHWC, 3, [_p(5, 7)]),
    "nhwc-bcast": (NHWC, 3, [_p(16, 5, s0=True)]),
    "nhwc-soff": (NHWC, 3, [_p(16, 5, s_off=1)]),
    "nhwc-aoff": (NHWC, 3, [_p(16, 5, a_off=2)]),
    "nhwc-ldpad": (NHWC, 3, [_p(16, 5, pad_s=2)]),
    "nhwc-3prob": (NHWC, 2, [_p(16, 5), _p(8, 9), _p(32, 2, s0=True)]),
    "nhwc-4prob-one": (NHWC, 2, [_p(16, 5), _p(8, 9), _p(5, 3), _p(24, 2)]),
}
# the form each case is there to reach: (dtype, additive term) -> form; a plain string holds for all four
SCALE_FORM = {
    "nchw-vec": "vec", "nchw-one": "one", "nchw-lookup": "lookup", "nchw-bcast": "vec", "nchw-offs": "vec",
    "nchw-xoff": "one", "nchw-3prob": "vec", "nchw-4prob-lookup": "lookup",
    "nhwc-vec": "vec", "nhwc-one": "one", "nhwc-bcast": "vec", "nhwc-soff": "one",
    "nhwc-aoff": {("bf16", False): "vec", ("f32", False): "vec", ("bf16", True): "one", ("f32", True): "one"},
    "nhwc-ldpad": "one", "nhwc-3prob": "vec", "nhwc-4prob-one": "one",
}


def scale_launch_fields(p):
    """ld_s, ld_a of a problem as the launch gets them."""
    return dict(p, ld_s=0 if p.get("s0") else p["C"] + p.get("pad_s", 0), ld_a=p["C"])


def scale_case_form(name, dtype, add):
    layout, B, probs = SCALE_CASES[name]
    return scale_plan([scale_launch_fields(p) for p in probs], B, ES[dtype], layout, add)


def scale_operands(B, C, HW, seed):
    """Integer numerators: m int64 [B, C, HW] (x = m / 16), j [B, C] (s = j / 1024), n [B, C]
    (a = n / 8) and alt [C] (the substituted row, alt / 1024).  Channels c % 4 == 1 hold the ties."""
    g = torch.Generator().manual_seed(seed)
    sign = lambda shape: torch.randint(0, 2, shape, generator=g) * 2 - 1  # noqa: E731
    m = torch.randint(1, 256, (B, C, HW), generator=g) * sign((B, C, HW))
    j = torch.randint(0, 1025, (B, C), generator=g)
    n = torch.randint(-64, 65, (B, C), generator=g)
    alt = torch.randint(0, 1025, (C,), generator=g)
    tie = torch.arange(C) % 4 == 1
    odd = (torch.randint(43, 85, (B, C, HW), generator=g) * 2 + 1) * sign((B, C, HW))      # odd, 87 .. 169
    m[:, tie] = odd[:, tie]
    j[:, tie] = 1536
    n[:, tie] = 0
    return types.SimpleNamespace(B=B, C=C, HW=HW, m=m, j=j, n=n, alt=alt,
                                 x=m.double() / 16, s=j.double() / 1024, a=n.double() / 8, alt_s=alt.double() / 1024)


def scale_numerator(o, add, s0=False, alt=False, alpha_num=512):
    """The exact y * 2^14 as int64 [B, C, HW]: m j + 512 n."""
    j = o.alt.view(1, -1).expand(o.B, -1) if alt else (o.j[:1].expand(o.B, -1) if s0 else o.j)
    num = o.m * j[:, :, None]
    if add:
        num = num + alpha_num * o.n[:, :, None]
    assert int(num.abs().max()) < X.LIMIT
    return num


def scale_expected(o, add, s0=False, alt=False, alpha_num=512):
    """fp64 [B, C, HW], exact (and exact in fp32)."""
    return scale_numerator(o, add, s0, alt, alpha_num).double() / 2.0 ** 14


def store(ref64, dtype, how="rne"):
    """The stored value of an exact fp64 result: fp32, then one rounding to bf16 (as fp32)."""
    r = ref64.float()
    assert torch.equal(r.double(), ref64), "not exact in fp32"
    if dtype == "f32":
        return r
    return {"rne": X.rne, "trunc": X.trunc, "rha": rha}[how](r)


def scale_mutants(o, add, s0, dtype):
    """name -> the stored tensor a wrong kernel would give."""
    out = {}
    ref = scale_expected(o, add, s0)
    if dtype == "bf16":
        out["trunc"] = store(ref, dtype, "trunc")
        out["half_away"] = store(ref, dtype, "rha")
    if add:
        out["no_alpha"] = store(scale_expected(o, add, s0, alpha_num=2048), dtype)     # a, not alpha * a
    return out


def scale_bounded(B, C, HW, dtype, add, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, HW, generator=g).to(DT[dtype]).float()
    s = torch.sigmoid(torch.randn(B, C, generator=g))
    a = torch.randn(B, C, generator=g)
    alpha = 1.0 / HW
    xs = x.double() * s.double()[:, :, None]
    aa = (alpha * a.double())[:, :, None].expand_as(xs) if add else torch.zeros_like(xs)
    ref = xs + aa
    bound = 3 * U * (xs.abs() + aa.abs())
    if dtype == "bf16":
        bound = bound + half_ulp_bf16(ref)
    return types.SimpleNamespace(x=x, s=s, a=a, alpha=alpha, ref=ref, bound=bound)


# ---- the gate ----------------------------------------------------------------------------------------------------

# (label, curation_mode, caring)
GATE_STATES = [("off-c0", 0, 0), ("off-c1", 0, 1), ("cur-none", 1, -1), ("cur-c0", 1, 0), ("cur-c1", 1, 1)]
GATE_STATES_N = GATE_STATES + [("cur-c2", 1, 2)]
MODS2 = [0, 1, -2, -2]              # the two-modality entry points' own table
MODS_N = {"with": [2, 0, -2, 2], "without": [0, 1, -2, 3]}


def substituted(cur, caring, mods):
    """The rule of the gated launches: problem i is substituted iff curating and mods[i] == caring >= 0."""
    sub = caring if cur else -1
    return [sub >= 0 and m == sub for m in mods]


def gate_mutant_flags(flags):
    """name -> the flags a wrong launch would act on."""
    n = len(flags)
    return {"no_subst": [False] * n, "subst_shift": [flags[(i - 1) % n] for i in range(n)],
            "zero_wrong": [flags[(i + 1) % n] for i in range(n)]}


def select_scale_rule(e_v, e_s, ra_v, ra_s, cur, caring):
    """gm_mmtm_select_scale by the header: (s_v, s_s, mask)."""
    B = e_v.shape[0]
    sub_v, sub_s = bool(cur) and caring == 0, bool(cur) and caring == 1
    s_v = ra_v[None].expand(B, -1) if sub_v else e_v
    s_s = ra_s[None].expand(B, -1) if sub_s else e_s
    return s_v, s_s, torch.tensor([0.0 if sub_v else 1.0, 0.0 if sub_s else 1.0])


# gated launches: name -> (kind, base case, entry point "2" / "n", mods).  kind "scale": SCALE_CASES name;
# "row": ROW_CASES name; "col": COL_CASES name
GATED_CASES = {
    "scale-nchw-3prob": ("scale", "nchw-3prob", "2", MODS2[:3]),
    "scale-nhwc-3prob": ("scale", "nhwc-3prob", "2", MODS2[:3]),
    "scale-nhwc-4prob-one": ("scale", "nhwc-4prob-one", "n", MODS_N["with"]),
    "scale-nhwc-4prob-one-without": ("scale", "nhwc-4prob-one", "n", MODS_N["without"]),
    "scale-nchw-4prob": ("scale", "nchw-4prob-lookup", "n", MODS_N["with"]),
    "row-2prob": ("row", "bf16-2prob", "2", MODS2[:2]),
    "row-4prob": ("row", "bf16-4prob", "n", MODS_N["with"]),
    "row-3prob-f32": ("row", "f32-3prob", "n", MODS_N["without"][:3]),
    "col-mixedS": ("col", "mixedS", "2", MODS2[:2]),
    "col-four": ("col", "four", "n", MODS_N["with"]),
    "col-four-without": ("col", "four", "n", MODS_N["without"]),
}
GATE_MUTANTS = {"scale": ["no_subst", "subst_shift"], "row": ["zero_wrong"], "col": ["zero_wrong"]}


def gated_states(name):
    return GATE_STATES if GATED_CASES[name][2] == "2" else GATE_STATES_N


def _not_checked():
    out = {}
    for name, (kind, _, _, mods) in GATED_CASES.items():
        for label, cur, caring in gated_states(name):
            if not any(substituted(cur, caring, mods)):
                for mut in GATE_MUTANTS[kind]:
                    out[name, label, mut] = "no problem of this launch is substituted in this state"
    return out


# (case, state, mutant) pairs that cannot show the mutant, with the reason.  Everything else must reach FLOOR.
NOT_CHECKED = _not_checked()


# ---- running averages --------------------------------------------------------------------------------------------

RA_C = [1, 63, 64, 65, 256, 257, 600]
RA_EXACT = [(B, step) for B in (1, 4, 16, 32) for step in (0, 7, 1023)]
RA_BOUNDED = [(B, step) for B in (1, 3, 4, 5, 15, 16, 17, 33) for step in (0, 1000)]


def ra_operands(B, C, ld, seed, exact):
    """e [B, ld] (columns past C are NaN: never read), e_s [B, C] (the other modality's scale, for the
    own-mean mutant), the old averages rv, rs [C]."""
    g = torch.Generator().manual_seed(seed)
    if exact:
        draw = lambda *s: torch.randint(0, 257, s, generator=g).float() / 256  # noqa: E731
    else:
        draw = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    e = torch.full((B, ld), float("nan"))
    e[:, :C] = draw(B, C)
    return types.SimpleNamespace(B=B, C=C, e=e, e_s=draw(B, C), rv=draw(C), rs=draw(C))


def ra_expected(o, step, own_mean=False, div_step=False):
    """The fp64 recurrence of the header: both averages follow the visual scale's batch mean."""
    m = o.e[:, :o.C].double().mean(0)
    ms = o.e_s.double().mean(0) if own_mean else m
    with np.errstate(all="ignore"):
        d = float(step) if div_step else float(step + 1)
        return (m + o.rv.double() * step) / d, (ms + o.rs.double() * step) / d


def ra_bound(o):
    m = o.e[:, :o.C].double().mean(0)
    return gamma(o.B + 4) * (m.abs() + o.rv.double().abs()), gamma(o.B + 4) * (m.abs() + o.rs.double().abs())


def ra_fp32_emulation(o, step):
    """k_running_avg's arithmetic in fp32 on the CPU: four partial sums over b = w, w + 4, ...,
    ((p0 + p1) + p2) + p3, / B, (m + r * k) / k1 without contraction."""
    e = o.e[:, :o.C].numpy().astype(np.float32)
    p = [np.zeros(o.C, np.float32) for _ in range(4)]
    for b in range(o.B):
        p[b & 3] = (p[b & 3] + e[b]).astype(np.float32)
    m = (((p[0] + p[1]) + p[2]) + p[3]).astype(np.float32) / np.float32(o.B)
    k, k1 = np.float32(step), np.float32(step + 1)
    f = lambda r: torch.from_numpy((((m + (r.numpy() * k).astype(np.float32)).astype(np.float32)) / k1)  # noqa: E731
                                   .astype(np.float64))
    return f(o.rv), f(o.rs)


def fmt(d):
    return ", ".join(f"{k} {v:.3f}" for k, v in d.items())


# ---- whole cases: operands and expected values per problem -------------------------------------------------------

def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=32)
def _reduce_ops(B, C, HW, i):
    return reduce_operands(B, C, HW, seed_of("reduce", B, C, HW, i))


def reduce_case_operands(B, probs):
    return [_reduce_ops(B, p["C"], p["HW"], i) for i, p in enumerate(probs)]


def reduce_case_expected(B, probs, bwd, flags=None):
    """fp64 [B, C] per problem; a problem whose flag is set (substituted under the gate) is all 0."""
    out = []
    for i, (p, o) in enumerate(zip(probs, reduce_case_operands(B, probs))):
        r = reduce_expected(o, bwd, p.get("e0", False))
        out.append(torch.zeros_like(r) if flags and flags[i] else r)
    return out


def col_problems(name, dtype):
    B, by_dtype, _ = COL_CASES[name]
    return B, by_dtype[dtype]


def gated_problems(name, dtype=None):
    """(kind, dtype, layout, B, problems, mods) of a gated case; dtype is free for the col cases."""
    kind, base, _, mods = GATED_CASES[name]
    if kind == "scale":
        layout, B, probs = SCALE_CASES[base]
        return kind, dtype, layout, B, probs, mods
    if kind == "row":
        dt, B, probs, _, _ = ROW_CASES[base]
        return kind, dt, NCHW, B, probs, mods
    B, probs = col_problems(base, dtype)
    return kind, dtype, NHWC, B, probs, mods


@functools.lru_cache(maxsize=None)
def _scale_ops(B, C, HW, i):
    return scale_operands(B, C, HW, seed_of("scale", B, C, HW, i))


def scale_case_operands(name):
    _, B, probs = SCALE_CASES[name]
    return [_scale_ops(B, p["C"], p["HW"], i) for i, p in enumerate(probs)]


def scale_case_expected(name, dtype, add, flags=None, how="rne"):
    """The stored y per problem, [B, C, HW] as fp32; a flagged problem scales by its alt row."""
    _, B, probs = SCALE_CASES[name]
    return [store(scale_expected(o, add, p.get("s0", False), alt=bool(flags and flags[i])), dtype, how)
            for i, (p, o) in enumerate(zip(probs, scale_case_operands(name)))]


def cat(ts):
    return torch.cat([t.reshape(-1).double() for t in ts])
