"""BatchNorm inputs that exercise every term, a closed-form fp64 reference and per-element bounds
(tests/test_cpu_bnregimes.py, tests/test_gpu_bn_regimes.py).  Everything here runs on the CPU.

Inputs.  The regime of channel c is c % 8, so every legal C (a power of two >= 8) holds all eight:

    r  x                                gamma          probes
    0  bf16(N(0.3, 1.7))                U(0.5, 1.5)    the ordinary case
    1  16 + k/8,  k in [-8, 8]          U(0.5, 1.5)    |mean|/std ~ 26, every value exact in bf16
    2  1 + k/128, k in [-2, 2]          U(0.5, 1.5)    var ~ 1.2e-4: eps moves invstd by 4 %
    3  16                               U(0.5, 1.5)    var = 0, invstd = eps^-1/2, cb = 0
    4  as 0                             -U(0.5, 1.5)   negative scale
    5  as 0                             0              y = beta, dx = 0, dgamma != 0
    6  as 0                             2^-10          a channel a max-norm cannot see
    7  -16 + k/8                        32             large scale, negative offset

beta = +-U(0.1, 0.5), positive where (c // 8) is even and negative where it is odd (so, from
C = 16 on, half of the gamma = 0 channels sit on either side of the ReLU), and never so close to 0
that a constant or gamma = 0 channel falls into the rounding band of the ReLU.  The gradient is
dy = bf16(0.75 + 0.5 clamp(xhat, +-4) + 0.5 N(0, 1)): nonzero mean and correlated with xhat, so the
three terms of dx = gamma is (dz - mean(dz) - xhat mean(dz xhat)) have comparable size.

Regimes 1, 2, 3 and 7 are dyadic: x and x^2 are integer multiples of 2^-3 / 2^-7 and their squares,
so every fp32 partial sum of x and x^2 is exact under any partition while M max|x / unit|^2 < 2^24.
build() asserts that on the shapes it reports as `exact` (M <= 693).

Bounds (u8 = 2^-8, u24 = 2^-24; per element, derived, not fitted):

  forward   |y - ref| <= u8 |ref| + 4 u24 (|x sc| + |sh|) + u24 |res|
            one round-to-nearest bf16 store (half an ulp <= u8 of the value), then the fp32
            roundings of sc, sh, the fma and the residual add.  fp32 outputs: no u8 term.
  backward  |dx - ref| <= u8 |ref| + K u24 A,
            A = |g is| (|dz| + mean|dz|) + |g is^3| mean|dz (x - mean)| (|x| + |mean|)
            K = 16 + the longest fp32 addition chain of the partial sums (rows per thread + rows
            per pass, chain()); K = 16 where every partial sum is exact or fp64 (the fp32 path,
            the emulation).  The sums of dz are fp32 sums of arbitrary bf16 values on every
            shape, the exact-sum ones included, so the bf16 paths always carry the chain.
            dres is dz itself: exact.
  dbeta     K u24 sum|dz| + u24 |ref|
  dgamma    K u24 is sum|dz| (|x| + |mean|) + u24 |ref|.  The terms summed are dz x and dz mean:
            the kernels (and the ABI: save_mean is fp32) form dz (x - float(mean)), and
            float(mean) is off by up to u24 |mean|, which moves the sum by u24 |mean| |sum dz|.
            At |mean|/std = 26 that alone is 16 * 0.75 M u24 against sum|dz (x - mean)| ~ 0.4 M:
            a bar of K u24 sum|dz (x - mean)| is not a bound on a correct kernel with K = 16.
  statistics, dyadic channels of exact-sum shapes: 8 fp32 ulps (2^-21 relative) on save_mean,
            save_invstd, running_mean, running_var (fp64 arithmetic on exact sums, one rounding),
            plus the fp64 roundings of S2 / M - mean^2, 8 * 2^-53 (var + mean^2), on the two that
            depend on var: all that is left where var = 0.
  statistics elsewhere: |var - ref| <= K u24 (var + mean^2)  (relative K u24 (1 + mean^2 / var)),
            invstd relative half of that (times var / (var + eps)), |mean - ref| <= K u24 mean|x|,
            each plus u24 of the value; the running statistics inherit momentum times these.

The ReLU mask of the backward reference is the device's own forward output (y > 0): that is what
dz is defined by.  The forward check requires it to equal z_ref > 0 wherever |z_ref| exceeds the
forward's fp32 slack; at most 0.1 % of a tensor may lie inside that band.
"""
import math
import types

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
U8, U21, U24 = 2.0 ** -8, 2.0 ** -21, 2.0 ** -24
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the ABI's `float eps`, as the kernels read it
DYADIC = (1, 2, 3, 7)
EXACT_M = 693
EXACT_SHAPES = [(3, 8, 5, 5), (2, 128, 7, 7), (7, 64, 9, 11), (1, 2048, 2, 2)]
INEXACT_SHAPES = [(8, 256, 14, 14)]
POOL_SHAPES = [(3, 8, 9, 7), (2, 64, 16, 16)]
MASK_BAND_CAP = 1e-3
FLOOR = 0.01  # a mutant must violate its bound on this fraction of the checked elements / channels


def seed(shape, group=0):
    """The seed of a shape's case (and of its further view groups): chosen so that the ReLU rounding
    band stays under the cap at every shape of the suite (test_cpu_bnregimes.py checks it)."""
    return 4000 + 17 * group + sum(shape)


def rne(t):
    """-> the nearest bf16 value (ties to even), as float64."""
    return t.float().to(BF16).double()


def nchw(t2d, shape):
    """[M, C] rows -> the [N, C, H, W] channels_last view of the same memory."""
    N, C, H, W = shape
    return t2d.view(N, H, W, C).permute(0, 3, 1, 2)


def rows(t):
    """[N, C, H, W] (any layout, any device) -> float64 [M, C] on the CPU."""
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().cpu()


def two_kernel_rows(M, C):
    """(rows per block, rows per pass) of the two-launch path: make_plan in csrc/batchnorm.hip."""
    SW = min(C, 64)
    rpp = 256 // (SW // 8)
    want = 512 // (C // SW)
    if M * C >= (16 << 20):
        want *= 2
    want = max(1, min(want, 512))
    rpb = -(-M // want)
    rpb = -(-rpb // rpp) * rpp
    return rpb, rpp


def chain(rpb, C):
    """Longest fp32 addition chain of a partial sum: rows per thread + rows per pass."""
    rpp = 256 // (min(C, 64) // 8)
    return -(-rpb // rpp) + rpp


def build(shape, seed, res=False):
    """The inputs of one case, on the CPU in float64 as [M, C] rows (fields x, dy, res) and
    float32 [C] parameters (gamma, beta, rm, rv); bf16-representable where the kernels read
    bf16.  `exact`: every fp32 partial sum of x and x^2 of a dyadic channel is exact."""
    N, C, H, W = shape
    assert C >= 8 and C & (C - 1) == 0
    M = N * H * W
    g = torch.Generator().manual_seed(seed)
    reg = torch.arange(C) % 8
    x = rne(torch.randn(M, C, generator=g, dtype=torch.float64) * 1.7 + 0.3)
    k8 = torch.randint(-8, 9, (M, C), generator=g).double()
    k2 = torch.randint(-2, 3, (M, C), generator=g).double()
    x = torch.where(reg == 1, 16 + k8 / 8, x)
    x = torch.where(reg == 2, 1 + k2 / 128, x)
    x = torch.where(reg == 3, torch.full_like(x, 16.0), x)
    x = torch.where(reg == 7, -16 + k8 / 8, x)
    assert torch.equal(x, rne(x))
    u = (torch.rand(C, generator=g) + 0.5).double()
    gamma = u.clone()
    gamma[reg == 4] = -u[reg == 4]
    gamma[reg == 5] = 0.0
    gamma[reg == 6] = 2.0 ** -10
    gamma[reg == 7] = 32.0
    sign = torch.where((torch.arange(C) // 8) % 2 == 0, 1.0, -1.0).double()
    beta = sign * (torch.rand(C, generator=g) * 0.4 + 0.1).double()
    rm = torch.randn(C, generator=g) * 0.1
    rv = torch.rand(C, generator=g) + 0.5
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    xhat = (x - mean) / torch.sqrt(var + EPS)
    dy = rne(0.75 + 0.5 * xhat.clamp(-4, 4) + 0.5 * torch.randn(M, C, generator=g, dtype=torch.float64))
    r = rne(torch.randn(M, C, generator=g, dtype=torch.float64)) if res else None
    exact = M <= EXACT_M
    if exact:  # unit^-1 = 8 (regimes 1, 3, 7) or 128 (regime 2)
        for rr, inv_unit in ((1, 8), (2, 128), (3, 8), (7, 8)):
            q = x[:, reg == rr] * inv_unit
            assert torch.equal(q, q.round()) and M * float(q.abs().max()) ** 2 < 2 ** 24
    dyadic = torch.zeros(C, dtype=torch.bool)
    for rr in DYADIC:
        dyadic |= reg == rr
    return types.SimpleNamespace(shape=shape, M=M, C=C, reg=reg, dyadic=dyadic, exact=exact, x=x, dy=dy, res=r,
                                 gamma=gamma.float(), beta=beta.float(), rm=rm, rv=rv)


def device_inputs(c, dev, dtype):
    """x, dy, res as [N, C, H, W] channels_last tensors of `dtype` and the fp32 parameters on dev."""
    t = lambda a: None if a is None else nchw(a, c.shape).to(dev, dtype)  # noqa: E731
    return t(c.x), t(c.dy), t(c.res), c.gamma.to(dev), c.beta.to(dev), c.rm.to(dev), c.rv.to(dev)


# ---- the fp64 reference ---------------------------------------------------------------------

def forward_ref(c, relu, res, eps=EPS, mean=None, var=None):
    """Closed-form forward in float64.  mean / var: the statistics to normalise with (eval mode);
    None = the batch's.  Returns z (before the ReLU), y, the statistics, the coefficients, the
    running statistics after one update at momentum 0.1 and 1, and the forward's fp32 slack."""
    x, g, b = c.x, c.gamma.double(), c.beta.double()
    M = c.M
    bmean = x.mean(0)
    bvar = ((x - bmean) ** 2).mean(0)
    mean = bmean if mean is None else mean.double()
    var = bvar if var is None else var.double()
    invstd = 1.0 / torch.sqrt(var + eps)
    sc = g * invstd
    sh = b - mean * sc
    z = (x - mean) * sc + b
    r = c.res if res else None
    if r is not None:
        z = z + r
    y = z.clamp_min(0) if relu else z
    slack = 4 * U24 * ((x * sc).abs() + sh.abs()) + (U24 * r.abs() if r is not None else 0.0)
    unb = bvar * M / (M - 1) if M > 1 else bvar
    run = {}
    for m in (0.1, 1.0):
        mf = float(torch.tensor(m, dtype=torch.float32))  # the ABI's `float momentum`
        run[m] = ((1 - mf) * c.rm.double() + mf * bmean, (1 - mf) * c.rv.double() + mf * unb)
    return types.SimpleNamespace(z=z, y=y, mean=mean, var=var, invstd=invstd, sc=sc, sh=sh, slack=slack, run=run,
                                 relu=relu, unb=unb)


def backward_ref(c, f, mask=None, dz=None, dz_stats=None, drop=()):
    """Closed-form backward in float64 from the forward reference f.  mask: the ReLU mask
    (None: z_ref > 0 when f.relu); dz: the gradient at the BatchNorm output, replacing
    dy * mask; dz_stats: the gradient the channel sums are taken of where it differs from the
    one applied (the pool-gathering stem backward).  drop: terms left out, for the mutants
    ("mean", "proj").  Returns dx, dres, dgamma, dbeta, the magnitude sum A and the sums of
    absolute values behind dgamma and dbeta."""
    x, g, M = c.x, c.gamma.double(), c.M
    if dz is None:
        if mask is None:
            mask = f.z > 0 if f.relu else torch.ones_like(x, dtype=torch.bool)
        dz = c.dy * mask
    ds = dz if dz_stats is None else dz_stats
    xc = x - f.mean
    S1, S2 = ds.sum(0), (ds * xc).sum(0)
    gi = g * f.invstd
    gi3 = gi * f.invstd * f.invstd
    t_mean = torch.zeros_like(S1) if "mean" in drop else S1 / M
    t_proj = torch.zeros_like(S2) if "proj" in drop else S2 / M
    dx = gi * (dz - t_mean) - gi3 * xc * t_proj
    A = gi.abs() * (dz.abs() + ds.abs().mean(0)) + gi3.abs() * (ds * xc).abs().mean(0) * (x.abs() + f.mean.abs())
    return types.SimpleNamespace(dx=dx, dres=dz, dgamma=S2 * f.invstd, dbeta=S1, A=A,
                                 dgamma_abs=f.invstd * (ds.abs() * (x.abs() + f.mean.abs())).sum(0),
                                 dgamma_centred_abs=f.invstd * (ds * xc).abs().sum(0), dbeta_abs=ds.abs().sum(0))


# ---- bounds and checks: each returns the worst ratio of error to bound and asserts it <= 1 ------

def worst_ratio(err, bound, what):
    zero = bound == 0
    assert bool((err[zero] == 0).all()), f"{what}: nonzero where the reference leaves no room"
    r = torch.where(zero, torch.zeros_like(err), err / torch.where(zero, torch.ones_like(bound), bound))
    worst = float(r.max()) if r.numel() else 0.0
    assert worst <= 1.0, (f"{what}: error / bound = {worst:.3f} at flat index {int(r.argmax())}; "
                          f"{float((r > 1).double().mean()):.4f} of the elements exceed the bound")
    return worst


def y_bound(f, bf16):
    return (U8 * f.y.abs() if bf16 else 0.0) + f.slack


def dx_bound(b, K, bf16):
    return (U8 * b.dx.abs() if bf16 else 0.0) + K * U24 * b.A


def mask_band(f):
    """Elements whose ReLU decision the forward's fp32 rounding may flip."""
    return f.z.abs() <= f.slack


def assert_band_small(f, what=""):
    frac = float(mask_band(f).double().mean())
    assert frac <= MASK_BAND_CAP, f"{what}: {frac:.5f} of the tensor lies inside the ReLU rounding band"
    return frac


def check_forward(f, y, bf16, what):
    """y: float64 [M, C] device output.  Returns (worst ratio, the device's ReLU mask or None)."""
    worst = worst_ratio((y - f.y).abs(), y_bound(f, bf16), f"{what} y")
    if not f.relu:
        return worst, None
    mask = y > 0
    band = mask_band(f)
    assert float(band.double().mean()) <= MASK_BAND_CAP, f"{what}: ReLU rounding band too wide"
    assert bool((mask == (f.z > 0))[~band].all()), f"{what}: ReLU mask differs from z_ref > 0 outside the band"
    return worst, mask


def check_backward(c, b, K, bf16, what, dx=None, dres=None, dgamma=None, dbeta=None):
    """Device outputs as float64 CPU tensors ([M, C] rows / [C]); returns the worst ratios."""
    out = {}
    if dx is not None:
        out["dx"] = worst_ratio((dx - b.dx).abs(), dx_bound(b, K, bf16), f"{what} dx")
    if dres is not None:
        assert torch.equal(dres, b.dres), f"{what} dres is not dz"
        out["dres"] = 0.0
    if dgamma is not None:
        # measured, not asserted: against K u24 is sum|dz (x - mean)|, the bar that leaves out
        # the fp32 rounding of save_mean (see the module docstring)
        narrow = K * U24 * b.dgamma_centred_abs + U24 * b.dgamma.abs()
        out["dgamma (centred bar)"] = float(((dgamma - b.dgamma).abs() / narrow.clamp_min(1e-300)).max())
        out["dgamma"] = worst_ratio((dgamma - b.dgamma).abs(), K * U24 * b.dgamma_abs + U24 * b.dgamma.abs(),
                               f"{what} dgamma")
    if dbeta is not None:
        out["dbeta"] = worst_ratio((dbeta - b.dbeta).abs(), K * U24 * b.dbeta_abs + U24 * b.dbeta.abs(), f"{what} dbeta")
    return out


def stat_bounds(c, f, K, momentum):
    """Absolute bounds per channel on save_mean, save_invstd, running_mean, running_var."""
    rmean, rvar = f.run[momentum]
    ex = c.dyadic & c.exact
    mean_b = K * U24 * c.x.abs().mean(0) + U24 * f.mean.abs()
    var_b = K * U24 * (f.var + f.mean ** 2)
    is_b = f.invstd * (0.5 * var_b / (f.var + EPS) + U24)
    unbf = c.M / (c.M - 1) if c.M > 1 else 1.0
    rm_b = momentum * mean_b + U24 * rmean.abs()
    rv_b = momentum * unbf * var_b + U24 * rvar.abs()
    # the kernels form var = S2 (1/M) - mean^2 in fp64: about eight roundings of 2^-53 relative
    # to var + mean^2 ahead of the cancellation (2.8e-14 at mean 16: a constant channel's var
    # comes out as +-1e-14, not 0, and moves invstd by 1e-9 relative)
    d64 = 8 * 2.0 ** -53 * (f.var + f.mean ** 2)
    pick = lambda ref, loose, extra=0.0: torch.where(ex, U21 * ref.abs() + extra, loose)  # noqa: E731
    return dict(save_mean=pick(f.mean, mean_b), save_invstd=pick(f.invstd, is_b, f.invstd * 0.5 * d64 / (f.var + EPS)),
                running_mean=pick(rmean, rm_b), running_var=pick(rvar, rv_b, momentum * unbf * d64))


def check_stats(c, f, K, momentum, what, save_mean=None, save_invstd=None, running_mean=None, running_var=None):
    ref = dict(save_mean=f.mean, save_invstd=f.invstd, running_mean=f.run[momentum][0],
               running_var=f.run[momentum][1])
    got = dict(save_mean=save_mean, save_invstd=save_invstd, running_mean=running_mean, running_var=running_var)
    bounds = stat_bounds(c, f, K, momentum)
    out = {}
    for k, v in got.items():
        if v is not None:
            out[k] = worst_ratio((v.double().cpu() - ref[k]).abs(), bounds[k], f"{what} {k}")
    return out


# ---- the pooled stem: MaxPool2d(k, s, pad) behind the BatchNorm + ReLU --------------------------

def pool_out(H, W, k, s, pad):
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def pool_forward_ref(c, f, k, s, pad):
    """Window maxima of relu(z_ref) and of the forward bound, [N, C, P, Q] float64."""
    yr = nchw(f.y, c.shape).contiguous()
    br = nchw(y_bound(f, True), c.shape).contiguous()
    return F.max_pool2d(yr, k, s, pad), F.max_pool2d(br, k, s, pad)


def pool_pixels(c, idx, k, s, pad):
    """Flat row index (into [M]) of the pixel each pooled output selected.  idx: [N, P, Q, C]
    window positions r * k + col as the pool kernels store them."""
    N, C, H, W = c.shape
    P, Q = pool_out(H, W, k, s, pad)
    idx = idx.long().cpu()
    n = torch.arange(N).view(N, 1, 1, 1)
    h = torch.arange(P).view(1, P, 1, 1) * s - pad + idx // k
    w = torch.arange(Q).view(1, 1, Q, 1) * s - pad + idx % k
    assert bool(((h >= 0) & (h < H) & (w >= 0) & (w < W)).all()), "pool index outside the image"
    return (n * H + h) * W + w


def check_pool_forward(c, f, yp, idx, k, s, pad, what):
    """yp [N, C, P, Q] device output, idx the device's argmax: the pooled values within the window
    maximum of the element bounds, and the selected pixel's reference value within twice that of
    the reference maximum (a tie or a near-tie may go either way)."""
    ref, bnd = pool_forward_ref(c, f, k, s, pad)
    got = yp.detach().double().cpu()
    worst = worst_ratio((got - ref).abs().reshape(-1), bnd.reshape(-1), f"{what} pooled y")
    pix = pool_pixels(c, idx, k, s, pad)                      # [N, P, Q, C]
    sel = torch.gather(f.y, 0, pix.reshape(-1, c.C)).view(pix.shape)
    gap = ref.permute(0, 2, 3, 1) - sel
    assert bool((gap <= 2 * bnd.permute(0, 2, 3, 1)).all()), f"{what}: the pool selected a pixel that is not a maximum"
    return worst


def pool_gather(c, dyp, yp, idx, k, s, pad):
    """The pooled gradient carried back to the pixels its windows selected, where the pooled
    output passed the ReLU: float64 [M, C], unrounded sums."""
    pix = pool_pixels(c, idx, k, s, pad).reshape(-1, c.C)
    d = (dyp.detach().double().cpu() * (yp.detach().double().cpu() > 0)).permute(0, 2, 3, 1).reshape(-1, c.C)
    return torch.zeros(c.M, c.C, dtype=torch.float64).scatter_add_(0, pix, d)


# ---- fp32 emulation of the kernels' formulas (CPU) -------------------------------------------

def _fma32(a, b, cc):
    """fp32 fma of fp32-valued float64 tensors (the float64 product of a bf16 and an fp32 value
    is exact; the one float64 rounding of the sum matters only at exact ties)."""
    return (a * b + cc).float().double()


def emulate_forward(c, f, relu, res):
    sc, sh = f.sc.float().double(), f.sh.float().double()
    z = _fma32(c.x, sc, sh)
    if res:
        z = (z + c.res).float().double()
    return rne(z.clamp_min(0) if relu else z)


def emulate_backward(c, f, b, dz):
    """dx = fma(ca, dz, fma(cb, x, cc)) with coefficients rounded once from float64."""
    g, M = c.gamma.double(), c.M
    ca = g * f.invstd
    cb = -g * f.invstd ** 3 * (b.dgamma / f.invstd) / M
    cc = -ca * b.dbeta / M - cb * f.mean.float().double()
    ca, cb, cc = (t.float().double() for t in (ca, cb, cc))
    return rne(_fma32(ca, dz, _fma32(cb, c.x, cc)))


# ---- mutants: each must violate its bound, or the bound checks nothing ---------------------------

def mutant_rates(c, K=16):
    """Violation rates of the wrong references against the bounds above, for the ReLU form without
    residual: name -> fraction of the checked elements or channels.  The statistics mutants are
    measured where the issue places them (regime 2; regimes 1 and 7; exact-sum shapes)."""
    f = forward_ref(c, True, False)
    b = backward_ref(c, f)
    bound = dx_bound(b, K, True)
    rate = lambda err, bnd: float((err > bnd).double().mean())  # noqa: E731
    out = {}
    out["dx_no_mean"] = rate((backward_ref(c, f, drop=("mean",)).dx - b.dx).abs(), bound)
    out["dx_no_proj"] = rate((backward_ref(c, f, drop=("proj",)).dx - b.dx).abs(), bound)
    sb = stat_bounds(c, f, K, 1.0)
    r2 = c.reg == 2
    out["invstd_no_eps"] = rate((1.0 / torch.sqrt(f.var[r2]) - f.invstd[r2]).abs(), sb["save_invstd"][r2])
    # the ReLU mask of a kernel that assumes sc > 0 (x > -sh / sc, i.e. |sc| x_hat + beta > 0)
    r4 = c.reg == 4
    zpos = (c.x - f.mean) * f.sc.abs() + c.beta.double()
    bm = backward_ref(c, f, mask=zpos > 0)
    out["mask_positive_gamma"] = rate((bm.dx - b.dx).abs()[:, r4], bound[:, r4])
    if c.exact:
        d = c.dyadic
        out["running_var_biased"] = rate((f.var[d] - f.run[1.0][1][d]).abs(), sb["running_var"][d])
        r17 = (c.reg == 1) | (c.reg == 7)
        x32 = c.x.float()
        m32 = x32.sum(0) / c.M
        v32 = ((x32 * x32).sum(0) / c.M - m32 * m32).double()
        out["var_fp32"] = rate((v32[r17] - f.var[r17]).abs(), U21 * f.var[r17])
    return out


def assert_discriminates(c, K=16, floor=FLOOR, what=""):
    rates = mutant_rates(c, K)
    for k, v in rates.items():
        assert v >= floor, f"{what}: the {k} mutant violates its bound on only {v:.4f} of the checked elements"
    return rates


def fmt(d):
    return ", ".join(f"{k} {v:.3f}" for k, v in d.items())


assert math.isclose(EPS, 1e-5, rel_tol=1e-6)
