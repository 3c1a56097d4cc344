"""References, input recipes and bounds for the kernels at the two ends of the network: the
max-pool (csrc/maxpool.hip), the branch-summed cross-entropy and the evaluation metrics
(csrc/xent.hip).  Used by tests/test_cpu_endsref.py (the conditions on the inputs and the bounds,
no GPU) and by tests/test_gpu_pool_edges.py, test_gpu_xent_edges.py and test_gpu_eval_metrics.py.
Everything here runs on the CPU.

Pool.  pool_scan is the rule the kernels document, written out: scan the in-bounds positions of a
window row-major and take a value when `v > m or isnan(v)`, starting from -inf with the argmax at
the first in-bounds position.  So the first of equal maxima wins, the LAST NaN of the scan wins,
and a window of nothing but -inf selects its first in-bounds position.  route() carries dy back
along the argmax in float64.  The inputs make every comparison exact: x is small integers (ties in
most windows) with NaN and -inf sprinkled at a density chosen per window size, dy is odd integers
|dy| <= 255 (exact in bf16), so every routed sum is an integer below 2^24, fp32 accumulation is
exact in any order, and the expected bf16 gradient is exactint.rne(exact sum): one rounding.
The rules pool_scan can be switched to ("ge", "skipnan", "stickynan") and the truncating store are
the mutants: mutant_rates measures how much of the expected result each would change.

Loss.  fp64 log-softmax and, with u = 2^-24, per row (lse the fp64 value):

    b_lse  = u (N + 4 + 2 |lse| + max|x|)                       |lse_kernel - lse| <= b_lse
    row    = b_lse + u (|lse| + |lse - x_y|)                    the row's loss term
    delta  = b_lse + 2 u (|x| + |lse|),  p = softmax in fp64
    grad   = (|g| / B) (p (expm1(delta) + 4 u) + 2^-125 + u |p - onehot|) + u |ref|

N u: the fp32 addition chain of the N exponentials and their own 2-ulp error; 4 u: a 2-ulp expf,
the subtraction and the scale; 2^-125: flushed subnormals.  max|x| is taken over the finite logits
and a logit of -inf has p = 0 with nothing to round (exp(-inf) = 0 exactly), so its p-term is 0.
emulate_xent is an fp32 restatement of the kernels' formulas; its switches are the loss mutants.

Metrics.  near_tie_logits builds inputs on which the two ways to form the branch mean of the
evaluation top-1, sum / nbranch and sum * (1 / nbranch), rank two classes differently.
"""
import math
import types

import numpy as np
import torch

import exactint as X
from bnregimes import FLOOR   # a mutant must change / violate this fraction of the checked elements

U = 2.0 ** -24
TINY = 2.0 ** -125

# ---- pool -------------------------------------------------------------------------------------

POOL_CASES = [
    ((3, 8, 9, 7), (3, 2, 1)),
    ((2, 16, 10, 10), (2, 2, 0)),
    ((1, 32, 13, 13), (3, 1, 1)),
    ((2, 8, 17, 19), (5, 2, 2)),
    ((2, 8, 17, 19), (5, 3, 1)),
    ((2, 8, 17, 19), (2, 3, 0)),       # stride > k: pixels no window covers
    ((2, 8, 17, 19), (4, 2, 2)),       # even k with pad = k / 2
    ((1, 8, 33, 31), (15, 4, 7)),
    ((2, 8, 12, 11), (3, 3, 1)),
    ((2, 8, 3, 3), (3, 1, 0)),         # P = Q = 1
    ((2, 8, 5, 1), (3, 2, 1)),         # W = Q = 1
    ((2, 8, 4, 4), (1, 1, 0)),
    ((2, 8, 4, 4), (1, 2, 0)),
]
TRUNC_WINDOWS = [(3, 2, 1), (3, 1, 1)]   # the overlapping windows the truncating-store mutant is run on
NAN_TARGET = 0.45                        # wanted fraction of NaN outputs; asserted to land in 10-60 %

# (shape, window, mutant) that cannot show there, with the reason.  Everything else must reach FLOOR.
NOT_CHECKED = {
    ((2, 8, 4, 4), (1, 1, 0), "ge"): "one value per window: no ties",
    ((2, 8, 4, 4), (1, 2, 0), "ge"): "one value per window: no ties",
    ((2, 8, 4, 4), (1, 1, 0), "stickynan"): "one value per window: the first NaN is the last",
    ((2, 8, 4, 4), (1, 2, 0), "stickynan"): "one value per window: the first NaN is the last",
    ((2, 8, 4, 4), (1, 1, 0), "skipnan_dx"): "one value per window: the argmax cannot move (y is checked)",
    ((2, 8, 4, 4), (1, 2, 0), "skipnan_dx"): "one value per window: the argmax cannot move (y is checked)",
    ((1, 8, 33, 31), (15, 4, 7), "stickynan"): "576 windows over 8184 inputs and neighbouring windows share their "
                                               "NaNs: 0.1-0.3 % of dx moves at any density that keeps the NaN "
                                               "outputs within 10-60 % (the mutant still fails torch.equal)",
    ((2, 8, 5, 1), (3, 2, 1), "truncated"): "W = 1: at most two terms per input, and a sum of two odd |dy| <= 255 "
                                            "is an even integer <= 510, exact in bf16",
}


def pool_out(H, W, k, s, pad):
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def pool_scan(x, k, s, pad, rule="torch"):
    """x: float64 numpy [N, C, H, W].  Returns y [N, C, P, Q] and the flat index h * W + w each
    window selected.  rule: "torch" (the kernels' rule) or a mutant - "ge" (the last maximum
    wins), "skipnan" (a NaN is never taken, as fmaxf), "stickynan" (the first NaN stays)."""
    N, C, H, W = x.shape
    P, Q = pool_out(H, W, k, s, pad)
    h0 = np.arange(P) * s - pad
    w0 = np.arange(Q) * s - pad
    hs, ws = np.maximum(h0, 0), np.maximum(w0, 0)
    m = np.full((N, C, P, Q), -np.inf)
    arg = np.broadcast_to((hs[:, None] * W + ws[None, :])[None, None], (N, C, P, Q)).copy()
    for r in range(k):
        for c in range(k):
            h, w = h0 + r, w0 + c
            inb = ((h >= 0) & (h < H))[:, None] & ((w >= 0) & (w < W))[None, :]      # [P, Q]
            hc, wc = np.clip(h, 0, H - 1), np.clip(w, 0, W - 1)
            v = x[:, :, hc][:, :, :, wc]                                              # [N, C, P, Q]
            with np.errstate(invalid="ignore"):
                if rule == "torch":
                    take = (v > m) | np.isnan(v)
                elif rule == "ge":
                    take = (v >= m) | np.isnan(v)
                elif rule == "skipnan":
                    take = v > m
                elif rule == "stickynan":
                    take = ((v > m) | np.isnan(v)) & ~np.isnan(m)
                else:
                    raise ValueError(rule)
            take &= inb[None, None]
            m = np.where(take, v, m)
            arg = np.where(take, (hc[:, None] * W + wc[None, :])[None, None], arg)
    return m, arg


def route(arg, dy, H, W):
    """dx[n, c, arg] += dy in float64: numpy [N, C, H, W]."""
    N, C, P, Q = dy.shape
    dx = np.zeros((N * C, H * W))
    rows = np.repeat(np.arange(N * C), P * Q)
    np.add.at(dx, (rows, arg.reshape(-1)), dy.astype(np.float64).reshape(-1))
    return dx.reshape(N, C, H, W)


def terms(arg, H, W):
    """How many windows selected each input: int [N, C, H, W]."""
    return route(arg, np.ones(arg.shape), H, W).astype(np.int64)


def pool_seed(shape, win):
    return 7000 + sum(shape) + 100 * win[0] + 10 * win[1] + win[2]


def plant_positions(H, W, k, s, pad):
    """Pixels spaced so that every window holds at most one of them and each is covered by
    ceil(k/s)^2 whole windows: with a value above everything else there, each is the maximum of
    all the windows that cover it.  (3, 2, 1): h, w = 1 mod 4, a subset of the odd/odd pixels;
    (3, 1, 1): h, w = 1 mod 3."""
    n = -(-k // s)
    step = n * s
    P, Q = pool_out(H, W, k, s, pad)
    cover = lambda i, L: [p for p in range(L) if p * s - pad <= i <= p * s - pad + k - 1]  # noqa: E731
    hs = [h for h in range(1, H, step) if len(cover(h, P)) == n]
    ws = [w for w in range(1, W, step) if len(cover(w, Q)) == n]
    return hs, ws, n * n


def pool_inputs(shape, win, seed=None):
    """The inputs of one case: x, dy as float32 torch tensors [N, C, H, W] / [N, C, P, Q] holding
    bf16-exact values, the planted mask (or None) and the number of terms a planted input gets."""
    N, C, H, W = shape
    k, s, pad = win
    P, Q = pool_out(H, W, k, s, pad)
    g = torch.Generator().manual_seed(pool_seed(shape, win) if seed is None else seed)
    x = X.ints(shape, 2, g)
    # density from the mean number of in-bounds positions of a window: a fixed 6 % would make every
    # output NaN at k = 15 (this gives 0.36 % there) and hardly any at W = 1
    inb = lambda L, n: sum(sum(0 <= p * s - pad + r < L for r in range(k)) for p in range(n)) / n  # noqa: E731
    d_nan = 1.0 - (1.0 - NAN_TARGET) ** (1.0 / (inb(H, P) * inb(W, Q)))
    r = torch.rand(shape, generator=g)
    x[r < d_nan] = float("nan")
    x[(r >= d_nan) & (r < d_nan * 5 / 3)] = float("-inf")     # two -inf for three NaN
    # blocks of nothing but -inf, each large enough to hold a whole window: the corner window's
    # in-bounds part, and an interior block that contains a window wherever the stride puts one
    cb = k - pad
    ib = k + s - 1
    x[0, C - 1, :cb, :cb] = float("-inf")
    h1, w1 = min(H // 3, max(H - ib, 0)), min(W // 3, max(W - ib, 0))
    x[0, C - 1, h1:h1 + ib, w1:w1 + ib] = float("-inf")
    planted, nterm = None, 0
    if win in TRUNC_WINDOWS and min(H, W) > 1:
        # half the channels: no NaN / -inf, and a high constant where the most windows overlap
        hs, ws, nterm = plant_positions(H, W, k, s, pad)
        half = C // 2
        clean = X.ints((N, half, H, W), 2, g)
        x[:, :half] = torch.where(torch.isfinite(x[:, :half]), x[:, :half], clean)
        planted = torch.zeros(shape, dtype=torch.bool)
        for h in hs:
            for w in ws:
                planted[:, :half, h, w] = True
        x[planted] = 7.0
    mag = torch.randint(0, 128, (N, C, P, Q), generator=g).float() * 2 + 1          # odd, 1 .. 255
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).view(1, C, 1, 1)
    flip = torch.where(torch.rand(N, C, P, Q, generator=g) < 0.15, -1.0, 1.0)
    dy = mag * sign * flip
    assert torch.equal(dy, X.rne(dy)) and float(dy.abs().max()) <= 255 and bool((dy % 2 != 0).all())
    fin = torch.isfinite(x)
    assert torch.equal(x[fin], X.rne(x[fin]))
    X.assert_exact_bound((-(-k // s)) ** 2, 255)
    return types.SimpleNamespace(shape=shape, win=win, x=x, dy=dy, planted=planted, nterm=nterm, P=P, Q=Q)


def pool_expected(c, rule="torch"):
    """y (float64 torch), the exact dx (float64 torch), the argmax and the term counts."""
    N, C, H, W = c.shape
    k, s, pad = c.win
    y, arg = pool_scan(c.x.double().numpy(), k, s, pad, rule)
    dx = route(arg, c.dy.numpy(), H, W)
    assert float(np.abs(dx).max()) < X.LIMIT
    return types.SimpleNamespace(y=torch.from_numpy(y), dx=torch.from_numpy(dx), arg=arg,
                                 terms=torch.from_numpy(terms(arg, H, W)))


def same(a, b):
    """Equal with NaN exactly where the other has NaN."""
    a, b = a.double(), b.double()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def frac_differs(a, b):
    a, b = a.double(), b.double()
    return float((~((a == b) | (torch.isnan(a) & torch.isnan(b)))).double().mean())


def pool_mutant_rates(c, e=None):
    """name -> fraction of the checked elements a mutant changes.  ge / stickynan / skipnan_dx: of
    the elements of dx; skipnan_y: of the NaN outputs; truncated (TRUNC_WINDOWS only): of the
    inputs that receive at least two contributions, bf16 store."""
    e = e or pool_expected(c)
    out = {}
    for rule in ("ge", "stickynan", "skipnan"):
        m = pool_expected(c, rule)
        out[rule if rule != "skipnan" else "skipnan_dx"] = frac_differs(m.dx, e.dx)
        if rule == "skipnan":
            nan = torch.isnan(e.y)
            out["skipnan_y"] = float((~torch.isnan(m.y[nan])).double().mean()) if bool(nan.any()) else 0.0
    if c.win in TRUNC_WINDOWS:
        multi = e.terms >= 2
        out["truncated"] = X.frac_ne(X.trunc(e.dx)[multi], X.rne(e.dx)[multi]) if bool(multi.any()) else 0.0
    return out


def assert_pool_discriminates(c, e=None, floor=FLOOR):
    rates = pool_mutant_rates(c, e)
    for name, r in rates.items():
        if (c.shape, c.win, name) in NOT_CHECKED:
            continue
        assert r >= floor, f"{c.shape} {c.win}: the {name} mutant changes only {r:.4f} of the checked elements"
    return rates


# ---- loss ---------------------------------------------------------------------------------------

XENT_CASES = [(3, 100, 40), (8, 70, 130), (1, 513, 7), (2, 257, 1000), (12, 32, 40)]   # (nbranch, B, N)
XENT_SETS = ["n3", "n3_shift", "n60", "n200_shift", "neginf"]
XENT_G = 3.0                                                                           # the incoming gradient


def xent_inputs(case, kind):
    """logits float32 [nbranch, B, N] and labels int64 [B] on the CPU."""
    nb, B, N = case
    g = torch.Generator().manual_seed(9000 + 7 * nb + 3 * B + N + 1000 * XENT_SETS.index(kind))
    z = torch.randn(nb, B, N, generator=g, dtype=torch.float64)
    y = torch.randint(0, N, (B,), generator=g)
    if kind == "n3":
        x = 3 * z
    elif kind == "n3_shift":
        x = 3 * z + 1e4
    elif kind == "n60":
        x = 60 * z
    elif kind == "n200_shift":
        x = 200 * z - 3e4
    elif kind == "neginf":
        x = 3 * z
        drop = torch.rand(nb, B, N, generator=g) < 0.3
        drop[:, torch.arange(B), y] = False              # the label's logit stays finite
        x[drop] = float("-inf")
    else:
        raise ValueError(kind)
    return x.float(), y


def xent_ref(x, y, g=XENT_G):
    """fp64 reference and the bounds of the module docstring.  x float32 [nb, B, N], y [B]."""
    nb, B, N = x.shape
    xd = x.double()
    lse = torch.logsumexp(xd, dim=2)                                      # [nb, B]
    fin = torch.isfinite(xd)
    amax = torch.where(fin, xd.abs(), torch.zeros_like(xd)).amax(dim=2)
    xy = xd[:, torch.arange(B), y]
    rows = lse - xy
    loss = rows.sum() / B
    p = torch.exp(xd - lse[..., None])
    onehot = torch.zeros_like(xd)
    onehot[:, torch.arange(B), y] = 1.0
    grad = (g / B) * (p - onehot)
    b_lse = U * (N + 4 + 2 * lse.abs() + amax)
    b_row = b_lse + U * (lse.abs() + rows.abs())
    ax = torch.where(fin, xd.abs(), torch.zeros_like(xd))
    delta = b_lse[..., None] + 2 * U * (ax + lse.abs()[..., None])
    pterm = torch.where(fin, p * (torch.expm1(delta) + 4 * U), torch.zeros_like(p))
    b_grad = (abs(g) / B) * (pterm + TINY + U * (p - onehot).abs()) + U * grad.abs()
    return types.SimpleNamespace(lse=lse, rows=rows, loss=loss, grad=grad, b_lse=b_lse, b_row=b_row,
                                 b_loss=b_row.sum() / B, b_grad=b_grad)


def emulate_xent(x, y, g=XENT_G, shift=True, add_back=True, div_rows=False):
    """The kernels' formulas in fp32 on the CPU (row_lse: max, a sequential fp32 sum of
    expf(x - m), m + logf(s); the row terms summed in fp64; dx = (g / B) (expf(x - lse) - onehot)).
    shift=False: no max shift; add_back=False: the max is not added back; div_rows=True: the
    gradient divided by nbranch * B.  Returns lse [nb, B], rows, loss (float32 values as float64)
    and dx."""
    nb, B, N = x.shape
    xn = x.numpy().astype(np.float32)
    with np.errstate(all="ignore"):
        m = xn.max(axis=2) if shift else np.zeros((nb, B), np.float32)
        s = np.zeros((nb, B), np.float32)
        for n in range(N):
            s = (s + np.exp((xn[:, :, n] - m).astype(np.float32)).astype(np.float32)).astype(np.float32)
        lse = (np.log(s).astype(np.float32) + (m if add_back else np.float32(0))).astype(np.float32)
        xy = xn[:, np.arange(B), y.numpy()]
        rows = (lse - xy).astype(np.float32)
        loss = np.float32(rows.astype(np.float64).sum() / B)
        gb = np.float32(np.float32(g) / np.float32(nb * B if div_rows else B))
        onehot = np.zeros_like(xn)
        onehot[:, np.arange(B), y.numpy()] = 1
        p = np.exp((xn - lse[..., None]).astype(np.float32)).astype(np.float32)
        dx = (gb * (p - onehot).astype(np.float32)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))  # noqa: E731
    return types.SimpleNamespace(lse=t(lse), rows=t(rows), loss=float(loss), grad=t(dx))


def used(err, bound):
    """The largest fraction of a bound that is used; inf where a value is not finite or the bound
    is exceeded without room."""
    err, bound = err.double(), bound.double()
    r = torch.where(torch.isfinite(err), err / bound, torch.full_like(err, float("inf")))
    return float(r.max())


def xent_fractions(ref, lse=None, rows=None, loss=None, grad=None):
    """name -> the largest fraction of its bound used (each must be <= 1)."""
    out = {}
    if lse is not None:
        out["lse"] = used((lse.double() - ref.lse).abs(), ref.b_lse)
    if rows is not None:
        out["row"] = used((rows.double() - ref.rows).abs(), ref.b_row)
    if loss is not None:
        out["loss"] = used(torch.tensor(abs(float(loss) - float(ref.loss))), ref.b_loss)
    if grad is not None:
        out["grad"] = used((grad.double() - ref.grad).abs(), ref.b_grad)
    return out


def violation_rate(err, bound):
    err = err.double()
    return float((~(err <= bound)).double().mean())     # a NaN or inf violates


def xent_mutant_rates(x, y, ref=None):
    """name -> fraction of the rows (lse, row loss) or gradient elements outside their bound."""
    ref = ref or xent_ref(x, y)
    out = {}
    e = emulate_xent(x, y, shift=False)
    out["no_shift"] = violation_rate((e.rows - ref.rows).abs(), ref.b_row)
    e = emulate_xent(x, y, add_back=False)
    out["no_add_back"] = violation_rate((e.lse - ref.lse).abs(), ref.b_lse)
    # checked: the elements whose gradient is not lost to underflow under either scale (at
    # N(0, 200^2) nearly every softmax is one-hot in fp32 and most of dx is an exact 0)
    e = emulate_xent(x, y, div_rows=True)
    live = ref.grad.abs() >= 2.0 ** -100
    out["div_rows"] = violation_rate((e.grad - ref.grad).abs()[live], ref.b_grad[live])
    return out


def xent_mutant_applies(case, kind, name):
    """Where a loss mutant can show: the max shift matters once exp(x) leaves the fp32 range
    (every set but N(0, 3^2) and its -inf variant); nbranch * B differs from B from two branches up."""
    if name == "no_shift":
        return kind in ("n3_shift", "n60", "n200_shift")
    if name == "div_rows":
        return case[0] > 1
    return True


# ---- metrics: near ties of the branch mean ------------------------------------------------------

NEAR_TIE_BRANCHES = (3, 5, 6, 7)


def mean_div(s, nb):
    return (s.float() / torch.tensor(float(nb), dtype=torch.float32)).float()


def mean_mul(s, nb):
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(nb), dtype=torch.float32)
    return (s.float() * inv).float()


def near_tie_logits(nb, B, N, collapse, seed=0):
    """logits float32 [nb, B, N], labels [B].  Sample b holds s_b at class 1 and nextafter(s_b) at
    class 2 of branch b % nb and zeros elsewhere, s_b in [1, 9) found by search so that the two
    class means stay distinct under one formula (the top-1 is class 2, the larger) and collapse to
    a tie under the other (the top-1 is class 1, the first).  collapse = "div": sum / nb collapses
    and sum * (1 / nb) does not; "mul": the other way round.  Two labels in three are 1, the
    third is 2, so the two formulas' hit counts differ by a third of the batch."""
    assert N > 2 and collapse in ("div", "mul")
    g = torch.Generator().manual_seed(11000 + 13 * nb + B + (0 if collapse == "div" else 500) + seed)
    found = torch.empty(0, dtype=torch.float32)
    for _ in range(200):
        s = (torch.rand(64 * B, generator=g, dtype=torch.float64) * 8 + 1).float()
        t = torch.nextafter(s, torch.tensor(float("inf")))
        cd = mean_div(s, nb) == mean_div(t, nb)
        cm = mean_mul(s, nb) == mean_mul(t, nb)
        ok = (cd & ~cm) if collapse == "div" else (cm & ~cd)
        found = torch.cat([found, s[ok]])
        if found.numel() >= B:
            break
    assert found.numel() >= B, f"no near ties found for nbranch {nb}, collapse {collapse}"
    s = found[:B]
    x = torch.zeros(nb, B, N)
    b = torch.arange(B)
    x[b % nb, b, 1] = s
    x[b % nb, b, 2] = torch.nextafter(s, torch.tensor(float("inf")))
    y = torch.where(b % 3 == 2, 2, 1)      # the two formulas then score B/3 and 2B/3 hits
    return x, y


def top1_by(x, nb, how):
    """The ensemble top-1 under one mean formula: the fp32 sum over the branches in order, then
    `how` (mean_div or mean_mul); the first maximum wins."""
    s = x[0].clone()
    for i in range(1, nb):
        s = (s + x[i]).float()
    return how(s, nb).argmax(1)


def fmt(d):
    return ", ".join(f"{k} {v:.3f}" for k, v in d.items())


assert math.isclose(U, 5.960464477539063e-08)
