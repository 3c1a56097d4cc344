"""Every BatchNorm path against the closed-form fp64 reference of tests/bnregimes.py, per element,
on inputs whose channels cover eight regimes (ordinary, |mean|/std ~ 26, var ~ 1e-4, constant,
negative / zero / tiny / large gamma) and whose gradient has a nonzero mean and is correlated
with x_hat, so that all three terms of dx are tens of percent of it at every size.

Paths: GMBatchNorm2d in bf16 under gm_bn_set_fused_mode 0 / 1 / 2 (two launches, register-held
single launch, streaming single launch: each row asserts the variant gm_bn_fused_form names),
GMBatchNorm2d in fp32 (fp64 sums, centred backward coefficients), the stem's fused
BatchNorm + ReLU + max-pool, the grouped launches of vtrunk.vbn and of the stem's pool-gathering
backward with two view groups of different statistics, and eval mode (gm_bn_fwd_infer_*,
gm_bn_infer_coef) on running statistics with a tiny and an exactly zero variance.  Forms: plain,
ReLU with the mask recomputed from x and read from y, residual + ReLU, and (GMBatchNorm2d only: the
form whose kernels nothing else launches) a residual without ReLU.  Checked: y, save_mean,
save_invstd, running statistics (momentum 1 in the plain form, 0.1 in the others),
num_batches_tracked, dx, dres, dgamma, dbeta - with the bounds derived in bnregimes.py and never
fitted.  K = 16 + the fp32 addition chain of the launch's plan (gm_bn_plan_rows) for every bf16
path, also on the exact-sum shapes: their sums of x and x^2 are exact on the dyadic channels
(which therefore get the 8-ulp bar), their sums of dz are not.

The streaming rows take the smallest M at C = 64 whose forward (backward) plans as streaming under
the concurrency and residency in effect: found by bisection on gm_bn_fused_form, and a row that
does not reach the variant it names fails.

Measured on an MI355X (worst ratio of error to bound over the rows of a path and variant; a bar
is 1; test_zz_report prints the table of the run at hand):
    GMBatchNorm2d bf16, two-kernel:        y 0.995, save_mean 0.125, save_invstd 0.111, running_mean
                                           0.125, running_var 0.602, dx 0.995, dgamma 0.036, dbeta 0.020
    GMBatchNorm2d bf16, register-held NR4: the same figures (dbeta 0.019)
    GMBatchNorm2d bf16, NR8 / NR16:        y 0.996, save_mean 0.011, save_invstd 0.027, running_mean
                                           0.037, running_var 0.134, dx 0.995, dgamma 0.020, dbeta 0.016
    GMBatchNorm2d bf16, streaming:         y 0.996, save_mean 0.003, save_invstd 0.030, running_mean
                                           0.034, running_var 0.134, dx 0.995, dgamma 0.025, dbeta 0.016
    GMBatchNorm2d fp32 (fp64 sums):        y 0.881, save_mean 0.125, save_invstd 0.111, running_mean
                                           0.136, running_var 0.767, dx 0.166, dgamma 0.096, dbeta 0.058
    relu_maxpool, FUSE_POOL:               y 0.962, save_mean 0.100, save_invstd 0.086, running_mean
                                           0.078, running_var 0.117, dx 0.978, dgamma 0.028, dbeta 0.012
    vtrunk.vbn G = 2 (two-kernel and NR4): y 0.995, save_mean 0.125, save_invstd 0.091, running_mean
                                           0.106, running_var 0.160, dx 0.995, dgamma 0.038, dbeta 0.020
    vstem BN + pool G = 2:                 y 0.980, save_mean 0.004, save_invstd 0.089, running_mean
                                           0.094, running_var 0.117, dx 0.992, dgamma 0.029, dbeta 0.011
    gm_bn_fwd_infer bf16 / fp32:           y 0.995 / 0.881;  gm_bn_infer_coef: sc, sh 0.120
    dres equals dz bit for bit everywhere.  y and dx sit at 0.99 because their bound is the bf16
    store's half ulp, which a correct kernel attains.
    Against the narrower dgamma bar K u24 is sum|dz (x - mean)| the same runs give up to 2.0 (bf16)
    and 6.0 (fp32 path, K = 16): the fp32 rounding of save_mean, see bnregimes.py.
    Smallest M at C = 64, default concurrency: forward NR8 32769, NR16 49153, streaming 65537;
    backward NR8 24577, streaming 32769.
Mutant violation rates on the CPU (test_cpu_bnregimes.py, fraction of checked elements / channels):
    dx without mean(dz) 0.75 - 0.875, dx without the projection term 0.65 - 0.75, invstd without eps
    1.0 (regime 2), biased running_var 0.75 (the constant channel has var 0 either way), fp32
    S2/M - mean^2 0.875 - 1.0 (regimes 1, 7), positive-gamma ReLU mask on regime 4 0.995 - 1.0.
"""
import pytest
import torch

import bnregimes as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
FORMS = [("plain", False, False, True), ("relu_maskx", True, False, True), ("relu_ymask", True, False, False),
         ("res_relu", True, True, True)]
ids = lambda s: "x".join(map(str, s))  # noqa: E731

WORST = {}     # (path, variant) -> {quantity: worst error / bound}
FOUND = {}     # what the planner answered: streaming M, forms per row
_cases, _frefs = {}, {}


def case(shape, group=0):
    if (shape, group) not in _cases:
        _cases[shape, group] = R.build(shape, R.seed(shape, group), res=True)
    return _cases[shape, group]


def fref(shape, group, relu, res):
    k = (shape, group, relu, res)
    if k not in _frefs:
        _frefs[k] = R.forward_ref(case(shape, group), relu, res)
    return _frefs[k]


def note(path, variant, d):
    w = WORST.setdefault((path, variant), {})
    for k, v in d.items():
        w[k] = max(w.get(k, 0.0), v)


def _lib():
    from greedy_multimodal_learning_amd import _lib as L
    return L, L.load()


@pytest.fixture
def fused_mode():
    """Switch the single-launch BatchNorm mode (gm_bn_set_fused_mode); restores 2."""
    L, lib = _lib()
    yield lambda m: L.check(lib.gm_bn_set_fused_mode(int(m)), "gm_bn_set_fused_mode")
    lib.gm_bn_set_fused_mode(2)


VARIANT = {0: "two-kernel", -1: "streaming"}


def plan(M, C, G=1):
    """(forward form, backward form, forward K, backward K) of a bf16 launch as planned now."""
    _, lib = _lib()
    ff, fb = lib.gm_bn_fused_form(M, C, 0, G), lib.gm_bn_fused_form(M, C, 1, G)
    kf = 16 + R.chain(lib.gm_bn_plan_rows(M, C, 0, G), C)
    kb = 16 + R.chain(lib.gm_bn_plan_rows(M, C, 1, G), C)
    return ff, fb, kf, kb


def variant(form):
    return VARIANT.get(form, f"register-held NR{form}")


ORDER = [4, 8, 16, -1]   # the forms in the order a growing map passes through them


def smallest_m(bwd, target, G=1):
    """Smallest M at C = 64 whose forward (backward) the planner gives the form `target` for a launch
    of G view groups (mode 2, concurrency and residency as they are): rows per thread grow with M, so
    the forms follow one another in ORDER and bisection finds where `target` begins."""
    key = f"{'bwd' if bwd else 'fwd'} {variant(target)}" + (f" G={G}" if G > 1 else "")
    if key not in FOUND:
        _, lib = _lib()
        form = lambda m: lib.gm_bn_fused_form(m, 64, int(bwd), G)  # noqa: E731
        reached = lambda m: form(m) in ORDER and ORDER.index(form(m)) >= ORDER.index(target)  # noqa: E731
        lo, hi = 1, 1 << 21
        assert form(hi) == -1, f"the planner never streams at C = 64 (form {form(hi)} at M = {hi})"
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if reached(mid) else (mid + 1, hi)
        assert form(lo) == target and form(lo - 1) != target, (lo, form(lo), form(lo - 1))
        FOUND[key] = lo
    return FOUND[key]


def _module(c, dtype, momentum):
    from greedy_multimodal_learning_amd.bn import GMBatchNorm2d
    m = GMBatchNorm2d(c.C, momentum=momentum).to(DEV).to(memory_format=torch.channels_last).train()
    with torch.no_grad():
        m.weight.copy_(c.gamma)
        m.bias.copy_(c.beta)
        m.running_mean.copy_(c.rm)
        m.running_var.copy_(c.rv)
    return m


def _train_case(shape, form, dtype, path, expect=None, bwd_two_kernel=False):
    """One GMBatchNorm2d forward + backward against the reference; expect(ff, fb): the variant
    assertion of the row.  bwd_two_kernel: the backward takes the two launches whatever the planner
    answers (a residual gradient without ReLU), so its K is the two-launch plan's.  Returns the
    forms reached."""
    from greedy_multimodal_learning_amd import bn as B
    name, relu, res, maskx = form
    c = case(shape)
    bf16 = dtype == BF
    momentum = 1.0 if name == "plain" else 0.1
    ff, fb, kf, kb = plan(c.M, c.C) if bf16 else (0, 0, 16, 16)
    if bwd_two_kernel and bf16:
        fb, kb = 0, 16 + R.chain(R.two_kernel_rows(c.M, c.C)[0], c.C)
    if expect is not None:
        expect(ff, fb)
    x, dy, r, *_ = R.device_inputs(c, DEV, dtype)
    m = _module(c, dtype, momentum)
    xg = x.clone().requires_grad_(True)
    rg = r.clone().requires_grad_(True) if res else None
    old = B.MASK_FROM_X
    B.MASK_FROM_X = maskx
    try:
        y = m(xg, residual=rg, relu=relu)
        sm, si = y.grad_fn.saved_tensors[4:6]
        y.backward(dy)
    finally:
        B.MASK_FROM_X = old
    assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
    what = f"{path} {ids(shape)} {name}"
    f = fref(shape, 0, relu, res)
    wy, mask = R.check_forward(f, R.rows(y), bf16, what)
    out = {"y": wy}
    out.update(R.check_stats(c, f, kf, momentum, what, save_mean=sm, save_invstd=si, running_mean=m.running_mean,
                             running_var=m.running_var))
    assert int(m.num_batches_tracked) == 1
    b = R.backward_ref(c, f, mask=mask)
    out.update(R.check_backward(c, b, kb, bf16, what, dx=R.rows(xg.grad), dres=R.rows(rg.grad) if res else None,
                                dgamma=m.weight.grad.double().cpu(), dbeta=m.bias.grad.double().cpu()))
    fwd = {k: v for k, v in out.items() if k in ("y", "save_mean", "save_invstd", "running_mean", "running_var")}
    bwd = {k: v for k, v in out.items() if k not in fwd}
    note(path, variant(ff) if bf16 else "fp64 sums", fwd)
    note(path, variant(fb) if bf16 else "fp64 sums", bwd)
    return ff, fb


# ---- 0. the planner query ------------------------------------------------------------------

def test_planner_query_is_read_only_and_matches_the_two_kernel_plan(fused_mode):
    _, lib = _lib()
    fused_mode(0)
    for M, C in [(75, 8), (98, 128), (693, 64), (4, 2048), (1568, 256), (70000, 64), (1 << 20, 64)]:
        for bwd in (0, 1):
            assert lib.gm_bn_fused_form(M, C, bwd, 1) == 0
            assert lib.gm_bn_plan_rows(M, C, bwd, 1) == R.two_kernel_rows(M, C)[0]
    fused_mode(1)
    assert all(lib.gm_bn_fused_form(M, 64, b, 1) >= 0 for M in (693, 70000, 1 << 20) for b in (0, 1))
    fused_mode(2)
    assert lib.gm_bn_fused_form(693, 64, 0, 1) in (4, 8, 16) and lib.gm_bn_fused_form(693, 64, 1, 1) in (4, 8)
    assert lib.gm_bn_fused_form(0, 64, 0, 1) == 0 and lib.gm_bn_fused_form(64, 24, 0, 1) == 0
    assert lib.gm_bn_fused_form(64, 64, 0, 0) == 0 and lib.gm_bn_plan_rows(64, 4096, 0, 1) == 0


# ---- 1. GMBatchNorm2d, bf16, the three modes -------------------------------------------------

@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("shape", R.EXACT_SHAPES + R.INEXACT_SHAPES, ids=ids)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bn_bf16(mode, shape, form, fused_mode):
    fused_mode(mode)

    def expect(ff, fb):
        if mode == 0:
            assert ff == 0 and fb == 0, (ff, fb)
        else:   # these maps fit the register-held strips
            assert ff in (4, 8, 16) and fb in (4, 8), (ff, fb)
    ff, fb = _train_case(shape, form, BF, "GMBatchNorm2d bf16", expect)
    FOUND[f"mode {mode} {ids(shape)}"] = (ff, fb)


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("which,target", [("fwd", 8), ("fwd", 16), ("fwd", -1), ("bwd", 8), ("bwd", -1)],
                         ids=["fwd-NR8", "fwd-NR16", "fwd-streaming", "bwd-NR8", "bwd-streaming"])
def test_bn_bf16_larger_variants(which, target, form, fused_mode):
    """The smallest map whose forward (backward) takes the wider register-held strips or streams
    (x re-read by the apply phase); the row fails if the launch does not take that form."""
    fused_mode(2)
    M = smallest_m(which == "bwd", target)
    shape = (1, 64, 1, M)

    def expect(ff, fb):
        assert (fb if which == "bwd" else ff) == target, f"M = {M}: forms {ff}, {fb}, wanted {target}"
    _train_case(shape, form, BF, "GMBatchNorm2d bf16", expect)


# ---- 2. GMBatchNorm2d, fp32 ------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("shape", R.EXACT_SHAPES + R.INEXACT_SHAPES, ids=ids)
def test_bn_f32(shape, form):
    _train_case(shape, form, F32, "GMBatchNorm2d fp32")


# ---- 2b. a residual without ReLU ---------------------------------------------------------------

RES_PLAIN = ("res_plain", False, True, True)


@pytest.mark.parametrize("target", [0, 4, 8, 16, -1, "fp32"],
                         ids=["two-kernel", "NR4", "NR8", "NR16", "streaming", "fp32"])
def test_bn_residual_without_relu(target, fused_mode):
    """y = x sc + sh + r with no ReLU: no ResNet block has the form and no other row launches its
    kernels - k_bn_apply<RES, no RELU> in bf16 and fp32, k_bn_fwd_fused<RES, no RELU, NR> at every
    NR (the smallest map that takes each, as the larger-variants rows) and k_bn_apply_bwd<no RELU,
    DRES> in bf16 and fp32: the backward of a residual gradient without ReLU is always the two
    launches - read from the dispatch code (bn_bwd in csrc/batchnorm.hip: the planner is not asked
    when dres && !relu), not observed here - so its K is the two-launch plan's."""
    if target == "fp32":
        _train_case((7, 64, 9, 11), RES_PLAIN, F32, "GMBatchNorm2d fp32")
        return
    fused_mode(0 if target == 0 else 2)
    shape = (7, 64, 9, 11) if target in (0, 4) else (1, 64, 1, smallest_m(False, target))

    def expect(ff, fb):
        assert ff == target, f"{shape}: forward form {ff}, wanted {target}"
    _train_case(shape, RES_PLAIN, BF, "GMBatchNorm2d bf16", expect, bwd_two_kernel=True)


# ---- 3. the stem's fused BatchNorm + ReLU + max-pool -------------------------------------------

def _pooled_dy(c, idx):
    """A pooled gradient with the regime recipe's properties: dy at the pixel each output selected."""
    N, C, H, W = c.shape
    pix = R.pool_pixels(c, idx, 3, 2, 1)
    d = torch.gather(c.dy, 0, pix.reshape(-1, C)).view(pix.shape)          # [N, P, Q, C]
    return d.permute(0, 3, 1, 2).to(DEV, BF)


@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=ids)
def test_relu_maxpool_fused(shape, fused_mode):
    from greedy_multimodal_learning_amd import bn as B
    from greedy_multimodal_learning_amd.pool import GMMaxPool2d
    assert B.FUSE_POOL and B.MASK_FROM_X
    fused_mode(2)
    c = case(shape)
    ff, fb, _, kb = plan(c.M, c.C)
    kf = 16 + R.chain(R.two_kernel_rows(c.M, c.C)[0], c.C)   # gm_bn_fwd_stats_bf16: the two-launch reduce
    x, *_ = R.device_inputs(c, DEV, BF)
    m = _module(c, BF, 0.1)
    xg = x.clone().requires_grad_(True)
    y = m.relu_maxpool(xg, GMMaxPool2d(kernel_size=3, stride=2, padding=1))
    assert "BNReluPool" in type(y.grad_fn).__name__
    _, coef, _, _, sm, si, idx = y.grad_fn.saved_tensors
    what = f"relu_maxpool {ids(shape)}"
    f = fref(shape, 0, True, False)
    out = {"y": R.check_pool_forward(c, f, y, idx, 3, 2, 1, what)}
    out.update(R.check_stats(c, f, kf, 0.1, what, save_mean=sm, save_invstd=si, running_mean=m.running_mean,
                             running_var=m.running_var))
    assert int(m.num_batches_tracked) == 1
    dyp = _pooled_dy(c, idx)
    y.backward(dyp)
    dz = R.rne(R.pool_gather(c, dyp, y, idx, 3, 2, 1))       # gm_maxpool2d_bwd_bf16 stores bf16
    b = R.backward_ref(c, f, dz=dz)
    out.update(R.check_backward(c, b, kb, True, what, dx=R.rows(xg.grad), dgamma=m.weight.grad.double().cpu(),
                                dbeta=m.bias.grad.double().cpu()))
    note("relu_maxpool FUSE_POOL", f"stats two-kernel, backward {variant(fb)}", out)


# ---- 4. the grouped launches: two view groups with different statistics --------------------------

def _group_modules(shape, G):
    ms = [_module(case(shape, g), BF, 0.1) for g in range(G)]
    return ms


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("shape", [(2, 128, 7, 7), (7, 64, 9, 11), (8, 256, 14, 14)], ids=ids)
@pytest.mark.parametrize("mode", [0, 2])
def test_vbn_two_groups(mode, shape, form, fused_mode, monkeypatch):
    from greedy_multimodal_learning_amd import vtrunk
    name, relu, res, maskx = form
    fused_mode(mode)
    monkeypatch.setattr(vtrunk, "MASK_FROM_X", maskx)
    G = 2
    cs = [case(shape, g) for g in range(G)]
    ff, fb, kf, kb = plan(cs[0].M, cs[0].C, G)
    assert (ff == 0 and fb == 0) if mode == 0 else (ff != 0 and fb != 0), (ff, fb)
    ins = [R.device_inputs(c, DEV, BF) for c in cs]
    cat = lambda i: torch.cat([t[i] for t in ins]).contiguous(memory_format=torch.channels_last)  # noqa: E731
    X = cat(0).requires_grad_(True)
    RS = cat(2).requires_grad_(True) if res else None
    bns = _group_modules(shape, G)
    y = vtrunk.vbn(X, bns, residual=RS, relu=relu)
    sm, si = y.grad_fn.saved_tensors[2:4]
    y.backward(cat(1))
    N = shape[0]
    for g, c in enumerate(cs):
        sl = slice(g * N, (g + 1) * N)
        what = f"vbn G=2 group {g} {ids(shape)} {name} mode {mode}"
        f = fref(shape, g, relu, res)
        wy, mask = R.check_forward(f, R.rows(y[sl]), True, what)
        out = {"y": wy}
        out.update(R.check_stats(c, f, kf, 0.1, what, save_mean=sm[g], save_invstd=si[g],
                                 running_mean=bns[g].running_mean, running_var=bns[g].running_var))
        assert int(bns[g].num_batches_tracked) == 1
        b = R.backward_ref(c, f, mask=mask)
        out.update(R.check_backward(c, b, kb, True, what, dx=R.rows(X.grad[sl]),
                                    dres=R.rows(RS.grad[sl]) if res else None,
                                    dgamma=bns[g].weight.grad.double().cpu(), dbeta=bns[g].bias.grad.double().cpu()))
        note("vtrunk.vbn G=2", f"forward {variant(ff)}, backward {variant(fb)}", out)


@pytest.mark.parametrize("dres", [True, False], ids=["dres", "nodres"])
@pytest.mark.parametrize("target", [4, 8, -1], ids=["bwd-NR4", "bwd-NR8", "bwd-streaming"])
def test_vbn_mask_byte_backward(target, dres, fused_mode, monkeypatch):
    """The backward that reads the forward's ReLU mask bytes in place of y (vtrunk.BN_RELU_MASK:
    k_bn_bwd_fused<BWD_RELU, DRES, NR, YM>), two view groups, residual + ReLU, at the smallest map
    whose backward of two groups takes each form - with the residual's gradient (DRES) and, the
    residual not requiring one, without it.  The row fails if the launch does not take that form
    or the forward stored no mask."""
    from greedy_multimodal_learning_amd import vtrunk
    fused_mode(2)
    monkeypatch.setattr(vtrunk, "BN_RELU_MASK", True)
    G = 2
    shape = (7, 64, 9, 11) if target == 4 else (1, 64, 1, smallest_m(True, target, G))
    cs = [case(shape, g) for g in range(G)]
    ff, fb, kf, kb = plan(cs[0].M, cs[0].C, G)
    assert fb == target, f"M = {cs[0].M}: backward form {fb}, wanted {target}"
    ins = [R.device_inputs(c, DEV, BF) for c in cs]
    cat = lambda i: torch.cat([t[i] for t in ins]).contiguous(memory_format=torch.channels_last)  # noqa: E731
    X = cat(0).requires_grad_(True)
    RS = cat(2).requires_grad_(dres)
    bns = _group_modules(shape, G)
    y = vtrunk.vbn(X, bns, residual=RS, relu=True)
    sm, si, ymask = y.grad_fn.saved_tensors[2:5]
    assert ymask is not None and int(ymask.count_nonzero()) > 0, "the forward stored no ReLU mask bytes"
    y.backward(cat(1))
    assert (RS.grad is not None) == dres
    N = shape[0]
    for g, c in enumerate(cs):
        sl = slice(g * N, (g + 1) * N)
        what = f"vbn mask bytes G=2 group {g} {ids(shape)} {'dres' if dres else 'no dres'}"
        f = fref(shape, g, True, True)
        wy, mask = R.check_forward(f, R.rows(y[sl]), True, what)
        out = {"y": wy}
        out.update(R.check_stats(c, f, kf, 0.1, what, save_mean=sm[g], save_invstd=si[g],
                                 running_mean=bns[g].running_mean, running_var=bns[g].running_var))
        b = R.backward_ref(c, f, mask=mask)
        out.update(R.check_backward(c, b, kb, True, what, dx=R.rows(X.grad[sl]),
                                    dres=R.rows(RS.grad[sl]) if dres else None,
                                    dgamma=bns[g].weight.grad.double().cpu(), dbeta=bns[g].bias.grad.double().cpu()))
        note("vtrunk.vbn G=2 mask bytes", f"backward {variant(fb)}", out)


def test_vstem_pool_backward_two_groups():
    """gm_bn_relu_maxpool2d_fwd_grouped_bf16 and gm_bn_relu_maxpool2d_bwd_grouped_bf16 through vstem's
    BatchNorm + pool function: the pool gradient gathered inside the BatchNorm backward, its channel
    sums taken of the pooled gradient itself (unrounded), dx of the bf16-rounded gathered one."""
    from greedy_multimodal_learning_amd import vtrunk
    assert vtrunk.FUSED_STEM_BWD and vtrunk.STEM_XSEL
    shape, G = (2, 64, 16, 16), 2
    cs = [case(shape, g) for g in range(G)]
    M, C, N = cs[0].M, 64, shape[0]
    ins = [R.device_inputs(c, DEV, BF) for c in cs]
    X = torch.cat([t[0] for t in ins]).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bns = _group_modules(shape, G)
    y = vtrunk._VBNReluPoolFn.apply(X, G, bns, 3, 2, 1, None, *[b.weight for b in bns], *[b.bias for b in bns])
    _, coef, sm, si, idx, xsel = y.grad_fn.saved_tensors[:6]
    assert xsel is not None
    kf = 16 + R.chain(R.two_kernel_rows(M, C)[0], C)           # gm_bn_fwd_stats_grouped_bf16
    items = N * 8 * 8 * (C // 8)                               # k_stem_pool_bn_bwd: <= 4 pixels per item
    nrc = min(-(-M // R.two_kernel_rows(M, C)[0]), 512)
    ipb = -(-(-(-items // nrc)) // 256) * 256
    kb = 16 + 4 * (ipb // 256) + 32
    dyps = [_pooled_dy(c, idx[g * N:(g + 1) * N]) for g, c in enumerate(cs)]
    y.backward(torch.cat(dyps).contiguous(memory_format=torch.channels_last))
    for g, c in enumerate(cs):
        sl = slice(g * N, (g + 1) * N)
        what = f"vstem pool G=2 group {g}"
        f = fref(shape, g, True, False)
        out = {"y": R.check_pool_forward(c, f, y[sl], idx[sl], 3, 2, 1, what)}
        out.update(R.check_stats(c, f, kf, 0.1, what, save_mean=sm[g], save_invstd=si[g],
                                 running_mean=bns[g].running_mean, running_var=bns[g].running_var))
        assert int(bns[g].num_batches_tracked) == 1
        gsum = R.pool_gather(c, dyps[g], y[sl], idx[sl], 3, 2, 1)
        b = R.backward_ref(c, f, dz=R.rne(gsum), dz_stats=gsum)
        out.update(R.check_backward(c, b, kb, True, what, dx=R.rows(X.grad[sl]),
                                    dgamma=bns[g].weight.grad.double().cpu(), dbeta=bns[g].bias.grad.double().cpu()))
        note("vstem BN+pool G=2", "pool-gathering backward", out)


# ---- 5. eval mode ------------------------------------------------------------------------------

def _eval_stats(c):
    """Running statistics in the regimes' image: the batch's own mean and variance as fp32 (tiny in
    regime 2, exactly 0 in regime 3)."""
    f = R.forward_ref(c, False, False)
    rm, rv = f.mean.float(), f.var.float()
    assert bool((rv[c.reg == 3] == 0).all()) and float(rv[c.reg == 2].max()) < 2.5e-4
    return rm, rv


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("form", [f for f in FORMS if f[3]], ids=lambda f: f[0])
@pytest.mark.parametrize("shape", [(3, 8, 5, 5), (7, 64, 9, 11), (8, 256, 14, 14)], ids=ids)
def test_bn_infer(shape, form, dtype):
    from greedy_multimodal_learning_amd.bn import bn_fwd_infer
    name, relu, res, _ = form
    c = case(shape)
    rm, rv = _eval_stats(c)
    x, _, r, w, b, _, _ = R.device_inputs(c, DEV, dtype)
    y = bn_fwd_infer(x, w, b, rm.to(DEV), rv.to(DEV), 1e-5, relu, r if res else None)
    f = R.forward_ref(c, relu, res, mean=rm, var=rv)
    wy, _ = R.check_forward(f, R.rows(y), dtype == BF, f"infer {ids(shape)} {name}")
    note("gm_bn_fwd_infer", "bf16" if dtype == BF else "fp32", {"y": wy})


def test_bn_infer_coef_table():
    """Two BatchNorms in one gm_bn_infer_coef launch: sc and sh within 8 fp32 ulps of fp64 (fp64
    arithmetic, one rounding), running_var tiny and exactly 0, gamma negative and zero included."""
    L, lib = _lib()
    cs = [case((7, 64, 9, 11)), case((8, 256, 14, 14))]
    keep, ents, coefs, refs = [], [], [], []
    for c in cs:
        rm, rv = _eval_stats(c)
        t = [v.to(DEV) for v in (c.gamma, c.beta, rm, rv)]
        coef = torch.zeros(2 * c.C, device=DEV)
        keep.append(t)
        coefs.append(coef)
        ents.append(L.BnCoefEntry(*[v.data_ptr() for v in t], coef.data_ptr(), c.C, 1e-5))
        f = R.forward_ref(c, False, False, mean=rm, var=rv)
        refs.append(torch.cat([f.sc, f.sh]))
    table = torch.frombuffer(bytearray(bytes(L.arr(L.BnCoefEntry, ents))), dtype=torch.uint8).to(DEV)
    L.check(lib.gm_bn_infer_coef(table.data_ptr(), len(ents), max(c.C for c in cs), L.stream_of(torch.device(DEV))),
            "gm_bn_infer_coef")
    torch.cuda.synchronize()
    for c, coef, ref in zip(cs, coefs, refs):
        got = coef.double().cpu()
        r5 = torch.cat([c.reg == 5, torch.zeros(c.C, dtype=torch.bool)])
        assert bool((got[r5] == 0).all())                                   # gamma = 0: sc = 0 exactly
        w = R.worst_ratio((got - ref).abs(), R.U21 * ref.abs(), f"infer coef C={c.C}")
        note("gm_bn_infer_coef", "table", {"sc, sh": w})


# ---- the record --------------------------------------------------------------------------------

def test_zz_report(capsys):
    """Prints what the rows above measured (worst error / bound per path and variant) and what
    the planner answered; nothing to assert."""
    with capsys.disabled():
        print("\nBatchNorm regimes: worst error / bound")
        for (path, var), d in sorted(WORST.items()):
            print(f"  {path} [{var}]: {R.fmt(d)}")
        print(f"  planner: {FOUND}")
