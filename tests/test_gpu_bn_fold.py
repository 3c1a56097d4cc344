"""The BatchNorm finalize folded into its apply launch (k_bn_finalize_apply,
k_bn_bwd_finalize_apply): gm_bn_fwd_finalize_apply_grouped_bf16_ex and
gm_bn_bwd_finalize_apply_grouped_bf16_ex with an explicit block count nb (so the host rule,
which may decline a shape, cannot hide a case) against the two existing launches -
gm_bn_fwd_stats_finalize_grouped + gm_bn_fwd_apply_grouped_bf16 and
gm_bn_bwd_stats_finalize_grouped + gm_bn_bwd_apply_grouped_bf16 - on the same inputs.

Every comparison is torch.equal; bf16 and fp32 tensors are compared as integers so NaN
payloads count.
The partial rows are built here from x itself: fp32 sums of x and x^2 (forward) or of dz and
dz (x - mean) (backward) over disjoint pixel chunks, in the documented
[G][C / 64][rows][64 x 2] layout followed by 2C floats of coefficient area per group.

The cases are where the combine loop and the streaming loop can go wrong: rows = 1, 33 (a row
group with two rows), 257 (second pass of the 256-row loop), 300 (ragged); C = 64 (one slice),
128, 512; M = 1, 105 (3 x 5 x 7: no multiple of a block's 128 pixels) and 3136; nb = 1 and an nb
that does not divide the 128-pixel chunks; G = 1, 2, 3 evenly strided and separately allocated;
the four residual / ReLU forms with the mask bytes; NaN and Inf in x and NaN in the residual;
two consecutive calls so the running state advances twice.

The residual-affine form (gm_bn_fwd_finalize_apply_res_affine_grouped_bf16_ex: the residual is
the raw input of its own BatchNorm, which the same launch finalizes and applies inside the
block-output apply) is compared against that BatchNorm's finalize + apply followed by the
block-output BatchNorm's finalize + residual apply: C = 128, M = 105 and 3136, G = 2, with and
without ReLU, folded (explicit nb) and through the rule's declining path (two finalizes and the
residual-affine k_bn_apply), NaN / Inf included."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _lib():
    from greedy_multimodal_learning_amd import _lib as L
    return L, L.load()


def _bits(t):  # NaN payloads count (and NaN == NaN): floating tensors compared as integers
    return t.view({BF: torch.int16, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what} differs from the two launches"


def _tensors(G, M, C, seed, strided, dev):
    """G bf16 [M, C] tensors: evenly strided (M * C elements apart) or 128 bytes further apart
    each, which the strided test of the apply entry points rejects."""
    g = torch.Generator().manual_seed(seed)
    gap = 0 if strided else 64
    buf = torch.zeros(G * (M * C + gap), dtype=BF, device=dev)
    out = [buf[i * (M * C + gap):i * (M * C + gap) + M * C].view(M, C) for i in range(G)]
    for t in out:
        t.copy_(torch.randn(M, C, generator=g).to(BF))
    return out


def _regime(G, M, C, dev):
    """The regime inputs of tests/bnregimes.py (|mean|/std ~ 26, var ~ 1e-4 and 0, negative, zero,
    tiny and large gamma; a gradient with a mean, correlated with x): one case per group."""
    import bnregimes as R
    cs = [R.build((1, C, 1, M), R.seed((1, C, 1, M), g), res=True) for g in range(G)]
    return cs, [c.gamma.to(dev) for c in cs], [c.beta.to(dev) for c in cs]


def _fill(ts, srcs):
    for t, s in zip(ts, srcs):
        t.copy_(s.to(BF))


def _rows_of(a, b, rows):
    """[C / 64][rows][64][2] partial rows: sums of a and b ([M, C] fp32) over `rows` disjoint
    pixel chunks (empty chunks, rows > M, are zero rows)."""
    M, C = a.shape
    out = torch.zeros(C // 64, rows, 64, 2, device=a.device, dtype=torch.float32)
    bounds = [(M * r) // rows for r in range(rows + 1)]
    for r in range(rows):
        lo, hi = bounds[r], bounds[r + 1]
        if hi > lo:
            out[:, r, :, 0] = a[lo:hi].sum(0).view(C // 64, 64)
            out[:, r, :, 1] = b[lo:hi].sum(0).view(C // 64, 64)
    return out


def _fwd_stats(xs, rows):
    G, (M, C) = len(xs), xs[0].shape
    st = torch.zeros(G, (rows + 1) * 2 * C, device=xs[0].device, dtype=torch.float32)
    for g, x in enumerate(xs):
        xf = x.float()
        st[g, :rows * 2 * C] = _rows_of(xf, xf * xf, rows).reshape(-1)
    return st


def _run_fwd(xs, ress, relu, rows, nb, calls=1, mask=True, strided=True, par=None):
    """Both arms `calls` times; returns per arm the list of every output tensor.  par: the
    groups' (gammas, betas) in place of the drawn ones."""
    L, lib = _lib()
    dev = xs[0].device
    G, (M, C) = len(xs), xs[0].shape
    stream = L.stream_of(dev)
    g = torch.Generator().manual_seed(C + rows)
    gam = [(torch.rand(C, generator=g) + 0.5).to(dev) for _ in range(G)]
    bet = [(torch.rand(C, generator=g) - 0.5).to(dev) for _ in range(G)]
    rm0 = [(torch.rand(C, generator=g) * 0.2 - 0.1).to(dev) for _ in range(G)]
    if par is not None:
        gam, bet = par
    stats0 = _fwd_stats(xs, rows)
    outs = []
    for arm in ("two", "fold"):
        stats = stats0.clone()
        ys = _tensors(G, M, C, 99, strided, dev)
        rm = [t.clone() for t in rm0]
        rv = [torch.ones(C, device=dev) for _ in range(G)]
        nbt = [torch.zeros((), device=dev, dtype=torch.int64) for _ in range(G)]
        sm, si = torch.zeros(G, C, device=dev), torch.zeros(G, C, device=dev)
        coef = torch.zeros(G, 2 * C, device=dev)
        want_mask = mask and relu and ress is not None
        mk = torch.zeros(G, M * C // 8, device=dev, dtype=torch.uint8) if want_mask else None
        descs = [L.BnFwd(M, C, int(relu), xs[i].data_ptr(), ress[i].data_ptr() if ress is not None else 0,
                         ys[i].data_ptr(), gam[i].data_ptr(), bet[i].data_ptr(), rm[i].data_ptr(), rv[i].data_ptr(),
                         0.1, 1e-5, sm[i].data_ptr(), si[i].data_ptr(), nbt[i].data_ptr(), coef[i].data_ptr(),
                         mk[i].data_ptr() if mk is not None else 0) for i in range(G)]
        arr = L.arr(L.BnFwd, descs)
        for _ in range(calls):
            if arm == "two":
                L.check(lib.gm_bn_fwd_stats_finalize_grouped(arr, G, stats.data_ptr(), rows, stream), "finalize")
                L.check(lib.gm_bn_fwd_apply_grouped_bf16(arr, G, stats.data_ptr(), rows, stream), "apply")
            else:
                L.check(lib.gm_bn_fwd_finalize_apply_grouped_bf16_ex(arr, G, stats.data_ptr(), rows, nb, stream),
                        "finalize_apply")
        torch.cuda.synchronize()
        outs.append(dict(y=torch.stack([y.reshape(-1) for y in ys]), mask=mk, save_mean=sm, save_invstd=si,
                         running_mean=torch.stack(rm), running_var=torch.stack(rv),
                         num_batches_tracked=torch.stack(nbt), coef_out=coef, stats=stats))
    return outs


def _check(outs):
    a, b = outs
    for k in a:
        if a[k] is not None:
            _same(b[k], a[k], k)


def _fwd_case(M, C, rows, G, res, relu, nb, strided=True, calls=1, poison=False, regime=False):
    dev = torch.device("cuda:0")
    xs = _tensors(G, M, C, 1000 * rows + M + C, strided, dev)
    ress = _tensors(G, M, C, 7 + M, strided, dev) if res else None
    par = None
    if regime:
        cs, *par = _regime(G, M, C, dev)
        _fill(xs, [c.x for c in cs])
        if res:
            _fill(ress, [c.res for c in cs])
    if poison:
        xs[0][M // 2, 3] = float("nan")
        xs[G - 1][M - 1, C - 1] = float("inf")
        if ress is not None:
            ress[0][0, 9] = float("nan")
    outs = _run_fwd(xs, ress, relu, rows, nb, calls, strided=strided, par=par)
    _check(outs)
    return outs


@pytest.mark.parametrize("rows", [1, 33, 257, 300])
def test_forward_rows(rows):
    _fwd_case(105, 128, rows, 2, True, True, 3)


@pytest.mark.parametrize("C", [64, 128, 512])
def test_forward_channels(C):
    _fwd_case(105, C, 33, 2, True, True, 2)


@pytest.mark.parametrize("M,nb", [(1, 1), (1, 3), (105, 1), (105, 3), (3136, 1), (3136, 7), (3136, 25)])
def test_forward_pixels_and_blocks(M, nb):
    """3136 pixels are 24.5 chunks of 128: nb = 7 divides neither the chunks nor the four-chunk
    batches; nb = 25 gives every block one (the last a ragged) chunk; nb = 3 at M = 1 leaves
    blocks without a pixel."""
    outs = _fwd_case(M, 128, 33, 2, True, True, nb)
    assert int(outs[1]["num_batches_tracked"][0]) == 1


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("strided", [True, False], ids=["strided", "separate"])
def test_forward_groups(G, strided):
    _fwd_case(105, 128, 33, G, True, True, 2, strided=strided)


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu"])
def test_forward_residual_relu_forms(res, relu):
    outs = _fwd_case(3136, 128, 25, 2, res, relu, 5)
    if res and relu:
        assert outs[1]["mask"] is not None and int(outs[1]["mask"].count_nonzero()) > 0


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
def test_forward_nan_inf(res):
    outs = _fwd_case(105, 128, 33, 2, res, True, 3, poison=True)
    assert bool(outs[1]["y"].float().isnan().any())


def test_forward_regime_inputs():
    """The regime inputs through both arms (residual + ReLU with the mask bytes, two groups)."""
    outs = _fwd_case(3136, 128, 25, 2, True, True, 5, regime=True)
    assert int(outs[1]["mask"].count_nonzero()) > 0


def test_forward_running_state_two_calls():
    outs = _fwd_case(105, 128, 33, 2, True, True, 3, calls=2)
    assert [int(v) for v in outs[1]["num_batches_tracked"]] == [2, 2]


def test_forward_rule_entry_matches():
    """The plain entry point (the rule picks the blocks, or declines and issues the two
    launches itself) on a shape it folds and on one it declines."""
    L, lib = _lib()
    dev = torch.device("cuda:0")
    stream = L.stream_of(dev)
    for M, C, rows in ((3136, 512, 25), (3136, 128, 1200)):
        xs = _tensors(2, M, C, 5, True, dev)
        outs = _run_fwd(xs, None, True, rows, max(1, lib.gm_bn_fold_blocks(M, C, rows, 2)))
        _check(outs)
        # the rule's own choice through the plain entry point
        stats = _fwd_stats(xs, rows)
        y = torch.zeros(2, M, C, device=dev, dtype=BF)
        sm, si = torch.zeros(2, C, device=dev), torch.zeros(2, C, device=dev)
        g = torch.Generator().manual_seed(C + rows)
        gam = [(torch.rand(C, generator=g) + 0.5).to(dev) for _ in range(2)]
        bet = [(torch.rand(C, generator=g) - 0.5).to(dev) for _ in range(2)]
        descs = [L.BnFwd(M, C, 1, xs[i].data_ptr(), 0, y[i].data_ptr(), gam[i].data_ptr(), bet[i].data_ptr(), 0, 0,
                         0.1, 1e-5, sm[i].data_ptr(), si[i].data_ptr(), 0, 0, 0) for i in range(2)]
        L.check(lib.gm_bn_fwd_finalize_apply_grouped_bf16(L.arr(L.BnFwd, descs), 2, stats.data_ptr(), rows, stream),
                "finalize_apply")
        torch.cuda.synchronize()
        _same(y.reshape(2, -1), outs[0]["y"], f"y (rule, rows {rows})")
        _same(sm, outs[0]["save_mean"], "save_mean (rule)")


# ---- backward from producer statistics ---------------------------------------------------

def _bwd_case(M, C, rows, G, relu, nb, accumulate, strided=True, regime=False):
    L, lib = _lib()
    dev = torch.device("cuda:0")
    stream = L.stream_of(dev)
    xs = _tensors(G, M, C, 31 * rows + M + C, strided, dev)
    dys = _tensors(G, M, C, 17 + M + C, strided, dev)
    g = torch.Generator().manual_seed(C + rows + M)
    gam = [(torch.rand(C, generator=g) + 0.5).to(dev) for _ in range(G)]
    bet = [torch.full((C,), 0.1, device=dev) for _ in range(G)]
    if regime:
        cs, gam, bet = _regime(G, M, C, dev)
        _fill(xs, [c.x for c in cs])
        _fill(dys, [c.dy for c in cs])
    mean = torch.stack([x.float().mean(0) for x in xs])
    var = torch.stack([x.float().var(0, unbiased=False) for x in xs])
    invstd = (var + 1e-5).rsqrt()
    # the forward's coefficients: the mask is x * sc + sh > 0
    fcoef = torch.stack([torch.cat([gam[i] * invstd[i], bet[i] - mean[i] * gam[i] * invstd[i]]) for i in range(G)])
    fcoef = fcoef.contiguous()
    off = lib.gm_bn_bwd_stats_coef_offset(C, G, rows)
    stats0 = torch.zeros(off + G * 4 * C, device=dev, dtype=torch.float32)
    for i in range(G):
        xf, dz = xs[i].float(), dys[i].float()
        if relu:
            dz = torch.where(torch.addcmul(fcoef[i, C:], xf, fcoef[i, :C]) > 0, dz, torch.zeros_like(dz))
        blk = _rows_of(dz, dz * (xf - mean[i]), rows).reshape(-1)
        stats0[i * (rows + 1) * 2 * C:i * (rows + 1) * 2 * C + blk.numel()] = blk
    outs = []
    for arm in ("two", "fold"):
        stats = stats0.clone()
        dxs = _tensors(G, M, C, 3, strided, dev)
        dg = torch.full((G, C), 0.25, device=dev)
        db = torch.full((G, C), -0.5, device=dev)
        descs = [L.BnBwd(M, C, int(relu), dys[i].data_ptr(), 0, xs[i].data_ptr(), gam[i].data_ptr(),
                         mean[i].data_ptr(), invstd[i].data_ptr(), dxs[i].data_ptr(), 0, dg[i].data_ptr(),
                         db[i].data_ptr(), int(accumulate), 0, fcoef[i].data_ptr() if relu else 0, 0)
                 for i in range(G)]
        arr = L.arr(L.BnBwd, descs)
        if arm == "two":
            L.check(lib.gm_bn_bwd_stats_finalize_grouped(arr, G, stats.data_ptr(), rows, stream), "finalize")
            L.check(lib.gm_bn_bwd_apply_grouped_bf16(arr, G, stats.data_ptr(), rows, stream), "apply")
        else:
            L.check(lib.gm_bn_bwd_finalize_apply_grouped_bf16_ex(arr, G, stats.data_ptr(), rows, nb, stream),
                    "finalize_apply")
        torch.cuda.synchronize()
        outs.append(dict(dx=torch.stack([d.reshape(-1) for d in dxs]), dgamma=dg, dbeta=db, stats=stats))
    _check(outs)
    if accumulate:
        assert not torch.equal(outs[1]["dbeta"], torch.full_like(outs[1]["dbeta"], -0.5))


BWD_CASES = [  # M, C, rows, G, nb, strided
    (105, 128, 1, 2, 3, True),
    (105, 128, 33, 3, 2, False),
    (105, 64, 257, 1, 1, True),
    (1, 128, 300, 2, 3, True),
    (3136, 512, 25, 2, 7, True),
    (3136, 128, 33, 2, 25, False),
]


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu_from_x"])
@pytest.mark.parametrize("accumulate", [0, 1], ids=["write", "accumulate"])
def test_backward(case, relu, accumulate):
    M, C, rows, G, nb, strided = case
    _bwd_case(M, C, rows, G, relu, nb, accumulate, strided)


@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu_from_x"])
def test_backward_regime_inputs(relu):
    _bwd_case(3136, 128, 33, 2, relu, 25, 0, False, regime=True)


# ---- the residual-affine form (a downsample block's output) -------------------------------

def _res_affine_case(M, C, rows, rrows, G, relu, nb, strided=True, poison=False, regime=False):
    L, lib = _lib()
    dev = torch.device("cuda:0")
    stream = L.stream_of(dev)
    xs = _tensors(G, M, C, 11 * rows + M + C, strided, dev)
    rs = _tensors(G, M, C, 13 * rrows + M, strided, dev)   # the raw downsample convolution output
    if poison:
        xs[0][M // 2, 3] = float("nan")
        rs[G - 1][M - 1, C - 1] = float("inf")
        rs[0][0, 9] = float("nan")
    g = torch.Generator().manual_seed(C + rows + rrows)
    par = [[(torch.rand(C, generator=g) + 0.5).to(dev) for _ in range(G)] for _ in range(2)]   # gammas
    par += [[(torch.rand(C, generator=g) - 0.5).to(dev) for _ in range(G)] for _ in range(2)]  # betas
    if regime:  # the block output's BatchNorm on groups 0 .. G - 1, the residual's on the next G cases
        cs, *pz = _regime(2 * G, M, C, dev)
        _fill(xs, [c.x for c in cs[:G]])
        _fill(rs, [c.x for c in cs[G:]])
        par = [pz[0][:G], pz[0][G:], pz[1][:G], pz[1][G:]]
    stats0, rstats0 = _fwd_stats(xs, rows), _fwd_stats(rs, rrows)
    outs = []
    for arm in ("separate", "res_affine"):
        stats, rstats = stats0.clone(), rstats0.clone()
        ys = _tensors(G, M, C, 99, strided, dev)
        ns = _tensors(G, M, C, 98, strided, dev)  # the normalised residual (separate arm only)
        state = {}
        for k in ("", "r"):
            state[k] = dict(rm=[torch.full((C,), 0.05, device=dev) for _ in range(G)],
                            rv=[torch.ones(C, device=dev) for _ in range(G)],
                            nbt=[torch.zeros((), device=dev, dtype=torch.int64) for _ in range(G)],
                            sm=torch.zeros(G, C, device=dev), si=torch.zeros(G, C, device=dev),
                            coef=torch.zeros(G, 2 * C, device=dev))
        mk = torch.zeros(G, M * C // 8, device=dev, dtype=torch.uint8) if relu else None

        def desc(i, k, x, res, y, gam, bet, do_relu, mask):
            s = state[k]
            return L.BnFwd(M, C, int(do_relu), x.data_ptr(), res, y, gam[i].data_ptr(), bet[i].data_ptr(),
                           s["rm"][i].data_ptr(), s["rv"][i].data_ptr(), 0.1, 1e-5, s["sm"][i].data_ptr(),
                           s["si"][i].data_ptr(), s["nbt"][i].data_ptr(), s["coef"][i].data_ptr(), mask)
        mptr = [mk[i].data_ptr() if mk is not None else 0 for i in range(G)]
        if arm == "separate":
            rarr = L.arr(L.BnFwd, [desc(i, "r", rs[i], 0, ns[i].data_ptr(), par[1], par[3], False, 0)
                                   for i in range(G)])
            arr = L.arr(L.BnFwd, [desc(i, "", xs[i], ns[i].data_ptr(), ys[i].data_ptr(), par[0], par[2], relu,
                                       mptr[i]) for i in range(G)])
            L.check(lib.gm_bn_fwd_stats_finalize_grouped(rarr, G, rstats.data_ptr(), rrows, stream), "finalize r")
            L.check(lib.gm_bn_fwd_apply_grouped_bf16(rarr, G, rstats.data_ptr(), rrows, stream), "apply r")
            L.check(lib.gm_bn_fwd_stats_finalize_grouped(arr, G, stats.data_ptr(), rows, stream), "finalize")
            L.check(lib.gm_bn_fwd_apply_grouped_bf16(arr, G, stats.data_ptr(), rows, stream), "apply")
        else:
            rarr = L.arr(L.BnFwd, [desc(i, "r", rs[i], 0, 0, par[1], par[3], False, 0) for i in range(G)])
            arr = L.arr(L.BnFwd, [desc(i, "", xs[i], rs[i].data_ptr(), ys[i].data_ptr(), par[0], par[2], relu,
                                       mptr[i]) for i in range(G)])
            L.check(lib.gm_bn_fwd_finalize_apply_res_affine_grouped_bf16_ex(
                arr, G, stats.data_ptr(), rows, rarr, rstats.data_ptr(), rrows, nb, stream), "res_affine")
        torch.cuda.synchronize()
        o = dict(y=torch.stack([y.reshape(-1) for y in ys]), mask=mk, stats=stats, rstats=rstats)
        for k in ("", "r"):
            s = state[k]
            o.update({k + "save_mean": s["sm"], k + "save_invstd": s["si"], k + "coef_out": s["coef"],
                      k + "running_mean": torch.stack(s["rm"]), k + "running_var": torch.stack(s["rv"]),
                      k + "num_batches_tracked": torch.stack(s["nbt"])})
        outs.append(o)
    _check(outs)
    assert [int(v) for v in outs[1]["rnum_batches_tracked"]] == [1] * G
    return outs


def test_forward_residual_affine_form():
    """The fifth residual / ReLU form, at the shape of test_forward_residual_relu_forms."""
    outs = _res_affine_case(3136, 128, 25, 49, 2, True, 5)
    assert int(outs[1]["mask"].count_nonzero()) > 0


def test_residual_affine_regime_inputs():
    """Both BatchNorms of the residual-affine form on regime inputs: two affines with negative,
    zero and large scales ahead of one ReLU."""
    outs = _res_affine_case(3136, 128, 25, 49, 2, True, 5, regime=True)
    assert int(outs[1]["mask"].count_nonzero()) > 0


@pytest.mark.parametrize("M,nb", [(105, 1), (105, 3), (3136, 7), (3136, 0)])
@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu"])
def test_residual_affine_apply(M, nb, relu):
    """C = 128, G = 2.  nb = 0: the rule; with 700 + 900 rows it declines, so the entry point
    issues the two finalizes and the residual-affine k_bn_apply."""
    L, lib = _lib()
    rows, rrows = (700, 900) if nb == 0 else (33, 65)
    if nb == 0:
        assert lib.gm_bn_fold_blocks(M, 128, rows + rrows, 2) == 0
    _res_affine_case(M, 128, rows, rrows, 2, relu, nb)


@pytest.mark.parametrize("nb", [3, 0])
def test_residual_affine_separate_groups_nan_inf(nb):
    rows, rrows = (700, 900) if nb == 0 else (33, 257)
    outs = _res_affine_case(105, 128, rows, rrows, 3, True, nb, strided=False, poison=True)
    assert bool(outs[1]["y"].float().isnan().any())
