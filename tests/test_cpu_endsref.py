"""The harness of the pool / loss / metrics edge tests (endsref.py) and the CPU-side conditions of
test_gpu_pool_edges.py, test_gpu_xent_edges.py and test_gpu_eval_metrics.py: the numpy pool scan
equals torch's CPU max_pool2d (values, indices, gradient) at every window, every mutant of a
reference changes or violates at least 1 % of the checked elements or is listed as not checked
there, an fp32 emulation of the loss kernels stays inside the derived bounds at every GPU case,
and the near-tie generator yields inputs on which the two mean formulas disagree.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import endsref as E
import exactint as X

pid = lambda c: "x".join(map(str, c[0])) + "-k%ds%dp%d" % c[1]  # noqa: E731

_pool = {}


def pool_case(shape, win):
    if (shape, win) not in _pool:
        c = E.pool_inputs(shape, win)
        _pool[shape, win] = (c, E.pool_expected(c))
    return _pool[shape, win]


@pytest.mark.parametrize("shape,win", E.POOL_CASES, ids=[pid(c) for c in E.POOL_CASES])
def test_pool_scan_equals_torch(shape, win):
    c, e = pool_case(shape, win)
    k, s, pad = win
    xr = c.x.double().requires_grad_(True)
    y, idx = F.max_pool2d(xr, k, s, pad, return_indices=True)
    y.backward(c.dy.double())
    assert E.same(y.detach(), e.y)
    assert np.array_equal(idx.numpy(), e.arg)
    assert torch.equal(xr.grad, e.dx)
    # in fp32 too (the precision the device reference of the second-trip cases runs in), channels_last
    x32 = c.x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y32, idx32 = F.max_pool2d(x32, k, s, pad, return_indices=True)
    y32.backward(c.dy)
    assert E.same(y32.detach(), e.y) and np.array_equal(idx32.numpy(), e.arg) and torch.equal(x32.grad.double(), e.dx)


@pytest.mark.parametrize("shape,win", E.POOL_CASES, ids=[pid(c) for c in E.POOL_CASES])
def test_pool_inputs_follow_the_recipe(shape, win):
    c, e = pool_case(shape, win)
    N, C, H, W = shape
    k, s, pad = win
    fin = torch.isfinite(c.x)
    assert bool((c.x[fin].abs() <= 7).all()) and torch.equal(c.x[fin], c.x[fin].round())
    assert bool(torch.isnan(c.x).any()) and bool((c.x == float("-inf")).any())
    nan_out = float(torch.isnan(e.y).double().mean())
    assert 0.10 <= nan_out <= 0.60, nan_out
    # ties: many windows without a NaN hold their maximum more than once (k > 1; the channels
    # without planted maxima)
    if k > 1:
        m = E.pool_expected(c, "ge")
        clean = ~torch.isnan(e.y[:, C // 2:])
        tied = float(torch.from_numpy(m.arg != e.arg)[:, C // 2:][clean].double().mean())
        assert tied > 0.25, tied
    # a window of nothing but -inf selects its first in-bounds position, and its gradient lands there
    allinf = e.y[0, C - 1] == float("-inf")
    assert bool(allinf[0, 0]) and int(allinf.sum()) >= (2 if min(e.y.shape[2:]) > 1 else 1)
    assert int(e.arg[0, C - 1, 0, 0]) == 0
    # every routed sum is an integer below 2^24, so fp32 accumulation is exact in any order
    assert torch.equal(e.dx, e.dx.round()) and float(e.dx.abs().max()) < X.LIMIT
    assert torch.equal(e.dx.float().double(), e.dx)
    # pixels no window selects get an exact 0; with stride > k some are not covered at all
    assert bool((e.dx[e.terms == 0] == 0).all())
    assert bool((e.terms == 0).any()) or (k, s) == (1, 1)     # the identity pool selects every pixel
    if s > k:
        covered = torch.from_numpy(E.terms(E.pool_scan(np.zeros(shape), k, s, pad, "ge")[1], H, W)
                                   + E.terms(E.pool_scan(np.zeros(shape), k, s, pad)[1], H, W)) > 0
        assert not bool(covered[:, :, k, :].any())          # row k lies between the windows
    if c.planted is not None:
        assert int(c.planted.sum()) > 0 and c.nterm == (-(-k // s)) ** 2
        assert bool((e.terms[c.planted] == c.nterm).all())


@pytest.mark.parametrize("shape,win", E.POOL_CASES, ids=[pid(c) for c in E.POOL_CASES])
def test_pool_mutants_change_the_expected_result(shape, win, capsys):
    c, e = pool_case(shape, win)
    rates = E.assert_pool_discriminates(c, e)
    assert ("truncated" in rates) == (win in E.TRUNC_WINDOWS)
    skipped = [n for n in rates if (shape, win, n) in E.NOT_CHECKED]
    with capsys.disabled():
        print(f"\n  pool mutants {pid((shape, win))}: {E.fmt(rates)}" + (f"; not checked: {skipped}" if skipped else ""))


def test_not_checked_list_names_real_cases():
    names = {"ge", "stickynan", "skipnan_dx", "skipnan_y", "truncated"}
    for (shape, win, name), reason in E.NOT_CHECKED.items():
        assert (shape, win) in E.POOL_CASES and name in names and reason
    # the NaN-skipping mutant is checked on y everywhere
    assert not any(n == "skipnan_y" for _, _, n in E.NOT_CHECKED)


# ---- loss -----------------------------------------------------------------------------------------

XCASES = [(c, k) for c in E.XENT_CASES for k in E.XENT_SETS]
xid = lambda ck: "x".join(map(str, ck[0])) + "-" + ck[1]  # noqa: E731


@pytest.mark.parametrize("case,kind", XCASES, ids=[xid(c) for c in XCASES])
def test_xent_emulation_inside_bounds_and_mutants_outside(case, kind, capsys):
    x, y = E.xent_inputs(case, kind)
    nb, B, N = case
    assert bool(torch.isfinite(x[:, torch.arange(B), y]).all())
    if kind == "neginf":
        frac = float((x == float("-inf")).double().mean())
        assert 0.25 < frac < 0.35
    ref = E.xent_ref(x, y)
    assert bool(torch.isfinite(ref.b_grad).all()) and bool(torch.isfinite(ref.b_row).all())
    e = E.emulate_xent(x, y)
    fr = E.xent_fractions(ref, e.lse, e.rows, e.loss, e.grad)
    for name, v in fr.items():
        assert v <= 1.0, f"{case} {kind}: the fp32 emulation uses {v:.3f} of the {name} bound"
    rates = E.xent_mutant_rates(x, y, ref)
    skipped = []
    for name, r in rates.items():
        if not E.xent_mutant_applies(case, kind, name):
            skipped.append(name)
            continue
        assert r >= E.FLOOR, f"{case} {kind}: the {name} mutant violates its bound on only {r:.4f}"
    with capsys.disabled():
        print(f"\n  xent {xid((case, kind))}: used {E.fmt(fr)}; mutants {E.fmt(rates)}"
              + (f"; not applicable: {skipped}" if skipped else ""))


def test_xent_no_shift_is_non_finite_on_the_shifted_and_wide_inputs():
    for kind in ("n3_shift", "n60", "n200_shift"):
        x, y = E.xent_inputs(E.XENT_CASES[0], kind)
        assert not np.isfinite(E.emulate_xent(x, y, shift=False).loss)
        assert np.isfinite(E.emulate_xent(x, y).loss)


def test_xent_cases_take_the_row_loop_more_than_once():
    assert [-(-nb * B // 256) for nb, B, _ in E.XENT_CASES] == [2, 3, 3, 3, 2]


# ---- metrics: near ties ------------------------------------------------------------------------------

def test_torch_cpu_mean_is_the_division():
    """torch.stack(...).mean(0) on the CPU is the sum in branch order divided by nbranch, bit for
    bit, and the reciprocal multiply differs from it by an ulp on about a third of random triples."""
    g = torch.Generator().manual_seed(5)
    for nb in E.NEAR_TIE_BRANCHES:
        x = torch.randn(nb, 200000, generator=g) * 3
        s = x[0].clone()
        for i in range(1, nb):
            s = s + x[i]
        want = torch.stack([x[i] for i in range(nb)]).mean(0)
        assert torch.equal(E.mean_div(s, nb), want)
        differ = float((E.mean_mul(s, nb) != want).double().mean())
        assert 0.05 < differ < 0.6, (nb, differ)


@pytest.mark.parametrize("nb", E.NEAR_TIE_BRANCHES)
@pytest.mark.parametrize("collapse", ["div", "mul"])
def test_near_tie_inputs_split_the_two_formulas(nb, collapse):
    from greedy_multimodal_learning_amd.losses import acc
    B, N = 257, 40
    x, y = E.near_tie_logits(nb, B, N, collapse)
    assert int((x != 0).sum()) == 2 * B
    d, m = E.top1_by(x, nb, E.mean_div), E.top1_by(x, nb, E.mean_mul)
    first, second = (d, m) if collapse == "div" else (m, d)
    assert bool((first == 1).all()) and bool((second == 2).all())     # the collapse moves the argmax
    outs = [x[i] for i in range(nb)]
    assert torch.equal(torch.stack(outs).mean(0).argmax(1), d)        # losses.acc on the CPU divides
    hits = lambda t: int((t == y).sum())  # noqa: E731
    assert int(round(float(acc(outs, y)) * B / 100)) == hits(d)
    assert abs(hits(d) - hits(m)) >= B // 3 - 1 and min(hits(d), hits(m)) > 0
