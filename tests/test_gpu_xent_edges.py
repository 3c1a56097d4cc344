"""gm_xent_fwd / gm_xent_bwd (csrc/xent.hip) past the first trip of their row loop and at the
logits a diverging or a confident model produces, against an fp64 log-softmax with per-row and
per-element bounds derived in endsref.py (not fitted): one 256-thread workgroup strides over
nbranch * B rows, and the suite's largest case so far had 132.

Input sets: N(0, 3^2), the same shifted by 1e4 (the max shift carries everything), N(0, 60^2) and
N(0, 200^2) - 3e4 (exp underflows for most classes), and N(0, 3^2) with 30 % of each row at -inf.
test_cpu_endsref.py shows that an fp32 emulation of the kernels stays inside the bounds on these
very tensors and that a missing max shift, a max not added back and a division by nbranch * B
each fall outside them."""
import pytest
import torch
import torch.nn.functional as F

import endsref as E

pytestmark = pytest.mark.gpu

CASES = [(c, k) for c in E.XENT_CASES for k in E.XENT_SETS]
xid = lambda ck: "x".join(map(str, ck[0])) + "-" + ck[1]  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _fwd_abi(x, y):
    """lse [nb, B] and the loss through the C ABI (the autograd path keeps lse to itself)."""
    from greedy_multimodal_learning_amd import _lib as L
    nb, B, N = x.shape
    lse = torch.empty(nb * B, device=x.device, dtype=torch.float32)
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    L.check(L.load().gm_xent_fwd(x.data_ptr(), nb, B, N, y.data_ptr(), lse.data_ptr(), loss.data_ptr(),
                                 L.stream_of(x.device)), "gm_xent_fwd")
    return lse.view(nb, B), loss


@pytest.mark.parametrize("case,kind", CASES, ids=[xid(c) for c in CASES])
def test_xent_within_derived_bounds(dev, case, kind):
    from greedy_multimodal_learning_amd.head import branch_xent
    nb, B, N = case
    assert nb * B > 256                                    # more than one trip of k_xent_fwd's row loop
    x, y = E.xent_inputs(case, kind)
    ref = E.xent_ref(x, y)
    xd, yd = x.to(dev).contiguous(), y.to(dev)
    lse, loss_abi = _fwd_abi(xd, yd)
    outs = [xd[i].clone().requires_grad_(True) for i in range(nb)]
    loss = branch_xent(outs, yd)
    (loss * E.XENT_G).backward()
    grad = torch.stack([o.grad for o in outs]).cpu()
    loss = loss.detach()
    assert float(loss) == float(loss_abi)                  # the same launch either way
    fr = E.xent_fractions(ref, lse=lse.cpu(), loss=float(loss), grad=grad)
    print(f"xent {xid((case, kind))}: fractions of the bounds used: {E.fmt(fr)}")
    for name, v in fr.items():
        assert v <= 1.0, f"{case} {kind}: {name} uses {v:.3f} of its bound"
    # against PyTorch's own fp64 cross-entropy: the reference is what the loss is defined by
    want = sum(F.cross_entropy(x[i].double(), y) for i in range(nb))
    assert abs(float(ref.loss) - float(want)) <= 1e-12 * abs(float(want))
    if kind == "neginf":                                   # exp(-inf) = 0: no gradient, no NaN
        assert bool((grad[x == float("-inf")] == 0).all())


@pytest.mark.parametrize("what", ["plus_inf", "all_minus_inf"])
def test_xent_non_finite_rows_give_nan_as_torch(dev, what):
    """A row holding +inf, or nothing but -inf, has no log-softmax: F.cross_entropy returns NaN
    and so does the kernel - from a row of the loop's second trip as well as of its first."""
    from greedy_multimodal_learning_amd.head import branch_xent
    nb, B, N = 3, 100, 40
    x, y = E.xent_inputs((nb, B, N), "n3")
    for br, b in ((0, 5), (2, 90)):                        # rows 5 and 290
        bad = x.clone()
        if what == "plus_inf":
            bad[br, b, (int(y[b]) + 1) % N] = float("inf")
        else:
            bad[br, b, :] = float("-inf")
        want = sum(F.cross_entropy(bad[i], y) for i in range(nb))
        assert bool(torch.isnan(want))
        got = branch_xent([bad[i].to(dev) for i in range(nb)], y.to(dev))
        assert bool(torch.isnan(got)), (what, br, b, float(got))
    good = branch_xent([x[i].to(dev) for i in range(nb)], y.to(dev))
    assert bool(torch.isfinite(good))
