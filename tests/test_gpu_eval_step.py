"""engine.EvalStep: the fused evaluation pass (view-batched eval trunk with the BatchNorms in the
convolution epilogues, the model's MMTM sites, stacked heads, device-side metrics) against the
module forward in eval mode.

Model: MMTM_MVCNN at 64 x 64 inputs with deterministic weights; every BatchNorm gets randomised
running statistics, gamma (both signs) and beta - the initial 0 / 1 / 1 / 0 would hide a swapped
or missing term.  Inputs and parameters are bf16-exact, so the paths differ by their arithmetic
alone.  The bar is the project's bf16 logits bar: 3e-2 of max |logit| (DESIGN section 5,
test_gpu_c2_bf16.py).

The MMTM sites advance their running averages and step counters on every forward, in eval mode
too (balanced_mmtm.py); curation reads those averages.  So every comparison starts both paths
from the same saved site state (_restore)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import weights

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
BAR = 3e-2
H = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _randomise_bn(model, seed):
    from greedy_multimodal_learning_amd.bn import GMBatchNorm2d
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, GMBatchNorm2d):
                C = m.weight.shape[0]
                sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
                m.weight.copy_(((0.5 + torch.rand(C, generator=g)) * sign).bfloat16().float())
                m.bias.copy_((0.3 * torch.randn(C, generator=g)).bfloat16().float())
                m.running_mean.copy_(0.3 * torch.randn(C, generator=g))
                m.running_var.copy_(0.5 * 4 ** torch.rand(C, generator=g))   # [0.5, 2]
                m.num_batches_tracked.fill_(17)


def _build(dev, n_views=2, seed=3, **kw):
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN, MMTM_MVCNN_N
    m = MMTM_MVCNN(**kw) if n_views == 2 else MMTM_MVCNN_N(num_views=n_views, trunk="resnet18", **kw)
    weights.apply_to_module(m, seed=seed)
    for p in m.parameters():
        p.data = p.data.bfloat16().float()
    _randomise_bn(m, seed + 1)
    return m.to(dev)


def _inputs(dev, B, V=2, seed=0):
    g = torch.Generator().manual_seed(1000 + 10 * B + seed)
    x = torch.randn(B, V, 3, H, H, generator=g).bfloat16().to(dev)
    y = torch.randint(0, 40, (B,), generator=g).to(dev)
    return x, y


def _sites(model):
    return [getattr(model, f"mmtm{i}") for i in (2, 3, 4)]


def _site_tensors(m):
    if hasattr(m, "running_avg"):
        return list(m.running_avg)
    return [m.running_avg_weight_visual, m.running_avg_weight_skeleton]


def _snapshot(model):
    return [([t.detach().clone() for t in _site_tensors(m)], m.step) for m in _sites(model)]


def _restore(model, snap):
    for m, (ts, step) in zip(_sites(model), snap):
        for t, s in zip(_site_tensors(m), ts):
            t.copy_(s.to(t.device))
        m.step = step  # (the site re-seeds its device counter when this differs from its mirror)


def _module_path(model, x, dtype, curation=(False, None)):
    """The module forward in eval mode, as train.evaluate runs it; (logits fp32, squeezed)."""
    model.eval()
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
            _, outs, _, sq = model(x if dtype != torch.float32 else x.float(), curation_mode=curation[0],
                                   caring_modality=curation[1])
    finally:
        model.train(True)
    return [o.float() for o in outs], sq


def _err(outs, ref):
    scale = max(float(r.abs().max()) for r in ref)
    return max(float((o - r).abs().max()) for o, r in zip(outs, ref)) / scale


@pytest.fixture(scope="module")
def world(dev):
    """The model, a warmed site state (non-zero running averages) and a fused step."""
    from greedy_multimodal_learning_amd.engine import EvalStep
    torch.manual_seed(0)
    model = _build(dev)
    _module_path(model, _inputs(dev, 4, seed=9)[0], BF)   # the sites' averages leave zero
    return dict(model=model, snap=_snapshot(model), step=EvalStep(model, graphs=False))


@pytest.mark.parametrize("B", [3, 8])
def test_logits_within_the_bf16_bar_of_fp32(dev, world, B):
    model, step = world["model"], world["step"]
    x, y = _inputs(dev, B)
    ref, _ = _module_path(model, x, torch.float32)
    mod, _ = _module_path(model, x, BF)
    step.begin()
    outs, sq = step(x, y)
    assert sq is None and len(outs) == 2 and all(o.dtype == torch.float32 and o.shape == (B, 40) for o in outs)
    e_fused, e_mod = _err(outs, ref), _err(mod, ref)
    print(f"B {B}: max |logit error| / max |logit| vs the fp32 module path: fused {e_fused:.3e}, "
          f"bf16 modules {e_mod:.3e} (bar {BAR})")
    assert e_fused <= BAR
    loss, acc, accm, n = step.result()
    assert n == B and len(accm) == 2
    want = float(sum(F.cross_entropy(o.double(), y) for o in outs))
    assert abs(loss - want) <= 1e-5 * abs(want)


def _pass(step, batches, curation=(False, None)):
    step.begin()
    got = []
    for x, y in batches:
        outs, sq = step(x, y, curation)
        got.append(([o.clone() for o in outs], None if sq is None else [[v.clone() for v in site] for site in sq]))
    return got, step.acc.clone()


def test_graph_replay_equals_eager(dev):
    """Three batches, the last one smaller, over two passes: the second pass replays (the first
    appearance of a shape runs eagerly).  Logits, squeezed maps, accumulators and the sites' state
    are bit-identical to the eager step's."""
    from greedy_multimodal_learning_amd.engine import EvalStep
    model = _build(dev, saving_mmtm_squeeze_array=True)
    _module_path(model, _inputs(dev, 4, seed=9)[0], BF)
    snap = _snapshot(model)
    batches = [_inputs(dev, 4, seed=1), _inputs(dev, 4, seed=2), _inputs(dev, 3, seed=3)]
    res = {}
    for graphs in (False, True):
        _restore(model, snap)
        step = EvalStep(model, graphs=graphs)
        _pass(step, batches)
        res[graphs] = _pass(step, batches) + (_snapshot(model),)
        if graphs:
            assert step.capture_failures == [] and step.graphs and step.replays == 4  # (pass 1: the second 4-batch)
    (ge, ae, se), (gg, ag, sg) = res[False], res[True]
    assert torch.equal(ae, ag)
    for (oe, qe), (og, qg) in zip(ge, gg):
        assert all(torch.equal(a, b) for a, b in zip(oe, og))
        assert len(qe) == len(qg) == 3
        for s1, s2 in zip(qe, qg):
            assert len(s1) == len(s2) == 2 and all(torch.equal(a, b) for a, b in zip(s1, s2))
    for (t1, n1), (t2, n2) in zip(se, sg):
        assert n1 == n2 and all(torch.equal(a, b) for a, b in zip(t1, t2))


def test_state_untouched(dev, world):
    """Parameters and BatchNorm buffers (running statistics, num_batches_tracked): torch.equal
    before and after a fused pass.  The MMTM sites' state is not frozen in eval mode on the module
    path either: the fused pass leaves the step counters the module path leaves, and running
    averages that agree with the module path's within the bf16 bar (they average the excitation
    scales, which carry each path's bf16 rounding) - and that did advance."""
    model, step, snap = world["model"], world["step"], world["snap"]
    batches = [_inputs(dev, 4, seed=1), _inputs(dev, 3, seed=3)]
    _restore(model, snap)
    for x, _ in batches:
        _module_path(model, x, BF)
    after_mod = _snapshot(model)
    _restore(model, snap)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _pass(step, batches)
    torch.cuda.synchronize()
    after = model.state_dict()
    assert set(after) == set(before) and any("running_var" in k for k in before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    for (tf, nf), (tm, nm), (t0, n0) in zip(_snapshot(model), after_mod, snap):
        assert nf == nm == n0 + len(batches)
        for a, b, c in zip(tf, tm, t0):
            assert float((a - b).abs().max()) <= BAR * float(b.abs().max())
            assert not torch.equal(a, c)


@pytest.mark.parametrize("mode", ["mmtm_off", "curation0", "curation1", "squeeze"])
def test_modes_against_the_bf16_module_path(dev, world, mode):
    model, step, snap = world["model"], world["step"], world["snap"]
    x, y = _inputs(dev, 4, seed=5)
    curation = {"curation0": (True, 0), "curation1": (True, 1)}.get(mode, (False, None))
    g = torch.Generator().manual_seed(21)
    try:
        if mode == "mmtm_off":
            model.mmtm_off = True
            model.mmtm_rescale = [None] + [[torch.rand(c, generator=g).to(dev), torch.rand(c, generator=g).to(dev)]
                                           for c in (128, 256, 512)]
        if mode == "squeeze":
            model.saving_mmtm_squeeze_array = True
        _restore(model, snap)
        ref, sq_ref = _module_path(model, x, BF, curation)
        _restore(model, snap)
        step.begin()
        outs, sq = step(x, y, curation)
        e = _err(outs, ref)
        print(f"{mode}: fused vs bf16 modules {e:.3e} (bar {BAR})")
        assert e <= BAR
        if mode == "squeeze":
            assert len(sq) == len(sq_ref) == 3
            for a, b in zip(sq, sq_ref):
                assert len(a) == len(b) == 2
                for u, v in zip(a, b):
                    assert u.is_cuda and u.shape == v.shape and u.dtype == v.dtype
                    assert float((u.cpu() - v).abs().max()) <= BAR * float(v.abs().max())
        else:
            assert sq is None and all(s is None for s in sq_ref)
    finally:
        model.mmtm_off = False
        model.saving_mmtm_squeeze_array = False
        if hasattr(model, "mmtm_rescale"):
            del model.mmtm_rescale


def _decisive_model(dev):
    """A model whose top-1 is decided by a wide margin on 24 given samples, as a trained model's is
    (a randomly initialised one gives every sample nearly the same logits: its top-2 gaps are
    below any bf16 bar).  The inputs are smooth fields that differ strongly between samples; each
    branch's head is a ridge-regularised prototype classifier on that branch's pooled features,
    which come from the pure-PyTorch oracle on the CPU (the HIP head never materialises them):
    class s answers to sample s, classes 24..39 are off.  The ridge (a fifth of the mean
    eigenvalue of the centred Gram matrix) keeps the head well conditioned, so it does not
    amplify the paths' bf16 differences."""
    from oracle import model_ref
    model = _build(torch.device("cpu"), seed=6)
    g = torch.Generator().manual_seed(31)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, H), indexing="ij")
    x = torch.zeros(24, 2, 3, H, H)
    for pl in x.view(-1, H, H):
        fx, fy = torch.randint(0, 4, (2,), generator=g).float()
        ph, amp = torch.rand(1, generator=g) * 6.28, 0.5 + 2 * torch.rand(1, generator=g)
        pl.copy_(2 * torch.randn(1, generator=g) + amp * torch.sin(6.28 * (fx * xx + fy * yy) + ph))
    x = x.bfloat16()
    o = model_ref.MMTM_MVCNN_Ref()
    assert not o.load_state_dict(model.state_dict(), strict=False)[0]
    o.eval()
    feats = [[], []]
    hooks = [getattr(o, f"net_view_{i}").avgpool.register_forward_hook(
        lambda mod, inp, out, i=i: feats[i].append(out.flatten(1))) for i in range(2)]
    with torch.no_grad():
        for i in range(3):   # the batches of the loader: the sites see what they will see
            o(x[8 * i:8 * i + 8].float())
    for h in hooks:
        h.remove()
    with torch.no_grad():
        for i in range(2):
            f = torch.cat(feats[i]).double()
            mu = f.mean(0)
            fc = f - mu
            K = fc @ fc.T
            W = torch.linalg.solve(K + 0.2 * K.trace() / 24 * torch.eye(24, dtype=torch.float64), fc)
            fcm = getattr(model, f"net_view_{i}").fc
            fcm.weight.zero_()
            fcm.bias.fill_(-1.0)
            fcm.weight[:24] = W.float().bfloat16().float()
            fcm.bias[:24] = (-(fcm.weight[:24].double() @ mu)).float().bfloat16().float()
    return model.to(dev), x.to(dev)


def test_evaluate_equivalence(dev):
    """train.evaluate(..., engine=step) against train.evaluate(...) on a 3-batch in-memory loader:
    same keys and indices; per sample the same top-1 wherever the module path's top-2 gap is at
    least the bf16 bar (at most one sample in 24 may fall below it), so the accuracies are equal
    up to those samples; the losses agree within what the paths' logit differences allow
    (cross-entropy is 2-Lipschitz in the max norm of the logits, per branch)."""
    from greedy_multimodal_learning_amd.engine import EvalStep
    from greedy_multimodal_learning_amd.train import evaluate
    model, x = _decisive_model(dev)
    step = EvalStep(model, graphs=False)
    snap = _snapshot(model)
    xs = [x[8 * i:8 * i + 8] for i in range(3)]
    # labels: right (class s for sample s) for every second sample
    ys = [torch.tensor([s if s % 2 == 0 else (s + 1) % 40 for s in range(8 * i, 8 * i + 8)], device=dev)
          for i in range(3)]
    mods, fus = [], []
    loader = [(torch.arange(8 * i, 8 * i + 8), x, y) for i, (x, y) in enumerate(zip(xs, ys))]
    _restore(model, snap)
    a = evaluate(model, loader, "test", BF)
    _restore(model, snap)
    b = evaluate(model, loader, "test", BF, engine=step)
    assert model.training
    assert list(a) == list(b)
    assert np.array_equal(a["test_indices"], b["test_indices"]) and a["test_indices"].dtype == b["test_indices"].dtype
    for k in a:
        if k != "test_indices":
            assert isinstance(b[k], (float, np.floating)) and isinstance(a[k], (float, np.floating)), k
    # the two paths' logits, per sample
    for x, y in zip(xs, ys):
        mods.append(_module_path(model, x, BF)[0])
        step.begin()
        fus.append([o.clone() for o in step(x, y)[0]])
    excluded, lip = set(), 0.0
    for bi, (m, f) in enumerate(zip(mods, fus)):
        bar = BAR * max(float(o.abs().max()) for o in m)
        for name, zm, zf in [("mean", torch.stack(m).mean(0), torch.stack(f).mean(0))] + \
                [(f"branch {i}", u, v) for i, (u, v) in enumerate(zip(m, f))]:
            top = zm.topk(2, dim=1).values
            close = (top[:, 0] - top[:, 1]) < bar
            excluded |= {(bi, int(i)) for i in torch.nonzero(close).flatten()}
            same = zm.argmax(1) == zf.argmax(1)
            assert bool((same | close).all()), (bi, name)
        d = max(float((u - v).abs().max()) for u, v in zip(m, f))
        assert d <= bar
        lip += sum(2 * float((u - v).abs().max(dim=1).values.sum()) for u, v in zip(m, f))
    print(f"evaluate: module {a['test_loss']:.6f} / {a['test_acc']:.3f}, fused {b['test_loss']:.6f} / "
          f"{b['test_acc']:.3f}; samples below the top-2 bar: {sorted(excluded)}; loss bound {lip / 24:.3e}")
    assert len(excluded) <= 1
    slack = 100.0 * len(excluded) / 24 + 1e-4
    for k in ("test_acc", "test_acc_modal_0", "test_acc_modal_1"):
        assert abs(a[k] - b[k]) <= slack, k
    assert 0 < b["test_acc"] < 100
    assert abs(a["test_loss"] - b["test_loss"]) <= lip / 24 + 1e-5 * abs(a["test_loss"])


def test_n_branch(dev):
    from greedy_multimodal_learning_amd.engine import EvalStep
    model = _build(dev, n_views=4, seed=5)
    x, y = _inputs(dev, 2, V=4)
    ref, _ = _module_path(model, x, torch.float32)
    mod, _ = _module_path(model, x, BF)
    step = EvalStep(model, graphs=False)
    step.begin()
    outs, _ = step(x, y)
    assert len(outs) == 4
    e_fused, e_mod = _err(outs, ref), _err(mod, ref)
    print(f"4 views: fused {e_fused:.3e}, bf16 modules {e_mod:.3e} vs fp32 (bar {BAR})")
    assert e_fused <= BAR
    assert step.result()[3] == 2 and len(step.result()[2]) == 4


def test_begin_picks_up_changed_weights(dev):
    from greedy_multimodal_learning_amd.bn import GMBatchNorm2d
    from greedy_multimodal_learning_amd.conv import GMConv2d
    from greedy_multimodal_learning_amd.engine import EvalStep
    model = _build(dev, seed=8)
    x, y = _inputs(dev, 3, seed=4)
    step = EvalStep(model, graphs=False)
    step.begin()
    old = [o.clone() for o in step(x, y)[0]]
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():  # an SGD-like step in place, and moved running statistics
        for m in model.modules():
            if isinstance(m, GMConv2d):
                m.weight.add_((0.2 * float(m.weight.std()) * torch.randn(m.weight.shape, generator=g)).to(dev))
                m.weight.copy_(m.weight.bfloat16().float())
            elif isinstance(m, GMBatchNorm2d):
                m.running_mean.add_(0.2).mul_(1.1)
                m.running_var.mul_(1.3)
                m.bias.add_(0.125)
    ref, _ = _module_path(model, x, BF)
    # without begin() the trunk still holds the old weight copies and coefficients (the stem's
    # weight, the MMTM sites and the heads are read from the modules every batch)
    stale = [o.clone() for o in step(x, y)[0]]
    step.begin()
    outs, _ = step(x, y)
    e, moved, off = _err(outs, ref), _err(old, ref), _err(stale, ref)
    print(f"after the in-place change: fused vs bf16 modules {e:.3e} (bar {BAR}); the old logits are off by "
          f"{moved:.3e}, a pass without begin() by {off:.3e}")
    assert e <= BAR < min(moved, off)


def test_fp32_keeps_the_module_forward(dev, world):
    from greedy_multimodal_learning_amd.engine import EvalStep
    model = world["model"]
    x, y = _inputs(dev, 3)
    ref, _ = _module_path(model, x, torch.float32)
    step = EvalStep(model, compute_dtype=torch.float32)
    assert not step.graphs and step.trunk is None
    step.begin()
    outs, _ = step(x.float(), y)
    assert all(torch.equal(a, b) for a, b in zip(outs, ref))
    loss, acc, accm, n = step.result()
    want = float(sum(F.cross_entropy(o.double(), y) for o in ref))
    assert n == 3 and abs(loss - want) <= 1e-5 * abs(want)
