"""engine.EvalStep(compute_dtype=torch.float32, f32_trunk="fused"): the fp32 evaluation pass with
every BatchNorm, residual add and ReLU in its convolution's epilogue (vtrunk.EvalTrunkF32 on
gm_conv2d_f32_affine), against the fp32 module forward in eval mode.

The epilogue applies gm_bn_fwd_infer_f32's arithmetic to the convolution's own accumulator and
the sites and heads are called as the module forward calls them, so the bar everywhere is
torch.equal: logits, squeezed maps, the sites' running averages and step counters.

Model recipe of test_gpu_eval_step.py: 64 x 64 inputs, deterministic weights, every BatchNorm
with randomised running statistics, gamma (both signs) and beta; the MMTM sites advance their
state on every forward, so each comparison starts both paths from the same saved site state."""
import numpy as np
import pytest
import torch

from oracle import weights

pytestmark = pytest.mark.gpu

F32 = torch.float32
H = 64
MODES = ["exact", "bf16x3", "bf16x6"]


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
                m.weight.copy_((0.5 + torch.rand(C, generator=g)) * sign)
                m.bias.copy_(0.3 * torch.randn(C, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(C, generator=g))
                m.running_var.copy_(0.5 * 4 ** torch.rand(C, generator=g))   # [0.5, 2]
                m.num_batches_tracked.fill_(17)


def _build(dev, n_views=2, trunk="resnet18", seed=3, n_model=False, **kw):
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN, MMTM_MVCNN_N
    m = MMTM_MVCNN_N(num_views=n_views, trunk=trunk, **kw) if n_model else MMTM_MVCNN(**kw)
    weights.apply_to_module(m, seed=seed)
    _randomise_bn(m, seed + 1)
    return m.to(dev)


def _inputs(dev, B, V=2, seed=0):
    g = torch.Generator().manual_seed(2000 + 10 * B + seed)
    x = torch.randn(B, V, 3, H, H, generator=g).to(dev)
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


def _same_state(a, b):
    return all(na == nb and all(torch.equal(u, v) for u, v in zip(ta, tb)) for (ta, na), (tb, nb) in zip(a, b))


def _module_path(model, x, curation=(False, None)):
    """The fp32 module forward in eval mode, as train.evaluate runs it; (logits, squeezed)."""
    model.eval()
    try:
        with torch.no_grad():
            _, outs, _, sq = model(x, curation_mode=curation[0], caring_modality=curation[1])
    finally:
        model.train(True)
    return [o.float() for o in outs], sq


def _equal(outs, ref):
    return len(outs) == len(ref) and all(
        bool(torch.isfinite(r).all()) and o.dtype == F32 and torch.equal(o, r) for o, r in zip(outs, ref))


def _fused(model, **kw):
    from greedy_multimodal_learning_amd.engine import EvalStep
    return EvalStep(model, F32, f32_trunk="fused", **kw)


@pytest.fixture(scope="module")
def world(dev):
    """The model, a warmed site state (non-zero running averages) and an eager fused fp32 step."""
    torch.manual_seed(0)
    model = _build(dev)
    _module_path(model, _inputs(dev, 4, seed=9)[0])   # the sites' averages leave zero
    return dict(model=model, snap=_snapshot(model), step=_fused(model, graphs=False))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [3, 8])
def test_logits_equal_the_module_path(dev, world, B, mode):
    from greedy_multimodal_learning_amd.conv import GMConv2d, set_f32_contraction
    model, snap = world["model"], world["snap"]
    x, y = _inputs(dev, B)
    try:
        terms = set_f32_contraction(model, mode, F32)
        _restore(model, snap)
        ref, _ = _module_path(model, x)
        after_ref = _snapshot(model)
        _restore(model, snap)
        step = _fused(model, graphs=False)
        assert step.trunk is not None and not step.graphs
        step.begin()
        assert {p.terms for p in step.trunk.pos} == {terms}
        outs, sq = step(x, y)
        assert sq is None and len(outs) == 2 and all(o.shape == (B, 40) for o in outs)
        assert _equal(outs, ref)
        assert _same_state(_snapshot(model), after_ref)
        assert step.result()[3] == B
    finally:
        set_f32_contraction(model, "exact", F32)
        assert all(c.f32_terms == 0 for c in model.modules() if isinstance(c, GMConv2d))


@pytest.mark.parametrize("mode", ["squeeze", "curation0", "curation1", "mmtm_off"])
def test_modes_equal_the_module_path(dev, world, mode):
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
        ref, sq_ref = _module_path(model, x, curation)
        after_ref = _snapshot(model)
        _restore(model, snap)
        step.begin()
        outs, sq = step(x, y, curation)
        assert _equal(outs, ref)
        assert _same_state(_snapshot(model), after_ref)
        assert all(n == n0 + 1 for (_, n), (_, n0) in zip(after_ref, snap))
        if mode == "squeeze":
            assert len(sq) == len(sq_ref) == 3
            for a, b in zip(sq, sq_ref):
                assert len(a) == len(b) == 2
                assert all(u.is_cuda and u.dtype == v.dtype and torch.equal(u.cpu(), v) for u, v in zip(a, b))
        else:
            assert sq is None and all(s is None for s in sq_ref)
    finally:
        model.mmtm_off = False
        model.saving_mmtm_squeeze_array = False
        if hasattr(model, "mmtm_rescale"):
            del model.mmtm_rescale


@pytest.mark.parametrize("trunk,V", [("resnet18", 4), ("resnet50", 2)])
def test_n_view_models(dev, trunk, V):
    """MMTM_MVCNN_N: four BasicBlock views; two Bottleneck views (1x1 convolutions, conv3 + bn3 +
    residual + ReLU)."""
    model = _build(dev, n_views=V, trunk=trunk, seed=5, n_model=True)
    x, y = _inputs(dev, 2, V=V)
    snap = _snapshot(model)
    ref, _ = _module_path(model, x)
    after_ref = _snapshot(model)
    _restore(model, snap)
    step = _fused(model, graphs=False)
    step.begin()
    outs, _ = step(x, y)
    assert len(outs) == V and _equal(outs, ref)
    assert _same_state(_snapshot(model), after_ref)
    assert step.result()[3] == 2 and len(step.result()[2]) == V


def test_graph_replay_equals_eager(dev, world):
    """Four batches of one shape.  The shape's first batch runs eagerly, the second is captured and
    launched, the third and fourth replay the captured graph: EvalStep.replays counts every graph
    launch (the capturing batch's too, as test_gpu_eval_step.py pins for the bf16 form), so it is 1
    after the second batch and two replays of the existing graph later it is 3.  Then a second pass:
    begin() again (the trunk's weight and coefficient buffers are rewritten in place, so the graph
    stays valid and two more batches replay it), and a pass under another contraction mode, which
    must not replay the first mode's graph."""
    from greedy_multimodal_learning_amd.conv import set_f32_contraction
    model, snap = world["model"], world["snap"]
    batches = [_inputs(dev, 4, seed=s) for s in (1, 2, 3, 4)]
    res = {}
    for graphs in (False, True):
        _restore(model, snap)
        step = _fused(model, graphs=graphs)
        step.begin()
        got, counts = [], []
        for x, y in batches:
            outs, sq = step(x, y)
            got.append([o.clone() for o in outs])
            counts.append(step.replays)
        acc = step.acc.clone()
        if graphs:
            assert step.capture_failures == [] and step.graphs
            assert counts[:2] == [0, 1]
            assert step.replays - counts[1] == 2
        else:
            assert counts == [0, 0, 0, 0]
        torch.empty(1 << 24, device=dev).fill_(float("nan"))  # freed memory does not keep old weights
        step.begin()
        for x, y in batches[:2]:
            got.append([o.clone() for o in step(x, y)[0]])
        if graphs:
            assert step.replays == 5 and step.capture_failures == []
        try:
            set_f32_contraction(model, "bf16x3", F32)
            step.begin()
            for x, y in batches[:2]:
                got.append([o.clone() for o in step(x, y)[0]])
        finally:
            set_f32_contraction(model, "exact", F32)
        if graphs:
            assert step.replays == 6 and step.capture_failures == []  # eager, then its own capture
        assert not _equal(got[-1], got[-3])  # (the other contraction does give other bits)
        res[graphs] = (got, acc, _snapshot(model))
    (ge, ae, se), (gg, ag, sg) = res[False], res[True]
    assert torch.equal(ae, ag)
    for oe, og in zip(ge, gg):
        assert _equal(og, oe)
    assert _same_state(se, sg)


def test_begin_picks_up_state_changes(dev):
    from greedy_multimodal_learning_amd.bn import GMBatchNorm2d
    from greedy_multimodal_learning_amd.conv import GMConv2d
    model = _build(dev, seed=8)
    x, y = _inputs(dev, 3, seed=4)
    snap = _snapshot(model)
    step = _fused(model, graphs=False)
    step.begin()
    old = [o.clone() for o in step(x, y)[0]]
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():  # an SGD-like step in place, and moved running statistics
        for m in model.modules():
            if isinstance(m, GMConv2d):
                m.weight.add_((0.2 * float(m.weight.std()) * torch.randn(m.weight.shape, generator=g)).to(dev))
            elif isinstance(m, GMBatchNorm2d):
                m.running_var.mul_(1.3)
    _restore(model, snap)
    ref, _ = _module_path(model, x)
    # without begin() the trunk still holds the old coefficients
    _restore(model, snap)
    stale = [o.clone() for o in step(x, y)[0]]
    _restore(model, snap)
    step.begin()
    outs, _ = step(x, y)
    assert not _equal(old, ref) and not _equal(stale, ref)
    assert _equal(outs, ref)


def test_evaluate_equals_the_module_loop(dev, world):
    """train.evaluate(engine=the fused fp32 step) against train.evaluate(engine=None): three
    batches, the last one smaller.  The loss is the fp64 device sum against the host's float
    sum: 1e-6 relative."""
    from greedy_multimodal_learning_amd.train import evaluate
    model, step, snap = world["model"], world["step"], world["snap"]
    sizes = (4, 4, 3)
    loader, at = [], 0
    for i, b in enumerate(sizes):
        x, y = _inputs(dev, b, seed=20 + i)
        loader.append((torch.arange(at, at + b), x, y))
        at += b
    _restore(model, snap)
    a = evaluate(model, loader, "test", F32)
    _restore(model, snap)
    b = evaluate(model, loader, "test", F32, engine=step)
    assert model.training
    assert list(a) == list(b)
    assert np.array_equal(a["test_indices"], b["test_indices"]) and a["test_indices"].dtype == b["test_indices"].dtype
    n = sum(sizes)
    for k in ("test_acc", "test_acc_modal_0", "test_acc_modal_1"):
        # the same correct counts (the host loop carries its percentages in fp32: 1e-4 of a percent)
        assert round(float(a[k]) * n / 100) == round(float(b[k]) * n / 100), k
        assert abs(float(a[k]) - float(b[k])) <= 1e-4, k
    assert abs(a["test_loss"] - b["test_loss"]) <= 1e-6 * abs(a["test_loss"])


def test_argument_errors(dev, world):
    from greedy_multimodal_learning_amd.engine import EvalStep
    from greedy_multimodal_learning_amd.train import eval_engine_arg
    model = world["model"]
    with pytest.raises(ValueError, match="f32_trunk"):
        EvalStep(model, torch.bfloat16, f32_trunk="fused")
    with pytest.raises(ValueError, match="f32_trunk"):
        EvalStep(model, F32, f32_trunk="stacked")
    with pytest.raises(ValueError, match="f32_trunk"):
        eval_engine_arg(model, F32, "modules", f32_trunk="fused")
    with pytest.raises(ValueError, match="f32_trunk"):
        eval_engine_arg(model, torch.bfloat16, "fused", f32_trunk="fused")
    assert eval_engine_arg(model, F32, "modules") is None
    step = eval_engine_arg(model, F32, "fused", f32_trunk="fused")
    assert step.fused_f32 and step.trunk is not None and step.graphs
    plain = eval_engine_arg(model, F32, "fused")
    assert plain.trunk is None and not plain.graphs and not plain.fused_f32
