"""The folded BatchNorm finalize (vtrunk.BN_FOLD) and the downsample blocks' residual-affine
block output (vtrunk.DS_RES_AFFINE) inside whole training steps: two BalancedStep
steps of the C2 model (B = 2, 64 x 64, bf16) from one seed with both flags on and off, eager and
under hipGraph capture, and once for MMTM_MVCNN_N on ResNet-50 with 3 views (the Bottleneck
path, three view groups).  Loss, branch logits, every parameter and every BatchNorm buffer must
be torch.equal: the fold changes launches, not a single bit.  At this batch every BatchNorm that
takes its statistics from a convolution epilogue has few partial rows, so the rule folds most
of them (asserted: the folded entry point ran and the rule took some shape)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(fold, graphs, kind, monkeypatch):
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import vtrunk
    from greedy_multimodal_learning_amd.callbacks import Bias_Mitigation_Strong
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN, MMTM_MVCNN_N
    dev = torch.device("cuda:0")
    monkeypatch.setattr(vtrunk, "BN_FOLD", fold)
    monkeypatch.setattr(vtrunk, "DS_RES_AFFINE", fold)
    torch.manual_seed(0)
    if kind == "C2":
        m, V = MMTM_MVCNN().to(dev), 2
        bn, mn = ["net_view_0", "net_view_1"], ["visual", "skeleton"]
    else:
        m, V = MMTM_MVCNN_N(num_views=3, trunk="resnet50").to(dev), 3
        bn, mn = m.branch_names(), m.mmtm_names()
    gate = Bias_Mitigation_Strong(epsilon=0.01, curation_windowsize=5, branchnames=bn, starting_epoch=1,
                                  MMTMnames=mn)
    st = BalancedStep(m, lr=0.05, gate=gate, graphs=graphs, branchnames=bn, MMTMnames=mn)
    st.on_epoch_begin(1)
    g = torch.Generator(device=dev).manual_seed(5)
    xs = [torch.randn(2, V, 3, 64, 64, device=dev, generator=g) for _ in range(2)]
    ys = [torch.randint(0, 40, (2,), device=dev, generator=g) for _ in range(2)]
    lib = L.load()
    folded = []
    real = lib.gm_bn_fwd_finalize_apply_grouped_bf16

    def spy(arr, G, part, rows, stream):
        import ctypes
        p = ctypes.cast(arr, ctypes.POINTER(L.BnFwd))[0]
        folded.append(lib.gm_bn_fold_blocks(p.M, p.C, rows, G))
        return real(arr, G, part, rows, stream)
    monkeypatch.setattr(lib, "gm_bn_fwd_finalize_apply_grouped_bf16", spy)
    affine = []
    real_ra = lib.gm_bn_fwd_finalize_apply_res_affine_grouped_bf16
    monkeypatch.setattr(lib, "gm_bn_fwd_finalize_apply_res_affine_grouped_bf16",
                        lambda *a: affine.append(1) or real_ra(*a))
    losses, logits = [], []
    for x, y in zip(xs, ys):
        losses.append(st(x, y).detach().clone())
        logits.append([o.detach().clone() for o in st.last_outs])
    torch.cuda.synchronize()
    assert st.graphs == graphs, "a capture failed and the engine fell back to eager steps"
    assert bool(folded) == fold, "the folded entry point is used exactly when BN_FOLD is set"
    assert bool(affine) == fold, "the downsample blocks use the residual-affine form exactly when DS_RES_AFFINE is set"
    assert not fold or any(n > 0 for n in folded), "the rule folded no BatchNorm of this model"
    return losses, logits, {k: v.detach().clone() for k, v in m.state_dict().items()}


def _equal(a, b):
    (la, oa, sa), (lb, ob, sb) = a, b
    for i, (u, v) in enumerate(zip(la, lb)):
        assert torch.equal(u, v), f"loss of step {i}"
    for i, (us, vs) in enumerate(zip(oa, ob)):
        for j, (u, v) in enumerate(zip(us, vs)):
            assert torch.equal(u, v), f"logits of branch {j}, step {i}"
    assert sa.keys() == sb.keys()
    for k in sa:  # every parameter and every BatchNorm buffer (running statistics, counters)
        assert torch.equal(sa[k].view(torch.int16) if sa[k].dtype == torch.bfloat16 else sa[k],
                           sb[k].view(torch.int16) if sb[k].dtype == torch.bfloat16 else sb[k]), k


def test_c2_steps_fold_on_equals_off(monkeypatch):
    _equal(_run(True, False, "C2", monkeypatch), _run(False, False, "C2", monkeypatch))


def test_c2_graph_steps_equal_eager_with_fold(monkeypatch):
    _equal(_run(True, True, "C2", monkeypatch), _run(True, False, "C2", monkeypatch))


def test_resnet50_three_views_fold_on_equals_off(monkeypatch):
    _equal(_run(True, False, "R50", monkeypatch), _run(False, False, "R50", monkeypatch))
