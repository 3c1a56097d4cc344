"""The split-bf16 fp32 convolution entries (gm_conv2d_f32_split / _split_scratch): declared,
exported and bound; `terms` is checked before any launch, so it is testable without a GPU;
the planner is the exact kernel's, so the scratch sizes agree; and the mode reaches every
GMConv2d through BalancedStep(f32_contraction=...)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_conv2d_f32_split_scratch", "gm_conv2d_f32_split")

DESCS = [  # mode, (N, H, W, C, K, R, S, stride, pad)
    (0, (2, 64, 64, 3, 64, 7, 7, 2, 3)),
    (0, (2, 16, 16, 64, 64, 3, 3, 1, 1)),
    (1, (2, 16, 16, 64, 128, 3, 3, 2, 1)),
    (2, (16, 56, 56, 64, 64, 3, 3, 1, 1)),    # long reduction: the plan splits
    (2, (4, 2, 2, 512, 512, 3, 3, 1, 1)),
    (0, (4, 2, 2, 512, 512, 3, 3, 1, 1)),     # small M: forward splits
    (1, (2, 7, 5, 6, 12, 3, 3, 1, 1)),
]


def _lib():
    from greedy_multimodal_learning_amd import build, _lib as L
    build.build()
    return L, L.load()


def _desc(L, mode, shape):
    # the pointers are never dereferenced on the host
    return L.ConvF32(mode, L.ConvDesc(*shape), 0x1000, 0x2000, 0x3000, 0x4000, 0, 0, 0)


def test_split_entry_points_declared_and_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "greedymml.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.EXPORTS, name
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name), name


def test_terms_is_checked_before_any_launch():
    L, lib = _lib()
    assert lib.gm_conv2d_f32_split(None, 3, None, 0, None) == -1
    assert b"null descriptor" in lib.gm_last_error() and b"terms" in lib.gm_last_error()
    p = _desc(L, *DESCS[1])
    for terms in (0, 1, 2, 4, 9):
        assert lib.gm_conv2d_f32_split(ctypes.byref(p), terms, None, 0, None) == -1, terms
        assert b"terms" in lib.gm_last_error(), terms
        assert lib.gm_conv2d_f32_split_scratch(ctypes.byref(p), terms) == 0
        assert b"terms" in lib.gm_last_error(), terms
    # a null descriptor with a bad term count names terms too (it is the first check)
    assert lib.gm_conv2d_f32_split(None, 4, None, 0, None) == -1
    assert b"terms" in lib.gm_last_error()


def test_split_scratch_equals_exact_scratch():
    L, lib = _lib()
    nonzero = 0
    for mode, shape in DESCS:
        p = _desc(L, mode, shape)
        want = lib.gm_conv2d_f32_scratch(ctypes.byref(p))
        nonzero += want > 0
        for terms in (3, 6):
            assert lib.gm_conv2d_f32_split_scratch(ctypes.byref(p), terms) == want, (mode, shape, terms)
    assert nonzero >= 2  # the list does exercise split plans


def test_conv_f32_rejects_other_term_counts():
    import torch
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import conv as G
    _lib()
    out = torch.empty(1)
    with pytest.raises(ValueError, match="terms"):
        G.conv_f32(L.GM_CONV_FWD, G._desc(1, 4, 4, 4, 4, 1, 1, 1, 0), x=out, w=out, out=out, terms=4)
    assert G.f32_terms_of(None) == 0 and G.f32_terms_of("exact") == 0
    assert G.f32_terms_of("bf16x3") == 3 and G.f32_terms_of("bf16x6") == 6


def test_balanced_step_f32_contraction():
    import torch
    from greedy_multimodal_learning_amd.conv import GMConv2d
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    assert GMConv2d.f32_terms == 0
    m = MMTM_MVCNN()
    convs = [c for c in m.modules() if isinstance(c, GMConv2d)]
    assert len(convs) >= 40  # two ResNet-18 trunks
    kw = dict(lr=0.05, channels_last=False)
    BalancedStep(m, compute_dtype=torch.float32, **kw)
    assert all(c.f32_terms == 0 for c in convs)
    BalancedStep(m, compute_dtype=torch.float32, f32_contraction=None, **kw)
    assert all(c.f32_terms == 0 for c in convs)
    st = BalancedStep(m, compute_dtype=torch.float32, f32_contraction="bf16x6", **kw)
    assert st.f32_contraction == "bf16x6" and all(c.f32_terms == 6 for c in convs)
    BalancedStep(m, compute_dtype=torch.float32, f32_contraction="bf16x3", **kw)
    assert all(c.f32_terms == 3 for c in convs)
    BalancedStep(m, compute_dtype=torch.float32, f32_contraction="exact", **kw)
    assert all(c.f32_terms == 0 for c in convs)
    with pytest.raises(ValueError, match="f32_contraction"):
        BalancedStep(m, compute_dtype=torch.bfloat16, f32_contraction="bf16x3", **kw)
    with pytest.raises(ValueError, match="f32_contraction"):
        BalancedStep(m, compute_dtype=torch.bfloat16, f32_contraction="exact", **kw)
    with pytest.raises(ValueError, match="f32_contraction"):
        BalancedStep(m, compute_dtype=torch.float32, f32_contraction="bf16x4", **kw)
    with pytest.raises(ValueError, match="f32_contraction"):
        BalancedStep(m, compute_dtype=torch.float32, f32_contraction=6, **kw)
    assert all(c.f32_terms == 0 for c in convs)  # a refused mode changes nothing


def test_gin_key_default_keeps_a_bf16_run_valid():
    import torch
    from greedy_multimodal_learning_amd.train import f32_contraction_arg
    assert f32_contraction_arg(torch.bfloat16, "exact") is None
    assert f32_contraction_arg(torch.float32, "exact") == "exact"
    assert f32_contraction_arg(torch.bfloat16, "bf16x3") == "bf16x3"  # the engine refuses it
    assert f32_contraction_arg(torch.float32, "bf16x6") == "bf16x6"
