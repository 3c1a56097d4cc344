"""The evaluation-pass entries (gm_bn_infer_coef, gm_conv2d_fwd_grouped_affine_bf16 /
gm_conv2d_fwd_affine_ok, gm_eval_metrics): declared, exported and bound, additive to ABI 5;
their arguments are checked before any launch, so that is testable without a GPU; and
gm_conv2d_fwd_affine_ok follows the planner's kernel choice - through the planner's own
switches too - on a small table of descriptors."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_bn_infer_coef", "gm_conv2d_fwd_affine_ok", "gm_conv2d_fwd_grouped_affine_bf16", "gm_eval_metrics")
GM_E_ARG, GM_E_UNSUP = -1, -3


def _sq(N, H, W, C, K, R, st):
    return (N, H, W, C, K, R, R, st, st, R // 2, R // 2)


def _lib():
    from greedy_multimodal_learning_amd import build, _lib as L
    build.build()
    return L, L.load()


def test_eval_entry_points_declared_and_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "greedymml.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.EXPORTS, name
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name), name
    assert re.search(r"\}\s*gm_bn_coef_entry\s*;", code)


def test_coef_entry_layout_matches_header(tmp_path):
    """The ctypes mirror of gm_bn_coef_entry has the C compiler's size and field offsets."""
    import shutil
    import subprocess
    from greedy_multimodal_learning_amd import _lib as L
    assert ctypes.sizeof(L.BnCoefEntry) == 5 * 8 + 8   # five pointers, an int, a float
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "greedymml.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(gm_bn_coef_entry));']
    for f, _ in L.BnCoefEntry._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(gm_bn_coef_entry, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.BnCoefEntry)
    for f, _ in L.BnCoefEntry._fields_:
        assert int(got[f]) == getattr(L.BnCoefEntry, f).offset, f


def test_abi_version_stays_5():
    L, lib = _lib()
    assert lib.gm_abi_version() == 5 == L.ABI_VERSION
    assert "#define GM_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "greedymml.h")).read()


def _affine(lib, d, G=2, x=0x1000, w=0x2000, w_stride=1 << 24, y=0x3000, coef=0x4000, coef_stride=1 << 12,
            residual=0, relu=1):
    return lib.gm_conv2d_fwd_grouped_affine_bf16(ctypes.byref(d) if d is not None else None, G, x, w, w_stride, y,
                                                 coef, coef_stride, residual, relu, None, 0, None)


def test_affine_arguments_are_checked_before_any_launch():
    L, lib = _lib()
    good = L.ConvDescHW(*_sq(2, 14, 14, 128, 128, 3, 1))
    assert _affine(lib, None) == GM_E_ARG
    assert b"descriptor" in lib.gm_last_error()
    for bad in (_sq(0, 14, 14, 128, 128, 3, 1), _sq(2, 14, 14, 96, 128, 3, 1), _sq(2, 14, 14, 128, 132, 3, 1),
                (2, 14, 14, 128, 128, 3, 3, 0, 1, 1, 1), (2, 1, 1, 128, 128, 3, 3, 1, 1, 0, 0)):
        assert _affine(lib, L.ConvDescHW(*bad)) == GM_E_ARG, bad
        assert lib.gm_last_error().startswith(b"conv:"), bad
    for kw, word in ((dict(x=0), b"x"), (dict(w=0), b"w"), (dict(y=0), b"y"), (dict(coef=0), b"coef"),
                     (dict(coef=0x4004), b"coef"), (dict(coef_stride=6), b"coef_stride"),
                     (dict(coef_stride=128), b"coef_stride"), (dict(residual=0x5008), b"residual"),
                     (dict(G=0), b"view groups"), (dict(G=65), b"view groups"), (dict(w_stride=8), b"weight stride")):
        assert _affine(lib, good, **kw) == GM_E_ARG, kw
        assert word in lib.gm_last_error(), (kw, lib.gm_last_error())
    # a declined shape: GM_E_UNSUP with the reason, nothing launched (there is no device here)
    assert _affine(lib, L.ConvDescHW(*_sq(4, 28, 28, 64, 128, 1, 2))) == GM_E_UNSUP
    assert b"k_gemm_ring" in lib.gm_last_error()
    assert lib.gm_conv2d_fwd_affine_ok(None, 2) == 0
    assert lib.gm_conv2d_fwd_affine_ok(ctypes.byref(good), 0) == 0
    assert lib.gm_conv2d_fwd_affine_ok(ctypes.byref(good), 65) == 0


def test_coef_table_and_metrics_arguments_are_checked():
    L, lib = _lib()
    assert lib.gm_bn_infer_coef(None, 1, 64, None) == GM_E_ARG and b"table" in lib.gm_last_error()
    assert lib.gm_bn_infer_coef(0x1000, 0, 64, None) == GM_E_ARG and b"n must" in lib.gm_last_error()
    assert lib.gm_bn_infer_coef(0x1000, 70000, 64, None) == GM_E_ARG and b"n must" in lib.gm_last_error()
    assert lib.gm_bn_infer_coef(0x1000, 2, 0, None) == GM_E_ARG and b"max_c" in lib.gm_last_error()
    m = lib.gm_eval_metrics
    assert m(None, 2, 3, 40, 0x2000, 0x3000, None) == GM_E_ARG and b"logits" in lib.gm_last_error()
    assert m(0x1000, 2, 3, 40, None, 0x3000, None) == GM_E_ARG and b"labels" in lib.gm_last_error()
    assert m(0x1000, 2, 3, 40, 0x2000, None, None) == GM_E_ARG and b"acc" in lib.gm_last_error()
    assert m(0x1000, 2, 3, 40, 0x2000, 0x3004, None) == GM_E_ARG and b"acc" in lib.gm_last_error()
    assert m(0x1000, 0, 3, 40, 0x2000, 0x3000, None) == GM_E_ARG and b"nbranch" in lib.gm_last_error()
    assert m(0x1000, 9, 3, 40, 0x2000, 0x3000, None) == GM_E_ARG and b"nbranch" in lib.gm_last_error()
    assert m(0x1000, 2, 0, 40, 0x2000, 0x3000, None) == GM_E_ARG and b"B, N" in lib.gm_last_error()
    assert m(0x1000, 2, 3, 0, 0x2000, 0x3000, None) == GM_E_ARG and b"B, N" in lib.gm_last_error()


# descriptor, G, the kernel the planner picks under the default switches, taken?
TABLE = [
    ("layer-1", _sq(3, 56, 56, 64, 64, 3, 1), 2, "k_conv_rw", 1),
    ("h9", _sq(2, 14, 14, 128, 128, 3, 1), 2, "k_conv_h9", 1),
    ("strided", _sq(3, 20, 20, 64, 128, 3, 2), 2, "k_conv_igemm_ut", 1),
    ("split-K", _sq(8, 7, 7, 512, 512, 3, 1), 2, "k_conv_h9 (split)", 1),
    ("1x1/s2", _sq(4, 28, 28, 64, 128, 1, 2), 2, "k_gemm_ring", 0),
    ("1x1/s1", _sq(4, 28, 28, 256, 64, 1, 1), 2, "k_gemm_ring", 0),
    ("narrow input, one group", _sq(2, 16, 16, 32, 64, 3, 1), 1, "k_conv_igemm", 0),
    ("pixel-pair stem", (2, 69, 35, 8, 64, 7, 4, 2, 1, 0, 0), 2, "k_conv_stem", 0),
]


@pytest.mark.parametrize("name,shape,G,kernel,want", TABLE, ids=[t[0] for t in TABLE])
def test_affine_ok_follows_the_plan(name, shape, G, kernel, want):
    L, lib = _lib()
    d = L.ConvDescHW(*shape)
    assert lib.gm_conv2d_fwd_affine_ok(ctypes.byref(d), G) == want, (name, kernel, lib.gm_last_error())
    if not want:  # the call itself declines the same shapes, saying why
        assert _affine(lib, d, G=G) == GM_E_UNSUP, name
        assert lib.gm_last_error(), name


def test_affine_ok_follows_the_switches():
    """One group of a 128-channel 3x3: k_conv_h9 takes it; with gm_conv_set_h9(0) the planner hands it
    to k_conv_halo, which has no affine form; with the halo kernels off too it is the lean kernel's."""
    L, lib = _lib()
    d = L.ConvDescHW(*_sq(2, 14, 14, 128, 128, 3, 1))
    try:
        assert lib.gm_conv2d_fwd_affine_ok(ctypes.byref(d), 1) == 1
        L.check(lib.gm_conv_set_h9(0), "h9")
        assert lib.gm_conv2d_fwd_affine_ok(ctypes.byref(d), 1) == 0
        assert b"k_conv_halo" in lib.gm_last_error()
        assert lib.gm_conv2d_fwd_affine_ok(ctypes.byref(d), 2) == 1  # view groups: the lean kernel
        L.check(lib.gm_conv_set_halo(0), "halo")
        assert lib.gm_conv2d_fwd_affine_ok(ctypes.byref(d), 1) == 1
    finally:
        L.check(lib.gm_conv_set_h9(1), "h9")
        L.check(lib.gm_conv_set_halo(1), "halo")
