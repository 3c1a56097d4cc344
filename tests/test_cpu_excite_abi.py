"""The chained-GEMM entry points of the C ABI (gm_gemm_f32_chain, gm_mmtm_excite_fwd / _bwd,
gm_gemm_chain_sync_bytes): declared, exported, bound, and their argument checks run before
any launch, so they are testable without a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_gemm_chain_sync_bytes", "gm_gemm_f32_chain", "gm_mmtm_excite_fwd", "gm_mmtm_excite_bwd")


def _lib():
    from greedy_multimodal_learning_amd import build, _lib as L
    build.build()
    return L, L.load()


def _problems(L, n, act):
    """n well-formed gm_gemm problems; the pointers are never dereferenced on the host."""
    op = L.Operand(0x1000, 8, 1)
    none = L.Operand(0, 0, 0)
    items = [L.Gemm(4, 8, (L.c_int * 2)(8, 0), (L.Operand * 2)(op, none), (L.Operand * 2)(op, none), 0, 0, 0,
                    0x2000, 8, act, 0) for _ in range(n)]
    return L.arr(L.Gemm, items)


def test_chain_entry_points_declared_and_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "greedymml.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.EXPORTS, name
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name), name
    assert "#define GM_FAULT_CHAIN_SPIN  4u" in hdr
    assert L.GM_FAULT_CHAIN_SPIN == 4
    assert L.ABI_VERSION == 5 and lib.gm_abi_version() == 5  # (the chain: since 4; 5 removed gm_conv_set_pipe)
    n = lib.gm_gemm_chain_sync_bytes()
    assert n >= 8 and n % 16 == 0


def test_excite_fwd_argument_errors_before_any_launch():
    L, lib = _lib()
    sync = 0x3000  # never touched: every call below fails its checks first
    rc = lib.gm_mmtm_excite_fwd(None, 0, None, 0, None, None, None, 0, sync, None)
    assert rc == -1 and b"1..6" in lib.gm_last_error()
    ok1, ok2 = _problems(L, 1, 1), _problems(L, 2, 2)
    rc = lib.gm_mmtm_excite_fwd(_problems(L, 7, 1), 7, ok2, 2, None, None, None, 0, sync, None)
    assert rc == -1 and b"1..6" in lib.gm_last_error()
    rc = lib.gm_mmtm_excite_fwd(ok1, 1, _problems(L, 7, 2), 7, None, None, None, 0, sync, None)
    assert rc == -1 and b"1..6" in lib.gm_last_error()
    rc = lib.gm_mmtm_excite_fwd(ok1, 1, ok2, 2, None, None, None, 0, None, None)
    assert rc == -1 and b"sync" in lib.gm_last_error()
    # fc1 must end in relu, fc2 in sigmoid
    rc = lib.gm_mmtm_excite_fwd(_problems(L, 1, 0), 1, ok2, 2, None, None, None, 0, sync, None)
    assert rc == -1 and b"relu" in lib.gm_last_error()
    rc = lib.gm_mmtm_excite_fwd(ok1, 1, _problems(L, 2, 1), 2, None, None, None, 0, sync, None)
    assert rc == -1 and b"sigmoid" in lib.gm_last_error()
    # gm_gemm_f32's own per-problem checks
    bad = _problems(L, 1, 1)
    bad[0].ld_c = 4  # < N
    rc = lib.gm_mmtm_excite_fwd(bad, 1, ok2, 2, None, None, None, 0, sync, None)
    assert rc == -1 and b"ld_c" in lib.gm_last_error()
    # a running average needs its second row and the step counter
    rc = lib.gm_mmtm_excite_fwd(ok1, 1, ok2, 2, 0x4000, None, None, 1, sync, None)
    assert rc == -1 and b"running average" in lib.gm_last_error()


def test_chain_and_bwd_argument_errors_before_any_launch():
    L, lib = _lib()
    ok = _problems(L, 2, 0)
    for fn in (lib.gm_gemm_f32_chain, lib.gm_mmtm_excite_bwd):
        assert fn(None, 0, ok, 2, 0x3000, None) == -1 and b"1..6" in lib.gm_last_error()
        assert fn(ok, 2, _problems(L, 7, 0), 7, 0x3000, None) == -1 and b"1..6" in lib.gm_last_error()
        assert fn(ok, 2, ok, 2, None, None) == -1 and b"sync" in lib.gm_last_error()
        bad = _problems(L, 2, 0)
        bad[1].act = 3
        assert fn(ok, 2, bad, 2, 0x3000, None) == -1 and b"act" in lib.gm_last_error()


def test_excite_form_switch_is_public_and_defaults_to_chain():
    import pytest
    import torch
    from greedy_multimodal_learning_amd.balanced_mmtm import MMTM_mitigate
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    assert MMTM_mitigate(8, 8, 4).excite_form == "chain"
    m = MMTM_MVCNN()
    sites = [s for s in m.modules() if isinstance(s, MMTM_mitigate)]
    assert sites
    BalancedStep(m, lr=0.05, compute_dtype=torch.float32, channels_last=False)
    assert all(s.excite_form == "chain" for s in sites)
    BalancedStep(m, lr=0.05, compute_dtype=torch.float32, channels_last=False, mmtm_excite="fused")
    assert all(s.excite_form == "fused" for s in sites)
    with pytest.raises(ValueError):
        BalancedStep(m, lr=0.05, compute_dtype=torch.float32, channels_last=False, mmtm_excite="both")
