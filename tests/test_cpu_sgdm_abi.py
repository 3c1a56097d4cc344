"""gm_group_sumsq_sgdm (the norms pass with torch.optim.SGD's momentum and weight decay) on the
C ABI and the opt-in that reaches it from the training entry: declared, exported, bound; its
argument checks run before any launch, so they are testable without a GPU."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gm_group_sumsq_sgdm"


def _lib():
    from greedy_multimodal_learning_amd import build, _lib as L
    build.build()
    return L, L.load()


def test_sgdm_entry_point_declared_and_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "greedymml.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, code)
    assert NAME in L.EXPORTS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), NAME)
    assert len(L.EXPORTS[NAME][1]) == 15
    assert ctypes.sizeof(L.Tensor) == 40  # the table keeps its layout: the buffers are a parallel array


def test_sgdm_argument_errors_before_any_launch():
    L, lib = _lib()
    # well-formed arguments; the pointers are never dereferenced on the host and every call below
    # fails its checks before a launch
    tab, mom, out, scratch, gate = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    nbytes = lib.gm_group_sumsq_scratch(100)

    def call(table=tab, mom=mom, ngroups=4, mu=0.9, wd=5e-4, gate=None, gate_n=0):
        rc = lib.gm_group_sumsq_sgdm(table, mom, 1, 100, ngroups, 1.0, 0.1, mu, wd, out, scratch, nbytes, gate,
                                     gate_n, None)
        return rc, lib.gm_last_error()

    rc, msg = call(table=None)
    assert rc == -1 and b"empty" in msg
    rc, msg = call(mu=-0.1)
    assert rc == -1 and b"momentum" in msg
    rc, msg = call(mu=float("nan"))
    assert rc == -1 and b"momentum" in msg
    rc, msg = call(mu=float("inf"))
    assert rc == -1 and b"momentum" in msg
    rc, msg = call(wd=-1e-4)
    assert rc == -1 and b"weight_decay" in msg
    rc, msg = call(wd=float("nan"))
    assert rc == -1 and b"weight_decay" in msg
    rc, msg = call(mom=None)  # momentum 0.9 without buffers
    assert rc == -1 and b"buffers" in msg
    rc, msg = call(mu=0.0)  # buffers without a momentum
    assert rc == -1 and b"buffers" in msg
    # a gate whose state type does not match the group count (gm_group_sumsq_gate's rule)
    rc, msg = call(ngroups=8, gate=gate, gate_n=0)
    assert rc == -1 and b"two-branch" in msg
    rc, msg = call(ngroups=5, gate=gate, gate_n=1)
    assert rc == -1 and b"N-branch" in msg
    rc, msg = call(ngroups=33)
    assert rc == -1 and b"ngroups" in msg


def test_group_norms_and_engine_take_the_hyper_parameters():
    import pytest
    import torch
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    sig = inspect.signature(GroupNorms.sums)
    assert sig.parameters["momentum"].default == 0.0 and sig.parameters["weight_decay"].default == 0.0
    assert sig.parameters["momentum_buffers"].default is None
    m = MMTM_MVCNN()
    st = BalancedStep(m, lr=0.05, compute_dtype=torch.float32, channels_last=True)
    assert st.momentum == 0.0 and st.weight_decay == 0.0
    assert st.flat_momentum is None and st.momentum_buffer(next(m.parameters())) is None
    st = BalancedStep(m, lr=0.05, compute_dtype=torch.float32, channels_last=True, momentum=0.9, weight_decay=5e-4)
    assert st.flat_momentum.shape == st.flat.param.shape and not st.flat_momentum.any()
    for p in m.parameters():  # the views pair with the parameters: same offsets, shape and stride
        b = st.momentum_buffer(p)
        assert b.shape == p.shape and b.stride() == p.stride()
        assert b.data_ptr() - st.flat_momentum.data_ptr() == p.data_ptr() - st.flat.param.data_ptr()
    for bad in (dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(momentum=float("nan"))):
        with pytest.raises(ValueError):
            BalancedStep(m, lr=0.05, compute_dtype=torch.float32, channels_last=False, **bad)


def test_training_loop_opt_in_is_bindable_and_off_by_default():
    import pytest
    from greedy_multimodal_learning_amd import gin_lite
    from greedy_multimodal_learning_amd.train import training_loop
    assert inspect.signature(training_loop).parameters["fused_momentum"].default is False
    gin_lite.clear_config()
    try:
        gin_lite.parse_config("training_loop.fused_momentum=True\n")
        assert gin_lite.query("training_loop", "fused_momentum") is True
        # the binding fills the call (an unknown parameter name would be a ValueError here)
        filled = gin_lite._fill("training_loop", inspect.signature(training_loop), (), {})
        assert filled == {"fused_momentum": True}
    finally:
        gin_lite.clear_config()
    with pytest.raises(NotImplementedError, match="fused_momentum"):
        training_loop(model=None, loss_function=None, metrics=[], optimizer=(0.1, 0.0, 5e-4), config={},
                      save_path=None, steps_per_epoch=1)
