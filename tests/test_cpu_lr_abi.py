"""The device-resident learning rate on the C ABI and above it, without a GPU: gm_group_sumsq_lr and
gm_lr_at declared, exported and bound; the LrState mirror's layout; the argument checks (they run
before any launch); the schedule rule on the host (gm_lr_at, the function the finalize kernel
runs) against its Python restatement (LRSchedule.lr_at) and against torch's schedulers; the gin
keys of the training entry.

Tolerance of gm_lr_at against lr_at: both work in fp64 and round once to fp32.  The C++ compiler
may contract the warm-up's s + (1 - s) * (t / W) and the cosine's min + (base - min) * c into
fused multiply-adds, which moves the fp64 value by at most an fp64 ulp and so the fp32 rounding
by at most one fp32 ulp.  Where no contraction can change the value the results are bit-equal:
held (no arithmetic), multistep at t >= W (products only) and cosine at t >= T (cos(pi) = -1
exactly, so the cosine term is 0 and the result (float)min_lr)."""
import ctypes
import inspect
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_group_sumsq_lr", "gm_lr_at")


def _lib():
    from greedy_multimodal_learning_amd import build, _lib as L
    build.build()
    return L, L.load()


def _schedules():
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    return {"held": (LRSchedule("held", 0.05), 40),
            "multistep": (LRSchedule("multistep", 0.05, warmup_steps=5, warmup_start=0.1, milestones=(8, 8, 20),
                                     gamma=0.3), 40),
            "cosine": (LRSchedule("cosine", 0.05, warmup_steps=5, warmup_start=0.1, total_steps=40, min_lr=1e-3),
                       40)}


def _ulps(a, b):
    """distance of two non-negative fp32 values in units of the last place"""
    ia, ib = (struct.unpack("i", struct.pack("f", v))[0] for v in (a, b))
    return abs(ia - ib)


def test_entry_points_declared_exported_and_bound():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "greedymml.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.EXPORTS, name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == L.EXPORTS[name][1], name
    assert len(L.EXPORTS["gm_group_sumsq_lr"][1]) == 15
    assert len(L.EXPORTS["gm_lr_at"][1]) == 3
    assert lib.gm_abi_version() == 5 and L.ABI_VERSION == 5  # additive: the version stays
    assert re.search(r"#define\s+GM_ABI_VERSION\s+5\b", hdr)
    assert re.search(r"#define\s+GM_LR_MAX_MILESTONES\s+%d\b" % L.LR_MAX_MILESTONES, hdr)


def test_lr_state_layout_matches_header(tmp_path):
    """The ctypes mirror has the C compiler's size and field offsets (as
    test_cpu_host.py::test_struct_layouts_match_header checks the other structs)."""
    from greedy_multimodal_learning_amd import _lib as L
    assert L.LrState.lr.offset == 0
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "greedymml.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(struct gm_lr_state));']
    for f, _ in L.LrState._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(struct gm_lr_state, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.LrState)
    for f, _ in L.LrState._fields_:
        assert int(got[f]) == getattr(L.LrState, f).offset, f


def test_group_sumsq_lr_argument_errors_before_any_launch():
    L, lib = _lib()
    # well-formed arguments; the pointers are never dereferenced on the host and every call below
    # fails its checks before a launch
    tab, mom, lrs, out, scratch, gate = 0x1000, 0x2000, 0x6000, 0x3000, 0x4000, 0x5000
    nbytes = lib.gm_group_sumsq_scratch(100)

    def call(table=tab, mom=mom, ngroups=4, lr=lrs, mu=0.9, wd=5e-4, gate=None, gate_n=0):
        rc = lib.gm_group_sumsq_lr(table, mom, 1, 100, ngroups, 1.0, lr, mu, wd, out, scratch, nbytes, gate,
                                   gate_n, None)
        return rc, lib.gm_last_error()

    rc, msg = call(lr=None)
    assert rc == -1 and b"null lr state" in msg
    rc, msg = call(lr=None, mom=None, mu=0.0, wd=0.0)  # (the plain form needs it too)
    assert rc == -1 and b"null lr state" in msg
    rc, msg = call(table=None)
    assert rc == -1 and b"empty" in msg
    for bad in (-0.1, float("nan"), float("inf")):
        rc, msg = call(mu=bad)
        assert rc == -1 and b"momentum" in msg
    for bad in (-1e-4, float("nan")):
        rc, msg = call(wd=bad)
        assert rc == -1 and b"weight_decay" in msg
    rc, msg = call(mom=None)  # momentum 0.9 without buffers
    assert rc == -1 and b"buffers" in msg
    rc, msg = call(mu=0.0)  # buffers without a momentum
    assert rc == -1 and b"buffers" in msg
    rc, msg = call(ngroups=8, gate=gate, gate_n=0)
    assert rc == -1 and b"two-branch" in msg
    rc, msg = call(ngroups=5, gate=gate, gate_n=1)
    assert rc == -1 and b"N-branch" in msg
    rc, msg = call(ngroups=33)
    assert rc == -1 and b"ngroups" in msg


def _at(lib, st, t):
    out = ctypes.c_float()
    rc = lib.gm_lr_at(ctypes.byref(st), t, ctypes.byref(out))
    return rc, out.value, lib.gm_last_error()


def test_lr_at_refuses_what_a_device_state_cannot_be_checked_for():
    L, lib = _lib()
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    good = LRSchedule("cosine", 0.05, warmup_steps=5, total_steps=40).struct()
    assert _at(lib, good, 3)[0] == 0
    st = LRSchedule("cosine", 0.05, warmup_steps=5, total_steps=40).struct()
    st.total_steps = 5  # T <= W
    rc, _, msg = _at(lib, st, 3)
    assert rc == -1 and b"total_steps" in msg
    st = LRSchedule("multistep", 0.05, milestones=(1, 2, 3)).struct()
    st.n_milestones = 9
    rc, _, msg = _at(lib, st, 3)
    assert rc == -1 and b"n_milestones" in msg
    for field in ("base_lr", "min_lr", "lr"):
        st = LRSchedule("multistep", 0.05, milestones=(1,)).struct()
        setattr(st, field, -0.01)
        rc, _, msg = _at(lib, st, 3)
        assert rc == -1 and b"rates" in msg, field
    st = LRSchedule("held", 0.05).struct()
    st.base_lr = float("nan")
    assert _at(lib, st, 0)[0] == -1
    st = LRSchedule("held", 0.05).struct()
    st.kind = 3
    rc, _, msg = _at(lib, st, 0)
    assert rc == -1 and b"kind" in msg
    assert _at(lib, good, -1)[0] == -1
    assert lib.gm_lr_at(None, 0, None) == -1
    # LRSchedule refuses the same on construction
    for kw in (dict(kind="cosine", base_lr=0.05, warmup_steps=5, total_steps=5), dict(kind="cosine", base_lr=0.05),
               dict(kind="multistep", base_lr=0.05, milestones=tuple(range(9))),
               dict(kind="multistep", base_lr=-0.05), dict(kind="cosine", base_lr=0.05, total_steps=9, min_lr=-1.0),
               dict(kind="multistep", base_lr=0.05, gamma=float("nan")), dict(kind="step", base_lr=0.05),
               dict(kind="multistep", base_lr=0.05, warmup_steps=-1)):
        with pytest.raises(ValueError):
            LRSchedule(**kw)


@pytest.mark.parametrize("name", ["held", "multistep", "cosine"])
def test_lr_at_matches_the_python_rule(name):
    L, lib = _lib()
    sch, T = _schedules()[name]
    st = sch.struct()
    W = sch.warmup_steps
    worst = 0
    for t in range(T + 6):
        rc, got, msg = _at(lib, st, t)
        assert rc == 0, msg
        want = sch.lr_at(t)
        closed = name == "held" or (name == "multistep" and t >= W) or (name == "cosine" and t >= T)
        if closed:
            assert got == want, (t, got, want)
        d = _ulps(got, want)
        worst = max(worst, d)
        assert d <= 1, (t, got, want, d)
    print(f"{name}: worst distance {worst} ulp over t = 0..{T + 5}")
    if name == "cosine":  # the schedule ends exactly on (float)min_lr, and warm-up starts on s * base
        assert _at(lib, st, T)[1] == struct.unpack("f", struct.pack("f", 1e-3))[0]
        assert sch.lr_at(T + 100) == sch.lr_at(T)
    if name != "held":
        assert _ulps(sch.lr_at(0), struct.unpack("f", struct.pack("f", 0.05 * 0.1))[0]) <= 1
        assert sch.lr_at(W) == struct.unpack("f", struct.pack("f", 0.05))[0]


def test_pack_is_the_struct_with_the_rate_of_its_step():
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd.lr_schedule import unpack
    sch, _ = _schedules()["multistep"]
    raw = sch.pack(9)
    assert len(raw) == ctypes.sizeof(L.LrState)
    st = unpack(raw)
    assert st.step == 9 and st.kind == 1 and st.lr == sch.lr_at(9)
    assert struct.unpack("f", raw[:4])[0] == sch.lr_at(9)  # lr at offset 0
    assert list(st.milestones[:3]) == [8, 8, 20] and st.n_milestones == 3
    assert unpack(sch.pack()).step == 0


def test_lr_at_matches_torch_schedulers_without_warmup():
    import torch
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    cases = [(LRSchedule("multistep", 0.05, milestones=(3, 3, 7), gamma=0.3),
              lambda o: torch.optim.lr_scheduler.MultiStepLR(o, milestones=[3, 3, 7], gamma=0.3), 12),
             (LRSchedule("cosine", 0.05, total_steps=20, min_lr=1e-3),
              lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20, eta_min=1e-3), 20)]
    for sch, make, last in cases:
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.05)
        ts = make(opt)
        worst = 0.0
        for t in range(last + 1):
            ref = opt.param_groups[0]["lr"]
            rel = abs(sch.lr_at(t) - ref) / ref
            worst = max(worst, rel)
            assert rel <= 1e-6, (sch.kind, t, sch.lr_at(t), ref)
            opt.step()
            ts.step()
        print(f"{sch.kind}: worst relative difference to torch {worst:.2e}")


def test_engine_and_group_norms_take_the_schedule():
    import torch
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    assert inspect.signature(GroupNorms.sums).parameters["lr_state"].default is None
    assert inspect.signature(BalancedStep.__init__).parameters["lr_schedule"].default is None
    m = MMTM_MVCNN()
    st = BalancedStep(m, lr=0.05, compute_dtype=torch.float32, channels_last=True)
    assert st.lr == 0.05 and st.lr_state is None and st.sync_lr() is None
    assert st._graph_key()[-1] == 0.05  # the default path keeps the rate in the graph key
    st.lr = 0.015
    assert st.lr == 0.015 and st._graph_key()[-1] == 0.015
    with pytest.raises(ValueError):
        st.set_lr_step(3)
    sch = LRSchedule("multistep", 0.05, warmup_steps=2, warmup_start=0.5, milestones=(5,))
    st = BalancedStep(m, lr=0.05, compute_dtype=torch.float32, channels_last=True, lr_schedule=sch)
    assert st.lr_state.dtype == torch.uint8 and bytes(st.lr_state.numpy().tobytes()) == sch.pack(0)
    assert st.lr == sch.lr_at(0) and st.sync_lr().step == 0
    key = st._graph_key()
    with pytest.raises(ValueError, match="multistep"):
        st.lr = 0.01
    st.set_lr_step(6)
    assert st.lr == sch.lr_at(6) and st.sync_lr().step == 6 and st.sync_lr().lr == sch.lr_at(6)
    assert st._graph_key() == key  # one key for every rate


def test_training_loop_keys_bind_and_default_to_off():
    from greedy_multimodal_learning_amd import gin_lite
    from greedy_multimodal_learning_amd.train import training_loop
    defaults = dict(lr_schedule=None, lr_warmup_steps=0, lr_warmup_start=0.0, lr_milestones=(), lr_gamma=0.1,
                    lr_total_steps=None, lr_min=0.0)
    par = inspect.signature(training_loop).parameters
    for k, v in defaults.items():
        assert par[k].default == v, k
    gin_lite.clear_config()
    try:
        gin_lite.parse_config("training_loop.lr_schedule='cosine'\ntraining_loop.lr_warmup_steps=5\n"
                              "training_loop.lr_warmup_start=0.1\ntraining_loop.lr_milestones=(8, 8, 20)\n"
                              "training_loop.lr_gamma=0.3\ntraining_loop.lr_total_steps=40\n"
                              "training_loop.lr_min=1e-3\n")
        filled = gin_lite._fill("training_loop", inspect.signature(training_loop), (), {})
        assert filled == dict(lr_schedule="cosine", lr_warmup_steps=5, lr_warmup_start=0.1, lr_milestones=(8, 8, 20),
                              lr_gamma=0.3, lr_total_steps=40, lr_min=1e-3)
    finally:
        gin_lite.clear_config()


def test_device_run_schedule_refuses_reduce_on_plateau():
    from greedy_multimodal_learning_amd.callbacks import ReduceLROnPlateau_PyTorch
    from greedy_multimodal_learning_amd.train import training_loop
    plateau = ReduceLROnPlateau_PyTorch(metric="loss")
    for kind, kw in (("multistep", dict(lr_milestones=(3,))), ("cosine", dict())):
        with pytest.raises(ValueError, match="ReduceLROnPlateau_PyTorch"):
            training_loop(model=None, loss_function=None, metrics=[], optimizer=(0.1, 0.0, 0.0), config={},
                          save_path=None, steps_per_epoch=4, n_epochs=3, custom_callbacks=[plateau],
                          lr_schedule=kind, **kw)
    with pytest.raises(ValueError, match="kind"):  # an unknown schedule name, before anything runs
        training_loop(model=None, loss_function=None, metrics=[], optimizer=(0.1, 0.0, 0.0), config={},
                      save_path=None, steps_per_epoch=4, lr_schedule="linear")
