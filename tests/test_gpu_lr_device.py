"""The device-resident learning rate (gm_group_sumsq_lr, BalancedStep(lr_schedule=...)).

Pass level: every update form of gm_group_sumsq_lr against the scalar entry points on clones at
the same rate - parameters, momentum buffers, sums and gate state torch.equal after every pass
(the kernels share stream_segment / chunk_sums; only where the rate comes from differs).
Schedule: 45 passes per schedule with the state read back after each - step counts the passes,
lr follows LRSchedule.lr_at (the bound of tests/test_cpu_lr_abi.py: 1 fp32 ulp where a compiler
may contract the fp64 expression, bit-equal where the rule is closed), and the update used
exactly the stored rate.
Engine: one captured graph over a schedule whose rate moves every few steps, torch.equal to an
engine without a schedule whose lr is set to lr_at(t) before each step (it re-captures per rate;
both run graphs, and graph-to-graph comparisons are exact here:
test_gpu_graphs.py::test_bound_batches_equal_copied_batches); held; momentum; one-rank data
parallel; the training entry."""
import ctypes
import os
import socket
import struct

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

# the two parameter sets of test_gpu_sgdm.py: 43 k elements in three 16384-element chunks, with
# tensors straddling a chunk boundary and 1- and 7-element tensors on the scalar head and tail ...
SHAPES8 = {"net_view_0.a": (3, 5), "net_view_0.b": (40000,), "net_view_1.c": (7,),
           "net_view_1.d": (100, 333), "mmtm2.fc_squeeze.weight": (16, 32),
           "mmtm2.fc_visual.bias": (16,), "mmtm3.fc_skeleton.weight": (64, 65),
           "net_view_1.e": (1,)}
TWO = (["net_view_0", "net_view_1"], ["visual", "skeleton"])
SENTINEL = 7.25


def _twelve():
    """... and 12 branches, 24 groups: the _runs kernels"""
    V = 12
    shapes = {}
    for i in range(V):
        shapes[f"net_view_{i}.conv.weight"] = (64, 3, 3, 3)
        shapes[f"net_view_{i}.bn.bias"] = (64,)
        shapes[f"mmtm4.fc_excite.{i}.weight"] = (32, 16)
    shapes["mmtm4.fc_squeeze.weight"] = (16, 384)
    return shapes, ([f"net_view_{i}" for i in range(V)], [f"fc_excite.{i}." for i in range(V)])


SETS = {"eight": lambda: (SHAPES8, TWO, None, "net_view_1.d"),
        "twelve": lambda: _twelve() + (12, "net_view_3.conv.weight")}
# (momentum, weight decay, buffers one float off congruence, one entry without a gradient)
FORMS = {"plain": (0.0, 0.0, False, False), "decay": (0.0, 5e-4, False, False),
         "momentum-decay": (0.9, 5e-4, False, False), "momentum-scalar-path": (0.9, 5e-4, True, False),
         "skipped-entry": (0.9, 5e-4, False, True)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _schedules():
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    return {"held": LRSchedule("held", 0.05),
            "multistep": LRSchedule("multistep", 0.05, warmup_steps=5, warmup_start=0.1, milestones=(8, 8, 20),
                                    gamma=0.3),
            "cosine": LRSchedule("cosine", 0.05, warmup_steps=5, warmup_start=0.1, total_steps=40, min_lr=1e-3)}


def _gate_state(dev, nb=None):
    from greedy_multimodal_learning_amd import _lib as L
    st = L.GateState() if nb is None else L.GateStateN()
    if nb is not None:
        st.nb = nb
    st.caring, st.window, st.eps = -1, 2, 2e-3
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).to(dev)


def _lr_state(dev, sch, step=0):
    return torch.frombuffer(bytearray(sch.pack(step)), dtype=torch.uint8).to(dev)


def _read(state):
    from greedy_multimodal_learning_amd.lr_schedule import unpack
    return unpack(state.cpu().numpy().tobytes())


def _param_sets(dev, shapes, mu, skew, nograd, seed, copies=2):
    """`copies` identical parameter sets (and momentum buffers, skewed alike) on the device"""
    g = torch.Generator().manual_seed(seed)
    host = {n: torch.randn(*s, generator=g) for n, s in shapes.items()}
    sets = []
    for _ in range(copies):
        params = [(n, torch.nn.Parameter(w.to(dev))) for n, w in host.items()]
        bufs = None
        if mu != 0:
            bufs = []
            for n, p in params:
                big = torch.zeros(p.numel() + 1, device=dev)
                b = big[1:].view(p.shape) if skew else big[:-1].view(p.shape)
                assert (b.data_ptr() - p.data_ptr()) % 16 == (4 if skew else 0)
                if n in nograd:
                    b.fill_(SENTINEL)
                bufs.append(b)
        sets.append((params, bufs))
    return g, host, sets


def _new_grads(g, sets, nograd, scale=1.0):
    for n, p in sets[0][0]:
        gr = None if n in nograd else torch.randn(p.shape, generator=g) * scale
        for params, _ in sets:
            dict(params)[n].grad = None if gr is None else gr.to(p.device)


def _ulps(a, b):
    ia, ib = (struct.unpack("i", struct.pack("f", v))[0] for v in (a, b))
    return abs(ia - ib)


# ---------------------------------------------------------------------------------------
# 1. pass level: bit for bit against the scalar entry points
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [False, True], ids=["no-gate", "gate"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", SETS)
def test_pass_equals_scalar_entry_points(dev, which, form, gated):
    """Three passes with a held state rewritten to 0.1, 0.03 and 0.0.  At rate 0 the scalar plain
    entry chooses the sums-only form and the device-rate one computes fmaf(-0, g, w): equal for
    finite gradients, which these are."""
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    shapes, names, nb, skipped = SETS[which]()
    mu, wd, skew, skip = FORMS[form]
    nograd = (skipped,) if skip else ()
    g, host, sets = _param_sets(dev, shapes, mu, skew, nograd, seed=21)
    (pa, ba), (pb, bb) = sets
    na, nbm = GroupNorms(pa, *names), GroupNorms(pb, *names)
    state = _lr_state(dev, LRSchedule("held", 0.5))
    gate_a = gate_b = None
    gkw = {}
    if gated:
        gate_a, gate_b = _gate_state(dev, nb), _gate_state(dev, nb)
        gkw = dict(gate_n=nb is not None)
    for k, rate in enumerate((0.1, 0.03, 0.0), 1):
        _new_grads(g, sets, nograd)
        state[:4].view(torch.float32).fill_(rate)
        out = na.sums(grad_scale=0.5, lr_state=state, momentum=mu, weight_decay=wd, momentum_buffers=ba,
                      gate=gate_a, **gkw)
        want = nbm.sums(grad_scale=0.5, lr=rate, momentum=mu, weight_decay=wd, momentum_buffers=bb, gate=gate_b,
                        **gkw)
        assert torch.equal(out, want), (k, (out - want).abs().max())
        assert bool(torch.isfinite(out).all()) and bool((out[::2] > 0).all())
        for (n, a), (_, b) in zip(pa, pb):
            assert torch.equal(a.detach(), b.detach()), (n, k)
            if n in nograd:
                assert torch.equal(a.detach().cpu(), host[n]), n
            elif rate != 0.0:
                assert not torch.equal(a.detach().cpu(), host[n]), n  # (the update ran)
        if ba is not None:
            for (n, _), a, b in zip(pa, ba, bb):
                assert torch.equal(a, b), (n, k)
                assert bool((a == SENTINEL).all()) == (n in nograd), n
        if gated:
            assert torch.equal(gate_a, gate_b), k
            assert bool(gate_a.any())
        st = _read(state)
        assert st.step == k and st.lr == struct.unpack("f", struct.pack("f", rate))[0]  # held: lr left alone


def test_group_norms_refuses_two_owners_and_misplaced_states(dev):
    from greedy_multimodal_learning_amd._lib import GreedyMMLError
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    p = torch.nn.Parameter(torch.randn(8, 4, device=dev))
    p.grad = torch.randn(8, 4, device=dev)
    w0 = p.detach().clone()
    gn = GroupNorms([("net_view_0.w", p)], *TWO)
    state = _lr_state(dev, _schedules()["held"])
    for kw in (dict(lr=0.1, lr_state=state), dict(lr_state=state[:64]), dict(lr_state=state.cpu()),
               dict(lr_state=state.view(torch.float32)), dict(lr_state=torch.zeros(137, dtype=torch.uint8,
                                                                                   device=dev)[1:])):
        with pytest.raises(GreedyMMLError):
            gn.sums(**kw)
    assert torch.equal(p.detach(), w0) and _read(state).step == 0


# ---------------------------------------------------------------------------------------
# 2. the schedule on the device
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mu,wd", [("held", 0.0, 5e-4), ("multistep", 0.9, 5e-4), ("cosine", 0.0, 0.0)])
def test_schedule_advances_on_the_device(dev, name, mu, wd):
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    sch = _schedules()[name]
    W, T = sch.warmup_steps, 40
    g, host, sets = _param_sets(dev, SHAPES8, mu, False, (), seed=22)
    (pa, ba), (pb, bb) = sets
    na, nbm = GroupNorms(pa, *TWO), GroupNorms(pb, *TWO)
    _new_grads(g, sets, (), scale=0.1)
    state = _lr_state(dev, sch)
    before = _read(state)
    assert before.step == 0 and before.lr == sch.lr_at(0)
    worst = 0
    for k in range(1, 46):
        out = na.sums(lr_state=state, momentum=mu, weight_decay=wd, momentum_buffers=ba)
        want = nbm.sums(lr=before.lr, momentum=mu, weight_decay=wd, momentum_buffers=bb)
        after = _read(state)
        assert after.step == k
        ref = sch.lr_at(k)
        closed = name == "held" or (name == "multistep" and k >= W) or (name == "cosine" and k >= T)
        d = _ulps(after.lr, ref)
        worst = max(worst, d)
        if closed:
            assert after.lr == ref, (k, after.lr, ref)
        assert d <= 1, (k, after.lr, ref, d)
        # the update used exactly the rate that was stored before the pass
        assert torch.equal(out, want), k
        for (n, a), (_, b) in zip(pa, pb):
            assert torch.equal(a.detach(), b.detach()), (n, k)
        if ba is not None:
            for a, b in zip(ba, bb):
                assert torch.equal(a, b), k
        # nothing but lr and step moves in the state
        assert bytes(after)[16:] == bytes(before)[16:] and after.kind == before.kind
        before = after
    print(f"{name}: worst distance to lr_at {worst} ulp over 45 passes")
    assert bool(torch.isfinite(pa[1][1]).all())
    if name == "cosine":
        assert before.lr == struct.unpack("f", struct.pack("f", 1e-3))[0]  # ends exactly on (float)min_lr


# ---------------------------------------------------------------------------------------
# 3-6. engine: the model, batches and gate of test_gpu_graphs.py
# ---------------------------------------------------------------------------------------
def _engine(steps, schedule=None, rates=None, set_after=None, momentum=0.0, weight_decay=0.0, pg=None, gated=True,
            probe=False):
    """`steps` graph steps.  schedule: the engine's LRSchedule; rates (no schedule): lr = rates(t)
    before step t; set_after = (k, value): lr = value after step k (both kinds of engine)."""
    from greedy_multimodal_learning_amd.callbacks import Bias_Mitigation_Strong
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = MMTM_MVCNN().to(dev)
    gate = Bias_Mitigation_Strong(epsilon=2e-3, curation_windowsize=2, branchnames=["net_view_0", "net_view_1"],
                                  starting_epoch=1) if gated else None
    kw = dict(process_group=pg, dp_buckets=True) if pg is not None else {}
    st = BalancedStep(m, lr=0.05, gate=gate, graphs=True, device_gate=True, momentum=momentum,
                      weight_decay=weight_decay, lr_schedule=schedule, **kw)
    assert st.device_gate == gated
    st.on_epoch_begin(1)
    g = torch.Generator(device=dev).manual_seed(5)
    xs = [torch.randn(4, 2, 3, 64, 64, device=dev, generator=g) for _ in range(3)]
    ys = [torch.randint(0, 40, (4,), device=dev, generator=g) for _ in range(3)]
    ngraphs, seen = [], []
    refused = None
    for i in range(steps):
        if rates is not None:
            st.lr = rates(i)
        seen.append(st.lr)
        st(xs[i % 3], ys[i % 3])
        ngraphs.append(len(st._graphs))
        if set_after is not None and i + 1 == set_after[0]:
            st.lr = set_after[1]
    if probe:  # setting the rate under a device-run schedule
        try:
            st.lr = 0.01
        except ValueError as e:
            refused = str(e)
    torch.cuda.synchronize()
    lrs = st.sync_lr()
    out = dict(state={k: v.detach().cpu() for k, v in m.state_dict().items()},
               mmtm={f"mmtm{i}.{s}": getattr(getattr(m, f"mmtm{i}"), f"running_avg_weight_{s}").detach().cpu()
                     for i in (2, 3, 4) for s in ("visual", "skeleton")},
               gate=st.gate_state.cpu() if gated else None, graphs=bool(st.graphs), ngraphs=ngraphs,
               failures=list(st.capture_failures), seen=seen, refused=refused,
               mom=None if st.flat_momentum is None else st.flat_momentum.cpu(),
               lr_step=None if lrs is None else int(lrs.step), lr=None if lrs is None else float(lrs.lr))
    return out


def _same(a, b):
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), k
    for k in a["mmtm"]:
        assert torch.equal(a["mmtm"][k], b["mmtm"][k]), k
    if a["gate"] is not None:
        assert torch.equal(a["gate"], b["gate"])
    if a["mom"] is not None:
        assert torch.equal(a["mom"], b["mom"])


def test_engine_one_graph_for_a_moving_rate(dev):
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    sch = LRSchedule("multistep", 0.05, warmup_steps=2, warmup_start=0.5, milestones=(5,), gamma=0.1)
    assert len({sch.lr_at(t) for t in range(8)}) == 4  # the rate moves: four rates in eight steps
    d = _engine(8, schedule=sch, probe=True)
    assert d["graphs"] and d["failures"] == []
    assert d["ngraphs"] == [0] + [1] * 7  # (the first step runs eagerly) one graph for every rate
    assert d["seen"] == [sch.lr_at(t) for t in range(8)]  # the getter, without a sync
    assert d["lr_step"] == 8 and d["lr"] == sch.lr_at(8)
    assert d["refused"] is not None and "multistep" in d["refused"]
    s = _engine(8, rates=sch.lr_at)
    assert s["graphs"] and s["failures"] == [] and s["lr_step"] is None
    assert s["ngraphs"][-1] == 1 and s["seen"] == d["seen"]
    _same(d, s)
    assert bool(d["gate"].any())


def test_engine_held_rate_is_a_fill(dev):
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    d = _engine(8, schedule=LRSchedule("held", 0.05), set_after=(4, 0.015))
    assert d["graphs"] and d["failures"] == []
    assert d["ngraphs"] == [0] + [1] * 7
    assert d["seen"] == [0.05] * 4 + [0.015] * 4
    assert d["lr_step"] == 8 and d["lr"] == struct.unpack("f", struct.pack("f", 0.015))[0]
    s = _engine(8, set_after=(4, 0.015))
    assert s["graphs"] and s["seen"] == d["seen"]
    _same(d, s)


def test_engine_momentum_under_a_schedule(dev):
    sch = _schedules()["cosine"]
    d = _engine(5, schedule=sch, momentum=0.9, weight_decay=5e-4)
    s = _engine(5, rates=sch.lr_at, momentum=0.9, weight_decay=5e-4)
    assert d["graphs"] and s["graphs"] and d["failures"] == [] and d["ngraphs"][-1] == 1
    assert d["lr_step"] == 5 and _ulps(d["lr"], sch.lr_at(5)) <= 1
    _same(d, s)
    assert bool(d["mom"].any())


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_schedule():
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    return LRSchedule("multistep", 0.05, warmup_steps=2, warmup_start=0.5, milestones=(4,), gamma=0.1)


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    out = _engine(5, schedule=_dp_schedule(), pg=dist.group.WORLD, gated=False)
    torch.save({k: out[k] for k in ("state", "mmtm", "graphs", "ngraphs", "lr_step", "lr")},
               os.path.join(out_dir, "dp.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_engine_one_rank_data_parallel_equals_no_group(dev, tmp_path):
    """A one-rank gloo group (the pass runs eagerly behind each replay, grad_scale = 1 / world)
    against the same run without a group, as test_gpu_sgdm.py's one-rank test."""
    mp.start_processes(_dp_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True, start_method="spawn")
    dp = torch.load(tmp_path / "dp.pt", weights_only=True)
    e = _engine(5, schedule=_dp_schedule(), gated=False)
    assert dp["graphs"] and e["graphs"]
    assert dp["ngraphs"][-1] == 1 and e["ngraphs"][-1] == 1
    assert dp["lr_step"] == e["lr_step"] == 5 and dp["lr"] == e["lr"] == _dp_schedule().lr_at(5)
    for k in e["state"]:
        assert torch.equal(dp["state"][k], e["state"][k]), k
    for k in e["mmtm"]:
        assert torch.equal(dp["mmtm"][k], e["mmtm"][k]), k


# ---------------------------------------------------------------------------------------
# 7. the training entry: test_gpu_entry.py's tiny dataset
# ---------------------------------------------------------------------------------------
ENTRY = """
MMTM_MVCNN.pretraining=False
MMTM_MVCNN.num_views=2
train.batch_size=4
train.lr=0.1
train.wd=0.0
train.momentum=0
train.callbacks=['Bias_Mitigation_Strong']
Bias_Mitigation_Strong.epsilon=0.01
Bias_Mitigation_Strong.curation_windowsize=5
Bias_Mitigation_Strong.starting_epoch=1
Bias_Mitigation_Strong.branchnames=['net_view_0', 'net_view_1']
Bias_Mitigation_Strong.MMTMnames = ['visual', 'skeleton']
training_loop.nummodalities=2
training_loop.device_numbers=[0]
training_loop.checkpoint_monitor='val_acc'
get_mvdcndata.num_views=2
get_mvdcndata.num_workers=0
get_mvdcndata.specific_views=[0, 6]
"""


def _dataset(root, n_train=14, n_test=5, H=64, views=12, seed=3):
    import json
    R = np.random.default_rng(seed)
    meta = {"classnames": [f"c{i}" for i in range(40)], "train": [], "test": []}
    for split, n in (("train", n_train), ("test", n_test)):
        os.makedirs(os.path.join(root, split))
        for i in range(n):
            c = int(R.integers(40))
            meta[split].append({"classname": f"c{c}", "model": f"m{split}{i}"})
            np.save(os.path.join(root, split, f"m{split}{i}.npy"),
                    R.integers(0, 256, (views, H, H, 3), dtype=np.uint8))
    with open(os.path.join(root, "metadata.json"), "w") as f:
        json.dump(meta, f)


def _train(text, save):
    from greedy_multimodal_learning_amd import gin_lite
    from greedy_multimodal_learning_amd.train import train
    gin_lite.clear_config()
    try:
        gin_lite.parse_config(text)
        os.makedirs(save, exist_ok=True)
        return train(save)
    finally:
        gin_lite.clear_config()


def test_training_entry_runs_the_schedule(dev, tmp_path):
    """12 training samples at batch 4: 3 steps per epoch, 2 epochs, a milestone inside epoch 2."""
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    data = str(tmp_path / "data")
    _dataset(data)
    ds = f"\nget_mvdcndata.root_dir='{data}'\n"
    sched = ("training_loop.n_epochs=3\ntraining_loop.lr_schedule='multistep'\ntraining_loop.lr_warmup_steps=2\n"
             "training_loop.lr_warmup_start=0.5\ntraining_loop.lr_milestones=(4,)\ntraining_loop.lr_gamma=0.3\n")
    H = _train(ENTRY + ds + sched, str(tmp_path / "sched"))
    ref = LRSchedule("multistep", 0.1, warmup_steps=2, warmup_start=0.5, milestones=(4,), gamma=0.3)
    assert len(H["loss"]) == 2 and all(np.isfinite(H["loss"]))
    assert H["lr"] == [ref.lr_at(3), ref.lr_at(6)] and ref.lr_at(3) != ref.lr_at(6)
    ck = torch.load(os.path.join(str(tmp_path / "sched"), "model_last_epoch.pt"), weights_only=True)
    assert set(ck) == {"model", "optimizer", "lr_schedule"}
    assert ck["optimizer"]["param_groups"][0]["lr"] == ref.lr_at(6)
    assert ck["lr_schedule"]["step"] == 6
    assert LRSchedule(**ck["lr_schedule"]["params"]).pack(6) == ref.pack(6)
    # off by default: no key in the checkpoint, no lr in the history
    H0 = _train(ENTRY + ds + "training_loop.n_epochs=2\n", str(tmp_path / "plain"))
    ck0 = torch.load(os.path.join(str(tmp_path / "plain"), "model_last_epoch.pt"), weights_only=True)
    assert set(ck0) == {"model", "optimizer"} and "lr" not in H0
    assert ck0["optimizer"]["param_groups"][0]["lr"] == 0.1
