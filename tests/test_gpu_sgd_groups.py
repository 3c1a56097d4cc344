"""gm_group_sumsq_pg: the norms pass with parameter groups (per-tensor rate scale and weight decay
from a device table) and Nesterov momentum.

Kernel level (GroupNorms.sums(lr_state=, pgroups=, nesterov=)): parameters and buffers against
torch.optim.SGD in float64 with real param groups, the group sums and both gate states against the
plain entry points on clones; every element exactly on dyadic operands; a one-group table against
gm_group_sumsq_lr bit for bit; the index clamp.
Engine level (BalancedStep(param_groups=, nesterov=)): each step's update recomputed in float64
per group from the flat buffers, graph == eager with one graph also across set_param_group, the
no-decay recipe, the defaults untouched, one-rank data parallel, a run continued from its own
checkpoint, and the training entry.

Bound after step k against float64: k * (1e-7 + 1e-6 * |ref|), test_gpu_sgdm.py's."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_sgdm import SENTINEL, SHAPES8, TWO, _free_port, _gate_state, _twelve, _within

pytestmark = pytest.mark.gpu

TABLE = [(1.0, 5e-4), (0.3, 0.0), (2.5, 1e-2)]
# consecutive tensors in different groups: every group boundary of SHAPES8 (78 011 elements, five
# workgroups' chunks of 16 384; boundaries at 15, 40 015, 40 022, 73 322, ...) falls inside one
# workgroup's chunk, none on a chunk's edge
ASSIGN8 = dict(zip(SHAPES8, (0, 1, 2, 0, 1, 2, 0, 1)))
SETS = {"eight": lambda: (SHAPES8, TWO, ASSIGN8, "net_view_1.d", None),
        "twelve": lambda: _twelve() + (None, "net_view_3.conv.weight", 12)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _set(which):
    shapes, names, assign, skipped, gate_nb = SETS[which]()
    if assign is None:
        assign = {n: i % 3 for i, n in enumerate(shapes)}
    return shapes, names, assign, skipped, gate_nb


def _lr_state(dev, lr, kind="held", **kw):
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    return torch.frombuffer(bytearray(LRSchedule(kind, lr, **kw).pack()), dtype=torch.uint8).to(dev)


def _table(dev, rows):
    return torch.tensor(rows, dtype=torch.float32, device=dev).reshape(-1, 2)


def _buffers(dev, params, skew=False, nograd=()):
    """zero buffers congruent with their parameters mod 16 bytes, or (skew) one float off: the
    scalar path; a sentinel where the entry has no gradient"""
    bufs = []
    for n, p in params:
        big = torch.zeros(p.numel() + 1, device=dev)
        b = big[1:].view(p.shape) if skew else big[:-1].view(p.shape)
        assert (b.data_ptr() - p.data_ptr()) % 16 == (4 if skew else 0)
        if n in nograd:
            b.fill_(SENTINEL)
        bufs.append(b)
    return bufs


# ---------------------------------------------------------------------------------------
# float64 torch.optim.SGD with real param groups
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nesterov", [False, True], ids=["momentum", "nesterov"])
@pytest.mark.parametrize("which", list(SETS))
def test_three_steps_match_float64_sgd_with_param_groups(dev, which, nesterov):
    """Momentum 0.9, grad_scale 0.5, three groups, 3 steps: parameters and buffers within the bound
    of torch.optim.SGD on float64 copies (each group's lr the double product of the fp32 rate and
    the fp32 scale); sums and gate state (two-branch on the eight-tensor set, N-branch on the
    twelve-branch one) torch.equal the plain gate entry's on clones."""
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    shapes, names, assign, _, gate_nb = _set(which)
    lr, mu = 0.1, 0.9
    g = torch.Generator().manual_seed(21)
    host = {n: torch.randn(*s, generator=g) for n, s in shapes.items()}
    params = [(n, torch.nn.Parameter(w.to(dev))) for n, w in host.items()]
    ref = {n: torch.nn.Parameter(w.double()) for n, w in host.items()}
    opt = torch.optim.SGD([{"params": [ref[n] for n in shapes if assign[n] == i], "lr": _f32(lr) * _f32(s),
                            "weight_decay": wd} for i, (s, wd) in enumerate(TABLE)],
                          lr=lr, momentum=mu, nesterov=nesterov)
    bufs = _buffers(dev, params)
    gn = GroupNorms(params, *names, pgroup_of=assign.__getitem__)
    state, table = _lr_state(dev, lr), _table(dev, TABLE)
    gate, gate_ref = _gate_state(dev, gate_nb), _gate_state(dev, gate_nb)
    for k in range(1, 4):
        clones = []
        for n, p in params:
            gr = torch.randn(p.shape, generator=g)
            p.grad = gr.to(dev)
            ref[n].grad = gr.double() * 0.5
            c = torch.nn.Parameter(p.detach().clone())
            c.grad = p.grad.clone()
            clones.append((n, c))
        want = GroupNorms(clones, *names).sums(grad_scale=0.5, lr=0.0, gate=gate_ref, gate_n=bool(gate_nb))
        out = gn.sums(grad_scale=0.5, lr_state=state, pgroups=table, nesterov=nesterov, momentum=mu,
                      momentum_buffers=bufs, gate=gate, gate_n=bool(gate_nb))
        opt.step()
        assert torch.equal(out, want), (k, (out - want).abs().max())
        assert torch.equal(gate, gate_ref), k
        for i, (n, p) in enumerate(params):
            _within(p, ref[n].detach(), k, n)
            _within(bufs[i], opt.state[ref[n]]["momentum_buffer"], k, n + " (buffer)")
    assert bool(gate.any())


# ---------------------------------------------------------------------------------------
# every element of the update, exactly: integer w, g in [-64, 64], grad_scale 0.5, rate 0.125,
# mu 0.5, scales (1, 0.5, 2) and decays (0.25, 0, 0.5) keep g', d, b', u and w' dyadic rationals
# that fp32 holds - for 3 steps without the Nesterov term and for 2 with it (its u = mu b' + d
# needs one more bit per step) - so any fma order gives the float64 recurrence's value.
# ---------------------------------------------------------------------------------------
EXACT_SCALE, EXACT_LR, EXACT_MU = 0.5, 0.125, 0.5
EXACT_TABLE = [(1.0, 0.25), (0.5, 0.0), (2.0, 0.5)]
# (buffers, nesterov, buffers one float off congruence, one entry without a gradient)
EXACT_FORMS = {"decay": (False, False, False, False), "momentum": (True, False, False, False),
               "nesterov": (True, True, False, False), "momentum-scalar-path": (True, False, True, False),
               "nesterov-scalar-path": (True, True, True, False),
               "momentum-skipped-entry": (True, False, False, True),
               "nesterov-skipped-entry": (True, True, False, True)}


def _exact_reference(shapes, assign, mom, nesterov, nograd, seed):
    """Start values, per-step gradients and the float64 recurrence's parameters and buffers after
    each step, with every intermediate checked to round-trip through float32."""
    def holds(t):
        assert torch.equal(t.float().double(), t), "the operands do not keep the recurrence exact in fp32"
        return t
    steps = 2 if nesterov else 3
    mu = EXACT_MU if mom else 0.0
    g = torch.Generator().manual_seed(seed)
    w = {n: torch.randint(-64, 65, s, generator=g).double() for n, s in shapes.items()}
    b = {n: torch.zeros(s, dtype=torch.float64) for n, s in shapes.items()}
    start, grads, after = {n: t.clone() for n, t in w.items()}, [], []
    for _ in range(steps):
        gr = {n: torch.randint(-64, 65, s, generator=g).double() for n, s in shapes.items() if n not in nograd}
        for n, t in gr.items():
            scale, wd = EXACT_TABLE[assign[n]]
            lr_g = holds(torch.tensor(EXACT_LR * scale, dtype=torch.float64))
            d = holds(wd * w[n] + holds(EXACT_SCALE * t))
            b[n] = holds(mu * b[n] + d)
            u = holds(mu * b[n] + d) if nesterov else b[n]
            w[n] = holds(w[n] - lr_g * u)
        grads.append(gr)
        after.append(({n: t.clone() for n, t in w.items()}, {n: t.clone() for n, t in b.items()}))
    return start, grads, after


@pytest.mark.parametrize("form", EXACT_FORMS)
@pytest.mark.parametrize("which", list(SETS))
def test_update_is_exact_on_dyadic_operands(dev, which, form):
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    shapes, names, assign, skipped, _ = _set(which)
    mom, nesterov, skew, skip = EXACT_FORMS[form]
    nograd = (skipped,) if skip else ()
    # (the reference asserts its own exactness before any launch)
    start, grads, after = _exact_reference(shapes, assign, mom, nesterov, nograd, seed=11)
    params = [(n, torch.nn.Parameter(w.float().to(dev))) for n, w in start.items()]
    bufs = _buffers(dev, params, skew, nograd) if mom else None
    gn = GroupNorms(params, *names, pgroup_of=assign.__getitem__)
    state, table = _lr_state(dev, EXACT_LR), _table(dev, EXACT_TABLE)
    for k in range(1, len(grads) + 1):
        clones = []
        for n, p in params:
            p.grad = grads[k - 1][n].float().to(dev) if n in grads[k - 1] else None
            c = torch.nn.Parameter(p.detach().clone())
            c.grad = None if p.grad is None else p.grad.clone()
            clones.append((n, c))
        want = GroupNorms(clones, *names).sums(grad_scale=EXACT_SCALE, lr=0.0)
        out = gn.sums(grad_scale=EXACT_SCALE, lr_state=state, pgroups=table, nesterov=nesterov,
                      momentum=EXACT_MU if mom else 0.0, momentum_buffers=bufs)
        if not skew:
            assert torch.equal(out, want), (k, (out - want).abs().max())
        else:  # (another accumulation order, as test_gpu_sgdm.py's scalar path)
            torch.testing.assert_close(out, want, rtol=2e-6, atol=0)
        ref_w, ref_b = after[k - 1]
        for i, (n, p) in enumerate(params):
            got = p.detach().double().cpu()
            assert torch.equal(got, ref_w[n]), (n, k, float((got - ref_w[n]).abs().max()))
            if bufs is not None:
                got = bufs[i].double().cpu()
                want_b = torch.full_like(got, SENTINEL) if n in nograd else ref_b[n]
                assert torch.equal(got, want_b), (n + " (buffer)", k, float((got - want_b).abs().max()))
    if skip:
        assert torch.equal(dict(params)[skipped].detach().double().cpu(), start[skipped])


# ---------------------------------------------------------------------------------------
# a one-group table (1, wd) without the Nesterov term is gm_group_sumsq_lr, bit for bit
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu,wd", [(0.9, 5e-4), (0.0, 5e-4), (0.0, 0.0)], ids=["momentum", "decay", "plain"])
@pytest.mark.parametrize("which", list(SETS))
def test_degenerate_table_is_the_device_rate_entry_bit_for_bit(dev, which, mu, wd):
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    shapes, names, _, _, gate_nb = _set(which)
    g = torch.Generator().manual_seed(31)
    host = {n: torch.randn(*s, generator=g) for n, s in shapes.items()}
    sides = []
    for _ in range(2):
        params = [(n, torch.nn.Parameter(w.to(dev))) for n, w in host.items()]
        # a multistep rate that changes at pass 1: the state's advance is part of the comparison
        sides.append(dict(params=params, bufs=_buffers(dev, params) if mu else None, gate=_gate_state(dev, gate_nb),
                          state=_lr_state(dev, 0.1, "multistep", milestones=(1,), gamma=0.5),
                          gn=GroupNorms(params, *names)))
    old, new = sides
    table = _table(dev, [(1.0, wd)])
    for k in range(2):
        grads = {n: torch.randn(s, generator=g).to(dev) for n, s in shapes.items()}
        for side in sides:
            for n, p in side["params"]:
                p.grad = grads[n].clone()
        kw = dict(grad_scale=0.5, momentum=mu, gate_n=bool(gate_nb))
        want = old["gn"].sums(lr_state=old["state"], weight_decay=wd, momentum_buffers=old["bufs"], gate=old["gate"],
                              **kw)
        out = new["gn"].sums(lr_state=new["state"], pgroups=table, momentum_buffers=new["bufs"], gate=new["gate"],
                             **kw)
        assert torch.equal(out, want), k
        assert torch.equal(new["gate"], old["gate"]) and torch.equal(new["state"], old["state"]), k
        for i, ((n, a), (_, b)) in enumerate(zip(old["params"], new["params"])):
            assert torch.equal(a.detach(), b.detach()), (n, k)
            assert not torch.equal(b.detach().cpu(), host[n]), n  # (the update ran)
            if mu:
                assert torch.equal(old["bufs"][i], new["bufs"][i]), (n, k)
    from greedy_multimodal_learning_amd.lr_schedule import unpack
    st = unpack(new["state"].cpu().numpy().tobytes())
    assert st.step == 2 and st.lr == _f32(0.05)


def test_index_beyond_the_table_is_its_last_entry(dev):
    """Indices >= npgroups behave as npgroups - 1 (the table is simply shorter than the index; its
    two entries sit at the start of a larger zero-filled allocation)."""
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    g = torch.Generator().manual_seed(41)
    host = {n: (torch.randn(*s, generator=g), torch.randn(*s, generator=g)) for n, s in SHAPES8.items()}
    wild = dict(zip(SHAPES8, (0, 1, 2, 5, 15, 16, 1000, 0xFFFFFFFF)))
    results = []
    for assign in (wild, {n: min(i, 1) for n, i in wild.items()}):
        params = []
        for n, (w, gr) in host.items():
            p = torch.nn.Parameter(w.to(dev))
            p.grad = gr.to(dev)
            params.append((n, p))
        bufs = _buffers(dev, params)
        backing = torch.zeros(64, 2, device=dev)
        backing[:2] = _table(dev, [(1.0, 5e-4), (0.3, 1e-2)])
        out = GroupNorms(params, *TWO, pgroup_of=assign.__getitem__).sums(
            grad_scale=0.5, lr_state=_lr_state(dev, 0.1), pgroups=backing[:2], nesterov=True, momentum=0.9,
            momentum_buffers=bufs)
        results.append((out, [p.detach() for _, p in params], bufs))
    (o0, p0, b0), (o1, p1, b1) = results
    assert torch.equal(o0, o1)
    for n, a, b, c, d in zip(SHAPES8, p0, p1, b0, b1):
        assert torch.equal(a, b) and torch.equal(c, d), n
        assert not torch.equal(a.cpu(), host[n][0]), n  # (a zero rate from beyond the table would leave it)


def test_binding_refuses_misuse(dev):
    from greedy_multimodal_learning_amd._lib import GreedyMMLError
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    p = torch.nn.Parameter(torch.randn(8, 4, device=dev))
    p.grad = torch.randn(8, 4, device=dev)
    gn = GroupNorms([("net_view_0.w", p)], *TWO)
    state, table, buf = _lr_state(dev, 0.1), _table(dev, [(1.0, 0.0)]), [torch.zeros(8, 4, device=dev)]
    for bad in (dict(pgroups=table), dict(lr_state=state, pgroups=table, weight_decay=1e-4),
                dict(lr_state=state, pgroups=table.double()), dict(lr_state=state, pgroups=table.reshape(-1)),
                dict(lr_state=state, pgroups=table.cpu()), dict(lr_state=state, pgroups=table[:0]),
                dict(lr_state=state, pgroups=_table(dev, [(1.0, 0.0)] * 17)),
                dict(lr_state=state, pgroups=table, nesterov=True),  # (momentum 0)
                dict(lr_state=state, nesterov=True, momentum=0.9, momentum_buffers=buf),  # (no table)
                dict(lr_state=state, pgroups=table, momentum=0.9)):  # (no buffers)
        with pytest.raises(GreedyMMLError):
            gn.sums(**bad)
    before = p.detach().clone()
    gn.sums(lr_state=state, pgroups=table, nesterov=True, momentum=0.9, momentum_buffers=buf)
    assert not torch.equal(p.detach(), before)


# ---------------------------------------------------------------------------------------
# engine: the model, batch and resolution of test_gpu_sgdm.py, fp32
# ---------------------------------------------------------------------------------------
MU, WD, LR = 0.9, 5e-4, 0.05
RULES = [(("bn1.", "bn2.", "downsample.1.", ".bias"), 1.0, 0.0), (("mmtm",), 2.5, 1e-2), (("net_view_1",), 0.3, WD)]
CHANGE = (2, dict(lr_scale=0.5, weight_decay=1e-3))  # set_param_group(2, ...) before step index 2


def _batches(dev):
    g = torch.Generator(device=dev).manual_seed(5)
    xs = [torch.randn(4, 2, 3, 64, 64, device=dev, generator=g) for _ in range(3)]
    ys = [torch.randint(0, 40, (4,), device=dev, generator=g) for _ in range(3)]
    return xs, ys


def _engine(graphs, pg=None, gated=True, groups=True, nesterov=True):
    from greedy_multimodal_learning_amd.callbacks import Bias_Mitigation_Strong
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    from greedy_multimodal_learning_amd.param_groups import ParamGroups
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = MMTM_MVCNN().to(dev)
    gate = Bias_Mitigation_Strong(epsilon=2e-3, curation_windowsize=2, branchnames=["net_view_0", "net_view_1"],
                                  starting_epoch=1) if gated else None
    kw = dict(process_group=pg, dp_buckets=True) if pg is not None else {}
    st = BalancedStep(m, lr=LR, gate=gate, compute_dtype=torch.float32, graphs=graphs, device_gate=True, momentum=MU,
                      weight_decay=WD, param_groups=ParamGroups(RULES) if groups else None, nesterov=nesterov, **kw)
    assert st.device_gate == gated
    st.on_epoch_begin(1)
    return m, st


def _per_element(st, key):
    """a group value (lr or weight_decay of param_group(i)) per element of the flat buffers, float64"""
    v = torch.empty(st.flat.total, dtype=torch.float64, device=st.device)
    for p in st.model.parameters():
        off, n = st.flat.slices[p]
        v[off:off + n] = st.param_group(st.param_group_of(p))[key]
    return v


def _engine_run(graphs, steps=4, change=None, check=False, **kw):
    """`steps` steps; change: (step index, set_param_group(2, ...) arguments) applied before that
    step; check: the worst error / one-step bound of every step's update recomputed in float64 per
    group from the flat buffers."""
    m, st = _engine(graphs, **kw)
    xs, ys = _batches(st.device)
    worst = []
    for i in range(steps):
        if change is not None and i == change[0]:
            st.set_param_group(2, **change[1])
        if check:
            p0, b0 = st.flat.param.double(), st.flat_momentum.double()
            lr_g, wd = _per_element(st, "lr"), _per_element(st, "weight_decay")
        st(xs[i % 3], ys[i % 3])
        if check:  # the flat gradient survives the step (lazy_zero): the recurrence in float64
            d = wd * p0 + st.flat.grad.double()
            b1 = MU * b0 + d
            p1 = p0 - lr_g * ((MU * b1 + d) if st.nesterov else b1)
            worst.append((float(((st.flat.param.double() - p1).abs() / (1e-7 + 1e-6 * p1.abs())).max()),
                          float(((st.flat_momentum.double() - b1).abs() / (1e-7 + 1e-6 * b1.abs())).max())))
    torch.cuda.synchronize()
    return m, st, dict(param=st.flat.param.cpu(), mom=st.flat_momentum.cpu(), worst=worst, graphs=bool(st.graphs),
                       gate=st.gate_state.cpu() if st.gate_state is not None else None, ngraphs=len(st._graphs),
                       lr=st.sync_lr())


@pytest.fixture(scope="module")
def engine_runs(dev):
    _, st, eager = _engine_run(False, change=CHANGE, check=True)
    _, _, graph = _engine_run(True, change=CHANGE)
    _, _, unchanged = _engine_run(True)
    return dict(eager=eager, graph=graph, unchanged=unchanged, step=st)


def test_engine_update_per_group_in_float64(engine_runs):
    worst = engine_runs["eager"]["worst"]
    print("engine steps, max error / one-step bound (parameters, buffer):", worst)
    assert len(worst) == 4
    for wp, wb in worst:
        assert wp <= 1.0 and wb <= 1.0, worst
    st = engine_runs["step"]
    groups = {st.param_group_of(p) for p in st.model.parameters()}
    assert groups == {0, 1, 2, 3}  # every rule of RULES and the default group are exercised
    assert st.param_group(2) == {"lr_scale": 0.5, "weight_decay": pytest.approx(1e-3), "lr": pytest.approx(LR * 0.5)}
    assert st.lr == LR and engine_runs["eager"]["lr"].step == 4 and engine_runs["eager"]["lr"].kind == 0


def test_engine_graph_equals_eager_across_set_param_group_with_one_graph(engine_runs):
    e, g, u = engine_runs["eager"], engine_runs["graph"], engine_runs["unchanged"]
    assert g["graphs"] and g["ngraphs"] == 1 and not e["graphs"] and u["ngraphs"] == 1
    assert torch.equal(g["param"], e["param"]) and torch.equal(g["mom"], e["mom"])
    assert torch.equal(g["gate"], e["gate"]) and bool(e["gate"].any())
    assert not torch.equal(g["param"], u["param"])  # (the change reached the replays)


def test_engine_no_decay_norm_bias(dev):
    """A gradient of zeros: a BatchNorm weight (no decay, zero buffer) stays bit for bit, a
    convolution weight in group 0 decays by lr * (1 + mu) * wd * w."""
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    from greedy_multimodal_learning_amd.param_groups import ParamGroups
    torch.manual_seed(0)
    m = MMTM_MVCNN().to(dev)
    st = BalancedStep(m, lr=LR, compute_dtype=torch.float32, momentum=MU, nesterov=True,
                      param_groups=ParamGroups.no_decay_norm_bias(WD))
    named = dict(m.named_parameters())
    gamma, conv = named["net_view_0.layer1.0.bn1.weight"], named["net_view_0.layer1.0.conv1.weight"]
    assert st.param_group_of(gamma) == 1 and st.param_group_of(conv) == 0
    with torch.no_grad():
        gamma.uniform_(0.5, 1.5)
    assert gamma.grad is not None and not st.flat.grad.any()
    g0, c0 = gamma.detach().clone(), conv.detach().clone()
    st._sums_and_gate()
    assert torch.equal(gamma.detach(), g0)
    assert not bool((st.momentum_buffer(gamma) != 0).any())
    want = c0.double() * (1.0 - LR * (1.0 + MU) * WD)
    assert not torch.equal(conv.detach(), c0)
    _within(conv.detach().reshape(-1), want.cpu().reshape(-1), 1, "conv weight")


def test_engine_defaults_untouched(dev):
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    g = torch.Generator(device=dev).manual_seed(9)
    x = torch.randn(4, 2, 3, 64, 64, device=dev, generator=g)
    y = torch.randint(0, 40, (4,), device=dev, generator=g)
    flats = []
    for kw in ({}, dict(param_groups=None, nesterov=False)):
        torch.manual_seed(0)
        m = MMTM_MVCNN().to(dev)
        st = BalancedStep(m, lr=LR, **kw)
        assert st.pgroups is None and st.lr_state is None and st.lr_schedule is None
        for _ in range(2):
            st(x, y)
        flats.append(st.flat.param.clone())
    assert torch.equal(flats[0], flats[1])


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    _, st, out = _engine_run(True, steps=3, pg=dist.group.WORLD, gated=False)
    assert st.buckets is not None
    torch.save({k: out[k] for k in ("param", "mom", "graphs")}, os.path.join(out_dir, "dp.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_engine_one_rank_data_parallel_equals_no_group(dev, tmp_path):
    mp.start_processes(_dp_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True, start_method="spawn")
    dp = torch.load(tmp_path / "dp.pt", weights_only=True)
    _, _, e = _engine_run(True, steps=3, gated=False)
    assert dp["graphs"] and e["graphs"]
    assert torch.equal(dp["param"], e["param"]) and torch.equal(dp["mom"], e["mom"])
    assert bool(e["mom"].any())


# ---------------------------------------------------------------------------------------
# a run continued from its own checkpoint (gate off, fp32, graphs on)
# ---------------------------------------------------------------------------------------
def test_continue_from_a_checkpoint(dev):
    import copy
    xs, ys = _batches(dev)
    _, full = _engine(True, gated=False)
    for i in range(3):
        full(xs[i], ys[i])
    m, st = _engine(True, gated=False)
    for i in range(2):
        st(xs[i], ys[i])
    # the checkpoint's two entries as training_loop builds them
    opt = torch.optim.SGD(st.torch_param_groups(), lr=LR, momentum=MU, weight_decay=WD, nesterov=True)
    for p in m.parameters():
        opt.state[p]["momentum_buffer"] = st.momentum_buffer(p).detach().clone()
    ck = {"model": {k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
          "optimizer": copy.deepcopy(opt.state_dict())}
    assert len(ck["optimizer"]["param_groups"]) == 4 and len(ck["optimizer"]["state"]) == 142
    m2, st2 = _engine(True, gated=False)
    m2.load_state_dict(ck["model"])
    st2.load_optimizer_state(ck["optimizer"])
    assert torch.equal(st2.flat.param, st.flat.param) and torch.equal(st2.flat_momentum, st.flat_momentum)
    st2(xs[2], ys[2])
    torch.cuda.synchronize()
    assert torch.equal(st2.flat.param, full.flat.param)
    assert torch.equal(st2.flat_momentum, full.flat_momentum)
    # what disagrees with the engine is refused, here between two steps
    bad = copy.deepcopy(ck["optimizer"])
    bad["state"][3]["momentum_buffer"] = bad["state"][3]["momentum_buffer"].reshape(-1)[1:].clone()
    with pytest.raises(ValueError, match="shape"):
        st2.load_optimizer_state(bad)
    bad = copy.deepcopy(ck["optimizer"])
    for g in bad["param_groups"]:
        g["momentum"] = 0.8
    with pytest.raises(ValueError, match="momentum"):
        st2.load_optimizer_state(bad)
    assert torch.equal(st2.flat_momentum, full.flat_momentum)  # (a refused state copies nothing)


# ---------------------------------------------------------------------------------------
# the training entry
# ---------------------------------------------------------------------------------------
def test_training_loop_saves_the_groups_and_every_buffer(dev, tmp_path):
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    from greedy_multimodal_learning_amd.train import training_loop
    xs, ys = _batches(dev)
    loader = [(torch.arange(4 * i, 4 * i + 4), xs[i], ys[i]) for i in range(2)]
    torch.manual_seed(0)
    m = MMTM_MVCNN()
    H = training_loop(model=m, loss_function=None, metrics=[], optimizer=(LR, MU, WD), config={},
                      save_path=str(tmp_path), steps_per_epoch=2, train=loader, n_epochs=2, verbose=False,
                      fused_momentum=True, param_groups="no_decay_norm_bias", nesterov=True)
    assert len(H["loss"]) == 1
    ck = torch.load(tmp_path / "model_last_epoch.pt", weights_only=True)
    groups = ck["optimizer"]["param_groups"]
    assert [(g["weight_decay"], g["nesterov"], g["momentum"]) for g in groups] == \
        [(pytest.approx(WD), True, MU), (0.0, True, MU)]
    assert all(g["lr"] == pytest.approx(LR) for g in groups)
    norm_bias = sum(1 for n, p in m.named_parameters() if p.dim() == 1)
    assert [len(g["params"]) for g in groups] == [142 - norm_bias, norm_bias]
    order = [p for want in (False, True) for p in m.parameters() if (p.dim() == 1) == want]
    assert sorted(ck["optimizer"]["state"]) == list(range(142))
    for k, p in enumerate(order):
        b = ck["optimizer"]["state"][k]["momentum_buffer"]
        assert tuple(b.shape) == tuple(p.shape) and bool(torch.isfinite(b).all()) and bool(b.any()), k
    # and the entry continues a run: training_loop.optimizer_state_from
    torch.manual_seed(0)
    m2 = MMTM_MVCNN()
    m2.load_state_dict(ck["model"])
    training_loop(model=m2, loss_function=None, metrics=[], optimizer=(LR, MU, WD), config={}, save_path=None,
                  steps_per_epoch=0, train=loader, n_epochs=2, verbose=False, fused_momentum=True,
                  param_groups="no_decay_norm_bias", nesterov=True,
                  optimizer_state_from=str(tmp_path / "model_last_epoch.pt"))
