"""gm_group_sumsq_sgdm: the norms pass with torch.optim.SGD's momentum and weight decay.

Kernel level (GroupNorms.sums with momentum / weight_decay): parameters and momentum buffers
against torch.optim.SGD in float64 over consecutive steps, the group sums and the on-device
gate's state against the plain entry points on clones, the scalar path (buffers not congruent
with their parameters), skipped entries (no gradient), the many-group form; every element of the
update exactly on dyadic operands (test_update_is_exact_on_dyadic_operands).
Engine level (BalancedStep(momentum=, weight_decay=)): each step's update recomputed in
float64 from the flat buffers, the accessor, graph == eager, one-rank data parallel == no
group, and the defaults untouched.

Bound after step k against float64: k * (1e-7 + 1e-6 * |ref|) - the one-step bound of
test_gpu_kernels.py::test_group_sumsq_and_fused_sgd scaled by the step count."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SHAPES8 = {"net_view_0.a": (3, 5), "net_view_0.b": (40000,), "net_view_1.c": (7,),
           "net_view_1.d": (100, 333), "mmtm2.fc_squeeze.weight": (16, 32),
           "mmtm2.fc_visual.bias": (16,), "mmtm3.fc_skeleton.weight": (64, 65),
           "net_view_1.e": (1,)}
TWO = (["net_view_0", "net_view_1"], ["visual", "skeleton"])
HYPER = [(0.1, 0.9, 0.0), (0.1, 0.0, 5e-4), (0.1, 0.9, 5e-4)]
SENTINEL = 7.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _twelve():
    """the parameter set of test_gpu_kernels.py::test_group_sumsq_twelve_branches (24 groups)"""
    V = 12
    shapes = {}
    for i in range(V):
        shapes[f"net_view_{i}.conv.weight"] = (64, 3, 3, 3)
        shapes[f"net_view_{i}.bn.bias"] = (64,)
        shapes[f"mmtm4.fc_excite.{i}.weight"] = (32, 16)
    shapes["mmtm4.fc_squeeze.weight"] = (16, 384)
    return shapes, ([f"net_view_{i}" for i in range(V)], [f"fc_excite.{i}." for i in range(V)])


def _gate_state(dev, nb=None):
    """a fresh device gate state as the engine makes it (two-branch, or N-branch with nb)"""
    from greedy_multimodal_learning_amd import _lib as L
    st = L.GateState() if nb is None else L.GateStateN()
    if nb is not None:
        st.nb = nb
    st.caring, st.window, st.eps = -1, 2, 2e-3
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).to(dev)


def _within(got, ref64, k, what):
    got = got.detach().double().cpu()
    err = (got - ref64).abs()
    bound = k * (1e-7 + 1e-6 * ref64.abs())
    worst = float((err / bound).max())
    print(f"{what}: step {k}: max error / bound = {worst:.3f}")
    assert worst <= 1.0, (what, k, worst)


def _steps(dev, shapes, names, steps, lr, mu, wd, seed, skew=False, nograd=(), gate_nb=False):
    """`steps` steps of GroupNorms.sums(grad_scale=0.5, lr, momentum, weight_decay) with a fresh
    random gradient each; after every step: parameters and buffers against torch.optim.SGD in
    float64, the sums (and the gate state, when gate_nb is not False: None = two-branch, else the
    branch count) against the plain entry points on clones of the same inputs.  skew: buffers at a
    one-float offset into their allocation (not congruent with the parameters: the scalar path).
    nograd: names without a gradient (their buffer holds a sentinel)."""
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    g = torch.Generator().manual_seed(seed)
    host = {n: torch.randn(*s, generator=g) for n, s in shapes.items()}
    params = [(n, torch.nn.Parameter(w.to(dev))) for n, w in host.items()]
    ref = [torch.nn.Parameter(w.double()) for w in host.values()]
    opt = torch.optim.SGD(ref, lr=lr, momentum=mu, weight_decay=wd)
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
    gn = GroupNorms(params, *names)
    gate = gate_ref = None
    if gate_nb is not False:
        gate, gate_ref = _gate_state(dev, gate_nb), _gate_state(dev, gate_nb)
    for k in range(1, steps + 1):
        clones = []
        for (n, p), r in zip(params, ref):
            if n in nograd:
                p.grad, r.grad = None, None
            else:
                gr = torch.randn(p.shape, generator=g)
                p.grad = gr.to(dev)
                r.grad = gr.double() * 0.5
            c = torch.nn.Parameter(p.detach().clone())
            c.grad = None if p.grad is None else p.grad.clone()
            clones.append((n, c))
        # the plain entry points on clones of the same inputs (lr 0: sums only)
        want = GroupNorms(clones, *names).sums(grad_scale=0.5, lr=0.0, gate=gate_ref, gate_n=bool(gate_nb))
        out = gn.sums(grad_scale=0.5, lr=lr, momentum=mu, weight_decay=wd, momentum_buffers=bufs, gate=gate,
                      gate_n=bool(gate_nb))
        opt.step()
        if not skew:  # (congruent buffers: the plain pass's accumulation order, bit for bit)
            assert torch.equal(out, want), (k, (out - want).abs().max())
        else:  # another order: each within test_group_sumsq_and_fused_sgd's 1e-6 of the exact sums
            torch.testing.assert_close(out, want, rtol=2e-6, atol=0)
        if gate is not None:
            assert torch.equal(gate, gate_ref), k
        for i, ((n, p), r) in enumerate(zip(params, ref)):
            if n in nograd:
                assert torch.equal(p.detach().cpu(), host[n]), n
                if bufs is not None:
                    assert bool((bufs[i] == SENTINEL).all()), n
                continue
            _within(p, r.detach(), k, n)
            if bufs is not None:
                _within(bufs[i], opt.state[r]["momentum_buffer"], k, n + " (buffer)")
    return params, bufs


@pytest.mark.parametrize("lr,mu,wd", HYPER)
def test_three_steps_match_float64_sgd_and_sums_unchanged(dev, lr, mu, wd):
    _steps(dev, SHAPES8, TWO, 3, lr, mu, wd, seed=1)


def test_two_branch_gate_state_matches_plain_gate_entry(dev):
    _steps(dev, SHAPES8, TWO, 3, 0.1, 0.9, 5e-4, seed=2, gate_nb=None)


def test_zero_hyper_parameters_are_the_plain_update(dev):
    """momentum = weight_decay = 0, mom = NULL: bit for bit gm_group_sumsq at the same lr."""
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    g = torch.Generator().manual_seed(4)
    sets = []
    host = {n: (torch.randn(*s, generator=g), torch.randn(*s, generator=g)) for n, s in SHAPES8.items()}
    for _ in range(2):
        ps = []
        for n, (w, gr) in host.items():
            p = torch.nn.Parameter(w.to(dev))
            p.grad = gr.to(dev)
            ps.append((n, p))
        sets.append(ps)
    plain, new = GroupNorms(sets[0], *TWO), GroupNorms(sets[1], *TWO)
    want = plain.sums(grad_scale=0.5, lr=0.1)
    new._build()
    out = torch.empty_like(want)
    L.check(L.load().gm_group_sumsq_sgdm(new._table.data_ptr(), None, len(new.params), new.total, new.ngroups, 0.5,
                                         0.1, 0.0, 0.0, out.data_ptr(), new._scratch.data_ptr(),
                                         new._scratch.numel(), None, 0, L.stream_of(dev)), "gm_group_sumsq_sgdm")
    assert torch.equal(out, want)
    for (n, a), (_, b) in zip(sets[0], sets[1]):
        assert torch.equal(a.detach(), b.detach()), n
        assert not torch.equal(b.detach().cpu(), host[n][0]), n  # (the update ran)


def test_scalar_path_and_skipped_entries(dev):
    _steps(dev, SHAPES8, TWO, 3, 0.1, 0.9, 5e-4, seed=5, skew=True, nograd=("net_view_1.d",))


def test_skipped_entry_on_the_vector_path(dev):
    _steps(dev, SHAPES8, TWO, 2, 0.1, 0.9, 5e-4, seed=6, nograd=("net_view_0.b", "net_view_1.e"))


def test_zero_gradient_still_decays_and_coasts(dev):
    """A gradient that is present but all zeros: the parameter decays and moves by its momentum."""
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    p = torch.nn.Parameter(torch.full((1000,), 2.0, device=dev))
    p.grad = torch.zeros(1000, device=dev)
    b = torch.full((1000,), 0.5, device=dev)
    GroupNorms([("net_view_0.w", p)], *TWO).sums(lr=0.1, momentum=0.9, weight_decay=0.25, momentum_buffers=[b])
    ref_b = 0.9 * 0.5 + 0.25 * 2.0
    _within(b, torch.full((1000,), ref_b, dtype=torch.float64), 1, "buffer")
    _within(p, torch.full((1000,), 2.0 - 0.1 * ref_b, dtype=torch.float64), 1, "parameter")


def test_many_group_form(dev):
    shapes, names = _twelve()
    _steps(dev, shapes, names, 2, 0.1, 0.9, 5e-4, seed=3, gate_nb=12)


def test_many_group_form_without_momentum(dev):
    shapes, names = _twelve()
    _steps(dev, shapes, names, 2, 0.1, 0.0, 5e-4, seed=7)


# ---------------------------------------------------------------------------------------
# every element of the update, exactly (the contract of tests/exactint.py): integer parameters
# and gradients in [-64, 64], zero buffers and dyadic hyper-parameters make g' = 0.5 g,
# d = wd w + g', b' = mu b + d and w' = w - 0.125 b' dyadic rationals that fp32 holds exactly
# for three steps, so any fma order or contraction gives the float64 recurrence's value.
# ---------------------------------------------------------------------------------------
EXACT_SCALE, EXACT_LR, EXACT_STEPS = 0.5, 0.125, 3
EXACT_SETS = {"eight": lambda: (SHAPES8, TWO, "net_view_1.d"),
              "twelve": lambda: _twelve() + ("net_view_3.conv.weight",)}
# (mu, wd, buffers one float off congruence, one entry without a gradient); (0, 0): the plain entry
EXACT_FORMS = {"momentum": (0.5, 0.25, False, False), "decay": (0.0, 0.25, False, False),
               "plain": (0.0, 0.0, False, False), "momentum-scalar-path": (0.5, 0.25, True, False),
               "momentum-skipped-entry": (0.5, 0.25, False, True)}


def _exact_reference(shapes, mu, wd, nograd, seed):
    """Start values, per-step gradients and the float64 recurrence's parameters and buffers after
    each step, with every intermediate checked to round-trip through float32."""
    def holds(t):
        assert torch.equal(t.float().double(), t), "the operands do not keep the recurrence exact in fp32"
        return t
    g = torch.Generator().manual_seed(seed)
    w = {n: torch.randint(-64, 65, s, generator=g).double() for n, s in shapes.items()}
    b = {n: torch.zeros(s, dtype=torch.float64) for n, s in shapes.items()}
    start, grads, after = {n: t.clone() for n, t in w.items()}, [], []
    for _ in range(EXACT_STEPS):
        gr = {n: torch.randint(-64, 65, s, generator=g).double() for n, s in shapes.items() if n not in nograd}
        for n, t in gr.items():
            d = holds(wd * w[n] + holds(EXACT_SCALE * t))
            b[n] = holds(mu * b[n] + d)
            w[n] = holds(w[n] - EXACT_LR * b[n])
        grads.append(gr)
        after.append(({n: t.clone() for n, t in w.items()}, {n: t.clone() for n, t in b.items()}))
    return start, grads, after


@pytest.mark.parametrize("form", EXACT_FORMS)
@pytest.mark.parametrize("which", EXACT_SETS)
def test_update_is_exact_on_dyadic_operands(dev, which, form):
    """Parameters and buffers torch.equal the float64 recurrence after each of three steps; at
    step 1 (integer w, per-thread partial sums below 2^24) the returned sums equal the host's
    float64 sums exactly, from step 2 on the plain entry's on clones as in _steps."""
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    shapes, names, skipped = EXACT_SETS[which]()
    mu, wd, skew, skip = EXACT_FORMS[form]
    nograd = (skipped,) if skip else ()
    start, grads, after = _exact_reference(shapes, mu, wd, nograd, seed=11)  # (asserts before any launch)
    params = [(n, torch.nn.Parameter(w.float().to(dev))) for n, w in start.items()]
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
    gn = GroupNorms(params, *names)
    for k in range(1, EXACT_STEPS + 1):
        clones = []
        for n, p in params:
            p.grad = grads[k - 1][n].float().to(dev) if n in grads[k - 1] else None
            c = torch.nn.Parameter(p.detach().clone())
            c.grad = None if p.grad is None else p.grad.clone()
            clones.append((n, c))
        want = GroupNorms(clones, *names).sums(grad_scale=EXACT_SCALE, lr=0.0)
        out = gn.sums(grad_scale=EXACT_SCALE, lr=EXACT_LR, momentum=mu, weight_decay=wd, momentum_buffers=bufs)
        if k == 1:
            host = torch.zeros(2 * gn.ngroups, dtype=torch.float64)
            for (n, _), m in zip(params, gn.masks):
                sw = float((start[n] ** 2).sum())
                sg = float(((EXACT_SCALE * grads[0][n]) ** 2).sum()) if n in grads[0] else 0.0
                for j in range(gn.ngroups):
                    if (m >> j) & 1:
                        host[2 * j] += sw
                        host[2 * j + 1] += sg
            assert torch.equal(out.cpu(), host), (out.cpu() - host).abs().max()
        elif not skew:
            assert torch.equal(out, want), (k, (out - want).abs().max())
        else:
            torch.testing.assert_close(out, want, rtol=2e-6, atol=0)
        ref_w, ref_b = after[k - 1]
        for i, (n, p) in enumerate(params):
            got = p.detach().double().cpu()
            assert torch.equal(got, ref_w[n]), (n, k, float((got - ref_w[n]).abs().max()))
            if bufs is not None:
                got = bufs[i].double().cpu()
                want_b = torch.full_like(got, SENTINEL) if n in nograd else ref_b[n]
                assert torch.equal(got, want_b), (n + " (buffer)", k, float((got - want_b).abs().max()))


def test_binding_refuses_misplaced_buffers(dev):
    from greedy_multimodal_learning_amd._lib import GreedyMMLError
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    p = torch.nn.Parameter(torch.randn(8, 4, device=dev))
    p.grad = torch.randn(8, 4, device=dev)
    gn = GroupNorms([("net_view_0.w", p)], *TWO)
    for bad in ([torch.zeros(4, 8, device=dev)], [torch.zeros(8, 4, device=dev, dtype=torch.float64)],
                [torch.zeros(8, 8, device=dev)[:, ::2]], [None], []):
        with pytest.raises(GreedyMMLError):
            gn.sums(lr=0.1, momentum=0.9, momentum_buffers=bad)
    with pytest.raises(GreedyMMLError):  # a momentum needs its buffers (the C entry's check)
        gn.sums(lr=0.1, momentum=0.9)
    with pytest.raises(GreedyMMLError):  # and buffers need a momentum
        gn.sums(lr=0.1, weight_decay=0.1, momentum_buffers=[torch.zeros(8, 4, device=dev)])


# ---------------------------------------------------------------------------------------
# engine: the model, batch and resolution of test_gpu_graphs.py, fp32
# ---------------------------------------------------------------------------------------
MU, WD, LR = 0.9, 5e-4, 0.05


def _engine_run(graphs, steps=3, pg=None, check=False, gated=True):
    """`steps` steps of BalancedStep(momentum, weight_decay), gated: with the on-device gate;
    returns the flat parameters, the flat momentum buffer and the gate state (host copies), with
    check the worst error / bound of every step's update recomputed in float64 from the flat
    buffers."""
    from greedy_multimodal_learning_amd.callbacks import Bias_Mitigation_Strong
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = MMTM_MVCNN().to(dev)
    gate = Bias_Mitigation_Strong(epsilon=2e-3, curation_windowsize=2, branchnames=["net_view_0", "net_view_1"],
                                  starting_epoch=1) if gated else None
    kw = dict(process_group=pg, dp_buckets=True) if pg is not None else {}
    st = BalancedStep(m, lr=LR, gate=gate, compute_dtype=torch.float32, graphs=graphs, device_gate=True,
                      momentum=MU, weight_decay=WD, **kw)
    assert st.device_gate == gated
    st.on_epoch_begin(1)
    g = torch.Generator(device=dev).manual_seed(5)
    xs = [torch.randn(4, 2, 3, 64, 64, device=dev, generator=g) for _ in range(3)]
    ys = [torch.randint(0, 40, (4,), device=dev, generator=g) for _ in range(3)]
    worst = []
    for i in range(steps):
        if check:
            p0, b0 = st.flat.param.double(), st.flat_momentum.double()
        st(xs[i % 3], ys[i % 3])
        if check:
            # the flat gradient survives the step (lazy_zero): the recurrence in float64
            b1 = MU * b0 + (WD * p0 + st.flat.grad.double())
            p1 = p0 - LR * b1
            worst.append((float(((st.flat.param.double() - p1).abs() / (1e-7 + 1e-6 * p1.abs())).max()),
                          float(((st.flat_momentum.double() - b1).abs() / (1e-7 + 1e-6 * b1.abs())).max())))
    torch.cuda.synchronize()
    out = dict(param=st.flat.param.cpu(), mom=st.flat_momentum.cpu(), worst=worst, graphs=bool(st.graphs),
               gate=st.gate_state.cpu() if gated else None, ngraphs=len(st._graphs))
    return m, st, out


@pytest.fixture(scope="module")
def engine_runs(dev):
    m, st, eager = _engine_run(False, check=True)
    views = {}
    named = dict(m.named_parameters())
    for name in ("net_view_0.layer2.0.conv1.weight", "net_view_1.bn1.weight", "net_view_0.fc.bias"):
        p = named[name]
        views[name] = (p, st.momentum_buffer(p), st.flat.slices[p])
    _, _, graph = _engine_run(True)
    return dict(eager=eager, graph=graph, views=views, step=st)


def test_engine_update_consistency(engine_runs):
    """Every step's parameters and buffer from the step's own flat gradient, in float64: pins the
    buffer <-> parameter pairing and the channels-last layout without trunk rounding noise."""
    worst = engine_runs["eager"]["worst"]
    print("engine steps, max error / one-step bound (parameters, buffer):", worst)
    assert len(worst) == 3
    for wp, wb in worst:
        assert wp <= 1.0 and wb <= 1.0, worst
    assert bool(engine_runs["eager"]["mom"].any())


def test_engine_momentum_buffer_accessor(engine_runs):
    st = engine_runs["step"]
    for name, (p, b, (off, n)) in engine_runs["views"].items():
        assert b.shape == p.shape and b.stride() == p.stride(), name
        assert b.data_ptr() == st.flat_momentum.data_ptr() + 4 * off, name
        assert p.data_ptr() == st.flat.param.data_ptr() + 4 * off, name
    p, b, _ = engine_runs["views"]["net_view_0.layer2.0.conv1.weight"]
    assert p.dim() == 4 and not p.is_contiguous() and p.is_contiguous(memory_format=torch.channels_last)


def test_engine_graph_steps_equal_eager_steps(engine_runs):
    e, g = engine_runs["eager"], engine_runs["graph"]
    assert g["graphs"] and g["ngraphs"] == 1 and not e["graphs"]
    assert torch.equal(g["param"], e["param"])
    assert torch.equal(g["mom"], e["mom"])


def test_engine_gate_state_graph_equals_eager(engine_runs):
    e, g = engine_runs["eager"], engine_runs["graph"]
    assert torch.equal(g["gate"], e["gate"])
    assert bool(e["gate"].any())


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    _, st, out = _engine_run(True, pg=dist.group.WORLD, gated=False)
    assert st.buckets is not None
    torch.save({k: out[k] for k in ("param", "mom", "graphs")}, os.path.join(out_dir, "dp.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_engine_one_rank_data_parallel_equals_no_group(dev, tmp_path):
    """A one-rank group with dp_buckets=True (bucketed all-reduce, the pass behind each replay with
    grad_scale = 1 / world) against the same run without a group, no gate.  One rank's all-reduce
    is the identity and every kernel is deterministic, so the criterion is the one
    test_gpu_dp_parity.py applies to two ranks' all-reduced results: identical."""
    mp.start_processes(_dp_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True, start_method="spawn")
    dp = torch.load(tmp_path / "dp.pt", weights_only=True)
    _, _, e = _engine_run(True, gated=False)
    assert dp["graphs"] and e["graphs"]
    assert torch.equal(dp["param"], e["param"])
    assert torch.equal(dp["mom"], e["mom"])
    assert bool(e["mom"].any())


def test_engine_defaults_untouched(dev):
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    g = torch.Generator(device=dev).manual_seed(9)
    x = torch.randn(4, 2, 3, 64, 64, device=dev, generator=g)
    y = torch.randint(0, 40, (4,), device=dev, generator=g)
    flats = []
    for kw in ({}, dict(momentum=0.0, weight_decay=0.0)):
        torch.manual_seed(0)
        m = MMTM_MVCNN().to(dev)
        st = BalancedStep(m, lr=LR, **kw)
        assert st.flat_momentum is None and st.momentum_buffer(next(m.parameters())) is None
        for _ in range(2):
            st(x, y)
        flats.append(st.flat.param.clone())
    assert torch.equal(flats[0], flats[1])
