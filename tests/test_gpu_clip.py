"""gm_group_sumsq_clip: global-norm gradient clipping (torch's clip_grad_norm_) and the non-finite
step skip in the norms pass, decided on the device.

Kernel level (GroupNorms.sums(lr_state=, clip_state=)), on test_gpu_sgdm.py's parameter sets, for
the plain, decay, momentum and Nesterov-with-groups forms: an inactive clip against the existing
entry points bit for bit; an active clip against the existing entry points on pre-scaled gradients
bit for bit, the sums and the gate against the unclipped ones; three steps against
clip_grad_norm_ + torch.optim.SGD in float64; inf and NaN gradients with and without the skip;
max_norm rewritten on the device; the binding's refusals.
Engine level (BalancedStep(clip_grad_norm=, skip_nonfinite_steps=)): the update recomputed in
float64 from the flat buffers, graph == eager with one graph across a change of the bound, the
gate blind to the clip, one-rank data parallel, the defaults untouched, the training entry.

Bound after step k against float64: k * (1e-7 + 1e-6 * |ref|), test_gpu_sgdm.py's.  The clip adds
two fp32 roundings to the gradient (the coefficient's and the product's, 2^-23 relative together),
which the rate (<= 0.25 here) scales far below that bound."""
import ctypes
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_sgdm import SENTINEL, SHAPES8, TWO, _free_port, _gate_state, _twelve, _within
from test_gpu_sgd_groups import ASSIGN8, TABLE, _buffers, _f32, _lr_state, _table

pytestmark = pytest.mark.gpu

INF = float("inf")
SETS = {"eight": lambda: (SHAPES8, TWO, ASSIGN8, "net_view_1.d", None),
        "twelve": lambda: _twelve() + (None, "net_view_3.conv.weight", 12)}
# randn gradients at grad_scale 0.5: the norm is ~139.7 on the eight-tensor set (78 011 elements)
# and ~91.9 on the twelve-branch one (33 792), so these bounds clip every step
ACTIVE = {"eight": 100.0, "twelve": 50.0}
# (momentum, weight decay, group table, nesterov); without a table the existing entry is
# gm_group_sumsq_lr, with one gm_group_sumsq_pg
FORMS = {"plain": (0.0, 0.0, None, False), "decay": (0.0, 5e-4, None, False), "momentum": (0.9, 5e-4, None, False),
         "nesterov-groups": (0.9, 0.0, TABLE, True)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _set(which):
    shapes, names, assign, skipped, gate_nb = SETS[which]()
    if assign is None:
        assign = {n: i % 3 for i, n in enumerate(shapes)}
    return shapes, names, assign, skipped, gate_nb


def _clip_state(dev, max_norm=INF, skip=False, eps=1e-6):
    from greedy_multimodal_learning_amd import _lib as L
    return torch.frombuffer(bytearray(L.clip_state_bytes(max_norm, eps, skip)), dtype=torch.uint8).to(dev)


def _decode(clip):
    from greedy_multimodal_learning_amd import _lib as L
    return L.ClipState.from_buffer_copy(clip.cpu().numpy().tobytes())


def _lr_of(state):
    from greedy_multimodal_learning_amd.lr_schedule import unpack
    return unpack(state.cpu().numpy().tobytes())


class Side:
    """One copy of a parameter set with everything a pass mutates: parameters, buffers, gate state,
    lr state and (clip=...) a clip state.  pass_(grads, grad_scale) sets the gradients and runs
    GroupNorms.sums through gm_group_sumsq_clip (with a clip state) or the existing entry of the
    form."""

    def __init__(self, dev, which, form, host, clip=None, skew=False, nograd=(), lr=None):
        from greedy_multimodal_learning_amd.callbacks import GroupNorms
        shapes, names, assign, _, gate_nb = _set(which)
        self.mu, self.wd, table, self.nesterov = FORMS[form]
        self.params = [(n, torch.nn.Parameter(host[n].to(dev))) for n in shapes]
        self.bufs = _buffers(dev, self.params, skew, nograd) if self.mu else None
        self.gate, self.gate_n = _gate_state(dev, gate_nb), bool(gate_nb)
        # a multistep rate that changes at pass 1: the state's advance and the clip's snapshot of
        # the rate are part of every comparison
        self.state = lr if lr is not None else _lr_state(dev, 0.1, "multistep", milestones=(1,), gamma=0.5)
        self.table = None if table is None else _table(dev, table)
        self.clip = clip
        self.nograd = set(nograd)
        self.gn = GroupNorms(self.params, *names, pgroup_of=assign.__getitem__)

    def pass_(self, grads, grad_scale):
        for n, p in self.params:
            p.grad = None if n in self.nograd else grads[n].clone()
        kw = dict(grad_scale=grad_scale, lr_state=self.state, momentum=self.mu, momentum_buffers=self.bufs,
                  gate=self.gate, gate_n=self.gate_n)
        if self.table is not None:
            kw.update(pgroups=self.table, nesterov=self.nesterov)
        else:
            kw.update(weight_decay=self.wd)
        if self.clip is not None:
            kw.update(clip_state=self.clip)
        return self.gn.sums(**kw)

    def snapshot(self):
        return ([p.detach().clone() for _, p in self.params], None if self.bufs is None else [b.clone() for b in self.bufs],
                self.gate.clone())


def _host(which, seed):
    shapes = _set(which)[0]
    g = torch.Generator().manual_seed(seed)
    return g, {n: torch.randn(*s, generator=g) for n, s in shapes.items()}


def _grads(dev, which, g):
    return {n: torch.randn(s, generator=g).to(dev) for n, s in _set(which)[0].items()}


def _same(a, b, what):
    """parameters, buffers, gate and lr state of two sides, bit for bit"""
    for (n, p), (_, q) in zip(a.params, b.params):
        assert torch.equal(p.detach(), q.detach()), (what, n)
    if a.bufs is not None:
        for (n, _), x, y in zip(a.params, a.bufs, b.bufs):
            assert torch.equal(x, y), (what, n + " (buffer)")
    assert torch.equal(a.gate, b.gate), (what, "gate")


# ---------------------------------------------------------------------------------------
# 1. an inactive clip changes nothing
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [INF, 1e4], ids=["inf", "1e4"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("which", list(SETS))
def test_inactive_clip_is_the_existing_entry_bit_for_bit(dev, which, form, max_norm):
    g, host = _host(which, 51)
    old = Side(dev, which, form, host)
    new = Side(dev, which, form, host, clip=_clip_state(dev, max_norm))
    for k in range(2):
        grads = _grads(dev, which, g)
        rate = _lr_of(new.state).lr
        want, out = old.pass_(grads, 0.5), new.pass_(grads, 0.5)
        assert torch.equal(out, want), k
        _same(new, old, k)
        assert torch.equal(new.state, old.state), k
        c = _decode(new.clip)
        assert c.coef == 1.0 and c.lr == rate and c.skipped_last == 0, k
        if k == 0:  # the clip keeps the rate its pass used; the state has moved on
            assert c.lr == _f32(0.1) and _lr_of(new.state).lr == _f32(0.05)
        assert not torch.equal(new.params[1][1].detach().cpu(), host[new.params[1][0]])  # (the update ran)
    c, lr = _decode(new.clip), _lr_of(new.state)
    assert (c.steps, c.clipped, c.skipped) == (2, 0, 0)
    assert lr.step == 2 and lr.lr == _f32(0.05) == c.lr
    assert bool(new.gate.any())


# ---------------------------------------------------------------------------------------
# 2. an active clip is the existing update on pre-scaled gradients, bit for bit
# ---------------------------------------------------------------------------------------
ACTIVE_CASES = [(f, "aligned") for f in FORMS] + [(f, v) for f in ("momentum", "nesterov-groups")
                                                  for v in ("scalar-path", "skipped-entry")]


@pytest.mark.parametrize("form,variant", ACTIVE_CASES, ids=[f"{f}-{v}" for f, v in ACTIVE_CASES])
@pytest.mark.parametrize("which", list(SETS))
def test_active_clip_is_the_existing_update_on_prescaled_gradients(dev, which, form, variant):
    from greedy_multimodal_learning_amd import _lib as L
    skipped = _set(which)[3]
    kw = dict(skew=variant == "scalar-path", nograd=(skipped,) if variant == "skipped-entry" else ())
    g, host = _host(which, 52)
    grads = _grads(dev, which, g)
    new = Side(dev, which, form, host, clip=_clip_state(dev, ACTIVE[which]), **kw)
    plain = Side(dev, which, form, host, **kw)      # the unclipped entry: its sums and gate
    scaled = Side(dev, which, form, host, **kw)     # the existing entry on (g * 0.5) * coef, grad_scale 1
    out = new.pass_(grads, 0.5)
    c = _decode(new.clip)
    assert 0.0 < c.coef < 1.0 and (c.steps, c.clipped, c.skipped, c.skipped_last) == (1, 1, 0, 0)
    coef = torch.tensor(c.coef, dtype=torch.float32, device=dev)
    want_out = plain.pass_(grads, 0.5)
    scaled.pass_({n: (t * 0.5) * coef for n, t in grads.items()}, 1.0)
    for (n, p), (_, q) in zip(new.params, scaled.params):
        assert torch.equal(p.detach(), q.detach()), n
        assert (n in new.nograd) == torch.equal(p.detach().cpu(), host[n]), n
    if new.bufs is not None:
        for (n, _), x, y in zip(new.params, new.bufs, scaled.bufs):
            assert torch.equal(x, y), n + " (buffer)"
            if n in new.nograd:
                assert bool((x == SENTINEL).all()), n
    # the sums and the gate see the unclipped gradient
    assert torch.equal(out, want_out), (out - want_out).abs().max()
    assert torch.equal(new.gate, plain.gate) and bool(new.gate.any())
    assert torch.equal(new.state, plain.state)
    # the state's own numbers: coef is the rule of total_sq, total_sq the float64 sum
    assert L.clip_coef(c.total_sq, c) == c.coef
    T = sum(float(((t.double().cpu() * 0.5) ** 2).sum()) for n, t in grads.items() if n not in new.nograd)
    assert abs(c.total_sq - T) <= 2e-6 * T, (c.total_sq, T)
    rule = ACTIVE[which] / (math.sqrt(T) + 1e-6)
    assert rule < 1.0 and abs(c.coef - rule) <= 2e-6 * rule, (c.coef, rule)


# ---------------------------------------------------------------------------------------
# 3. three steps against clip_grad_norm_ + torch.optim.SGD with real param groups in float64
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nesterov", [False, True], ids=["momentum", "nesterov"])
@pytest.mark.parametrize("which", list(SETS))
def test_three_steps_match_float64_clip_grad_norm_and_sgd(dev, which, nesterov):
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    shapes, names, assign, _, gate_nb = _set(which)
    lr, mu, max_norm = 0.1, 0.9, ACTIVE[which]
    g, host = _host(which, 53)
    steps = [{n: torch.randn(s, generator=g) for n, s in shapes.items()} for _ in range(3)]
    # the reference first, whole: it must clip before anything is launched
    ref = {n: torch.nn.Parameter(w.double()) for n, w in host.items()}
    opt = torch.optim.SGD([{"params": [ref[n] for n in shapes if assign[n] == i], "lr": _f32(lr) * _f32(s),
                            "weight_decay": wd} for i, (s, wd) in enumerate(TABLE)],
                          lr=lr, momentum=mu, nesterov=nesterov)
    after, norms = [], []
    for gr in steps:
        for n in shapes:
            ref[n].grad = gr[n].double() * 0.5
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(ref.values()), max_norm)))
        opt.step()
        after.append(({n: p.detach().clone() for n, p in ref.items()},
                      {n: opt.state[p]["momentum_buffer"].clone() for n, p in ref.items()}))
    assert sum(nm > max_norm for nm in norms) >= 1, norms
    params = [(n, torch.nn.Parameter(w.to(dev))) for n, w in host.items()]
    bufs = _buffers(dev, params)
    gn = GroupNorms(params, *names, pgroup_of=assign.__getitem__)
    state, table, clip = _lr_state(dev, lr), _table(dev, TABLE), _clip_state(dev, max_norm)
    gate = _gate_state(dev, gate_nb)
    for k in range(1, 4):
        for n, p in params:
            p.grad = steps[k - 1][n].to(dev)
        gn.sums(grad_scale=0.5, lr_state=state, pgroups=table, nesterov=nesterov, momentum=mu, momentum_buffers=bufs,
                gate=gate, gate_n=bool(gate_nb), clip_state=clip)
        c = _decode(clip)
        assert abs(math.sqrt(c.total_sq) - norms[k - 1]) <= 2e-6 * norms[k - 1], k
        ref_w, ref_b = after[k - 1]
        for i, (n, p) in enumerate(params):
            _within(p, ref_w[n], k, n)
            _within(bufs[i], ref_b[n], k, n + " (buffer)")
    c = _decode(clip)
    assert c.steps == 3 and c.clipped == sum(nm > max_norm for nm in norms) and c.skipped == 0


# ---------------------------------------------------------------------------------------
# 4. non-finite gradients: ordinary floating-point values in ordinary buffers
# ---------------------------------------------------------------------------------------
def _poison(grads, name, value):
    out = {n: t.clone() for n, t in grads.items()}
    flat = out[name].view(-1)
    flat[flat.numel() // 2] = value  # the middle of a tensor in the middle of a chunk
    return out


@pytest.mark.parametrize("value", [INF, float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("which", list(SETS))
def test_nonfinite_step_is_skipped(dev, which, value):
    victim = _set(which)[3]
    g, host = _host(which, 54)
    s = Side(dev, which, "nesterov-groups", host, clip=_clip_state(dev, ACTIVE[which], skip=True))
    s.pass_(_grads(dev, which, g), 0.5)
    p1, b1, gate1 = s.snapshot()
    assert bool(gate1.any())
    out = s.pass_(_poison(_grads(dev, which, g), victim, value), 0.5)
    p2, b2, gate2 = s.snapshot()
    for i, (n, _) in enumerate(s.params):
        assert torch.equal(p2[i], p1[i]) and torch.equal(b2[i], b1[i]), n
    assert torch.equal(gate2, gate1)
    c = _decode(s.clip)
    assert _lr_of(s.state).step == 2  # the schedule advances on a skipped step too
    assert (c.steps, c.skipped, c.skipped_last, c.clipped) == (2, 1, 1, 1)
    assert not math.isfinite(c.total_sq) and (math.isnan(c.total_sq) if value != value else c.total_sq == INF)
    assert not bool(torch.isfinite(out).all())  # out carries the non-finite sum
    s.pass_(_grads(dev, which, g), 0.5)
    p3, b3, gate3 = s.snapshot()
    for i, (n, _) in enumerate(s.params):
        assert not torch.equal(p3[i], p2[i]) and bool(torch.isfinite(p3[i]).all()), n
        assert bool(torch.isfinite(b3[i]).all()), n
    c = _decode(s.clip)
    assert (c.steps, c.skipped, c.skipped_last, c.clipped) == (3, 1, 0, 2)
    assert not torch.equal(gate3, gate2) and _lr_of(s.state).step == 3


@pytest.mark.parametrize("form", ["momentum", "nesterov-groups"])
@pytest.mark.parametrize("which", list(SETS))
def test_nonfinite_step_without_the_skip(dev, which, form):
    """T = NaN: coef NaN, as torch.clamp keeps it.  T = inf: coef 0 - a parameter whose gradient was
    finite moves by decay and momentum alone, as the existing entry moves it on zero gradients."""
    victim = _set(which)[3]
    g, host = _host(which, 55)
    first, second = _grads(dev, which, g), _grads(dev, which, g)
    # (a bound far above any norm here: the first pass is the existing entry's, test 1)
    a = Side(dev, which, form, host, clip=_clip_state(dev, 1e4, skip=False))
    a.pass_(first, 0.5)
    a.pass_(_poison(second, victim, float("nan")), 0.5)
    c = _decode(a.clip)
    assert math.isnan(c.total_sq) and math.isnan(c.coef) and (c.skipped, c.skipped_last) == (0, 0)
    a = Side(dev, which, form, host, clip=_clip_state(dev, 1e4, skip=False))
    b = Side(dev, which, form, host)
    a.pass_(first, 0.5)
    b.pass_(first, 0.5)
    _same(a, b, "first pass")
    a.pass_(_poison(second, victim, INF), 0.5)
    b.pass_({n: torch.zeros_like(t) for n, t in second.items()}, 0.5)
    c = _decode(a.clip)
    assert c.total_sq == INF and c.coef == 0.0 and (c.steps, c.clipped, c.skipped, c.skipped_last) == (2, 1, 0, 0)
    for i, ((n, p), (_, q)) in enumerate(zip(a.params, b.params)):
        if n == victim:
            continue  # (inf * 0: its own element is NaN)
        assert torch.equal(p.detach(), q.detach()), n
        assert torch.equal(a.bufs[i], b.bufs[i]), n + " (buffer)"
        assert not torch.equal(p.detach().cpu(), host[n]), n


# ---------------------------------------------------------------------------------------
# 5. max_norm rewritten on the device between two passes
# ---------------------------------------------------------------------------------------
def test_max_norm_rewritten_between_passes(dev):
    from greedy_multimodal_learning_amd import _lib as L
    g, host = _host("eight", 56)
    s = Side(dev, "eight", "momentum", host, clip=_clip_state(dev, 100.0))
    s.pass_(_grads(dev, "eight", g), 0.5)
    c1 = _decode(s.clip)
    s.clip[:4].view(torch.float32).fill_(30.0)  # a stream-ordered write, no new state
    s.pass_(_grads(dev, "eight", g), 0.5)
    c2 = _decode(s.clip)
    assert c1.max_norm == 100.0 and c2.max_norm == 30.0
    assert c1.coef == L.clip_coef(c1.total_sq, c1) and c2.coef == L.clip_coef(c2.total_sq, c2)
    assert 0.6 < c1.coef < 0.8 and 0.18 < c2.coef < 0.25  # 100 / ~139.7, 30 / ~139.7
    assert c2.coef != L.clip_coef(c2.total_sq, c1) and c2.clipped == 2


# ---------------------------------------------------------------------------------------
# 6. the binding refuses misuse
# ---------------------------------------------------------------------------------------
def test_binding_refuses_misuse(dev):
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    p = torch.nn.Parameter(torch.randn(8, 4, device=dev))
    p.grad = torch.randn(8, 4, device=dev)
    gn = GroupNorms([("net_view_0.w", p)], *TWO)
    state, clip = _lr_state(dev, 0.1), _clip_state(dev, 1.0)
    n = ctypes.sizeof(L.ClipState)
    padded = torch.zeros(n + 8, dtype=torch.uint8, device=dev)
    padded[4:4 + n] = clip
    before = p.detach().clone()
    for bad in (dict(clip_state=clip), dict(lr_state=state, clip_state=clip.cpu()),
                dict(lr_state=state, clip_state=clip.view(torch.int8)), dict(lr_state=state, clip_state=clip[:n - 8]),
                dict(lr_state=state, clip_state=padded[4:4 + n]),
                dict(lr_state=state, clip_state=clip, nesterov=True),  # (momentum 0)
                dict(lr_state=state, clip_state=clip, momentum=0.9)):  # (no buffers)
        with pytest.raises(L.GreedyMMLError):
            gn.sums(**bad)
    assert torch.equal(p.detach(), before)
    gn.sums(lr_state=state, clip_state=clip)
    assert not torch.equal(p.detach(), before)


# ---------------------------------------------------------------------------------------
# engine: the model, batch and resolution of test_gpu_sgdm.py / test_gpu_sgd_groups.py, fp32
# ---------------------------------------------------------------------------------------
MU, WD, LR = 0.9, 5e-4, 0.05
RULES = [(("bn1.", "bn2.", "downsample.1.", ".bias"), 1.0, 0.0), (("mmtm",), 2.5, 1e-2), (("net_view_1",), 0.3, WD)]


def _batches(dev):
    g = torch.Generator(device=dev).manual_seed(5)
    xs = [torch.randn(4, 2, 3, 64, 64, device=dev, generator=g) for _ in range(3)]
    ys = [torch.randint(0, 40, (4,), device=dev, generator=g) for _ in range(3)]
    return xs, ys


def _engine(graphs, pg=None, gated=True, **kw):
    from greedy_multimodal_learning_amd.callbacks import Bias_Mitigation_Strong
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    from greedy_multimodal_learning_amd.param_groups import ParamGroups
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = MMTM_MVCNN().to(dev)
    gate = Bias_Mitigation_Strong(epsilon=2e-3, curation_windowsize=2, branchnames=["net_view_0", "net_view_1"],
                                  starting_epoch=1) if gated else None
    if pg is not None:
        kw.update(process_group=pg, dp_buckets=True)
    st = BalancedStep(m, lr=LR, gate=gate, compute_dtype=torch.float32, graphs=graphs, device_gate=True, momentum=MU,
                      weight_decay=WD, param_groups=ParamGroups(RULES), nesterov=True, **kw)
    assert st.device_gate == gated
    st.on_epoch_begin(1)
    return m, st


def _per_element(st, key):
    v = torch.empty(st.flat.total, dtype=torch.float64, device=st.device)
    for p in st.model.parameters():
        off, n = st.flat.slices[p]
        v[off:off + n] = st.param_group(st.param_group_of(p))[key]
    return v


def _engine_run(graphs, steps=4, change=None, check=False, **kw):
    """`steps` steps; change: (step index, new clip_grad_norm) set before that step; check: step 1's
    update recomputed in float64 (norm -> coef -> per-group recurrence) from the flat buffers."""
    m, st = _engine(graphs, **kw)
    xs, ys = _batches(st.device)
    first = None
    for i in range(steps):
        if change is not None and i == change[0]:
            st.clip_grad_norm = change[1]
        if check and i == 0:
            p0, b0 = st.flat.param.double(), st.flat_momentum.double()
            lr_g, wd = _per_element(st, "lr"), _per_element(st, "weight_decay")
        st(xs[i % 3], ys[i % 3])
        if i == 0:
            first = dict(gate=None if st.gate_state is None else st.gate_state.cpu(), clip=st.sync_clip())
            if check:  # the flat gradient survives the step (lazy_zero)
                g64 = st.flat.grad.double()
                T = float((g64 * g64).sum())
                coef = min(1.0, st.clip_grad_norm / (math.sqrt(T) + 1e-6))
                d = wd * p0 + g64 * coef
                b1 = MU * b0 + d
                p1 = p0 - lr_g * (MU * b1 + d)
                first.update(T=T, coef=coef,
                             worst=(float(((st.flat.param.double() - p1).abs() / (1e-7 + 1e-6 * p1.abs())).max()),
                                    float(((st.flat_momentum.double() - b1).abs() / (1e-7 + 1e-6 * b1.abs())).max())))
    torch.cuda.synchronize()
    return m, st, dict(param=st.flat.param.cpu(), mom=st.flat_momentum.cpu(), graphs=bool(st.graphs), first=first,
                       gate=st.gate_state.cpu() if st.gate_state is not None else None, ngraphs=len(st._graphs),
                       clip=st.sync_clip(), lr=st.sync_lr())


@pytest.fixture(scope="module")
def engine_runs(dev):
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    _, _, inactive = _engine_run(False, steps=3, skip_nonfinite_steps=True)
    _, _, plain = _engine_run(False, steps=3, lr_schedule=LRSchedule("held", LR))
    norm1 = math.sqrt(inactive["first"]["clip"].total_sq)
    change = (2, 0.25 * norm1)
    _, _, eager = _engine_run(False, change=change, check=True, clip_grad_norm=0.5 * norm1)
    _, _, graph = _engine_run(True, change=change, clip_grad_norm=0.5 * norm1)
    _, _, unchanged = _engine_run(True, clip_grad_norm=0.5 * norm1)
    return dict(inactive=inactive, plain=plain, eager=eager, graph=graph, unchanged=unchanged, norm1=norm1)


def test_engine_inactive_guard_is_the_plain_engine(engine_runs):
    i, p = engine_runs["inactive"], engine_runs["plain"]
    assert torch.equal(i["param"], p["param"]) and torch.equal(i["mom"], p["mom"]) and torch.equal(i["gate"], p["gate"])
    c = i["clip"]
    assert (c.steps, c.clipped, c.skipped) == (3, 0, 0) and c.coef == 1.0 and c.max_norm == INF
    assert p["clip"] is None and i["lr"].step == 3 == p["lr"].step
    assert math.isfinite(engine_runs["norm1"]) and engine_runs["norm1"] > 0


def test_engine_clipped_update_in_float64(engine_runs):
    first, norm1 = engine_runs["eager"]["first"], engine_runs["norm1"]
    print("clipped engine step 1: max error / one-step bound (parameters, buffer):", first["worst"],
          "norm", norm1, "coef", first["clip"].coef)
    assert first["worst"][0] <= 1.0 and first["worst"][1] <= 1.0, first["worst"]
    c = first["clip"]
    assert c.clipped == 1 and abs(c.total_sq - first["T"]) <= 2e-6 * first["T"]
    assert abs(c.coef - first["coef"]) <= 2e-6 * first["coef"] and abs(c.coef - 0.5) < 1e-3
    assert math.sqrt(c.total_sq) == norm1  # the same first gradient as the unclipped run's
    assert engine_runs["eager"]["clip"].clipped >= 1


def test_engine_graph_equals_eager_across_a_change_of_the_bound(engine_runs):
    e, g, u = engine_runs["eager"], engine_runs["graph"], engine_runs["unchanged"]
    assert g["graphs"] and g["ngraphs"] == 1 and not e["graphs"] and u["ngraphs"] == 1
    assert torch.equal(g["param"], e["param"]) and torch.equal(g["mom"], e["mom"])
    assert torch.equal(g["gate"], e["gate"]) and bool(e["gate"].any())
    assert bytes(g["clip"]) == bytes(e["clip"]) and g["clip"].steps == 4
    assert g["clip"].max_norm == _f32(0.25 * engine_runs["norm1"])
    assert not torch.equal(g["param"], u["param"])  # (the change reached the replays)


def test_engine_gate_does_not_see_the_clip(engine_runs):
    clipped, unclipped = engine_runs["eager"]["first"], engine_runs["inactive"]["first"]
    assert clipped["clip"].coef < 1.0 and unclipped["clip"].coef == 1.0
    assert torch.equal(clipped["gate"], unclipped["gate"]) and bool(clipped["gate"].any())
    assert not torch.equal(engine_runs["eager"]["param"], engine_runs["inactive"]["param"])


def _dp_worker(rank, world, port, out_dir, max_norm):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    _, st, out = _engine_run(True, steps=3, pg=dist.group.WORLD, gated=False, clip_grad_norm=max_norm,
                             skip_nonfinite_steps=True)
    assert st.buckets is not None
    torch.save({"param": out["param"], "mom": out["mom"], "graphs": out["graphs"],
                "clip": torch.frombuffer(bytearray(bytes(out["clip"])), dtype=torch.uint8)},
               os.path.join(out_dir, "dp.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_engine_one_rank_data_parallel_equals_no_group(dev, tmp_path, engine_runs):
    max_norm = 0.5 * engine_runs["norm1"]
    mp.start_processes(_dp_worker, args=(1, _free_port(), str(tmp_path), max_norm), nprocs=1, join=True,
                       start_method="spawn")
    dp = torch.load(tmp_path / "dp.pt", weights_only=True)
    _, _, e = _engine_run(True, steps=3, gated=False, clip_grad_norm=max_norm, skip_nonfinite_steps=True)
    assert dp["graphs"] and e["graphs"]
    assert torch.equal(dp["param"], e["param"]) and torch.equal(dp["mom"], e["mom"])
    assert bytes(dp["clip"].numpy()) == bytes(e["clip"]) and e["clip"].clipped >= 1 and e["clip"].steps == 3


def test_engine_defaults_untouched(dev):
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    g = torch.Generator(device=dev).manual_seed(9)
    x = torch.randn(4, 2, 3, 64, 64, device=dev, generator=g)
    y = torch.randint(0, 40, (4,), device=dev, generator=g)
    flats = []
    for kw in ({}, dict(clip_grad_norm=None, skip_nonfinite_steps=False)):
        torch.manual_seed(0)
        m = MMTM_MVCNN().to(dev)
        st = BalancedStep(m, lr=LR, **kw)
        assert st.clip_state is None and st.lr_state is None and st.lr_schedule is None and st.sync_clip() is None
        for _ in range(2):
            st(x, y)
        flats.append(st.flat.param.clone())
    assert torch.equal(flats[0], flats[1])


def test_training_loop_logs_norms_coefficients_and_skips(dev, tmp_path, engine_runs, capsys):
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    from greedy_multimodal_learning_amd.train import training_loop
    xs, ys = _batches(dev)
    loader = [(torch.arange(4 * i, 4 * i + 4), xs[i], ys[i]) for i in range(2)]
    torch.manual_seed(0)
    m = MMTM_MVCNN()
    # momentum = wd = 0: clipping needs no fused_momentum opt-in
    H = training_loop(model=m, loss_function=None, metrics=[], optimizer=(LR, 0.0, 0.0), config={},
                      save_path=str(tmp_path), steps_per_epoch=2, train=loader, n_epochs=2, verbose=True,
                      clip_grad_norm=0.5 * engine_runs["norm1"], skip_nonfinite_steps=True)
    assert len(H["loss"]) == 1
    norms, coefs, skips = H["grad_norm"][0], H["clip_coef"][0], H["step_skipped"][0]
    assert len(norms) == len(coefs) == len(skips) == 2
    assert all(math.isfinite(v) and v > 0 for v in norms) and all(0.0 < c <= 1.0 for c in coefs)
    assert skips == [False, False] and coefs[0] < 1.0
    assert f"clipped {sum(c < 1.0 for c in coefs)} skipped 0" in capsys.readouterr().out
    ck = torch.load(tmp_path / "model_last_epoch.pt", weights_only=True)
    m2 = MMTM_MVCNN()
    m2.load_state_dict(ck["model"])
    assert all(bool(torch.isfinite(v).all()) for v in ck["model"].values() if v.is_floating_point())
