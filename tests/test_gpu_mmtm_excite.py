"""The MMTM site's FC work in one launch each way (gm_gemm_f32_chain, gm_mmtm_excite_fwd /
gm_mmtm_excite_bwd; MMTM_mitigate.excite_form = "fused").

The chained kernel runs gm_gemm_f32's own tile arithmetic under its own tile plan, so every
comparison with the separate launches is torch.equal - no tolerance.  The golden fixture is
checked with the reference test's tolerance (helpers.close, rtol 1e-4)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import spec
from helpers import close
from oracle import weights

pytestmark = pytest.mark.gpu

tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------
# 1. gemm_chain == two gemm launches
# ---------------------------------------------------------------------------------------
def _fc_pair(M, K1, N1, N2):
    """x[M,K1] -> z = relu(x W1^T + b1) [M,N1] -> e = sigmoid(z W2^T + b2) [M,N2]"""
    def build(t, out, Op, ONES):
        first = [dict(M=M, N=N1, segs=[(K1, Op(t["x"], K1, 1), Op(t["w1"], 1, K1))], C=out["z"], ld_c=N1,
                      bias=t["b1"], act=1)]
        second = [dict(M=M, N=N2, segs=[(N1, Op(out["z"], N1, 1), Op(t["w2"], 1, N1))], C=out["e"], ld_c=N2,
                       bias=t["b2"], act=2)]
        return first, second
    shapes = dict(x=(M, K1), w1=(N1, K1), b1=(N1,), w2=(N2, N1), b2=(N2,))
    return shapes, dict(z=(M, N1), e=(M, N2)), build


def _two_segments(M, C, N1, N2):
    """the turn-off form: z_v = relu([x_v | avg_s] W^T + b), z_s = relu([avg_v | x_s] W^T + b) with
    the averages as broadcast rows (ld0 = 0), then one excite FC per branch"""
    def build(t, out, Op, ONES):
        C2 = 2 * C
        first = [dict(M=M, N=N1, segs=[(C, Op(t["x"], C2, 1), Op(t["w1"], 1, C2)),
                                       (C, Op(t["avg"], 0, 1), Op(t["w1"], 1, C2, off=C))],
                      C=out["zv"], ld_c=N1, bias=t["b1"], act=1),
                 dict(M=M, N=N1, segs=[(C, Op(t["avg"], 0, 1, off=C), Op(t["w1"], 1, C2)),
                                       (C, Op(t["x"], C2, 1, off=C), Op(t["w1"], 1, C2, off=C))],
                      C=out["zs"], ld_c=N1, bias=t["b1"], act=1)]
        second = [dict(M=M, N=N2, segs=[(N1, Op(out[z], N1, 1), Op(t["w2"], 1, N1))], C=out[e], ld_c=N2,
                       bias=t["b2"], act=2) for z, e in (("zv", "ev"), ("zs", "es"))]
        return first, second
    shapes = dict(x=(M, 2 * C), avg=(2 * C,), w1=(N1, 2 * C), b1=(N1,), w2=(N2, N1), b2=(N2,))
    return shapes, dict(zv=(M, N1), zs=(M, N1), ev=(M, N2), es=(M, N2)), build


def _backward_like(B, C, Cz):
    """round 1: dW = da^T z (transposed view), db = 1^T da (all-ones A), dz = (da W) * (z > 0) (relu
    mask); round 2 reads dz: dWsq += dz^T sq (accumulate into a non-zero C), dbsq = 1^T dz, dsq = dz Wsq"""
    def build(t, out, Op, ONES):
        C2 = 2 * C
        first = [dict(M=C, N=Cz, segs=[(B, Op(t["da"], 1, C), Op(t["z"], Cz, 1))], C=out["gw"], ld_c=Cz),
                 dict(M=1, N=C, segs=[(B, ONES, Op(t["da"], C, 1))], C=out["gb"], ld_c=C),
                 dict(M=B, N=Cz, segs=[(C, Op(t["da"], C, 1), Op(t["w"], Cz, 1))], C=out["dz"], ld_c=Cz,
                      mask=t["z"], ld_mask=Cz)]
        second = [dict(M=Cz, N=C2, segs=[(B, Op(out["dz"], 1, Cz), Op(t["sq"], C2, 1))], C=out["gwsq"], ld_c=C2,
                       accumulate=1),
                  dict(M=1, N=Cz, segs=[(B, ONES, Op(out["dz"], Cz, 1))], C=out["gbsq"], ld_c=Cz),
                  dict(M=B, N=C2, segs=[(Cz, Op(out["dz"], Cz, 1), Op(t["wsq"], C2, 1))], C=out["dsq"], ld_c=C2)]
        return first, second
    shapes = dict(da=(B, C), z=(B, Cz), w=(C, Cz), sq=(B, 2 * C), wsq=(Cz, 2 * C))
    outs = dict(gw=(C, Cz), gb=(C,), dz=(B, Cz), gwsq=(Cz, 2 * C), gbsq=(Cz,), dsq=(B, 2 * C))
    return shapes, outs, build


def _many_tiles():
    """round 2 is 512 x 1024 with K = 4: 512 workgroup tiles, more than any grid cap (one workgroup
    per CU at the most), so every workgroup walks several tiles"""
    def build(t, out, Op, ONES):
        first = [dict(M=512, N=4, segs=[(8, Op(t["x"], 8, 1), Op(t["w1"], 1, 8))], C=out["u"], ld_c=4)]
        second = [dict(M=512, N=1024, segs=[(4, Op(out["u"], 4, 1), Op(t["v"], 1024, 1))], C=out["c"], ld_c=1024)]
        return first, second
    return dict(x=(512, 8), w1=(4, 8), v=(4, 1024)), dict(u=(512, 4), c=(512, 1024)), build


CHAIN_CASES = {
    "ragged_m3_k40_k20": _fc_pair(3, 40, 20, 40),
    "ragged_k37": _fc_pair(3, 37, 20, 37),        # K % 4 != 0 in round 1, N % 16 != 0 in round 2
    "ksplit_k256": _fc_pair(4, 256, 64, 48),      # K split 2 (form 1: 128 k per wave)
    "ksplit_k1024": _fc_pair(4, 1024, 256, 512),  # K split 4, then 2
    "two_segments_broadcast": _two_segments(3, 24, 20, 24),
    "backward_like": _backward_like(5, 24, 12),
    "backward_like_c128": _backward_like(64, 128, 128),
    "many_tiles": _many_tiles(),
}


@pytest.mark.parametrize("form", [0, 2, 3, 257], ids=lambda f: f"form{f}")
@pytest.mark.parametrize("name", ["ksplit_k1024", "backward_like_c128"])
def test_gemm_chain_follows_the_gemm_form(dev, name, form):
    """k_gemm_chain has one instance per gm_gemm_set_form form (4 / 8 / 16 waves, 8 / 16 k-steps per
    round, scalar k-steps) and plans its tiles and K splits as gm_gemm_f32 does under that form."""
    from greedy_multimodal_learning_amd import _lib as L
    lib = L.load()
    try:
        L.check(lib.gm_gemm_set_form(form), "gm_gemm_set_form")
        test_gemm_chain_equals_two_launches(dev, name)
        torch.cuda.synchronize()
    finally:
        L.check(lib.gm_gemm_set_form(1), "gm_gemm_set_form")


@pytest.mark.parametrize("name", list(CHAIN_CASES))
def test_gemm_chain_equals_two_launches(dev, name):
    from greedy_multimodal_learning_amd import ops
    from greedy_multimodal_learning_amd.ops import ONES, Op
    shapes, outs, build = CHAIN_CASES[name]
    g = torch.Generator(device=dev).manual_seed(len(name))
    t = {k: torch.randn(*s, device=dev, generator=g) for k, s in shapes.items()}
    seed = {k: torch.randn(*s, device=dev, generator=g) for k, s in outs.items()}  # non-zero C everywhere
    ref = {k: v.clone() for k, v in seed.items()}
    first, second = build(t, ref, Op, ONES)
    ops.gemm(first, dev)
    ops.gemm(second, dev)
    for rep in range(2):  # twice: the second launch meets the sync words the first one left
        got = {k: v.clone() for k, v in seed.items()}
        first, second = build(t, got, Op, ONES)
        ops.gemm_chain(first, second, dev)
        for k in outs:
            assert torch.isfinite(ref[k]).all(), k
            assert torch.equal(got[k], ref[k]), (name, k, rep)


def test_excite_fwd_op_equals_chain_with_running_average(dev):
    """ops.mmtm_excite_fwd: FC pair + the running average of fc2[0]'s output with the device step
    counter, against gemm, gemm, running_avg_dev - at B not a multiple of 16 and C > 256 (more
    than one channel per thread), with ra_s == ra_v allowed and increment off."""
    from greedy_multimodal_learning_amd import ops
    from greedy_multimodal_learning_amd.ops import ONES, Op
    B, K1, N1, C = 21, 96, 48, 300
    shapes, outs, build = _fc_pair(B, K1, N1, C)
    g = torch.Generator(device=dev).manual_seed(3)
    t = {k: torch.randn(*s, device=dev, generator=g) for k, s in shapes.items()}
    ra0 = torch.randn(C, device=dev, generator=g)
    for same, inc in ((False, True), (True, True), (False, False)):
        res = []
        for fused in (False, True):
            out = {k: torch.empty(*s, device=dev) for k, s in outs.items()}
            ra_v = ra0.clone()
            ra_s = ra_v if same else (2 * ra0)
            step = torch.full((1,), 5, dtype=torch.int32, device=dev)
            fc1, fc2 = build(t, out, Op, ONES)
            for _ in range(2):
                if fused:
                    ops.mmtm_excite_fwd(fc1, fc2, dev, ra_v, ra_s, step, increment=inc)
                else:
                    ops.gemm(fc1, dev)
                    ops.gemm(fc2, dev)
                    ops.running_avg_dev(out["e"], ra_v, ra_s, step, increment=inc)
            res.append((out["z"], out["e"], ra_v, ra_s, step))
        assert int(res[0][4].item()) == (7 if inc else 5)
        for a, b in zip(*res):
            assert torch.equal(a, b), (same, inc)


# ---------------------------------------------------------------------------------------
# 2. every MMTM case with excite_form = "fused"
# ---------------------------------------------------------------------------------------
def _kwargs(case, dev):
    mode = case["mode"]
    avg = spec.mmtm_avg(case)
    return dict(return_scale=True, return_squeezed_mps=(mode == "normal"),
                turnoff_cross_modal_flow=(mode == "turnoff"),
                average_squeezemaps=[tt(avg[0]).to(dev), tt(avg[1]).to(dev)] if mode == "turnoff" else None,
                curation_mode=mode.startswith("cur"),
                caring_modality=int(mode[-1]) if mode.startswith("cur") else 0)


def _run(case, dev, form, dtype=torch.float32, channels_last=False):
    from greedy_multimodal_learning_amd.balanced_mmtm import MMTM_mitigate
    C = case["C"]
    m = MMTM_mitigate(C, C, 4, SEonly=case.get("SEonly", False), shareweight=case.get("shareweight", False))
    weights.apply_to_module(m, seed=spec.SEED_MMTM)
    m = m.to(dev)
    m.excite_form = form
    fmt = torch.channels_last if channels_last else torch.contiguous_format

    def prep(a, grad=False):
        return tt(a).to(dev).to(dtype).contiguous(memory_format=fmt).requires_grad_(grad)
    for k in range(case.get("warm", 0)):
        wv, ws = spec.mmtm_warm_inputs(case, k)
        with torch.no_grad():
            m(prep(wv), prep(ws))
    xv, xs, dyv, dys = spec.mmtm_inputs(case)
    Xv, Xs = prep(xv, True), prep(xs, True)
    Yv, Ys, sc, sq = m(Xv, Xs, **_kwargs(case, dev))
    torch.autograd.backward([Yv, Ys], [prep(dyv), prep(dys)])
    return m, Xv, Xs, Yv, Ys, sc, sq


def _assert_same_site(a, b):
    """two _run results: Y, e, sq, dX, every parameter gradient (None-ness included), both running
    averages and the step counters, bit for bit"""
    ma, Xva, Xsa, Yva, Ysa, sca, sqa = a
    mb, Xvb, Xsb, Yvb, Ysb, scb, sqb = b
    for n, x, y in (("Yv", Yva, Yvb), ("Ys", Ysa, Ysb), ("ev", sca[0], scb[0]), ("es", sca[1], scb[1]),
                    ("dXv", Xva.grad, Xvb.grad), ("dXs", Xsa.grad, Xsb.grad),
                    ("ra_v", ma.running_avg_weight_visual, mb.running_avg_weight_visual),
                    ("ra_s", ma.running_avg_weight_skeleton, mb.running_avg_weight_skeleton)):
        assert torch.equal(x, y), n
    assert (sqa is None) == (sqb is None)
    if sqa is not None:
        assert torch.equal(sqa[0], sqb[0]) and torch.equal(sqa[1], sqb[1])
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert (pa.grad is None) == (pb.grad is None), n
        if pa.grad is not None:
            assert torch.equal(pa.grad, pb.grad), n
    assert ma.step == mb.step
    assert int(ma._step_dev.item()) == int(mb._step_dev.item()) == ma.step


@pytest.mark.parametrize("case", spec.MMTM_CASES, ids=lambda c: c["id"])
def test_fused_mmtm_fp32_vs_reference_and_chain(golden, dev, case):
    fix = golden["mmtm"]
    res = _run(case, dev, "fused")
    m, Xv, Xs, Yv, Ys, sc, sq = res
    p = case["id"] + "/"
    f = lambda t: t.detach().float().cpu().contiguous()  # noqa: E731
    close(fix, p + "Yv", f(Yv))
    close(fix, p + "Ys", f(Ys))
    close(fix, p + "ev", sc[0])
    close(fix, p + "es", sc[1])
    if sq is not None:
        close(fix, p + "sqv", sq[0])
        close(fix, p + "sqs", sq[1])
    close(fix, p + "dXv", f(Xv.grad))
    close(fix, p + "dXs", f(Xs.grad))
    for n, prm in m.named_parameters():
        g = f(prm.grad) if prm.grad is not None else torch.full(prm.shape, float("nan"))
        close(fix, p + "grad." + n, g.numpy(), rtol=1e-4, atol=1e-5)
    close(fix, p + "ra_v", f(m.running_avg_weight_visual))
    close(fix, p + "ra_s", f(m.running_avg_weight_skeleton))
    assert int(fix[p + "step"]) == m.step
    _assert_same_site(res, _run(case, dev, "chain"))


@pytest.mark.parametrize("case", [c for c in spec.MMTM_CASES if c["id"] in ("n128", "c1", "off", "se", "sw")],
                         ids=lambda c: c["id"])
def test_fused_mmtm_bf16_channels_last_equals_chain(dev, case):
    _assert_same_site(_run(case, dev, "fused", torch.bfloat16, True), _run(case, dev, "chain", torch.bfloat16, True))


# ---------------------------------------------------------------------------------------
# 3. back to back, and under graph replay
# ---------------------------------------------------------------------------------------
def _site(dev, form, C=128):
    from greedy_multimodal_learning_amd.balanced_mmtm import MMTM_mitigate
    m = MMTM_mitigate(C, C, 4)
    weights.apply_to_module(m, seed=spec.SEED_MMTM)
    m = m.to(dev)
    m.excite_form = form
    return m


def _call(m, xv, xs, dyv, dys):
    for p in m.parameters():
        p.grad = None
    Xv, Xs = xv.clone().requires_grad_(True), xs.clone().requires_grad_(True)
    Yv, Ys, _, _ = m(Xv, Xs)
    torch.autograd.backward([Yv, Ys], [dyv, dys])
    return [Yv.detach(), Ys.detach(), Xv.grad, Xs.grad] + [p.grad for p in m.parameters()] + \
        [m.running_avg_weight_visual.clone(), m.running_avg_weight_skeleton.clone()]


def test_fifty_fused_calls_back_to_back_equal_chain(dev):
    """No host-side reset and no synchronisation between the launches: the sync words re-arm
    themselves."""
    g = torch.Generator(device=dev).manual_seed(50)
    ins = [[torch.randn(3, 128, 5, 5, device=dev, generator=g) for _ in range(4)] for _ in range(5)]
    outs = {}
    for form in ("chain", "fused"):
        m = _site(dev, form)
        outs[form] = [_call(m, *ins[i % 5]) for i in range(50)]
        assert int(m._step_dev.item()) == 50
    for i, (a, b) in enumerate(zip(outs["chain"], outs["fused"])):
        for x, y in zip(a, b):
            assert torch.equal(x, y), i


def test_fused_site_under_graph_replay(dev):
    """One site forward + backward captured once and replayed three times == three eager calls;
    the kernel arguments are frozen and nothing resets the sync words between replays."""
    from greedy_multimodal_learning_amd import streams
    from greedy_multimodal_learning_amd.balanced_mmtm import _step_counter
    g = torch.Generator(device=dev).manual_seed(9)
    xv, xs, dyv, dys = [torch.randn(3, 128, 5, 5, device=dev, generator=g) for _ in range(4)]
    _call(_site(dev, "fused"), xv, xs, dyv, dys)  # eager first: the stream's sync words exist
    m_e = _site(dev, "chain")
    for _ in range(3):
        want = _call(m_e, xv, xs, dyv, dys)
    m_g = _site(dev, "fused")
    _step_counter(m_g, dev)  # created outside the capture (its fill must not be replayed)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    eager_sid = torch.cuda.current_stream(dev).stream_id
    with torch.cuda.graph(graph):
        streams.alias_capture_stream(dev.index, eager_sid)
        Xv, Xs = xv.clone().requires_grad_(True), xs.clone().requires_grad_(True)
        Yv, Ys, _, _ = m_g(Xv, Xs)
        torch.autograd.backward([Yv, Ys], [dyv, dys])
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(m_g._step_dev.item()) == 3
    got = [Yv.detach(), Ys.detach(), Xv.grad, Xs.grad] + [p.grad for p in m_g.parameters()] + \
        [m_g.running_avg_weight_visual, m_g.running_avg_weight_skeleton]
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i


# ---------------------------------------------------------------------------------------
# 5. engine level
# ---------------------------------------------------------------------------------------
def test_engine_step_fused_equals_default(dev):
    from greedy_multimodal_learning_amd.balanced_mmtm import MMTM_mitigate
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(2, 2, 3, 64, 64, device=dev, generator=g)
    y = torch.randint(0, 40, (2,), device=dev, generator=g)
    res = []
    for form in (None, "fused"):
        torch.manual_seed(0)
        m = MMTM_MVCNN().to(dev)
        st = BalancedStep(m, lr=0.05, mmtm_excite=form)
        sites = [s for s in m.modules() if isinstance(s, MMTM_mitigate)]
        assert sites and all(s.excite_form == (form or "chain") for s in sites)
        loss = st(x, y)
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), m))
    assert torch.isfinite(res[0][0]).all()
    assert torch.equal(res[0][0], res[1][0])
    for (n, a), (_, b) in zip(res[0][1].named_parameters(), res[1][1].named_parameters()):
        assert torch.equal(a, b), n
    for a, b in zip(*[[s for s in r[1].modules() if isinstance(s, MMTM_mitigate)] for r in res]):
        assert torch.equal(a.running_avg_weight_visual, b.running_avg_weight_visual)
        assert int(a._step_dev.item()) == int(b._step_dev.item()) == 1


# ---------------------------------------------------------------------------------------
# 6. residency: beside a kernel that holds 64 CUs and never yields
# ---------------------------------------------------------------------------------------
HOLD_CUS, HOLD_US = 64, 300_000


def _worker(rank, out_dir):
    from greedy_multimodal_learning_amd import _lib as L
    import testkit
    L.set_residency(streams=1, sharers=1, reserved_cus=HOLD_CUS)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    B, C, H = 64, 512, 7  # the layer-4 site at the benchmark batch
    xv, xs, dyv, dys = [torch.randn(B, C, H, H, device=dev, generator=g) for _ in range(4)]
    m = _site(dev, "fused", C)

    def work():
        return _call(m, xv, xs, dyv, dys)[:-2]  # (the running averages move with every call)

    ref = work()
    torch.cuda.synchronize()
    f0 = L.device_faults(clear=True)
    hold = torch.cuda.Stream(device=dev)
    e0 = torch.cuda.Event(enable_timing=True)
    e_hold = torch.cuda.Event(enable_timing=True)
    e_work = torch.cuda.Event(enable_timing=True)
    e0.record()
    hold.wait_stream(torch.cuda.current_stream())
    testkit.hold_cus(HOLD_CUS, 256, 160 * 1024, HOLD_US, hold.cuda_stream)
    e_hold.record(hold)
    torch.cuda._sleep(2_000_000)  # let the holding workgroups land first
    out = work()
    e_work.record()
    torch.cuda.synchronize()
    res = dict(f0=f0, f1=L.device_faults(clear=True), t_work=e0.elapsed_time(e_work),
               t_hold=e0.elapsed_time(e_hold), equal=all(torch.equal(a, b) for a, b in zip(out, ref)),
               finite=all(bool(torch.isfinite(a).all()) for a in out))
    torch.save(res, os.path.join(out_dir, "excite_residency.pt"))


def test_fused_site_beside_a_cu_holding_kernel(tmp_path, monkeypatch):
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "8")  # as test_gpu_residency: the holder on a queue of its own
    mp.start_processes(_worker, args=(str(tmp_path),), nprocs=1, join=True, start_method="spawn")
    r = torch.load(tmp_path / "excite_residency.pt", weights_only=True)
    print(f"work done at {r['t_work']:.2f} ms, CU-holding kernel done at {r['t_hold']:.2f} ms")
    assert r["f0"] == 0 and r["f1"] == 0
    assert r["t_work"] < r["t_hold"], "the chained launches waited for the CU-holding kernel"
    assert r["equal"] and r["finite"]


# ---------------------------------------------------------------------------------------
# 4. no hand-off of this module's tests timed out (runs last)
# ---------------------------------------------------------------------------------------
def test_no_device_fault_was_raised(dev):
    from greedy_multimodal_learning_amd import _lib as L
    assert L.device_faults(clear=True) == 0
