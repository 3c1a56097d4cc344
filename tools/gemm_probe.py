"""Latency of the MMTM FC GEMMs (k_gemm_f32 via gm_gemm_f32) on the C2 site shapes, in
isolation: the forward joint FC [B, 2C] x [2C, C'] (+bias, ReLU), the excite FC pair
[B, C'] x [C', C] (+bias, sigmoid) and the backward weight-gradient problems, for each
site (C = 128, 256, 512 per modality, ratio 4 as in MMTM_MVCNN), B = 64.  Interleaved
rounds of the GEMM forms (gm_gemm_set_form 0-3) in one process; HIP events on
the launch stream, 50 launches per timing.

    python tools/gemm_probe.py                 # event timing (host-launch-bound: Python ctypes)
    python tools/gemm_probe.py report TRACE    # kernel durations per (form, case) from a rocprofv3
                                               # kernel trace of the run above
    python tools/gemm_probe.py fused [FORM ..] # one site's FC work, separate launches ("chain") against
                                               # the one-launch form ("fused", gm_mmtm_excite_fwd / _bwd),
                                               # under each gm_gemm_set_form FORM (default: 1)
    python tools/gemm_probe.py step            # the C2 step (B=64, bf16, graphs), mmtm_excite chain / fused

fused: forward (squeeze FC, excite FCs, running average) and backward (excite gradients + dz, squeeze
gradients + dsq) of one NORMAL-mode site at B = 64, C = 128 / 256 / 512.  Each form is captured as a
hipGraph of 20 repetitions (device time, no Python launch cost between the kernels); the two graphs are
replayed alternately in one process, 15 rounds after 3 warm-up rounds, HIP events around each replay.
step: two engines on the same seed in one process, 20 steps per timing, alternating, 7 rounds.
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problems(dev, B, C, ratio=4):
    from greedy_multimodal_learning_amd.ops import ONES, Op
    C2 = 2 * C
    Cz = int(2 * C2 / ratio)
    f = dict(device=dev, dtype=torch.float32)
    sq, w_sq, b_sq = torch.randn(B, C2, **f), torch.randn(Cz, C2, **f), torch.randn(Cz, **f)
    z, w_v, b_v = torch.randn(B, Cz, **f), torch.randn(C, Cz, **f), torch.randn(C, **f)
    e_v, e_s = torch.empty(B, C, **f), torch.empty(B, C, **f)
    da, gw, gb, dz = torch.randn(B, C, **f), torch.empty(C, Cz, **f), torch.empty(C, **f), torch.empty(B, Cz, **f)
    zj = torch.empty(B, Cz, **f)
    return {
        "joint": [dict(M=B, N=Cz, segs=[(C2, Op(sq, C2, 1), Op(w_sq, 1, C2))], C=zj, ld_c=Cz, bias=b_sq, act=1)],
        "excite": [dict(M=B, N=C, segs=[(Cz, Op(z, Cz, 1), Op(w_v, 1, Cz))], C=e, ld_c=C, bias=b_v, act=2)
                   for e in (e_v, e_s)],
        "bwd_w": [dict(M=C, N=Cz, segs=[(B, Op(da, 1, C), Op(z, Cz, 1))], C=gw, ld_c=Cz),
                  dict(M=1, N=C, segs=[(B, ONES, Op(da, C, 1))], C=gb, ld_c=C),
                  dict(M=B, N=Cz, segs=[(C, Op(da, C, 1), Op(w_v, Cz, 1))], C=dz, ld_c=Cz, mask=z, ld_mask=Cz)],
    }


FORMS = (1, 257, 0, 256, 4)
ROUNDS, REPS = 3, 53


def case_keys():
    return [(C, k) for C in (128, 512) for k in ("joint", "excite", "bwd_w")]


def report(trace):
    import csv
    rows = [r for r in csv.DictReader(open(trace)) if "k_gemm_f32" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    res, i = {}, 0
    for _ in range(ROUNDS):
        for f in FORMS:
            for key in case_keys():
                chunk = sorted(dur[i + 3:i + REPS])
                i += REPS
                res.setdefault((key, f), []).append(chunk[len(chunk) // 2])
    assert i == len(dur), (i, len(dur))
    for (key, f), ts in sorted(res.items()):
        ts.sort()
        print(f"C={key[0]:4d} {key[1]:7s} form={f:3d}: kernel median {ts[len(ts) // 2]:6.2f} us")


def site_problems(dev, B, C, ratio=4):
    """The FC problems of one NORMAL-mode MMTM site (balanced_mmtm.py): forward rounds fc1, fc2 (+ the
    running-average state) and backward rounds first, second."""
    from greedy_multimodal_learning_amd.ops import ONES, Op
    C2 = 2 * C
    Cz = int(2 * C2 / ratio)
    f = dict(device=dev, dtype=torch.float32)
    r = lambda *s: torch.randn(*s, **f)  # noqa: E731
    e = lambda *s: torch.empty(*s, **f)  # noqa: E731
    sq, w_sq, b_sq, z = r(B, C2), r(Cz, C2), r(Cz), e(B, Cz)
    w_v, b_v, w_s, b_s, e_v, e_s = r(C, Cz), r(C), r(C, Cz), r(C), e(B, C), e(B, C)
    fc1 = [dict(M=B, N=Cz, segs=[(C2, Op(sq, C2, 1), Op(w_sq, 1, C2))], C=z, ld_c=Cz, bias=b_sq, act=1)]
    fc2 = [dict(M=B, N=C, segs=[(Cz, Op(z, Cz, 1), Op(w, 1, Cz))], C=o, ld_c=C, bias=b, act=2)
           for w, b, o in ((w_v, b_v, e_v), (w_s, b_s, e_s))]
    ra = (e_v, torch.zeros(C, **f), torch.zeros(C, **f), torch.zeros(1, device=dev, dtype=torch.int32))
    da_v, da_s, zf, dz, dsq = r(B, C), r(B, C), r(B, Cz), e(B, Cz), e(B, C2)
    first = []
    for da, w in ((da_v, w_v), (da_s, w_s)):
        first += [dict(M=C, N=Cz, segs=[(B, Op(da, 1, C), Op(zf, Cz, 1))], C=e(C, Cz), ld_c=Cz),
                  dict(M=1, N=C, segs=[(B, ONES, Op(da, C, 1))], C=e(C), ld_c=C)]
    first.append(dict(M=B, N=Cz, segs=[(C, Op(da_v, C, 1), Op(w_v, Cz, 1)), (C, Op(da_s, C, 1), Op(w_s, Cz, 1))],
                      C=dz, ld_c=Cz, mask=zf, ld_mask=Cz))
    second = [dict(M=Cz, N=C2, segs=[(B, Op(dz, 1, Cz), Op(sq, C2, 1))], C=e(Cz, C2), ld_c=C2),
              dict(M=1, N=Cz, segs=[(B, ONES, Op(dz, Cz, 1))], C=e(Cz), ld_c=Cz),
              dict(M=B, N=C2, segs=[(Cz, Op(dz, Cz, 1), Op(w_sq, C2, 1))], C=dsq, ld_c=C2)]
    return fc1, fc2, ra, first, second


def _stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fused():
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import ops
    dev = torch.device("cuda:0")
    L.load()
    INNER, WARM, ROUNDS_F = 20, 3, 15
    print(f"residency plan (streams, sharers, reserved_cus) = {L.get_residency()}")
    forms = [int(v) for v in sys.argv[2:]] or [1]
    for form, C in [(f, C) for f in forms for C in (128, 256, 512)]:
        L.check(L.load().gm_gemm_set_form(form), "set_form")
        fc1, fc2, ra, first, second = site_problems(dev, 64, C)
        runs = {
            ("fwd", "chain"): lambda: (ops.gemm(fc1, dev), ops.gemm(fc2, dev), ops.running_avg_dev(*ra)),
            ("fwd", "fused"): lambda: ops.mmtm_excite_fwd(fc1, fc2, dev, ra[1], ra[2], ra[3]),
            ("bwd", "chain"): lambda: (ops.gemm(first, dev), ops.gemm(second, dev)),
            ("bwd", "fused"): lambda: ops.mmtm_excite_bwd(first, second, dev),
        }
        graphs = {}
        for key, run in runs.items():
            run()  # eager first: code objects loaded, the stream's sync words exist
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(INNER):
                    run()
            graphs[key] = g
        res = {k: [] for k in runs}
        for rnd in range(WARM + ROUNDS_F):
            for key, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                if rnd >= WARM:
                    res[key].append(e0.elapsed_time(e1) / INNER * 1e3)
        for d in ("fwd", "bwd"):
            (mc, lc, hc), (mf, lf, hf) = _stats(res[(d, "chain")]), _stats(res[(d, "fused")])
            print(f"form={form} C={C:4d} B=64 {d}: chain median {mc:6.2f} us [{lc:6.2f}, {hc:6.2f}]   fused median {mf:6.2f} us "
                  f"[{lf:6.2f}, {hf:6.2f}]   fused/chain {mf / mc:5.2f}")
    L.check(L.load().gm_gemm_set_form(1), "set_form")
    faults = L.device_faults(clear=True)
    print(f"device fault word after the run: {faults}")


def step_ab():
    from greedy_multimodal_learning_amd.callbacks import Bias_Mitigation_Strong
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    dev = torch.device("cuda:0")
    B, STEPS, WARM, ROUNDS_S = 64, 20, 8, 7
    g = torch.Generator(device=dev).manual_seed(1000)
    xs = [torch.randn(2, B, 224, 224, 3, device=dev, generator=g).bfloat16().permute(1, 0, 4, 2, 3) for _ in range(2)]
    ys = [torch.randint(0, 40, (B,), device=dev, generator=g) for _ in range(2)]
    eng = {}
    for form in ("chain", "fused"):
        torch.manual_seed(0)
        model = MMTM_MVCNN().to(dev)
        gate = Bias_Mitigation_Strong(epsilon=0.01, curation_windowsize=5, branchnames=["net_view_0", "net_view_1"],
                                      starting_epoch=1, MMTMnames=["visual", "skeleton"])
        st = BalancedStep(model, lr=0.1, gate=gate, compute_dtype=torch.bfloat16, channels_last=True, graphs=True,
                          mmtm_excite=form)
        st.on_epoch_begin(1)
        st.bind_batches(*zip(xs, ys))
        for i in range(WARM):
            st(xs[i % 2], ys[i % 2])
        torch.cuda.synchronize()
        assert st.graphs, st.capture_failures
        eng[form] = st
    res = {k: [] for k in eng}
    for _ in range(ROUNDS_S):
        for form, st in eng.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(STEPS):
                st(xs[i % 2], ys[i % 2])
            torch.cuda.synchronize()
            res[form].append((time.perf_counter() - t0) / STEPS * 1e3)
    for form in eng:
        m, lo, hi = _stats(res[form])
        print(f"C2 step B=64 bf16 graphs mmtm_excite={form}: median {m:7.3f} ms [{lo:7.3f}, {hi:7.3f}] "
              f"loss {float(eng[form].last_loss):.6f}")
    from greedy_multimodal_learning_amd import _lib as L
    print(f"device fault word after the run: {L.device_faults(clear=True)}")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "report":
        return report(sys.argv[2])
    if len(sys.argv) > 1 and sys.argv[1] == "fused":
        return fused()
    if len(sys.argv) > 1 and sys.argv[1] == "step":
        return step_ab()
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd import ops
    dev = torch.device("cuda:0")
    lib = L.load()
    cases = {(C, k): v for C in (128, 512) for k, v in problems(dev, 64, C).items()}
    assert list(cases) == case_keys()
    # a trivial torch kernel for the launch floor
    t = torch.empty(16, device=dev)
    cases[(0, "fill")] = t
    res = {}
    for _ in range(ROUNDS):
        for nw in FORMS:
            L.check(lib.gm_gemm_set_form(nw), "set_form")
            for key, probs in cases.items():
                run = (lambda: probs.fill_(1.0)) if key[1] == "fill" else (lambda: ops.gemm(probs, dev))
                for _ in range(REPS - 50):
                    run()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50):
                    run()
                e1.record()
                torch.cuda.synchronize()
                res.setdefault((key, nw), []).append(e0.elapsed_time(e1) / 50 * 1e3)
    for (key, nw), ts in sorted(res.items()):
        ts.sort()
        print(f"C={key[0]:4d} {key[1]:7s} form={nw}: median {ts[len(ts) // 2]:7.2f} us per launch")


if __name__ == "__main__":
    main()
