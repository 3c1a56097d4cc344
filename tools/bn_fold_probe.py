"""Per-shape timing of the BatchNorm finalize folded into its apply (k_bn_finalize_apply,
k_bn_bwd_finalize_apply) against the two launches it replaces, for every BatchNorm of a
workload's step that takes its statistics from a convolution epilogue:

    python tools/bn_fold_probe.py [--workload C2|C5] [--rounds 7] [--reps 20] [--out FILE.json]

The shapes (M, C, rows, G, residual, relu) are recorded from one eager step of the workload's
model (the entry points of the trunk wrapped for that step).  Each shape is then timed on
synthetic tensors: per round, every arm - the two launches, and the folded kernel at the
rule's block count and at 1/2x, 2x and 4x of it (or a fixed ladder where the rule declines) -
runs `reps` back-to-back calls between two HIP events queued behind a device sleep, so the host
is ahead of the device and the figure is the device-side cost of the chain, launch and
dependency floor included.  Arms alternate within a round; reported: median, min, max over the
rounds, in microseconds per call.  The rule's constants (kFoldGrid, kFoldMaxRows,
kFoldReread, kFoldMaxElems in batchnorm.hip) are set from this table: a shape folds only where the folded
median is below the two launches' by more than the larger of the two spreads."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16


def record_shapes(workload, batch, size):
    """One eager BalancedStep of the workload with the statistics-fed BatchNorm entry points
    wrapped: the set of (kind, M, C, rows, G, residual, relu) they were called with."""
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd.callbacks import Bias_Mitigation_Strong
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN, MMTM_MVCNN_N
    lib = L.load()
    dev = torch.device("cuda:0")
    seen = {}
    names = ("gm_bn_fwd_finalize_apply_grouped_bf16", "gm_bn_bwd_finalize_apply_grouped_bf16")
    real = {n: getattr(lib, n) for n in names}

    def wrap(name, struct):
        def f(arr, G, part, rows, st):
            p = ctypes.cast(arr, ctypes.POINTER(struct))[0]
            res = bool(getattr(p, "residual", None))
            key = (name.split("_")[2], int(p.M), int(p.C), int(rows), int(G), res, bool(p.relu))
            seen[key] = seen.get(key, 0) + 1
            return real[name](arr, G, part, rows, st)
        return f
    for n, s in zip(names, (L.BnFwd, L.BnBwd)):
        setattr(lib, n, wrap(n, s))
    try:
        torch.manual_seed(0)
        if workload == "C2":
            model, V = MMTM_MVCNN().to(dev), 2
            bn, mn = ["net_view_0", "net_view_1"], ["visual", "skeleton"]
        else:
            V = {"C4": 4, "C5": 12}[workload]
            model = MMTM_MVCNN_N(num_views=V, trunk="resnet50" if workload == "C5" else "resnet18").to(dev)
            bn, mn = model.branch_names(), model.mmtm_names()
        gate = Bias_Mitigation_Strong(epsilon=0.01, curation_windowsize=5, branchnames=bn, starting_epoch=1,
                                      MMTMnames=mn)
        step = BalancedStep(model, lr=0.1, gate=gate, compute_dtype=BF, channels_last=True, graphs=False,
                            branchnames=bn, MMTMnames=mn)
        step.on_epoch_begin(1)
        x = torch.randn(V, batch, size, size, 3, device=dev).to(BF).permute(1, 0, 4, 2, 3)
        y = torch.randint(0, 40, (batch,), device=dev)
        step(x, y)
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(lib, n, real[n])
    del step, model
    torch.cuda.empty_cache()
    return seen


def arms_for(kind, M, C, rows, G, res, relu):
    """{arm name: callable} on synthetic tensors of the shape."""
    from greedy_multimodal_learning_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    st = L.stream_of(dev)
    x = torch.randn(G, M, C, device=dev).to(BF)
    o = torch.empty_like(x)
    gam, bet = torch.rand(G, C, device=dev) + 0.5, torch.rand(G, C, device=dev) - 0.5
    sm, si = x.float().mean(1).contiguous(), (x.float().var(1) + 1e-5).rsqrt().contiguous()
    keep = [x, o, gam, bet, sm, si]
    if kind == "fwd":
        r = torch.randn(G, M, C, device=dev).to(BF) if res else None
        mk = torch.empty(G, M * C // 8, device=dev, dtype=torch.uint8) if res and relu else None
        coef = torch.empty(G, 2 * C, device=dev)
        rm, rv = torch.zeros(G, C, device=dev), torch.ones(G, C, device=dev)
        stats = torch.randn(G, (rows + 1) * 2 * C, device=dev).abs()
        keep += [r, mk, coef, rm, rv, stats]
        arr = L.arr(L.BnFwd, [L.BnFwd(M, C, int(relu), x[g].data_ptr(), r[g].data_ptr() if res else 0,
                                      o[g].data_ptr(), gam[g].data_ptr(), bet[g].data_ptr(), rm[g].data_ptr(),
                                      rv[g].data_ptr(), 0.1, 1e-5, sm[g].data_ptr(), si[g].data_ptr(), 0,
                                      coef[g].data_ptr(), mk[g].data_ptr() if mk is not None else 0)
                                      for g in range(G)])

        def two():
            lib.gm_bn_fwd_stats_finalize_grouped(arr, G, stats.data_ptr(), rows, st)
            lib.gm_bn_fwd_apply_grouped_bf16(arr, G, stats.data_ptr(), rows, st)

        def fold(nb):
            return lambda: lib.gm_bn_fwd_finalize_apply_grouped_bf16_ex(arr, G, stats.data_ptr(), rows, nb, st)
    else:
        dy = torch.randn(G, M, C, device=dev).to(BF)
        fc = torch.cat([gam * si, bet - sm * gam * si], 1).contiguous()
        dg, db = torch.empty(G, C, device=dev), torch.empty(G, C, device=dev)
        off = lib.gm_bn_bwd_stats_coef_offset(C, G, rows)
        stats = torch.randn(off + G * 4 * C, device=dev)
        keep += [dy, fc, dg, db, stats]
        arr = L.arr(L.BnBwd, [L.BnBwd(M, C, int(relu), dy[g].data_ptr(), 0, x[g].data_ptr(), gam[g].data_ptr(),
                                      sm[g].data_ptr(), si[g].data_ptr(), o[g].data_ptr(), 0, dg[g].data_ptr(),
                                      db[g].data_ptr(), 0, 0, fc[g].data_ptr() if relu else 0, 0) for g in range(G)])

        def two():
            lib.gm_bn_bwd_stats_finalize_grouped(arr, G, stats.data_ptr(), rows, st)
            lib.gm_bn_bwd_apply_grouped_bf16(arr, G, stats.data_ptr(), rows, st)

        def fold(nb):
            return lambda: lib.gm_bn_bwd_finalize_apply_grouped_bf16_ex(arr, G, stats.data_ptr(), rows, nb, st)
    rule = lib.gm_bn_fold_blocks(M, C, rows, G)
    chunks = (M + 127) // 128
    ladder = sorted({max(1, min(chunks, n)) for n in
                     ((rule // 2, rule, 2 * rule, 4 * rule) if rule else (8, 16, 32, 64, 128))})
    arms = {"two": two}
    for nb in ladder:
        arms[f"fold{nb}"] = fold(nb)
    return arms, rule, keep


def time_shape(arms, rounds, reps):
    res = {k: [] for k in arms}
    for f in arms.values():  # warm
        f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(2_000_000)  # the host runs ahead: the events time the device alone
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
            for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", choices=["C2", "C4", "C5"])
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batch = a.batch or (32 if a.workload == "C5" else 64)
    shapes = record_shapes(a.workload, batch, a.size)
    table = []
    for key, count in sorted(shapes.items()):
        kind, M, C, rows, G, res, relu = key
        arms, rule, keep = arms_for(*key)
        t = time_shape(arms, a.rounds, a.reps)
        row = dict(kind=kind, M=M, C=C, rows=rows, G=G, residual=res, relu=relu, per_step=count, rule_nb=rule, us=t)
        table.append(row)
        print(json.dumps(row), flush=True)
        del arms, keep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(workload=a.workload, batch=batch, rounds=a.rounds, reps=a.reps,
                           method="HIP events behind a device sleep, arms interleaved per round, us per call",
                           shapes=table), f, indent=1)


if __name__ == "__main__":
    main()
