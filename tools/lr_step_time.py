"""The C2 training step with the learning rate in device memory against the default (the rate a
kernel argument), and what a change of the rate costs each of them.

Two engines on the same seed in one process (the method of tools/gemm_probe.py step): B = 64,
bf16, hipGraph steps on bound batches, 20 steps per timing, alternating, 7 rounds after 8 warm-up
steps; per engine the median over the rounds of the round's mean step and the rounds' spread.
Then one change of the rate on each engine and the wall time of the first step after it (device
drained before and after): the default engine synchronises, destroys its graphs and captures a new
one; the held device state is a 4-byte fill in front of the same replay.  One JSON line.

    python tools/lr_step_time.py [--rounds 7] [--steps 20] [--clip] [--out FILE]

--clip adds a third engine on the same seed, alternating with the other two: the held device rate
plus BalancedStep(clip_grad_norm=1e9, skip_nonfinite_steps=True) - a bound that never clips, so it
computes what the others compute with gm_group_sumsq_clip's three launches in place of two
(`clip_minus_default_ms`, `clip_minus_held_ms`: differences of medians, against the spreads).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--clip", action="store_true", help="a third engine with the clip on at a bound that never clips")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from greedy_multimodal_learning_amd.callbacks import Bias_Mitigation_Strong
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    if not torch.cuda.is_available():
        raise SystemExit("lr_step_time: needs a HIP device (no CPU timing)")
    dev = torch.device("cuda:0")
    B, WARM, LR = 64, 8, 0.1
    g = torch.Generator(device=dev).manual_seed(1000)
    xs = [torch.randn(2, B, 224, 224, 3, device=dev, generator=g).bfloat16().permute(1, 0, 4, 2, 3) for _ in range(2)]
    ys = [torch.randint(0, 40, (B,), device=dev, generator=g) for _ in range(2)]
    eng = {}
    configs = [("default", None, {}), ("held_device_lr", LRSchedule("held", LR), {})]
    if a.clip:
        configs.append(("clip_never_clips", LRSchedule("held", LR), dict(clip_grad_norm=1e9, skip_nonfinite_steps=True)))
    for name, sch, extra in configs:
        torch.manual_seed(0)
        model = MMTM_MVCNN().to(dev)
        gate = Bias_Mitigation_Strong(epsilon=0.01, curation_windowsize=5, branchnames=["net_view_0", "net_view_1"],
                                      starting_epoch=1, MMTMnames=["visual", "skeleton"])
        st = BalancedStep(model, lr=LR, gate=gate, compute_dtype=torch.bfloat16, channels_last=True, graphs=True,
                          lr_schedule=sch, **extra)
        st.on_epoch_begin(1)
        st.bind_batches(*zip(xs, ys))
        for i in range(WARM):
            st(xs[i % 2], ys[i % 2])
        torch.cuda.synchronize()
        assert st.graphs, st.capture_failures
        eng[name] = st

    def timed(st, n, first=0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(first, first + n):
            st(xs[i % 2], ys[i % 2])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    ms = {k: [] for k in eng}
    for _ in range(a.rounds):
        for name, st in eng.items():
            ms[name].append(timed(st, a.steps))
    res = {"batch": B, "rounds": a.rounds, "steps_per_round": a.steps}
    for name in eng:
        res[name] = {"step_ms": round(statistics.median(ms[name]), 4),
                     "spread_ms": round(max(ms[name]) - min(ms[name]), 4), "graphs": len(eng[name]._graphs)}
    res["held_minus_default_ms"] = round(res["held_device_lr"]["step_ms"] - res["default"]["step_ms"], 4)
    if a.clip:
        res["clip_minus_default_ms"] = round(res["clip_never_clips"]["step_ms"] - res["default"]["step_ms"], 4)
        res["clip_minus_held_ms"] = round(res["clip_never_clips"]["step_ms"] - res["held_device_lr"]["step_ms"], 4)
        c = eng["clip_never_clips"].sync_clip()
        res["clip_never_clips"].update(steps=c.steps, clipped=c.clipped, skipped=c.skipped, grad_norm=c.total_sq ** 0.5)
    # one change of the rate: the first step after it on each slot's graph, then a settled step
    for name, st in eng.items():
        st.lr = 0.03
        first = [timed(st, 1, i) for i in range(2)]  # (bound batches: one graph per slot)
        res[name]["first_step_after_lr_change_ms"] = [round(v, 3) for v in first]
        res[name]["settled_step_ms"] = round(timed(st, a.steps), 4)
        res[name]["graphs_after"] = len(st._graphs)
        assert st.graphs, st.capture_failures
    same = all(torch.equal(p, q) for name in list(eng)[1:]
               for p, q in zip(eng["default"].model.state_dict().values(), eng[name].model.state_dict().values()))
    res["engines_bit_identical"] = bool(same)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
