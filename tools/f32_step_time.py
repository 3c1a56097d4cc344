"""Step time of the fp32 (reference-precision) C2 step per contraction mode: BalancedStep
(compute_dtype=float32, graphs on) at the benchmark's shapes (B=64, two views, 224^2), one
engine per mode, timed interleaved (round r: every mode in turn, `--steps` steps each, wall
clock around a device sync).  Prints one JSON line: per mode the median ms/step over the
rounds, the (max - min) / median spread, the loss of the first step (same weights and batch
in every mode: the modes can be compared there) and of the last one (after warmup + rounds x
steps SGD steps at lr 0.1 the runs have drifted apart as any two fp32 runs do), and `--label`.

    python tools/f32_step_time.py [--modes exact,bf16x3,bf16x6] [--batch 64] [--size 224]
                                  [--warmup 6] [--steps 10] [--rounds 5] [--label TEXT]

To time an earlier commit's exact step beside this one's, copy this file into a checkout of that
commit and run it there with `--modes exact --label <commit>` (it imports the package of the
tree it sits in; "exact" passes no argument an older engine lacks).

bench.py stays the yardstick of the bf16 step; this tool exists because the fp32 step's
modes have to be compared in one process on one device.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(mode, B, size, dev):
    from greedy_multimodal_learning_amd.callbacks import Bias_Mitigation_Strong
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    torch.manual_seed(0)
    model = MMTM_MVCNN().to(dev)
    gate = Bias_Mitigation_Strong(epsilon=0.01, curation_windowsize=5, branchnames=["net_view_0", "net_view_1"],
                                  starting_epoch=1, MMTMnames=["visual", "skeleton"])
    kw = {} if mode == "exact" else {"f32_contraction": mode}  # ("exact" is the engine's default)
    step = BalancedStep(model, lr=0.1, gate=gate, compute_dtype=torch.float32, channels_last=True, graphs=True, **kw)
    step.on_epoch_begin(1)
    g = torch.Generator(device=dev).manual_seed(1000)
    xs = [torch.randn(2, B, size, size, 3, device=dev, generator=g).permute(1, 0, 4, 2, 3) for _ in range(2)]
    ys = [torch.randint(0, 40, (B,), device=dev, generator=g) for _ in range(2)]
    step.bind_batches(*zip(xs, ys))
    return step, xs, ys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="exact,bf16x3,bf16x6")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="", help="copied into the output line (which tree, which run)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from greedy_multimodal_learning_amd import build
    build.build()
    modes = a.modes.split(",")
    runs = {m: make(m, a.batch, a.size, dev) for m in modes}
    first = {}
    for m, (step, xs, ys) in runs.items():
        for i in range(a.warmup):
            loss = step(xs[i % 2], ys[i % 2])
            if i == 0:
                first[m] = float(loss)
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m, (step, xs, ys) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                step(xs[i % 2], ys[i % 2])
            torch.cuda.synchronize()
            ms[m].append(1e3 * (time.perf_counter() - t0) / a.steps)
    out = {"label": a.label, "batch": a.batch, "size": a.size, "steps": a.steps, "rounds": a.rounds, "modes": {}}
    for m in modes:
        med = statistics.median(ms[m])
        out["modes"][m] = {"ms_per_step": round(med, 3), "spread": round((max(ms[m]) - min(ms[m])) / med, 4),
                           "loss_first_step": first.get(m), "loss_last_step": float(runs[m][0].last_loss)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
