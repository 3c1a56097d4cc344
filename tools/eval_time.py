"""Time of one evaluation pass, module path against fused path (engine.EvalStep), at the
benchmark's shapes: train.evaluate(model, loader, ...) and train.evaluate(..., engine=step) run
alternately in one process over the same resident batches (round r: one pass of each, wall clock
around a device sync), after warm-up passes of both (the fused path's first pass runs eagerly,
its second captures the batch's hipGraph).  Prints one JSON line per workload: per path the
median ms per batch over the rounds with min and max, both passes' loss and accuracy (same
weights, same batches: they must agree within the bf16 bar's effect), and whether the fused
path is faster by more than the spread - the larger (max - min) of the two.

    python tools/eval_time.py [--workloads C2,C4,C5] [--batches 8] [--rounds 5] [--warmup 2]
                              [--size 224] [--eager] [--label TEXT] [--f32 [--contractions exact,bf16x3,bf16x6]]

C2: 2 x ResNet-18, B = 64; C4: 4 x ResNet-18, B = 64; C5: 12 x ResNet-50, B = 32 (bench.py's
workloads), bf16, the loader's view-major channels_last input layout.  No GPU, no number: the
tool fails without a HIP device.

--f32: the fp32 evaluation pass instead - the fp32 module path against EvalStep(torch.float32,
f32_trunk="fused") (BatchNorm, residual and ReLU in the fp32 convolution epilogues), one line per
contraction mode (conv.set_f32_contraction on the same model and batches, the two paths
alternating within each mode).  The two paths compute the same bits, so each line also says
whether the two passes' losses and accuracies agree ("same_metrics": loss within 1e-6 relative -
a device fp64 sum against a host float sum - and equal accuracy).
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

WORKLOADS = {"C2": dict(views=2, trunk="resnet18", batch=64), "C4": dict(views=4, trunk="resnet18", batch=64),
             "C5": dict(views=12, trunk="resnet50", batch=32)}


def make(name, size, nbatches, dev, batch=None, dtype=torch.bfloat16):
    from greedy_multimodal_learning_amd.bn import GMBatchNorm2d
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN, MMTM_MVCNN_N
    w = WORKLOADS[name]
    B = batch or w["batch"]
    torch.manual_seed(0)
    model = (MMTM_MVCNN() if name == "C2" else MMTM_MVCNN_N(num_views=w["views"], trunk=w["trunk"])).to(dev)
    g = torch.Generator(device=dev).manual_seed(1000)
    with torch.no_grad():  # running statistics as after training, not the initial 0 / 1
        for m in model.modules():
            if isinstance(m, GMBatchNorm2d):
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, device=dev, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, device=dev, generator=g))
    loader = []
    for i in range(nbatches):
        x = torch.randn(w["views"], B, size, size, 3, device=dev, generator=g).to(dtype).permute(1, 0, 4, 2, 3)
        y = torch.randint(0, 40, (B,), device=dev, generator=g)
        loader.append((torch.arange(i * B, (i + 1) * B), x, y))
    return model, loader


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C2")
    ap.add_argument("--batches", type=int, default=8, help="resident batches per pass")
    ap.add_argument("--batch", type=int, default=None, help="batch size (default: the workload's)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--eager", action="store_true", help="no hipGraph capture of the fused batch")
    ap.add_argument("--label", default="", help="copied into the output line (which tree, which run)")
    ap.add_argument("--f32", action="store_true", help="the fp32 pass: module path against f32_trunk='fused'")
    ap.add_argument("--contractions", default="exact,bf16x3,bf16x6", help="--f32: the contraction modes to time")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("eval_time.py: no HIP device (a pass is only timed on the GPU)")
    from greedy_multimodal_learning_amd.engine import EvalStep
    from greedy_multimodal_learning_amd.train import evaluate
    from greedy_multimodal_learning_amd.conv import set_f32_contraction
    dev = torch.device("cuda:0")
    BF = torch.float32 if a.f32 else torch.bfloat16  # the pass's compute dtype
    cases = [(n, c) for n in a.workloads.split(",") for c in (a.contractions.split(",") if a.f32 else [None])]
    for name, contraction in cases:
        model, loader = make(name, a.size, a.batches, dev, a.batch, BF)
        if a.f32:
            set_f32_contraction(model, contraction, BF)
        step = EvalStep(model, compute_dtype=BF, graphs=not a.eager, f32_trunk="fused" if a.f32 else "modules")
        paths = {"modules": lambda: evaluate(model, loader, "val", BF),
                 "fused": lambda: evaluate(model, loader, "val", BF, engine=step)}
        logs = {}
        for _ in range(a.warmup):
            for k, run in paths.items():
                logs[k] = run()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k, run in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                logs[k] = run()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3 / len(loader))
        out = {"tool": "eval_time", "label": a.label, "workload": name, "batch": len(loader[0][2]), "size": a.size,
               "batches_per_pass": len(loader), "rounds": a.rounds, "graphs": bool(step.graphs),
               "graph_replays": step.replays, "capture_failures": step.capture_failures}
        if a.f32:
            out.update(compute_dtype="fp32", f32_contraction=contraction, f32_trunk="fused", warmup=a.warmup)
        for k, ts in times.items():
            out[k] = {"ms_per_batch_median": round(statistics.median(ts), 4), "min": round(min(ts), 4),
                      "max": round(max(ts), 4), "val_loss": float(logs[k]["val_loss"]),
                      "val_acc": float(logs[k]["val_acc"])}
        spread = max(max(ts) - min(ts) for ts in times.values())
        gain = out["modules"]["ms_per_batch_median"] - out["fused"]["ms_per_batch_median"]
        out["spread_ms"] = round(spread, 4)
        out["fused_faster_by_more_than_spread"] = bool(gain > spread)
        out["speedup"] = round(out["modules"]["ms_per_batch_median"] / out["fused"]["ms_per_batch_median"], 3)
        if a.f32:
            lm, lf = out["modules"]["val_loss"], out["fused"]["val_loss"]
            out["same_metrics"] = bool(abs(lm - lf) <= 1e-6 * abs(lm)
                                       and abs(out["modules"]["val_acc"] - out["fused"]["val_acc"]) <= 1e-4)
        print(json.dumps(out), flush=True)
        del model, loader, step, paths
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
