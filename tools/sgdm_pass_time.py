"""Time the norms+update pass in its three forms at the C2 parameter set (MMTM_MVCNN, 2 views:
23,773,008 elements in the engine's flat buffers): the plain update (gm_group_sumsq, 12 B per
element), weight decay alone (gm_group_sumsq_sgdm without buffers, 12 B) and momentum + weight
decay (20 B), each next to its device-rate sibling (`*_dlr`: gm_group_sumsq_lr, the rate read
from a held gm_lr_state holding the same value; `dlr_minus_scalar_us`: the pair's difference of
medians, to be read against the larger of the pair's spreads).  One process, the forms
interleaved launch by launch within a round, HIP events around each launch pair (pass +
finalize) behind a device sleep, as bench.time_group_sumsq does; prints one JSON line: per form
the median over rounds of the round's mean, the spread over the rounds, and the achieved bytes/s
against the 8.0 TB/s HBM3E peak.

    python tools/sgdm_pass_time.py [--rounds 7] [--launches 20] [--swap] [--groups | --clip] [--out FILE]

A launch's time depends on what the launch before it left in the caches (the momentum forms touch
a third 95 MB buffer).  --swap runs each pair device-rate first on every other launch, so both
members of a pair follow the same predecessors equally often.

--groups times the parameter-group forms (gm_group_sumsq_pg) instead, each launch-paired with the
device-rate momentum form (`momentum_dlr`, 20 B per element like all of them): momentum and
Nesterov over a one-group table (1, 5e-4) (`*_pg1`) and over ParamGroups.no_decay_norm_bias(5e-4)
(`*_ndnb`: two groups, the index changing from tensor to tensor); `pg_minus_dlr_us`: the pair's
difference of medians, against the larger of the pair's spreads.

--clip times the clipped forms (gm_group_sumsq_clip: a sums launch, the finalize, an apply launch;
20 B per element, 28 B with buffers) launch by launch next to their unclipped siblings: the plain
and the momentum device-rate forms and Nesterov over no_decay_norm_bias (`*_clip`).  The bound (1.0,
a fifth of this gradient's norm) clips every pass.  `clip_minus_unclipped_us`: the pair's difference
of medians, against the larger of the pair's spreads.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--swap", action="store_true", help="alternate the order within each scalar / device-rate pair")
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--groups", action="store_true", help="the parameter-group forms against momentum_dlr")
    mode.add_argument("--clip", action="store_true", help="the clipped forms against their unclipped siblings")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from greedy_multimodal_learning_amd.engine import BalancedStep
    from greedy_multimodal_learning_amd.model import MMTM_MVCNN
    if not torch.cuda.is_available():
        raise SystemExit("sgdm_pass_time: needs a HIP device (no CPU timing)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    st = BalancedStep(MMTM_MVCNN().to(dev), lr=1e-4, momentum=0.9, weight_decay=5e-4)
    st.flat.grad.normal_(generator=torch.Generator(device=dev).manual_seed(1)).mul_(1e-3)
    n = st.flat.total
    forms = {
        "plain": (12, dict()),
        "weight_decay": (12, dict(weight_decay=5e-4)),
        "momentum": (20, dict(momentum=0.9, weight_decay=5e-4, momentum_buffers=st._mom_bufs)),
    }
    from greedy_multimodal_learning_amd.lr_schedule import LRSchedule
    state = torch.frombuffer(bytearray(LRSchedule("held", st.lr).pack()), dtype=torch.uint8).to(dev)
    scalar = list(forms)
    forms = {k + suffix: (bpe, dict(kw, **extra)) for k, (bpe, kw) in forms.items()
             for suffix, extra in (("", dict(lr=st.lr)), ("_dlr", dict(lr_state=state)))}
    norms_of, pairs = {}, None
    if a.groups:
        from greedy_multimodal_learning_amd.callbacks import GroupNorms
        from greedy_multimodal_learning_amd.param_groups import ParamGroups
        ndnb = ParamGroups.no_decay_norm_bias(5e-4)
        named = list(st.model.named_parameters())
        grouped = GroupNorms(named, ["net_view_0", "net_view_1"], ["visual", "skeleton"], pgroup_of=ndnb.group_of)
        tables = {"pg1": torch.tensor([[1.0, 5e-4]], device=dev), "ndnb": torch.tensor(ndnb.table(), device=dev)}
        base = forms["momentum_dlr"]
        forms = {"momentum_dlr": base}
        for tab, norms in (("pg1", st.norms), ("ndnb", grouped)):
            for name, nest in (("momentum", False), ("nesterov", True)):
                k = f"{name}_{tab}"
                forms[k] = (20, dict(momentum=0.9, momentum_buffers=st._mom_bufs, lr_state=state, pgroups=tables[tab],
                                     nesterov=nest))
                norms_of[k] = norms
        pairs = [("momentum_dlr", k) for k in forms if k != "momentum_dlr"]
        res_extra = {"tensors_in_group_1": sum(grouped.pgroup), "tensors": len(grouped.pgroup)}
    if a.clip:
        from greedy_multimodal_learning_amd import _lib as L
        from greedy_multimodal_learning_amd.callbacks import GroupNorms
        from greedy_multimodal_learning_amd.param_groups import ParamGroups
        ndnb = ParamGroups.no_decay_norm_bias(5e-4)
        grouped = GroupNorms(list(st.model.named_parameters()), ["net_view_0", "net_view_1"], ["visual", "skeleton"],
                             pgroup_of=ndnb.group_of)
        clip = torch.frombuffer(bytearray(L.clip_state_bytes(1.0)), dtype=torch.uint8).to(dev)
        mom = dict(momentum=0.9, momentum_buffers=st._mom_bufs, lr_state=state)
        base = {"plain": (12, dict(lr_state=state)), "momentum": (20, dict(mom, weight_decay=5e-4)),
                "nesterov_ndnb": (20, dict(mom, pgroups=torch.tensor(ndnb.table(), device=dev), nesterov=True))}
        forms, pairs = {}, []
        for k, (bpe, kw) in base.items():
            forms[k] = (bpe, kw)
            forms[k + "_clip"] = (bpe + 8, dict(kw, clip_state=clip))
            pairs.append((k, k + "_clip"))
        norms_of = {k: grouped for k in forms if k.startswith("nesterov_ndnb")}
    stream = torch.cuda.current_stream()
    for k, (_, kw) in forms.items():  # warm up every form
        for _ in range(3):
            norms_of.get(k, st.norms).sums(**kw)
    means = {k: [] for k in forms}
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        torch.cuda._sleep(50_000_000)
        evs = {k: [] for k in forms}
        for li in range(a.launches):
            order = list(forms) if pairs is None else [k for pair in pairs for k in pair]
            if a.swap and li % 2:
                order = [k for i in range(0, len(order), 2) for k in (order[i + 1], order[i])]
            for k in order:
                kw = forms[k][1]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                norms_of.get(k, st.norms).sums(**kw)
                e1.record(stream)
                evs[k].append((e0, e1))
        torch.cuda.synchronize()
        for k in forms:
            means[k].append(sum(x.elapsed_time(y) for x, y in evs[k]) / len(evs[k]) * 1e3)  # us
    res = {"elements": n, "rounds": a.rounds, "launches_per_round": a.launches, "swap": a.swap}
    for k, (bpe, _) in forms.items():
        med = statistics.median(means[k])
        res[k] = {"us": round(med, 2), "spread_us": round(max(means[k]) - min(means[k]), 2),
                  "bytes": bpe * n, "tb_per_s": round(bpe * n / (med * 1e-6) / 1e12, 3),
                  "hbm_peak_fraction": round(bpe * n / (med * 1e-6) / HBM_PEAK, 3)}
    if a.clip:
        for k, c in pairs:
            res[c]["clip_minus_unclipped_us"] = round(res[c]["us"] - res[k]["us"], 2)
        st_clip = L.ClipState.from_buffer_copy(clip.cpu().numpy().tobytes())
        res["clip"] = {"max_norm": st_clip.max_norm, "coef": st_clip.coef, "steps": st_clip.steps,
                       "clipped": st_clip.clipped}
    elif pairs is None:
        res["momentum_over_plain"] = round(res["momentum"]["us"] / res["plain"]["us"], 3)
        for k in scalar:
            res[k + "_dlr"]["dlr_minus_scalar_us"] = round(res[k + "_dlr"]["us"] - res[k]["us"], 2)
    else:
        res.update(res_extra)
        for _, k in pairs:
            res[k]["pg_minus_dlr_us"] = round(res[k]["us"] - res["momentum_dlr"]["us"], 2)
    assert torch.isfinite(st.flat.param).all() and torch.isfinite(st.flat_momentum).all()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
