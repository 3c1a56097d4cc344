"""Record the bits of the fused norms+SGD pass: every entry point x update form the library exposes,
three passes each, on the two small parameter sets of tests/test_gpu_sgdm.py.

    python tools/record_group_pass_bits.py [--out tests/golden/group_pass_bits.json]

Uses GroupNorms.sums and _lib alone, so the same file runs against any tree that has the six
gm_group_sumsq* entries.  tests/test_gpu_group_pass_bits.py imports the cases and run_case() from
here and asserts equality with the committed recording: a change of the pass's kernels that moves
one bit of any parameter, momentum buffer, returned sum or device state fails there.

A case's record is three SHA-256 digests, one after each pass, over the raw bytes of the
parameters, the momentum buffers (where the form has them), the returned fp64 sums and the gate,
rate and clip states (where the entry takes them), in that order.  Inputs come from seeded CPU
generators and are moved to the device: one start value per tensor and one gradient per tensor and
pass, shared by every case of a set.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PASSES = 3
GRAD_SCALE = 0.5
LR, MU, WD = 0.1, 0.9, 5e-4
TABLE = [(1.0, 5e-4), (0.3, 0.0), (2.5, 1e-2)]  # (lr_scale, weight_decay) of three parameter groups
SENTINEL = 7.25
# randn gradients at grad_scale 0.5: the norm is ~140 on the eight-tensor set and ~92 on the
# twelve-branch one, so 1.0 clips every pass and 1e6 none
CLIPS, NO_CLIP = 1.0, 1.0e6
INF_PASS = 1  # the pass (0-based) whose gradient holds an inf in the `inf` conditions


def _eight():
    """78 011 elements in 8 tensors: five workgroups at the 16 384-element chunk, 4 groups (the
    <= 8-group body), tensors of 1, 7, 15 and 16 elements (scalar head, scalar tail, the short
    vector loops) and a 40 000-element tensor across chunk boundaries.  The parameter groups put
    consecutive tensors into different groups."""
    shapes = {"net_view_0.a": (3, 5), "net_view_0.b": (40000,), "net_view_1.c": (7,),
              "net_view_1.d": (100, 333), "mmtm2.fc_squeeze.weight": (16, 32),
              "mmtm2.fc_visual.bias": (16,), "mmtm3.fc_skeleton.weight": (64, 65),
              "net_view_1.e": (1,)}
    return dict(shapes=shapes, names=(["net_view_0", "net_view_1"], ["visual", "skeleton"]),
                assign=dict(zip(shapes, (0, 1, 2, 0, 1, 2, 0, 1))), nograd="net_view_1.d", gate_nb=None, seed=101)


def _twelve():
    """12 branches: 24 groups (the run body), 33 792 elements in three workgroups"""
    V = 12
    shapes = {}
    for i in range(V):
        shapes[f"net_view_{i}.conv.weight"] = (64, 3, 3, 3)
        shapes[f"net_view_{i}.bn.bias"] = (64,)
        shapes[f"mmtm4.fc_excite.{i}.weight"] = (32, 16)
    shapes["mmtm4.fc_squeeze.weight"] = (16, 384)
    return dict(shapes=shapes, names=([f"net_view_{i}" for i in range(V)], [f"fc_excite.{i}." for i in range(V)]),
                assign={n: i % 3 for i, n in enumerate(shapes)}, nograd="net_view_3.conv.weight", gate_nb=V, seed=202)


SETS = {"eight": _eight, "twelve": _twelve}


def cases():
    """{case id: spec}.  A spec: set, entry, the update's hyper-parameters (lr: the scalar rate of
    the three scalar-rate entries), gate, variant (None / "skew": buffers off by 4 bytes, the
    scalar path / "nograd": one entry without a gradient) and, for the clipped entry, the condition."""
    out = {}

    def add(which, entry, form, variants=(None,), cond=None, **spec):
        for v in variants:
            cid = "-".join(str(s) for s in (which, entry, form, cond, v) if s is not None)
            out[cid] = dict(spec, set=which, entry=entry, variant=v, cond=cond)

    mom_variants = (None, "skew", "nograd")
    for which in SETS:
        add(which, "sumsq", "none", lr=0.0)
        add(which, "sumsq", "sgd", lr=LR)
        add(which, "gate", "none", lr=0.0, gate=True)
        add(which, "gate", "sgd", lr=LR, gate=True)
        add(which, "sgdm", "decay", lr=LR, wd=WD)
        add(which, "sgdm", "mom", mom_variants, lr=LR, mu=MU, wd=WD, gate=True)
        add(which, "lr", "sgd", gate=True)
        add(which, "lr", "decay", wd=WD, gate=True)
        add(which, "lr", "mom", mom_variants, mu=MU, wd=WD, gate=True)
        add(which, "pg", "decay", pg=True, gate=True)
        add(which, "pg", "mom", mom_variants, pg=True, mu=MU, gate=True)
        add(which, "pg", "nest", mom_variants, pg=True, mu=MU, nest=True, gate=True)
        for cond in ("clips", "noclip", "inf_skip", "inf_noskip"):
            add(which, "clip", "sgd", cond=cond, gate=True)
            add(which, "clip", "decay", cond=cond, wd=WD, gate=True)
            add(which, "clip", "mom", mom_variants, cond=cond, mu=MU, wd=WD, gate=True)
            add(which, "clip", "nest_pg", mom_variants, cond=cond, pg=True, mu=MU, nest=True, gate=True)
    return out


_inputs = {}


def inputs(which):
    """The set's description with its start values and per-pass gradients (CPU, made once, never
    written) and the inf-holding copy of pass INF_PASS's gradients"""
    import torch
    if which not in _inputs:
        s = SETS[which]()
        g = torch.Generator().manual_seed(s["seed"])
        s["start"] = {n: torch.randn(*shape, generator=g) for n, shape in s["shapes"].items()}
        s["grads"] = [{n: torch.randn(*shape, generator=g) for n, shape in s["shapes"].items()} for _ in range(PASSES)]
        bad = {n: t.clone() for n, t in s["grads"][INF_PASS].items()}
        first = next(iter(bad))
        bad[first].view(-1)[bad[first].numel() // 2] = float("inf")
        s["grads_inf"] = bad
        _inputs[which] = s
    return _inputs[which]


def _state(dev, raw):
    import torch
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)


def _gate_state(dev, nb):
    from greedy_multimodal_learning_amd import _lib as L
    st = L.GateState() if nb is None else L.GateStateN()
    if nb is not None:
        st.nb = nb
    st.caring, st.window, st.eps = -1, 2, 2e-3
    return _state(dev, bytes(st))


def _lr_state(dev):
    """multistep from 0.1, gamma 0.1, one milestone at pass 2: inside the three passes"""
    from greedy_multimodal_learning_amd import _lib as L
    st = L.LrState(lr=LR, kind=1, step=0, base_lr=LR, gamma=0.1, n_milestones=1)
    st.milestones[0] = 2
    out = ctypes.c_float()
    L.check(L.load().gm_lr_at(ctypes.addressof(st), 0, ctypes.addressof(out)), "gm_lr_at")  # (the host-side check)
    st.lr = out.value
    return _state(dev, bytes(st))


def run_case(dev, spec):
    """The case's PASSES digests (hex)"""
    import torch
    from greedy_multimodal_learning_amd import _lib as L
    from greedy_multimodal_learning_amd.callbacks import GroupNorms
    s = inputs(spec["set"])
    variant, mu = spec["variant"], spec.get("mu", 0.0)
    nograd = (s["nograd"],) if variant == "nograd" else ()
    params = [(n, torch.nn.Parameter(w.to(dev))) for n, w in s["start"].items()]
    bufs = None
    if mu != 0.0:
        bufs = []
        for n, p in params:
            big = torch.zeros(p.numel() + 1, device=dev)
            b = big[1:].view(p.shape) if variant == "skew" else big[:-1].view(p.shape)
            assert (b.data_ptr() - p.data_ptr()) % 16 == (4 if variant == "skew" else 0)
            if n in nograd:
                b.fill_(SENTINEL)
            bufs.append(b)
    pg = spec.get("pg", False)
    gn = GroupNorms(params, *s["names"], pgroup_of=s["assign"].__getitem__ if pg else None)
    kw = dict(grad_scale=GRAD_SCALE, momentum=mu, momentum_buffers=bufs)
    states = []
    if spec.get("gate"):
        kw.update(gate=_gate_state(dev, s["gate_nb"]), gate_n=s["gate_nb"] is not None)
        states.append(kw["gate"])
    if spec["entry"] in ("lr", "pg", "clip"):
        kw.update(lr_state=_lr_state(dev))
        states.append(kw["lr_state"])
    else:
        kw.update(lr=spec["lr"])
    if pg:
        kw.update(pgroups=torch.tensor(TABLE, dtype=torch.float32, device=dev).reshape(-1, 2))
    else:
        kw.update(weight_decay=spec.get("wd", 0.0))
    kw.update(nesterov=spec.get("nest", False))
    cond = spec["cond"]
    if cond is not None:
        raw = L.clip_state_bytes(CLIPS if cond == "clips" else NO_CLIP, 1e-6, cond == "inf_skip")
        kw.update(clip_state=_state(dev, raw))
        states.append(kw["clip_state"])
    digests = []
    for k in range(PASSES):
        grads = s["grads_inf"] if (cond or "").startswith("inf") and k == INF_PASS else s["grads"][k]
        for n, p in params:
            p.grad = None if n in nograd else grads[n].to(dev)
        out = gn.sums(**kw)
        h = hashlib.sha256()
        with torch.no_grad():
            h.update(torch.cat([p.reshape(-1) for _, p in params]).cpu().numpy().tobytes())
            if bufs is not None:
                h.update(torch.cat([b.reshape(-1) for b in bufs]).cpu().numpy().tobytes())
        h.update(out.cpu().numpy().tobytes())
        for st in states:
            h.update(st.cpu().numpy().tobytes())
        digests.append(h.hexdigest())
    return digests


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("tests", "golden", "group_pass_bits.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("record_group_pass_bits: needs a HIP device")
    dev = torch.device("cuda:0")
    rec = {cid: run_case(dev, spec) for cid, spec in cases().items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cases x {PASSES} passes to {a.out}")


if __name__ == "__main__":
    main()
