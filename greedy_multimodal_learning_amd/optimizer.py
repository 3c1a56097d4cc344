"""The update of the fused training step: torch.optim.SGD (+ clip_grad_norm_) on the device.

FusedSGD owns what the norms+update pass (callbacks.GroupNorms.sums, csrc/group_sumsq.hip) needs
beyond parameters and gradients: hyper-parameters, the device-resident rate and its schedule, the
parameter-group table, the clip state, the flat momentum buffer, and the checkpoint view of all that
as a torch.optim.SGD would hold it.  The engine (engine.BalancedStep) touches it at three points:
step() launches the pass, graph_key() is the rate's part of a captured step's key, after_step()
counts the pass.  Two phases, because the engine flattens the model's parameters in between: the
constructor checks the arguments (it raises before the model is touched), attach() makes the device
state on the flat buffers, before anything is captured.
"""
import math
import struct

import torch

from . import _lib as L
from .callbacks import GroupNorms


class FusedSGD:
    def __init__(self, lr=0.1, momentum=0.0, weight_decay=0.0, lr_schedule=None, param_groups=None, nesterov=False,
                 clip_grad_norm=None, skip_nonfinite_steps=False):
        # clip_grad_norm (torch's clip_grad_norm_ max_norm, > 0) / skip_nonfinite_steps (a step whose
        # gradient's global norm is inf or NaN leaves parameters, momentum buffers and the gate alone):
        # the update runs through gm_group_sumsq_clip, which decides both on the device from a small
        # state (self.clip_state, made in attach).  skip_nonfinite_steps alone is max_norm = +inf: the
        # guard and the norm's log, no clipping.  Either implies a device rate, as the parameter
        # groups do.  Both off (the default): nothing of this exists.
        self.skip_nonfinite_steps = bool(skip_nonfinite_steps)
        self._clip_max = None if clip_grad_norm is None else float(clip_grad_norm)
        if self._clip_max is not None and not self._clip_max > 0.0:
            raise ValueError(f"BalancedStep: clip_grad_norm must be > 0 (got {clip_grad_norm!r})")
        self.clipping = self._clip_max is not None or self.skip_nonfinite_steps
        # param_groups (a param_groups.ParamGroups) / nesterov: the update runs through
        # gm_group_sumsq_pg - each parameter's rate scale and weight decay from a small device table
        # (self.pgroups, made in attach), optionally torch's Nesterov step.  Either implies a device
        # rate: without a schedule the optimizer holds one itself (kind "held", so `lr = x` stays a
        # 4-byte fill).  Both off (the default): nothing of this exists.
        self.param_groups, self.nesterov = param_groups, bool(nesterov)
        if self.nesterov and not float(momentum) > 0.0:
            raise ValueError("BalancedStep: nesterov=True requires a momentum > 0")
        if (param_groups is not None or self.nesterov or self.clipping) and lr_schedule is None:
            from .lr_schedule import LRSchedule
            lr_schedule = LRSchedule("held", lr)
        # lr_schedule (an lr_schedule.LRSchedule; None: the rate is the `lr` argument of the update
        # kernels and part of every captured graph's key): the rate lives in a device gm_lr_state
        # (self.lr_state, made in attach), the update kernels read it there and the finalize launch
        # advances it, so one captured graph serves every rate
        self.lr_schedule = lr_schedule
        self.lr_state = None
        self._lr_t = 0  # update passes applied under the schedule (host mirror of gm_lr_state.step)
        self._lr = float(lr) if lr_schedule is None else lr_schedule.base_lr  # (a schedule's base_lr replaces lr)
        # torch.optim.SGD's momentum and weight decay (dampening 0), fixed per engine; both 0 (the
        # default): the plain update, no momentum buffer
        self.momentum, self.weight_decay = float(momentum), float(weight_decay)
        for name, v in (("momentum", self.momentum), ("weight_decay", self.weight_decay)):
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"BalancedStep: {name} must be finite and >= 0 (got {v!r})")
        # the device state, made in attach: the group table (fp32 [npgroups, 2]: lr_scale, weight_decay)
        # with its host mirror, the gm_clip_state, the flat momentum buffer and its per-parameter views
        self.pgroups = self._pgroups_host = self.clip_state = self.flat_momentum = self.mom_bufs = self.norms = None

    def attach(self, model, flat, channels_last, branchnames, MMTMnames):
        """The device state, on the engine's flat buffers (`flat`, an engine.FlatParams of `model`)."""
        self.model, self.flat, self.channels_last, self.device = model, flat, channels_last, flat.device
        named = list(model.named_parameters())
        if self.param_groups is not None or self.nesterov:
            from .param_groups import ParamGroups, pack_table
            groups = self.param_groups if self.param_groups is not None else ParamGroups()
            if groups.weight_decay is not None and self.weight_decay not in (0.0, groups.weight_decay):
                raise ValueError(f"BalancedStep: weight_decay={self.weight_decay!r} and the parameter groups' "
                                 f"own default {groups.weight_decay!r} disagree")
            raw = pack_table(groups.table(self.weight_decay))  # (the library's host-side check)
            self._pgroups_host = [list(row) for row in struct.iter_unpack("ff", raw)]  # as the device holds them
            self.pgroups = torch.frombuffer(bytearray(raw), dtype=torch.float32).view(-1, 2).to(self.device)
            self.norms = GroupNorms(named, list(branchnames), list(MMTMnames), pgroup_of=groups.group_of)
        else:
            self.norms = GroupNorms(named, list(branchnames), list(MMTMnames))
        if self.lr_schedule is not None:
            self.lr_state = torch.frombuffer(bytearray(self.lr_schedule.pack(0)), dtype=torch.uint8).to(self.device)
        if self.clipping:
            raw = L.clip_state_bytes(math.inf if self._clip_max is None else self._clip_max, 1e-6,
                                     self.skip_nonfinite_steps)  # (the library's host-side check)
            self.clip_state = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
        # one flat zero momentum buffer at FlatParams' offsets (so co-aligned with the parameter
        # and gradient buffers: the fused pass keeps its 16-byte path), made here, before any
        # capture: the graph mutates it in place
        if self.momentum != 0.0:
            self.flat_momentum = torch.zeros(flat.total, device=self.device, dtype=torch.float32)
            self.mom_bufs = [self.momentum_buffer(p) for _, p in named]

    # ---------------- the engine's three calls ----------------
    def step(self, grad_scale, gate=None, gate_n=False):
        """The fused norms+update pass; returns the step's group sums (device fp64).  gate (a device
        gate state): its step rides in the same finalize launch (gm_group_sumsq_gate)."""
        kw = {}
        if self.pgroups is not None:  # gm_group_sumsq_pg: rate scale and weight decay from the group table
            kw = dict(pgroups=self.pgroups, nesterov=self.nesterov, momentum=self.momentum,
                      momentum_buffers=self.mom_bufs)
        elif self.momentum != 0.0 or self.weight_decay != 0.0:  # gm_group_sumsq_sgdm
            kw = dict(momentum=self.momentum, weight_decay=self.weight_decay, momentum_buffers=self.mom_bufs)
        if gate is not None:
            kw.update(gate=gate, gate_n=gate_n)
        if self.clip_state is not None:  # gm_group_sumsq_clip: the same update behind the clip and the skip
            kw.update(clip_state=self.clip_state)
        if self.lr_state is not None:  # gm_group_sumsq_lr: the rate is read from (and advanced in) device memory
            return self.norms.sums(grad_scale=grad_scale, lr_state=self.lr_state, **kw)
        return self.norms.sums(grad_scale=grad_scale, lr=self.lr, **kw)

    def graph_key(self):
        """The rate's part of a graph key: the rate itself when the kernels take it as an
        argument, a constant when they read it from the device state"""
        return self._lr if self.lr_state is None else "device-lr"

    def after_step(self):
        """One pass was applied (eagerly or by a replay): the host mirror of the device's pass count."""
        if self.lr_state is not None:
            self._lr_t += 1

    # ---------------- learning rate ----------------
    @property
    def lr(self):
        """The rate the next step's update uses.  Under a device-run schedule: lr_at(passes so
        far), from the host mirror of the pass count (no sync)."""
        sch = self.lr_schedule
        if sch is not None and sch.device_run:
            return sch.lr_at(self._lr_t)
        return self._lr

    @lr.setter
    def lr(self, value):
        value = float(value)
        sch = self.lr_schedule
        if sch is None:
            self._lr = value
            return
        if sch.device_run:
            raise ValueError(f"BalancedStep.lr: the {sch.kind} schedule owns the rate on the device "
                             "(set_lr_step moves it)")
        if value != self._lr:  # held: a stream-ordered fill of the state's first four bytes, no re-capture
            self.lr_state[:4].view(torch.float32).fill_(value)
            self._lr = value

    def sync_lr(self):
        """The device gm_lr_state as its ctypes mirror (LrState: lr, step, ...); one host sync,
        for tests and checkpoints.  None without a schedule."""
        if self.lr_state is None:
            return None
        from .lr_schedule import unpack
        return unpack(self.lr_state.cpu().numpy().tobytes())

    def set_lr_step(self, t):
        """A resumed run: the state of a run that has applied t update passes (step = t, lr =
        lr_at(t); held keeps its rate), written on the current stream."""
        if self.lr_state is None:
            raise ValueError("BalancedStep.set_lr_step: no lr_schedule")
        st = self.lr_schedule.struct(int(t))
        if not self.lr_schedule.device_run:
            st.lr = self._lr
        self.lr_state.copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8))
        self._lr_t = int(t)

    # ---------------- gradient clipping ----------------
    @property
    def clip_grad_norm(self):
        """The global-norm bound the next step clips to (None: no clipping)."""
        return self._clip_max

    @clip_grad_norm.setter
    def clip_grad_norm(self, value):
        if self.clip_state is None:
            raise ValueError("BalancedStep.clip_grad_norm: the engine was made without clip_grad_norm / "
                             "skip_nonfinite_steps (no clip state)")
        new = math.inf if value is None else float(value)
        if not new > 0.0:
            raise ValueError(f"BalancedStep.clip_grad_norm must be > 0 (got {value!r})")
        # a stream-ordered fill of the state's first four bytes: no re-capture, one graph for every value
        self.clip_state[:4].view(torch.float32).fill_(new)
        self._clip_max = None if value is None else new

    def sync_clip(self):
        """The device gm_clip_state as its ctypes mirror (ClipState: total_sq, coef, skipped_last,
        the counters, ...); one host sync, for tests and logs.  None without clipping."""
        if self.clip_state is None:
            return None
        return L.ClipState.from_buffer_copy(self.clip_state.cpu().numpy().tobytes())

    def momentum_buffer(self, p):
        """The momentum buffer of parameter p: a view of the flat buffer shaped and strided like
        p (a channels-last conv weight's is the same permuted view as p.data); None with
        momentum 0."""
        if self.flat_momentum is None:
            return None
        off, n = self.flat.slices[p]
        view = self.flat_momentum[off:off + n]
        if p.dim() == 4 and self.channels_last:
            O, I, kh, kw = p.shape
            return view.view(O, kh, kw, I).permute(0, 3, 1, 2)
        return view.view(p.shape)

    # ---------------- parameter groups ----------------
    def _need_groups(self, what):
        if self.pgroups is None:
            raise ValueError(f"BalancedStep.{what}: no parameter groups (param_groups=None, nesterov=False)")

    def param_group_of(self, p):
        """The group index of parameter p (a tensor of the model, or its name)."""
        self._need_groups("param_group_of")
        if isinstance(p, str):
            return self.norms.pgroup[self.norms.names.index(p)]
        for q, g in zip(self.norms.params, self.norms.pgroup):
            if q is p:
                return g
        raise KeyError("param_group_of: not a parameter of this engine's model")

    def param_group(self, i):
        """Group i as {'lr_scale', 'weight_decay', 'lr'} from the host mirror of the device table
        (no sync); lr: the group's rate at the next step, the fp64 product rounded to fp32."""
        self._need_groups("param_group")
        from .lr_schedule import _f32
        s, wd = self._pgroups_host[i]
        return {"lr_scale": s, "weight_decay": wd, "lr": _f32(_f32(self.lr) * s)}

    def set_param_group(self, i, lr_scale=None, weight_decay=None):
        """Change group i's rate scale and / or weight decay from the next step on: one
        stream-ordered 8-byte fill of the device entry, which the captured step reads - no host
        sync, no re-capture.  Under data parallelism every rank makes the same call."""
        self._need_groups("set_param_group")
        from .param_groups import _value
        i = int(i)
        if not 0 <= i < len(self._pgroups_host):
            raise IndexError(f"set_param_group: group {i} of {len(self._pgroups_host)}")
        row = self._pgroups_host[i]
        new = [row[0] if lr_scale is None else _value("lr_scale", lr_scale),
               row[1] if weight_decay is None else _value("weight_decay", weight_decay)]
        bits = struct.pack("ff", *new)  # (OverflowError beyond fp32's range)
        new = list(struct.unpack("ff", bits))  # as the device holds them: fp32
        self.pgroups.view(torch.int64)[i].fill_(struct.unpack("q", bits)[0])
        self._pgroups_host[i] = new

    def torch_param_groups(self):
        """The param groups a torch.optim.SGD over this engine's model holds: one dict per
        non-empty engine group, in group order, its parameters in model.parameters() order, with
        the group's lr (the step's rate x lr_scale), weight_decay, momentum and nesterov.  Without
        parameter groups: one group of everything.  load_optimizer_state reads a state_dict's
        parameter indices in this order."""
        params = list(self.model.parameters())
        common = {"momentum": self.momentum, "nesterov": self.nesterov}
        if self.pgroups is None:
            return [dict(common, params=params, lr=self.lr, weight_decay=self.weight_decay)]
        by_id = {id(q): g for q, g in zip(self.norms.params, self.norms.pgroup)}
        out = []
        for i, (scale, wd) in enumerate(self._pgroups_host):
            ps = [p for p in params if by_id[id(p)] == i]
            if ps:
                out.append(dict(common, params=ps, lr=self.lr * scale, weight_decay=wd))
        return out

    def load_optimizer_state(self, sd):
        """Continue from a checkpoint's 'optimizer' entry: `sd` is the state_dict() of a
        torch.optim.SGD built over torch_param_groups(), as training_loop saves it.  Every
        `momentum_buffer` is copied into the engine's flat momentum buffer (through
        momentum_buffer(p): a channels-last parameter's buffer is the channels-last view).  Raises
        ValueError - before anything is copied - on a missing or mis-shaped buffer, on groups that
        are not the engine's (sizes, indices) and on a group whose momentum, nesterov, dampening,
        weight decay or ratio of rates disagrees with the engine's.  Valid before the first step and
        between steps: captured graphs update the flat buffer in place.  The rate itself is not
        taken from `sd` (step.lr / the schedule own it)."""
        mine, theirs = self.torch_param_groups(), sd["param_groups"]
        k = 0
        for j, g in enumerate(mine):
            n = len(g["params"])
            if j >= len(theirs) or list(theirs[j]["params"]) != list(range(k, k + n)):
                raise ValueError(f"load_optimizer_state: the state_dict's param groups are not the engine's "
                                 f"(group {j}: {n} parameters from index {k})")
            k += n
        if len(theirs) != len(mine):
            raise ValueError(f"load_optimizer_state: {len(theirs)} param groups, the engine has {len(mine)}")

        def close(a, b):
            return math.isclose(float(a), float(b), rel_tol=1e-6, abs_tol=1e-12)

        base = None  # one rate behind all groups: lr_j / scale_j is the same for every j
        for j, (g, t) in enumerate(zip(mine, theirs)):
            for key in ("momentum", "weight_decay"):
                if not close(t.get(key, 0.0), g[key]):
                    raise ValueError(f"load_optimizer_state: group {j}: {key} {t.get(key)!r} != the engine's "
                                     f"{g[key]!r}")
            if bool(t.get("nesterov", False)) != self.nesterov:
                raise ValueError(f"load_optimizer_state: group {j}: nesterov {t.get('nesterov')!r} != the engine's "
                                 f"{self.nesterov!r}")
            if float(t.get("dampening", 0.0)) != 0.0:
                raise ValueError("load_optimizer_state: dampening is not supported")
            if g["lr"] > 0.0 and self.lr > 0.0:
                ratio = float(t["lr"]) / (g["lr"] / self.lr)
                base = ratio if base is None else base
                if not close(ratio, base):
                    raise ValueError(f"load_optimizer_state: group {j}: lr {t['lr']!r} is not in the engine's "
                                     f"ratio to the other groups' (base rate {base!r})")
        if self.flat_momentum is None:
            if any(st.get("momentum_buffer") is not None for st in sd["state"].values()):
                raise ValueError("load_optimizer_state: the state_dict holds momentum buffers, the engine has "
                                 "momentum 0")
            return
        params = [p for g in mine for p in g["params"]]
        bufs = []
        for k, p in enumerate(params):
            b = sd["state"].get(k, {}).get("momentum_buffer")
            if b is None:
                raise ValueError(f"load_optimizer_state: no momentum_buffer for parameter {k}")
            if tuple(b.shape) != tuple(p.shape):
                raise ValueError(f"load_optimizer_state: parameter {k}: momentum_buffer of shape {tuple(b.shape)} "
                                 f"for a parameter of shape {tuple(p.shape)}")
            bufs.append(b)
        with torch.no_grad():
            for p, b in zip(params, bufs):
                self.momentum_buffer(p).copy_(b.to(device=self.device, dtype=torch.float32))
