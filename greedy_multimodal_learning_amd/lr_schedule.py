"""Learning-rate schedules that run on the device (gm_lr_state, include/greedymml.h).

`LRSchedule` holds a schedule's parameters, restates the rule of csrc/lr_rule.h in Python
(`lr_at`: fp64 with one rounding to fp32) and packs the device struct (`pack`).  The engine
(BalancedStep(lr_schedule=...)) puts the packed state in device memory once; the update kernels
read the rate from it and the finalize launch advances it, so one captured step serves every
rate.  All counts are update passes (optimizer steps), 0-based: `lr_at(t)` is the rate pass t
reads.
"""
import ctypes
import math
import struct

from . import _lib as L

KINDS = {"held": 0, "multistep": 1, "cosine": 2}


def _f32(v):
    """v rounded to fp32 (round to nearest even), as a Python float"""
    return struct.unpack("f", struct.pack("f", v))[0]


class LRSchedule:
    """kind "held": the rate is base_lr until the host writes another (BalancedStep.lr = ...);
    "multistep": base_lr * gamma^(milestones reached), a milestone listed twice counting twice
    (torch.optim.lr_scheduler.MultiStepLR); "cosine": from base_lr to min_lr over passes
    warmup_steps .. total_steps (CosineAnnealingLR), min_lr from then on.  warmup_steps > 0: the
    first passes ramp linearly from warmup_start * base_lr to base_lr (multistep, cosine)."""

    def __init__(self, kind, base_lr, warmup_steps=0, warmup_start=0.0, milestones=(), gamma=0.1, total_steps=None,
                 min_lr=0.0):
        if kind not in KINDS:
            raise ValueError(f"LRSchedule: kind must be one of {sorted(KINDS)} (got {kind!r})")
        self.kind = kind
        self.base_lr, self.min_lr = float(base_lr), float(min_lr)
        self.gamma, self.warmup_start = float(gamma), float(warmup_start)
        self.warmup_steps = int(warmup_steps)
        self.milestones = tuple(int(m) for m in milestones)
        self.total_steps = 0 if total_steps is None else int(total_steps)
        for name in ("base_lr", "min_lr", "gamma", "warmup_start"):
            v = getattr(self, name)
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"LRSchedule: {name} must be finite and >= 0 (got {v!r})")
        if self.warmup_steps < 0:
            raise ValueError("LRSchedule: warmup_steps must be >= 0")
        if len(self.milestones) > L.LR_MAX_MILESTONES:
            raise ValueError(f"LRSchedule: at most {L.LR_MAX_MILESTONES} milestones (got {len(self.milestones)})")
        if kind == "cosine" and (total_steps is None or self.total_steps <= self.warmup_steps):
            raise ValueError("LRSchedule: cosine needs total_steps > warmup_steps")

    @property
    def device_run(self):
        """True when the device advances the rate (every kind but held)"""
        return self.kind != "held"

    def params(self):
        """The constructor's arguments as a dict (what a checkpoint records)"""
        return dict(kind=self.kind, base_lr=self.base_lr, warmup_steps=self.warmup_steps,
                    warmup_start=self.warmup_start, milestones=list(self.milestones), gamma=self.gamma,
                    total_steps=self.total_steps if self.kind == "cosine" else None, min_lr=self.min_lr)

    def lr_at(self, t):
        """The rate update pass t reads (held: base_lr, the rate before any host write)"""
        t = int(t)
        if t < 0:
            raise ValueError("LRSchedule.lr_at: pass index must be >= 0")
        W, s, T = self.warmup_steps, self.warmup_start, self.total_steps
        w = s + (1.0 - s) * (t / W) if (W > 0 and t < W) else 1.0
        if self.kind == "multistep":
            f = 1.0
            for m in self.milestones:
                if t >= m:
                    f *= self.gamma
            return _f32((self.base_lr * w) * f)
        if self.kind == "cosine":
            if t < W:
                return _f32(self.base_lr * w)
            tt = min(t, T)
            c = math.cos(math.pi * (tt - W) / (T - W))
            return _f32(self.min_lr + (self.base_lr - self.min_lr) * (0.5 * (1.0 + c)))
        return _f32(self.base_lr)

    def struct(self, step=0):
        """The gm_lr_state (ctypes mirror) of a run that has applied `step` passes"""
        st = L.LrState()
        st.lr, st.kind, st.step = self.lr_at(step), KINDS[self.kind], int(step)
        st.base_lr, st.min_lr, st.gamma, st.warmup_start = self.base_lr, self.min_lr, self.gamma, self.warmup_start
        st.warmup_steps, st.total_steps = self.warmup_steps, self.total_steps
        st.n_milestones = len(self.milestones)
        for i, m in enumerate(self.milestones):
            st.milestones[i] = m
        return st

    def pack(self, step=0):
        """The struct's bytes with lr = lr_at(step)"""
        return bytes(self.struct(step))


def unpack(raw):
    """An LrState from the struct's bytes"""
    return L.LrState.from_buffer_copy(bytes(raw)[:ctypes.sizeof(L.LrState)])
