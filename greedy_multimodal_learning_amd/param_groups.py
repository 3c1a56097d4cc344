"""Parameter groups of the fused norms+SGD pass (gm_group_sumsq_pg, include/greedymml.h).

`ParamGroups(rules)` maps parameter names to group indices by substring, the reference's own
grouping idiom (src/callbacks.py:207-223: `if modal in name`): `rules` is a sequence of
`(substrings, lr_scale, weight_decay)`; a name belongs to the first rule one of whose substrings it
contains and gets group `1 + that rule's index`; every other name is group 0, with lr_scale 1 and
the engine's weight decay.  A group's rate is the step's rate times its lr_scale; its weight decay
is its own.  At most GM_SGD_MAX_PGROUPS groups (group 0 included).
"""
import ctypes
import math

SGD_MAX_PGROUPS = 16  # GM_SGD_MAX_PGROUPS (_lib.SGD_MAX_PGROUPS)

# torchvision ResNet BatchNorm parameters (the stem's and the blocks' bn1..bn3, the down-sampling
# path's second module) and every bias (the heads' fc, the MMTM sites' FCs)
_NORM_BIAS = ("bn1.", "bn2.", "bn3.", "downsample.1.", ".bias")


class ParamGroups:
    def __init__(self, rules=(), weight_decay=None):
        """weight_decay: group 0's (None: the engine's `weight_decay`)"""
        self.rules = []
        for rule in rules:
            if len(rule) != 3:
                raise ValueError(f"ParamGroups: a rule is (substrings, lr_scale, weight_decay) (got {rule!r})")
            subs, scale, wd = rule
            subs = (subs,) if isinstance(subs, str) else tuple(subs)
            if not subs or not all(isinstance(s, str) and s for s in subs):
                raise ValueError(f"ParamGroups: a rule needs non-empty substrings (got {rule[0]!r})")
            self.rules.append((subs, _value("lr_scale", scale), _value("weight_decay", wd)))
        if 1 + len(self.rules) > SGD_MAX_PGROUPS:
            raise ValueError(f"ParamGroups: at most {SGD_MAX_PGROUPS} groups, the default group included "
                             f"(got {1 + len(self.rules)})")
        self.weight_decay = None if weight_decay is None else _value("weight_decay", weight_decay)

    @classmethod
    def no_decay_norm_bias(cls, weight_decay):
        """The standard ResNet recipe: `weight_decay` on the convolution and FC weights (group 0),
        none on the BatchNorm weights and biases and on the other biases (group 1)."""
        return cls([(_NORM_BIAS, 1.0, 0.0)], weight_decay=weight_decay)

    @property
    def ngroups(self):
        return 1 + len(self.rules)

    def group_of(self, name):
        """The group index of a parameter name: first matching rule + 1, else 0"""
        for i, (subs, _, _) in enumerate(self.rules):
            if any(s in name for s in subs):
                return i + 1
        return 0

    def table(self, weight_decay=0.0):
        """[(lr_scale, weight_decay)] per group; weight_decay: the engine's, for group 0 unless the
        groups carry their own"""
        wd0 = self.weight_decay if self.weight_decay is not None else _value("weight_decay", weight_decay)
        return [(1.0, wd0)] + [(s, wd) for _, s, wd in self.rules]

    def pack(self, weight_decay=0.0):
        """The gm_sgd_pgroup array's bytes, checked by the library (gm_sgd_pgroups_check)"""
        return pack_table(self.table(weight_decay))


def _value(name, v):
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"ParamGroups: {name} must be finite and >= 0 (got {v!r})")
    return v


def pack_table(table):
    """[(lr_scale, weight_decay)] as a gm_sgd_pgroup array's bytes (fp32), after the library's
    host-side check: 1..GM_SGD_MAX_PGROUPS entries, every value finite and >= 0."""
    from . import _lib as L
    arr = (L.SgdPGroup * len(table))(*[L.SgdPGroup(float(s), float(wd)) for s, wd in table])
    L.check(L.load().gm_sgd_pgroups_check(ctypes.cast(arr, ctypes.c_void_p) if len(table) else None, len(table)),
            "gm_sgd_pgroups_check")
    return bytes(arr)


def from_config(value, weight_decay):
    """training_loop.param_groups as a ParamGroups: None, the string "no_decay_norm_bias" (with the
    optimizer's weight decay) or a tuple of (substrings, lr_scale, weight_decay) triples."""
    if value is None or isinstance(value, ParamGroups):
        return value
    if isinstance(value, str):
        if value != "no_decay_norm_bias":
            raise ValueError(f"param_groups: the only named recipe is 'no_decay_norm_bias' (got {value!r})")
        return ParamGroups.no_decay_norm_bias(weight_decay)
    return ParamGroups(value)
