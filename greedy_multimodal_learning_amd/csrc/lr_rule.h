// The device-resident learning rate's schedule rule (gm_lr_state, greedymml.h) as one function of
// the pass index, shared by the host (gm_lr_at) and the device: thread 0 of k_group_finalize
// (group_sumsq.hip) advances the state behind each update pass, so the rate never is a kernel
// argument and one captured step serves every rate.  fp64 throughout, one rounding to fp32.
#pragma once
#include <cmath>

#include "gm_common.h"

namespace gm {

constexpr int kLrHeld = 0, kLrMultistep = 1, kLrCosine = 2;

// The rate update pass t (0-based) reads.  Safe for any struct contents: the milestone loop has a
// constant bound, nothing is indexed by a value from memory, and a bad kind is held (a division
// by zero gives a non-finite rate, never a fault).  gm_lr_at refuses such states on the host.
__host__ __device__ inline float lr_rule(const gm_lr_state& s, long long t) {
    const long long W = s.warmup_steps, T = s.total_steps;
    const double w = (W > 0 && t < W) ? s.warmup_start + (1.0 - s.warmup_start) * ((double)t / (double)W) : 1.0;
    if (s.kind == kLrMultistep) {
        const int n = s.n_milestones < 0 ? 0 : (s.n_milestones > GM_LR_MAX_MILESTONES ? GM_LR_MAX_MILESTONES
                                                                                       : s.n_milestones);
        double f = 1.0;
#pragma unroll
        for (int i = 0; i < GM_LR_MAX_MILESTONES; ++i)
            if (i < n && t >= s.milestones[i]) f *= s.gamma;  // listed twice counts twice (MultiStepLR)
        return (float)((s.base_lr * w) * f);
    }
    if (s.kind == kLrCosine) {
        if (t < W) return (float)(s.base_lr * w);
        const long long tt = t < T ? t : T;
        const double c = cos(3.14159265358979323846 * (double)(tt - W) / (double)(T - W));
        return (float)(s.min_lr + (s.base_lr - s.min_lr) * (0.5 * (1.0 + c)));
    }
    return s.lr;  // held: the host sets it
}

// One update pass has run: step = t = step + 1 and, unless held, lr = rule(t).  One thread, plain
// stores.
__device__ inline void lr_advance(gm_lr_state* st) {
    const long long t = st->step + 1;
    st->step = t;
    if (st->kind == kLrMultistep || st->kind == kLrCosine) st->lr = lr_rule(*st, t);
}

}  // namespace gm
