// The global-norm gradient clip's rule (gm_clip_state, greedymml.h) as one function of the step's
// total sum of squares, shared by the host (gm_clip_coef) and the device: thread 0 of
// k_group_finalize (group_sumsq.hip) evaluates it between the sums launch and the apply launch
// of gm_group_sumsq_clip.  torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): fp64
// throughout, one rounding to fp32.
#pragma once
#include <cmath>

#include "gm_common.h"

namespace gm {

// coef = clamp(max_norm / (sqrt(T) + eps), max = 1), a NaN kept as torch.clamp keeps it: the
// comparison is false for NaN, so the quotient passes through (fmin would return the 1).
// max_norm = +inf: 1 for every finite T.  T = +inf: 0.  T = NaN: NaN.
__host__ __device__ inline float clip_coef(double total_sq, float max_norm, float eps) {
    const double c = (double)max_norm / (sqrt(total_sq) + (double)eps);
    return (float)(c > 1.0 ? 1.0 : c);
}

// A step is non-finite if and only if its total is (inf or NaN; false for both in the comparison)
__host__ __device__ inline bool clip_nonfinite(double total_sq) { return !(fabs(total_sq) <= 1.7976931348623157e308); }

// One pass's finalize, in two parts around the gate's rule and the rate's hand-over
// (k_group_finalize).  One thread, plain stores.
// First: total, coefficient and the skip decision.  Returns skipped_last (the caller leaves the
// gate's rule out of a skipped step).
__device__ inline int clip_decide(double total_sq, gm_clip_state* st) {
    const int skip = (st->skip_nonfinite != 0 && clip_nonfinite(total_sq)) ? 1 : 0;
    st->total_sq = total_sq;
    st->coef = clip_coef(total_sq, st->max_norm, st->eps);
    st->skipped_last = skip;
    return skip;
}

// Last: the counters of the pass just decided - every pass, the skipped ones, and those that ran
// with coef < 1
__device__ inline void clip_count(gm_clip_state* st) {
    st->steps += 1;
    if (st->skipped_last) st->skipped += 1;
    else if (st->coef < 1.f) st->clipped += 1;
}

}  // namespace gm
