// Branch-summed cross-entropy of the training step (reference train.py:22-29 blend_loss:
// loss = sum over branches of F.cross_entropy(logits_branch, y), mean over the batch)
// and its gradient, for all branches in one launch each.  Replaces ~20 small
// PyTorch kernels (log_softmax / nll_loss forward and backward per branch, fills,
// the branch sum) at the end of the step.
//
//   gm_xent_fwd: rows r = br*B + b; lse_r = log sum_n exp(x[r,n]) (max-shifted fp32,
//                as log_softmax), loss = sum_br (1/B) sum_b (lse_r - x[r, y_b]); one
//                workgroup, row losses combined in fp64 in a fixed order: deterministic.
//                A label outside [0, N) makes the loss NaN (PyTorch asserts).
//   gm_xent_bwd: dx[r,n] = g * (exp(x[r,n] - lse_r) - [n == y_b]) / B, g = *gout
//                (the loss's incoming gradient, read on the device).
#include "gm_common.h"

namespace gm {
namespace {

constexpr int kXT = 256;

__device__ __forceinline__ float row_lse(const float* x, int N) {
    float m = -INFINITY;
    for (int n = 0; n < N; ++n) m = fmaxf(m, x[n]);
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += expf(x[n] - m);
    return m + logf(s);
}

__global__ __launch_bounds__(kXT) void k_xent_fwd(const float* __restrict__ x, int rows, int B, int N,
                                                  const long long* __restrict__ y, float* __restrict__ lse,
                                                  float* __restrict__ loss) {
    __shared__ double red[kXT];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int r = t; r < rows; r += kXT) {
        const float* xr = x + (size_t)r * N;
        const float l = row_lse(xr, N);
        lse[r] = l;
        const long long lab = y[r % B];
        const float v = (lab >= 0 && lab < N) ? l - xr[lab] : NAN;
        acc += (double)v;
    }
    red[t] = acc;
    __syncthreads();
    for (int s = kXT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) *loss = (float)(red[0] / (double)B);
}

__global__ __launch_bounds__(kXT) void k_xent_bwd(const float* __restrict__ x, const float* __restrict__ lse,
                                                  int rows, int B, int N, const long long* __restrict__ y,
                                                  const float* __restrict__ gout, float* __restrict__ dx) {
    const long long i = (long long)blockIdx.x * kXT + threadIdx.x;
    if (i >= (long long)rows * N) return;
    const int r = (int)(i / N), n = (int)(i - (long long)r * N);
    const float g = *gout / (float)B;
    const float p = expf(x[i] - lse[r]);
    dx[i] = g * (p - (y[r % B] == n ? 1.f : 0.f));
}

// The evaluation pass's metrics behind the heads (gm_eval_metrics): per sample b the branch-summed
// cross-entropy (row_lse in fp32, as k_xent_fwd; summed in fp64), the top-1 of the branch-mean
// logits (losses.acc: the fp32 sum over the branches in order, times 1 / nbranch) and of each
// branch - the first maximal index wins, a NaN counts as maximal (torch.argmax).  One workgroup,
// the threads' partial sums combined by an LDS tree: a fixed order, no atomics; thread 0 adds
// them to the caller's accumulators (launches on one stream follow each other).
constexpr int kMaxBranch = 8;

__device__ __forceinline__ bool arg_gt(float v, float best) { return v > best || (v != v && best == best); }

__global__ __launch_bounds__(kXT) void k_eval_metrics(const float* __restrict__ x, int nbr, int B, int N,
                                                      const long long* __restrict__ y, long long* __restrict__ out) {
    __shared__ double red[kXT];
    __shared__ int redc[kMaxBranch + 1][kXT];
    const int t = threadIdx.x;
    double loss = 0.0;
    int hit[kMaxBranch + 1];  // [0]: the branch mean; [1 + br]: branch br
#pragma unroll
    for (int k = 0; k <= kMaxBranch; ++k) hit[k] = 0;
    const float inv = 1.f / (float)nbr;
    for (int b = t; b < B; b += kXT) {
        const long long lab = y[b];
        const bool lab_ok = lab >= 0 && lab < N;
#pragma unroll
        for (int br = 0; br < kMaxBranch; ++br) {
            if (br >= nbr) break;
            const float* xr = x + ((size_t)br * B + b) * N;
            const float v = lab_ok ? row_lse(xr, N) - xr[lab] : NAN;
            loss += (double)v;
            int am = 0;
            float best = xr[0];
            for (int n = 1; n < N; ++n)
                if (arg_gt(xr[n], best)) { best = xr[n]; am = n; }
            hit[1 + br] += (lab_ok && am == (int)lab) ? 1 : 0;
        }
        int am = 0;
        float best = 0.f;
        for (int n = 0; n < N; ++n) {
            float s = 0.f;
            for (int br = 0; br < nbr; ++br) s += x[((size_t)br * B + b) * N + n];
            s *= inv;
            if (n == 0 || arg_gt(s, best)) { best = s; am = n; }
        }
        hit[0] += (lab_ok && am == (int)lab) ? 1 : 0;
    }
    red[t] = loss;
#pragma unroll
    for (int k = 0; k <= kMaxBranch; ++k) redc[k][t] = hit[k];
    __syncthreads();
    for (int s = kXT / 2; s > 0; s >>= 1) {
        if (t < s) {
            red[t] += red[t + s];
#pragma unroll
            for (int k = 0; k <= kMaxBranch; ++k) redc[k][t] += redc[k][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        double* lsum = reinterpret_cast<double*>(out);
        *lsum += red[0];
        out[1] += B;
        out[2] += redc[0][0];
        for (int br = 0; br < nbr; ++br) out[3 + br] += redc[1 + br][0];
    }
}

}  // namespace
}  // namespace gm

using namespace gm;

extern "C" int gm_eval_metrics(const float* logits, int nbranch, int B, int N, const long long* labels, void* acc,
                               void* stream) {
    const char* fn = "gm_eval_metrics";
    GM_REQUIRE(logits, "%s: null logits", fn);
    GM_REQUIRE(labels, "%s: null labels", fn);
    GM_REQUIRE(acc && (reinterpret_cast<uintptr_t>(acc) & 7) == 0, "%s: acc null or not 8-byte aligned", fn);
    GM_REQUIRE(nbranch >= 1 && nbranch <= kMaxBranch, "%s: nbranch must be 1..%d (got %d)", fn, kMaxBranch, nbranch);
    GM_REQUIRE(B > 0 && N > 0, "%s: need B, N > 0", fn);
    hipLaunchKernelGGL(k_eval_metrics, dim3(1), dim3(kXT), 0, as_stream(stream), logits, nbranch, B, N, labels,
                       static_cast<long long*>(acc));
    return check_launch("k_eval_metrics");
}

extern "C" int gm_xent_fwd(const float* logits, int nbranch, int B, int N, const long long* labels, float* lse,
                           float* loss, void* stream) {
    GM_REQUIRE(logits && labels && lse && loss, "gm_xent_fwd: null argument");
    GM_REQUIRE(nbranch > 0 && B > 0 && N > 0, "gm_xent_fwd: need nbranch, B, N > 0");
    hipLaunchKernelGGL(k_xent_fwd, dim3(1), dim3(kXT), 0, as_stream(stream), logits, nbranch * B, B, N, labels,
                       lse, loss);
    return check_launch("k_xent_fwd");
}

extern "C" int gm_xent_bwd(const float* logits, const float* lse, int nbranch, int B, int N,
                           const long long* labels, const float* gout, float* dlogits, void* stream) {
    GM_REQUIRE(logits && lse && labels && gout && dlogits, "gm_xent_bwd: null argument");
    GM_REQUIRE(nbranch > 0 && B > 0 && N > 0, "gm_xent_bwd: need nbranch, B, N > 0");
    const long long n = (long long)nbranch * B * N;
    hipLaunchKernelGGL(k_xent_bwd, dim3((unsigned)((n + kXT - 1) / kXT)), dim3(kXT), 0, as_stream(stream), logits,
                       lse, nbranch * B, B, N, labels, gout, dlogits);
    return check_launch("k_xent_bwd");
}
