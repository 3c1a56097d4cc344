// Per-branch weight/gradient norms (+ fused SGD) for the conditional-learning-
// speed gate: one multi-tensor pass over all parameters and gradients.
//
// Reference: Bias_Mitigation_Strong.compute_BDR (src/callbacks.py:199-233) runs
// `(p**2).sum().item()` and `(g**2).sum().item()` for each of the 142 parameter
// tensors (284 host syncs per step) and then torch.optim.SGD updates them
// (train.py:48-51).  Here: ONE streaming pass.  The virtual concatenation of all
// tensors is cut into fixed chunks; each workgroup streams its chunk with 16-byte
// loads, accumulates per-thread fp32 partials per tensor segment, folds them into
// fp64 per-group sums, and writes one fp64 row per workgroup; a second 1-block
// pass adds the rows in fixed order.  HBM bytes/step: 8*N (read p, g) without the
// update, 12*N with it (read p, g; write p), 20*N with a momentum buffer (gm_group_sumsq_sgdm:
// + read and write b).  Deterministic.
//
// One of each: the update rule (sgd_update<upd>), the streaming loops and sums
// (stream_segment<upd>), the chunk body per group-count form (chunk_sums, chunk_sums_runs) and
// the host launch path (group_sumsq).  The update form - none, sgd, decay, mom, nest - is a template
// parameter all the way down; the __global__ kernels and the entry points are wrappers that
// choose it.  The device-rate wrappers (k_group_sumsq_dlr, gm_group_sumsq_lr) read
// the learning rate from a gm_lr_state in device memory instead of an argument, and their
// finalize advances its schedule (lr_rule.h): one captured step for every rate.  The parameter-group
// wrappers (k_group_sumsq_pg, gm_group_sumsq_pg) also read each tensor's rate scale and weight decay
// from a small device table, per segment.
//
// The clipped forms (gm_group_sumsq_clip: torch's clip_grad_norm_ and the non-finite step skip, decided
// on the device) need every gradient summed before any element is updated, so they split the pass
// into three ordinary launches in stream (graph) order - nothing spins, nothing shares a launch:
//   1. k_group_sumsq_tot[_runs]: the sums without an update (stream_segment<none, pass::sums>), with
//      the total T = sum g'^2 over every entry as one more column behind the rows;
//   2. k_group_finalize_clip: the group sums, then T -> coef, skipped_last (clip_rule.h), the gate's
//      rule unless skipped, clip->lr = lrs->lr, the schedule's advance;
//   3. k_group_apply[_pg]<upd>: the update alone (stream_segment<upd, pass::apply>) on
//      g'' = (g * gscale) * coef at clip->lr, or nothing at all on skipped_last.
// The same loops, update rule, argument functors and host path as the fused forms.
#include <cmath>

#include "gm_common.h"
#include "clip_rule.h"
#include "gate_rule.h"
#include "lr_rule.h"

namespace gm {

constexpr int kChunk = 16384;     // minimum elements per workgroup
constexpr int kMaxRows = 4096;    // larger totals get longer chunks (fewer rows to finalize)
constexpr int kMaxGroups = 32;  // group_mask bits; 8-group instantiation for <= 4 branches

// Elements per workgroup: 16384, or a multiple of 4096 keeping the grid (= the finalize
// rows) at <= kMaxRows.  C2 (23.8 M elements) stays at 16384; C5 (415 M) gets 102400:
// 4055 rows instead of 25 345, which cost the 1-block finalize 0.71 ms.
__host__ __device__ inline long long chunk_elems(long long total) {
    const long long per = (total + kMaxRows - 1) / kMaxRows;
    const long long c = (per + 4095) / 4096 * 4096;
    return c > kChunk ? c : kChunk;
}

__device__ __forceinline__ int find_tensor(const gm_tensor* t, int nt, long long e) {
    int lo = 0, hi = nt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t[mid].offset <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- the update: torch.optim.SGD(lr, momentum, weight_decay), dampening 0, no Nesterov term ----
// Per element, with g' = gscale*g and each line one fma:
//   d = wd*w + g';  b' = mu*b + d;  w' = w - lr*b'
// A zero-initialised buffer gives torch's first step (b' = d) exactly, so there is no step
// counter.  The form is a compile-time choice: decay keeps b' = d in registers (no buffer
// stream), sgd is d = g' as well (w' = w - lr*g'), none writes nothing.  nest is mom with torch's
// Nesterov step: w' = w - lr*(mu*b' + d), one more fma.
enum class upd { none, sgd, decay, mom, nest };

constexpr bool has_buffer(upd u) { return u == upd::mom || u == upd::nest; }

struct sgdm_args {
    float gscale, lr, mu, wd;
};

template <upd U>
__device__ __forceinline__ float sgd_update(float w, float g, float& b, const sgdm_args& h) {
    if (U == upd::sgd) return fmaf(-h.lr, g, w);
    const float d = fmaf(h.wd, w, g);
    b = has_buffer(U) ? fmaf(h.mu, b, d) : d;
    return fmaf(-h.lr, U == upd::nest ? fmaf(h.mu, b, d) : b, w);
}

// Streams elements [tb, te) of one tensor: accumulates w^2 and g'^2 into sw, sg and applies the
// update in place; mb: the tensor's momentum buffer (upd::mom and nest only).  The sums take w before the
// update and g' without the decay term, in one order for every form: they are bit-identical
// between the forms.  16-byte path: p, g (and mb) congruent mod 16, else the scalar loop.  HBM
// bytes per element: 8 (none), 12 (sgd, decay), 20 (mom, nest: + read and write mb).
// An entry without a gradient is summed for w^2 only and not written (torch: grad is None).  The
// sgd form tests for it inline; decay and mom hand it to the sums-only form up front, and so know
// the gradient present below at compile time (inline it costs upd::mom 5 VGPRs and a wave per
// SIMD).  mom also hands over a gradient without a buffer (the caller's error): nothing of it is
// dereferenced or updated.
// The clipped update (gm_group_sumsq_clip) splits the pass in two, the same loops both times:
//   pass::sums  (upd::none) - the sums alone; mb is not read, but where the update form will
//               stream it, it decides the 16-byte path as it does there, so the sums keep the
//               fused pass's order bit for bit;
//   pass::apply - the update alone with g'' = g' * coef (a second multiplication, not a folded
//               scale); the sums are dead code, and an entry the fused pass would only sum is left.
enum class pass { fused, sums, apply };

template <upd U, pass P = pass::fused>
__device__ __forceinline__ void stream_segment(const gm_tensor& T, float* __restrict__ mb, long long tb,
                                               long long te, const sgdm_args& h, float& sw, float& sg,
                                               float coef = 1.f) {
    constexpr bool MOM = has_buffer(U), EARLY = U == upd::decay || MOM;
    if (P == pass::apply && (T.grad == nullptr || (MOM && mb == nullptr))) return;
    if (EARLY && (T.grad == nullptr || (MOM && mb == nullptr))) {
        stream_segment<upd::none>(T, nullptr, tb, te, h, sw, sg);
        return;
    }
    float* __restrict__ p = T.param;
    const float* __restrict__ gr = T.grad;
    const bool hg = EARLY || gr != nullptr;
    const bool bskew = MOM || (P == pass::sums && hg && mb != nullptr);
    const uintptr_t skew = (hg ? (uintptr_t)(p + tb) ^ (uintptr_t)(gr + tb) : (uintptr_t)0) |
                           (bskew ? (uintptr_t)(p + tb) ^ (uintptr_t)(mb + tb) : (uintptr_t)0);
    // scalar head up to 16-byte alignment of p (and g, mb)
    long long head = tb;
    if ((skew & 15) == 0) {
        while (head < te && ((uintptr_t)(p + head) & 15)) ++head;
    } else {
        head = te;
    }
    auto one = [&](long long i) {
        const float w = p[i];
        float g = hg ? gr[i] * h.gscale : 0.f;
        sw = fmaf(w, w, sw);
        sg = fmaf(g, g, sg);
        if (P == pass::apply) g *= coef;
        if (U != upd::none && hg) {
            float b = MOM ? mb[i] : 0.f;
            p[i] = sgd_update<U>(w, g, b, h);
            if (MOM) mb[i] = b;
        }
    };
    float4* pv = (float4*)(p + head);
    const float4* gv = (const float4*)(hg ? gr + head : nullptr);
    float4* bv = (float4*)(MOM ? mb + head : nullptr);
    auto sumw4 = [&](const float4 w) {
        sw = fmaf(w.x, w.x, sw); sw = fmaf(w.y, w.y, sw);
        sw = fmaf(w.z, w.z, sw); sw = fmaf(w.w, w.w, sw);
    };
    auto grad4 = [&](long long i, const float4 w, float4 g, float4 b) {
        g.x *= h.gscale; g.y *= h.gscale; g.z *= h.gscale; g.w *= h.gscale;
        sg = fmaf(g.x, g.x, sg); sg = fmaf(g.y, g.y, sg);
        sg = fmaf(g.z, g.z, sg); sg = fmaf(g.w, g.w, sg);
        if (P == pass::apply) { g.x *= coef; g.y *= coef; g.z *= coef; g.w *= coef; }
        if (U != upd::none)
            pv[i] = make_float4(sgd_update<U>(w.x, g.x, b.x, h), sgd_update<U>(w.y, g.y, b.y, h),
                                sgd_update<U>(w.z, g.z, b.z, h), sgd_update<U>(w.w, g.w, b.w, h));
        if (MOM) bv[i] = b;
    };
    for (long long i = tb + threadIdx.x; i < head; i += 256) one(i);
    const long long nv = (te - head) >> 2;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    long long i0 = threadIdx.x;
    if (hg) {
        // 4 independent 16-B loads of each stream in flight per thread
        for (; i0 + 3 * 256 < nv; i0 += 4 * 256) {
            float4 w[4], g[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                w[u] = pv[i0 + u * 256];
                g[u] = gv[i0 + u * 256];
                b[u] = MOM ? bv[i0 + u * 256] : zero4;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                sumw4(w[u]);
                grad4(i0 + u * 256, w[u], g[u], b[u]);
            }
        }
    }
    for (long long i = i0; i < nv; i += 256) {
        const float4 w = pv[i];
        sumw4(w);
        if (hg) grad4(i, w, gv[i], MOM ? bv[i] : zero4);
    }
    for (long long i = head + nv * 4 + threadIdx.x; i < te; i += 256) one(i);
}

// The hyper-parameters of a tensor segment, as the chunk bodies below ask for them (hs(T)): one
// sgdm_args for the whole pass, or per parameter group.  A segment is uniform across the workgroup,
// so either way they sit in scalar registers.
struct uniform_args {
    sgdm_args h;
    __device__ __forceinline__ const sgdm_args& operator()(const gm_tensor&) const { return h; }
};

// gm_group_sumsq_pg: rate scale and weight decay from the tensor's entry of the device group table
// (index clamped to the table); the group's rate is the fp64 product rounded once
struct pgroup_args {
    float gscale, lr, mu;
    const gm_sgd_pgroup* __restrict__ pg;
    unsigned last;  // npgroups - 1
    __device__ __forceinline__ sgdm_args operator()(const gm_tensor& T) const {
        const gm_sgd_pgroup e = pg[min(T.pgroup, last)];
        // (the fp64 product is vector arithmetic; readfirstlane puts the uniform result back into a
        // scalar register - left in a VGPR it costs upd::mom 6 VGPRs and its fourth wave per SIMD)
        const float lr_g = (float)((double)lr * (double)e.lr_scale);
        return {gscale, __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, lr_g))), mu,
                e.weight_decay};
    }
};

// One workgroup's chunk, <= 8 groups: per-thread fp64 sums per group, folded over the waves in
// fixed order into one row.  mom: the tensors' buffers (upd::mom and nest only)
// TOT (gm_group_sumsq_clip's sums launch, pass::sums): the chunk's g'^2 over every segment whatever
// its mask, as one more fp64 sum folded the same way, written behind the row block:
// rows[gridDim.x * 2 * ngroups + blockIdx.x].  The rows themselves are the same either way.
template <upd U, int MG, class H, bool TOT = false>
__device__ __forceinline__ void chunk_sums(const gm_tensor* __restrict__ tab, float* const* __restrict__ mom,
                                           int nt, long long total, int ngroups, const H& hs,
                                           long long chunk, double* __restrict__ rows) {
    constexpr pass P = TOT ? pass::sums : pass::fused;
    __shared__ double sred[4][2 * MG + (TOT ? 1 : 0)];
    const long long e0 = (long long)blockIdx.x * chunk;
    const long long e1 = min(total, e0 + chunk);
    double gw[MG], gg[MG], tg = 0.0;
#pragma unroll
    for (int g = 0; g < MG; ++g) { gw[g] = 0.0; gg[g] = 0.0; }
    int ti = find_tensor(tab, nt, e0);
    long long e = e0;
    while (e < e1) {
        const gm_tensor T = tab[ti];
        const long long tb = e - T.offset;                       // first local element
        const long long te = min(T.n, e1 - T.offset);            // end (exclusive)
        float sw = 0.f, sg = 0.f;
        stream_segment<U, P>(T, (has_buffer(U) || (TOT && mom)) ? mom[ti] : nullptr, tb, te, hs(T), sw, sg);
        const unsigned m = T.group_mask;
#pragma unroll
        for (int g = 0; g < MG; ++g)
            if (g < ngroups && ((m >> g) & 1u)) { gw[g] += (double)sw; gg[g] += (double)sg; }
        if (TOT) tg += (double)sg;
        e = T.offset + te;
        ++ti;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < MG; ++g) {
        if (g >= ngroups) break;
        const double w = wave_sum_d(gw[g]);
        const double s = wave_sum_d(gg[g]);
        if (lane == 0) { sred[wave][2 * g] = w; sred[wave][2 * g + 1] = s; }
    }
    if (TOT) {
        const double s = wave_sum_d(tg);
        if (lane == 0) sred[wave][2 * MG] = s;
    }
    __syncthreads();
    if (threadIdx.x < 2 * ngroups) {
        const int j = threadIdx.x;
        rows[(size_t)blockIdx.x * 2 * ngroups + j] = ((sred[0][j] + sred[1][j]) + sred[2][j]) + sred[3][j];
    }
    if (TOT && threadIdx.x == 64) {
        const int j = 2 * MG;
        rows[(size_t)gridDim.x * 2 * ngroups + blockIdx.x] = ((sred[0][j] + sred[1][j]) + sred[2][j]) + sred[3][j];
    }
}

// Many-group form (N-branch gates, up to 32 groups).  The per-thread fp64 arrays of the
// form above cost 128 VGPRs at 32 groups (2.6 TB/s on C5).  Segments are uniform across
// the workgroup, so here each thread keeps ONE fp64 pair for the current run of tensors
// with the same group mask; when the mask changes (a few times per chunk) the workgroup
// reduces the run in fixed order and thread 0 adds it to the LDS per-group sums.
__device__ __forceinline__ void flush_run(double& aw, double& ag, unsigned mask, int ngroups,
                                          double (*sred)[2], double* acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double w = wave_sum_d(aw), g = wave_sum_d(ag);
    if (lane == 0) { sred[wave][0] = w; sred[wave][1] = g; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tw = ((sred[0][0] + sred[1][0]) + sred[2][0]) + sred[3][0];
        const double tg = ((sred[0][1] + sred[1][1]) + sred[2][1]) + sred[3][1];
        for (int k = 0; k < ngroups; ++k)
            if ((mask >> k) & 1u) { acc[2 * k] += tw; acc[2 * k + 1] += tg; }
    }
    __syncthreads();
    aw = 0.0;
    ag = 0.0;
}

// TOT: as in chunk_sums - one more per-thread fp64 sum over the whole chunk, folded at the end
template <upd U, class H, bool TOT = false>
__device__ __forceinline__ void chunk_sums_runs(const gm_tensor* __restrict__ tab, float* const* __restrict__ mom,
                                                int nt, long long total, int ngroups, const H& hs,
                                                long long chunk, double* __restrict__ rows) {
    constexpr pass P = TOT ? pass::sums : pass::fused;
    __shared__ double sred[4][2];
    __shared__ double acc[2 * kMaxGroups];
    if (threadIdx.x < 2 * kMaxGroups) acc[threadIdx.x] = 0.0;
    const long long e0 = (long long)blockIdx.x * chunk;
    const long long e1 = min(total, e0 + chunk);
    int ti = find_tensor(tab, nt, e0);
    unsigned cur = tab[ti].group_mask;
    double aw = 0.0, ag = 0.0, tg = 0.0;
    long long e = e0;
    while (e < e1) {
        const gm_tensor T = tab[ti];
        if (T.group_mask != cur) {
            flush_run(aw, ag, cur, ngroups, sred, acc);
            cur = T.group_mask;
        }
        const long long tb = e - T.offset;
        const long long te = min(T.n, e1 - T.offset);
        float sw = 0.f, sg = 0.f;
        stream_segment<U, P>(T, (has_buffer(U) || (TOT && mom)) ? mom[ti] : nullptr, tb, te, hs(T), sw, sg);
        aw += (double)sw;
        ag += (double)sg;
        if (TOT) tg += (double)sg;
        e = T.offset + te;
        ++ti;
    }
    flush_run(aw, ag, cur, ngroups, sred, acc);
    if (threadIdx.x < 2 * ngroups) rows[(size_t)blockIdx.x * 2 * ngroups + threadIdx.x] = acc[threadIdx.x];
    if (TOT) {  // (flush_run ended on a barrier: sred is free)
        const double s = wave_sum_d(tg);
        if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6][0] = s;
        __syncthreads();
        if (threadIdx.x == 0)
            rows[(size_t)gridDim.x * 2 * ngroups + blockIdx.x] = ((sred[0][0] + sred[1][0]) + sred[2][0]) + sred[3][0];
    }
}

// The apply launch of gm_group_sumsq_clip: the same walk over the chunk's segments with the update
// alone (pass::apply) - no sums, no rows, no finalize.  (Walking the chunks last to first, to start
// with what the sums launch touched last, was measured and did not win: DESIGN §4.)
template <upd U, class H>
__device__ __forceinline__ void chunk_apply(const gm_tensor* __restrict__ tab, float* const* __restrict__ mom,
                                            int nt, long long total, const H& hs, float coef, long long chunk) {
    const long long e0 = (long long)blockIdx.x * chunk;
    const long long e1 = min(total, e0 + chunk);
    int ti = find_tensor(tab, nt, e0);
    long long e = e0;
    while (e < e1) {
        const gm_tensor T = tab[ti];
        const long long tb = e - T.offset;
        const long long te = min(T.n, e1 - T.offset);
        float sw = 0.f, sg = 0.f;  // (dead: the apply pass returns no sums)
        stream_segment<U, pass::apply>(T, has_buffer(U) ? mom[ti] : nullptr, tb, te, hs(T), sw, sg, coef);
        e = T.offset + te;
        ++ti;
    }
}

// The kernels: the two bodies above per update form.  The plain pair (gm_group_sumsq, _gate) keeps
// its name and argument layout: profiles and tools find the step boundary by `k_group_sumsq<true`.
template <bool SGD, int MG>
__global__ __launch_bounds__(256) void k_group_sumsq(const gm_tensor* __restrict__ tab, int nt,
                                                     long long total, int ngroups, float gscale,
                                                     float lr, long long chunk, double* __restrict__ rows) {
    chunk_sums<SGD ? upd::sgd : upd::none, MG>(tab, nullptr, nt, total, ngroups, uniform_args{{gscale, lr, 0.f, 0.f}},
                                               chunk, rows);
}

template <bool SGD>
__global__ __launch_bounds__(256) void k_group_sumsq_runs(const gm_tensor* __restrict__ tab, int nt,
                                                          long long total, int ngroups, float gscale,
                                                          float lr, long long chunk, double* __restrict__ rows) {
    chunk_sums_runs<SGD ? upd::sgd : upd::none>(tab, nullptr, nt, total, ngroups, uniform_args{{gscale, lr, 0.f, 0.f}},
                                                chunk, rows);
}

template <bool MOM, int MG>
__global__ __launch_bounds__(256) void k_group_sumsq_sgdm(const gm_tensor* __restrict__ tab,
                                                          float* const* __restrict__ mom, int nt, long long total,
                                                          int ngroups, sgdm_args h, long long chunk,
                                                          double* __restrict__ rows) {
    chunk_sums<MOM ? upd::mom : upd::decay, MG>(tab, mom, nt, total, ngroups, uniform_args{h}, chunk, rows);
}

template <bool MOM>
__global__ __launch_bounds__(256) void k_group_sumsq_sgdm_runs(const gm_tensor* __restrict__ tab,
                                                               float* const* __restrict__ mom, int nt,
                                                               long long total, int ngroups, sgdm_args h,
                                                               long long chunk, double* __restrict__ rows) {
    chunk_sums_runs<MOM ? upd::mom : upd::decay>(tab, mom, nt, total, ngroups, uniform_args{h}, chunk, rows);
}

// The device-rate forms: the rate is *lrs, read once per workgroup (a uniform load that ends in a
// scalar register as the argument does); otherwise the kernels above, for every update form.
template <upd U, int MG>
__global__ __launch_bounds__(256) void k_group_sumsq_dlr(const gm_tensor* __restrict__ tab,
                                                         float* const* __restrict__ mom, int nt, long long total,
                                                         int ngroups, float gscale,
                                                         const gm_lr_state* __restrict__ lrs, float mu, float wd,
                                                         long long chunk, double* __restrict__ rows) {
    chunk_sums<U, MG>(tab, mom, nt, total, ngroups, uniform_args{{gscale, lrs->lr, mu, wd}}, chunk, rows);
}

template <upd U>
__global__ __launch_bounds__(256) void k_group_sumsq_dlr_runs(const gm_tensor* __restrict__ tab,
                                                              float* const* __restrict__ mom, int nt,
                                                              long long total, int ngroups, float gscale,
                                                              const gm_lr_state* __restrict__ lrs, float mu,
                                                              float wd, long long chunk,
                                                              double* __restrict__ rows) {
    chunk_sums_runs<U>(tab, mom, nt, total, ngroups, uniform_args{{gscale, lrs->lr, mu, wd}}, chunk, rows);
}

// The parameter-group forms (decay, mom, nest): the device-rate kernels with each segment's rate
// scale and weight decay read from the group table pg[0..npg) by the tensor's index (pgroup_args).
template <upd U, int MG>
__global__ __launch_bounds__(256) void k_group_sumsq_pg(const gm_tensor* __restrict__ tab,
                                                        float* const* __restrict__ mom, int nt, long long total,
                                                        int ngroups, float gscale,
                                                        const gm_lr_state* __restrict__ lrs, float mu,
                                                        const gm_sgd_pgroup* __restrict__ pg, int npg,
                                                        long long chunk, double* __restrict__ rows) {
    chunk_sums<U, MG>(tab, mom, nt, total, ngroups, pgroup_args{gscale, lrs->lr, mu, pg, (unsigned)(npg - 1)}, chunk,
                      rows);
}

template <upd U>
__global__ __launch_bounds__(256) void k_group_sumsq_pg_runs(const gm_tensor* __restrict__ tab,
                                                             float* const* __restrict__ mom, int nt,
                                                             long long total, int ngroups, float gscale,
                                                             const gm_lr_state* __restrict__ lrs, float mu,
                                                             const gm_sgd_pgroup* __restrict__ pg, int npg,
                                                             long long chunk, double* __restrict__ rows) {
    chunk_sums_runs<U>(tab, mom, nt, total, ngroups, pgroup_args{gscale, lrs->lr, mu, pg, (unsigned)(npg - 1)}, chunk,
                       rows);
}

// The clipped forms (gm_group_sumsq_clip).  Launch 1, the sums with the total behind the rows
// (mom: null, or the buffers the apply launch will stream - for the 16-byte path only):
template <int MG>
__global__ __launch_bounds__(256) void k_group_sumsq_tot(const gm_tensor* __restrict__ tab,
                                                         float* const* __restrict__ mom, int nt, long long total,
                                                         int ngroups, float gscale, long long chunk,
                                                         double* __restrict__ rows) {
    chunk_sums<upd::none, MG, uniform_args, true>(tab, mom, nt, total, ngroups, uniform_args{{gscale, 0.f, 0.f, 0.f}},
                                                  chunk, rows);
}

__global__ __launch_bounds__(256) void k_group_sumsq_tot_runs(const gm_tensor* __restrict__ tab,
                                                              float* const* __restrict__ mom, int nt,
                                                              long long total, int ngroups, float gscale,
                                                              long long chunk, double* __restrict__ rows) {
    chunk_sums_runs<upd::none, uniform_args, true>(tab, mom, nt, total, ngroups, uniform_args{{gscale, 0.f, 0.f, 0.f}},
                                                   chunk, rows);
}

// Launch 3, the apply: coefficient, rate and the skip decision are what the finalize launch left in
// *clip, read once per workgroup (uniform loads that end in scalar registers, as lrs->lr does in the
// device-rate forms).  A skipped step returns before it touches anything.
template <upd U>
__global__ __launch_bounds__(256) void k_group_apply(const gm_tensor* __restrict__ tab,
                                                     float* const* __restrict__ mom, int nt, long long total,
                                                     float gscale, const gm_clip_state* __restrict__ clip, float mu,
                                                     float wd, long long chunk) {
    if (clip->skipped_last) return;  // (uniform)
    chunk_apply<U>(tab, mom, nt, total, uniform_args{{gscale, clip->lr, mu, wd}}, clip->coef, chunk);
}

template <upd U>
__global__ __launch_bounds__(256) void k_group_apply_pg(const gm_tensor* __restrict__ tab,
                                                        float* const* __restrict__ mom, int nt, long long total,
                                                        float gscale, const gm_clip_state* __restrict__ clip,
                                                        float mu, const gm_sgd_pgroup* __restrict__ pg, int npg,
                                                        long long chunk) {
    if (clip->skipped_last) return;  // (uniform)
    chunk_apply<U>(tab, mom, nt, total, pgroup_args{gscale, clip->lr, mu, pg, (unsigned)(npg - 1)}, clip->coef, chunk);
}

// 1024 threads stream the [nrows][w] row block as one flat array with fully coalesced
// 8-byte loads: thread t < S (S = the largest multiple of w <= 1024) owns column t % w and
// reads elements t, t + S, ... (8 in flight).  The former form gave each thread whole
// 128-B rows (every load instruction touched 64 cache lines; 13 us on the serial end of
// the C2 step for 1451 rows).  Then per column 32 fixed partial sums of its slots and
// their fixed-order total => deterministic.  (Threads t >= S hold 0 and take no part.)
constexpr int kFinT = 1024;
// The column totals of a [nrows][w] block (w <= 2 kMaxGroups): to tot_s (shared, valid behind the
// caller's next barrier) and, where given, to out.
__device__ __forceinline__ void column_totals(const double* __restrict__ rows, int nrows, int w,
                                              double* __restrict__ out, double* tot_s) {
    __shared__ double s[kFinT];
    __shared__ double part[32 * 2 * kMaxGroups];
    const int S = (kFinT / w) * w, R = S / w;  // R row slots per column
    const int t = threadIdx.x;
    const long long n = (long long)nrows * w;
    double acc = 0.0;
    if (t < S) {
        long long e = t;
        for (; e + 7ll * S < n; e += 8ll * S) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = rows[e + u * (long long)S];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; e < n; e += S) acc += rows[e];
    }
    s[t] = acc;
    __syncthreads();
    const int P = min(32, R);  // partial sums per column (R = kFinT / w >= 16)
    if (t < P * w) {  // column c = t % w, partial q = t / w over slots q, q + P, ...
        const int c = t % w, q = t / w;
        double p = 0.0;
        for (int j = q; j < R; j += P) p += s[j * w + c];
        part[q * w + c] = p;
    }
    __syncthreads();
    if (t < w) {
        double tot = 0.0;
        for (int q = 0; q < P; ++q) tot += part[q * w + t];
        if (out) out[t] = tot;
        tot_s[t] = tot;
    }
}

// gate (optional): the on-device gate's state - gm_gate_state (gate_n 0) or gm_gate_state_n (1) -
// whose step rule thread 0 applies to the finished sums (gm_group_sumsq_gate: no gate launch)
__device__ __forceinline__ void gate_rule(const double* tot_s, void* gate, int gate_n) {
    if (gate_n) gate_strong_rule_n(tot_s, static_cast<gm_gate_state_n*>(gate));
    else gate_strong_rule(tot_s, static_cast<gm_gate_state*>(gate));
}

__device__ __forceinline__ void finalize_sums(const double* __restrict__ rows, int nrows, int ngroups,
                                              double* __restrict__ out, void* gate, int gate_n) {
    __shared__ double tot_s[2 * kMaxGroups];
    column_totals(rows, nrows, 2 * ngroups, out, tot_s);
    if (gate == nullptr) return;  // (uniform)
    __syncthreads();
    if (threadIdx.x == 0) gate_rule(tot_s, gate, gate_n);
}

__global__ __launch_bounds__(kFinT) void k_group_finalize(const double* __restrict__ rows, int nrows,
                                                          int ngroups, double* __restrict__ out,
                                                          void* gate = nullptr, int gate_n = 0) {
    finalize_sums(rows, nrows, ngroups, out, gate, gate_n);
}

// The finalize of the device-rate forms: thread 0 also advances the rate's schedule, after the
// sums and the gate's rule (the pass that read the old rate ended before this launch began)
__global__ __launch_bounds__(kFinT) void k_group_finalize_lr(const double* __restrict__ rows, int nrows,
                                                             int ngroups, double* __restrict__ out, void* gate,
                                                             int gate_n, gm_lr_state* lrs) {
    finalize_sums(rows, nrows, ngroups, out, gate, gate_n);
    if (threadIdx.x == 0) lr_advance(lrs);
}

// The finalize of the clipped forms, between the sums launch and the apply launch: the group sums
// as above (the same block, the same order), then the total from the column behind the rows, and
// thread 0 runs the clip's rule, the gate's rule unless the step is skipped, hands the apply launch
// its rate and advances the schedule - on a skipped step too (greedymml.h)
__global__ __launch_bounds__(kFinT) void k_group_finalize_clip(const double* __restrict__ rows, int nrows,
                                                               int ngroups, double* __restrict__ out, void* gate,
                                                               int gate_n, gm_lr_state* lrs, gm_clip_state* clip) {
    __shared__ double tot_s[2 * kMaxGroups];
    __shared__ double tot_t[1];
    column_totals(rows, nrows, 2 * ngroups, out, tot_s);
    __syncthreads();  // (column_totals' LDS is read no more)
    column_totals(rows + (size_t)nrows * 2 * ngroups, nrows, 1, nullptr, tot_t);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int skipped = clip_decide(tot_t[0], clip);
        if (gate != nullptr && !skipped) gate_rule(tot_s, gate, gate_n);
        clip->lr = lrs->lr;
        lr_advance(lrs);
        clip_count(clip);
    }
}

}  // namespace gm

using namespace gm;

extern "C" size_t gm_group_sumsq_scratch(long long total) {
    if (total <= 0) return 0;
    const long long nb = (total + chunk_elems(total) - 1) / chunk_elems(total);
    return (size_t)nb * 2 * kMaxGroups * sizeof(double);
}

// The launch path of every entry point: shared checks, chunking, the kernel of (form, group
// count), finalize.  mom: the buffers of upd::mom; gate: optional (null: sums only); lrs: the
// device rate of the device-rate forms (null: h.lr, the argument).
template <upd U>
static auto dlr_kernel(bool few) {
    return few ? k_group_sumsq_dlr<U, 8> : k_group_sumsq_dlr_runs<U>;
}

template <upd U>
static auto pg_kernel(bool few) {
    return few ? k_group_sumsq_pg<U, 8> : k_group_sumsq_pg_runs<U>;
}

template <upd U>
static void launch_apply(int nb, hipStream_t st, const gm_tensor* table, float* const* mom, int nt, long long total,
                         const sgdm_args& h, const gm_clip_state* clip, const gm_sgd_pgroup* pg, int npg,
                         long long chunk) {
    if (pg) k_group_apply_pg<U><<<nb, 256, 0, st>>>(table, mom, nt, total, h.gscale, clip, h.mu, pg, npg, chunk);
    else k_group_apply<U><<<nb, 256, 0, st>>>(table, mom, nt, total, h.gscale, clip, h.mu, h.wd, chunk);
}

// pg (with lrs): the device group table of gm_group_sumsq_pg (null: h.wd for every tensor)
// clip (with lrs): gm_group_sumsq_clip - the sums launch, the clip's finalize, the apply launch
static int group_sumsq(const gm_tensor* table, float* const* mom, int nt, long long total, int ngroups,
                       const sgdm_args& h, upd form, double* out, void* scratch, size_t scratch_bytes, void* gate,
                       int gate_n, void* stream, gm_lr_state* lrs = nullptr, const gm_sgd_pgroup* pg = nullptr,
                       int npg = 0, gm_clip_state* clip = nullptr) {
    // (main, bypass) groups per branch: 4 for the two-branch gate, 2 nb for the N-branch one (nb in
    // the state: the rule reads 4 nb sums)
    GM_REQUIRE(!gate || (gate_n ? (ngroups >= 4 && ngroups % 2 == 0) : ngroups == 4),
               "group_sumsq_gate: %d groups do not match the %s gate", ngroups, gate_n ? "N-branch" : "two-branch");
    GM_REQUIRE(table && nt >= 1 && total >= 1, "group_sumsq: empty tensor table");
    GM_REQUIRE(ngroups >= 1 && ngroups <= kMaxGroups, "group_sumsq: ngroups must be 1..%d", kMaxGroups);
    // (the total's column lies behind the rows in the scratch, which is sized for kMaxGroups)
    GM_REQUIRE(!clip || ngroups < kMaxGroups, "group_sumsq_clip: ngroups must be 1..%d", kMaxGroups - 1);
    GM_REQUIRE(out, "group_sumsq: null output");
    const long long chunk = chunk_elems(total);
    GM_REQUIRE((total + chunk - 1) / chunk < (1ll << 31), "group_sumsq: too many elements");
    GM_REQUIRE(scratch && scratch_bytes >= gm_group_sumsq_scratch(total),
               "group_sumsq: scratch %zu < %zu bytes", scratch_bytes, gm_group_sumsq_scratch(total));
    const int nb = (int)((total + chunk - 1) / chunk);
    hipStream_t st = as_stream(stream);
    double* rows = (double*)scratch;
    const bool few = ngroups <= 8;  // else the N-branch gates (C5: 12 branches -> 24 groups)
    const bool plain = form == upd::none || form == upd::sgd;
    if (clip) {
        const auto k = few ? k_group_sumsq_tot<8> : k_group_sumsq_tot_runs;
        k<<<nb, 256, 0, st>>>(table, has_buffer(form) ? mom : nullptr, nt, total, ngroups, h.gscale, chunk, rows);
        int rc = check_launch("k_group_sumsq_tot");
        if (rc) return rc;
        k_group_finalize_clip<<<1, kFinT, 0, st>>>(rows, nb, ngroups, out, gate, gate && gate_n ? 1 : 0, lrs, clip);
        rc = check_launch("k_group_finalize_clip");
        if (rc) return rc;
        switch (form) {
            case upd::nest: launch_apply<upd::nest>(nb, st, table, mom, nt, total, h, clip, pg, npg, chunk); break;
            case upd::mom: launch_apply<upd::mom>(nb, st, table, mom, nt, total, h, clip, pg, npg, chunk); break;
            case upd::decay: launch_apply<upd::decay>(nb, st, table, mom, nt, total, h, clip, pg, npg, chunk); break;
            default: launch_apply<upd::sgd>(nb, st, table, mom, nt, total, h, clip, pg, npg, chunk); break;
        }
        return check_launch("k_group_apply");
    }
    if (pg) {
        const auto k = form == upd::nest ? pg_kernel<upd::nest>(few)
                                         : (form == upd::mom ? pg_kernel<upd::mom>(few) : pg_kernel<upd::decay>(few));
        k<<<nb, 256, 0, st>>>(table, mom, nt, total, ngroups, h.gscale, lrs, h.mu, pg, npg, chunk, rows);
    } else if (lrs) {
        const auto k = form == upd::sgd ? dlr_kernel<upd::sgd>(few)
                                        : (form == upd::mom ? dlr_kernel<upd::mom>(few) : dlr_kernel<upd::decay>(few));
        k<<<nb, 256, 0, st>>>(table, mom, nt, total, ngroups, h.gscale, lrs, h.mu, h.wd, chunk, rows);
    } else if (plain) {
        const bool sgd = form == upd::sgd;
        const auto k = few ? (sgd ? k_group_sumsq<true, 8> : k_group_sumsq<false, 8>)
                           : (sgd ? k_group_sumsq_runs<true> : k_group_sumsq_runs<false>);
        k<<<nb, 256, 0, st>>>(table, nt, total, ngroups, h.gscale, h.lr, chunk, rows);
    } else {
        const bool mo = form == upd::mom;
        const auto k = few ? (mo ? k_group_sumsq_sgdm<true, 8> : k_group_sumsq_sgdm<false, 8>)
                           : (mo ? k_group_sumsq_sgdm_runs<true> : k_group_sumsq_sgdm_runs<false>);
        k<<<nb, 256, 0, st>>>(table, mom, nt, total, ngroups, h, chunk, rows);
    }
    int rc = check_launch(pg ? "k_group_sumsq_pg"
                             : (lrs ? "k_group_sumsq_dlr" : (plain ? "k_group_sumsq" : "k_group_sumsq_sgdm")));
    if (rc) return rc;
    if (lrs) k_group_finalize_lr<<<1, kFinT, 0, st>>>(rows, nb, ngroups, out, gate, gate && gate_n ? 1 : 0, lrs);
    else k_group_finalize<<<1, kFinT, 0, st>>>(rows, nb, ngroups, out, gate, gate && gate_n ? 1 : 0);
    return check_launch("k_group_finalize");
}

extern "C" int gm_group_sumsq(const gm_tensor* table, int nt, long long total, int ngroups, float gscale,
                              float lr, double* out, void* scratch, size_t scratch_bytes, void* stream) {
    return group_sumsq(table, nullptr, nt, total, ngroups, {gscale, lr, 0.f, 0.f}, lr != 0.f ? upd::sgd : upd::none,
                       out, scratch, scratch_bytes, nullptr, 0, stream);
}

extern "C" int gm_group_sumsq_gate(const gm_tensor* table, int nt, long long total, int ngroups, float gscale,
                                   float lr, double* out, void* scratch, size_t scratch_bytes, void* gate,
                                   int gate_n, void* stream) {
    GM_REQUIRE(gate, "group_sumsq_gate: null gate state");
    return group_sumsq(table, nullptr, nt, total, ngroups, {gscale, lr, 0.f, 0.f}, lr != 0.f ? upd::sgd : upd::none,
                       out, scratch, scratch_bytes, gate, gate_n, stream);
}

extern "C" int gm_group_sumsq_sgdm(const gm_tensor* table, float* const* mom, int nt, long long total,
                                   int ngroups, float gscale, float lr, float momentum, float weight_decay,
                                   double* out, void* scratch, size_t scratch_bytes, void* gate, int gate_n,
                                   void* stream) {
    GM_REQUIRE(std::isfinite(momentum) && momentum >= 0.f, "group_sumsq_sgdm: momentum must be finite and >= 0");
    GM_REQUIRE(std::isfinite(weight_decay) && weight_decay >= 0.f,
               "group_sumsq_sgdm: weight_decay must be finite and >= 0");
    GM_REQUIRE((mom != nullptr) == (momentum != 0.f),
               "group_sumsq_sgdm: momentum buffers must be given if and only if momentum != 0");
    return group_sumsq(table, mom, nt, total, ngroups, {gscale, lr, momentum, weight_decay},
                       mom ? upd::mom : upd::decay, out, scratch, scratch_bytes, gate, gate_n, stream);
}

extern "C" int gm_group_sumsq_lr(const gm_tensor* table, float* const* mom, int nt, long long total, int ngroups,
                                 float gscale, gm_lr_state* lr, float momentum, float weight_decay, double* out,
                                 void* scratch, size_t scratch_bytes, void* gate, int gate_n, void* stream) {
    GM_REQUIRE(lr, "group_sumsq_lr: null lr state");
    GM_REQUIRE(std::isfinite(momentum) && momentum >= 0.f, "group_sumsq_lr: momentum must be finite and >= 0");
    GM_REQUIRE(std::isfinite(weight_decay) && weight_decay >= 0.f,
               "group_sumsq_lr: weight_decay must be finite and >= 0");
    GM_REQUIRE((mom != nullptr) == (momentum != 0.f),
               "group_sumsq_lr: momentum buffers must be given if and only if momentum != 0");
    const upd form = mom ? upd::mom : (weight_decay != 0.f ? upd::decay : upd::sgd);
    return group_sumsq(table, mom, nt, total, ngroups, {gscale, 0.f, momentum, weight_decay}, form, out, scratch,
                       scratch_bytes, gate, gate_n, stream, lr);
}

extern "C" int gm_group_sumsq_pg(const gm_tensor* table, float* const* mom, int nt, long long total, int ngroups,
                                 float gscale, gm_lr_state* lr, const gm_sgd_pgroup* pgroups, int npgroups,
                                 float momentum, int nesterov, double* out, void* scratch, size_t scratch_bytes,
                                 void* gate, int gate_n, void* stream) {
    GM_REQUIRE(lr, "group_sumsq_pg: null lr state");
    GM_REQUIRE(pgroups, "group_sumsq_pg: null parameter-group table");
    GM_REQUIRE(npgroups >= 1 && npgroups <= GM_SGD_MAX_PGROUPS, "group_sumsq_pg: npgroups must be 1..%d",
               GM_SGD_MAX_PGROUPS);
    GM_REQUIRE(std::isfinite(momentum) && momentum >= 0.f, "group_sumsq_pg: momentum must be finite and >= 0");
    GM_REQUIRE(!nesterov || momentum > 0.f, "group_sumsq_pg: nesterov requires a momentum > 0");
    GM_REQUIRE((mom != nullptr) == (momentum != 0.f),
               "group_sumsq_pg: momentum buffers must be given if and only if momentum != 0");
    const upd form = mom ? (nesterov ? upd::nest : upd::mom) : upd::decay;
    return group_sumsq(table, mom, nt, total, ngroups, {gscale, 0.f, momentum, 0.f}, form, out, scratch,
                       scratch_bytes, gate, gate_n, stream, lr, pgroups, npgroups);
}

extern "C" int gm_group_sumsq_clip(const gm_tensor* table, float* const* mom, int nt, long long total, int ngroups,
                                   float gscale, gm_lr_state* lr, const gm_sgd_pgroup* pgroups, int npgroups,
                                   float momentum, float weight_decay, int nesterov, gm_clip_state* clip,
                                   double* out, void* scratch, size_t scratch_bytes, void* gate, int gate_n,
                                   void* stream) {
    GM_REQUIRE(clip, "group_sumsq_clip: null clip state");
    GM_REQUIRE(lr, "group_sumsq_clip: null lr state");
    GM_REQUIRE(!pgroups || (npgroups >= 1 && npgroups <= GM_SGD_MAX_PGROUPS),
               "group_sumsq_clip: npgroups must be 1..%d", GM_SGD_MAX_PGROUPS);
    GM_REQUIRE(std::isfinite(momentum) && momentum >= 0.f, "group_sumsq_clip: momentum must be finite and >= 0");
    GM_REQUIRE(std::isfinite(weight_decay) && weight_decay >= 0.f,
               "group_sumsq_clip: weight_decay must be finite and >= 0");
    GM_REQUIRE(!pgroups || weight_decay == 0.f,
               "group_sumsq_clip: the parameter-group table owns the weight decay (weight_decay must be 0)");
    GM_REQUIRE(!nesterov || momentum > 0.f, "group_sumsq_clip: nesterov requires a momentum > 0");
    GM_REQUIRE((mom != nullptr) == (momentum != 0.f),
               "group_sumsq_clip: momentum buffers must be given if and only if momentum != 0");
    const upd form = mom ? (nesterov ? upd::nest : upd::mom)
                         : ((pgroups || weight_decay != 0.f) ? upd::decay : upd::sgd);
    return group_sumsq(table, mom, nt, total, ngroups, {gscale, 0.f, momentum, weight_decay}, form, out, scratch,
                       scratch_bytes, gate, gate_n, stream, lr, pgroups, pgroups ? npgroups : 0, clip);
}

extern "C" int gm_clip_state_check(const gm_clip_state* host) {
    GM_REQUIRE(host, "clip_state_check: null state");
    GM_REQUIRE(host->max_norm > 0.f, "clip_state_check: max_norm must be > 0 (+inf: never clips)");
    GM_REQUIRE(std::isfinite(host->eps) && host->eps >= 0.f, "clip_state_check: eps must be finite and >= 0");
    GM_REQUIRE(host->skip_nonfinite == 0 || host->skip_nonfinite == 1, "clip_state_check: skip_nonfinite must be 0 or 1");
    return 0;
}

extern "C" int gm_clip_coef(double total_sq, const gm_clip_state* host, float* coef_out) {
    GM_REQUIRE(host && coef_out, "clip_coef: null argument");
    *coef_out = clip_coef(total_sq, host->max_norm, host->eps);
    return 0;
}

extern "C" int gm_sgd_pgroups_check(const gm_sgd_pgroup* host, int npgroups) {
    GM_REQUIRE(host, "sgd_pgroups_check: null table");
    GM_REQUIRE(npgroups >= 1 && npgroups <= GM_SGD_MAX_PGROUPS, "sgd_pgroups_check: npgroups must be 1..%d",
               GM_SGD_MAX_PGROUPS);
    for (int i = 0; i < npgroups; ++i) {
        GM_REQUIRE(std::isfinite(host[i].lr_scale) && host[i].lr_scale >= 0.f,
                   "sgd_pgroups_check: group %d: lr_scale must be finite and >= 0", i);
        GM_REQUIRE(std::isfinite(host[i].weight_decay) && host[i].weight_decay >= 0.f,
                   "sgd_pgroups_check: group %d: weight_decay must be finite and >= 0", i);
    }
    return 0;
}

extern "C" int gm_lr_at(const gm_lr_state* s, long long t, float* lr_out) {
    GM_REQUIRE(s && lr_out, "lr_at: null argument");
    GM_REQUIRE(t >= 0, "lr_at: pass index must be >= 0");
    GM_REQUIRE(s->kind == kLrHeld || s->kind == kLrMultistep || s->kind == kLrCosine, "lr_at: unknown kind %d",
               s->kind);
    const auto rate = [](double v) { return std::isfinite(v) && v >= 0.0; };
    GM_REQUIRE(rate(s->lr) && rate(s->base_lr) && rate(s->min_lr), "lr_at: rates must be finite and >= 0");
    GM_REQUIRE(rate(s->gamma) && rate(s->warmup_start), "lr_at: gamma and warmup_start must be finite and >= 0");
    GM_REQUIRE(s->warmup_steps >= 0, "lr_at: warmup_steps must be >= 0");
    GM_REQUIRE(s->n_milestones >= 0 && s->n_milestones <= GM_LR_MAX_MILESTONES, "lr_at: n_milestones must be 0..%d",
               GM_LR_MAX_MILESTONES);
    GM_REQUIRE(s->kind != kLrCosine || s->total_steps > s->warmup_steps,
               "lr_at: cosine needs total_steps > warmup_steps");
    *lr_out = lr_rule(*s, t);
    return 0;
}
