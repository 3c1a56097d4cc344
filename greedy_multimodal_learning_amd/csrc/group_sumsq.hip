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
// (stream_segment<upd>), the chunk body per group-count form (chunk_sums, chunk_sums_runs), the
// argument rules of the entry points (check_update) and the host launch path (group_sumsq).  The
// update form - none, sgd, decay, mom, nest - is a template parameter all the way down.
//
// Three __global__ templates; the two streaming ones take one by-value pass_args and the four
// arrays they stream through:
//   k_group_sumsq<upd, body, H, TOT>  the sums, fused with the update unless upd::none.  body: the
//       <= 8-group form or the run form.  H: where a segment's hyper-parameters come from -
//       uniform_args (one set for the pass) or pgroup_args (gm_group_sumsq_pg: each tensor's rate
//       scale and weight decay from a small device table).  The rate is the argument, or, given a
//       gm_lr_state (gm_group_sumsq_lr, _pg), its lr in device memory: one captured step for every
//       rate.  TOT: the total T = sum g'^2 over every entry as one more column behind the rows.
//   k_group_finalize  one block: the rows' column totals in fixed order, then thread 0 applies what
//       the entry asked for - the clip's rule, the gate's rule, the schedule's advance (lr_rule.h).
//   k_group_apply<upd, H>  the update alone (stream_segment<upd, pass::apply>).
// Every entry but one is k_group_sumsq then k_group_finalize.  The clipped entry
// (gm_group_sumsq_clip: torch's clip_grad_norm_ and the non-finite step skip, decided on the
// device) needs every gradient summed before any element is updated, so it is three ordinary
// launches in stream (graph) order - nothing spins, nothing shares a launch: the sums without an
// update (k_group_sumsq<none, ., uniform_args, TOT>), the finalize, and k_group_apply on
// g'' = (g * gscale) * coef at clip->lr, or nothing at all on skipped_last.
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

// What the two streaming kernels take: one by-value pass_args, and beside it the four arrays the
// loops read and write through - the tensor table, the tensors' momentum buffers (null without),
// the parameter-group table (pgroup_args only) and the workgroups' rows (k_group_sumsq only) - each
// a __restrict__ kernel parameter of its own.  Only there does __restrict__ reach the compiler:
// with the four pointers inside the struct upd::mom takes up to 6 more VGPRs and loses its fourth
// wave per SIMD in three instantiations.  A kernel loads only the fields it reads.
struct pass_args {
    int nt;
    long long total;
    int ngroups;  // k_group_sumsq only
    float gscale, lr, mu, wd;
    const gm_lr_state* lrs;  // k_group_sumsq: non-null: the rate is lrs->lr, not lr
    int npg;                 // pgroup_args only
    const gm_clip_state* clip;  // k_group_apply only
    long long chunk;
};

// The hyper-parameters of a tensor segment, as the chunk bodies below ask for them (hs(T)): one
// sgdm_args for the whole pass, or per parameter group.  A segment is uniform across the workgroup,
// so either way they sit in scalar registers.  The choice is a compile-time one: a run-time "table
// or no table" test in one functor costs upd::mom its fourth wave per SIMD.
struct uniform_args {
    sgdm_args h;
    __device__ __forceinline__ uniform_args(const pass_args& a, const gm_sgd_pgroup*, float lr)
        : h{a.gscale, lr, a.mu, a.wd} {}
    __device__ __forceinline__ const sgdm_args& operator()(const gm_tensor&) const { return h; }
};

// gm_group_sumsq_pg: rate scale and weight decay from the tensor's entry of the device group table
// (index clamped to the table); the group's rate is the fp64 product rounded once
struct pgroup_args {
    float gscale, lr, mu;
    const gm_sgd_pgroup* __restrict__ pg;
    unsigned last;  // npgroups - 1
    __device__ __forceinline__ pgroup_args(const pass_args& a, const gm_sgd_pgroup* pg, float lr)
        : gscale(a.gscale), lr(lr), mu(a.mu), pg(pg), last((unsigned)(a.npg - 1)) {}
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

// The sums, fused with the update of form U: one chunk body with one functor.  The rate is read
// once per workgroup - the argument, or *lrs (a uniform load that ends in a scalar register as the
// argument does).  TOT (gm_group_sumsq_clip's sums launch, U none): mom is null, or the buffers
// the apply launch will stream - for the 16-byte path only.
enum class body { few, runs };

template <upd U, body B, class H, bool TOT>
__global__ __launch_bounds__(256) void k_group_sumsq(pass_args a, const gm_tensor* __restrict__ tab,
                                                     float* const* __restrict__ mom, const gm_sgd_pgroup* __restrict__ pg,
                                                     double* __restrict__ rows) {
    const H hs(a, pg, a.lrs ? a.lrs->lr : a.lr);
    if constexpr (B == body::few) chunk_sums<U, 8, H, TOT>(tab, mom, a.nt, a.total, a.ngroups, hs, a.chunk, rows);
    else chunk_sums_runs<U, H, TOT>(tab, mom, a.nt, a.total, a.ngroups, hs, a.chunk, rows);
}

// The apply launch of gm_group_sumsq_clip: coefficient, rate and the skip decision are what the
// finalize launch left in *clip, read once per workgroup (uniform loads, as lrs->lr above).  A
// skipped step returns before it touches anything.  (rows: unused - one signature for both.)
template <upd U, class H>
__global__ __launch_bounds__(256) void k_group_apply(pass_args a, const gm_tensor* __restrict__ tab,
                                                     float* const* __restrict__ mom, const gm_sgd_pgroup* __restrict__ pg,
                                                     double* __restrict__ rows) {
    if (a.clip->skipped_last) return;  // (uniform)
    chunk_apply<U>(tab, mom, a.nt, a.total, H(a, pg, a.clip->lr), a.clip->coef, a.chunk);
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

// The finalize of every entry: the group sums, then what thread 0 owes the state the entry gave -
//   gate  the gate's rule on the finished sums (not on a skipped step);
//   lrs   the schedule's advance, after the sums and the gate's rule (the pass that read the old
//         rate ended before this launch began);
//   clip  (with lrs; between the sums launch and the apply launch) first of all the clip's rule
//         on the total from the column behind the rows, and the rate handed to the apply launch
//         before the schedule advances - which it does on a skipped step too (greedymml.h).
__global__ __launch_bounds__(kFinT) void k_group_finalize(const double* __restrict__ rows, int nrows,
                                                          int ngroups, double* __restrict__ out, void* gate,
                                                          int gate_n, gm_lr_state* lrs, gm_clip_state* clip) {
    __shared__ double tot_s[2 * kMaxGroups];
    __shared__ double tot_t[1];
    column_totals(rows, nrows, 2 * ngroups, out, tot_s);
    if (gate == nullptr && lrs == nullptr) return;  // (uniform; a clip comes with a rate)
    if (clip) {
        __syncthreads();  // (column_totals' LDS is read no more)
        column_totals(rows + (size_t)nrows * 2 * ngroups, nrows, 1, nullptr, tot_t);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int skipped = clip ? clip_decide(tot_t[0], clip) : 0;
        if (gate != nullptr && !skipped) gate_rule(tot_s, gate, gate_n);
        if (clip) clip->lr = lrs->lr;
        if (lrs) lr_advance(lrs);
        if (clip) clip_count(clip);
    }
}

}  // namespace gm

using namespace gm;

extern "C" size_t gm_group_sumsq_scratch(long long total) {
    if (total <= 0) return 0;
    const long long nb = (total + chunk_elems(total) - 1) / chunk_elems(total);
    return (size_t)nb * 2 * kMaxGroups * sizeof(double);
}

// What an entry point asks of the launch path.
struct pass_spec {
    const char* entry;  // the entry's name in its messages ("group_sumsq_lr")
    const gm_tensor* table;
    float* const* mom;  // the buffers of upd::mom and nest
    int nt;
    long long total;
    int ngroups;
    sgdm_args h;  // (h.lr: the rate where lrs is null)
    upd form;
    gm_lr_state* lrs;          // the device rate (null: h.lr, the argument)
    const gm_sgd_pgroup* pg;   // with lrs: the device group table (null: h.wd for every tensor)
    int npg;
    gm_clip_state* clip;       // with lrs: the sums launch, the clip's finalize, the apply launch
    double* out;
    void* scratch;
    size_t scratch_bytes;
    void* gate;  // optional (null: sums only)
    int gate_n;
    void* stream;
};

using kernel_t = void (*)(pass_args, const gm_tensor*, float* const*, const gm_sgd_pgroup*, double*);

template <upd U, class H>
static kernel_t fused_kernel(bool few) {
    return few ? k_group_sumsq<U, body::few, H, false> : k_group_sumsq<U, body::runs, H, false>;
}

template <upd U>
static kernel_t apply_kernel(bool pg) {
    return pg ? k_group_apply<U, pgroup_args> : k_group_apply<U, uniform_args>;
}

template <upd U>
static kernel_t table_or_not(bool pg, bool few) {
    return pg ? fused_kernel<U, pgroup_args>(few) : fused_kernel<U, uniform_args>(few);
}

// The kernel of (form, functor, body) - the fused pass, or the clipped entry's apply launch.  Null:
// a combination no entry point asks for (a table owns a weight decay, so there is no none or sgd
// over it; Nesterov's step without a table is the clipped entry's alone).
static kernel_t kernel_of(upd form, bool pg, bool few, bool apply) {
    switch (form) {
        case upd::none:
            return apply || pg ? nullptr : fused_kernel<upd::none, uniform_args>(few);
        case upd::sgd:
            return apply ? apply_kernel<upd::sgd>(pg) : (pg ? nullptr : fused_kernel<upd::sgd, uniform_args>(few));
        case upd::decay:
            return apply ? apply_kernel<upd::decay>(pg) : table_or_not<upd::decay>(pg, few);
        case upd::mom:
            return apply ? apply_kernel<upd::mom>(pg) : table_or_not<upd::mom>(pg, few);
        case upd::nest:
            return apply ? apply_kernel<upd::nest>(pg) : (pg ? fused_kernel<upd::nest, pgroup_args>(few) : nullptr);
    }
    return nullptr;
}

// The launch path of every entry point: shared checks, chunking, the kernel of (form, functor,
// group count), finalize; for the clipped entry the sums, the finalize, the apply.
static int group_sumsq(const pass_spec& s) {
    const int ngroups = s.ngroups;
    // (main, bypass) groups per branch: 4 for the two-branch gate, 2 nb for the N-branch one (nb in
    // the state: the rule reads 4 nb sums)
    GM_REQUIRE(!s.gate || (s.gate_n ? (ngroups >= 4 && ngroups % 2 == 0) : ngroups == 4),
               "group_sumsq_gate: %d groups do not match the %s gate", ngroups, s.gate_n ? "N-branch" : "two-branch");
    GM_REQUIRE(s.table && s.nt >= 1 && s.total >= 1, "group_sumsq: empty tensor table");
    GM_REQUIRE(ngroups >= 1 && ngroups <= kMaxGroups, "group_sumsq: ngroups must be 1..%d", kMaxGroups);
    // (the total's column lies behind the rows in the scratch, which is sized for kMaxGroups)
    GM_REQUIRE(!s.clip || ngroups < kMaxGroups, "group_sumsq_clip: ngroups must be 1..%d", kMaxGroups - 1);
    GM_REQUIRE(s.out, "group_sumsq: null output");
    const long long chunk = chunk_elems(s.total);
    GM_REQUIRE((s.total + chunk - 1) / chunk < (1ll << 31), "group_sumsq: too many elements");
    GM_REQUIRE(s.scratch && s.scratch_bytes >= gm_group_sumsq_scratch(s.total),
               "group_sumsq: scratch %zu < %zu bytes", s.scratch_bytes, gm_group_sumsq_scratch(s.total));
    const int nb = (int)((s.total + chunk - 1) / chunk);
    const bool few = ngroups <= 8;  // else the N-branch gates (C5: 12 branches -> 24 groups)
    const kernel_t update = kernel_of(s.form, s.pg != nullptr, few, s.clip != nullptr);
    GM_REQUIRE(update, "%s: no kernel for this update form", s.entry);
    hipStream_t st = as_stream(s.stream);
    double* rows = (double*)s.scratch;
    const pass_args a{s.nt, s.total, ngroups, s.h.gscale, s.h.lr, s.h.mu, s.h.wd, s.lrs, s.npg, s.clip, chunk};
    // the clipped entry: the sums alone first (the buffers, where the apply launch will stream
    // them, for the 16-byte path only), and the update behind the finalize
    const kernel_t sums = !s.clip ? update
                                  : (few ? k_group_sumsq<upd::none, body::few, uniform_args, true>
                                         : k_group_sumsq<upd::none, body::runs, uniform_args, true>);
    sums<<<nb, 256, 0, st>>>(a, s.table, !s.clip || has_buffer(s.form) ? s.mom : nullptr, s.pg, rows);
    int rc = check_launch("k_group_sumsq");
    if (rc) return rc;
    k_group_finalize<<<1, kFinT, 0, st>>>(rows, nb, ngroups, s.out, s.gate, s.gate && s.gate_n ? 1 : 0, s.lrs, s.clip);
    rc = check_launch("k_group_finalize");
    if (rc || !s.clip) return rc;
    update<<<nb, 256, 0, st>>>(a, s.table, s.mom, s.pg, rows);
    return check_launch("k_group_apply");
}

// The update's argument rules, stated once; each entry applies them under its own name.  pgroups
// (an entry with a parameter-group table): the table owns the weight decay.
static int check_update(const char* entry, float* const* mom, float momentum, float weight_decay, int nesterov,
                        const gm_sgd_pgroup* pgroups, int npgroups) {
    GM_REQUIRE(!pgroups || (npgroups >= 1 && npgroups <= GM_SGD_MAX_PGROUPS), "%s: npgroups must be 1..%d", entry,
               GM_SGD_MAX_PGROUPS);
    GM_REQUIRE(std::isfinite(momentum) && momentum >= 0.f, "%s: momentum must be finite and >= 0", entry);
    GM_REQUIRE(std::isfinite(weight_decay) && weight_decay >= 0.f, "%s: weight_decay must be finite and >= 0", entry);
    GM_REQUIRE(!pgroups || weight_decay == 0.f,
               "%s: the parameter-group table owns the weight decay (weight_decay must be 0)", entry);
    GM_REQUIRE(!nesterov || momentum > 0.f, "%s: nesterov requires a momentum > 0", entry);
    GM_REQUIRE((mom != nullptr) == (momentum != 0.f),
               "%s: momentum buffers must be given if and only if momentum != 0", entry);
    return 0;
}

// The update form an entry's arguments ask for (after check_update)
static upd form_of(float* const* mom, bool decay, int nesterov) {
    return mom ? (nesterov ? upd::nest : upd::mom) : (decay ? upd::decay : upd::sgd);
}

extern "C" int gm_group_sumsq(const gm_tensor* table, int nt, long long total, int ngroups, float gscale,
                              float lr, double* out, void* scratch, size_t scratch_bytes, void* stream) {
    return group_sumsq({"group_sumsq", table, nullptr, nt, total, ngroups, {gscale, lr, 0.f, 0.f},
                        lr != 0.f ? upd::sgd : upd::none, nullptr, nullptr, 0, nullptr, out, scratch, scratch_bytes,
                        nullptr, 0, stream});
}

extern "C" int gm_group_sumsq_gate(const gm_tensor* table, int nt, long long total, int ngroups, float gscale,
                                   float lr, double* out, void* scratch, size_t scratch_bytes, void* gate,
                                   int gate_n, void* stream) {
    GM_REQUIRE(gate, "group_sumsq_gate: null gate state");
    return group_sumsq({"group_sumsq_gate", table, nullptr, nt, total, ngroups, {gscale, lr, 0.f, 0.f},
                        lr != 0.f ? upd::sgd : upd::none, nullptr, nullptr, 0, nullptr, out, scratch, scratch_bytes,
                        gate, gate_n, stream});
}

extern "C" int gm_group_sumsq_sgdm(const gm_tensor* table, float* const* mom, int nt, long long total,
                                   int ngroups, float gscale, float lr, float momentum, float weight_decay,
                                   double* out, void* scratch, size_t scratch_bytes, void* gate, int gate_n,
                                   void* stream) {
    const char* entry = "group_sumsq_sgdm";
    const int rc = check_update(entry, mom, momentum, weight_decay, 0, nullptr, 0);
    if (rc) return rc;
    // (this entry's update runs at any weight decay: 0 is the decay form with wd 0)
    return group_sumsq({entry, table, mom, nt, total, ngroups, {gscale, lr, momentum, weight_decay},
                        form_of(mom, true, 0), nullptr, nullptr, 0, nullptr, out, scratch, scratch_bytes, gate, gate_n,
                        stream});
}

extern "C" int gm_group_sumsq_lr(const gm_tensor* table, float* const* mom, int nt, long long total, int ngroups,
                                 float gscale, gm_lr_state* lr, float momentum, float weight_decay, double* out,
                                 void* scratch, size_t scratch_bytes, void* gate, int gate_n, void* stream) {
    const char* entry = "group_sumsq_lr";
    GM_REQUIRE(lr, "%s: null lr state", entry);
    const int rc = check_update(entry, mom, momentum, weight_decay, 0, nullptr, 0);
    if (rc) return rc;
    return group_sumsq({entry, table, mom, nt, total, ngroups, {gscale, 0.f, momentum, weight_decay},
                        form_of(mom, weight_decay != 0.f, 0), lr, nullptr, 0, nullptr, out, scratch, scratch_bytes, gate,
                        gate_n, stream});
}

extern "C" int gm_group_sumsq_pg(const gm_tensor* table, float* const* mom, int nt, long long total, int ngroups,
                                 float gscale, gm_lr_state* lr, const gm_sgd_pgroup* pgroups, int npgroups,
                                 float momentum, int nesterov, double* out, void* scratch, size_t scratch_bytes,
                                 void* gate, int gate_n, void* stream) {
    const char* entry = "group_sumsq_pg";
    GM_REQUIRE(lr, "%s: null lr state", entry);
    GM_REQUIRE(pgroups, "%s: null parameter-group table", entry);
    const int rc = check_update(entry, mom, momentum, 0.f, nesterov, pgroups, npgroups);
    if (rc) return rc;
    return group_sumsq({entry, table, mom, nt, total, ngroups, {gscale, 0.f, momentum, 0.f}, form_of(mom, true, nesterov),
                        lr, pgroups, npgroups, nullptr, out, scratch, scratch_bytes, gate, gate_n, stream});
}

extern "C" int gm_group_sumsq_clip(const gm_tensor* table, float* const* mom, int nt, long long total, int ngroups,
                                   float gscale, gm_lr_state* lr, const gm_sgd_pgroup* pgroups, int npgroups,
                                   float momentum, float weight_decay, int nesterov, gm_clip_state* clip,
                                   double* out, void* scratch, size_t scratch_bytes, void* gate, int gate_n,
                                   void* stream) {
    const char* entry = "group_sumsq_clip";
    GM_REQUIRE(clip, "%s: null clip state", entry);
    GM_REQUIRE(lr, "%s: null lr state", entry);
    const int rc = check_update(entry, mom, momentum, weight_decay, nesterov, pgroups, npgroups);
    if (rc) return rc;
    return group_sumsq({entry, table, mom, nt, total, ngroups, {gscale, 0.f, momentum, weight_decay},
                        form_of(mom, pgroups || weight_decay != 0.f, nesterov), lr, pgroups, pgroups ? npgroups : 0, clip,
                        out, scratch, scratch_bytes, gate, gate_n, stream});
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
