// Training-mode BatchNorm2d over NHWC bf16 activations, fused with the residual
// add and ReLU that follow it in the torchvision ResNet blocks (the reference's
// trunk, src/model.py:65-106 via torchvision.models.resnet18).
//
// Forward  y = relu?( (x - mean) * invstd * gamma + beta  (+ residual) )
//   1. k_bn_reduce<FWD>: per-block fp32 partial sums of x and x^2 per channel; the
//      last-arriving block (agent-scope release/acquire ticket) combines the
//      partials in fp64 (fixed order: deterministic), writes save_mean/save_invstd,
//      the per-channel affine coefficients and the running-stat update
//      (momentum, unbiased variance - torch.nn.functional.batch_norm semantics).
//   2. k_bn_apply: one pass, 16-byte vectors, coefficients held in registers.
// Backward (dz = dy * (y > 0) when relu):
//   1. k_bn_reduce<BWD>: S1 = sum dz, S2 = sum dz*(x-mean) -> dbeta = S1,
//      dgamma = S2*invstd, dx = a*dz + b*x + c per channel.
//   2. k_bn_apply_bwd: dx (and dres = dz for the residual branch).
// Bytes per element (bf16): fwd 2 (stats) + 4..6 (apply); bwd 4..6 + 6..8.
// The apply kernels are templated on the element type E: bf16 (the performance trunk) or
// fp32 (the reference-precision trunk, gm_bn_*_f32, whose reduce is k_bn_reduce_f64);
// k_bn_reduce and the single-launch fused kernels are bf16 only.
// Each shared part has one definition, in this order: the element rules (form_dz, form_dx,
// form_y, store_y) and accum_vals; the per-channel coefficients (fwd_coef, bwd_coef), their
// side outputs (fwd_store, bwd_store) and the batch counter (count_batch); the strip of a reduce
// block (Strip, store_partial_row) and the partial-row combine (combine_rows); the folded
// kernels' band_loop; the coefficient hand-off (combine_coefs, handoff_coefs); then the
// kernels, and on the host launch_apply / launch_apply_bwd, apply_args, fwd_groups /
// bwd_groups and the two shape rules (shape_ok, stats_shape_ok).
#include <cstdlib>
#include <initializer_list>
#include <type_traits>

#include "gm_common.h"

namespace gm {
namespace {

constexpr int kT = 256;          // threads per block
constexpr int kMaxC = 2048;      // channels supported (ResNet-50 ends at 2048)
constexpr size_t kHdr = 256;     // scratch header (ticket counters)
constexpr int kMaxRC = 512;      // row chunks per channel slice (partials the last block combines)
constexpr int kRedF = 4096;      // LDS floats of the row-group combine (rpp * 2 * SW == 4096)

// 2-D reduce grid: (row chunk, 64-channel slice), ~512 blocks (2x for large maps).  Every block
// streams a [rows x SW] strip (SW = min(C, 64) channels, 128-B row segments),
// unrolled x8 so ~32 KB per block is in flight, and writes one partial row of
// 2*SW floats; ONE ticketed level per slice: the last-arriving block combines the
// slice's <= kMaxRC partial rows with all 256 threads (16-B sc1 loads, all in
// flight at once, fp64, fixed order) and finalizes.  One dependent memory round
// trip after the ticket instead of two ticket levels: the small maps of layer3/4
// are latency-, not bandwidth-bound.
struct Plan {
    int SW, tpr_log, rpp;  // slice width, log2(threads per row), rows per pass
    int nslice, nrc;       // slices, row chunks per slice
    long long rpb;         // rows per block
    size_t off_coef, off_p1, bytes;
};

inline int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

constexpr int kBnBlocks = 512;  // workgroups of a reduce launch (make_plan)

inline Plan make_plan(long long M, int C) {
    Plan p;
    p.SW = C < 64 ? C : 64;
    p.tpr_log = ilog2(p.SW / 8);
    p.rpp = kT >> p.tpr_log;
    p.nslice = C / p.SW;
    long long want = kBnBlocks / p.nslice;
    if (M * C >= (16ll << 20)) want *= 2;  // large maps: bandwidth-bound, more blocks
    if (want < 1) want = 1;
    if (want > kMaxRC) want = kMaxRC;
    long long rpb = (M + want - 1) / want;
    rpb = (rpb + p.rpp - 1) / p.rpp * p.rpp;
    p.rpb = rpb;
    p.nrc = (int)((M + rpb - 1) / rpb);
    const size_t cnt = (size_t)p.nslice * sizeof(unsigned);
    p.off_coef = (cnt + kHdr - 1) / kHdr * kHdr;
    p.off_p1 = p.off_coef + (size_t)4 * C * sizeof(float);
    p.bytes = p.off_p1 + (size_t)p.nslice * p.nrc * 2 * p.SW * sizeof(double);  // fp64 partials (fp32 path)
    return p;
}

inline size_t scratch_bytes(long long M, int C) { return make_plan(M, C).bytes; }

__device__ __forceinline__ void unpack8(uint4 u, float* f) {
    f[0] = bf_lo(u.x); f[1] = bf_hi(u.x); f[2] = bf_lo(u.y); f[3] = bf_hi(u.y);
    f[4] = bf_lo(u.z); f[5] = bf_hi(u.z); f[6] = bf_lo(u.w); f[7] = bf_hi(u.w);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    return make_uint4(pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7]));
}

// The ReLU mask of 8 stored bf16 values as one byte (bit j: value j > 0 - the bf16 half in
// 0x0001 .. 0x7f80, positive and not NaN: exactly the backward's y > 0 test on the stored y, also
// for the NaN poison a spin timeout writes), and back as 8 bf16 values (1.0 where set) that the
// y-mask code paths test unchanged
__device__ __forceinline__ unsigned mask_byte(uint4 w) {
    const unsigned v[4] = {w.x, w.y, w.z, w.w};
    unsigned b = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b |= ((v[k] & 0xffffu) - 1u < 0x7f80u ? 1u : 0u) << (2 * k);
        b |= ((v[k] >> 16) - 1u < 0x7f80u ? 1u : 0u) << (2 * k + 1);
    }
    return b;
}
__device__ __forceinline__ uint4 mask_vals(unsigned b) {
    unsigned v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        v[k] = ((b >> (2 * k)) & 1u ? 0x3f80u : 0u) | ((b >> (2 * k + 1)) & 1u ? 0x3f800000u : 0u);
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// Pin loaded values at this point: every load issued before is complete here, and none is sunk
// past it to its first use (the compiler otherwise issues a streaming loop's loads one round
// trip at a time - the ReLU mask bytes after the 16-B vectors had landed)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // a 16-B vector as one register tuple
__device__ __forceinline__ uint4 u4(u32x4 w) { return make_uint4(w.x, w.y, w.z, w.w); }
__device__ __forceinline__ void pin(u32x4& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(u32x4& v, u32x4& w) { asm volatile("" : "+v"(v), "+v"(w)); }  // one wait for both
__device__ __forceinline__ void pin(uint4& v) {
    u32x4 w = {v.x, v.y, v.z, v.w};
    pin(w);
    v = u4(w);
}
__device__ __forceinline__ void pin(unsigned& v) { asm volatile("" : "+v"(v)); }

__device__ __forceinline__ uint4 ld_nt16(const uint4* p) {  // streamed once: nontemporal
    return u4(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)));
}
__device__ __forceinline__ void st_nt16(uint4* p, uint4 v) {
    const u32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(p));
}

// Per-view-group operands: a grouped launch (gm_bn_*_grouped_bf16) normalises G views
// stacked along the batch, each with its own parameters, statistics and scratch, in one
// grid (blockIdx.z = group); every kernel starts from group_args().
constexpr int kMaxBnG = 16;  // view groups per grouped launch (C5: 12 views)
struct BnGroup {
    const void* x;
    const void* dy;
    const void* y;
    const float* gamma;
    const float* beta;
    float* rmean;
    float* rvar;
    float* save_mean;
    float* save_invstd;
    float* dgamma;
    float* dbeta;
    long long* nbt;
    float* coef_out;
    const float* fcoef;
    const uint4* res;
    uint4* yout;
    uint4* dres_out;
    uint8_t* mask_out;      // fwd (relu + residual), optional: the ReLU mask, one byte per 8 channels
    const uint8_t* ymask;   // bwd: that mask in place of y (k_bn_bwd_fused<BWD_RELU, ..., YM>)
};

struct ReduceArgs {
    long long M;
    int C, tpr_log, relu, accumulate;
    int SW, nrc;
    long long rpb;
    const void* x;       // fwd: x; bwd: x   (E elements)
    const void* dy;      // bwd
    const void* y;       // bwd relu mask
    const float* gamma;
    const float* beta;
    float* rmean;
    float* rvar;
    float momentum, eps;
    float* save_mean;    // fwd: out; bwd: in
    float* save_invstd;  // fwd: out; bwd: in
    float* dgamma;
    float* dbeta;
    unsigned* counter;   // [nslice] tickets (zero between calls)
    long long* nbt;      // num_batches_tracked (fwd, may be null)
    float* coef;         // [4][C]
    float* part;         // [nslice][nrc][SW][2] fp32 per-block partials
    float* coef_out;     // fwd, optional: the affine coefficients sc[C], sh[C] for the backward
    const float* fcoef;  // BWD_RELUX: the forward's sc[C], sh[C]
    unsigned* gen;       // fused fwd: [nslice] generation words (coefficients published)
    const uint4* res;    // fused fwd: residual
    uint4* yout;         // fused fwd: output / fused bwd: dx
    uint4* dres_out;     // fused bwd: dres
    uint8_t* mask_out;   // fused fwd, optional: ReLU mask bytes (bit j: channel 8 v + j of vector v > 0)
    const uint8_t* ymask;  // fused bwd: the mask in place of y
    unsigned spin_limit; // fused: poll budget of the coefficient hand-off
    int redundant;       // fused, small maps: every block combines the partial rows itself
    unsigned long long scr_stride;  // bytes between the groups' coefficient + partial areas
    unsigned hdr_words;             // words between the groups' ticket / generation headers
    BnGroup grp[kMaxBnG];           // grp[blockIdx.z] replaces the per-group pointers above
};

// this block's group: its pointers and its slice of the scratch (tickets, coefficients,
// partials, generation words)
__device__ __forceinline__ ReduceArgs group_args(const ReduceArgs& a0) {
    ReduceArgs a = a0;
    const int g = blockIdx.z;
    const BnGroup& q = a0.grp[g];
    a.x = q.x; a.dy = q.dy; a.y = q.y;
    a.gamma = q.gamma; a.beta = q.beta; a.rmean = q.rmean; a.rvar = q.rvar;
    a.save_mean = q.save_mean; a.save_invstd = q.save_invstd;
    a.dgamma = q.dgamma; a.dbeta = q.dbeta; a.nbt = q.nbt;
    a.coef_out = q.coef_out; a.fcoef = q.fcoef;
    a.res = q.res; a.yout = q.yout; a.dres_out = q.dres_out;
    a.mask_out = q.mask_out; a.ymask = q.ymask;
    const unsigned long long off = (unsigned long long)g * a0.scr_stride;
    a.counter = a0.counter + g * a0.hdr_words;
    a.coef = reinterpret_cast<float*>(reinterpret_cast<char*>(a0.coef) + off);
    a.part = reinterpret_cast<float*>(reinterpret_cast<char*>(a0.part) + off);
    if (a0.gen) a.gen = a0.gen + g * a0.hdr_words;
    return a;
}

// sticky fault word of this translation unit (gm_device_faults): a fused launch whose
// coefficient hand-off timed out
__device__ unsigned g_bn_fault = 0;

// Wait (thread 0, bounded) until the slice's generation word moves past g0; on
// timeout raise the fault bit and return false in EVERY thread of the block (the
// caller then applies NaN coefficients instead of stale ones).
__device__ __forceinline__ bool wait_generation(const unsigned* gen, unsigned g0, unsigned limit, float* flag) {
    if (threadIdx.x == 0) {
        unsigned it = 0;
        bool ok = true;
        while (__hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g0) {
            if (++it >= limit) {
                ok = false;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        if (!ok) atomicOr(&g_bn_fault, GM_FAULT_BN_SPIN);
        *flag = ok ? 1.f : 0.f;
    }
    __syncthreads();
    return *flag != 0.f;
}

// BWD_RELUX: the relu mask recomputed from x and the forward's affine coefficients
// (z = x*sc + sh > 0, the forward's own fp32 value) instead of read back from y
enum { FWD = 0, BWD = 1, BWD_RELU = 2, BWD_RELUX = 3 };  // relu as a template arg: no per-load branch

// The element rules, each on 8 values (float[8]); every kernel below forms its values here.
// dz: dy where the forward's ReLU passed - y > 0 on the stored output (BWD_RELU; yf may be the
// mask_vals of its mask byte) or x*sc + sh > 0 recomputed (BWD_RELUX); BWD: dz = dy
template <int MODE>
__device__ __forceinline__ void form_dz(float* d, const float* xf, const float* yf, const float* fsc,
                                        const float* fsh) {
    if (MODE == BWD_RELU) {
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = yf[j] > 0.f ? d[j] : 0.f;
    }
    if (MODE == BWD_RELUX) {
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = fmaf(xf[j], fsc[j], fsh[j]) > 0.f ? d[j] : 0.f;
    }
}
// dx = ca*dz + cb*x + cc, or (CENTER, the fp32 path) ca*dz + cb*(x - mean) + cc
template <bool CENTER = false>
__device__ __forceinline__ void form_dx(float* o, const float* d, const float* xf, const float* ca, const float* cb,
                                        const float* cc, const float* mu = nullptr) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
        o[j] = CENTER ? fmaf(ca[j], d[j], fmaf(cb[j], xf[j] - mu[j], cc[j])) : fmaf(ca[j], d[j], fmaf(cb[j], xf[j], cc[j]));
}
// y = relu?(x*sc + sh (+ r)) in place
template <bool RES, bool RELU>
__device__ __forceinline__ void form_y(float* f, const float* r, const float* sc, const float* sh) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float z = fmaf(f[j], sc[j], sh[j]);
        if (RES) z += r[j];
        f[j] = RELU ? relu_nan(z) : z;
    }
}
// the bf16 store of y, with (MASK, where the caller gave a mask buffer) its ReLU mask byte
template <bool MASK, typename I>
__device__ __forceinline__ void store_y(uint4* y, uint8_t* mask, I i, const float* f) {
    const uint4 w = pack8(f);
    y[i] = w;
    if (MASK && mask) mask[i] = (uint8_t)mask_byte(w);
}

// one vector's terms of the statistics sums (zero vectors contribute nothing in every mode)
template <int MODE>
__device__ __forceinline__ void accum_vals(uint4 ux, uint4 ud, uint4 uy, const float* mu, float* s1, float* s2,
                                           const float* fsc = nullptr, const float* fsh = nullptr) {
    float xf[8];
    unpack8(ux, xf);
    if (MODE == FWD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s1[j] += xf[j];
            s2[j] = fmaf(xf[j], xf[j], s2[j]);
        }
    } else {
        float d[8], yf[8];
        unpack8(ud, d);
        if (MODE == BWD_RELU) unpack8(uy, yf);
        form_dz<MODE>(d, xf, yf, fsc, fsh);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s1[j] += d[j];
            s2[j] = fmaf(d[j], xf[j] - mu[j], s2[j]);
        }
    }
}

// accum_vals() on vector v of the launch's bf16 tensors
template <int MODE>
__device__ __forceinline__ void accum(const ReduceArgs& a, long long v, const float* mu, float* s1, float* s2,
                                      const float* fsc, const float* fsh) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    const uint4 ux = static_cast<const uint4*>(a.x)[v];
    const uint4 ud = MODE != FWD ? static_cast<const uint4*>(a.dy)[v] : z;
    const uint4 uy = MODE == BWD_RELU ? static_cast<const uint4*>(a.y)[v] : z;
    accum_vals<MODE>(ux, ud, uy, mu, s1, s2, fsc, fsh);
}

// per-channel operands of finalize(), loaded by every block BEFORE its ticket so the
// last block's dependent chain after the ticket has one memory round trip fewer
struct FinOps {
    float g, b, rm, rv;  // FWD: gamma, beta, running mean/var; BWD: gamma, -, save_mean, save_invstd
};

template <int MODE>
__device__ __forceinline__ FinOps fin_load(const ReduceArgs& a, int c) {
    FinOps f;
    f.g = a.gamma[c];
    if (MODE == FWD) {
        f.b = a.beta[c];
        f.rm = a.rmean ? a.rmean[c] : 0.f;
        f.rv = a.rmean ? a.rvar[c] : 0.f;
    } else {
        f.b = 0.f;
        f.rm = a.save_mean[c];
        f.rv = a.save_invstd[c];
    }
    return f;
}

// The per-channel arithmetic of finalize() on its own (fp64, one rounding to fp32 per output):
// every kernel that finalizes - the ticketed last block, the redundant combine, the
// statistics finalizes and the folded finalize + apply kernels, whose blocks other than the
// first keep the coefficients and store nothing - computes its coefficients here.
struct FwdCoef {
    float sc, sh, mean, invstd, rmean, rvar;
};
struct BwdCoef {
    float ca, cb, cc, c3, dg, db;
};

__device__ __forceinline__ FwdCoef fwd_coef(const ReduceArgs& a, double S1, double S2, double invM, const FinOps& f) {
    FwdCoef k;
    const double g = (double)f.g;
    const double mean = S1 * invM;
    double var = S2 * invM - mean * mean;
    if (var < 0.0) var = 0.0;
    const double invstd = 1.0 / sqrt(var + (double)a.eps);
    const double sc = g * invstd;
    k.sc = (float)sc;
    k.sh = (float)((double)f.b - mean * sc);
    k.mean = (float)mean;
    k.invstd = (float)invstd;
    const double m = (double)a.momentum;
    const double unb = a.M > 1 ? var * (double)a.M / (double)(a.M - 1) : var;
    k.rmean = (float)((1.0 - m) * (double)f.rm + m * mean);
    k.rvar = (float)((1.0 - m) * (double)f.rv + m * unb);
    return k;
}

template <bool CENTER>
__device__ __forceinline__ BwdCoef bwd_coef(double S1, double S2, double invM, const FinOps& f) {
    BwdCoef k;
    const double g = (double)f.g;
    const double mean = (double)f.rm;
    const double is = (double)f.rv;
    const double ca = g * is;
    const double cb = -g * is * is * is * S2 * invM;
    k.ca = (float)ca;
    k.cb = (float)cb;
    if (CENTER) {  // dx = ca*dz + cb*(x - mean) + cc (fp32 path: no cb*x - cb*mean cancellation)
        k.cc = (float)(-ca * S1 * invM);
        k.c3 = (float)mean;
    } else {
        k.cc = (float)(-ca * S1 * invM - cb * mean);
        k.c3 = 0.f;
    }
    k.dg = (float)(S2 * is);
    k.db = (float)S1;
    return k;
}

// num_batches_tracked += 1, by the thread that finalizes channel 0.  Not part of fwd_store: the
// callers place its read-modify-write round trip where it overlaps their loads - in fwd_store it
// sat between the coefficient stores and the generation word of the fused forward's hand-off,
// 0.5 - 1.3 us per launch that every waiting block paid
__device__ __forceinline__ void count_batch(const ReduceArgs& a, int c) {
    if (a.nbt && c == 0) *a.nbt += 1;
}

// the side outputs of a finalize: statistics, running averages, coefficient area(s) (FWD);
// coefficient area and parameter gradients (BWD)
template <bool SC1>
__device__ __forceinline__ void fwd_store(const ReduceArgs& a, int c, const FwdCoef& k) {
    const int C = a.C;
    a.coef[c] = k.sc;
    a.coef[C + c] = k.sh;
    if (SC1) {
        st_sc1(&a.coef[c], k.sc);
        st_sc1(&a.coef[C + c], k.sh);
    }
    if (a.coef_out) {
        a.coef_out[c] = k.sc;
        a.coef_out[C + c] = k.sh;
    }
    a.save_mean[c] = k.mean;
    a.save_invstd[c] = k.invstd;
    if (a.rmean) {
        a.rmean[c] = k.rmean;
        a.rvar[c] = k.rvar;
    }
}

template <bool SC1, bool CENTER>
__device__ __forceinline__ void bwd_store(const ReduceArgs& a, int c, const BwdCoef& k) {
    const int C = a.C;
    a.coef[c] = k.ca;
    a.coef[C + c] = k.cb;
    a.coef[2 * C + c] = k.cc;
    if (CENTER) a.coef[3 * C + c] = k.c3;
    if (SC1) {
        st_sc1(&a.coef[c], k.ca);
        st_sc1(&a.coef[C + c], k.cb);
        st_sc1(&a.coef[2 * C + c], k.cc);
    }
    if (a.accumulate) {
        a.dgamma[c] += k.dg;
        a.dbeta[c] += k.db;
    } else {
        a.dgamma[c] = k.dg;
        a.dbeta[c] = k.db;
    }
}

// SC1: the coefficients are published with write-through stores (read by the other
// blocks of the same launch in the fused forward, k_bn_fwd_fused)
template <int MODE, bool SC1 = false, bool CENTER = false>
__device__ __forceinline__ void finalize(const ReduceArgs& a, int c, double S1, double S2, double invM,
                                         const FinOps& f) {
    if (MODE == FWD) fwd_store<SC1>(a, c, fwd_coef(a, S1, S2, invM, f));
    else bwd_store<SC1, CENTER>(a, c, bwd_coef<CENTER>(S1, S2, invM, f));
}

// Cross-workgroup hand-off without fences (cdna_hip_programming.md, in-launch
// split-K recipe, sc1 form): partials are written with agent-scope atomic stores
// (write-through sc1), every wave drains vmcnt, the block barriers, lane 0 takes a
// relaxed agent-scope ticket; the block that draws the last ticket reads the
// partials back with agent-scope atomic loads (sc1), so no L2 write-back or
// invalidate is needed.  Returns true in that last block.

__device__ __forceinline__ bool ticket(unsigned* ctr, unsigned n, float* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tk = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = tk == n - 1;
        if (last) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // reset
        *flag = last ? 1.f : 0.f;
    }
    __syncthreads();
    return *flag != 0.f;
}

// A block's strip of the 2-D reduce grid (blockIdx.x = row chunk rc, blockIdx.y = slice cs):
// thread t holds the 8 channels from c0 (vector cv of a row of vpr vectors) of the rows
// r0, r0 + rpp, ... of [rbeg, rend).
struct Strip {
    int t, rc, cs, cg, r0, rpp, c0;
    long long vpr, cv, rbeg, rend;
    __device__ __forceinline__ explicit Strip(const ReduceArgs& a) {
        t = threadIdx.x;
        rc = blockIdx.x;
        cs = blockIdx.y;
        const int tpr = 1 << a.tpr_log;
        cg = t & (tpr - 1);
        r0 = t >> a.tpr_log;
        rpp = kT >> a.tpr_log;
        vpr = a.C >> 3;
        c0 = cs * a.SW + cg * 8;
        cv = c0 >> 3;
        rbeg = (long long)rc * a.rpb;
        rend = rbeg + a.rpb;
        if (rend > a.M) rend = a.M;
    }
};

// row-group combine in LDS, red[r0][SW][2] (rpp * 2SW == 4096 values), then the block's partial
// row with write-through stores (T: fp32 sums, or the fp64 sums of the reference-precision reduce)
template <typename T>
__device__ __forceinline__ void store_partial_row(const ReduceArgs& a, const Strip& sp, T* red, const T* s1,
                                                  const T* s2) {
    const int S2w = 2 * a.SW;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        red[sp.r0 * S2w + (sp.cg * 8 + j) * 2] = s1[j];
        red[sp.r0 * S2w + (sp.cg * 8 + j) * 2 + 1] = s2[j];
    }
    __syncthreads();
    T* p1 = reinterpret_cast<T*>(a.part) + ((size_t)sp.cs * a.nrc + sp.rc) * S2w;
    if (sp.t < S2w) {
        T acc = 0;
        for (int i = 0; i < sp.rpp; ++i) acc += red[i * S2w + sp.t];
        st_sc1(&p1[sp.t], acc);
    }
}

// Combine slice cs's nrc partial rows in fp64 (lane group of L threads per row, one float4
// each, G = 256/L row groups, rows g, g+G, ...; 16-B sc1 loads, fixed order: every block that
// combines computes the same sums) and call fin(t, S1, S2) in thread t < SW, channel cs * SW + t.
template <typename F>
__device__ __forceinline__ void combine_rows(const ReduceArgs& a, int cs, float* red, F fin) {
    const int t = threadIdx.x;
    const int SW = a.SW, S2w = 2 * SW;
    const int L = S2w >> 2, G = kT / L;  // L in {4..32}, G in {8..64}
    const int lv = t % L, g = t / L;
    const auto rq = rsrc_of(a.part + (size_t)cs * a.nrc * S2w);
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
    for (int i0 = g; i0 < a.nrc; i0 += 8 * G) {  // 8 independent 16-B loads in flight
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * G;
            v[u] = i < a.nrc ? ld_sc1_f32x4(rq, (unsigned)(i * S2w + 4 * lv) * 4u) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            d0 += (double)v[u].x; d1 += (double)v[u].y; d2 += (double)v[u].z; d3 += (double)v[u].w;
        }
    }
    __syncthreads();  // red[] is free again
    double* rd = reinterpret_cast<double*>(red);  // [G][S2w] doubles: G * S2w == 2 * kT <= kRedF / 2
    rd[g * S2w + 4 * lv + 0] = d0;
    rd[g * S2w + 4 * lv + 1] = d1;
    rd[g * S2w + 4 * lv + 2] = d2;
    rd[g * S2w + 4 * lv + 3] = d3;
    __syncthreads();
    if (t < SW) {
        double S1 = 0.0, S2 = 0.0;
        for (int i = 0; i < G; ++i) {
            S1 += rd[i * S2w + 2 * t];
            S2 += rd[i * S2w + 2 * t + 1];
        }
        fin(t, S1, S2);
    }
}

// The last block of a slice: combine the slice's partial rows and finalize its channels.
template <int MODE, bool SC1 = false>
__device__ __forceinline__ void combine_finalize(const ReduceArgs& a, int cs, float* red, const FinOps& fo) {
    if (MODE == FWD) count_batch(a, cs * a.SW + threadIdx.x);  // ahead of the row loads
    combine_rows(a, cs, red, [&](int t, double S1, double S2) {
        finalize<MODE, SC1>(a, cs * a.SW + t, S1, S2, 1.0 / (double)a.M, fo);
    });
}

// One launch: partial sums per (row chunk, channel slice) + one ticketed combine
// per slice + per-channel finalize.  bf16 only (E is kept in the kernel's name); the fp32
// reduce is k_bn_reduce_f64.
template <int MODE, typename E>
__global__ __launch_bounds__(kT) void k_bn_reduce(ReduceArgs a0) {
    static_assert(std::is_same<E, uint16_t>::value, "k_bn_reduce: bf16 (fp32: k_bn_reduce_f64)");
    const ReduceArgs a = group_args(a0);
    __shared__ float red[kRedF + 4];  // the one LDS object: row-group partials, flag
    const Strip sp(a);
    const int C = a.C, SW = a.SW, c0 = sp.c0, rpp = sp.rpp;
    const long long vpr = sp.vpr, cv = sp.cv, rend = sp.rend;

    float fsc[8], fsh[8];
    if (MODE == BWD_RELUX) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            fsc[j] = a.fcoef[c0 + j];
            fsh[j] = a.fcoef[C + c0 + j];
        }
    }
    float mu[8];
    if (MODE != FWD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) mu[j] = a.save_mean[c0 + j];
    }
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;

    long long r = sp.rbeg + sp.r0;
    const long long st = (long long)rpp * vpr;
    for (; r + 7 * rpp < rend; r += 8 * rpp) {
        const long long v = r * vpr + cv;
#pragma unroll
        for (int u = 0; u < 8; ++u) accum<MODE>(a, v + u * st, mu, s1, s2, fsc, fsh);
    }
    if (MODE == FWD && r < rend) {  // the tail as ONE predicated batch
        const uint4* X = static_cast<const uint4*>(a.x);
        uint4 vx[8];
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int u = 0; u < 8; ++u) vx[u] = X[(r + u * rpp < rend ? r + u * rpp : r) * vpr + cv];
#pragma unroll
        for (int u = 0; u < 8; ++u) accum_vals<MODE>(r + u * rpp < rend ? vx[u] : z, z, z, mu, s1, s2);
    } else {
        for (; r < rend; r += rpp) accum<MODE>(a, r * vpr + cv, mu, s1, s2, fsc, fsh);
    }

    store_partial_row(a, sp, red, s1, s2);
    FinOps fo{};
    if (sp.t < SW) fo = fin_load<MODE>(a, sp.cs * SW + sp.t);  // in flight with the partial store
    if (!ticket(a.counter + sp.cs, (unsigned)a.nrc, &red[kRedF])) return;
    combine_finalize<MODE>(a, sp.cs, red, fo);
}

// ---------------------------------------------------------------------------------
// The stem's max-pool backward gathered straight into its BatchNorm + ReLU backward
// (torchvision stem: relu(bn1(x)) -> MaxPool2d(3, 2, 1); reference src/model.py:65-106).
// The pool gradient dz (input resolution, 205 MB at C2) is never written: each thread owns
// a 2 x 2 block of input pixels (rows 2k, 2k+1, columns 2l, 2l+1) x 8 channels and gathers
// their pool gradient from the (at most) 2 x 2 windows (k..k+1, l..l+1) that can select
// them - one window read serves four pixels instead of the per-pixel gather's one (four
// times fewer L2 reads than k_maxpool_bwd) - summed in k_maxpool_bwd's order (window row,
// then column, ascending) and rounded to bf16 as k_maxpool_bwd stores it, then masked by
// the forward's ReLU (x*sc + sh > 0).  Pass 1 (APPLY = false) reduces S1 = sum dz,
// S2 = sum dz*(x - mean) per channel into partial rows + the ticketed fp64 combine and
// finalize of k_bn_reduce; pass 2 applies dx = ca*dz + cb*x + cc.  HBM: pass 1 reads x and
// the pooled gradient + argmax, pass 2 the same and writes dx - against k_maxpool_bwd
// (read pooled, write dz) + the BN backward (read dz and x twice, write dx).
// With xs (the forward's selected raw x per pooled output) pass 1 needs no pixel gather:
// S1 and S2 are linear in the per-pixel gradient, so they sum over the pooled outputs -
// dy_pool * mask(xs) and dy_pool * mask(xs) * (xs - mean) - reading the pooled gradient and
// xs (a quarter of the pixels, 2 x 51 MB at C2) instead of x, the gradient and the argmax.
// (The per-pixel bf16 rounding of the gathered gradient, which pass 2 applies to dx, is not
// applied to these sums: they are the fp32 sums of the same terms.)
struct StemPoolGeo {
    int Ng, H, W, P, Q;      // images per view group, input and pooled sizes
    long long items;         // owner blocks x channel groups per view group
    long long ipb;           // items per block (pass 1; a multiple of kT)
    const uint2* idx;        // [G*Ng][P][Q][C] window-relative argmax bytes
    const uint4* gp;         // [G*Ng][P][Q][C] bf16 pool gradient
    const uint4* xs;         // [G*Ng][P][Q][C] bf16 selected x (optional)
};

template <bool APPLY>
__global__ __launch_bounds__(kT) void k_stem_pool_bn_bwd(ReduceArgs a0, StemPoolGeo pg) {
    const ReduceArgs a = group_args(a0);
    __shared__ float red[kRedF + 4];
    const int t = threadIdx.x;
    const int C = a.C, C8 = C >> 3;
    const int g = blockIdx.z;
    const long long goff = (long long)g * pg.Ng * pg.P * pg.Q * C8;  // this group's pooled vectors
    const uint2* __restrict__ IDX = pg.idx + goff;
    const uint4* __restrict__ GP = pg.gp + goff;
    const uint4* __restrict__ X = static_cast<const uint4*>(a.x);
    float fsc[8], fsh[8], mu[8], ca[8], cb[8], cc[8];
    const int cg0 = t % C8;  // fixed per thread in pass 1 (kT and the block base are multiples of C8)
    auto ld_coef = [&](const float* p, int cg, float* v) {
        const float4 u0 = *reinterpret_cast<const float4*>(p + cg * 8);
        const float4 u1 = *reinterpret_cast<const float4*>(p + cg * 8 + 4);
        v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
    };
    ld_coef(a.fcoef, cg0, fsc);
    ld_coef(a.fcoef + C, cg0, fsh);
    if (!APPLY) ld_coef(a.save_mean, cg0, mu);
    else {
        ld_coef(a.coef, cg0, ca);
        ld_coef(a.coef + C, cg0, cb);
        ld_coef(a.coef + 2 * C, cg0, cc);
    }
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
    // one owner block x channel group, in two phases (loads, then arithmetic) so that a
    // thread keeps UI items' loads in flight together
    struct Item {
        uint2 iv[4];
        uint4 gq[4], xv[4];
        int n, k, l, cg;
        unsigned okw;  // bit u: window u exists (a select on the loaded value instead would
                       // make hipcc branch around the load and drain vmcnt per window)
    };
    // 32-bit index math (a group's pooled and input vectors are < 2^31: checked on the host)
    const unsigned QC8 = (unsigned)pg.Q * C8, WC8 = (unsigned)pg.W * C8;
    auto load = [&](long long i64, Item& it) {
        const unsigned i = (unsigned)i64;
        const unsigned ob = i / (unsigned)C8;
        it.cg = (int)(i - ob * (unsigned)C8);
        const unsigned r1 = ob / (unsigned)pg.Q;
        it.l = (int)(ob - r1 * (unsigned)pg.Q);
        const unsigned nn = r1 / (unsigned)pg.P;
        it.k = (int)(r1 - nn * (unsigned)pg.P);
        it.n = (int)nn;
        const int k = it.k, l = it.l;
        // windows (k + wr, l + wc); pixel (dh, dw) of the block is covered by window
        // (k + wr, l + wc) iff wr <= dh and wc <= dw (and the window exists)
        const unsigned o0 = i;  // the block's own window (k, l) = pooled vector i
        it.okw = 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int wr = u >> 1, wc = u & 1;
            const bool ok = k + wr < pg.P && l + wc < pg.Q;
            const unsigned o = ok ? o0 + (unsigned)wr * QC8 + (unsigned)wc * (unsigned)C8 : o0;
            it.iv[u] = IDX[o];
            it.gq[u] = GP[o];
            it.okw |= ok ? (1u << u) : 0u;
        }
        const unsigned x0 = ((nn * (unsigned)pg.H + 2u * (unsigned)k) * (unsigned)pg.W + 2u * (unsigned)l) * C8 + it.cg;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int dh = q >> 1, dw = q & 1;
            const bool in = 2 * k + dh < pg.H && 2 * l + dw < pg.W;
            it.xv[q] = ld_nt16(&X[in ? x0 + (unsigned)dh * WC8 + (unsigned)dw * (unsigned)C8 : x0]);
        }
    };
    auto compute = [&](const Item& it) {
        const int n = it.n, k = it.k, l = it.l, cg = it.cg;
        float gv[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) unpack8(it.gq[u], gv[u]);
        // a missing window's argmax bytes become 0xff (never a position 0..8): one select per
        // window here instead of a mask AND per channel compare below
        uint2 ivm[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) ivm[u] = ((it.okw >> u) & 1u) ? it.iv[u] : make_uint2(~0u, ~0u);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int dh = q >> 1, dw = q & 1;
            const int h = 2 * k + dh, w = 2 * l + dw;
            if (h >= pg.H || w >= pg.W) continue;
            float d[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int wr = u >> 1, wc = u & 1;
                if (wr > dh || wc > dw) continue;
                // position of pixel (h, w) in window (k + wr, l + wc): rows 2(k+wr)-1 .., cols 2(l+wc)-1 ..
                // (h - 2k = dh, w - 2l = dw: a compile-time constant per (q, u))
                const uint32_t pos = (uint32_t)((dh - 2 * wr + 1) * 3 + (dw - 2 * wc + 1));
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t b = ((j < 4 ? ivm[u].x : ivm[u].y) >> (8 * (j & 3))) & 0xffu;
                    if (b == pos) d[j] += gv[u][j];
                }
            }
            float xf[8];
            unpack8(it.xv[q], xf);
            // (dz, dx and the partial row stay written out in this kernel: form_dz / form_dx /
            // store_partial_row compute the same but moved its register figures, 120 -> 117, 229 -> 231)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float dr = __uint_as_float((uint32_t)Elem<uint16_t>::f2bf(d[j]) << 16);  // k_maxpool_bwd's bf16 dz
                d[j] = fmaf(xf[j], fsc[j], fsh[j]) > 0.f ? dr : 0.f;
            }
            if (APPLY) {
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = fmaf(ca[j], d[j], fmaf(cb[j], xf[j], cc[j]));
                st_nt16(&reinterpret_cast<uint4*>(a.yout)[(((long long)n * pg.H + h) * pg.W + w) * C8 + cg], pack8(o));
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    s1[j] += d[j];
                    s2[j] = fmaf(d[j], xf[j] - mu[j], s2[j]);
                }
            }
        }
    };
    auto item = [&](long long i) {
        Item it;
        load(i, it);
        compute(it);
    };
    if (APPLY) {
        // (the coefficient registers hold channel group cg0: a grid-stride step is a multiple of C8)
        // two items' loads in flight per thread
        const long long stride = (long long)gridDim.x * kT;
        long long i = (long long)blockIdx.x * kT + t;
        for (; i + stride < pg.items; i += 2 * stride) {
            Item u, v;
            load(i, u);
            load(i + stride, v);
            compute(u);
            compute(v);
        }
        if (i < pg.items) item(i);
        return;
    }
    const int rc = blockIdx.x;
    const long long i0 = (long long)rc * pg.ipb;
    const long long i1 = i0 + pg.ipb < pg.items ? i0 + pg.ipb : pg.items;
    if (pg.xs) {
        // pooled outputs i (an item index is a pooled (n, k, l, cg) vector: the same decode)
        const uint4* __restrict__ XS = pg.xs + goff;
        for (long long i = i0 + t; i < i1; i += 4 * kT) {
            uint4 gq[4], xq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // four vectors' loads in flight
                const long long iu = i + u * kT < i1 ? i + u * kT : i;
                gq[u] = GP[iu];
                xq[u] = XS[iu];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i + u * kT >= i1) break;
                float gv[8], xf[8];
                unpack8(gq[u], gv);
                unpack8(xq[u], xf);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float d = fmaf(xf[j], fsc[j], fsh[j]) > 0.f ? gv[j] : 0.f;
                    s1[j] += d;
                    s2[j] = fmaf(d, xf[j] - mu[j], s2[j]);
                }
            }
        }
    } else {
        for (long long i = i0 + t; i < i1; i += kT) item(i);  // (two items in flight per thread: slower)
    }
    // row-group combine in LDS as k_bn_reduce: red[r0][SW][2], r0 = t / C8 (C8 threads per row)
    const int S2w = 2 * C, r0 = t / C8, rpp = kT / C8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        red[r0 * S2w + (cg0 * 8 + j) * 2] = s1[j];
        red[r0 * S2w + (cg0 * 8 + j) * 2 + 1] = s2[j];
    }
    __syncthreads();
    float* p1 = a.part + (size_t)rc * S2w;
    if (t < S2w) {
        float acc = 0.f;
        for (int i = 0; i < rpp; ++i) acc += red[i * S2w + t];
        st_sc1(&p1[t], acc);
    }
    FinOps fo{};
    if (t < C) fo = fin_load<BWD_RELUX>(a, t);
    if (!ticket(a.counter, (unsigned)a.nrc, &red[kRedF])) return;
    combine_finalize<BWD_RELUX>(a, 0, red, fo);
}

// Finalize of BatchNorm forward statistics whose per-workgroup partial rows were written by
// the producer (k_conv_stem's epilogue): one block per view group combines the rows in fp64
// (fixed order) and finalizes as k_bn_reduce's last block does.  a0.part / a0.coef: group 0's
// rows and coefficient area, the groups scr_stride bytes apart.
// 1024 threads per (64-channel slice, group): 32 lanes per partial row (one float4 each), 32
// row groups with 8 rows' loads in flight each (the producers' rows are many - a 3x3 layer-2
// convolution writes one per 64-pixel slab - and the combine sits on the forward's critical
// path), fp64, then the row groups combined in a fixed order.
constexpr int kFinT = 1024;
__device__ __forceinline__ void load_coef(const float* p, int cg, float* c);

// the residual-affine form's residual: r <- bf16(fmaf(r, sc, sh)) as floats, the 8 values a
// BatchNorm apply without ReLU stores (pack8's rounding) and the consuming apply reads back
__device__ __forceinline__ void res_affine(float* r, const float* sc, const float* sh) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = fmaf(r[j], sc[j], sh[j]);
    unpack8(pack8(r), r);
}

// the combine of the finalize kernels: sums of slice cs's nrc partial rows, (S1, S2) of channel
// cs * 64 + t in the threads t < 64 (rd: the block's [32][128] fp64 LDS)
__device__ __forceinline__ void fin_combine(const ReduceArgs& a, int cs, double (*rd)[128], double& S1, double& S2) {
    const int t = threadIdx.x;
    const int lv = t & 31, rg = t >> 5;
    const float4* rows = reinterpret_cast<const float4*>(a.part + (size_t)cs * a.nrc * 128);
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
    for (int i0 = rg; i0 < a.nrc; i0 += 8 * 32) {
        float4 v[8];  // clamped rows, all eight loads in flight, then the value select (a
#pragma unroll    // conditional load compiled to a branch and a full wait per row)
        for (int u = 0; u < 8; ++u) v[u] = rows[(size_t)min(i0 + u * 32, a.nrc - 1) * 32 + lv];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (i0 + u * 32 >= a.nrc) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            d0 += (double)v[u].x; d1 += (double)v[u].y; d2 += (double)v[u].z; d3 += (double)v[u].w;
        }
    }
    rd[rg][4 * lv] = d0; rd[rg][4 * lv + 1] = d1; rd[rg][4 * lv + 2] = d2; rd[rg][4 * lv + 3] = d3;
    __syncthreads();
    S1 = 0.0;
    S2 = 0.0;
    if (t < 64) {
        for (int i = 0; i < kFinT / 32; ++i) {
            S1 += rd[i][2 * t];
            S2 += rd[i][2 * t + 1];
        }
    }
}

// the forward finalize's per-channel operands: every thread, no branch (a conditional load
// here cost wave 0 a waited round trip before its row loads); threads t >= 64 load channel
// t % 64's again, unused
__device__ __forceinline__ FinOps fin_load_fwd_all(const ReduceArgs& a, int cs) {
    FinOps fo;
    const int c = cs * 64 + (threadIdx.x & 63);
    const float* rm = a.rmean ? a.rmean : a.gamma;
    const float* rv = a.rmean ? a.rvar : a.gamma;
    fo.g = a.gamma[c];
    fo.b = a.beta[c];
    fo.rm = rm[c];
    fo.rv = rv[c];
    return fo;
}

__global__ __launch_bounds__(kFinT) void k_bn_stats_finalize(ReduceArgs a0) {
    const ReduceArgs a = group_args(a0);
    __shared__ double rd[kFinT / 32][128];
    const int t = threadIdx.x, cs = blockIdx.y;  // channel slice cs (64 channels)
    const FinOps fo = fin_load_fwd_all(a, cs);
    double S1, S2;
    fin_combine(a, cs, rd, S1, S2);
    if (t < 64) {
        finalize<FWD>(a, cs * 64 + t, S1, S2, 1.0 / (double)a.M, fo);  // (rm / rv unused without rmean)
        count_batch(a, cs * 64 + t);
    }
}

// The backward's statistics (sum dz, sum dz * (x - mean) per channel) from producer partial
// rows (the input-gradient convolution's epilogue, gm_conv2d_dgrad_grouped_bn_stats_bf16):
// combined like k_bn_stats_finalize, then finalize<BWD> - dgamma / dbeta (accumulate) and the
// apply's coefficients ca, cb, cc at coef0 + g * cstride (the partial rows' group blocks are
// packed: no room for 3 C coefficients at their end).
__global__ __launch_bounds__(kFinT) void k_bn_bwd_stats_finalize(ReduceArgs a0, float* coef0, long long cstride) {
    ReduceArgs a = group_args(a0);
    a.coef = coef0 + blockIdx.z * cstride;
    __shared__ double rd[kFinT / 32][128];
    const int t = threadIdx.x, cs = blockIdx.y;
    const FinOps fo = fin_load<BWD>(a, cs * 64 + (t & 63));  // every thread: no branch, no early wait
    double S1, S2;
    fin_combine(a, cs, rd, S1, S2);
    if (t < 64) finalize<BWD>(a, cs * 64 + t, S1, S2, 1.0 / (double)a.M, fo);
}

// Finalize and apply in one launch (gm_bn_fwd_finalize_apply_grouped_bf16): grid (nb, C / 64, G).
// Every block of (slice cs, group g) combines the slice's partial rows itself - fin_combine and
// fwd_coef, k_bn_stats_finalize's own code, so all nb blocks hold the same coefficients bit for
// bit - keeps sc / sh in LDS and streams its share of the slice's 128-byte channel band with
// k_bn_apply's per-element arithmetic: 8 threads per pixel, four 16-B loads in flight per
// thread, the block's 128-pixel chunks bx, bx + nb, ...  Only block bx == 0 of a slice stores
// the finalize's side outputs (statistics, running averages, coef_out, the coefficient area), and
// only (bx, cs) == (0, 0) the counter.  No block waits for another: the redundant combine costs
// nb * rows * 512 B of L2 reads per (slice, group), which fold_blocks() bounds.
// RAFF (the residual-affine form, gm_bn_fwd_finalize_apply_res_affine_grouped_bf16): the residual
// is the raw output of a downsample convolution and rb its own BatchNorm (no ReLU), whose apply
// pass is not run: the block combines that BatchNorm's rows too (one launch finalizes both, the
// side outputs of both from block 0) and adds bf16(fmaf(r, sc_r, sh_r)) - the value that
// BatchNorm's apply would have stored, rounded as it stores it - so every output bit is the same.
struct ResBn {
    int nrc;                        // the residual BatchNorm's partial rows per slice
    float momentum, eps;
    float* part;                    // group 0's rows; its coefficient area follows them
    unsigned long long scr_stride;  // bytes between the groups' row + coefficient blocks
    struct Grp {
        const float* gamma;
        const float* beta;
        float* rmean;
        float* rvar;
        float* save_mean;
        float* save_invstd;
        long long* nbt;
        float* coef_out;
    } grp[kMaxBnG];
};

// a (this block's group) with the residual BatchNorm's parameters, statistics and rows
__device__ __forceinline__ ReduceArgs res_bn_args(const ReduceArgs& a, const ResBn& rb) {
    ReduceArgs r = a;
    const ResBn::Grp& q = rb.grp[blockIdx.z];
    r.nrc = rb.nrc; r.momentum = rb.momentum; r.eps = rb.eps;
    r.part = reinterpret_cast<float*>(reinterpret_cast<char*>(rb.part) + blockIdx.z * rb.scr_stride);
    r.coef = r.part + (size_t)rb.nrc * 2 * a.C;
    r.gamma = q.gamma; r.beta = q.beta; r.rmean = q.rmean; r.rvar = q.rvar;
    r.save_mean = q.save_mean; r.save_invstd = q.save_invstd; r.nbt = q.nbt; r.coef_out = q.coef_out;
    return r;
}

// The predicated band loop of the folded kernels: the block's pixels p, p + st, ... of the slice's
// 128-byte band, four pixels' 16-B loads in flight per thread - vector pixel * vpr + lane of A and
// (TWO) of B, 32-bit offsets off a uniform base (the host checks M * C < 2^31) - and f(i, wa, wb)
// per vector.  One loop, the ragged last batch predicated (pixels past M load pixel p's vectors
// again and call nothing); M + 4 st < 2^32: no wrap.  SCHED: one vector's arithmetic at a time.
template <bool TWO, bool SCHED, typename F>
__device__ __forceinline__ void band_loop(const u32x4* A, const u32x4* B, unsigned M, unsigned vpr, F f) {
    constexpr unsigned U = 4;
    const int t = threadIdx.x;
    const unsigned st = gridDim.x * (kFinT / 8);  // pixels per grid pass
    unsigned p = blockIdx.x * (kFinT / 8) + (t >> 3);
    const unsigned lane = t & 7;
    for (; p < M; p += U * st) {
        u32x4 ra[U], rb[U];
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            const unsigned q = p + u * st < M ? p + u * st : p;
            ra[u] = A[q * vpr + lane];
            if (TWO) rb[u] = B[q * vpr + lane];
        }
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            if (TWO) pin(ra[u], rb[u]);
            else pin(ra[u]);
        }
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            if (p + u * st < M) f((p + u * st) * vpr + lane, ra[u], TWO ? rb[u] : ra[u]);
            if (SCHED) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <bool RES, bool RELU, bool RAFF>
__device__ __forceinline__ void finalize_apply_body(const ReduceArgs& a0, const ResBn* rb) {
    const ReduceArgs a = group_args(a0);
    __shared__ double rd[kFinT / 32][128];
    __shared__ float cf[RAFF ? 4 : 2][64];
    const int t = threadIdx.x, cs = blockIdx.y;
    // one BatchNorm's combine and finalize: sc / sh into cf[n], cf[n + 1]; block 0 stores the rest
    auto fin_bn = [&](const ReduceArgs& b, int n) {
        const FinOps fo = fin_load_fwd_all(b, cs);
        double S1, S2;
        fin_combine(b, cs, rd, S1, S2);
        if (t < 64) {
            const FwdCoef k = fwd_coef(b, S1, S2, 1.0 / (double)b.M, fo);
            cf[n][t] = k.sc;
            cf[n + 1][t] = k.sh;
            if (blockIdx.x == 0) {
                fwd_store<false>(b, cs * 64 + t, k);
                count_batch(b, cs * 64 + t);
            }
        }
        __syncthreads();  // (rd is free again: every thread is past this barrier)
    };
    fin_bn(a, 0);
    if (RAFF) fin_bn(res_bn_args(a, *rb), 2);  // the residual's BatchNorm, on its own rows
    const int j8 = (t & 7) * 8;
    float sc[8], sh[8], rsc[8], rsh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sc[j] = cf[0][j8 + j];
        sh[j] = cf[1][j8 + j];
        if constexpr (RAFF) {
            rsc[j] = cf[2][j8 + j];
            rsh[j] = cf[3][j8 + j];
        }
    }
    uint4* YY = a.yout + cs * 8;
    uint8_t* MM = a.mask_out ? a.mask_out + cs * 8 : nullptr;
    band_loop<RES, false>(static_cast<const u32x4*>(a.x) + cs * 8, reinterpret_cast<const u32x4*>(a.res) + cs * 8,
                          (unsigned)a.M, (unsigned)a.C >> 3, [&](unsigned i, u32x4 wx, u32x4 wr) {
                              float f[8], r[8];
                              unpack8(u4(wx), f);
                              if (RES) unpack8(u4(wr), r);
                              if (RAFF) res_affine(r, rsc, rsh);
                              form_y<RES, RELU>(f, r, sc, sh);
                              store_y<RES && RELU>(YY, MM, i, f);
                          });
}

template <bool RES, bool RELU>
__global__ __launch_bounds__(kFinT) void k_bn_finalize_apply(ReduceArgs a0) {
    finalize_apply_body<RES, RELU, false>(a0, nullptr);
}

template <bool RELU>
__global__ __launch_bounds__(kFinT) void k_bn_finalize_apply_raff(ReduceArgs a0, ResBn rb) {
    finalize_apply_body<true, RELU, true>(a0, &rb);
}

// The same fold for the backward from producer statistics (gm_bn_bwd_finalize_apply_grouped_bf16):
// k_bn_bwd_stats_finalize's combine and bwd_coef in every block, then k_bn_apply_bwd<RELU, false,
// MASKX = RELU>'s arithmetic over the block's share of the band.  Block bx == 0 of a slice alone
// writes dgamma / dbeta (accumulate honoured) and the ca / cb / cc coefficient area.
template <bool RELU>
__global__ __launch_bounds__(kFinT) void k_bn_bwd_finalize_apply(ReduceArgs a0, float* coef0, long long cstride) {
    ReduceArgs a = group_args(a0);
    a.coef = coef0 + blockIdx.z * cstride;
    __shared__ double rd[kFinT / 32][128];
    __shared__ float cf[3][64];
    const int t = threadIdx.x, cs = blockIdx.y;
    const FinOps fo = fin_load<BWD>(a, cs * 64 + (t & 63));
    const int j8 = (t & 7) * 8;
    double S1, S2;
    fin_combine(a, cs, rd, S1, S2);
    float fs[8], fh[8];
    if (RELU) {  // the forward's coefficients: in flight over the coefficient arithmetic
        load_coef(a.fcoef, cs * 8 + (t & 7), fs);
        load_coef(a.fcoef + a.C, cs * 8 + (t & 7), fh);
    }
    if (t < 64) {
        const BwdCoef k = bwd_coef<false>(S1, S2, 1.0 / (double)a.M, fo);
        cf[0][t] = k.ca;
        cf[1][t] = k.cb;
        cf[2][t] = k.cc;
        if (blockIdx.x == 0) bwd_store<false, false>(a, cs * 64 + t, k);
    }
    __syncthreads();
    float ca[8], cb[8], cc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        ca[j] = cf[0][j8 + j];
        cb[j] = cf[1][j8 + j];
        cc[j] = cf[2][j8 + j];
    }
    uint4* DX = a.yout + cs * 8;
    // (SCHED: one vector's arithmetic at a time keeps the kernel at 128 VGPRs, no scratch)
    band_loop<true, true>(static_cast<const u32x4*>(a.dy) + cs * 8, static_cast<const u32x4*>(a.x) + cs * 8,
                          (unsigned)a.M, (unsigned)a.C >> 3, [&](unsigned i, u32x4 wd, u32x4 wx) {
                              float d[8], xf[8], o[8];
                              unpack8(u4(wd), d);
                              unpack8(u4(wx), xf);
                              form_dz<RELU ? BWD_RELUX : BWD>(d, xf, nullptr, fs, fh);
                              form_dx(o, d, xf, ca, cb, cc);
                              DX[i] = pack8(o);
                          });
}

// ---------------------------------------------------------------------------------
// Redundant-finalize hand-off of the single-launch kernels for small maps (a.redundant):
// the last-arriving block no longer combines, finalizes, publishes the coefficients and a
// generation word that the other blocks poll and then read the coefficients from - four
// dependent memory round trips after the last partial row lands.  Every block polls the
// slice's ticket counter itself (the partial rows' writers add to it after their sc1
// stores: cdna_hip_programming.md Guideline 16, the sc1 poll row), combines the <= nrc
// partial rows (sc1 loads, fp64, the fixed order of combine_finalize: every block computes
// the same coefficients) and keeps the coefficients in LDS; the block whose ticket came
// last also writes the side outputs (statistics, running averages, counter, coef_out /
// dgamma, dbeta) through fwd_store / bwd_store.  The counter then counts a second round (each block
// once it has seen nrc arrivals), and the block completing that round re-zeroes it, so
// no poller can miss the value nrc and the ticket words are zero between calls again.
__device__ __forceinline__ bool arrive(unsigned* ctr, unsigned n, float* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tk = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = tk == n - 1 ? 1.f : 0.f;
    }
    __syncthreads();
    return *flag != 0.f;
}

__device__ __forceinline__ bool wait_count(unsigned* ctr, unsigned n, unsigned limit, float* flag) {
    if (threadIdx.x == 0) {
        unsigned it = 0;
        bool ok = true;
        while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < n) {
            if (++it >= limit) {
                ok = false;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (!ok) atomicOr(&g_bn_fault, GM_FAULT_BN_SPIN);
        *flag = ok ? 1.f : 0.f;
    }
    __syncthreads();
    return *flag != 0.f;
}

__device__ __forceinline__ void depart(unsigned* ctr, unsigned n) {
    if (threadIdx.x == 0) {
        const unsigned tk = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tk == 2 * n - 1) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the slice's coefficients into cf[3][SW] (LDS): FWD sc, sh; BWD ca, cb, cc (bf16 form) - one
// fwd_coef / bwd_coef per channel, which the last-arriving block also stores (side outputs)
template <int MODE>
__device__ __forceinline__ void combine_coefs(const ReduceArgs& a, int cs, float* red, const FinOps& fo, bool last,
                                              float* cf) {
    const int SW = a.SW;
    combine_rows(a, cs, red, [&](int t, double S1, double S2) {
        const double invM = 1.0 / (double)a.M;
        const int c = cs * SW + t;
        if (MODE == FWD) {
            if (last) count_batch(a, c);  // (its load in flight over the coefficient arithmetic)
            const FwdCoef k = fwd_coef(a, S1, S2, invM, fo);
            if (last) fwd_store<false>(a, c, k);
            cf[t] = k.sc;
            cf[SW + t] = k.sh;
        } else {
            const BwdCoef k = bwd_coef<false>(S1, S2, invM, fo);
            if (last) bwd_store<false, false>(a, c, k);
            cf[t] = k.ca;
            cf[SW + t] = k.cb;
            cf[2 * SW + t] = k.cc;
        }
    });
    __syncthreads();
}

// the slice's generation word before the block's own work (thread 0; the others hold 0)
__device__ __forceinline__ unsigned gen_read(const ReduceArgs& a, int cs) {
    return threadIdx.x == 0 ? __hip_atomic_load(a.gen + cs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
}

// The coefficient hand-off of the single-launch kernels, after the block's partial row is stored:
// the redundant form above (a.redundant), or the slice's last block (ticket) finalizes and
// publishes the coefficients (write-through stores, then the generation word g0 + 1) while the
// others poll that word (bounded) and read them back with sc1 loads.  Fills this thread's N
// coefficient vectors co[N][8] (FWD: sc, sh; BWD: ca, cb, cc) - NaN where the wait timed out:
// never stale coefficients (the fault word is set) - and returns whether they are fresh.
template <int MODE>
__device__ __forceinline__ bool handoff_coefs(const ReduceArgs& a, const Strip& sp, float* red, unsigned g0,
                                              float (*co)[8]) {
    constexpr int N = MODE == FWD ? 2 : 3;
    const int C = a.C, SW = a.SW, cs = sp.cs;
    FinOps fo{};
    if (sp.t < SW) fo = fin_load<MODE>(a, cs * SW + sp.t);
    bool fresh = true;
    if (a.redundant) {
        __shared__ float cf[3 * 64];
        const bool last = arrive(a.counter + cs, (unsigned)a.nrc, &red[kRedF]);
        fresh = wait_count(a.counter + cs, (unsigned)a.nrc, a.spin_limit, &red[kRedF + 1]);
        combine_coefs<MODE>(a, cs, red, fo, last, cf);
        depart(a.counter + cs, (unsigned)a.nrc);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int n = 0; n < N; ++n) co[n][j] = cf[n * SW + sp.cg * 8 + j];
        }
    } else {
        unsigned* gen = a.gen + cs;
        if (ticket(a.counter + cs, (unsigned)a.nrc, &red[kRedF])) {
            combine_finalize<MODE, true>(a, cs, red, fo);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (sp.t == 0) __hip_atomic_store(gen, g0 + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            fresh = wait_generation(gen, g0, a.spin_limit, &red[kRedF + 1]);
        }
        const auto rq = rsrc_of(a.coef);
        float4 lo[N], hi[N];
#pragma unroll
        for (int n = 0; n < N; ++n) {
            lo[n] = ld_sc1_f32x4(rq, (unsigned)(n * C + sp.c0) * 4u);
            hi[n] = ld_sc1_f32x4(rq, (unsigned)(n * C + sp.c0 + 4) * 4u);
        }
#pragma unroll
        for (int n = 0; n < N; ++n) {
            float* o = co[n];
            o[0] = lo[n].x; o[1] = lo[n].y; o[2] = lo[n].z; o[3] = lo[n].w;
            o[4] = hi[n].x; o[5] = hi[n].y; o[6] = hi[n].z; o[7] = hi[n].w;
        }
    }
    if (!fresh) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
#pragma unroll
            for (int j = 0; j < 8; ++j) co[n][j] = __builtin_nanf("");
        }
    }
    return fresh;
}

// The reference-precision (fp32) reduce: the reference's CPU BatchNorm accumulates its
// sums in double (ATen acc_type<float> on the CPU), and long fp32 sums of gradients with
// mixed signs lose the digits the parameter gradients are made of (1e-3 relative at
// 224x224 maps, measured).  So every level accumulates in fp64: per-thread sums, the
// row-group combine, the per-block partials (sc1 stores, 8 B) and the last block's
// combine; the centred backward coefficients (finalize<CENTER>).
template <int MODE>
__global__ __launch_bounds__(kT) void k_bn_reduce_f64(ReduceArgs a0) {
    const ReduceArgs a = group_args(a0);
    __shared__ double red[kRedF];  // rpp * 2 * SW == 4096 doubles
    __shared__ float flag;
    const Strip sp(a);
    const int t = sp.t, C = a.C, SW = a.SW, cs = sp.cs, c0 = sp.c0;
    const float* X = static_cast<const float*>(a.x);
    const float* DY = static_cast<const float*>(a.dy);
    const float* Y = static_cast<const float*>(a.y);
    float fsc[8], fsh[8];
    double mu[8], s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        fsc[j] = MODE == BWD_RELUX ? a.fcoef[c0 + j] : 0.f;
        fsh[j] = MODE == BWD_RELUX ? a.fcoef[C + c0 + j] : 0.f;
        mu[j] = MODE != FWD ? (double)a.save_mean[c0 + j] : 0.0;
        s1[j] = s2[j] = 0.0;
    }
    for (long long r = sp.rbeg + sp.r0; r < sp.rend; r += sp.rpp) {
        const long long e = r * C + c0;
        float xf[8], d[8], yf[8];
        V8<float>::ld(X + e, 0, xf);
        if (MODE != FWD) V8<float>::ld(DY + e, 0, d);
        if (MODE == BWD_RELU) V8<float>::ld(Y + e, 0, yf);
        if (MODE != FWD) form_dz<MODE>(d, xf, yf, fsc, fsh);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (MODE == FWD) {
                s1[j] += (double)xf[j];
                s2[j] = fma((double)xf[j], (double)xf[j], s2[j]);
            } else {
                s1[j] += (double)d[j];
                s2[j] = fma((double)d[j], (double)xf[j] - mu[j], s2[j]);
            }
        }
    }
    store_partial_row(a, sp, red, s1, s2);
    const int S2w = 2 * SW;
    FinOps fo{};
    if (t < SW) fo = fin_load<MODE>(a, cs * SW + t);
    if (!ticket(a.counter + cs, (unsigned)a.nrc, &flag)) return;
    if (MODE == FWD) count_batch(a, cs * SW + t);
    const double* pp = reinterpret_cast<const double*>(a.part) + (size_t)cs * a.nrc * S2w;
    if (t < S2w) {  // fixed order over the row chunks
        double acc = 0.0;
        for (int i = 0; i < a.nrc; ++i)
            acc += __hip_atomic_load(pp + (size_t)i * S2w + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        red[t] = acc;
    }
    __syncthreads();
    if (t < SW) finalize<MODE, false, true>(a, cs * SW + t, red[2 * t], red[2 * t + 1], 1.0 / (double)a.M, fo);
}

// Fused forward for maps whose grid is co-resident (fused_plan) and whose rows
// fit NR 16-B vectors per thread: the block keeps its x strip in registers, takes
// its ticket, the slice's last block finalizes and publishes the coefficients
// (write-through stores, then a generation word), the other blocks spin on the
// generation word (bounded) and every block applies y = relu?(x*sc + sh (+res)) from
// its registers.  One launch and one read of x instead of two launches and two reads.

template <bool RES, bool RELU, int NR>
__global__ __launch_bounds__(kT, NR == 16 ? 2 : NR == 8 ? 3 : 4) void k_bn_fwd_fused(ReduceArgs a0) {  // NR 0: streaming
    const ReduceArgs a = group_args(a0);
    __shared__ float red[kRedF + 4];
    const Strip sp(a);
    const int r0 = sp.r0, rpp = sp.rpp;
    const long long vpr = sp.vpr, cv = sp.cv, rbeg = sp.rbeg, rend = sp.rend;
    const unsigned g0 = gen_read(a, sp.cs);
    const uint4* X = static_cast<const uint4*>(a.x);

    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    constexpr int NV = NR > 0 ? NR : 1;
    uint4 v[NV];
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
    if (NR > 0) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {  // clamped loads (always valid), then a value select
            const long long r = rbeg + r0 + (long long)u * rpp;
            const uint4 w = X[(r < rend ? r : rend - 1) * vpr + cv];
            v[u] = r < rend ? w : z;
        }
#pragma unroll
        for (int u = 0; u < NV; ++u) accum_vals<FWD>(v[u], z, z, nullptr, s1, s2);
    } else {  // streaming: 8 rows in flight per thread, x re-read (L2 / MALL) by the apply
        // (this loop and the apply's stay written out, as k_bn_bwd_fused's: behind one walker
        // taking the per-vector action the streaming forms ran 1.5 % slower)
        long long r = rbeg + r0;
        const long long st = (long long)rpp * vpr;
        for (; r + 7 * rpp < rend; r += 8 * rpp) {
            uint4 w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) w[u] = X[r * vpr + cv + u * st];
#pragma unroll
            for (int u = 0; u < 8; ++u) accum_vals<FWD>(w[u], z, z, nullptr, s1, s2);
        }
        for (; r < rend; r += rpp) accum_vals<FWD>(X[r * vpr + cv], z, z, nullptr, s1, s2);
    }

    store_partial_row(a, sp, red, s1, s2);
    float co[2][8];
    const bool fresh = handoff_coefs<FWD>(a, sp, red, g0, co);
    auto apply = [&](uint4 xv, long long i) {
        float f[8], q[8];
        unpack8(xv, f);
        if (RES) unpack8(a.res[i], q);
        // (form_y's loop written out: the poison select belongs inside it - after it, the compiler
        // drops the coefficients' own poison and waits for them inside every output block)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float zz = fmaf(f[j], co[0][j], co[1][j]);
            if (RES) zz += q[j];
            f[j] = RELU ? relu_nan(zz) : zz;
            if (!fresh) f[j] = __builtin_nanf("");  // poisoned (fmaxf would turn NaN into 0)
        }
        store_y<RES && RELU>(a.yout, a.mask_out, i, f);
    };
    if (NR > 0) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const long long r = rbeg + r0 + (long long)u * rpp;
            if (r < rend) apply(v[u], r * vpr + cv);
        }
    } else {
        long long r = rbeg + r0;
        const long long st = (long long)rpp * vpr;
        for (; r + 3 * rpp < rend; r += 4 * rpp) {
            uint4 w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = X[r * vpr + cv + u * st];
#pragma unroll
            for (int u = 0; u < 4; ++u) apply(w[u], r * vpr + cv + u * st);
        }
        for (; r < rend; r += rpp) apply(X[r * vpr + cv], r * vpr + cv);
    }
}

// y for the ReLU mask, or (YM) the forward's mask byte expanded to 1.0 / 0 bf16 values
template <bool YM>
__device__ __forceinline__ uint4 ld_ymask(const ReduceArgs& a, long long i) {
    return YM ? mask_vals(a.ymask[i]) : static_cast<const uint4*>(a.y)[i];
}

// Fused backward, same scheme as k_bn_fwd_fused: the block holds its x / dy (/ y)
// strip in registers (NR 4 or 8) or re-reads it (NR 0), the slice's last block
// publishes (a, b, c) and every block writes dx = a*dz + b*x + c (and dres = dz).
template <int MODE, bool DRES, int NR, bool YM = false>
__global__ __launch_bounds__(kT, NR == 8 ? 2 : 3) void k_bn_bwd_fused(ReduceArgs a0) {
    const ReduceArgs a = group_args(a0);
    __shared__ float red[kRedF + 4];
    const Strip sp(a);
    const int C = a.C, r0 = sp.r0, rpp = sp.rpp, c0 = sp.c0;
    const long long vpr = sp.vpr, cv = sp.cv, rbeg = sp.rbeg, rend = sp.rend;
    const unsigned g0 = gen_read(a, sp.cs);
    const uint4* X = static_cast<const uint4*>(a.x);
    const uint4* DY = static_cast<const uint4*>(a.dy);
    const uint4* Y = static_cast<const uint4*>(a.y);
    // streaming rows in flight (register budget: y's vectors; the mask bytes (YM) cost one each)
    constexpr int US = MODE == BWD_RELU && !YM ? 2 : 4;
    float mu[8], fsc[8], fsh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mu[j] = a.save_mean[c0 + j];
        if (MODE == BWD_RELUX) {
            fsc[j] = a.fcoef[c0 + j];
            fsh[j] = a.fcoef[C + c0 + j];
        }
    }
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    constexpr int NV = NR > 0 ? NR : 1;
    constexpr int NY = MODE == BWD_RELU ? NV : 1;
    uint4 vx[NV], vd[NV], vy[NY];
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
    if (NR > 0) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {  // clamped loads, then value selects (zero rows add nothing)
            const long long r = rbeg + r0 + (long long)u * rpp;
            const long long i = (r < rend ? r : rend - 1) * vpr + cv;
            const uint4 wx = X[i], wd = DY[i];
            vx[u] = r < rend ? wx : z;
            vd[u] = r < rend ? wd : z;
            if (MODE == BWD_RELU) vy[u] = ld_ymask<YM>(a, i);
        }
#pragma unroll
        for (int u = 0; u < NV; ++u)
            accum_vals<MODE>(vx[u], vd[u], MODE == BWD_RELU ? vy[u < NY ? u : 0] : z, mu, s1, s2, fsc, fsh);
    } else {
        // streaming: US rows' loads in flight, every load of a batch issued before the first use
        // (pin).  This loop and its twin in the output pass stay written out: behind one walker
        // taking the per-vector action, three forms' register allocation lost a wave per SIMD.
        long long r = rbeg + r0;
        const long long st = (long long)rpp * vpr;
        for (; r + (US - 1) * rpp < rend; r += US * rpp) {
            uint4 wx[US], wd[US], wy[US];
            unsigned wm[US];
#pragma unroll
            for (int u = 0; u < US; ++u) {
                const long long i = r * vpr + cv + u * st;
                wx[u] = X[i];
                wd[u] = DY[i];
                if (MODE == BWD_RELU && YM) wm[u] = a.ymask[i];
                else if (MODE == BWD_RELU) wy[u] = Y[i];
            }
#pragma unroll
            for (int u = 0; u < US; ++u) {
                pin(wx[u]);
                pin(wd[u]);
                if (MODE == BWD_RELU && YM) pin(wm[u]);
                else if (MODE == BWD_RELU) pin(wy[u]);
            }
#pragma unroll
            for (int u = 0; u < US; ++u)
                accum_vals<MODE>(wx[u], wd[u], MODE == BWD_RELU ? (YM ? mask_vals(wm[u]) : wy[u]) : z, mu, s1, s2, fsc, fsh);
        }
        for (; r < rend; r += rpp) {
            const long long i = r * vpr + cv;
            accum_vals<MODE>(X[i], DY[i], MODE == BWD_RELU ? ld_ymask<YM>(a, i) : z, mu, s1, s2, fsc, fsh);
        }
    }

    store_partial_row(a, sp, red, s1, s2);
    float co[3][8];
    handoff_coefs<MODE>(a, sp, red, g0, co);
    auto out = [&](uint4 ux, uint4 ud, uint4 uy, long long i) {
        float d[8], xf[8], yf[8], o[8];
        unpack8(ud, d);
        unpack8(ux, xf);
        if (MODE == BWD_RELU) unpack8(uy, yf);
        form_dz<MODE>(d, xf, yf, fsc, fsh);
        if (DRES) a.dres_out[i] = pack8(d);
        form_dx(o, d, xf, co[0], co[1], co[2]);
        a.yout[i] = pack8(o);
    };
    if (NR > 0) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const long long r = rbeg + r0 + (long long)u * rpp;
            if (r < rend) out(vx[u], vd[u], MODE == BWD_RELU ? vy[u < NY ? u : 0] : z, r * vpr + cv);
        }
    } else {
        long long r = rbeg + r0;
        const long long st = (long long)rpp * vpr;
        for (; r + (US - 1) * rpp < rend; r += US * rpp) {
            uint4 wx[US], wd[US], wy[US];
            unsigned wm[US];
#pragma unroll
            for (int u = 0; u < US; ++u) {
                const long long i = r * vpr + cv + u * st;
                wx[u] = X[i];
                wd[u] = DY[i];
                if (MODE == BWD_RELU && YM) wm[u] = a.ymask[i];
                else if (MODE == BWD_RELU) wy[u] = Y[i];
            }
#pragma unroll
            for (int u = 0; u < US; ++u) {
                pin(wx[u]);
                pin(wd[u]);
                if (MODE == BWD_RELU && YM) pin(wm[u]);
                else if (MODE == BWD_RELU) pin(wy[u]);
            }
#pragma unroll
            for (int u = 0; u < US; ++u)
                out(wx[u], wd[u], MODE == BWD_RELU ? (YM ? mask_vals(wm[u]) : wy[u]) : z, r * vpr + cv + u * st);
        }
        for (; r < rend; r += rpp) {
            const long long i = r * vpr + cv;
            out(X[i], DY[i], MODE == BWD_RELU ? ld_ymask<YM>(a, i) : z, i);
        }
    }
}

struct ApplyArgs {
    long long nvec;      // M * C / 8
    int tpr_log;
    int relu;
    const void* x;       // E elements
    const void* res;     // fwd residual / bwd: y (relu mask)
    const void* dy;      // bwd
    void* out;           // fwd y / bwd dx
    void* out2;          // bwd dres
    const float* coef;   // [4][C]
    int C;
    const float* fcoef;  // bwd MASKX: the forward's sc[C], sh[C]
    long long gvec;      // view groups (gridDim.y): group g's x / res / dy / out / out2 gvec
    long long cgs;       // vectors and its coefficients cgs floats after group 0's
    long long fcgs;      // bwd MASKX: group g's fcoef fcgs floats after group 0's
    uint8_t* mask_out;   // fwd (relu + residual), optional: the ReLU mask bytes (as gvec)
    const float* rcoef;  // fwd RAFF: the residual BatchNorm's sc[C], sh[C]
    long long rcgs;      // and group g's rcgs floats after group 0's
};

__device__ __forceinline__ void load_coef(const float* p, int cg, float* c) {
    const float4 a = reinterpret_cast<const float4*>(p)[cg * 2];
    const float4 b = reinterpret_cast<const float4*>(p)[cg * 2 + 1];
    c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w; c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
}

template <bool RES, bool RELU, typename E, bool RAFF = false>
__global__ __launch_bounds__(kT) void k_bn_apply(ApplyArgs a) {
    const long long stride = (long long)gridDim.x * kT;  // multiple of C/8
    long long v = (long long)blockIdx.x * kT + threadIdx.x;
    const int cg = (int)(v & ((1 << a.tpr_log) - 1));
    const long long go = blockIdx.y * a.gvec;  // view group blockIdx.y
    const float* coef = a.coef + blockIdx.y * a.cgs;
    float sc[8], sh[8];
    load_coef(coef, cg, sc);
    load_coef(coef + a.C, cg, sh);
    float rsc[8], rsh[8];
    if (RAFF) {  // the residual's own BatchNorm coefficients (res_affine)
        load_coef(a.rcoef + blockIdx.y * a.rcgs, cg, rsc);
        load_coef(a.rcoef + blockIdx.y * a.rcgs + a.C, cg, rsh);
    }
    auto fin = [&](long long i, float* f, float* r) {
        if (RAFF) res_affine(r, rsc, rsh);
        form_y<RES, RELU>(f, r, sc, sh);
        if constexpr (std::is_same<E, uint16_t>::value) store_y<RES && RELU>(static_cast<uint4*>(a.out), a.mask_out, i, f);
        else V8<E>::st(a.out, i, f);
    };
    auto one = [&](long long i) {
        i += go;
        float f[8];
        V8<E>::ld(a.x, i, f);
        float r[8];
        if (RES) V8<E>::ld(a.res, i, r);
        fin(i, f, r);
    };
    if constexpr (std::is_same<E, uint16_t>::value) {
        // four vectors' 16-B loads issued before the first use (as k_bn_apply_bwd)
        constexpr int U = 4;
        const u32x4* XX = static_cast<const u32x4*>(a.x) + go;
        const u32x4* RR = static_cast<const u32x4*>(a.res) + go;
        for (; v + (U - 1) * stride < a.nvec; v += U * stride) {
            u32x4 rx[U], rr[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                rx[u] = XX[v + u * stride];
                if (RES) rr[u] = RR[v + u * stride];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                pin(rx[u]);
                if (RES) pin(rr[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float f[8], r[8];
                unpack8(u4(rx[u]), f);
                if (RES) unpack8(u4(rr[u]), r);
                fin(go + v + u * stride, f, r);
            }
        }
        for (; v < a.nvec; v += stride) one(v);
        return;
    }
    for (; v + stride < a.nvec; v += 2 * stride) {
        one(v);
        one(v + stride);
    }
    if (v < a.nvec) one(v);
}

template <bool RELU, bool DRES, bool MASKX, typename E>
__global__ __launch_bounds__(kT) void k_bn_apply_bwd(ApplyArgs a) {
    constexpr bool CENTER = std::is_same<E, float>::value;  // finalize<CENTER>: slot 3 = mean
    const long long stride = (long long)gridDim.x * kT;
    long long v = (long long)blockIdx.x * kT + threadIdx.x;
    const int cg = (int)(v & ((1 << a.tpr_log) - 1));
    const long long go = blockIdx.y * a.gvec;  // view group blockIdx.y
    const float* coef = a.coef + blockIdx.y * a.cgs;
    float ca[8], cb[8], cc[8], fs[8], fh[8], mu[8];
    load_coef(coef, cg, ca);
    load_coef(coef + a.C, cg, cb);
    load_coef(coef + 2 * a.C, cg, cc);
    if (CENTER) load_coef(coef + 3 * a.C, cg, mu);
    if (MASKX) {
        load_coef(a.fcoef + blockIdx.y * a.fcgs, cg, fs);
        load_coef(a.fcoef + blockIdx.y * a.fcgs + a.C, cg, fh);
    }
    constexpr bool YR = RELU && !MASKX;  // the mask read from y
    auto ld = [&](long long i, float* d, float* xf, float* yf) {
        V8<E>::ld(a.dy, go + i, d);
        V8<E>::ld(a.x, go + i, xf);
        if (YR) V8<E>::ld(a.res, go + i, yf);
    };
    constexpr int MODE = !RELU ? BWD : MASKX ? BWD_RELUX : BWD_RELU;
    auto out = [&](long long i, float* d, const float* xf, const float* yf) {
        form_dz<MODE>(d, xf, yf, fs, fh);
        if (DRES) V8<E>::st(a.out2, go + i, d);
        float o[8];
        form_dx<CENTER>(o, d, xf, ca, cb, cc, mu);
        V8<E>::st(a.out, go + i, o);
    };
    // U vectors' loads issued before the first store (the pointers may alias as far as the
    // compiler knows: one vector at a time serialised load -> wait -> store, 32 B in flight)
    constexpr int U = 4;
    if constexpr (std::is_same<E, uint16_t>::value) {  // raw 16-B loads first, unpacked after
        const u32x4* DY = static_cast<const u32x4*>(a.dy) + go;
        const u32x4* XX = static_cast<const u32x4*>(a.x) + go;
        const u32x4* YY = static_cast<const u32x4*>(a.res) + go;
        for (; v + (U - 1) * stride < a.nvec; v += U * stride) {
            u32x4 rd[U], rx[U], ry[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                rd[u] = DY[v + u * stride];
                rx[u] = XX[v + u * stride];
                if (YR) ry[u] = YY[v + u * stride];
            }
            // every load issued before the first use (the compiler otherwise sinks each load to
            // its use: one vector's 32 B in flight per thread)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                pin(rd[u], rx[u]);
                if (YR) pin(ry[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float d[8], xf[8], yf[8];
                unpack8(u4(rd[u]), d);
                unpack8(u4(rx[u]), xf);
                if (YR) unpack8(u4(ry[u]), yf);
                out(v + u * stride, d, xf, yf);
            }
        }
    } else {
        for (; v + (U - 1) * stride < a.nvec; v += U * stride) {
            float d[U][8], xf[U][8], yf[U][YR ? 8 : 1];
#pragma unroll
            for (int u = 0; u < U; ++u) ld(v + u * stride, d[u], xf[u], yf[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) out(v + u * stride, d[u], xf[u], yf[u]);
        }
    }
    for (; v < a.nvec; v += stride) {
        float d[8], xf[8], yf[YR ? 8 : 1];
        ld(v, d, xf, yf);
        out(v, d, xf, yf);
    }
}

// the inference coefficients of channel c = blockIdx.x * blockDim.x + threadIdx.x (fp64 from the
// running statistics, one rounding each): both kernels below, so the two agree bit for bit
__device__ __forceinline__ void infer_coef(int C, const float* gamma, const float* beta, const float* rm,
                                           const float* rv, float eps, float* coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double is = 1.0 / sqrt((double)rv[c] + (double)eps);
    const double sc = (double)gamma[c] * is;
    coef[c] = (float)sc;
    coef[C + c] = (float)((double)beta[c] - (double)rm[c] * sc);
}

__global__ void k_bn_infer_coef(int C, const float* gamma, const float* beta, const float* rm, const float* rv,
                                float eps, float* coef) {
    infer_coef(C, gamma, beta, rm, rv, eps, coef);
}

// The same coefficients for a table of BatchNorms in one launch (gm_bn_infer_coef): entry blockIdx.y
__global__ void k_bn_infer_coef_table(const gm_bn_coef_entry* tab) {
    const gm_bn_coef_entry e = tab[blockIdx.y];
    infer_coef(e.C, e.gamma, e.beta, e.running_mean, e.running_var, e.eps, e.coef);
}

inline int apply_grid(long long nvec) {
    // ~4 vectors per thread, grid a multiple of nothing in particular: kT is a
    // multiple of C/8 so the channel group of a thread is fixed
    long long g = (nvec + kT * 4 - 1) / (kT * 4);
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return (int)g;
}

// the fields every apply launch shares; the caller adds its tensors and coefficient areas
inline ApplyArgs apply_args(long long M, int C, int relu) {
    ApplyArgs b{};
    b.nvec = M * (C / 8);
    b.tpr_log = ilog2(C / 8);
    b.C = C;
    b.relu = relu;
    return b;
}

// the template switches of the two apply kernels (raff: the residual-affine form, bf16 only)
template <typename E>
void launch_apply(bool res, bool relu, bool raff, dim3 g, hipStream_t st, const ApplyArgs& b) {
    if constexpr (std::is_same<E, uint16_t>::value) {
        if (raff) {
            if (relu) hipLaunchKernelGGL((k_bn_apply<true, true, E, true>), g, dim3(kT), 0, st, b);
            else hipLaunchKernelGGL((k_bn_apply<true, false, E, true>), g, dim3(kT), 0, st, b);
            return;
        }
    }
    if (res) {
        if (relu) hipLaunchKernelGGL((k_bn_apply<true, true, E>), g, dim3(kT), 0, st, b);
        else hipLaunchKernelGGL((k_bn_apply<true, false, E>), g, dim3(kT), 0, st, b);
    } else {
        if (relu) hipLaunchKernelGGL((k_bn_apply<false, true, E>), g, dim3(kT), 0, st, b);
        else hipLaunchKernelGGL((k_bn_apply<false, false, E>), g, dim3(kT), 0, st, b);
    }
}

template <typename E>
void launch_apply_bwd(bool relu, bool dres, bool maskx, dim3 g, hipStream_t st, const ApplyArgs& b) {
    if (maskx) {
        hipLaunchKernelGGL((k_bn_apply_bwd<true, false, true, E>), g, dim3(kT), 0, st, b);
    } else if (relu) {
        if (dres) hipLaunchKernelGGL((k_bn_apply_bwd<true, true, false, E>), g, dim3(kT), 0, st, b);
        else hipLaunchKernelGGL((k_bn_apply_bwd<true, false, false, E>), g, dim3(kT), 0, st, b);
    } else {
        if (dres) hipLaunchKernelGGL((k_bn_apply_bwd<false, true, false, E>), g, dim3(kT), 0, st, b);
        else hipLaunchKernelGGL((k_bn_apply_bwd<false, false, false, E>), g, dim3(kT), 0, st, b);
    }
}

constexpr int kGenOff = 32;  // generation words: header words [32, 32 + nslice) (nslice <= 32)

// Plan of the fused forward: rows per thread NR in {4, 8, 16} (the register-held
// strip) and a grid that stays co-resident even when `concurrency` such launches run
// at once on different streams (the view trunks): grid <= CUs * occupancy / concurrency,
// the occupancy MEASURED for the kernel instantiations that can be launched
// (hipOccupancyMaxActiveBlocksPerMultiprocessor, the minimum over their variants) and
// the concurrency set by the caller (gm_bn_set_concurrency: the number of trunk streams
// that run concurrently plus headroom; default 4).  A grid
// that could exceed the resident capacity would let spinning blocks wait on blocks that
// cannot be scheduled (the spin is bounded and then faults loudly, see wait_generation).
// Returns NR (pl rewritten), -1 for the streaming variant (x re-read by the apply phase;
// gm_bn_set_fused_mode(1) disables it) or 0: use the two-kernel path (gm_bn_set_fused_mode(0)).
int g_concurrency = 4;  // gm_bn_set_concurrency (>= 1: never a division by zero)
int g_fused_env = 2;    // gm_bn_set_fused_mode: 0 = two-kernel path, 1 = no streaming variant

template <typename K>
int occ_min(std::initializer_list<K> ks) {
    int best = 1 << 30;
    for (K k : ks) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(k), kT, 0) != hipSuccess)
            n = 0;
        best = n < best ? n : best;
    }
    return best == (1 << 30) ? 0 : best;
}

struct Occ {
    int fwd[4];  // NR 4, 8, 16, streaming
    int bwd[3];  // NR 4, 8, streaming
};

const Occ& occupancy() {
    static const Occ o = [] {
        Occ r{};
#define GM_F(NR) occ_min({k_bn_fwd_fused<true, true, NR>, k_bn_fwd_fused<true, false, NR>, \
                          k_bn_fwd_fused<false, true, NR>, k_bn_fwd_fused<false, false, NR>})
#define GM_B(NR) occ_min({k_bn_bwd_fused<BWD_RELUX, false, NR>, k_bn_bwd_fused<BWD_RELU, true, NR>, \
                          k_bn_bwd_fused<BWD_RELU, false, NR>, k_bn_bwd_fused<BWD, false, NR>,       \
                          k_bn_bwd_fused<BWD_RELU, true, NR, true>, k_bn_bwd_fused<BWD_RELU, false, NR, true>})
        r.fwd[0] = GM_F(4); r.fwd[1] = GM_F(8); r.fwd[2] = GM_F(16); r.fwd[3] = GM_F(0);
        r.bwd[0] = GM_B(4); r.bwd[1] = GM_B(8); r.bwd[2] = GM_B(0);
#undef GM_F
#undef GM_B
        return r;
    }();
    return o;
}

int device_cus() {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                     hipSuccess)
            return 0;
        return n;
    }();
    return cus;
}

// the redundant-finalize hand-off (every block combines the partial rows): small maps only,
// where a block's extra partial-row reads are a few KB
constexpr int kRedundantMax = 16;  // measured: 8 / 16 help layer 4 (~1-1.3 us a launch), 32+ slow layer 3
inline int redundant_ok(int nrc) { return nrc <= kRedundantMax ? 1 : 0; }

inline int fused_plan(long long M, int C, Plan& pl, bool bwd = false, int G = 1) {
    if (g_fused_env == 0) return 0;
    // co-residency under the device residency plan (gm_set_residency): CUs held by
    // never-yielding kernels (RCCL) are not counted, and every process sharing the GPU
    // may run its own launches at once
    const Residency& rs = residency();
    const int cus = usable_cus(device_cus());
    // a grouped launch (G views in one grid) holds G plans' worth of workgroups at once
    const int conc = (g_concurrency > rs.streams ? g_concurrency : rs.streams) * rs.sharers * G;
    const Plan base = make_plan(M, C);
    const Occ& oc = occupancy();
    const int nrs[3] = {4, 8, 16};
    const int occ_reg[3] = {bwd ? oc.bwd[0] : oc.fwd[0], bwd ? oc.bwd[1] : oc.fwd[1], bwd ? 0 : oc.fwd[2]};
    // the co-resident grid of a kernel with occupancy occ: pl, if it fits the base plan's partials
    // area and (max_nr > 0) a thread's rows fit max_nr registers-held vectors
    auto fit = [&](int occ, int max_nr) {
        const long long want = (long long)cus * occ / conc / base.nslice;
        if (want < 1) return false;
        long long rpb = (M + want - 1) / want;
        rpb = (rpb + base.rpp - 1) / base.rpp * base.rpp;
        if (max_nr > 0 && rpb / base.rpp > max_nr) return false;
        const long long nrc = (M + rpb - 1) / rpb;
        if (nrc > base.nrc) return false;  // partials area sized by the base plan
        pl = base;
        pl.rpb = rpb;
        pl.nrc = (int)nrc;
        return true;
    };
    for (int i = 0; i < 3; ++i)
        if (fit(occ_reg[i], nrs[i])) return nrs[i];
    if (g_fused_env >= 2 && fit(bwd ? oc.bwd[2] : oc.fwd[3], 0)) return -1;  // streaming variant: any map size
    return 0;
}

// the two shape rules: a training / planning call's map, and a producer statistics buffer's
// (whole 64-channel slices of partial rows)
inline bool shape_ok(long long M, int C) { return M > 0 && C >= 8 && C <= kMaxC && (C & (C - 1)) == 0; }
inline bool stats_shape_ok(const float* stats, int rows, int C) {
    return stats && rows >= 1 && C >= 64 && C % 64 == 0;
}

int check_common(long long M, int C, const void* scratch, size_t bytes, const char* fn) {
    if (!shape_ok(M, C)) {
        set_error("%s: need M > 0 and C a power of two in [8, %d] (M=%lld C=%d)", fn, kMaxC, M, C);
        return GM_E_ARG;
    }
    if (!scratch || bytes < scratch_bytes(M, C)) {
        set_error("%s: scratch %zu bytes < required %zu", fn, bytes, scratch_bytes(M, C));
        return GM_E_SCRATCH;
    }
    return GM_OK;
}

}  // namespace
}  // namespace gm

using namespace gm;

extern "C" size_t gm_bn_scratch(long long M, int C) {
    if (M <= 0 || C < 8 || C > kMaxC) return 0;
    return scratch_bytes(M, C);
}

namespace {

// Grouped scratch layout (the gm_bn_*_grouped_bf16 calls; never mixed with ungrouped calls
// on one buffer): kMaxBnG fixed 256-byte headers (each group's tickets and generation
// words: they stay at the same place whatever the shape, so a ticket word is only ever
// a ticket word and stays zero between calls), then per group its coefficients and
// partials (no zero invariant) at a shape-dependent stride.
constexpr size_t kGrpHdr = kMaxBnG * kHdr;
inline size_t group_stride(long long M, int C) {
    const Plan p = make_plan(M, C);
    return (p.bytes - p.off_coef + 255) / 256 * 256;
}
inline size_t grouped_bytes(long long M, int C, int G) { return kGrpHdr + G * group_stride(M, C); }

// the scratch pointers of a call: ungrouped layout (header, coefficients, partials) or
// the grouped one above
void set_scratch(ReduceArgs& a, const Plan& pl, char* s, bool grouped) {
    a.counter = reinterpret_cast<unsigned*>(s);
    if (grouped) {
        a.coef = reinterpret_cast<float*>(s + kGrpHdr);
        a.part = reinterpret_cast<float*>(s + kGrpHdr + (pl.off_p1 - pl.off_coef));
        a.scr_stride = group_stride(a.M, a.C);
        a.hdr_words = kHdr / sizeof(unsigned);
    } else {
        a.coef = reinterpret_cast<float*>(s + pl.off_coef);
        a.part = reinterpret_cast<float*>(s + pl.off_p1);
        a.scr_stride = 0;
        a.hdr_words = 0;
    }
}

// the G descriptors of a grouped call must agree on everything but their pointers
int check_groups_fwd(const gm_bn_fwd* ps, int G, const char* fn) {
    GM_REQUIRE(ps && G >= 1 && G <= kMaxBnG, "%s: 1..%d groups (got %d)", fn, kMaxBnG, G);
    for (int g = 0; g < G; ++g) {
        const gm_bn_fwd& p = ps[g], &q = ps[0];
        GM_REQUIRE(p.x && p.gamma && p.beta && p.save_mean && p.save_invstd, "%s: null argument (group %d)", fn, g);
        GM_REQUIRE(!p.running_mean == !p.running_var, "%s: running_mean/var both or neither", fn);
        GM_REQUIRE(p.M == q.M && p.C == q.C && p.relu == q.relu && !p.residual == !q.residual &&
                       !p.running_mean == !q.running_mean && !p.num_batches_tracked == !q.num_batches_tracked &&
                       !p.coef_out == !q.coef_out && !p.y == !q.y && p.momentum == q.momentum && p.eps == q.eps,
                   "%s: group %d differs from group 0 in shape or options", fn, g);
    }
    return GM_OK;
}

int check_groups_bwd(const gm_bn_bwd* ps, int G, const char* fn) {
    GM_REQUIRE(ps && G >= 1 && G <= kMaxBnG, "%s: 1..%d groups (got %d)", fn, kMaxBnG, G);
    for (int g = 0; g < G; ++g) {
        const gm_bn_bwd& p = ps[g], &q = ps[0];
        GM_REQUIRE(p.dy && p.x && p.gamma && p.save_mean && p.save_invstd && p.dx && p.dgamma && p.dbeta,
                   "%s: null argument (group %d)", fn, g);
        GM_REQUIRE(!p.relu || p.y || (p.fwd_coef && !p.dres),
                   "%s: relu needs the forward output y (or fwd_coef, without a residual)", fn);
        GM_REQUIRE(p.M == q.M && p.C == q.C && p.relu == q.relu && !p.y == !q.y && !p.dres == !q.dres &&
                       !p.fwd_coef == !q.fwd_coef && p.accumulate == q.accumulate,
                   "%s: group %d differs from group 0 in shape or options", fn, g);
    }
    return GM_OK;
}

int check_scratch(long long M, int C, int G, bool grouped, const void* scratch, size_t bytes, const char* fn) {
    int rc = check_common(M, C, scratch, bytes, fn);
    if (rc) return rc;
    const size_t need = grouped ? grouped_bytes(M, C, G) : scratch_bytes(M, C);
    if (bytes < need) {
        set_error("%s: scratch %zu bytes < required %zu for %d groups", fn, bytes, need, G);
        return GM_E_SCRATCH;
    }
    return GM_OK;
}

// the per-group pointers of a forward / backward call into grp[] (kernels read grp[] only)
void fwd_groups(ReduceArgs& a, const gm_bn_fwd* ps, int G) {
    for (int g = 0; g < G; ++g) {
        BnGroup& q = a.grp[g];
        q.x = ps[g].x;
        q.gamma = ps[g].gamma; q.beta = ps[g].beta;
        q.rmean = ps[g].running_mean; q.rvar = ps[g].running_var;
        q.save_mean = ps[g].save_mean; q.save_invstd = ps[g].save_invstd;
        q.nbt = ps[g].num_batches_tracked;
        q.coef_out = ps[g].coef_out;
        q.res = static_cast<const uint4*>(ps[g].residual);
        q.yout = static_cast<uint4*>(ps[g].y);
        q.mask_out = static_cast<uint8_t*>(ps[g].relu_mask);
    }
}

void bwd_groups(ReduceArgs& a, const gm_bn_bwd* ps, int G) {
    for (int g = 0; g < G; ++g) {
        BnGroup& q = a.grp[g];
        q.x = ps[g].x; q.dy = ps[g].dy; q.y = ps[g].y;
        q.gamma = ps[g].gamma;
        q.save_mean = const_cast<float*>(ps[g].save_mean);
        q.save_invstd = const_cast<float*>(ps[g].save_invstd);
        q.dgamma = ps[g].dgamma; q.dbeta = ps[g].dbeta;
        q.fcoef = ps[g].fwd_coef;
        q.yout = static_cast<uint4*>(ps[g].dx);
        q.dres_out = static_cast<uint4*>(ps[g].dres);
        q.ymask = static_cast<const uint8_t*>(ps[g].relu_mask);
    }
}

// shared fields from group 0, per-group pointers into grp[], scratch split per group
void fill_fwd(ReduceArgs& a, const gm_bn_fwd* ps, int G, bool grouped, const Plan& pl, char* s) {
    const gm_bn_fwd* p = ps;
    a.M = p->M; a.C = p->C; a.tpr_log = pl.tpr_log; a.rpb = pl.rpb;
    a.SW = pl.SW; a.nrc = pl.nrc;
    a.momentum = p->momentum; a.eps = p->eps;
    set_scratch(a, pl, s, grouped);
    fwd_groups(a, ps, G);
}

// the single-launch form's plan into a (fused_plan chose it): its grid
dim3 fused_args(ReduceArgs& a, const Plan& fp, char* s, int G) {
    a.rpb = fp.rpb;
    a.nrc = fp.nrc;
    a.gen = reinterpret_cast<unsigned*>(s) + kGenOff;
    a.spin_limit = spin_limit();
    a.redundant = redundant_ok(a.nrc);
    return dim3(fp.nrc, fp.nslice, G);
}

template <typename E>
int bn_fwd_train(const gm_bn_fwd* ps, int G, bool grouped, void* scratch, size_t bytes, void* stream,
                 const char* fn) {
    int rc = check_groups_fwd(ps, G, fn);
    if (rc) return rc;
    const gm_bn_fwd* p = ps;
    GM_REQUIRE(p->y, "%s: null argument (y)", fn);
    if ((rc = check_scratch(p->M, p->C, G, grouped, scratch, bytes, fn))) return rc;
    const Plan pl = make_plan(p->M, p->C);
    char* s = static_cast<char*>(scratch);
    ReduceArgs a{};
    fill_fwd(a, ps, G, grouped, pl, s);
    hipStream_t st = as_stream(stream);
    const dim3 rg(pl.nrc, pl.nslice, G);
    if constexpr (std::is_same<E, float>::value) {  // reference precision: fp64 accumulation
        hipLaunchKernelGGL((k_bn_reduce_f64<FWD>), rg, dim3(kT), 0, st, a);
    } else {
        Plan fp;
        const int nr = fused_plan(p->M, p->C, fp, false, G);
        if (nr) {
            const dim3 g = fused_args(a, fp, s, G);
            const bool res = p->residual != nullptr, relu = p->relu != 0;
#define GM_BN_FUSED_LAUNCH(NR)                                                                        \
    if (res && relu) hipLaunchKernelGGL((k_bn_fwd_fused<true, true, NR>), g, dim3(kT), 0, st, a);     \
    else if (res) hipLaunchKernelGGL((k_bn_fwd_fused<true, false, NR>), g, dim3(kT), 0, st, a);       \
    else if (relu) hipLaunchKernelGGL((k_bn_fwd_fused<false, true, NR>), g, dim3(kT), 0, st, a);      \
    else hipLaunchKernelGGL((k_bn_fwd_fused<false, false, NR>), g, dim3(kT), 0, st, a);
            if (nr < 0) { GM_BN_FUSED_LAUNCH(0) }
            else if (nr == 4) { GM_BN_FUSED_LAUNCH(4) }
            else if (nr == 8) { GM_BN_FUSED_LAUNCH(8) }
            else { GM_BN_FUSED_LAUNCH(16) }
#undef GM_BN_FUSED_LAUNCH
            return check_launch("k_bn_fwd_fused");
        }
        hipLaunchKernelGGL((k_bn_reduce<FWD, E>), rg, dim3(kT), 0, st, a);
    }
    if ((rc = check_launch("k_bn_reduce<fwd>"))) return rc;
    for (int gi = 0; gi < G; ++gi) {  // the apply: one launch per group
        ApplyArgs b = apply_args(p->M, p->C, p->relu);
        b.x = ps[gi].x; b.res = ps[gi].residual; b.out = ps[gi].y;
        b.mask_out = static_cast<uint8_t*>(ps[gi].relu_mask);
        b.coef = reinterpret_cast<float*>(reinterpret_cast<char*>(a.coef) + gi * a.scr_stride);
        launch_apply<E>(p->residual, p->relu, false, dim3(apply_grid(b.nvec)), st, b);
        if ((rc = check_launch("k_bn_apply"))) return rc;
    }
    return GM_OK;
}

template <typename E>
int bn_fwd_infer(const gm_bn_fwd* p, void* scratch, size_t bytes, void* stream, const char* fn) {
    GM_REQUIRE(p && p->x && p->y && p->gamma && p->beta && p->running_mean && p->running_var, "%s: null argument",
               fn);
    int rc = check_common(p->M, p->C, scratch, bytes, fn);
    if (rc) return rc;
    char* s = static_cast<char*>(scratch);
    float* coef = reinterpret_cast<float*>(s + make_plan(p->M, p->C).off_coef);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_bn_infer_coef, dim3((p->C + 255) / 256), dim3(256), 0, st, p->C, p->gamma, p->beta,
                       p->running_mean, p->running_var, p->eps, coef);
    if ((rc = check_launch("k_bn_infer_coef"))) return rc;
    ApplyArgs b = apply_args(p->M, p->C, p->relu);
    b.x = p->x; b.res = p->residual; b.out = p->y; b.coef = coef;
    launch_apply<E>(p->residual, p->relu, false, dim3(apply_grid(b.nvec)), st, b);
    return check_launch("k_bn_apply");
}

template <typename E>
int bn_bwd(const gm_bn_bwd* ps, int G, bool grouped, void* scratch, size_t bytes, void* stream, const char* fn) {
    int rc = check_groups_bwd(ps, G, fn);
    if (rc) return rc;
    const gm_bn_bwd* p = ps;
    const bool maskx = p->relu && !p->y;
    if ((rc = check_scratch(p->M, p->C, G, grouped, scratch, bytes, fn))) return rc;
    const Plan pl = make_plan(p->M, p->C);
    char* s = static_cast<char*>(scratch);
    ReduceArgs a{};
    a.M = p->M; a.C = p->C; a.tpr_log = pl.tpr_log; a.rpb = pl.rpb; a.relu = p->relu;
    a.SW = pl.SW; a.nrc = pl.nrc;
    a.accumulate = p->accumulate;
    set_scratch(a, pl, s, grouped);
    bwd_groups(a, ps, G);
    hipStream_t st = as_stream(stream);
    const dim3 rg(pl.nrc, pl.nslice, G);
    if constexpr (std::is_same<E, float>::value) {  // reference precision: fp64 accumulation
        if (maskx) hipLaunchKernelGGL((k_bn_reduce_f64<BWD_RELUX>), rg, dim3(kT), 0, st, a);
        else if (p->relu) hipLaunchKernelGGL((k_bn_reduce_f64<BWD_RELU>), rg, dim3(kT), 0, st, a);
        else hipLaunchKernelGGL((k_bn_reduce_f64<BWD>), rg, dim3(kT), 0, st, a);
    } else {
        Plan fp;
        const int nr = (!p->dres || p->relu) ? fused_plan(p->M, p->C, fp, true, G) : 0;
        if (nr) {
            const dim3 g = fused_args(a, fp, s, G);
            const bool ym = p->relu && p->relu_mask && !maskx;  // the forward's mask bytes in place of y
#define GM_BN_BWD_FUSED_LAUNCH(NR)                                                                                  \
    if (maskx) hipLaunchKernelGGL((k_bn_bwd_fused<BWD_RELUX, false, NR>), g, dim3(kT), 0, st, a);                   \
    else if (ym && p->dres) hipLaunchKernelGGL((k_bn_bwd_fused<BWD_RELU, true, NR, true>), g, dim3(kT), 0, st, a);  \
    else if (ym) hipLaunchKernelGGL((k_bn_bwd_fused<BWD_RELU, false, NR, true>), g, dim3(kT), 0, st, a);            \
    else if (p->relu && p->dres) hipLaunchKernelGGL((k_bn_bwd_fused<BWD_RELU, true, NR>), g, dim3(kT), 0, st, a);   \
    else if (p->relu) hipLaunchKernelGGL((k_bn_bwd_fused<BWD_RELU, false, NR>), g, dim3(kT), 0, st, a);             \
    else hipLaunchKernelGGL((k_bn_bwd_fused<BWD, false, NR>), g, dim3(kT), 0, st, a);
            if (nr < 0) { GM_BN_BWD_FUSED_LAUNCH(0) }
            else if (nr == 4) { GM_BN_BWD_FUSED_LAUNCH(4) }
            else { GM_BN_BWD_FUSED_LAUNCH(8) }
#undef GM_BN_BWD_FUSED_LAUNCH
            return check_launch("k_bn_bwd_fused");
        }
        if (maskx) hipLaunchKernelGGL((k_bn_reduce<BWD_RELUX, E>), rg, dim3(kT), 0, st, a);
        else if (p->relu) hipLaunchKernelGGL((k_bn_reduce<BWD_RELU, E>), rg, dim3(kT), 0, st, a);
        else hipLaunchKernelGGL((k_bn_reduce<BWD, E>), rg, dim3(kT), 0, st, a);
    }
    if ((rc = check_launch("k_bn_reduce<bwd>"))) return rc;
    for (int gi = 0; gi < G; ++gi) {  // the apply: one launch per group
        const gm_bn_bwd* q = ps + gi;
        ApplyArgs b = apply_args(p->M, p->C, p->relu);
        b.x = q->x; b.res = q->y; b.dy = q->dy; b.out = q->dx;
        b.out2 = q->dres;
        b.coef = reinterpret_cast<float*>(reinterpret_cast<char*>(a.coef) + gi * a.scr_stride);
        b.fcoef = q->fwd_coef;
        launch_apply_bwd<E>(p->relu, p->dres, maskx, dim3(apply_grid(b.nvec)), st, b);
        if ((rc = check_launch("k_bn_apply_bwd"))) return rc;
    }
    return GM_OK;
}

int bn_fwd_stats(const gm_bn_fwd* ps, int G, bool grouped, void* scratch, size_t bytes, void* stream,
                 const char* fn) {
    int rc = check_groups_fwd(ps, G, fn);
    if (rc) return rc;
    const gm_bn_fwd* p = ps;
    GM_REQUIRE(p->coef_out, "%s: coef_out required", fn);
    if ((rc = check_scratch(p->M, p->C, G, grouped, scratch, bytes, fn))) return rc;
    const Plan pl = make_plan(p->M, p->C);
    ReduceArgs a{};
    fill_fwd(a, ps, G, grouped, pl, static_cast<char*>(scratch));
    hipLaunchKernelGGL((k_bn_reduce<FWD, uint16_t>), dim3(pl.nrc, pl.nslice, G), dim3(kT), 0, as_stream(stream), a);
    return check_launch("k_bn_reduce<fwd>");
}

}  // namespace

namespace gm {
unsigned bn_faults_read(bool clear) {
    unsigned v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_bn_fault), sizeof(v), 0, hipMemcpyDeviceToHost) != hipSuccess) return ~0u;
    if (clear && v) {
        const unsigned z = 0;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_bn_fault), &z, sizeof(z), 0, hipMemcpyHostToDevice);
    }
    return v;
}
}  // namespace gm

extern "C" int gm_bn_set_concurrency(int n) {
    GM_REQUIRE(n >= 1 && n <= 1024, "gm_bn_set_concurrency: n must be in [1, 1024] (got %d)", n);
    gm::g_concurrency = n;
    return GM_OK;
}

extern "C" int gm_bn_set_fused_mode(int mode) {
    GM_REQUIRE(mode >= 0 && mode <= 2, "gm_bn_set_fused_mode: mode must be 0, 1 or 2 (got %d)", mode);
    gm::g_fused_env = mode;
    return GM_OK;
}

// What the planner picks for a bf16 training launch of G groups of [M, C] under the mode,
// concurrency and residency in effect: fused_plan's own return value.  Read-only.
extern "C" int gm_bn_fused_form(long long M, int C, int bwd, int G) {
    if (!shape_ok(M, C) || G < 1 || G > kMaxBnG) return 0;
    Plan fp;
    return fused_plan(M, C, fp, bwd != 0, G);
}

// Rows per workgroup of that launch (the fused plan's, or make_plan's on the two-launch path):
// a thread sums rows / (256 / min(C, 64) * 8) of them in fp32, then the row groups are summed.
extern "C" long long gm_bn_plan_rows(long long M, int C, int bwd, int G) {
    if (!shape_ok(M, C) || G < 1 || G > kMaxBnG) return 0;
    Plan fp;
    return fused_plan(M, C, fp, bwd != 0, G) ? fp.rpb : make_plan(M, C).rpb;
}

// Statistics half of the training forward only (one reduce launch): save_mean/invstd,
// running statistics, num_batches_tracked and the affine coefficients in coef_out
// (required); no y.  The apply is fused into the consumer (gm_bn_relu_maxpool2d_fwd_bf16).
extern "C" int gm_bn_fwd_stats_bf16(const gm_bn_fwd* p, void* scratch, size_t bytes, void* stream) {
    return bn_fwd_stats(p, 1, false, scratch, bytes, stream, "gm_bn_fwd_stats_bf16");
}

extern "C" size_t gm_bn_scratch_grouped(long long M, int C, int G) {
    if (M <= 0 || C < 8 || C > kMaxC || G < 1 || G > kMaxBnG) return 0;
    return grouped_bytes(M, C, G);
}

extern "C" int gm_bn_fwd_train_grouped_bf16(const gm_bn_fwd* ps, int G, void* scratch, size_t bytes, void* stream) {
    return bn_fwd_train<uint16_t>(ps, G, true, scratch, bytes, stream, "gm_bn_fwd_train_grouped_bf16");
}
extern "C" int gm_bn_bwd_grouped_bf16(const gm_bn_bwd* ps, int G, void* scratch, size_t bytes, void* stream) {
    return bn_bwd<uint16_t>(ps, G, true, scratch, bytes, stream, "gm_bn_bwd_grouped_bf16");
}
extern "C" int gm_bn_fwd_stats_grouped_bf16(const gm_bn_fwd* ps, int G, void* scratch, size_t bytes, void* stream) {
    return bn_fwd_stats(ps, G, true, scratch, bytes, stream, "gm_bn_fwd_stats_grouped_bf16");
}

extern "C" int gm_bn_fwd_train_bf16(const gm_bn_fwd* p, void* scratch, size_t bytes, void* stream) {
    return bn_fwd_train<uint16_t>(p, 1, false, scratch, bytes, stream, "gm_bn_fwd_train_bf16");
}
extern "C" int gm_bn_fwd_infer_bf16(const gm_bn_fwd* p, void* scratch, size_t bytes, void* stream) {
    return bn_fwd_infer<uint16_t>(p, scratch, bytes, stream, "gm_bn_fwd_infer_bf16");
}
extern "C" int gm_bn_bwd_bf16(const gm_bn_bwd* p, void* scratch, size_t bytes, void* stream) {
    return bn_bwd<uint16_t>(p, 1, false, scratch, bytes, stream, "gm_bn_bwd_bf16");
}
extern "C" int gm_bn_fwd_train_f32(const gm_bn_fwd* p, void* scratch, size_t bytes, void* stream) {
    return bn_fwd_train<float>(p, 1, false, scratch, bytes, stream, "gm_bn_fwd_train_f32");
}
extern "C" int gm_bn_infer_coef(const gm_bn_coef_entry* table, int n, int max_c, void* stream) {
    const char* fn = "gm_bn_infer_coef";
    GM_REQUIRE(table, "%s: null table", fn);
    GM_REQUIRE(n >= 1 && n <= 65535, "%s: n must be 1..65535 (got %d)", fn, n);
    GM_REQUIRE(max_c >= 1, "%s: max_c must be >= 1 (got %d)", fn, max_c);
    hipLaunchKernelGGL(k_bn_infer_coef_table, dim3((max_c + 255) / 256, n), dim3(256), 0, as_stream(stream), table);
    return check_launch("k_bn_infer_coef_table");
}

extern "C" int gm_bn_fwd_infer_f32(const gm_bn_fwd* p, void* scratch, size_t bytes, void* stream) {
    return bn_fwd_infer<float>(p, scratch, bytes, stream, "gm_bn_fwd_infer_f32");
}
extern "C" int gm_bn_bwd_f32(const gm_bn_bwd* p, void* scratch, size_t bytes, void* stream) {
    return bn_bwd<float>(p, 1, false, scratch, bytes, stream, "gm_bn_bwd_f32");
}

// The stem's BatchNorm + ReLU + max-pool backward in two launches (k_stem_pool_bn_bwd):
// d describes one view group's pool (N images, k 3, stride 2, pad 1, C 64); ps[g] the BN
// backward of group g with relu, fwd_coef (the mask from x) and no y / dres; ps[g].dy unused.
// apply = false: pass 1 only (statistics, dgamma / dbeta, the coefficients ca, cb, cc); the
// weight gradient of the stem then forms dx itself (gm_conv2d_wgrad_stem_bn_grouped_bf16).
static int stem_pool_bwd(const gm_pool_desc* d, int G, const void* dy_pool, const void* idx, const void* xsel,
                         const gm_bn_bwd* ps, void* scratch, size_t bytes, bool apply, const float** bcoef,
                         long long* bcoef_gs, void* stream, const char* fn) {
    GM_REQUIRE(d && dy_pool && idx && ps && G >= 1 && G <= kMaxBnG, "%s: bad arguments", fn);
    GM_REQUIRE(d->k == 3 && d->stride == 2 && d->pad == 1 && d->C == 64 && d->N >= 1 && d->H >= 2 && d->W >= 2,
               "%s: the stem's pool only (k 3, stride 2, pad 1, C 64)", fn);
    const int P = (d->H + 2 - 3) / 2 + 1, Q = (d->W + 2 - 3) / 2 + 1;
    GM_REQUIRE((d->H + 1) / 2 == P && (d->W + 1) / 2 == Q, "%s: pool geometry", fn);
    for (int g = 0; g < G; ++g) {
        const gm_bn_bwd& p = ps[g];
        GM_REQUIRE(p.M == (long long)d->N * d->H * d->W && p.C == d->C && p.relu && p.fwd_coef && !p.y && !p.dres &&
                       p.x && (p.dx || !apply) && p.gamma && p.save_mean && p.save_invstd && p.dgamma && p.dbeta &&
                       p.accumulate == ps[0].accumulate,
                   "%s: group %d: BN backward must be M = N*H*W, C, relu with fwd_coef, no y / dres", fn, g);
    }
    int rc;
    if ((rc = check_scratch(ps[0].M, ps[0].C, G, true, scratch, bytes, fn))) return rc;
    const Plan pl = make_plan(ps[0].M, ps[0].C);
    ReduceArgs a{};
    a.M = ps[0].M; a.C = ps[0].C; a.relu = 1; a.SW = ps[0].C; a.tpr_log = 3;
    a.accumulate = ps[0].accumulate;
    set_scratch(a, pl, static_cast<char*>(scratch), true);
    bwd_groups(a, ps, G);  // (dy, y, dres, relu_mask: unused by k_stem_pool_bn_bwd)
    StemPoolGeo pg;
    pg.Ng = d->N; pg.H = d->H; pg.W = d->W; pg.P = P; pg.Q = Q;
    pg.items = (long long)d->N * P * Q * (d->C / 8);
    GM_REQUIRE((long long)d->N * d->H * d->W * (d->C / 8) < (1ll << 31), "%s: a group's map exceeds 2^31 vectors", fn);
    // pass-1 partial rows: at most the plan's (the grouped scratch holds pl.nrc rows per group)
    int nrc = pl.nrc < kMaxRC ? pl.nrc : kMaxRC;
    pg.ipb = (pg.items + nrc - 1) / nrc;
    pg.ipb = (pg.ipb + kT - 1) / kT * kT;
    nrc = (int)((pg.items + pg.ipb - 1) / pg.ipb);
    a.nrc = nrc;
    pg.idx = static_cast<const uint2*>(idx);
    pg.gp = static_cast<const uint4*>(dy_pool);
    pg.xs = static_cast<const uint4*>(xsel);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL((k_stem_pool_bn_bwd<false>), dim3(nrc, 1, G), dim3(kT), 0, st, a, pg);
    if ((rc = check_launch("k_stem_pool_bn_bwd<reduce>"))) return rc;
    if (!apply) {  // group g's ca, cb, cc: a.coef + g * scr_stride bytes (group_args)
        *bcoef = a.coef;
        *bcoef_gs = (long long)(a.scr_stride / sizeof(float));
        return GM_OK;
    }
    long long grid = (pg.items + kT - 1) / kT;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL((k_stem_pool_bn_bwd<true>), dim3((unsigned)grid, 1, G), dim3(kT), 0, st, a, pg);
    return check_launch("k_stem_pool_bn_bwd<apply>");
}

extern "C" int gm_bn_relu_maxpool2d_bwd_grouped_bf16(const gm_pool_desc* d, int G, const void* dy_pool,
                                                     const void* idx, const void* xsel, const gm_bn_bwd* ps,
                                                     void* scratch, size_t bytes, void* stream) {
    return stem_pool_bwd(d, G, dy_pool, idx, xsel, ps, scratch, bytes, true, nullptr, nullptr, stream,
                         "gm_bn_relu_maxpool2d_bwd_grouped_bf16");
}

extern "C" int gm_bn_relu_maxpool2d_bwd_stats_grouped_bf16(const gm_pool_desc* d, int G, const void* dy_pool,
                                                           const void* idx, const void* xsel, const gm_bn_bwd* ps,
                                                           void* scratch, size_t bytes, const float** bcoef,
                                                           long long* bcoef_gs, void* stream) {
    const char* fn = "gm_bn_relu_maxpool2d_bwd_stats_grouped_bf16";
    GM_REQUIRE(bcoef && bcoef_gs, "%s: null coefficient outputs", fn);
    return stem_pool_bwd(d, G, dy_pool, idx, xsel, ps, scratch, bytes, false, bcoef, bcoef_gs, stream, fn);
}

// the kernel arguments of the finalizes from producer partial rows (and of the folded finalize +
// apply kernels, which also read the apply's tensors from grp[])
static void fwd_stats_args(gm::ReduceArgs& a, const gm_bn_fwd* ps, int G, float* stats, int rows) {
    const int C = ps[0].C;
    a.M = ps[0].M; a.C = C; a.SW = 64; a.tpr_log = 3; a.nrc = rows;
    a.momentum = ps[0].momentum; a.eps = ps[0].eps;
    a.part = stats;
    a.coef = stats + (size_t)rows * 2 * C;
    a.scr_stride = (unsigned long long)(rows + 1) * 2 * C * sizeof(float);
    a.hdr_words = 0;
    fwd_groups(a, ps, G);
}

static void bwd_stats_args(gm::ReduceArgs& a, const gm_bn_bwd* ps, int G, float* stats, int rows) {
    const int C = ps[0].C;
    a.M = ps[0].M; a.C = C; a.SW = 64; a.tpr_log = 3; a.nrc = rows;
    a.accumulate = ps[0].accumulate;
    a.part = stats;
    a.coef = stats;
    a.scr_stride = (unsigned long long)(rows + 1) * 2 * C * sizeof(float);
    a.hdr_words = 0;
    bwd_groups(a, ps, G);  // (y, dres, relu_mask: unused by the kernels from producer statistics)
}

// BatchNorm forward statistics from producer partial rows (gm_conv2d_fwd_grouped_bn_stats_bf16,
// the stem's gm_conv2d_fwd_grouped_stats_bf16): stats = [G] x ([C / 64 slices][rows][64 x (sum,
// sum of squares)] then 2C floats of coefficient scratch); ps[g] as for
// gm_bn_fwd_stats_grouped_bf16 (C a multiple of 64).  One block per (slice, group).
extern "C" int gm_bn_fwd_stats_finalize_grouped(const gm_bn_fwd* ps, int G, float* stats, int rows, void* stream) {
    const char* fn = "gm_bn_fwd_stats_finalize_grouped";
    int rc = check_groups_fwd(ps, G, fn);
    if (rc) return rc;
    const int C = ps[0].C;
    GM_REQUIRE(stats_shape_ok(stats, rows, C) && ps[0].M >= 1, "%s: C a multiple of 64, rows >= 1",
               fn);
    ReduceArgs a{};
    fwd_stats_args(a, ps, G, stats, rows);
    hipLaunchKernelGGL(k_bn_stats_finalize, dim3(1, C / 64, G), dim3(kFinT), 0, as_stream(stream), a);
    return check_launch("k_bn_stats_finalize");
}

// The apply after gm_bn_fwd_stats_finalize_grouped: y = relu?(x*sc + sh (+ residual)), the
// coefficients read from the statistics buffer; one launch for the G groups when their
// tensors are evenly strided (the view-batched trunk), else one per group.
// rstats / rrows: the residual-affine form (the residual BatchNorm's finalized statistics buffer)
static int fwd_apply(const gm_bn_fwd* ps, int G, const float* stats, int rows, const float* rstats, int rrows,
                     void* stream, const char* fn) {
    int rc = check_groups_fwd(ps, G, fn);
    if (rc) return rc;
    const gm_bn_fwd* p = ps;
    const int C = p->C;
    GM_REQUIRE(stats_shape_ok(stats, rows, C) && p->y, "%s: C a multiple of 64, rows >= 1, y", fn);
    const long long gs = p->M * C;  // elements
    bool strided = true;
    for (int g = 1; g < G; ++g) {
        const uint16_t* x0 = static_cast<const uint16_t*>(p->x);
        strided = strided && ps[g].x == x0 + g * gs &&
                  ps[g].y == static_cast<uint16_t*>(p->y) + g * gs &&
                  (!p->residual || ps[g].residual == static_cast<const uint16_t*>(p->residual) + g * gs) &&
                  (!p->relu_mask || ps[g].relu_mask == static_cast<uint8_t*>(p->relu_mask) + g * gs / 8);
    }
    const long long cgs = (long long)(rows + 1) * 2 * C;
    hipStream_t st = as_stream(stream);
    const int ng = strided ? 1 : G;
    for (int gi = 0; gi < ng; ++gi) {
        ApplyArgs b = apply_args(p->M, C, p->relu);
        b.x = ps[gi].x; b.res = ps[gi].residual; b.out = ps[gi].y;
        b.mask_out = static_cast<uint8_t*>(ps[gi].relu_mask);
        b.coef = stats + gi * cgs + (size_t)rows * 2 * C;
        b.gvec = strided ? gs / 8 : 0;
        b.cgs = strided ? cgs : 0;
        if (rstats) {
            const long long rcgs = (long long)(rrows + 1) * 2 * C;
            b.rcoef = rstats + gi * rcgs + (size_t)rrows * 2 * C;
            b.rcgs = strided ? rcgs : 0;
        }
        launch_apply<uint16_t>(p->residual, p->relu, rstats != nullptr, dim3(apply_grid(b.nvec), strided ? G : 1), st, b);
        if ((rc = check_launch("k_bn_apply"))) return rc;
    }
    return GM_OK;
}

extern "C" int gm_bn_fwd_apply_grouped_bf16(const gm_bn_fwd* ps, int G, const float* stats, int rows, void* stream) {
    return fwd_apply(ps, G, stats, rows, nullptr, 0, stream, "gm_bn_fwd_apply_grouped_bf16");
}

// The BatchNorm backward from producer statistics (include/greedymml.h): stats as written by
// gm_conv2d_dgrad_grouped_bn_stats_bf16 - [G] x ([C / 64][rows][64 x (sum dz, sum dz (x - mean))]
// + 2C floats), then G x 4C floats of backward coefficients.  ps[g]: the backward descriptor
// (relu with fwd_coef - the mask recomputed from x - or no relu; no dres), C a multiple of 64.
extern "C" size_t gm_bn_bwd_stats_coef_offset(int C, int G, int rows) {
    return (size_t)G * 2 * C * (size_t)(rows + 1);
}

static int check_bwd_from_stats(const gm_bn_bwd* ps, int G, const float* stats, int rows, const char* fn) {
    int rc = check_groups_bwd(ps, G, fn);
    if (rc) return rc;
    const int C = ps[0].C;
    GM_REQUIRE(stats_shape_ok(stats, rows, C) && ps[0].M >= 1, "%s: C a multiple of 64, rows >= 1",
               fn);
    GM_REQUIRE(!ps[0].dres && (!ps[0].relu || ps[0].fwd_coef),
               "%s: relu needs fwd_coef (mask from x); no residual gradient", fn);
    return GM_OK;
}

extern "C" int gm_bn_bwd_stats_finalize_grouped(const gm_bn_bwd* ps, int G, float* stats, int rows, void* stream) {
    const char* fn = "gm_bn_bwd_stats_finalize_grouped";
    int rc = check_bwd_from_stats(ps, G, stats, rows, fn);
    if (rc) return rc;
    const int C = ps[0].C;
    ReduceArgs a{};
    bwd_stats_args(a, ps, G, stats, rows);
    float* coef0 = stats + gm_bn_bwd_stats_coef_offset(C, G, rows);
    hipLaunchKernelGGL(k_bn_bwd_stats_finalize, dim3(1, C / 64, G), dim3(kFinT), 0, as_stream(stream), a, coef0,
                       (long long)4 * C);
    return check_launch("k_bn_bwd_stats_finalize");
}

extern "C" int gm_bn_bwd_apply_grouped_bf16(const gm_bn_bwd* ps, int G, const float* stats, int rows, void* stream) {
    const char* fn = "gm_bn_bwd_apply_grouped_bf16";
    int rc = check_bwd_from_stats(ps, G, stats, rows, fn);
    if (rc) return rc;
    const gm_bn_bwd* p = ps;
    const int C = p->C;
    GM_REQUIRE(p->dx && p->dy && p->x, "%s: null argument (dx, dy, x)", fn);
    const long long gs = p->M * C;
    bool strided = true;
    for (int g = 1; g < G; ++g)
        strided = strided && ps[g].x == static_cast<const uint16_t*>(p->x) + g * gs &&
                  ps[g].dy == static_cast<const uint16_t*>(p->dy) + g * gs &&
                  ps[g].dx == static_cast<uint16_t*>(p->dx) + g * gs &&
                  (!p->relu || ps[g].fwd_coef == p->fwd_coef + (size_t)g * 2 * C);
    const float* coef0 = stats + gm_bn_bwd_stats_coef_offset(C, G, rows);
    hipStream_t st = as_stream(stream);
    const int ng = strided ? 1 : G;
    for (int gi = 0; gi < ng; ++gi) {
        ApplyArgs b = apply_args(p->M, C, p->relu);
        b.x = ps[gi].x; b.dy = ps[gi].dy; b.out = ps[gi].dx;
        b.coef = coef0 + (size_t)gi * 4 * C;
        b.fcoef = ps[gi].fwd_coef;
        b.gvec = strided ? gs / 8 : 0;
        b.cgs = strided ? 4 * C : 0;
        b.fcgs = strided ? 2 * C : 0;
        // (check_bwd_from_stats: relu means the mask from x, and no dres)
        launch_apply_bwd<uint16_t>(p->relu, false, p->relu, dim3(apply_grid(b.nvec), strided ? G : 1), st, b);
        if ((rc = check_launch("k_bn_apply_bwd"))) return rc;
    }
    return GM_OK;
}

// ---------------------------------------------------------------------------------
// Finalize folded into the apply (k_bn_finalize_apply / k_bn_bwd_finalize_apply).
// The rule: blocks per (64-channel slice, group) of the folded launch, 0 = decline (the two
// launches).  From the per-shape table of tools/bn_fold_probe.py: the
// folded launch is fastest with about one 1024-thread block per CU over the whole grid
// (nb * C / 64 * G ~ kFoldGrid; half of that or twice that lost 1 - 3 us at every trunk shape),
// with at least two 128-pixel chunks per block, and it still won where every block re-reads
// twice the slice's own x + y bytes of partial rows (nb * rows * 512 B against M * 256 B: the
// downsample BatchNorm of layer 2, 784 rows), the largest share measured - so that is the bound.
// Past 2^25 elements over the G groups (64 MiB of bf16) the apply is bound by its streaming, and
// k_bn_apply's grid streams better than one 1024-thread block per CU: the largest shape that won
// had 25.7 M elements (layer 1 at C2), the smallest that lost 38.5 M (layer 2 of ResNet-50, 12 views).
constexpr int kFoldGrid = 256;
constexpr int kFoldMaxRows = 1024;
constexpr int kFoldReread = 2;
constexpr long long kFoldMaxElems = 1ll << 25;

extern "C" int gm_bn_fold_blocks(long long M, int C, int rows, int G) {
    if (M < 1 || rows < 1 || rows > kFoldMaxRows || C < 64 || C % 64 != 0 || G < 1) return 0;
    if (M * C >= (1ll << 31)) return 0;  // the folded kernels index a group's vectors in 32 bits
    if (M * C * G > kFoldMaxElems) return 0;
    long long nb = kFoldGrid / ((long long)(C / 64) * G);
    if (nb < 1) nb = 1;
    const long long by_pixels = (M + 255) / 256;  // <= the 4-vector work items (2 M per slice)
    if (nb > by_pixels) nb = by_pixels;
    const long long by_reread = (long long)kFoldReread * M * 256 / ((long long)rows * 512);
    if (nb > by_reread) nb = by_reread;
    return nb < 1 ? 0 : (int)nb;
}

static int fold_nb_arg(long long M, int C, int rows, int G, int nb, const char* fn) {
    GM_REQUIRE(nb >= 0 && nb <= 65535, "%s: nb in 0 (the rule) .. 65535 (got %d)", fn, nb);
    GM_REQUIRE(nb == 0 || M * C < (1ll << 31), "%s: nb > 0 needs M * C < 2^31", fn);
    return nb > 0 ? nb : gm_bn_fold_blocks(M, C, rows, G);
}

// nb > 0: the folded kernel with that many blocks per (slice, group), whatever the rule says
// (tests, tools/bn_fold_probe.py); nb == 0: the rule, and where it declines the two launches.
extern "C" int gm_bn_fwd_finalize_apply_grouped_bf16_ex(const gm_bn_fwd* ps, int G, float* stats, int rows, int nb,
                                                        void* stream) {
    const char* fn = "gm_bn_fwd_finalize_apply_grouped_bf16_ex";
    int rc = check_groups_fwd(ps, G, fn);
    if (rc) return rc;
    const int C = ps[0].C;
    GM_REQUIRE(stats_shape_ok(stats, rows, C) && ps[0].M >= 1 && ps[0].y,
               "%s: C a multiple of 64, rows >= 1, y", fn);
    for (int g = 0; g < G; ++g)
        GM_REQUIRE(!ps[g].relu_mask == !ps[0].relu_mask, "%s: relu_mask in all groups or none", fn);
    nb = fold_nb_arg(ps[0].M, C, rows, G, nb, fn);
    if (nb < 0) return nb;
    if (nb == 0) {
        if ((rc = gm_bn_fwd_stats_finalize_grouped(ps, G, stats, rows, stream))) return rc;
        return gm_bn_fwd_apply_grouped_bf16(ps, G, stats, rows, stream);
    }
    ReduceArgs a{};
    fwd_stats_args(a, ps, G, stats, rows);
    const dim3 grid(nb, C / 64, G), blk(kFinT);
    hipStream_t st = as_stream(stream);
    if (ps[0].residual) {
        if (ps[0].relu) hipLaunchKernelGGL((k_bn_finalize_apply<true, true>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((k_bn_finalize_apply<true, false>), grid, blk, 0, st, a);
    } else {
        if (ps[0].relu) hipLaunchKernelGGL((k_bn_finalize_apply<false, true>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((k_bn_finalize_apply<false, false>), grid, blk, 0, st, a);
    }
    return check_launch("k_bn_finalize_apply");
}

extern "C" int gm_bn_fwd_finalize_apply_grouped_bf16(const gm_bn_fwd* ps, int G, float* stats, int rows, void* stream) {
    return gm_bn_fwd_finalize_apply_grouped_bf16_ex(ps, G, stats, rows, 0, stream);
}

// The residual-affine form (include/greedymml.h): ps[g].residual is the raw input of the BatchNorm
// rps[g] (its x), which is finalized here too and never applied on its own.
extern "C" int gm_bn_fwd_finalize_apply_res_affine_grouped_bf16_ex(const gm_bn_fwd* ps, int G, float* stats, int rows,
                                                                   const gm_bn_fwd* rps, float* rstats, int rrows,
                                                                   int nb, void* stream) {
    const char* fn = "gm_bn_fwd_finalize_apply_res_affine_grouped_bf16_ex";
    int rc = check_groups_fwd(ps, G, fn);
    if (rc || (rc = check_groups_fwd(rps, G, fn))) return rc;
    const int C = ps[0].C;
    GM_REQUIRE(stats_shape_ok(stats, rows, C) && stats_shape_ok(rstats, rrows, C) && ps[0].M >= 1 && ps[0].y,
               "%s: C a multiple of 64, rows >= 1, y", fn);
    for (int g = 0; g < G; ++g) {
        GM_REQUIRE(!ps[g].relu_mask == !ps[0].relu_mask, "%s: relu_mask in all groups or none", fn);
        GM_REQUIRE(ps[g].residual && rps[g].x == ps[g].residual && rps[g].M == ps[0].M && rps[g].C == C &&
                       !rps[g].relu && !rps[g].residual,
                   "%s: group %d: the residual must be its BatchNorm's input (same shape, no ReLU, no residual)",
                   fn, g);
    }
    // both BatchNorms' rows are re-read by every block
    nb = fold_nb_arg(ps[0].M, C, rows + rrows, G, nb, fn);
    if (nb < 0) return nb;
    if (nb == 0) {  // two finalizes and one apply: still no apply pass for the residual's BatchNorm
        if ((rc = gm_bn_fwd_stats_finalize_grouped(ps, G, stats, rows, stream))) return rc;
        if ((rc = gm_bn_fwd_stats_finalize_grouped(rps, G, rstats, rrows, stream))) return rc;
        return fwd_apply(ps, G, stats, rows, rstats, rrows, stream, fn);
    }
    ReduceArgs a{};
    fwd_stats_args(a, ps, G, stats, rows);
    ResBn rb{};
    rb.nrc = rrows; rb.momentum = rps[0].momentum; rb.eps = rps[0].eps;
    rb.part = rstats;
    rb.scr_stride = (unsigned long long)(rrows + 1) * 2 * C * sizeof(float);
    for (int g = 0; g < G; ++g) {
        ResBn::Grp& q = rb.grp[g];
        q.gamma = rps[g].gamma; q.beta = rps[g].beta;
        q.rmean = rps[g].running_mean; q.rvar = rps[g].running_var;
        q.save_mean = rps[g].save_mean; q.save_invstd = rps[g].save_invstd;
        q.nbt = rps[g].num_batches_tracked; q.coef_out = rps[g].coef_out;
    }
    const dim3 grid(nb, C / 64, G), blk(kFinT);
    hipStream_t st = as_stream(stream);
    if (ps[0].relu) hipLaunchKernelGGL(k_bn_finalize_apply_raff<true>, grid, blk, 0, st, a, rb);
    else hipLaunchKernelGGL(k_bn_finalize_apply_raff<false>, grid, blk, 0, st, a, rb);
    return check_launch("k_bn_finalize_apply_raff");
}

extern "C" int gm_bn_fwd_finalize_apply_res_affine_grouped_bf16(const gm_bn_fwd* ps, int G, float* stats, int rows,
                                                                const gm_bn_fwd* rps, float* rstats, int rrows,
                                                                void* stream) {
    return gm_bn_fwd_finalize_apply_res_affine_grouped_bf16_ex(ps, G, stats, rows, rps, rstats, rrows, 0, stream);
}

extern "C" int gm_bn_bwd_finalize_apply_grouped_bf16_ex(const gm_bn_bwd* ps, int G, float* stats, int rows, int nb,
                                                        void* stream) {
    const char* fn = "gm_bn_bwd_finalize_apply_grouped_bf16_ex";
    int rc = check_bwd_from_stats(ps, G, stats, rows, fn);
    if (rc) return rc;
    const int C = ps[0].C;
    nb = fold_nb_arg(ps[0].M, C, rows, G, nb, fn);
    if (nb < 0) return nb;
    if (nb == 0) {
        if ((rc = gm_bn_bwd_stats_finalize_grouped(ps, G, stats, rows, stream))) return rc;
        return gm_bn_bwd_apply_grouped_bf16(ps, G, stats, rows, stream);
    }
    ReduceArgs a{};
    bwd_stats_args(a, ps, G, stats, rows);
    float* coef0 = stats + gm_bn_bwd_stats_coef_offset(C, G, rows);
    const dim3 grid(nb, C / 64, G), blk(kFinT);
    hipStream_t st = as_stream(stream);
    if (ps[0].relu) hipLaunchKernelGGL(k_bn_bwd_finalize_apply<true>, grid, blk, 0, st, a, coef0, (long long)4 * C);
    else hipLaunchKernelGGL(k_bn_bwd_finalize_apply<false>, grid, blk, 0, st, a, coef0, (long long)4 * C);
    return check_launch("k_bn_bwd_finalize_apply");
}

extern "C" int gm_bn_bwd_finalize_apply_grouped_bf16(const gm_bn_bwd* ps, int G, float* stats, int rows, void* stream) {
    return gm_bn_bwd_finalize_apply_grouped_bf16_ex(ps, G, stats, rows, 0, stream);
}
