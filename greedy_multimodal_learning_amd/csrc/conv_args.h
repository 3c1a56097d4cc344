// conv_igemm.hip's kernel argument structs and the epilogues its kernels share.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "gm_common.h"

namespace gm {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kMaxTap = 49;
constexpr int kMaxCls = 4;

struct ConvCls {
    uint16_t* out;
    int P, Q;                 // GEMM output grid of this class
    int oS, oH, oW;           // output pixel = (p*oS + oH, q*oS + oW)
    int ntap;
    int tile_start;           // first workgroup of this class
    int tiles_m;
    short tw[kMaxTap];        // weight tap index (r*S + s)
    signed char dh[kMaxTap], dw[kMaxTap];
    // the same taps as an Rc x Sc grid (tap = i*Sc + j): dh = cdh[i], dw = cdw[j],
    // weight tap = crs[i] + cs[j]; i = (tap * smag) >> 8 (exact for tap < ntap).  The
    // kernel reads them as 4-bit fields: pk_dh/pk_dw hold dh+8 / dw+8, pk_r/pk_s the
    // weight row r_i / column s_j (weight tap = r_i * Sw + s_j).
    int Rc, Sc, smag;
    int dh0, sh, dw0, sw;     // dh_i = dh0 + sh*i, dw_j = dw0 + sw*j (sh, sw = +-1)
    unsigned pk_dh, pk_dw, pk_r, pk_s;
    FastDiv fd_pq, fd_q;      // output pixel -> (b, p, q)
    signed char cdh[8], cdw[8];
    unsigned char crs[8], cs[8];
};

struct ConvArgs {
    const uint16_t* in;       // [N][Hi][Wi][C]
    const uint16_t* wt;       // [Nout][T][C]
    int N, Hi, Wi, C, logC;
    int Nout, T;              // output channels, taps per weight row
    int Sw;                   // weight columns (S)
    int Ho, Wo;               // full output spatial dims
    int sAh, sAw;             // input strides of the GEMM's A rows (H, W)
    int ncls;
    // split-K (lean kernel): grid = splits x tiles, split-major; split s of a tile takes
    // k-tiles [s*nk/S, (s+1)*nk/S) and the tile's splits hand their fp32 accumulators
    // on in order 0 -> 1 -> ... -> S-1 through ws (turnstile flags[tile], zero between
    // launches); the last split writes the output.  Deterministic (fixed order).
    const uint16_t* addend;   // dgrad, optional: out = conv + addend (same layout as out)
    // with it, optional: the addend's 1-bit mask (mask_bf2; group g at amask + g * gs_out / 8) -
    // out = conv + (addend where the bit is set), the addend never aliasing out
    const uint8_t* amask;
    int splits, tiles_total;
    float* ws;                // [tiles][MT*NT*16/4][256] float4
    unsigned* flags;          // [tiles]
    unsigned spin_limit;      // poll budget of the turnstile wait
    // view groups in one launch (the view-batched trunk): group g's input, weights and output
    // (and addend) sit gs_in / gs_wt / gs_out elements after group 0's; tiled kernels give
    // group g the tiles [g * tiles_g, (g + 1) * tiles_g), persistent ones gridDim / G workgroups
    int G, tiles_g;
    long long gs_in, gs_wt, gs_out;
    // forward, optional: BatchNorm statistics of the stored (bf16) output from the epilogue -
    // per group [Nout / 64 slices][stats_rows][64 channels][sum, sum of squares] fp32 partial
    // rows (k_conv_rw: one per persistent workgroup; store_tile_lds: one per output tile), then
    // 2 Nout floats of coefficient area: group g at stats + g * 2 Nout (stats_rows + 1)
    // (gm_bn_fwd_stats_finalize_grouped combines them)
    float* stats;
    int stats_rows;
    // input gradient, optional (with stats): the statistics of the BatchNorm backward whose dy
    // this launch writes - the BN's input x (out's layout), its forward coefficients sc, sh
    // ([G][2 Nout]) and save_mean ([G][Nout]): partial rows of (sum dz, sum dz (x - mean)) with
    // dz = dy where x sc + sh > 0 (the forward's ReLU; gm_bn_bwd_stats_finalize_grouped)
    const uint16_t* bnx;
    const float* bncoef;
    const float* bnmean;
    ConvCls cls[kMaxCls];
    // forward, optional (the *_affine kernel forms alone read these; last, so the fields above keep
    // their offsets): the evaluation epilogue y = act(acc sc[n] + sh[n] (+ addend)) with group g's
    // fp32 [2][Nout] (sc, sh) at coef + g * gs_coef, the addend as the residual (no mask), act the
    // NaN-propagating ReLU (relu != 0) or the identity; one rounding, no statistics
    const float* coef;
    long long gs_coef;
    int relu;
};

typedef float f32x2 __attribute__((ext_vector_type(2)));  // channel pairs: packed fp32 math

// BatchNorm statistics of one stored 16-B chunk (8 channels) into s1 / s2 (channel pairs):
// forward - sum y, sum y^2 of the stored values v; backward (BnB) - sum dz, sum dz (x - mean)
// of the stored input gradient v with x's chunk xv.  Invalid chunks arrive as zeros (no sum).
struct BnB {
    f32x2 sc[4], sh[4], mu[4];
};
__device__ __forceinline__ void bnb_load(const ConvArgs& a, int grp, int n, BnB& q) {
    const float* cf = a.bncoef + (size_t)grp * 2 * a.Nout + n;
    const float* mu = a.bnmean + (size_t)grp * a.Nout + n;
    const float4 s0 = *reinterpret_cast<const float4*>(cf), s1 = *reinterpret_cast<const float4*>(cf + 4);
    const float4 h0 = *reinterpret_cast<const float4*>(cf + a.Nout), h1 = *reinterpret_cast<const float4*>(cf + a.Nout + 4);
    const float4 m0 = *reinterpret_cast<const float4*>(mu), m1 = *reinterpret_cast<const float4*>(mu + 4);
    q.sc[0] = {s0.x, s0.y}; q.sc[1] = {s0.z, s0.w}; q.sc[2] = {s1.x, s1.y}; q.sc[3] = {s1.z, s1.w};
    q.sh[0] = {h0.x, h0.y}; q.sh[1] = {h0.z, h0.w}; q.sh[2] = {h1.x, h1.y}; q.sh[3] = {h1.z, h1.w};
    q.mu[0] = {m0.x, m0.y}; q.mu[1] = {m0.z, m0.w}; q.mu[2] = {m1.x, m1.y}; q.mu[3] = {m1.z, m1.w};
}
__device__ __forceinline__ void bn_acc_fwd(const unsigned (&v)[4], f32x2 (&s1)[4], f32x2 (&s2)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const f32x2 f = {bf_lo(v[k]), bf_hi(v[k])};
        s1[k] += f;
        s2[k] = __builtin_elementwise_fma(f, f, s2[k]);
    }
}
__device__ __forceinline__ void bn_acc_bwd(const unsigned (&v)[4], const unsigned (&xv)[4], const BnB& q,
                                           f32x2 (&s1)[4], f32x2 (&s2)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f32x2 d = {bf_lo(v[k]), bf_hi(v[k])};
        const f32x2 x = {bf_lo(xv[k]), bf_hi(xv[k])};
        const f32x2 z = __builtin_elementwise_fma(x, q.sc[k], q.sh[k]);  // fmaf(x, sc, sh) > 0: the
        d.x = z.x > 0.f ? d.x : 0.f;                                       // single-launch backward's mask
        d.y = z.y > 0.f ? d.y : 0.f;
        s1[k] += d;
        s2[k] = __builtin_elementwise_fma(d, x - q.mu[k], s2[k]);
    }
}

// sticky fault word of this translation unit (gm_device_faults): a split whose
// turnstile wait timed out
__device__ unsigned g_conv_fault = 0;

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

__device__ __attribute__((aligned(16))) const uint4 g_zero16[1] = {{0u, 0u, 0u, 0u}};

// bits i in [0, n) with 0 <= x + d0 + s*i < lim (s = +-1): one contiguous range
__device__ __forceinline__ unsigned span_mask(int x, int d0, int s, int n, int lim) {
    int lo, hi;
    if (s > 0) {
        lo = -(x + d0);
        hi = lim - 1 - (x + d0);
    } else {
        lo = x + d0 - (lim - 1);
        hi = x + d0;
    }
    lo = lo < 0 ? 0 : lo;
    hi = hi > n - 1 ? n - 1 : hi;
    return lo > hi ? 0u : ((2u << hi) - (1u << lo));
}

// ---- shared epilogue: D[n][m] layout: lane -> pixel m (col = lane&31), registers
// 4g..4g+3 -> channels 8g + 4h + 0..3: 8-byte NHWC stores, no LDS.  Through buffer
// resources, the stores and the addend loads (fused gradient join) are issued for the
// whole tile with no per-element branch: out-of-tile positions get an offset past the
// buffer's range, which the hardware drops (stores) or reads as zero (loads), so the
// addend loads are all in flight together instead of one dependent round trip per store.
// MASK: the masked addend (a.amask) is handled here - store_tile_lds's fallback; the kernels that
// store through store_tile directly (k_conv_igemm, k_conv_halo) get their masked addend
// materialised in dx before the launch (demask) and so keep their registers.
template <int MT, int NT, int BM, int BN, bool MASK = false>
__device__ __forceinline__ void store_tile(const ConvArgs& a, const ConvCls& cl, int m0, int n0, int wm, int wn,
                                           int fr, int fh, int M, floatx16 (&acc)[MT][NT], long long goff = 0) {
    const int PQ = cl.P * cl.Q;
    uint16_t* const outp = cl.out + goff;  // this group's output (and addend)
    const uint16_t* const addp = a.addend ? a.addend + goff : nullptr;
    const size_t out_bytes = (size_t)a.N * a.Ho * a.Wo * a.Nout * 2;
    if (out_bytes < 0x7ffff000u) {
        const auto orsrc = __builtin_amdgcn_make_buffer_rsrc(outp, 0, (int)out_bytes, 0x00020000);
        unsigned off[MT];
        bool mok[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            int m = m0 + wm * (BM / 2) + i * 32 + fr;
            mok[i] = m < M;
            m = mok[i] ? m : m0;
            const int b = (int)cl.fd_pq.div((uint32_t)m), pq = m - b * PQ;
            const int p = (int)cl.fd_q.div((uint32_t)pq), q = pq - p * cl.Q;
            const int ho = p * cl.oS + cl.oH, wo = q * cl.oS + cl.oW;
            off[i] = (unsigned)(((b * a.Ho + ho) * a.Wo + wo) * a.Nout) * 2u;
        }
        auto boff = [&](int i, int j, int gq) {
            const int n = n0 + wn * (BN / 2) + j * 32 + 8 * gq + 4 * fh;
            return (mok[i] && n < a.Nout) ? off[i] + (unsigned)n * 2u : 0xfffffff0u;
        };
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        u32x2 av[MT][NT][4];
        if (a.addend) {
            const auto arsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(addp), 0, (int)out_bytes,
                                                                 0x00020000);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq)
                        av[i][j][gq] = __builtin_amdgcn_raw_buffer_load_b64(arsrc, boff(i, j, gq), 0, 0);
            if (MASK && a.amask) {  // (Nout % 32 == 0) one mask dword per 32 channels: gq's byte, fh's nibble
                const auto mrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.amask + goff / 8), 0,
                                                                     (int)(out_bytes >> 4), 0x00020000);
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const unsigned w = __builtin_amdgcn_raw_buffer_load_b32(mrsrc, (boff(i, j, 0) - 8u * fh) >> 4,
                                                                                0, 0) >> (4 * fh);
#pragma unroll
                        for (int gq = 0; gq < 4; ++gq) {
                            av[i][j][gq].x = mask_bf2(av[i][j][gq].x, w >> (8 * gq));
                            av[i][j][gq].y = mask_bf2(av[i][j][gq].y, w >> (8 * gq + 2));
                        }
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    float o0 = acc[i][j][4 * gq], o1 = acc[i][j][4 * gq + 1];
                    float o2 = acc[i][j][4 * gq + 2], o3 = acc[i][j][4 * gq + 3];
                    if (a.addend) {
                        o0 += bf_lo(av[i][j][gq].x); o1 += bf_hi(av[i][j][gq].x);
                        o2 += bf_lo(av[i][j][gq].y); o3 += bf_hi(av[i][j][gq].y);
                    }
                    const u32x2 v = {pack_bf2(o0, o1), pack_bf2(o2, o3)};
                    __builtin_amdgcn_raw_buffer_store_b64(v, orsrc, boff(i, j, gq), 0, 0);
                }
        return;
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {  // outputs of 2 GB or more: 64-bit addressing
        const int m = m0 + wm * (BM / 2) + i * 32 + fr;
        if (m >= M) continue;
        const int b = (int)cl.fd_pq.div((uint32_t)m), pq = m - b * PQ;
        const int p = (int)cl.fd_q.div((uint32_t)pq), q = pq - p * cl.Q;
        const int ho = p * cl.oS + cl.oH, wo = q * cl.oS + cl.oW;
        uint16_t* dst = outp + ((size_t)(b * a.Ho + ho) * a.Wo + wo) * a.Nout;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int n = n0 + wn * (BN / 2) + j * 32 + 8 * gq + 4 * fh;
                if (n >= a.Nout) continue;
                float o0 = acc[i][j][4 * gq], o1 = acc[i][j][4 * gq + 1];
                float o2 = acc[i][j][4 * gq + 2], o3 = acc[i][j][4 * gq + 3];
                if (a.addend) {
                    uint2 av = *(const uint2*)(addp + (dst - outp) + n);
                    if (MASK && a.amask) {
                        const size_t e = (size_t)goff + (size_t)(dst - outp) + n;
                        const unsigned b = (unsigned)a.amask[e >> 3] >> (e & 4);
                        av.x = mask_bf2(av.x, b);
                        av.y = mask_bf2(av.y, b >> 2);
                    }
                    o0 += bf_lo(av.x); o1 += bf_hi(av.x); o2 += bf_lo(av.y); o3 += bf_hi(av.y);
                }
                uint2 v;
                v.x = pack_bf2(o0, o1);
                v.y = pack_bf2(o2, o3);
                *(uint2*)(dst + n) = v;
            }
    }
}

// The same epilogue through LDS for the 256-thread tiled kernels (2 x 2 waves of MT x NT
// fragments, the k-loop's LDS idle: every DMA has landed, the caller's barrier-free reads
// end at the __syncthreads below): the tile's BM pixel rows of BN channels are assembled in
// LDS - bf16, or fp32 with the fused gradient-join addend (added before the one rounding) -
// 16-B chunks XOR-swizzled by pixel, and leave as 16-B stores, BN / 8 lanes per contiguous
// pixel row segment.  The direct 8-B stores from the MFMA layout touch 32 pixel rows per
// instruction: 13 % of the layer-3 halo launch (41.4 us with, 36.0 without them).  Falls
// back to store_tile when the LDS is too small or the output needs 64-bit offsets.
// EPI = 1 (the *_affine kernels): acc sc[n] + sh[n] on the accumulators first, the ReLU after
// the residual (a.addend) joined in fp32; the plan holds the LDS of the fp32 tile and 32-bit
// output offsets (plan_epilogue), so there is no store_tile fallback and no statistics.
template <int MT, int NT, int BM, int BN, int EPI = 0>
__device__ __forceinline__ void store_tile_lds(const ConvArgs& a, const ConvCls& cl, int m0, int n0, int wm, int wn,
                                               int fr, int fh, int M, floatx16 (&acc)[MT][NT], long long goff,
                                               char* lds, int lds_bytes, int t, int grp) {
    static_assert(BM == 64 * MT && BN == 64 * NT, "store_tile_lds: 2 x 2 waves of MT x NT fragments");
    const size_t out_bytes = (size_t)a.N * a.Ho * a.Wo * a.Nout * 2;
    const bool f32 = a.addend != nullptr;
    if constexpr (EPI) {
        const float* const cf = a.coef + (long long)grp * a.gs_coef;
        const bool act = a.relu && !f32;  // with a residual the ReLU follows the join
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                int n = n0 + wn * (BN / 2) + j * 32 + 8 * gq + 4 * fh;  // this lane's 4 channels
                n = n < a.Nout ? n : 0;                                  // (Nout % 8 == 0; not stored past it)
                const float4 s = *reinterpret_cast<const float4*>(cf + n);
                const float4 h = *reinterpret_cast<const float4*>(cf + a.Nout + n);
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    float o0 = fmaf(acc[i][j][4 * gq], s.x, h.x), o1 = fmaf(acc[i][j][4 * gq + 1], s.y, h.y);
                    float o2 = fmaf(acc[i][j][4 * gq + 2], s.z, h.z), o3 = fmaf(acc[i][j][4 * gq + 3], s.w, h.w);
                    if (act) {
                        o0 = relu_nan(o0); o1 = relu_nan(o1); o2 = relu_nan(o2); o3 = relu_nan(o3);
                    }
                    acc[i][j][4 * gq] = o0; acc[i][j][4 * gq + 1] = o1;
                    acc[i][j][4 * gq + 2] = o2; acc[i][j][4 * gq + 3] = o3;
                }
            }
    } else {
        if (out_bytes >= 0x7ffff000u || BM * BN * (f32 ? 4 : 2) + 4 * (BN / 8) * 64 > lds_bytes) {
            store_tile<MT, NT, BM, BN, true>(a, cl, m0, n0, wm, wn, fr, fh, M, acc, goff);
            return;
        }
    }
    constexpr int CH = BN / 8, CF = BN / 4;  // bf16 / fp32 16-B chunks per pixel row
    constexpr int NU = BM * CH / 256;          // output chunks per thread
    __syncthreads();  // every wave is done with the k-loop's LDS
    if (f32) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int px = wm * (BM / 2) + i * 32 + fr, c = wn * (CF / 2) + 8 * j + 2 * gq + fh;
                    *reinterpret_cast<float4*>(lds + px * (BN * 4) + ((c ^ (px & (CF - 1))) << 4)) =
                        make_float4(acc[i][j][4 * gq], acc[i][j][4 * gq + 1], acc[i][j][4 * gq + 2], acc[i][j][4 * gq + 3]);
                }
    } else {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int px = wm * (BM / 2) + i * 32 + fr, c = wn * (CH / 2) + 4 * j + gq;
                    *reinterpret_cast<uint2*>(lds + px * (BN * 2) + ((c ^ (px & (CH - 1))) << 4) + 8 * fh) =
                        make_uint2(pack_bf2(acc[i][j][4 * gq], acc[i][j][4 * gq + 1]),
                                   pack_bf2(acc[i][j][4 * gq + 2], acc[i][j][4 * gq + 3]));
                }
    }
    __syncthreads();
    // this thread's chunks: pixel row px = e / CH, chunk c = e % CH of e = t + 256 u
    const int PQ = cl.P * cl.Q;
    // dense classes (forward, stride-1 input gradient): output pixel m is NHWC row m
    const bool dense = cl.oS == 1 && cl.oH == 0 && cl.oW == 0 && cl.P == a.Ho && cl.Q == a.Wo;
    unsigned off[NU];  // (computed branch-free per lane: a per-lane branch in these unrolled loops
                       // serialises them)
    if (dense) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int e = t + 256 * u, px = e / CH, c = e - px * CH;
            const int m = m0 + px, n = n0 + 8 * c;
            const unsigned o = (unsigned)m * (unsigned)a.Nout * 2u + (unsigned)n * 2u;
            off[u] = (m < M) & (n < a.Nout) ? o : 0xfffffff0u;
        }
    } else {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int e = t + 256 * u, px = e / CH, c = e - px * CH;
            const int n = n0 + 8 * c;
            const int m = min(m0 + px, M - 1);
            const int b = (int)cl.fd_pq.div((uint32_t)m), pq = m - b * PQ;
            const int p = (int)cl.fd_q.div((uint32_t)pq), q = pq - p * cl.Q;
            const unsigned o = (unsigned)((((b * a.Ho + p * cl.oS + cl.oH) * a.Wo + q * cl.oS + cl.oW) * a.Nout + n) * 2);
            off[u] = (m0 + px < M) & (n < a.Nout) ? o : 0xfffffff0u;
        }
    }
    uint16_t* const outp = cl.out + goff;
    const auto orsrc = __builtin_amdgcn_make_buffer_rsrc(outp, 0, (int)out_bytes, 0x00020000);
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    if (f32) {
        const auto arsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.addend + goff), 0, (int)out_bytes,
                                                             0x00020000);
        u32x4 av[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) av[u] = __builtin_amdgcn_raw_buffer_load_b128(arsrc, off[u], 0, 0);
        if (a.amask) {  // one mask byte per 16-B chunk: byte off / 16 (past the range: 0)
            const auto mrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.amask + goff / 8), 0,
                                                                 (int)(out_bytes >> 4), 0x00020000);
            unsigned mb[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) mb[u] = __builtin_amdgcn_raw_buffer_load_b8(mrsrc, off[u] >> 4, 0, 0);
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                av[u].x = mask_bf2(av[u].x, mb[u]);
                av[u].y = mask_bf2(av[u].y, mb[u] >> 2);
                av[u].z = mask_bf2(av[u].z, mb[u] >> 4);
                av[u].w = mask_bf2(av[u].w, mb[u] >> 6);
            }
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int e = t + 256 * u, px = e / CH, c = e - px * CH;
            const float4 f0 = *reinterpret_cast<const float4*>(lds + px * (BN * 4) + (((2 * c) ^ (px & (CF - 1))) << 4));
            const float4 f1 = *reinterpret_cast<const float4*>(lds + px * (BN * 4) + (((2 * c + 1) ^ (px & (CF - 1))) << 4));
            if constexpr (EPI) {
                float z[8] = {f0.x + bf_lo(av[u].x), f0.y + bf_hi(av[u].x), f0.z + bf_lo(av[u].y), f0.w + bf_hi(av[u].y),
                              f1.x + bf_lo(av[u].z), f1.y + bf_hi(av[u].z), f1.z + bf_lo(av[u].w), f1.w + bf_hi(av[u].w)};
                if (a.relu) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) z[k] = relu_nan(z[k]);
                }
                const u32x4 o = {pack_bf2(z[0], z[1]), pack_bf2(z[2], z[3]), pack_bf2(z[4], z[5]), pack_bf2(z[6], z[7])};
                __builtin_amdgcn_raw_buffer_store_b128(o, orsrc, off[u], 0, 0);
                continue;
            }
            const u32x4 o = {pack_bf2(f0.x + bf_lo(av[u].x), f0.y + bf_hi(av[u].x)),
                             pack_bf2(f0.z + bf_lo(av[u].y), f0.w + bf_hi(av[u].y)),
                             pack_bf2(f1.x + bf_lo(av[u].z), f1.y + bf_hi(av[u].z)),
                             pack_bf2(f1.z + bf_lo(av[u].w), f1.w + bf_hi(av[u].w))};
            __builtin_amdgcn_raw_buffer_store_b128(o, orsrc, off[u], 0, 0);
        }
        return;
    }
    u32x4 v[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int e = t + 256 * u, px = e / CH, c = e - px * CH;
        v[u] = *reinterpret_cast<const u32x4*>(lds + px * (BN * 2) + ((c ^ (px & (CH - 1))) << 4));
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) __builtin_amdgcn_raw_buffer_store_b128(v[u], orsrc, off[u], 0, 0);
    if constexpr (EPI) return;
    if (a.stats) {
        // BatchNorm statistics of the stored values (forward: y; input gradient: the BN
        // backward's dz against x): this thread's chunk c = t % CH (8 channels) over its NU
        // pixels, then the lanes sharing c (c + CH k: xor 8 / 16 / 32) and the four waves (LDS
        // past the tile) - one partial row per output tile, row m0 / BM
        f32x2 s1[4], s2[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s1[k] = s2[k] = f32x2{0.f, 0.f};
        if (a.bnx) {
            const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.bnx + goff), 0,
                                                                 (int)out_bytes, 0x00020000);
            u32x4 xv[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) xv[u] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off[u], 0, 0);
            const int n = n0 + 8 * (t % CH);
            BnB q;
            bnb_load(a, grp, n < a.Nout ? n : 0, q);
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const bool ok = off[u] != 0xfffffff0u;
                const unsigned w4[4] = {ok ? v[u].x : 0u, ok ? v[u].y : 0u, ok ? v[u].z : 0u, ok ? v[u].w : 0u};
                const unsigned x4[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
                bn_acc_bwd(w4, x4, q, s1, s2);
            }
        } else {
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const bool ok = off[u] != 0xfffffff0u;
                const unsigned w4[4] = {ok ? v[u].x : 0u, ok ? v[u].y : 0u, ok ? v[u].z : 0u, ok ? v[u].w : 0u};
                bn_acc_fwd(w4, s1, s2);
            }
        }
        float r[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r[4 * k] = s1[k].x; r[4 * k + 1] = s2[k].x; r[4 * k + 2] = s1[k].y; r[4 * k + 3] = s2[k].y;
        }
        const int lane = t & 63, wave = t >> 6;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float x = r[q];
            if (CH == 8) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xf, 0xf, false));
            x += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), 0x401f));
            x += __shfl_xor(x, 32);
            r[q] = x;
        }
        float* red = reinterpret_cast<float*>(lds + BM * BN * 2);  // [4 waves][CH chunks][16]
        if (lane < CH) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<float4*>(red + (wave * CH + lane) * 16 + 4 * q) =
                    make_float4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
        }
        __syncthreads();
        if (t < BN) {  // channel n0 + t: chunk t / 8, channel j = t % 8 of it
            const int c = t >> 3, j = t & 7;
            float S1 = 0.f, S2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                S1 += red[(w * CH + c) * 16 + 2 * j];
                S2 += red[(w * CH + c) * 16 + 2 * j + 1];
            }
            const int n = n0 + t;
            if (n < a.Nout) {
                float* sp = a.stats + (size_t)grp * 2 * a.Nout * (a.stats_rows + 1);
                *reinterpret_cast<float2*>(sp + ((size_t)(n >> 6) * a.stats_rows + m0 / BM) * 128 + (n & 63) * 2) =
                    make_float2(S1, S2);
            }
        }
    }
}

// s_barrier that is also a compiler memory barrier: without the fences the scheduler may
// move an LDS access of the next tile above the raw barrier (it is not a memory fence)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// LDS fragment read as inline asm (k_conv_rw, k_conv_stem): hipcc does not see these as
// LDS accesses, so it neither drains the LDS-DMA in flight before them nor counts them;
// the kernels wait for them explicitly (lgkmcnt(0) tied to the fragments about to be used)
template <int OFF>
__device__ __forceinline__ bf16x8 lds_rd128(unsigned addr) {
    bf16x8 d;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF));
    return d;
}

}  // namespace gm
