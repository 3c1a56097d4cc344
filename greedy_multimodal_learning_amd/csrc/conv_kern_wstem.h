// The pixel-pair stem's weight gradient: k_wgrad_stem, k_wgrad_stem_bn (dy formed in the loader
// from the stem's BatchNorm + ReLU + max-pool backward) and k_stem_dw_crop.
#pragma once
#include "conv_kern_wfrag.h"

namespace gm {

// ---------------------------------------------------------------------------------
// Weight gradient of the pixel-pair stem (7 x 4 filter over 8-channel pairs, strides
// (2, 1), 64 output channels, no padding): dw[n][r][s][c] = sum over output pixels
// (b, p, q) of dy[b][p][q][n] x[b][2p + r][q + s][c].  A workgroup walks a contiguous
// run of output rows of one image with ONE WAVE PER TAP ROW r (7 waves): per output row
// the dy row (Q x 64 channels, 128-B pixel rows, XOR-swizzled 16-B chunks) and the input
// rows 2p .. 2p + 6 (a ring of two-row units, as k_conv_stem) sit in LDS; wave r reduces
// over the row's pixels in 16-pixel k-steps: A = dy^T (two 32-channel blocks), B = the
// input row 2p + r read as the [q][(s, c)] matrix whose rows overlap (row q = pairs
// q .. q + 3, 64 B at a 16-B pitch) - both by ds_read_b64_tr_b16, so one B fragment
// feeds two MFMAs and the whole tap row (s, c) = 32 columns is one accumulator column
// block.  Operands are register-staged two rows ahead (compiler-visible LDS accesses,
// exact waits); each workgroup writes its fp32 [64][224] partial, k_wgrad_sum reduces
// them in a fixed order.  The generic kernel (k_conv_wgrad4 <1, 2>) re-staged every
// input pixel per tap through an im2col tile: 117 us alone, 142 us in the step.
struct WStemArgs {
    const uint16_t* dy;  // [G][N][P][Q][64]: the output gradient, or (BN) the stem output y
    const uint16_t* x;   // [G][N][Hi][Wi][8] (pixel pairs)
    float* part;         // [G][splits][64][R * S * 8]
    int P, Q, Wi;
    int cpi, L, splits;  // chunks per image, output rows per chunk, workgroups per group (N * cpi)
    int uchunks, upitch, ichunks;  // 16-B chunks per unit (two input rows), LDS slot bytes, chunks per image
    long long gs_dy, gs_x;
    // BN (k_wgrad_stem<R, S, true>): dy formed in the loader from the stem's BatchNorm + ReLU +
    // max-pool backward (gm_conv2d_wgrad_stem_bn_grouped_bf16)
    const uint4* gp;     // [G][N][Pp][Qp][64] bf16 pool gradient
    const uint2* pidx;   // [G][N][Pp][Qp][64] window-relative argmax bytes
    const float* fcoef;  // group g: fcoef + g * fcoef_gs = sc[64], sh[64]
    const float* bcoef;  // group g: bcoef + g * bcoef_gs = ca[64], cb[64], cc[64]
    long long fcoef_gs, bcoef_gs, gs_pool;  // floats, floats, 16-B vectors
    int Pp, Qp;
};

// BN: the stem BatchNorm + ReLU + max-pool backward of the 8-channel chunks cg of the stem output y
// at row s, columns 2 pp and 2 pp + 1 (y0, y1), exactly as k_stem_pool_bn_bwd<true> forms dx
// (batchnorm.hip): the fp32 sum, in window order, of the pool gradients whose argmax is the
// element, rounded to bf16, masked by relu(y * sc + sh), then ca * d + (cb * y + cc) rounded to
// bf16.  Both columns lie in pool column pp (the odd one also in pp + 1), so each window's data is
// read once for the pair.  pool_g / pool_i: the two LDS slots of pooled rows (slot k & 1: gradient
// [Qp][64] bf16, argmax bytes [Qp][64]); cf: sc, sh, ca, cb, cc [64] each.
__device__ __forceinline__ void stem_bn_dx2(uint4& y0, uint4& y1, int s, int pp, int cg, const char* pool_g,
                                            const char* pool_i, const float* cf, int Pp, int Qp) {
    const int k0 = s >> 1, dh = s & 1;
    const uint32_t yw[2][4] = {{y0.x, y0.y, y0.z, y0.w}, {y1.x, y1.y, y1.z, y1.w}};
    uint32_t ow[2][4];
    const bool right = pp + 1 < Qp;
    // two halves of four channels, one after the other
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float d0[4] = {0.f, 0.f, 0.f, 0.f}, d1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int wr = 0; wr < 2; ++wr) {
            const int k = k0 + wr;
            if (wr > dh || k >= Pp) continue;  // uniform
            const int rb = (dh - 2 * wr + 1) * 3;  // window row of row s, times 3
            const char* gk = pool_g + (k & 1) * Qp * 128 + cg * 16 + h * 8;
            const char* ik = pool_i + (k & 1) * Qp * 64 + cg * 8 + h * 4;
            const uint2 ga = *reinterpret_cast<const uint2*>(gk + pp * 128);
            const uint32_t ia = *reinterpret_cast<const uint32_t*>(ik + pp * 64);
            uint2 gb = make_uint2(0, 0);
            uint32_t ib = ~0u;  // no window right of the last pool column: never a position
            if (right) {
                gb = *reinterpret_cast<const uint2*>(gk + (pp + 1) * 128);
                ib = *reinterpret_cast<const uint32_t*>(ik + (pp + 1) * 64);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t ba = (ia >> (8 * i)) & 0xffu, bb = (ib >> (8 * i)) & 0xffu;
                const float va = (i & 1) ? bf_hi(i < 2 ? ga.x : ga.y) : bf_lo(i < 2 ? ga.x : ga.y);
                const float vb = (i & 1) ? bf_hi(i < 2 ? gb.x : gb.y) : bf_lo(i < 2 ? gb.x : gb.y);
                // column 2pp: window (k, pp) at window column 1; column 2pp + 1: window (k, pp) at
                // column 2, then window (k, pp + 1) at column 0 (the reference's window order)
                if (ba == (uint32_t)(rb + 1)) d0[i] += va;
                if (ba == (uint32_t)(rb + 2)) d1[i] += va;
                if (bb == (uint32_t)rb) d1[i] += vb;
            }
        }
        const float4* c4 = reinterpret_cast<const float4*>(cf + cg * 8 + 4 * h);
        const float4 sc = c4[0], sh = c4[16], ca = c4[32], cb = c4[48], cc = c4[64];
        const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
        const float cav[4] = {ca.x, ca.y, ca.z, ca.w}, cbv[4] = {cb.x, cb.y, cb.z, cb.w};
        const float ccv[4] = {cc.x, cc.y, cc.z, cc.w};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = 4 * h + i;
                const float xf = (j & 1) ? bf_hi(yw[c][j >> 1]) : bf_lo(yw[c][j >> 1]);
                const float dr = __uint_as_float((uint32_t)Elem<uint16_t>::f2bf(c ? d1[i] : d0[i]) << 16);
                const float dm = fmaf(xf, scv[i], shv[i]) > 0.f ? dr : 0.f;
                o[i] = fmaf(cav[i], dm, fmaf(cbv[i], xf, ccv[i]));
            }
            ow[c][2 * h] = pack_bf2(o[0], o[1]);
            ow[c][2 * h + 1] = pack_bf2(o[2], o[3]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    y0 = make_uint4(ow[0][0], ow[0][1], ow[0][2], ow[0][3]);
    y1 = make_uint4(ow[1][0], ow[1][1], ow[1][2], ow[1][3]);
}

template <int R, int S>
__global__ __launch_bounds__(64 * R) void k_wgrad_stem(WStemArgs a) {
    constexpr int NT = 64 * R;                // threads: one wave per tap row
    constexpr int TC = R * S * 8;             // dw columns per output channel
    constexpr int DPT = (1024 + NT - 1) / NT;  // dy chunks per thread per row (Q <= 128)
    constexpr int RING = 8;
    static_assert(S * 8 == 32, "k_wgrad_stem: one tap row = one 32-column accumulator block");
    extern __shared__ __attribute__((aligned(16))) uint4 wsm[];
    char* lds = reinterpret_cast<char*>(wsm);  // [dy tiles 2 x Q*128][ring 8 x upitch]
    const int t = threadIdx.x, lane = t & 63;
    const int rr = __builtin_amdgcn_readfirstlane(t >> 6);
    const int grp = blockIdx.x / a.splits, wg = blockIdx.x - grp * a.splits;
    const int b = wg / a.cpi, c = wg - b * a.cpi;
    const int p0 = c * a.L, p1 = min(a.P, p0 + a.L);
    const int tileb = a.Q * 128, dchunks = a.Q * 8;
    char* const ring = lds + 2 * tileb;
    const uint4* const gdy = reinterpret_cast<const uint4*>(a.dy + grp * a.gs_dy) + (size_t)b * a.P * dchunks;
    const uint4* const gx = reinterpret_cast<const uint4*>(a.x + grp * a.gs_x) + (size_t)b * a.ichunks;
    struct Stage {
        uint4 d[DPT];
        uint4 x;
    };
    // dy row pr and input unit u (rows 2u, 2u + 1) -> registers; zeros past the image
    auto fetch = [&](int pr, int u, Stage& st, bool with_dy = true) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < DPT && with_dy; ++h) {
            const int cc = t + NT * h;
            st.d[h] = (cc < dchunks && pr < a.P) ? gdy[(size_t)pr * dchunks + cc] : make_uint4(0, 0, 0, 0);
        }
        const int gi = u * a.uchunks + t;
        st.x = (t < a.uchunks && gi < a.ichunks) ? gx[gi] : make_uint4(0, 0, 0, 0);
    };
    auto stash = [&](int pr, int u, const Stage& st, bool with_dy = true) __attribute__((always_inline)) {
        char* tile = lds + (pr & 1) * tileb;
#pragma unroll
        for (int h = 0; h < DPT && with_dy; ++h) {
            const int cc = t + NT * h;
            if (cc < dchunks) {
                const int px = cc >> 3, j = cc & 7;
                *reinterpret_cast<uint4*>(tile + px * 128 + ((j ^ wswz<128>(px)) << 4)) = st.d[h];
            }
        }
        if (t < a.uchunks) *reinterpret_cast<uint4*>(ring + (u & (RING - 1)) * a.upitch + t * 16) = st.x;
    };
    {  // prologue: dy row p0 and units p0 .. p0 + 3 (row p0's window)
        Stage s0, s1;
        fetch(p0, p0, s0, true);
        fetch(0, p0 + 1, s1, false);
        stash(p0, p0, s0, true);
        stash(0, p0 + 1, s1, false);
        fetch(0, p0 + 2, s0, false);
        fetch(0, p0 + 3, s1, false);
        stash(0, p0 + 2, s0, false);
        stash(0, p0 + 3, s1, false);
    }
    Stage sa, sb;  // iteration p stashes dy row p + 1 and unit p + 4, then fetches row p + 3, unit p + 6
    fetch(p0 + 1, p0 + 4, sa);
    fetch(p0 + 2, p0 + 5, sb);

    floatx16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    // tr-read lane geometry: 16-lane group g reads pixel rows 8 (g >> 1) + q4 (+ 4) of a
    // 16-pixel slice, columns 16 (g & 1) + 4 p4 .. + 3; lane l receives column l % 32
    const int g4 = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
    const int krow = 8 * (g4 >> 1) + q4, col = 16 * (g4 & 1) + 4 * p4;
    auto rowoff = [](int row, int ch) { return row * 128 + ((((ch >> 3) ^ wswz<128>(row))) << 4) + (ch & 7) * 2; };
    const int nks = a.Q >> 4;
    auto iteration = [&](int p, Stage& st) __attribute__((always_inline)) {
        __syncthreads();  // row p's dy tile and units p .. p + 3 are in LDS; row p - 1's reads are done
        stash(p + 1, p + 4, st);
        fetch(p + 3, p + 6, st);
        const char* tile = lds + (p & 1) * tileb;
        const char* xrow = ring + ((p + (rr >> 1)) & (RING - 1)) * a.upitch + (rr & 1) * a.Wi * 16;
        for (int ks = 0; ks < nks; ++ks) {
            const int px = 16 * ks + krow;
            const bf16x8 A0 = tr_frag(reinterpret_cast<const uint16_t*>(tile + rowoff(px, col)),
                                      reinterpret_cast<const uint16_t*>(tile + rowoff(px + 4, col)));
            const bf16x8 A1 = tr_frag(reinterpret_cast<const uint16_t*>(tile + rowoff(px, 32 + col)),
                                      reinterpret_cast<const uint16_t*>(tile + rowoff(px + 4, 32 + col)));
            const char* xb = xrow + (px + (col >> 3)) * 16 + (col & 7) * 2;
            const bf16x8 B = tr_frag(reinterpret_cast<const uint16_t*>(xb), reinterpret_cast<const uint16_t*>(xb + 64));
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, B, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, B, acc[1], 0, 0, 0);
        }
    };
    for (int p = p0; p < p1; p += 2) {
        iteration(p, sa);
        if (p + 1 < p1) iteration(p + 1, sb);
    }
    // the partial: dw[channel][rr * 32 + (s, c)], lane -> column, registers -> channels
    float* out = a.part + ((size_t)grp * a.splits + wg) * (64 * TC) + rr * 32 + (lane & 31);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int e = 0; e < 16; ++e) out[(size_t)(nb * 32 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3)) * TC] = acc[nb][e];
}

// k_wgrad_stem_bn: k_wgrad_stem with dy formed in the loader (stem_bn_dx2 above) - the stem's
// BatchNorm + ReLU + max-pool backward is never written (gm_conv2d_wgrad_stem_bn_grouped_bf16).
// Forming dy costs ~450 VALU instructions per wave and row, so the MFMA waves of ONE workgroup
// would serialise it with their MFMAs (barrier per row); here a workgroup is FOUR waves (tap rows
// {2w, 2w + 1}, wave 3 row 6 only: the busiest SIMD issues the same 28 MFMAs per row as
// k_wgrad_stem's), so two workgroups fit a CU (81 KB of LDS each, 2 waves per SIMD: up to 256
// VGPRs) and one's dy forming overlaps the other's MFMAs.  The A fragments (dy) of a k-slice feed
// both of a wave's tap rows.  Rows are prefetched three iterations ahead.  Same MFMA operands and
// order as k_wgrad_stem on the same tiles: bit-identical partials.
constexpr int kStemBnDepth = 3;  // rows of y in flight (registers; 2: 216 VGPRs, room for a split-sum wave beside it - equal in the step, profiles/r06_stem_wgrad_ab.txt)
template <int R, int S>
__global__ __launch_bounds__(256) void k_wgrad_stem_bn(WStemArgs a) {
    constexpr int NT = 256;
    constexpr int TC = R * S * 8;
    constexpr int RING = 8;
    static_assert(S * 8 == 32 && R == 7, "k_wgrad_stem_bn: the 7 x 4 pixel-pair stem");
    extern __shared__ __attribute__((aligned(16))) uint4 wsm[];
    char* lds = reinterpret_cast<char*>(wsm);  // [dy tiles 2][unit ring 8][pooled 2 x (grad, argmax)][coef]
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int grp = blockIdx.x / a.splits, wg = blockIdx.x - grp * a.splits;
    const int b = wg / a.cpi, c = wg - b * a.cpi;
    const int p0 = c * a.L, p1 = min(a.P, p0 + a.L);
    const int tileb = a.Q * 128, dchunks = a.Q * 8;
    const int npair = a.Q * 4;   // (column pair, channel chunk) items per row, <= 2 NT (host)
    const int npool = a.Qp * 8;  // pooled vectors per row, <= 2 NT (host)
    char* const ring = lds + 2 * tileb;
    char* const pool_g = ring + RING * a.upitch;
    char* const pool_i = pool_g + 2 * a.Qp * 128;
    float* const cf = reinterpret_cast<float*>(pool_i + 2 * a.Qp * 64);
    const uint4* const gy = reinterpret_cast<const uint4*>(a.dy + grp * a.gs_dy) + (size_t)b * a.P * dchunks;
    const uint4* const gx = reinterpret_cast<const uint4*>(a.x + grp * a.gs_x) + (size_t)b * a.ichunks;
    const size_t pimg = (size_t)b * a.Pp * a.Qp * 8;
    const uint4* const gpp = a.gp + grp * a.gs_pool + pimg;
    const uint2* const gpi = a.pidx + grp * a.gs_pool + pimg;
    const int cg = t & 7;  // the channel chunk of every item of this thread (NT % 8 == 0)
    struct Stage {
        uint4 y[2][2];  // item h = t + NT h: columns 2 pp, 2 pp + 1 of chunk cg (pp = item >> 3)
        uint4 x;        // unit chunk t
    };
    struct Pool {
        uint4 g[2];  // pooled vector t + NT h
        uint2 i[2];
    };
    auto fetch = [&](int pr, int u, Stage& st) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int it = t + NT * h;
            const bool ok = it < npair && pr < a.P;
            const size_t o = (size_t)pr * dchunks + (size_t)(it >> 3) * 16 + cg;
            st.y[h][0] = ok ? gy[o] : make_uint4(0, 0, 0, 0);
            st.y[h][1] = ok ? gy[o + 8] : make_uint4(0, 0, 0, 0);
        }
        const int gi = u * a.uchunks + t;
        st.x = (t < a.uchunks && gi < a.ichunks) ? gx[gi] : make_uint4(0, 0, 0, 0);
    };
    auto fetch_pool = [&](int pk, Pool& pq) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int v = t + NT * h;
            const bool ok = pk < a.Pp && v < npool;
            const size_t o = (size_t)pk * npool + v;
            pq.g[h] = ok ? gpp[o] : make_uint4(0, 0, 0, 0);
            pq.i[h] = ok ? gpi[o] : make_uint2(0, 0);
        }
    };
    auto stash_pool = [&](int pk, const Pool& pq) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int v = t + NT * h;
            if (v < npool) {
                *reinterpret_cast<uint4*>(pool_g + (pk & 1) * a.Qp * 128 + v * 16) = pq.g[h];
                *reinterpret_cast<uint2*>(pool_i + (pk & 1) * a.Qp * 64 + v * 8) = pq.i[h];
            }
        }
    };
    auto stash_unit = [&](int u, const Stage& st) __attribute__((always_inline)) {
        if (t < a.uchunks) *reinterpret_cast<uint4*>(ring + (u & (RING - 1)) * a.upitch + t * 16) = st.x;
    };
    // dy row pr from y row pr (registers) and the pooled rows in LDS, into tile pr & 1
    auto stash_dy = [&](int pr, const Stage& st) __attribute__((always_inline)) {
        char* tile = lds + (pr & 1) * tileb;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int it = t + NT * h;
            if (it < npair) {
                const int pp = it >> 3;
                uint4 v0 = st.y[h][0], v1 = st.y[h][1];
                stem_bn_dx2(v0, v1, pr, pp, cg, pool_g, pool_i, cf, a.Pp, a.Qp);
                const int px = 2 * pp;
                *reinterpret_cast<uint4*>(tile + px * 128 + ((cg ^ wswz<128>(px)) << 4)) = v0;
                *reinterpret_cast<uint4*>(tile + (px + 1) * 128 + ((cg ^ wswz<128>(px + 1)) << 4)) = v1;
            }
        }
    };
    const int k0 = p0 >> 1;  // p0 is even (the host plan's L is)
    Pool pq;
    {  // prologue: units p0 .. p0 + 3, pooled rows k0, k0 + 1, the coefficients; then dy row p0
        Stage s0, s1;
        fetch(p0, p0, s0);
        fetch(a.P, p0 + 1, s1);
        fetch_pool(k0, pq);
        stash_unit(p0, s0);
        stash_unit(p0 + 1, s1);
        stash_pool(k0, pq);
        fetch_pool(k0 + 1, pq);
        if (t < 64) {
            const float* fc = a.fcoef + grp * a.fcoef_gs;
            const float* bc = a.bcoef + grp * a.bcoef_gs;
            cf[t] = fc[t];
            cf[64 + t] = fc[64 + t];
            cf[128 + t] = bc[t];
            cf[192 + t] = bc[64 + t];
            cf[256 + t] = bc[128 + t];
        }
        stash_pool(k0 + 1, pq);
        fetch(a.P, p0 + 2, s1);
        stash_unit(p0 + 2, s1);
        fetch(a.P, p0 + 3, s1);
        stash_unit(p0 + 3, s1);
        __syncthreads();  // pooled rows k0, k0 + 1 and the coefficients are in LDS
        stash_dy(p0, s0);
    }
    // iteration p stashes dy row p + 1 and unit p + 4, then fetches row p + 4, unit p + 7.  Pooled
    // row j is fetched in iteration 2j - 5 and stashed in iteration 2j - 3 (odd iterations, one
    // register set), one iteration before row 2j - 1 - its first reader - is formed, after the
    // last reader of row j - 2 (its slot) - row 2j - 3, formed in iteration 2j - 4
    Stage sa, sb, sc;
    fetch(p0 + 1, p0 + 4, sa);
    fetch(p0 + 2, p0 + 5, sb);
    if constexpr (kStemBnDepth == 3) fetch(p0 + 3, p0 + 6, sc);
    fetch_pool(k0 + 2, pq);

    floatx16 acc[2][2];  // [tap row of the wave][channel block]
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[r][i][e] = 0.f;
    const bool two = w < 3;  // wave 3: tap row 6 only
    const int g4 = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
    const int krow = 8 * (g4 >> 1) + q4, col = 16 * (g4 & 1) + 4 * p4;
    auto rowoff = [](int row, int ch) { return row * 128 + ((((ch >> 3) ^ wswz<128>(row))) << 4) + (ch & 7) * 2; };
    const int nks = a.Q >> 4;
    auto iteration = [&](int p, Stage& st) __attribute__((always_inline)) {
        __syncthreads();  // row p's dy tile and units p .. p + 3 are in LDS; row p - 1's reads are done
        stash_unit(p + 4, st);
        if (p & 1) {
            stash_pool((p + 3) >> 1, pq);
            fetch_pool((p + 5) >> 1, pq);
        }
        stash_dy(p + 1, st);
        fetch(p + kStemBnDepth + 1, p + kStemBnDepth + 4, st);
        const char* tile = lds + (p & 1) * tileb;
        // tap rows 2w, 2w + 1 read input rows 2(p + w), 2(p + w) + 1: one unit
        const char* xrow = ring + ((p + w) & (RING - 1)) * a.upitch;
        for (int ks = 0; ks < nks; ++ks) {
            const int px = 16 * ks + krow;
            const bf16x8 A0 = tr_frag(reinterpret_cast<const uint16_t*>(tile + rowoff(px, col)),
                                      reinterpret_cast<const uint16_t*>(tile + rowoff(px + 4, col)));
            const bf16x8 A1 = tr_frag(reinterpret_cast<const uint16_t*>(tile + rowoff(px, 32 + col)),
                                      reinterpret_cast<const uint16_t*>(tile + rowoff(px + 4, 32 + col)));
            const char* xb = xrow + (px + (col >> 3)) * 16 + (col & 7) * 2;
            const bf16x8 B0 = tr_frag(reinterpret_cast<const uint16_t*>(xb), reinterpret_cast<const uint16_t*>(xb + 64));
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, B0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, B0, acc[0][1], 0, 0, 0);
            if (two) {
                const char* xb1 = xb + a.Wi * 16;
                const bf16x8 B1 = tr_frag(reinterpret_cast<const uint16_t*>(xb1),
                                          reinterpret_cast<const uint16_t*>(xb1 + 64));
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, B1, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, B1, acc[1][1], 0, 0, 0);
            }
        }
    };
    if constexpr (kStemBnDepth == 3) {
        for (int p = p0; p < p1; p += 3) {
            iteration(p, sa);
            if (p + 1 < p1) iteration(p + 1, sb);
            if (p + 2 < p1) iteration(p + 2, sc);
        }
    } else {
        for (int p = p0; p < p1; p += 2) {
            iteration(p, sa);
            if (p + 1 < p1) iteration(p + 1, sb);
        }
    }
    // the partial: dw[channel][rr * 32 + (s, c)] for the wave's tap rows rr = 2w (+ 1)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r == 1 && !two) break;
        float* out = a.part + ((size_t)grp * a.splits + wg) * (64 * TC) + (2 * w + r) * 32 + (lane & 31);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                out[(size_t)(nb * 32 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3)) * TC] = acc[r][nb][e];
    }
}
// The stem's weight gradient from its padded pixel-pair layout [G][K][R][Sp][2][4] (fp32) into each
// view's parameter gradient [K][R][S][C0] (the channels_last [K, C0, R, S] parameter): one launch
// for every view instead of a strided copy per view (gm_stem_dw_crop)
constexpr int kCropG = 16;
struct StemCropArgs {
    const float* dwp;
    float* dst[kCropG];
    int K, R, S, C0, Sp, accumulate;
};

__global__ __launch_bounds__(256) void k_stem_dw_crop(StemCropArgs a) {
    const int g = blockIdx.y;
    const int n = a.K * a.R * a.S * a.C0;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= n) return;
    int t = o;
    const int c = t % a.C0;
    t /= a.C0;
    const int s = t % a.S;
    t /= a.S;
    const int r = t % a.R, k = t / a.R;
    const float v = a.dwp[(size_t)g * a.K * a.R * a.Sp * 8 + ((size_t)(k * a.R + r) * a.Sp + (s >> 1)) * 8 + (s & 1) * 4 + c];
    float* d = a.dst[g] + o;
    *d = a.accumulate ? *d + v : v;
}
}  // namespace gm
