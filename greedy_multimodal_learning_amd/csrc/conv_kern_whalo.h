// k_wgrad_halo64: the weight gradient of 3x3 / stride-1 / pad-1 convolutions with W <= 62.
#pragma once
#include "conv_kern_wfrag.h"

namespace gm {

// k_wgrad_halo64: weight gradient of a 3x3 / stride-1 / pad-1 convolution with 64-channel
// multiples and W <= 62 (the ResNet-18 identity-block shapes), as 64 x (9 taps x 64) blocks of
// a view group's gradient held in the accumulators of one workgroup's four compute waves
// (wave (kh, ch): output channels 32 kh .., input channels 32 ch .., 9 taps = 9 x 32x32
// accumulators) while it walks a contiguous range of image rows.
//
// Staging unit: a "super-row" of 64 positions x 128 B = RPS = 64 / PP consecutive image rows
// of PP >= W + 2 positions each (PP = 64, 32, 16 for W <= 62, 30, 14).  In the x image,
// position m of a row holds input column m - 1 (zeros outside the image); in the dy image,
// position m holds output pixel m - 2 (two leading zeros).  Tap (rr, s) of output row p is
//   dw[rr][s] = sum over positions m of dy_p[m + 2 - s] (x) x_{p + rr - 1}[m]   (m from 0)
// per 16-position k-slice.  Operand economy (LDS fragment reads set this kernel's speed:
// halving them took the layer-1 launch from 47 to 37 us, while relaxing every wait did
// nothing): per slice ONE dy fragment is read (shift s = 2, rows m) and the shifts s = 1, 0 are
// made in registers from it and the next slice's fragment (v_permlane32_swap + v_alignbit:
// rows m + 1, m + 2 = this fragment moved up by one / two elements plus the next fragment's
// first rows); the x fragments of input rows p - 1, p, p + 1 stay in registers across output
// rows (a 4-set rotation), so per slice ONE x fragment is read (row p + 2, for the next output
// row).  2 + 2 transposed reads feed 9 MFMAs (12 before).  Kernel rows outside the image
// multiply zeroed operands.
//
// Both operands come through ds_read_b64_tr_b16 transposed reads (rows of 128 B, chunk XOR
// 4 * ((row >> 1) & 1): conflict-free for any 4 consecutive rows).  Four loader waves (one
// beside each compute wave's SIMD) keep D super-rows of LDS-DMA in flight (dy of super-row S
// with x of S + 2) under counted vmcnt waits; one raw barrier per super-row, before its second
// slice (the dy reads run three slices ahead, the x reads one image row ahead).  Each workgroup
// writes its fp32 partial slab [64][9 x 64] (split over rows; k_wgrad_sum reduces the splits in
// a fixed order).
struct WHaloArgs {
    const uint16_t* dy;  // [G][N*P][Q][K]  (P = H, Q = W)
    const uint16_t* x;   // [G][N*H][W][C]
    float* part;         // [G][splits][K][9*C] (tile (kb, cb) writes its 64 x 9 x 64 block)
    int N, H, W, rows, srows, splits, rpw;  // rows = N*H image rows per group, srows = super-rows,
                                            // rpw = super-rows per workgroup
    int K, C, kt, ct;    // channels; 64-channel tiles of dy (kt) and x (ct)
    long long gs_dy, gs_x;  // group strides (elements)
};

template <int D, int PP>
__global__ __launch_bounds__(512) void k_wgrad_halo64(WHaloArgs a) {
    static_assert(D >= 2 && (PP == 16 || PP == 32 || PP == 64), "halo64: D >= 2 super-rows in flight, PP = 16/32/64");
    constexpr int RPS = 64 / PP, SPR = PP / 16;  // image rows per super-row, k-slices per image row
    constexpr int XS = D + 3, DS = D + 1;  // x ring (super-rows R .. R+D+2), dy ring (R .. R+D)
    constexpr int SL = 8192, DSL = SL + 256;  // one super-row; dy slot + 2 zero pad positions
    constexpr int OX = 0, OD = XS * SL;       // x ring | dy ring
    extern __shared__ __attribute__((aligned(16))) uint4 wsm[];
    char* lds = reinterpret_cast<char*>(wsm);
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // block -> (group, 64 x 64 channel tile, split): splits innermost
    int bid = blockIdx.x;
    const int split = bid % a.splits;
    bid /= a.splits;
    const int tile = bid % (a.kt * a.ct), grp = bid / (a.kt * a.ct);
    const int kb = tile % a.kt, cb = tile / a.kt;
    const int R0 = split * a.rpw;
    const int R1 = min(a.srows, R0 + a.rpw);
    // each dy slot's two pad positions: ds_write, never a DMA target
    if (t < DS * 16) *reinterpret_cast<uint4*>(lds + OD + (t >> 4) * DSL + SL + (t & 15) * 16) = make_uint4(0, 0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // visible to every wave at the first barrier

    if (wave >= 4) {
        // loader waves: all LDS-DMA, so the compute waves' MFMA stream never carries a DMA issue.
        // Piece (lw, j) = slot positions 8 (2 lw + j) .. + 7, one image row (PP is a multiple of
        // 8); lane -> position 8 (2 lw + j) + lane / 8, source chunk (lane % 8) ^ swizzle(position).
        const int lw = wave - 4;
        typedef __attribute__((address_space(1))) const void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
        const void* zero = (const void*)g_wzero16;
        const uint16_t* __restrict__ gdy = a.dy + grp * a.gs_dy + kb * 64;
        const uint16_t* __restrict__ gx = a.x + grp * a.gs_x + cb * 64;
        int sub[2], xcol[2], dpx[2], xo[2], dyo[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int pos = (2 * lw + j) * 8 + (lane >> 3);
            const int sc = ((lane & 7) ^ wswz<128>(pos)) << 3;
            sub[j] = pos / PP;
            xcol[j] = pos % PP - 1;
            dpx[j] = pos % PP - 2;
            xo[j] = xcol[j] * a.C + sc;
            dyo[j] = dpx[j] * a.K + sc;
        }
        auto dma = [&](const void* src, int off) __attribute__((always_inline)) {
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + off), 16, 0, 0);
        };
        auto issue_x = [&](int R, int xs) __attribute__((always_inline)) {  // x super-row R into slot xs
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int g = R * RPS + sub[j];
                const bool ok = R >= 0 && g < a.rows && xcol[j] >= 0 && xcol[j] < a.W;
                dma(ok ? (const void*)(gx + (size_t)g * a.W * a.C + xo[j]) : zero, OX + xs * SL + (2 * lw + j) * 1024);
            }
        };
        auto issue_dy = [&](int R, int ds) __attribute__((always_inline)) {  // dy super-row R into slot ds
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int g = R * RPS + sub[j];
                const bool ok = R < R1 && g < a.rows && dpx[j] >= 0 && dpx[j] < a.W;
                dma(ok ? (const void*)(gdy + (size_t)g * a.W * a.K + dyo[j]) : zero, OD + ds * DSL + (2 * lw + j) * 1024);
            }
        };
        auto slot = [](int v, int n) { return ((v % n) + n) % n; };
        if (R0 < R1) {
            // prologue: x super-rows R0 - 1 .. R0 + 1, then D steps of (dy S, x S + 2); step R0 landed
            issue_x(R0 - 1, slot(R0 - 1, XS));
            issue_x(R0, slot(R0, XS));
            issue_x(R0 + 1, slot(R0 + 1, XS));
            for (int i = 0; i < D; ++i) {
                issue_dy(R0 + i, slot(R0 + i, DS));
                issue_x(R0 + i + 2, slot(R0 + i + 2, XS));
            }
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (D - 1)) : "memory");
            __builtin_amdgcn_s_barrier();
        }
        int dsn = slot(R0 + D, DS), xsn = slot(R0 + D + 2, XS);  // slots of DMA step R + D
        for (int R = R0; R < R1; ++R) {
            // step R + 1 landed (later steps may stay in flight); after the barrier no compute
            // wave reads dy super-row R - 1 or x super-row R - 1 any more (their slots are the
            // ones step R + D refills; uniform counts: past the range the pieces load zeros)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (D - 2)) : "memory");
            __builtin_amdgcn_s_barrier();
            issue_dy(R + D, dsn);
            issue_x(R + D + 2, xsn);
            dsn = dsn + 1 == DS ? 0 : dsn + 1;
            xsn = xsn + 1 == XS ? 0 : xsn + 1;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }

    const int kh = wave & 1, ch = wave >> 1;
    floatx16 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    // tr-read lane geometry (k_conv_wgrad4's): half-wave g >> 1 reads rows 8 (g >> 1) + q4 (+4) of
    // a 16-row slice, 4-column block p4 of the 32-column fragment, 16-column half g & 1; lane l
    // receives channel l % 32, rows 8 (l / 32) .. + 7 (the MFMA operand layout)
    const int g = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
    const int rbase = 8 * (g >> 1) + q4;
    const int acol = kh * 32 + 16 * (g & 1) + 4 * p4;
    const int bcol = ch * 32 + 16 * (g & 1) + 4 * p4;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
    auto rowoff = [](int row, int col) { return (unsigned)(row * 128 + ((((col >> 3) ^ wswz<128>(row))) << 4) + (col & 7) * 2); };
    const unsigned a_lane = rowoff(rbase, acol), b_lane = rowoff(rbase, bcol);
    const bool lo_half = lane < 32;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 F[4];  // dy fragments (shift 2) of slices ks .. ks + 3 of the super-row (ring by ks % 4)
    // x fragments of image rows g - 1, g, g + 1 and the prefetched g + 2, per slice of a row;
    // rotated by register copies at each image row's end (VALU beside the MFMAs)
    u32x4 Xm[SPR], X0[SPR], Xp[SPR], Xn[SPR];
    auto rd = [&](unsigned ad) __attribute__((always_inline)) {
        short4_t lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(ad));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:512" : "=v"(hi) : "v"(ad));
        return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
    auto mfma = [&](int i, u32x4 A, u32x4 B) __attribute__((always_inline)) {
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, B),
                                                        acc[i], 0, 0, 0);
    };
    // uniform slot bases of super-rows R (dy), R + 1 (dy, the reads two slices ahead) and
    // R - 1 .. R + 2 (x); the lane offsets are added per read
    int dsl = R0 % DS, xsl = (R0 - 1 + XS) % XS;
    auto dy_base = [&](int i) { const int d = dsl + i; return lds0 + (unsigned)(OD + (d >= DS ? d - DS : d) * DSL); };
    auto x_base = [&](int i) { const int x = xsl + i; return lds0 + (unsigned)(OX + (x >= XS ? x - XS : x) * SL); };
    // x fragment of image row R * RPS + r (r = -1 .. RPS + 1), slice kk of that row
    auto xaddr = [&](int r, int kk) __attribute__((always_inline)) {
        const int rr = r + RPS;  // >= 0: super-row R - 1 + rr / RPS
        return x_base(rr / RPS) + b_lane + (unsigned)(((rr % RPS) * PP + kk * 16) * 128);
    };

    int p = 0;  // image row (within its image) of the current output row
    if (R0 < R1) {
        __builtin_amdgcn_s_barrier();  // step R0 landed: dy R0, x R0 - 1 .. R0 + 2
        p = (int)(((long long)R0 * RPS) % a.H);
#pragma unroll
        for (int kk = 0; kk < SPR; ++kk) {
            Xm[kk] = rd(xaddr(-1, kk));
            X0[kk] = rd(xaddr(0, kk));
            Xp[kk] = rd(xaddr(1, kk));
        }
        F[0] = rd(dy_base(0) + a_lane);
        F[1] = rd(dy_base(0) + a_lane + 2048);
        F[2] = rd(dy_base(0) + a_lane + 4096);
    }
    for (int R = R0; R < R1; ++R) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int j = ks / SPR, kk = ks % SPR;  // image row of the super-row, slice of it
            if (ks == 1)  // super-row R + 1 landed; every wave done with super-row R - 1
                __builtin_amdgcn_s_barrier();
            // everything this slice consumes has landed: the last slice's reads were its x
            // fragment, then the dy fragment three slices ahead - only that one may still fly
            // (LDS reads return in order; no other LDS or scalar-memory op in this loop)
            asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(F[ks]), "+v"(F[(ks + 1) & 3]), "+v"(Xm[kk]), "+v"(X0[kk]),
                         "+v"(Xp[kk]));
            const u32x4 f2 = F[ks], fn = F[(ks + 1) & 3];
            // kernel rows 0 / 2 outside the image take zero operands (masks, not branches: a
            // conditional MFMA costs accumulator copies)
            const unsigned mt = p != 0 ? ~0u : 0u, mb = p != a.H - 1 ? ~0u : 0u;
            const u32x4 xm = Xm[kk] & mt, x0 = X0[kk], xp = Xp[kk] & mb;
            // shift s = 2 (the fragment as read); reads for later slices threaded behind
            mfma(2, f2, xm);
            __builtin_amdgcn_sched_barrier(0);
            Xn[kk] = rd(xaddr(j + 2, kk));  // image row + 2, for the next output row
            __builtin_amdgcn_sched_barrier(0);
            mfma(5, f2, x0);
            __builtin_amdgcn_sched_barrier(0);
            // dy three slices ahead (slices 1..3 read super-row R + 1's)
            F[(ks + 3) & 3] = rd(dy_base(ks >= 1 ? 1 : 0) + a_lane + (unsigned)(((ks + 3) & 3) * 2048));
            __builtin_amdgcn_sched_barrier(0);
            mfma(8, f2, xp);
            // shifts s = 1, 0: rows m + 1, m + 2 - the fragment moved up by one / two elements,
            // the vacated top elements from lane l + 32 (lanes 0-31: this fragment's rows 8, 9)
            // or lane l - 32 of the next fragment (lanes 32-63: its rows 0, 1)
            const auto sw = __builtin_amdgcn_permlane32_swap(f2[0], fn[0], false, false);
            const unsigned donor = lo_half ? sw[1] : sw[0];
            u32x4 f1, f0;
            f1[0] = __builtin_amdgcn_alignbit(f2[1], f2[0], 16);
            f1[1] = __builtin_amdgcn_alignbit(f2[2], f2[1], 16);
            f1[2] = __builtin_amdgcn_alignbit(f2[3], f2[2], 16);
            f1[3] = __builtin_amdgcn_alignbit(donor, f2[3], 16);
            f0[0] = f2[1]; f0[1] = f2[2]; f0[2] = f2[3]; f0[3] = donor;
            mfma(1, f1, xm);
            mfma(4, f1, x0);
            mfma(7, f1, xp);
            mfma(0, f0, xm);
            mfma(3, f0, x0);
            mfma(6, f0, xp);
            __builtin_amdgcn_sched_barrier(0);
            if (kk == SPR - 1) {  // the image row ends: rotate the x rows, next output row
                // (the register copies read the prefetched fragments: their reads must have landed)
#pragma unroll
                for (int q = 0; q < SPR; ++q) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(Xn[q]));
#pragma unroll
                for (int q = 0; q < SPR; ++q) {
                    Xm[q] = X0[q];
                    X0[q] = Xp[q];
                    Xp[q] = Xn[q];
                }
                p = p + 1 == a.H ? 0 : p + 1;
            }
        }
        dsl = dsl + 1 == DS ? 0 : dsl + 1;
        xsl = xsl + 1 == XS ? 0 : xsl + 1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // D[k][c]: col = lane & 31 (c), row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) (k)
    // the split's slab [K][9*C]; this tile fills rows kb*64 .., columns tap*C + cb*64 ..
    // (bf16 partials in the accumulators' own layout with 16-B stores measured no faster:
    // l1 49.6 vs 49.4 us with the sum, r04)
    const int TC = 9 * a.C;
    float* out = a.part + ((size_t)grp * a.splits + split) * ((size_t)a.K * TC);
#pragma unroll
    for (int tp = 0; tp < 9; ++tp) {
        const int col = tp * a.C + cb * 64 + ch * 32 + (lane & 31);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = kb * 64 + kh * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            out[(size_t)row * TC + col] = acc[tp][e];
        }
    }
}
}  // namespace gm
