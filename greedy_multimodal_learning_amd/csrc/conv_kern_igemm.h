// conv_igemm.hip: the im2col kernel (k_conv_igemm) and its lean variant (k_conv_igemm_ut).
#pragma once
#include "conv_args.h"

namespace gm {

// (ST: always 2 LDS stages - it keeps the kernel's name in the profiles; the 3-stage ring measured
// slower and is gone)
template <int BM, int BN, bool UT, int ST = 2>
__global__ __launch_bounds__(256) void k_conv_igemm(ConvArgs a) {
    constexpr int BK = 64;
    constexpr int AR = BM / 32;       // A rows per thread
    constexpr int BR = BN / 32;       // B rows per thread
    constexpr int MT = BM / 64, NT = BN / 64;  // 32x32 MFMA tiles per wave
    static_assert(ST == 2, "k_conv_igemm: two LDS stages");
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    uint4* As = smem;                           // [ST][BM][8] (16-B chunks)
    uint4* Bs = smem + ST * BM * 8;             // [ST][BN][8]

    const int bid = blockIdx.x;
    int ci = 0;
#pragma unroll
    for (int q = 1; q < kMaxCls; ++q)
        if (q < a.ncls && bid >= a.cls[q].tile_start) ci = q;
    const ConvCls& cl = a.cls[ci];
    const int wgid = bid - cl.tile_start;
    const int tm = wgid % cl.tiles_m, tn = wgid / cl.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int PQ = cl.P * cl.Q;
    const int M = a.N * PQ;
    const int Ktot = cl.ntap * a.C;
    const int nk = (Ktot + BK - 1) / BK;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    // tap table -> LDS (static indices only into the kernel-argument struct)
    int* tapt = (int*)(smem + ST * (BM + BN) * 8);
#pragma unroll
    for (int i = 0; i < kMaxTap; ++i)
        if (t == i && i < cl.ntap)
            tapt[i] = (int)cl.tw[i] | ((int)(cl.dh[i] + 128) << 8) | ((int)(cl.dw[i] + 128) << 16);
    __syncthreads();
    const int wm = wave >> 1, wn = wave & 1;
    const int slot = lane & 7;                  // 16-B LDS slot this lane's DMA fills

    // Staging is LDS-DMA (global_load_lds_dwordx4): a wave instruction writes 64 x 16 B
    // = 8 rows x 128 B linearly, so the XOR swizzle moves to the SOURCE: the lane that
    // fills slot s of row r loads global chunk s ^ f(r).  Zero taps (padding) read a
    // 16-B zero block of the code object.
    const uint16_t* a_ptr[AR];
    int a_h[AR], a_w[AR], a_gc[AR];
#pragma unroll
    for (int j = 0; j < AR; ++j) {
        const int row = (wave * AR + j) * 8 + (lane >> 3);
        const int m = m0 + row;
        a_gc[j] = slot ^ ((row >> 1) & 7);
        if (m < M) {
            const int b = m / PQ, pq = m - b * PQ;
            const int p = pq / cl.Q, q = pq - p * cl.Q;
            a_h[j] = p * a.sAh;
            a_w[j] = q * a.sAw;
            a_ptr[j] = a.in + ((size_t)((b * a.Hi + a_h[j]) * a.Wi + a_w[j]) << a.logC);
        } else {
            a_h[j] = -(1 << 28);  // never valid
            a_w[j] = 0;
            a_ptr[j] = a.in;
        }
    }
    const uint16_t* b_ptr[BR];
    bool b_ok[BR];
    int b_gc[BR];
#pragma unroll
    for (int j = 0; j < BR; ++j) {
        const int row = (wave * BR + j) * 8 + (lane >> 3);
        const int n = n0 + row;
        b_gc[j] = slot ^ ((row >> 1) & 7);
        b_ok[j] = n < a.Nout;
        b_ptr[j] = a.wt + (size_t)(b_ok[j] ? n : 0) * a.T * a.C;
    }
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    auto issue = [&](int kt, int buf) {
        if constexpr (UT) {
            // C >= 64: a 64-wide k-tile lies inside one tap -> ONE table read per tile
            const int k = kt * BK;
            const int te = __builtin_amdgcn_readfirstlane(tapt[k >> a.logC]);
            const int dh = ((te >> 8) & 0xff) - 128, dw = ((te >> 16) & 0xff) - 128;
            const int c0 = k & (a.C - 1);
            const int aoff = ((dh * a.Wi + dw) << a.logC) + c0;
            const int boff = (te & 0xff) * a.C + c0;
#pragma unroll
            for (int j = 0; j < AR; ++j) {
                const bool ok = (unsigned)(a_h[j] + dh) < (unsigned)a.Hi && (unsigned)(a_w[j] + dw) < (unsigned)a.Wi;
                const void* src = ok ? (const void*)(a_ptr[j] + aoff + a_gc[j] * 8) : (const void*)g_zero16;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(As + (buf * BM + (wave * AR + j) * 8) * 8),
                                                 16, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < BR; ++j) {
                const void* src = b_ok[j] ? (const void*)(b_ptr[j] + boff + b_gc[j] * 8) : (const void*)g_zero16;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(Bs + (buf * BN + (wave * BR + j) * 8) * 8),
                                                 16, 0, 0);
            }
        } else {
#pragma unroll
            for (int j = 0; j < AR; ++j) {
                const int k = kt * BK + a_gc[j] * 8;
                const bool kin = k < Ktot;
                const int te = tapt[kin ? (k >> a.logC) : 0];
                const int c = k & (a.C - 1);
                const int dh = ((te >> 8) & 0xff) - 128, dw = ((te >> 16) & 0xff) - 128;
                const int hi = a_h[j] + dh, wi = a_w[j] + dw;
                const bool ok = kin && (unsigned)hi < (unsigned)a.Hi && (unsigned)wi < (unsigned)a.Wi;
                const void* src = ok ? (const void*)(a_ptr[j] + (((dh * a.Wi + dw) << a.logC) + c))
                                     : (const void*)g_zero16;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(As + (buf * BM + (wave * AR + j) * 8) * 8),
                                                 16, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < BR; ++j) {
                const int k = kt * BK + b_gc[j] * 8;
                const bool kin = k < Ktot;
                const int te = tapt[kin ? (k >> a.logC) : 0];
                const int c = k & (a.C - 1);
                const void* src = (kin && b_ok[j]) ? (const void*)(b_ptr[j] + (te & 0xff) * a.C + c)
                                                   : (const void*)g_zero16;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(Bs + (buf * BN + (wave * BR + j) * 8) * 8),
                                                 16, 0, 0);
            }
        }
    };

    floatx16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;
    auto compute = [&](int buf) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int chunk = ks * 2 + fh;
            bf16x8 af[MT], bfr[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int row = wm * (BM / 2) + i * 32 + fr;
                af[i] = __builtin_bit_cast(bf16x8, As[(buf * BM + row) * 8 + swz(row, chunk)]);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int row = wn * (BN / 2) + j * 32 + fr;
                bfr[j] = __builtin_bit_cast(bf16x8, Bs[(buf * BN + row) * 8 + swz(row, chunk)]);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    // weights as the MFMA A operand, pixels as B: D[n][m], so each lane ends
                    // up holding 4 consecutive output channels of ONE pixel per register group
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
        }
    };
    // 2 LDS buffers: the DMA of tile kt+1 runs under the MFMAs of tile kt; the barrier
    // at the end of each step (vmcnt(0) + s_barrier) publishes it.
    if (nk > 0) issue(0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) issue(kt + 1, buf ^ 1);
        compute(buf);
        __syncthreads();
    }

    store_tile<MT, NT, BM, BN>(a, cl, m0, n0, wm, wn, fr, fh, M, acc);
}

// Lean variant for C >= 64 (a 64-wide k-tile lies inside one tap) and <= 32 taps:
//  * per-row tap validity precomputed as a bitmask (one bit test per DMA, no bounds math),
//  * wave index in an SGPR, so every LDS-DMA destination (M0) is scalar arithmetic,
//  * per-lane LDS fragment offsets precomputed and the k-loop unrolled by the two
//    buffers, so every ds_read_b128 is base VGPR + immediate (no address VALU),
//  * the tap-table entry of the next k-tile is read one step ahead.
// Main loop: two LDS stages with ONE raw barrier per k-tile: wait for tile k's DMA, barrier,
// refill the stage compute(k-1) released, compute(k) with the next k-step's fragments read
// from LDS under the current k-step's MFMAs.  (PIPE: always 2 - it keeps the kernel's name in
// the profiles; the __syncthreads form 0 and the 3-stage form 3 measured slower and are gone,
// DESIGN.md section 8.)
// (The kernel's text is conv_igemm_ut_body, inlined into k_conv_igemm_ut - EPI = 0, the symbol
// and the code of the training step - and into k_conv_igemm_ut_affine, EPI = 1: the evaluation
// epilogue of store_tile_lds, applied by the split that writes the output.)
template <int BM, int BN, int EPI>
__device__ __forceinline__ void conv_igemm_ut_body(const ConvArgs& a) {
    constexpr int BK = 64;
    constexpr int AR = BM / 32, BR = BN / 32;
    constexpr int MT = BM / 64, NT = BN / 64;
    constexpr int SA = BM * 128, SB = BN * 128;  // bytes per stage
    constexpr int NST = 2;                       // LDS stages
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    char* lds = reinterpret_cast<char*>(smem);   // [A0..A(NST-1)][B0..B(NST-1)]

    int bid = blockIdx.x;
    int split = 0;
    if (a.splits > 1) {
        split = bid / a.tiles_total;
        bid -= split * a.tiles_total;
    }
    const int tid = bid;  // launch-wide tile index: split-K slab and turnstile word
    int g = 0;            // view group
    if (a.G > 1) {
        g = bid / a.tiles_g;
        bid -= g * a.tiles_g;
    }
    const uint16_t* const gin = a.in + g * a.gs_in;
    const uint16_t* const gwt = a.wt + g * a.gs_wt;
    int ci = 0;
#pragma unroll
    for (int q = 1; q < kMaxCls; ++q)
        if (q < a.ncls && bid >= a.cls[q].tile_start) ci = q;
    const ConvCls& cl = a.cls[ci];
    const int wgid = bid - cl.tile_start;
    // tile order: tn fastest (split-K needs the dispatch order), so that
    // with a power-of-two column count the round-robin XCD dealing (block b on XCD b % 8)
    // keeps each weight slice on the same XCD(s) - L2-resident instead of re-fetched
    const int tiles_n = (a.Nout + BN - 1) / BN;
    const int tm = wgid / tiles_n;
    const int tn = wgid - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int PQ = cl.P * cl.Q;
    const int M = a.N * PQ;
    const int nk_all = (cl.ntap * a.C) / BK;
    const int kt0 = split * nk_all / a.splits;
    const int nk = (split + 1) * nk_all / a.splits - kt0;

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int slot = lane & 7;
    // the class's tap grid, unpacked in SGPRs from 4-bit fields
    const unsigned pk_dh = cl.pk_dh, pk_dw = cl.pk_dw, pk_r = cl.pk_r, pk_s = cl.pk_s;

    // per A row: pixel base pointer and the tap validity as two bitmasks over the
    // grid's rows (bit i: h + cdh[i] in range) and columns (bit j: w + cdw[j] in range)
    const uint16_t* a_ptr[AR];
    unsigned a_vr[AR], a_vs[AR];
#pragma unroll
    for (int j = 0; j < AR; ++j) {
        const int row = (wave * AR + j) * 8 + (lane >> 3);
        const int m = m0 + row;
        const int gc = slot ^ ((row >> 1) & 7);
        const int b = (int)cl.fd_pq.div((uint32_t)m), pq = m - b * PQ;
        const int p = (int)cl.fd_q.div((uint32_t)pq), q = pq - p * cl.Q;
        const int h = p * a.sAh, w = q * a.sAw;
        // dh_i = dh_0 + sh*i with sh = +-1 (fwd: r - pad; dgrad class: (ph+pad-r)/st), so
        // the valid grid rows are one contiguous bit range [lo, hi]; same for columns
        const unsigned vr = span_mask(h, cl.dh0, cl.sh, cl.Rc, a.Hi);
        const unsigned vs = span_mask(w, cl.dw0, cl.sw, cl.Sc, a.Wi);
        const bool in = m < M;
        a_vr[j] = in ? vr : 0u;
        a_vs[j] = vs;
        a_ptr[j] = gin + (in ? ((size_t)((b * a.Hi + h) * a.Wi + w) << a.logC) : 0) + gc * 8;
    }
    const uint16_t* b_ptr[BR];
    bool b_ok[BR];
#pragma unroll
    for (int j = 0; j < BR; ++j) {
        const int row = (wave * BR + j) * 8 + (lane >> 3);
        const int n = n0 + row;
        const int gc = slot ^ ((row >> 1) & 7);
        b_ok[j] = n < a.Nout;
        b_ptr[j] = gwt + (size_t)(b_ok[j] ? n : 0) * a.T * a.C + gc * 8;
    }
    // per-lane fragment byte offsets inside a stage: row*128 + swizzled 16-B chunk
    const int fr = lane & 31, fh = lane >> 5;
    int a_rd[MT][4], b_rd[NT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int row = wm * (BM / 2) + i * 32 + fr;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a_rd[i][ks] = row * 128 + (swz(row, ks * 2 + fh) << 4);
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int row = wn * (BN / 2) + j * 32 + fr;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) b_rd[j][ks] = NST * SA + row * 128 + (swz(row, ks * 2 + fh) << 4);
    }

    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    auto issue = [&](int kt, int buf) {
        const int k = (kt0 + kt) * BK;
        const int tap = __builtin_amdgcn_readfirstlane(k >> a.logC);
        const int ti = (tap * cl.smag) >> 8, tj = tap - ti * cl.Sc;
        const int dh = (int)((pk_dh >> (4 * ti)) & 15u) - 8, dw = (int)((pk_dw >> (4 * tj)) & 15u) - 8;
        const int tw = (int)((pk_r >> (4 * ti)) & 15u) * a.Sw + (int)((pk_s >> (4 * tj)) & 15u);
        const int c0 = k & (a.C - 1);
        const long aoff = (long)(((dh * a.Wi + dw) << a.logC) + c0);
        const long boff = (long)(tw * a.C + c0);
#pragma unroll
        for (int j = 0; j < AR; ++j) {
            const bool ok = ((a_vr[j] >> ti) & (a_vs[j] >> tj)) & 1u;
            const void* src = ok ? (const void*)(a_ptr[j] + aoff) : (const void*)g_zero16;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + buf * SA + (wave * AR + j) * 1024), 16, 0,
                                             0);
        }
#pragma unroll
        for (int j = 0; j < BR; ++j) {
            const void* src = b_ok[j] ? (const void*)(b_ptr[j] + boff) : (const void*)g_zero16;
            __builtin_amdgcn_global_load_lds((gptr_t)src,
                                             (lptr_t)(lds + NST * SA + buf * SB + (wave * BR + j) * 1024), 16, 0, 0);
        }
    };

    floatx16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // fragments of k-step ks+1 are read while k-step ks's MFMAs run
    auto compute_pf = [&](int buf) {
        bf16x8 af[2][MT], bfr[2][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) af[0][i] = *reinterpret_cast<const bf16x8*>(lds + buf * SA + a_rd[i][0]);
#pragma unroll
        for (int j = 0; j < NT; ++j) bfr[0][j] = *reinterpret_cast<const bf16x8*>(lds + buf * SB + b_rd[j][0]);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int c = ks & 1;
            if (ks < 3) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    af[c ^ 1][i] = *reinterpret_cast<const bf16x8*>(lds + buf * SA + a_rd[i][ks + 1]);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    bfr[c ^ 1][j] = *reinterpret_cast<const bf16x8*>(lds + buf * SB + b_rd[j][ks + 1]);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[c][j], af[c][i], acc[i][j], 0, 0, 0);
        }
        // emitted order: k-step ks + 1's reads BEFORE k-step ks's MFMAs, so they stay in
        // flight under the matrix pipe.  (Threading them between the MFMAs, one read per
        // MFMA, issued each k-step's last read after its MFMAs into a register an MFMA had
        // just released, and the lgkmcnt(0) the compiler put before the next MFMAs then
        // exposed that read's whole LDS latency once per k-step.)
        constexpr int NR = MT + NT, NM = MT * NT;
        __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
    };
    // s_waitcnt immediate (gfx9 encoding: vmcnt[3:0] + [15:14], expcnt[6:4], lgkmcnt[11:8])
    constexpr int kWaitAll = (7 << 4) | (15 << 8);  // vmcnt(0)
    issue(0, 0);
    int s = 0;  // stage of tile kt
    for (int kt = 0; kt < nk; ++kt) {
        __builtin_amdgcn_s_waitcnt(kWaitAll);
        __builtin_amdgcn_s_barrier();
        if (kt + 1 < nk) issue(kt + 1, s ^ 1);
        compute_pf(s);
        s ^= 1;
    }

    if (a.splits > 1) {
        constexpr int NQ = MT * NT * 4;  // float4 groups of accumulators per lane
        const auto rs = rsrc_of(a.ws + (size_t)tid * NQ * 256 * 4);
        if (split > 0) {  // wait for the previous split's running sum, then add it
            __shared__ int late;
            if (t == 0) {  // bounded: a broken hand-off never hangs, it faults loudly
                unsigned n = 0;
                bool ok = true;
                while (__hip_atomic_load(a.flags + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) !=
                       (unsigned)split) {
                    if (++n >= a.spin_limit) {
                        ok = false;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                if (!ok) atomicOr(&g_conv_fault, GM_FAULT_SPLITK_SPIN);
                late = ok ? 0 : 1;
            }
            __syncthreads();
            if (late) {  // poison: the running sum was not handed over (the fault word is set)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[i][j][r] = __builtin_nanf("");
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 v = ld_sc1_f32x4(rs, (unsigned)((((i * NT + j) * 4 + g) * 256 + t) * 16));
                        acc[i][j][4 * g] += v.x;
                        acc[i][j][4 * g + 1] += v.y;
                        acc[i][j][4 * g + 2] += v.z;
                        acc[i][j][4 * g + 3] += v.w;
                    }
        }
        if (split < a.splits - 1) {  // publish the running sum to the next split
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        st_sc1_f32x4(rs, (unsigned)((((i * NT + j) * 4 + g) * 256 + t) * 16),
                                     make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2],
                                                 acc[i][j][4 * g + 3]));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (t == 0) __hip_atomic_store(a.flags + tid, (unsigned)(split + 1), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (t == 0) __hip_atomic_store(a.flags + tid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    store_tile_lds<MT, NT, BM, BN, EPI>(a, cl, m0, n0, wm, wn, fr, fh, M, acc, g * a.gs_out, lds, NST * (SA + SB), t,
                                        g);
}

template <int BM, int BN, int PIPE = 2>
__global__ __launch_bounds__(256) void k_conv_igemm_ut(ConvArgs a) {
    static_assert(PIPE == 2, "k_conv_igemm_ut: one main-loop form");
    conv_igemm_ut_body<BM, BN, 0>(a);
}

template <int BM, int BN>
__global__ __launch_bounds__(256) void k_conv_igemm_ut_affine(ConvArgs a) {
    conv_igemm_ut_body<BM, BN, 1>(a);
}

}  // namespace gm
