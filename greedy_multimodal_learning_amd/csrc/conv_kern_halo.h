// conv_igemm.hip: the halo-staged 3x3 / stride-1 kernels (k_conv_halo, k_conv_h9).
#pragma once
#include "conv_args.h"

namespace gm {

// ---------------------------------------------------------------------------------
// 3x3 / stride-1 / pad-1 convolutions (the ResNet trunk's 13 main convolutions per view
// and their stride-1 input gradients) with the A operand staged ONCE per 64-channel
// chunk as a halo instead of once per tap (implicit-GEMM im2col re-stages every input
// pixel 9 times).  The lean kernel (conv_kern_igemm.h) is bound by the per-CU LDS-DMA rate
// (~26 B/clk/CU measured: tools/conv_ab.py diagnostics), so bytes staged per FLOP is
// the lever: per 64-deep k-tile the A stage shrinks from 16 KB to (halo / 9) ~3-6 KB.
//
// Geometry.  An M tile is 128 consecutive output pixels (b, p, q) of the flat
// N*H*W order (it may span rows and images).  Input rows live in a "padded row" space:
// image b's row h is padded row b*(H+1) + 1 + h, and padded rows b*(H+1) are zero rows
// (one between consecutive images, one after the last), columns are padded by one zero
// column each side.  Output (b, p, q) with tap offset (dh, dw) in [-1, 1]^2 reads halo
// pixel ((b*(H+1) + 1 + p + dh) - pr0) * (W+2) + (1 + q + dw), pr0 the tile's first
// padded row - so every tap reads in-range LDS and padding is real zeros (DMA'd from a
// zero vector), with no per-lane predicates.  Halo pixels are 128-B LDS rows (64
// channels) with the 16-B chunk XOR-swizzled by ((pixel >> 1) & 7), applied on the DMA
// source as everywhere in this file.
//
// Schedule: k-tiles run chunk-major, tap-minor (k = chunk * 9 + tap); the halo of a
// chunk is loaded at the chunk's first k-tile (one buffer; the other co-resident
// workgroup of the CU hides that stall), the B operand (weights) through the usual
// 2-stage ring with one barrier per k-tile.  Epilogue and split-K turnstile as in the
// lean kernel.
struct HaloArgs {
    int halo_bytes;           // LDS bytes of the halo region (multiple of 1 KB)
    FastDiv fd_w2, fd_h1;     // W + 2, H + 1
};

// BM = 256 (one workgroup per CU): the weight bytes staged per FLOP - the binding
// LDS-DMA traffic of the BM = 128 form - halve; the halo is double-buffered and the
// next chunk's halo is DMA'd in pieces under the current chunk's first eight k-tiles
// (the BM = 128 form relies on its co-resident second workgroup to hide that load).
template <int BM, int BN, int NB>
__global__ __launch_bounds__(BM == 256 ? 512 : 256) void k_conv_halo(ConvArgs a, HaloArgs h) {
    constexpr int BK = 64;  // NB: stages of the weight (B) ring, 2 or 3
    constexpr bool kHB2 = BM == 256;  // double-buffered halo, prefetched in pieces
    constexpr int NW = BM == 256 ? 8 : 4;  // waves: (NW/2) x 2, each a 64x64 sub-tile
    constexpr int NT_ = NW * 64;           // threads
    constexpr int BR = BN / (8 * NW);      // B-stage DMA instructions per wave
    constexpr int MT = 2, NT = BN / 64;
    constexpr int SB = BN * 128;
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    char* lds = reinterpret_cast<char*>(smem);  // [halo (x2 when kHB2)][B0][B1]([B2])
    const int HB = h.halo_bytes;
    const int BOFF = kHB2 ? 2 * HB : HB;  // start of the B ring

    int bid = blockIdx.x;
    int split = 0;
    if (a.splits > 1) {
        split = bid / a.tiles_total;
        bid -= split * a.tiles_total;
    }
    const ConvCls& cl = a.cls[0];
    // tn fastest: blocks are dealt round-robin over the 8 XCDs (b on XCD b % 8), so with a
    // power-of-two column count each XCD's blocks share one weight slice (L2-resident)
    const int tiles_n = (a.Nout + BN - 1) / BN;
    const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int H = a.Hi, W = a.Wi, W2 = W + 2, H1 = H + 1;
    const int PQ = cl.P * cl.Q;  // == H * W (stride 1, same size)
    const int M = a.N * PQ;
    const int nk_all = 9 * (a.C >> 6);
    const int kt0 = split * nk_all / a.splits;
    const int nk = (split + 1) * nk_all / a.splits - kt0;

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int slot = lane & 7;
    const unsigned pk_dh = cl.pk_dh, pk_dw = cl.pk_dw, pk_r = cl.pk_r, pk_s = cl.pk_s;

    // tile's padded row range
    int pr0, npix;
    {
        const int b0 = (int)cl.fd_pq.div((uint32_t)m0), q0 = m0 - b0 * PQ;
        const int p0 = (int)cl.fd_q.div((uint32_t)q0);
        const int m1 = min(m0 + BM, M) - 1;
        const int b1 = (int)cl.fd_pq.div((uint32_t)m1), q1 = m1 - b1 * PQ;
        const int p1 = (int)cl.fd_q.div((uint32_t)q1);
        pr0 = b0 * H1 + p0;
        npix = (b1 * H1 + p1 + 2 - pr0 + 1) * W2;
    }
    pr0 = __builtin_amdgcn_readfirstlane(pr0);
    npix = __builtin_amdgcn_readfirstlane(npix);
    const int nI = (npix + 7) >> 3;  // halo DMA instructions of the workgroup

    // A fragments: per MFMA row block i the lane's output pixel's halo index (tap 0,0)
    const int fr = lane & 31, fh = lane >> 5;
    int hbase[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int m = m0 + wm * (MT * 32) + i * 32 + fr;
        m = m < M ? m : m0;  // rows past M read a valid pixel; their outputs are not stored
        const int b = (int)cl.fd_pq.div((uint32_t)m), pq = m - b * PQ;
        const int p = (int)cl.fd_q.div((uint32_t)pq), q = pq - p * cl.Q;
        hbase[i] = (b * H1 + 1 + p - pr0) * W2 + 1 + q;
    }
    // B rows (weights [Nout][9][C])
    const uint16_t* b_ptr[BR];
    bool b_ok[BR];
#pragma unroll
    for (int j = 0; j < BR; ++j) {
        const int row = (wave * BR + j) * 8 + (lane >> 3);
        const int n = n0 + row;
        const int gc = slot ^ ((row >> 1) & 7);
        b_ok[j] = n < a.Nout;
        b_ptr[j] = a.wt + (size_t)(b_ok[j] ? n : 0) * a.T * a.C + gc * 8;
    }
    int b_rd[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int row = wn * (BN / 2) + j * 32 + fr;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) b_rd[j][ks] = BOFF + row * 128 + (swz(row, ks * 2 + fh) << 4);
    }

    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    // the halo of channel chunk cc: instructions I = wave, wave+4, ... of nI, 8 pixels each
    // (instructions [I0, I1) only, into halo buffer hb)
    auto issue_halo_part = [&](int cc, int hb, int I0, int I1) {
        const int cbase = cc << 6;
        char* dst = lds + hb * HB;
        for (int I = I0 + wave; I < I1; I += NW) {
            const int hp = I * 8 + (lane >> 3);
            const void* src = (const void*)g_zero16;
            if (hp < npix) {
                const int r = (int)h.fd_w2.div((uint32_t)hp), c = hp - r * W2;
                const int pr = pr0 + r;
                const int b = (int)h.fd_h1.div((uint32_t)pr), rr = pr - b * H1;
                if (rr != 0 && c != 0 && c != W + 1 && b < a.N) {
                    const int gc = slot ^ ((hp >> 1) & 7);
                    src = (const void*)(a.in + ((size_t)((b * H + rr - 1) * W + c - 1) << a.logC) + cbase + gc * 8);
                }
            }
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(dst + I * 1024), 16, 0, 0);
        }
    };
    auto issue_halo = [&](int cc) { issue_halo_part(cc, kHB2 ? (cc & 1) : 0, 0, nI); };
    // the kHB2 prefetch: piece tp (0..7) of the next chunk's halo, NW instructions a
    // multiple so every wave issues whole rounds
    const int nIp = (nI + 8 * NW - 1) / (8 * NW) * NW;  // instructions per piece
    auto issue_b = [&](int kt, int buf) {
        const int k = kt0 + kt;
        const int cc = k / 9, tp = k - cc * 9;
        const int ti = tp / 3, tj = tp - ti * 3;
        const int tw = (int)((pk_r >> (4 * ti)) & 15u) * a.Sw + (int)((pk_s >> (4 * tj)) & 15u);
        const long boff = (long)(tw * a.C + (cc << 6));
#pragma unroll
        for (int j = 0; j < BR; ++j) {
            const void* src = b_ok[j] ? (const void*)(b_ptr[j] + boff) : (const void*)g_zero16;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + BOFF + buf * SB + (wave * BR + j) * 1024), 16,
                                             0, 0);
        }
    };

    floatx16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int buf, int toff, int hoff) {
        int abase[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int hp = hbase[i] + toff;
            abase[i] = hoff + ((hp << 7) | ((((hp >> 1) & 7) ^ fh) << 4));  // chunk (2ks+fh)^swz = this ^ (ks<<5)
        }
        bf16x8 af[2][MT], bfr[2][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) af[0][i] = *reinterpret_cast<const bf16x8*>(lds + abase[i]);
#pragma unroll
        for (int j = 0; j < NT; ++j) bfr[0][j] = *reinterpret_cast<const bf16x8*>(lds + buf * SB + b_rd[j][0]);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int c = ks & 1;
            if (ks < 3) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    af[c ^ 1][i] = *reinterpret_cast<const bf16x8*>(lds + (abase[i] ^ ((ks + 1) << 5)));
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
        constexpr int NR = MT + NT, NM = MT * NT;  // next k-step's reads before these MFMAs
        __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
    };

    constexpr int kWaitAll = (7 << 4) | (15 << 8);  // s_waitcnt vmcnt(0)
    issue_halo(kt0 / 9);
    issue_b(0, 0);
    if (NB == 3 && nk > 1) issue_b(1, 1);
    constexpr int kWaitB = (BR & 15) | (7 << 4) | (15 << 8);  // vmcnt(BR): the newest B stage stays in flight
    int sb = 0;  // B stage of k-tile kt
    for (int kt = 0; kt < nk; ++kt) {
        const int k = kt0 + kt;
        const int tp = k % 9;
        if (NB == 3 && kt + 1 < nk) __builtin_amdgcn_s_waitcnt(kWaitB);
        else __builtin_amdgcn_s_waitcnt(kWaitAll);
        __builtin_amdgcn_s_barrier();
        if (!kHB2 && kt > 0 && tp == 0) {  // next channel chunk: every wave is done with the old halo
            issue_halo(k / 9);
            __builtin_amdgcn_s_waitcnt(kWaitAll);
            __builtin_amdgcn_s_barrier();
        }
        // kHB2: the next chunk's halo goes to the other buffer (last read by the previous
        // chunk, whose k-tiles every wave has passed at this barrier), issued before this
        // k-tile's B stage so the counted B waits stay valid, landed by the chunk's first wait
        if (kHB2 && kt - tp + 9 < nk) {
            // pieces [lo, hi): a split that starts mid-chunk issues the pieces it skipped
            const int lo = kt == 0 ? 0 : tp, hi = tp < 8 ? tp + 1 : 8;
            const int cn = k / 9 + 1;
            if (lo < hi) issue_halo_part(cn, cn & 1, lo * nIp, min(hi * nIp, nI));
        }
        if (kt + NB - 1 < nk) {
            int sn = sb + NB - 1;
            if (sn >= NB) sn -= NB;
            issue_b(kt + NB - 1, sn);
        }
        const int ti = tp / 3, tj = tp - ti * 3;
        const int dh = (int)((pk_dh >> (4 * ti)) & 15u) - 8, dw = (int)((pk_dw >> (4 * tj)) & 15u) - 8;
        compute(sb, dh * W2 + dw, kHB2 ? ((k / 9) & 1) * HB : 0);
        if (++sb == NB) sb = 0;
    }

    if (a.splits > 1) {
        constexpr int NQ = MT * NT * 4;  // float4 groups of accumulators per lane
        const auto rs = rsrc_of(a.ws + (size_t)bid * NQ * NT_ * 4);
        if (split > 0) {  // wait for the previous split's running sum, then add it
            __shared__ int late;
            if (t == 0) {  // bounded: a broken hand-off never hangs, it faults loudly
                unsigned n = 0;
                bool ok = true;
                while (__hip_atomic_load(a.flags + bid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) !=
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
                        const float4 v = ld_sc1_f32x4(rs, (unsigned)((((i * NT + j) * 4 + g) * NT_ + t) * 16));
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
                        st_sc1_f32x4(rs, (unsigned)((((i * NT + j) * 4 + g) * NT_ + t) * 16),
                                     make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2],
                                                 acc[i][j][4 * g + 3]));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (t == 0) __hip_atomic_store(a.flags + bid, (unsigned)(split + 1), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (t == 0) __hip_atomic_store(a.flags + bid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    // (BM = 256: two 128-row halves of wave rows 0-1 and 2-3)
    store_tile<MT, NT, 128, BN>(a, cl, m0 + (wm >> 1) * 128, n0, wm & 1, wn, fr, fh, M, acc);
}

// ---------------------------------------------------------------------------------
// k_conv_h9: the halo-staged 3x3 / stride-1 convolution (forward and stride-1 input
// gradient, C a multiple of 64) with its nine taps UNROLLED.  k_conv_halo decodes the
// tap of every k-tile at run time (k / 9, tap / 3, packed-field shifts, the ring stage
// modulo, per-DMA pointer selects): ~45 scalar and ~40 vector instructions per 16 MFMAs
// per wave, which at two waves per SIMD issue-bind the loop (ISA census, round 3).  Here
// the k-loop runs over 64-channel chunks with the nine taps as compile-time steps, so
//   * the weight-ring stage of a tap is tap % 3 (nine is a multiple of the ring depth):
//     the B fragment addresses are precomputed lane offsets + an immediate;
//   * each tap's halo offset and weight tap index are decoded ONCE per workgroup (the A
//     fragment address of tap t / fragment i is a precomputed VGPR);
//   * the halo pixel decode (two fast divides per DMA instruction) is done once per tile,
//     not once per channel chunk; chunks only add their channel base;
//   * weights are DMA'd without per-lane bounds selects (Nout % BN == 0 is required).
// Split-K splits whole channel chunks (splits <= C / 64) and hands the fp32 running sum
// on through the same turnstile as k_conv_halo.  One workgroup = 128 output pixels x BN
// channels, 4 waves of 64x64 (v_mfma_f32_32x32x16_bf16), two workgroups per CU.
constexpr int kH9MaxQ = 12;  // halo DMA instructions per wave (nI <= 48)

// NB: weight-ring stages (NB - 2 stay in flight across a k-tile).  Weights and halo both by
// LDS-DMA.  Measured and dropped (r03-r04): register-staged weights, a register prefetch of
// the next chunk's halo, weight pieces spread between the k-slices' MFMAs (0.05-0.07 ms/step
// slower or neutral).
// (The kernel's text is conv_h9_body, inlined into k_conv_h9 - EPI = 0, the symbol and the code
// of the training step - and into k_conv_h9_affine, EPI = 1: store_tile_lds's evaluation epilogue.)
template <int BN, int NB, int EPI>
__device__ __forceinline__ void conv_h9_body(const ConvArgs& a, const HaloArgs& h) {
    constexpr int BM = 128, MT = 2, NT = BN / 64, NW = 4;
    static_assert(NB >= 2 && NB <= 8, "ring depth");
    constexpr int BR = BN / (8 * NW);  // weight DMA instructions per wave per k-tile
    constexpr int SB = BN * 128;       // bytes of one ring stage
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    char* lds = reinterpret_cast<char*>(smem);  // [halo][B0]..[B(NB-1)]
    const int HB = h.halo_bytes;

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
    const ConvCls& cl = a.cls[0];
    const int tiles_n = a.Nout / BN;
    const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int H = a.Hi, W = a.Wi, W2 = W + 2, H1 = H + 1;
    const int PQ = cl.P * cl.Q;
    const int M = a.N * PQ;
    const int nch = a.C >> 6;
    const int c0 = split * nch / a.splits, c1 = (split + 1) * nch / a.splits;

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int slot = lane & 7;
    const int fr = lane & 31, fh = lane >> 5;

    // the tile's padded halo rows
    int pr0, npix;
    {
        const int b0 = (int)cl.fd_pq.div((uint32_t)m0), q0 = m0 - b0 * PQ;
        const int p0 = (int)cl.fd_q.div((uint32_t)q0);
        const int m1 = min(m0 + BM, M) - 1;
        const int b1 = (int)cl.fd_pq.div((uint32_t)m1), q1 = m1 - b1 * PQ;
        const int p1 = (int)cl.fd_q.div((uint32_t)q1);
        pr0 = b0 * H1 + p0;
        npix = (b1 * H1 + p1 + 2 - pr0 + 1) * W2;
    }
    pr0 = __builtin_amdgcn_readfirstlane(pr0);
    npix = __builtin_amdgcn_readfirstlane(npix);
    const int nI = (npix + 7) >> 3;
    const int nq = (nI - wave + NW - 1) / NW;  // this wave's halo instructions

    // per-tap halo offset and weight tap (uniform), decoded once
    int toff[9], twc[9];
#pragma unroll
    for (int tp = 0; tp < 9; ++tp) {
        const int ti = tp / 3, tj = tp % 3;
        const int dh = (int)((cl.pk_dh >> (4 * ti)) & 15u) - 8, dw = (int)((cl.pk_dw >> (4 * tj)) & 15u) - 8;
        toff[tp] = __builtin_amdgcn_readfirstlane(dh * W2 + dw);
        const int tw = (int)((cl.pk_r >> (4 * ti)) & 15u) * a.Sw + (int)((cl.pk_s >> (4 * tj)) & 15u);
        twc[tp] = __builtin_amdgcn_readfirstlane(tw * a.C);
    }
    // A fragment addresses (ks = 0) per tap and row block: chunk (2ks+fh) ^ swz(pixel)
    int aad[9][MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int m = m0 + wm * (MT * 32) + i * 32 + fr;
        m = m < M ? m : m0;  // rows past M read a valid pixel; their outputs are not stored
        const int b = (int)cl.fd_pq.div((uint32_t)m), pq = m - b * PQ;
        const int p = (int)cl.fd_q.div((uint32_t)pq), q = pq - p * cl.Q;
        const int hb = (b * H1 + 1 + p - pr0) * W2 + 1 + q;
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
            const int hp = hb + toff[tp];
            aad[tp][i] = (hp << 7) | ((((hp >> 1) & 7) ^ fh) << 4);
        }
    }
    // B: weight rows of this wave's DMA instructions ([Nout][9][C]), source-swizzled
    const uint16_t* b_src[BR];
#pragma unroll
    for (int j = 0; j < BR; ++j) {
        const int row = (wave * BR + j) * 8 + (lane >> 3);
        b_src[j] = gwt + (size_t)(n0 + row) * a.T * a.C + ((slot ^ ((row >> 1) & 7)) << 3);
    }
    int b_rd[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int row = wn * (BN / 2) + j * 32 + fr;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) b_rd[j][ks] = HB + row * 128 + (swz(row, ks * 2 + fh) << 4);
    }
    // halo sources of this wave's DMA instructions: channel-0 element offset or -1 (zero)
    int hsrc[kH9MaxQ];
#pragma unroll
    for (int q = 0; q < kH9MaxQ; ++q) {
        hsrc[q] = -1;
        const int hp = (wave + NW * q) * 8 + (lane >> 3);
        if (q < nq && hp < npix) {
            const int r = (int)h.fd_w2.div((uint32_t)hp), c = hp - r * W2;
            const int pr = pr0 + r;
            const int b = (int)h.fd_h1.div((uint32_t)pr), rr = pr - b * H1;
            if (rr != 0 && c != 0 && c != W + 1 && b < a.N)
                hsrc[q] = (((b * H + rr - 1) * W + c - 1) << a.logC) + ((slot ^ ((hp >> 1) & 7)) << 3);
        }
    }

    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    auto issue_halo = [&](int cc) {
        const int cbase = cc << 6;
#pragma unroll
        for (int q = 0; q < kH9MaxQ; ++q) {
            if (q < nq) {
                const void* src = hsrc[q] >= 0 ? (const void*)(gin + hsrc[q] + cbase) : (const void*)g_zero16;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + (wave + NW * q) * 1024), 16, 0, 0);
            }
        }
    };
    // k-tile (chunk cc, tap tp) -> ring stage st
    auto issue_b = [&](int cc, int tp, int st) {
        const int off = twc[tp] + (cc << 6);
#pragma unroll
        for (int j = 0; j < BR; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(b_src[j] + off),
                                             (lptr_t)(lds + HB + st * SB + (wave * BR + j) * 1024), 16, 0, 0);
    };

    floatx16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int tp, int st) {
        bf16x8 af[2][MT], bfr[2][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) af[0][i] = *reinterpret_cast<const bf16x8*>(lds + aad[tp][i]);
#pragma unroll
        for (int j = 0; j < NT; ++j) bfr[0][j] = *reinterpret_cast<const bf16x8*>(lds + st * SB + b_rd[j][0]);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int c = ks & 1;
            if (ks < 3) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    af[c ^ 1][i] = *reinterpret_cast<const bf16x8*>(lds + (aad[tp][i] ^ ((ks + 1) << 5)));
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    bfr[c ^ 1][j] = *reinterpret_cast<const bf16x8*>(lds + st * SB + b_rd[j][ks + 1]);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[c][j], af[c][i], acc[i][j], 0, 0, 0);
        }
        constexpr int NR = MT + NT, NM = MT * NT;
        // slice ks + 1's fragment reads are issued BEFORE slice ks's MFMAs (the compiler's
        // counted lgkmcnt then waits for slice ks's reads only, slice ks + 1's stay in
        // flight under the MFMAs).  The read/MFMA interleave this replaces issued each
        // slice's last read after its MFMAs, into a register an MFMA had just released,
        // and waited lgkmcnt(0) on it: one exposed LDS round trip per k-slice.
        __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
    };

    // vmcnt(n): all but the wave's n newest vector-memory operations done
    auto wait_vm = [](int n) {
        switch (n) {
        case 0: __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8)); break;
        case 1: __builtin_amdgcn_s_waitcnt(1 | (7 << 4) | (15 << 8)); break;
        case 2: __builtin_amdgcn_s_waitcnt(2 | (7 << 4) | (15 << 8)); break;
        case 3: __builtin_amdgcn_s_waitcnt(3 | (7 << 4) | (15 << 8)); break;
        case 4: __builtin_amdgcn_s_waitcnt(4 | (7 << 4) | (15 << 8)); break;
        case 5: __builtin_amdgcn_s_waitcnt(5 | (7 << 4) | (15 << 8)); break;
        case 6: __builtin_amdgcn_s_waitcnt(6 | (7 << 4) | (15 << 8)); break;
        case 7: __builtin_amdgcn_s_waitcnt(7 | (7 << 4) | (15 << 8)); break;
        case 8: __builtin_amdgcn_s_waitcnt(8 | (7 << 4) | (15 << 8)); break;
        case 9: __builtin_amdgcn_s_waitcnt(9 | (7 << 4) | (15 << 8)); break;
        case 10: __builtin_amdgcn_s_waitcnt(10 | (7 << 4) | (15 << 8)); break;
        case 11: __builtin_amdgcn_s_waitcnt(11 | (7 << 4) | (15 << 8)); break;
        default: __builtin_amdgcn_s_waitcnt(12 | (7 << 4) | (15 << 8)); break;
        }
    };
    static_assert((NB - 2) * BR <= 12, "counted wait range");
    const int nkt = (c1 - c0) * 9;
    issue_halo(c0);
#pragma unroll
    for (int k = 0; k < NB - 1; ++k)
        if (k < nkt) issue_b(c0 + k / 9, k % 9, k);
    int sb = 0;  // ring slot of k-tile kt
    int kt = 0;
    for (int cc = c0; cc < c1; ++cc) {
#pragma unroll
        for (int tp = 0; tp < 9; ++tp, ++kt) {
            // stages issued after k-tile kt: min(NB - 2, nkt - 1 - kt), left in flight
            const int ahead = min(NB - 2, nkt - 1 - kt);
            wait_vm(ahead * BR);
            __builtin_amdgcn_s_barrier();
            if (tp == 0 && cc > c0) {  // every wave is done with the previous chunk's halo
                issue_halo(cc);
                wait_vm(0);
                __builtin_amdgcn_s_barrier();
            }
            int sn = sb + NB - 1;
            if (sn >= NB) sn -= NB;
            if (kt + NB - 1 < nkt) {
                if (tp + NB - 1 < 9) issue_b(cc, tp + NB - 1, sn);
                else issue_b(cc + 1, tp + NB - 1 - 9, sn);
            }
            compute(tp, sb);
            if (++sb == NB) sb = 0;
        }
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
            if (late) {
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
    store_tile_lds<MT, NT, 128, BN, EPI>(a, cl, m0, n0, wm, wn, fr, fh, M, acc, g * a.gs_out, lds, HB + NB * SB, t, g);
}

template <int BN, int NB>
__global__ __launch_bounds__(256, 2) void k_conv_h9(ConvArgs a, HaloArgs h) {
    conv_h9_body<BN, NB, 0>(a, h);
}

template <int BN, int NB>
__global__ __launch_bounds__(256, 2) void k_conv_h9_affine(ConvArgs a, HaloArgs h) {
    conv_h9_body<BN, NB, 1>(a, h);
}

}  // namespace gm
