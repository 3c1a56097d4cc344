// k_wgrad_ring: the weight gradient of 3x3 convolutions with K % 128 == 0 and C a power of two >= 32.
#pragma once
#include "conv_kern_wfrag.h"

namespace gm {

// k_wgrad_ring: weight gradient of a 3 x 3 convolution (any stride / padding) with K % 128 == 0
// and C % 32 == 0 - the layer-2..4 shapes k_conv_wgrad4 served at 0.15-0.23 of the MFMA peak.
// What bound k_conv_wgrad4: one 64-pixel step of LDS-DMA in flight per workgroup (issue ->
// landed is ~1 us under load, MI355X_MICROARCH.md ldsdma rows) against 16 MFMAs per wave
// (~0.25 us), so its two workgroups per CU took in ~35 GB/s; and every DMA issue sat in the
// compute waves' MFMA stream.  Here, per CU ONE workgroup of 512 threads:
//   * four LOADER waves own all LDS-DMA: a 3-slot ring of 64-pixel steps, 2 steps in flight
//     (156 KB), one raw s_barrier per step after a counted vmcnt (the step about to be read has
//     landed; the younger one stays in flight across the barrier);
//   * four COMPUTE waves never touch VMEM in the loop.  The workgroup tile is 128 output channels
//     x 288 (tap, channel) columns = a 4 x 9 grid of 32 x 32 blocks (k-block kb, column block cb);
//     compute wave w = kh + 2 ch owns k-blocks {2 kh, 2 kh + 1} x column blocks 5 ch .. 5 ch + 3
//     plus the single cell (2 kh + ch, 4) of the middle column: 9 accumulators and 9 MFMAs per
//     16-pixel k-slice, fed by 2 A + 5 B fragments (14 ds_read_b64_tr_b16) read one k-slice
//     ahead.  (r05's layout - wave w owning k-block w x all 9 column blocks - read 1 A + 9 B
//     fragments per wave, every B fragment by all four waves: 80 instead of 56 transposed reads
//     per k-slice and CU, 2.22 instead of 1.56 LDS instructions per MFMA (PMC), 2.5 % slower.)
//   * every 3x3 shape with C % 32 == 0 splits into whole tiles; 88.6 FLOP per staged byte.
// LDS slot: B (x gathered per tap) as 9 blocks of [64 px][32 columns] (64-B rows: the tr reads of a
// half-wave cover 4 rows x 64 B = all 64 banks, no swizzle), then A (dy) as 2 blocks of
// [64 px][64 k] (128-B rows, chunk XOR 4 ((row >> 1) & 1): k_conv_wgrad4's image).  Splits over the
// pixel steps write fp32 partial slabs that k_wgrad_sum reduces in a fixed order (deterministic);
// one split writes (or accumulates into) the gradient directly.
// What bounds it now (r06 A/B): the LDS-DMA feed - 52 KB staged per 64-pixel step, ~38 GB/s per CU
// at half the CUs - not the LDS reads (30 % fewer of them bought 2.5 %).
struct WRingArgs {
    const uint16_t* dy;  // [G][M][K]  (M = N*P*Q)
    const uint16_t* x;   // [G][N][H][W][C]
    float* part;         // [G][splits][K][9C], or dw (one split)
    int N, H, W, C, logC, K, P, Q, sth, stw, padh, padw, M;
    int tiles_k, tiles_n, splits, sps;  // sps: 64-pixel steps per split
    FastDiv fd_pq, fd_q;
    int adv_b, adv_p, adv_q;            // one step of 64 pixels in (b, p, q)
    long long gs_dy, gs_x, gs_part;     // group strides (elements)
    int accumulate;
};

namespace ring {
constexpr int S = 3, BK = 64;                      // ring slots, pixels per step
constexpr int BB = BK * 64, AB = BK * 128;         // bytes per B / A block
constexpr int B = 9 * BB, A = 2 * AB, SLOT = B + A;
constexpr int SLICES = BK / 16;                    // 16-pixel k-slices per step
constexpr size_t LDS = (size_t)S * SLOT;
}  // namespace ring

// one 32 x 16 fragment by two transposed reads at base + LO / + HI
template <int LO, int HI>
__device__ __forceinline__ bf16x8 ring_frag(unsigned base) {
    const short4_t lo = tr_rd<LO>(base), hi = tr_rd<HI>(base);
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// the compute waves (see above): wave w = kh + 2 CH
template <int CH>
__device__ __forceinline__ void ring_compute(const WRingArgs& a, int w, int lane, unsigned lds0, int nst, int grp,
                                             int split, int k0, int n0) {
    using namespace ring;
    const int kh = w & 1;
    floatx16 acc[9];  // [4 i + jj]: k-block 2 kh + i x column block 5 CH + jj; [8]: (2 kh + CH, 4)
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    // tr-read geometry (k_conv_wgrad4's): half-wave g >> 1 reads rows 8 (g >> 1) + q4 (+4) of a
    // 16-row k-slice, 4-column block p4 of the 32-column fragment, 16-column half g & 1.  The A
    // image's chunk swizzle (XOR 4 on odd row pairs) flips the 64-column half's bit, so the two A
    // fragments of a lane sit at +-64 B of each other by row: two base registers.
    const int g = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
    const int rbase = 8 * (g >> 1) + q4;
    const int cin = 16 * (g & 1) + 4 * p4;
    unsigned a_l[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ac = 32 * i + cin;
        a_l[i] = B + kh * AB + rbase * 128 + ((((ac >> 3) ^ wswz<128>(rbase))) << 4) + (ac & 7) * 2;
    }
    const unsigned b_l = rbase * 64 + cin * 2 + 5 * CH * BB, b_4 = rbase * 64 + cin * 2 + 4 * BB;
    bf16x8 fa[2][2], fb[2][5];
    auto load_ks = [&](auto ksc, int c, unsigned sb) __attribute__((always_inline)) {
        constexpr int KS = decltype(ksc)::value;
        fa[c][0] = ring_frag<KS * 2048, KS * 2048 + 512>(sb + a_l[0]);
        fa[c][1] = ring_frag<KS * 2048, KS * 2048 + 512>(sb + a_l[1]);
        fb[c][0] = ring_frag<0 * BB + KS * 1024, 0 * BB + KS * 1024 + 256>(sb + b_l);
        fb[c][1] = ring_frag<1 * BB + KS * 1024, 1 * BB + KS * 1024 + 256>(sb + b_l);
        fb[c][2] = ring_frag<2 * BB + KS * 1024, 2 * BB + KS * 1024 + 256>(sb + b_l);
        fb[c][3] = ring_frag<3 * BB + KS * 1024, 3 * BB + KS * 1024 + 256>(sb + b_l);
        fb[c][4] = ring_frag<KS * 1024, KS * 1024 + 256>(sb + b_4);
    };
    auto load = [&](int ks, int c, unsigned sb) __attribute__((always_inline)) {
        switch (ks) {
            case 0: load_ks(std::integral_constant<int, 0>{}, c, sb); break;
            case 1: load_ks(std::integral_constant<int, 1>{}, c, sb); break;
            case 2: load_ks(std::integral_constant<int, 2>{}, c, sb); break;
            default: load_ks(std::integral_constant<int, 3>{}, c, sb); break;
        }
    };
    // lgkmcnt(0), then every fragment of buffer c re-defined after it (asm reads are invisible
    // to the compiler's own waits; the MFMAs must not be hoisted above the wait)
    auto wait_frags = [&](int c) __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        asm volatile("" : "+v"(fa[c][0]), "+v"(fa[c][1]));
#pragma unroll
        for (int j = 0; j < 5; ++j) asm volatile("" : "+v"(fb[c][j]));
        __builtin_amdgcn_sched_barrier(0);
    };
    int slot = 0;
    if (nst > 0) {
        __builtin_amdgcn_s_barrier();  // step 0 landed
        unsigned sb = lds0;
        load(0, 0, sb);
        for (int i = 0; i < nst; ++i) {
#pragma unroll
            for (int ks = 0; ks < SLICES; ++ks) {
                const int c = ks & 1;
                wait_frags(c);
                if (ks + 1 < SLICES) {
                    load(ks + 1, c ^ 1, sb);
                } else if (i + 1 < nst) {
                    // every read of this step is done: the barrier lets the loaders refill the
                    // previous step's slot and tells us step i + 1 has landed - read its first
                    // slice under this slice's MFMAs
                    __builtin_amdgcn_s_barrier();
                    slot = slot + 1 == S ? 0 : slot + 1;
                    sb = lds0 + (unsigned)slot * SLOT;
                    load(0, c ^ 1, sb);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
                        acc[4 * ii + jj] =
                            __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[c][ii], fb[c][jj], acc[4 * ii + jj], 0, 0, 0);
                acc[8] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[c][CH], fb[c][4], acc[8], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // D[k][col]: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5).  Direct dword stores
    // (an LDS-staged dwordx4 epilogue measured 3-4 us slower per launch: hipcc serialised its
    // stores on vmcnt(0)); the accumulate test is hoisted out of the loops (a per-element select
    // would branch and wait vmcnt(0) around every load)
    const int TC = 9 * a.C;
    float* base = a.part + grp * a.gs_part + (size_t)split * a.K * TC + (size_t)(k0 + 4 * (lane >> 5)) * TC + n0 +
                  (lane & 31);
    auto out_of = [&](int j) __attribute__((always_inline)) -> float* {
        const int kb = j < 8 ? 2 * kh + (j >> 2) : 2 * kh + CH;
        const int cb = j < 8 ? 5 * CH + (j & 3) : 4;
        return base + (size_t)(32 * kb) * TC + 32 * cb;
    };
    if (a.accumulate) {
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            float* out = out_of(j);
            float v[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = out[(size_t)((e & 3) + 8 * (e >> 2)) * TC];
#pragma unroll
            for (int e = 0; e < 16; ++e) out[(size_t)((e & 3) + 8 * (e >> 2)) * TC] = v[e] + acc[j][e];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            float* out = out_of(j);
#pragma unroll
            for (int e = 0; e < 16; ++e) out[(size_t)((e & 3) + 8 * (e >> 2)) * TC] = acc[j][e];
        }
    }
}

__global__ __launch_bounds__(512) void k_wgrad_ring(WRingArgs a) {
    using namespace ring;
    constexpr int D = S - 1;  // steps in flight
    extern __shared__ __attribute__((aligned(16))) uint4 wsm[];
    char* lds = reinterpret_cast<char*>(wsm);
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    int bid = blockIdx.x;
    {   // XCD-major: the tiles of one pixel range (split) share an XCD and its L2 copy of the rows
        const int n = gridDim.x, q = n >> 3, r = n & 7, x = bid & 7;
        bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
    }
    const int tiles = a.tiles_k * a.tiles_n;
    const int grp = bid / (tiles * a.splits);
    bid -= grp * tiles * a.splits;
    const int split = bid / tiles, tile = bid - split * tiles;
    const int tk = tile % a.tiles_k, tn = tile / a.tiles_k;
    const int k0 = tk * 128, n0 = tn * 288;
    const int step0 = split * a.sps;
    const int nst = max(0, min((a.M + BK - 1) / BK, step0 + a.sps) - step0);
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds;

    if (wave < 4) {
        if (wave >> 1) ring_compute<1>(a, wave, lane, lds0, nst, grp, split, k0, n0);
        else ring_compute<0>(a, wave, lane, lds0, nst, grp, split, k0, n0);
        return;
    }
    // ---- loader waves: wave 4 + lw stages B rows 16 lw .. + 15 of the 9 blocks and A rows
    // 16 lw .. + 15 of both blocks (9 + 4 pieces per step) ----
    const int lw = wave - 4;
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    const void* zero = (const void*)g_wzero16;
    const uint16_t* __restrict__ gdy = a.dy + grp * a.gs_dy;
    const uint16_t* __restrict__ gx = a.x + grp * a.gs_x;
    const int brow = 16 * lw + (lane >> 2), bc = (lane & 3) * 8;
    int bdh[9], bdw[9], boff[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int n = n0 + 32 * j + bc;
        const int tap = n >> a.logC, c = n & (a.C - 1);
        const int r = tap / 3, s = tap - 3 * r;
        bdh[j] = r - a.padh;
        bdw[j] = s - a.padw;
        boff[j] = ((bdh[j] * a.W + bdw[j]) << a.logC) + c;
    }
    // A sources advance by BK pixel rows per step (no per-step 64-bit multiply)
    int arow[2];
    const uint16_t* ap[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        arow[h] = 16 * lw + 8 * h + (lane >> 3);
#pragma unroll
        for (int ab = 0; ab < 2; ++ab)
            ap[h][ab] = gdy + (size_t)(step0 * BK + arow[h]) * a.K + k0 + 64 * ab +
                        (((lane & 7) ^ wswz<128>(arow[h])) << 3);
    }
    const size_t astep = (size_t)BK * a.K;
    const int PQ = a.P * a.Q;
    int m = step0 * BK + brow;
    int b = (int)a.fd_pq.div((uint32_t)m);
    int p = (int)a.fd_q.div((uint32_t)(m - b * PQ));
    int q = m - b * PQ - p * a.Q;
    auto dma = [&](const void* src, unsigned off) __attribute__((always_inline)) {
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + off), 16, 0, 0);
    };
    int slot = 0;
    auto issue = [&](int i) __attribute__((always_inline)) {  // step step0 + i into the next slot
        const unsigned sb = (unsigned)slot * SLOT;
        const int ms = (step0 + i) * BK;
        const int hi0 = p * a.sth, wi0 = q * a.stw;
        const bool rok = ms + brow < a.M;
        const long pix = ((long)(b * a.H + hi0) * a.W + wi0) << a.logC;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int hi = hi0 + bdh[j], wi = wi0 + bdw[j];
            const bool ok = rok & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
            dma(ok ? (const void*)(gx + pix + boff[j]) : zero, sb + j * BB + lw * 1024);
        }
        // next step's pixel: + BK = (adv_b, adv_p, adv_q), one carry per component at most
        int nq = q + a.adv_q, np = p + a.adv_p, nb = b + a.adv_b;
        if (nq >= a.Q) { nq -= a.Q; ++np; }
        if (np >= a.P) { np -= a.P; ++nb; }
        b = nb; p = np; q = nq;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool ok = ms + arow[h] < a.M;
#pragma unroll
            for (int ab = 0; ab < 2; ++ab) {
                dma(ok ? (const void*)ap[h][ab] : zero, sb + B + ab * AB + (2 * lw + h) * 1024);
                ap[h][ab] += astep;
            }
        }
        slot = slot + 1 == S ? 0 : slot + 1;
    };
    for (int i = 0; i < D && i < nst; ++i) issue(i);
    for (int i = 0; i < nst; ++i) {
        // step i has landed (13 pieces per step per loader wave; the D - 1 younger steps may stay
        // in flight, at the tail everything); after the barrier no compute wave reads step i - 1's
        // slot any more: step i + D refills it.  No DMA past the range, so none is in flight once
        // the last barrier has passed.
        if (i + D - 1 < nst) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(13 * (D - 1)) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (i + D < nst) issue(i + D);
    }
}
}  // namespace gm
