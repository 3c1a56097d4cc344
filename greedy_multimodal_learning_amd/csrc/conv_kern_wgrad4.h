// k_conv_wgrad4: the general bf16 weight-gradient kernel (any filter, stride and padding; C a
// power of two >= 8, K a multiple of 8).
#pragma once
#include "conv_kern_wfrag.h"

namespace gm {

struct WgradArgs {
    const uint16_t* dy;         // [N][P][Q][Kc]
    const uint16_t* x;          // [N][H][W][C]
    float* part;                // [splits][Kc][T*C]
    int N, H, W, C, logC, Kc, T, P, Q, sth, stw;
    int tiles_k, tiles_n, splits, steps_per_split;  // steps of 64 pixels
    FastDiv fd_pq, fd_q;        // pixel -> (b, p, q) without integer division
    int accumulate;             // k_conv_wgrad4 with one split: add into part (= dw) instead of storing
    int S, padh, padw;          // k_conv_wgrad4 decodes taps arithmetically
    int adv_b, adv_p, adv_q;    // one 64-pixel step in (b, p, q): 64 = adv_b*P*Q + adv_p*Q + adv_q
    long long gs_dy, gs_x, gs_part;  // view group g reads dy + g*gs_dy, x + g*gs_x, writes part + g*gs_part (elements)
};

// fragment of k-slice ks (rows 16ks + {q, q+4}) at immediate offsets BASE + ks*16*R (+4R)
template <int BASE, int R>
__device__ __forceinline__ bf16x8 tr_frag_asm(int ks, unsigned a) {
    short4_t lo, hi;
    switch (ks) {
        case 0: lo = tr_rd<BASE>(a); hi = tr_rd<BASE + 4 * R>(a); break;
        case 1: lo = tr_rd<BASE + 16 * R>(a); hi = tr_rd<BASE + 20 * R>(a); break;
        case 2: lo = tr_rd<BASE + 32 * R>(a); hi = tr_rd<BASE + 36 * R>(a); break;
        default: lo = tr_rd<BASE + 48 * R>(a); hi = tr_rd<BASE + 52 * R>(a); break;
    }
    const short8_t s = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, s);
}

// lgkmcnt(0), tied to the fragments (MT + NT of them) the next MFMAs read
template <int MT, int NT>
__device__ __forceinline__ void wait_lgkm0(bf16x8 (&a)[MT], bf16x8 (&b)[NT]) {
    static_assert(MT <= 2 && NT <= 2, "wait_lgkm0: tiles of 64 or 128");
    if constexpr (MT == 2 && NT == 2)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]));
    else if constexpr (MT == 2)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]));
    else if constexpr (NT == 2)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(b[0]), "+v"(b[1]));
    else
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(b[0]));
}

// Workgroup tile (64*MT) x (64*NT) of dw, 2x2 waves each owning MT*NT independent 32x32
// accumulators (the MFMAs of a k-slice do not wait on each other).  Operands are staged
// by LDS-DMA (global_load_lds_dwordx4) into two buffers, the DMA of pixel step s+1
// running under the MFMAs of step s, with the loop unrolled by the two buffers so every
// LDS fragment read is a base VGPR + immediate offset.  A DMA instruction writes 64 x
// 16 B linearly, so rows are unpadded (2*BM bytes) and a source-side XOR swizzle of the
// 16-B chunk keeps the tr-read half-waves conflict-free (the four rows a half-wave
// reads get their 64-B column window in four distinct bank quarters).  Padding taps
// read a zero block of the code object.
// WR = 1: the operands register-staged instead of LDS-DMA'd: global_load_dwordx4 of step
// s+2 into VGPRs while step s computes, ds_write_b128 of step s+1 into the buffer step s-1
// freed - an LDS-DMA piece costs its wave ~60-185 issue cycles among MFMAs (MI355X_MICROARCH.md
// price table), eight of them per 16-MFMA step at 128 x 128 tiles; a load + ds_write_b128
// costs ~20.  Same LDS image, same arithmetic (bit-identical results).
template <int MT, int NT, int WR = 0>
__global__ __launch_bounds__(256) void k_conv_wgrad4(WgradArgs a) {
    constexpr int BK = 64;
    constexpr int BM = 64 * MT, BN = 64 * NT;
    constexpr int RA = 2 * BM, RB = 2 * BN;          // row bytes
    constexpr int SA = BK * RA, SB = BK * RB;        // bytes per buffer
    constexpr int GA = SA / 1024 / 4, GB = SB / 1024 / 4;  // DMA instructions per wave per step
    constexpr int LPA = RA / 16, LPB = RB / 16;      // lanes per row
    extern __shared__ __attribute__((aligned(16))) uint4 wsm[];
    char* lds = reinterpret_cast<char*>(wsm);        // [A0][B0][A1][B1]
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    int bid = blockIdx.x;
    {   // XCD-major: the tiles of one pixel range share an XCD (and its L2 copy of the rows)
        const int n = gridDim.x, q = n >> 3, r = n & 7, x = bid & 7;
        bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
    }
    const int tiles = a.tiles_k * a.tiles_n;
    const int grp = bid / (tiles * a.splits);  // group-major: a group's tiles share XCDs
    bid -= grp * tiles * a.splits;
    const uint16_t* __restrict__ gdy = a.dy + grp * a.gs_dy;
    const uint16_t* __restrict__ gx = a.x + grp * a.gs_x;
    const int split = bid / tiles, tile = bid - split * tiles;
    const int tk = tile % a.tiles_k, tn = tile / a.tiles_k;
    const int k0 = tk * BM, n0 = tn * BN;
    const int PQ = a.P * a.Q;
    const int M = a.N * PQ;
    const int TC = a.T * a.C;
    const int step0 = split * a.steps_per_split;
    const int step1 = min((M + BK - 1) / BK, step0 + a.steps_per_split);
    const int nst = step1 - step0;

    // A (dy) DMA lanes: row a_row[j] of the step, 16-B chunk (swizzled) of channels
    const int a_rsub = lane / LPA, a_slot = lane % LPA;
    const uint16_t* a_ptr[GA];
    int a_row[GA];
    bool a_cok[GA];
#pragma unroll
    for (int j = 0; j < GA; ++j) {
        a_row[j] = (wave * GA + j) * (64 / LPA) + a_rsub;
        const int col = k0 + ((a_slot ^ wswz<RA>(a_row[j])) << 3);
        a_cok[j] = col < a.Kc;
        a_ptr[j] = gdy + ((size_t)step0 * BK + a_row[j]) * a.Kc + (a_cok[j] ? col : 0);
    }
    // B (x) DMA lanes: fixed (tap, channel chunk) per instruction; the lane's pixel
    // (b, p, q) is decoded once and then advanced by one 64-pixel step per issue
    // (adv_*: no per-step division in the issue path)
    const int b_rsub = lane / LPB, b_slot = lane % LPB;
    int b_row[GB], b_toff[GB], b_dh[GB], b_dw[GB];
    int b_b[GB], b_p[GB], b_q[GB];
    bool b_cok[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) {
        b_row[j] = (wave * GB + j) * (64 / LPB) + b_rsub;
        const int col = n0 + ((b_slot ^ wswz<RB>(b_row[j])) << 3);
        b_cok[j] = col < TC;
        const int tap = b_cok[j] ? col >> a.logC : 0;
        const int r = tap / a.S, s = tap - r * a.S;
        b_dh[j] = r - a.padh;
        b_dw[j] = s - a.padw;
        b_toff[j] = ((b_dh[j] * a.W + b_dw[j]) << a.logC) + (col & (a.C - 1));
        const int m = step0 * BK + b_row[j];
        b_b[j] = (int)a.fd_pq.div((uint32_t)m);
        const int pq = m - b_b[j] * PQ;
        b_p[j] = (int)a.fd_q.div((uint32_t)pq);
        b_q[j] = pq - b_p[j] * a.Q;
    }
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    const void* zero = (const void*)g_wzero16;
    // the sources of step step0 + i's pieces (A: dy rows, B: gathered x rows), in call order
    // (B's pixel walk advances one step per call)
    auto sources = [&](int i, const void* (&sa)[GA], const void* (&sb)[GB]) __attribute__((always_inline)) {
        const bool full = (step0 + i + 1) * BK <= M;
#pragma unroll
        for (int j = 0; j < GA; ++j) {
            const bool ok = a_cok[j] & (full | ((step0 + i) * BK + a_row[j] < M));  // no short-circuit branch
            sa[j] = ok ? (const void*)(a_ptr[j] + (size_t)i * BK * a.Kc) : zero;
        }
#pragma unroll
        for (int j = 0; j < GB; ++j) {
            const int b = b_b[j], p = b_p[j], q = b_q[j];
            const int h0 = p * a.sth, w0 = q * a.stw;
            const int hi = h0 + b_dh[j], wi = w0 + b_dw[j];
            const bool ok = b_cok[j] & (b < a.N) & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
            const int pix = (b * a.H + h0) * a.W + w0;
            sb[j] = ok ? (const void*)(gx + (((long)pix << a.logC) + b_toff[j])) : zero;
            // next step's pixel: + 64 = (adv_b, adv_p, adv_q), one carry per component at most
            int nq = q + a.adv_q, np = p + a.adv_p, nb = b + a.adv_b;
            if (nq >= a.Q) { nq -= a.Q; ++np; }
            if (np >= a.P) { np -= a.P; ++nb; }
            b_b[j] = nb; b_p[j] = np; b_q[j] = nq;
        }
    };
    auto issue = [&](int i, int bufoff) __attribute__((always_inline)) {  // step step0 + i
        const void* sa[GA];
        const void* sb[GB];
        sources(i, sa, sb);
#pragma unroll
        for (int j = 0; j < GA; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)sa[j], (lptr_t)(lds + bufoff + (wave * GA + j) * 1024), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < GB; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)sb[j], (lptr_t)(lds + bufoff + SA + (wave * GB + j) * 1024), 16, 0,
                                             0);
    };
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    u32x4 ra[WR ? GA : 1], rb[WR ? GB : 1];
    auto gload = [&](int i) __attribute__((always_inline)) {  // step step0 + i into registers
        const void* sa[GA];
        const void* sb[GB];
        sources(i, sa, sb);
#pragma unroll
        for (int j = 0; j < GA; ++j) ra[WR ? j : 0] = *reinterpret_cast<const u32x4*>(sa[j]);
#pragma unroll
        for (int j = 0; j < GB; ++j) rb[WR ? j : 0] = *reinterpret_cast<const u32x4*>(sb[j]);
    };
    auto swrite = [&](int bufoff) __attribute__((always_inline)) {  // the same LDS image as issue()
#pragma unroll
        for (int j = 0; j < GA; ++j)
            *reinterpret_cast<u32x4*>(lds + bufoff + (wave * GA + j) * 1024 + lane * 16) = ra[WR ? j : 0];
#pragma unroll
        for (int j = 0; j < GB; ++j)
            *reinterpret_cast<u32x4*>(lds + bufoff + SA + (wave * GB + j) * 1024 + lane * 16) = rb[WR ? j : 0];
    };

    floatx16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // tr-read geometry: half-wave g>>1 reads rows 8*(g>>1)+q4 (+4) of a 16-row k-slice, 4-column
    // block p4 of the 32-column fragment, 16-column half g&1.  The swizzle term depends on q4 only,
    // so (k-slice, +4 row) offsets are immediates on one base per fragment.
    const int g = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
    const int rbase = 8 * (g >> 1) + q4;
    int a_base[MT], b_base[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int c = wm * (32 * MT) + 32 * i + 16 * (g & 1) + 4 * p4;
        a_base[i] = rbase * RA + (((c >> 3) ^ wswz<RA>(rbase)) << 4) + (c & 7) * 2;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = wn * (32 * NT) + 32 * j + 16 * (g & 1) + 4 * p4;
        b_base[j] = SA + rbase * RB + (((c >> 3) ^ wswz<RB>(rbase)) << 4) + (c & 7) * 2;
    }
    unsigned a_lds[MT], b_lds[NT];  // LDS byte addresses of the fragment bases
#pragma unroll
    for (int i = 0; i < MT; ++i)
        a_lds[i] = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)(lds + a_base[i]);
#pragma unroll
    for (int j = 0; j < NT; ++j)
        b_lds[j] = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)(lds + b_base[j]);
    // one k-slice's fragments (asm reads; the caller waits), then its MFMAs; the next
    // slice's reads are issued before this slice's MFMAs
    // buffer 1 at an immediate offset while that fits the 16-bit field, else from its own
    // base registers (wide tiles: 64 KB buffers)
    constexpr bool kFarBuf = 2 * (SA + SB) > 65536;
    unsigned a_lds1[MT], b_lds1[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) a_lds1[i] = a_lds[i] + (SA + SB);
#pragma unroll
    for (int j = 0; j < NT; ++j) b_lds1[j] = b_lds[j] + (SA + SB);
    auto compute = [&](auto bufc) {
        constexpr int BO0 = decltype(bufc)::value;
        constexpr int BO = kFarBuf ? 0 : BO0;
        const unsigned* ab = (kFarBuf && BO0) ? a_lds1 : a_lds;
        const unsigned* bb = (kFarBuf && BO0) ? b_lds1 : b_lds;
        bf16x8 af[2][MT], bfr[2][NT];
        auto load = [&](int ks, int c) {
#pragma unroll
            for (int i = 0; i < MT; ++i) af[c][i] = tr_frag_asm<BO, RA>(ks, ab[i]);
#pragma unroll
            for (int j = 0; j < NT; ++j) bfr[c][j] = tr_frag_asm<BO, RB>(ks, bb[j]);
        };
        load(0, 0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int c = ks & 1;
            wait_lgkm0<MT, NT>(af[c], bfr[c]);
            if (ks < 3) load(ks + 1, c ^ 1);
            __builtin_amdgcn_sched_barrier(0);  // the next slice's reads go out before these MFMAs
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[c][i], bfr[c][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    constexpr int BUF1 = SA + SB;
    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, BUF1>;
    int i = 0;
    if constexpr (WR) {
        // LDS stores drained, then the barrier; the clobber keeps LDS accesses on their side
        auto bar = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
        if (nst > 0) {
            gload(0);
            swrite(0);
        }
        if (nst > 1) gload(1);
        bar();
        for (; i + 1 < nst; i += 2) {  // steps i (buffer 0) and i+1 (buffer 1)
            compute(B0{});
            swrite(BUF1);  // step i+1 (buffer 1 was freed by step i-1, before the last barrier)
            if (i + 2 < nst) gload(i + 2);
            bar();
            compute(B1{});
            if (i + 2 < nst) swrite(0);
            if (i + 3 < nst) gload(i + 3);
            bar();
        }
    } else {
        if (nst > 0) issue(0, 0);
        __syncthreads();
        for (; i + 1 < nst; i += 2) {  // steps i (buffer 0) and i+1 (buffer 1)
            issue(i + 1, BUF1);
            compute(B0{});
            __syncthreads();
            if (i + 2 < nst) issue(i + 2, 0);
            compute(B1{});
            __syncthreads();
        }
    }
    if (i < nst) compute(B0{});  // odd step count: the last step sits in buffer 0

    float* out = a.part + grp * a.gs_part + (size_t)split * a.Kc * TC;
    const bool inner = k0 + BM <= a.Kc && n0 + BN <= TC;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = n0 + wn * (32 * NT) + 32 * j + (lane & 31);
#pragma unroll
        for (int ii = 0; ii < MT; ++ii) {
            const int row0 = k0 + wm * (32 * MT) + 32 * ii + 4 * (lane >> 5);
            float* o = out + (size_t)row0 * TC + col;
            if (inner) {
                if (a.accumulate) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float* p = o + (size_t)((r & 3) + 8 * (r >> 2)) * TC;
                        *p += acc[ii][j][r];
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[(size_t)((r & 3) + 8 * (r >> 2)) * TC] = acc[ii][j][r];
                }
            } else if (col < TC) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row0 + (r & 3) + 8 * (r >> 2);
                    if (row < a.Kc) {
                        float* p = o + (size_t)((r & 3) + 8 * (r >> 2)) * TC;
                        *p = a.accumulate ? *p + acc[ii][j][r] : acc[ii][j][r];
                    }
                }
            }
        }
    }
}
}  // namespace gm
