// conv_igemm.hip: the resident-weight layer-1 kernel (k_conv_rw).
#pragma once
#include "conv_args.h"

namespace gm {

// ---------------------------------------------------------------------------------
// 3x3 / stride-1 convolutions with 64 input and 64 output channels (ResNet layer 1:
// forward and input gradient).  The whole weight tensor (9 taps x 64 x 64 bf16 = 72 KB)
// stays resident in LDS for the life of a persistent workgroup, which walks output tiles
// of RT whole image rows (RT*W <= 128 pixels; MFMA rows past RT*W are padding whose
// outputs are not stored).  A tile's input is its (RT+2) x (W+2) zero-bordered halo
// (29 KB at 56x56), DMA'd into the second of two halo buffers while the MFMAs of the
// current tile run, so the only bytes staged per tile are the halo - instead of nine
// 16 KB im2col A tiles plus 72 KB of weights in the im2col kernel - and the k-loop is
// LDS reads + MFMAs only.  Halo pixels are 128-B rows XOR-swizzled as in k_conv_halo;
// weights are [tap][n][128 B] with the same swizzle on n.
struct RwArgs {
    int RT;        // image rows per tile
    int tpi;       // tiles per image (H / RT)
    int tiles;     // N * tpi
    int hbytes;    // one halo buffer (multiple of 1 KB)
    int nI;        // halo DMA instructions per tile
    int npix;      // (RT + 2) * (W + 2)
    FastDiv fd_w2, fd_tpi;
};

constexpr int kRwWeightBytes = 9 * 64 * 128;

// Form 0: the training step's kernel (the template keeps the symbol of earlier profiles).  Form 1,
// the evaluation epilogue: acc sc[n] + sh[n] on the accumulators before they are packed (a.coef),
// the residual through the addend path, the ReLU (a.relu) after the join; no statistics.
template <int Form = 0>
__global__ __launch_bounds__(256) void k_conv_rw(ConvArgs a, RwArgs r) {
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    char* lds = reinterpret_cast<char*>(smem);  // [weights][halo 0][halo 1]
    constexpr int WB = kRwWeightBytes;
    const ConvCls& cl = a.cls[0];
    const int H = a.Hi, W = a.Wi, W2 = W + 2;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int slot = lane & 7, fr = lane & 31, fh = lane >> 5;
    const unsigned pk_dh = cl.pk_dh, pk_dw = cl.pk_dw, pk_r = cl.pk_r, pk_s = cl.pk_s;
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    // view groups: gridDim / G workgroups per group, each walking that group's tiles
    int g = 0, tl = blockIdx.x, nwg = gridDim.x;
    if (a.G > 1) {
        nwg = gridDim.x / a.G;
        g = tl / nwg;
        tl -= g * nwg;
    }
    if (tl >= r.tiles || g >= a.G) return;
    const uint16_t* const gin = a.in + g * a.gs_in;
    const uint16_t* const gwt = a.wt + g * a.gs_wt;
    const uint16_t* const gadd = a.addend ? a.addend + g * a.gs_out : nullptr;

    // weights, once: instruction I = tap (I >> 3), rows n = 8 (I & 7) .. + 7
    for (int I = wave; I < 72; I += 4) {
        const int tp = I >> 3, n = (I & 7) * 8 + (lane >> 3);
        const int ti = tp / 3, tj = tp - ti * 3;
        const int tw = (int)((pk_r >> (4 * ti)) & 15u) * a.Sw + (int)((pk_s >> (4 * tj)) & 15u);
        const int gc = slot ^ ((n >> 1) & 7);
        __builtin_amdgcn_global_load_lds((gptr_t)(gwt + ((size_t)n * a.T + tw) * 64 + gc * 8),
                                         (lptr_t)(lds + I * 1024), 16, 0, 0);
    }
    // the halo of tile tl (image b, output rows p0 .. p0+RT-1) into buffer bb.  The halo's
    // geometry relative to the tile origin is the same for every tile, so each lane's
    // source offsets (kMaxHI instructions per wave at most) are decoded once: per tile only
    // the origin and the image-border rows (top row valid iff p0 > 0, bottom iff p0+RT < H).
    constexpr int kMaxHI = 12;
    int h_rel[kMaxHI];
    unsigned h_cls = 0;  // 2 bits per instruction: 0 always, 1 top row, 2 bottom row, 3 never
#pragma unroll
    for (int j = 0; j < kMaxHI; ++j) {
        const int I = wave + 4 * j;
        const int hp = I * 8 + (lane >> 3);
        const int rr = (int)r.fd_w2.div((uint32_t)hp), c = hp - rr * W2;
        const int gc = slot ^ ((hp >> 1) & 7);
        h_rel[j] = ((rr - 1) * W + c - 1) * 64 + gc * 8;
        unsigned k = rr == 0 ? 1u : rr == r.RT + 1 ? 2u : 0u;
        if (I >= r.nI || hp >= r.npix || c == 0 || c == W + 1) k = 3u;
        h_cls |= k << (2 * j);
    }
    auto issue_halo = [&](int tile, int bb) {
        const int b = (int)r.fd_tpi.div((uint32_t)tile);
        const int p0 = (tile - b * r.tpi) * r.RT;
        const uint16_t* origin = gin + ((size_t)(b * H + p0) * W << 6);
        const unsigned okmask = 1u | (p0 > 0 ? 2u : 0u) | (p0 + r.RT < H ? 4u : 0u);  // bit k: class k valid
        char* base = lds + WB + bb * r.hbytes;
#pragma unroll
        for (int j = 0; j < kMaxHI; ++j) {
            const int I = wave + 4 * j;
            if (I >= r.nI) break;
            const bool ok = (okmask >> ((h_cls >> (2 * j)) & 3u)) & 1u;
            const void* src = ok ? (const void*)(origin + h_rel[j]) : (const void*)g_zero16;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(base + I * 1024), 16, 0, 0);
        }
    };
    issue_halo(tl, 0);

    // tile-invariant fragment geometry: MFMA row block i of this wave -> tile pixel
    const int valid = r.RT * W;
    int hbase[2], prow[2], pcol[2];
    bool pok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int m = wm * 64 + i * 32 + fr;
        pok[i] = m < valid;
        m = pok[i] ? m : 0;
        prow[i] = m / W;
        pcol[i] = m - prow[i] * W;
        hbase[i] = (prow[i] + 1) * W2 + pcol[i] + 1;
    }
    const int nb = wn * 32 + fr;
    const int b0 = nb * 128 + ((fh ^ ((nb >> 1) & 7)) << 4);  // B fragment, tap 0, k-step 0
    int b_ks[4];  // per k-step (the tap adds an immediate tap * 8192)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) b_ks[ks] = b0 ^ (ks << 5);

    constexpr int kWaitAll = (7 << 4) | (15 << 8);  // s_waitcnt vmcnt(0)
    constexpr int kStores = 8;                      // epilogue stores per wave per tile (addend path)
    constexpr int kWaitStores = kStores | (7 << 4) | (15 << 8);  // vmcnt(kStores)
    constexpr int kWaitStores4 = 4 | (7 << 4) | (15 << 8);       // LDS-tile path: 4 16-B stores
    __builtin_amdgcn_s_waitcnt(kWaitAll);
    lds_barrier();
    const size_t out_bytes = (size_t)a.N * a.Ho * a.Wo * a.Nout * 2;
    const __amdgpu_buffer_rsrc_t orsrc =
        __builtin_amdgcn_make_buffer_rsrc(cl.out + g * a.gs_out, 0, (int)(out_bytes < 0x7fffffffu ? out_bytes : 0x7fffffffu),
                                          0x00020000);

    // BatchNorm statistics (a.stats; forward: y, input gradient: the BN backward's dz against
    // a.bnx): this thread's channel group t % 8 summed over the pixels it stores, combined over
    // the workgroup after the last tile (partial row wg)
    const int wg = tl;
    f32x2 bs1[4], bs2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) bs1[k] = bs2[k] = f32x2{0.f, 0.f};
    BnB bq;
    if (a.stats && a.bnx) bnb_load(a, g, 8 * (t & 7), bq);
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint16_t*>(a.bnx ? a.bnx + g * a.gs_out : cl.out), 0,
        (int)(out_bytes < 0x7fffffffu ? out_bytes : 0x7fffffffu), 0x00020000);
    // Form 1: this lane's channels n = wn * 32 + 8 gq + 4 fh + 0..3, the same for every tile
    float4 csc[Form == 1 ? 4 : 1], csh[Form == 1 ? 4 : 1];
    if constexpr (Form == 1) {
        const float* const cf = a.coef + (long long)g * a.gs_coef + wn * 32 + 4 * fh;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            csc[gq] = *reinterpret_cast<const float4*>(cf + 8 * gq);
            csh[gq] = *reinterpret_cast<const float4*>(cf + 64 + 8 * gq);
        }
    }
    int bb = 0;
    for (; tl < r.tiles; tl += nwg) {
        const int nx = tl + nwg;
        const int b = (int)r.fd_tpi.div((uint32_t)tl);
        const int p0 = (tl - b * r.tpi) * r.RT;
        const unsigned tbase = (unsigned)(((size_t)(b * a.Ho + p0) * a.Wo) * a.Nout * 2);
        // backward statistics: the BN input's chunks of this tile, loaded under the MFMAs
        // (issued before the next halo's DMA so their wait does not include it)
        __attribute__((ext_vector_type(4))) unsigned xv[4];
        if (a.stats && a.bnx && !a.addend) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = t + 256 * u;
                xv[u] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, (e >> 3) < valid ? tbase + (unsigned)e * 16u
                                                                                     : 0xfffffff0u, 0, 0);
            }
        }
        if (nx < r.tiles) issue_halo(nx, bb ^ 1);  // buffer bb^1 was released by the last barrier
        const int hoff = WB + bb * r.hbytes;

        floatx16 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
        bf16x8 af[2][2], bfr[2];
        unsigned abase[2];
        const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
        auto tap_base = [&](int tp) {
            const int ti = tp / 3, tj = tp - ti * 3;
            const int dh = (int)((pk_dh >> (4 * ti)) & 15u) - 8, dw = (int)((pk_dw >> (4 * tj)) & 15u) - 8;
            const int toff = dh * W2 + dw;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int hp = hbase[i] + toff;
                abase[i] = lds0 + ((unsigned)(hoff + (hp << 7)) | (unsigned)((((hp >> 1) & 7) ^ fh) << 4));
            }
        };
        auto load_b = [&](auto tpc, int ks, int c) {
            constexpr int TP = decltype(tpc)::value;  // ds offsets are 16-bit: tap 8 moves the base
            if constexpr (TP < 8) bfr[c] = lds_rd128<TP * 8192>(lds0 + (unsigned)b_ks[ks]);
            else bfr[c] = lds_rd128<0>(lds0 + (unsigned)b_ks[ks] + TP * 8192u);
        };
        auto load = [&](int k, int c) {  // k-step k = 4 * tap + ks
            const int tp = k >> 2, ks = k & 3;
            if (ks == 0) tap_base(tp);
#pragma unroll
            for (int i = 0; i < 2; ++i) af[c][i] = lds_rd128<0>(abase[i] ^ (unsigned)(ks << 5));
            switch (tp) {
                case 0: load_b(std::integral_constant<int, 0>{}, ks, c); break;
                case 1: load_b(std::integral_constant<int, 1>{}, ks, c); break;
                case 2: load_b(std::integral_constant<int, 2>{}, ks, c); break;
                case 3: load_b(std::integral_constant<int, 3>{}, ks, c); break;
                case 4: load_b(std::integral_constant<int, 4>{}, ks, c); break;
                case 5: load_b(std::integral_constant<int, 5>{}, ks, c); break;
                case 6: load_b(std::integral_constant<int, 6>{}, ks, c); break;
                case 7: load_b(std::integral_constant<int, 7>{}, ks, c); break;
                default: load_b(std::integral_constant<int, 8>{}, ks, c); break;
            }
        };
        // one k-step of fragments in flight under the MFMAs: wait for everything, issue the
        // next k-step's reads, then this k-step's MFMAs (counted waits that keep two
        // k-steps in flight are not used: k_conv_stem showed sporadic wrong tiles with them)
        load(0, 0);
#pragma unroll
        for (int k = 0; k < 36; ++k) {
            const int c = k & 1;
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[c][0]), "+v"(af[c][1]), "+v"(bfr[c]));
            if (k + 1 < 36) load(k + 1, c ^ 1);
            __builtin_amdgcn_sched_barrier(0);  // the next k-step's reads go out before these MFMAs
#pragma unroll
            for (int i = 0; i < 2; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[c], af[c][i], acc[i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }

        if constexpr (Form == 1) {
            const bool act = a.relu && !a.addend;  // with a residual the ReLU follows the join
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    float o0 = fmaf(acc[i][4 * gq], csc[gq].x, csh[gq].x), o1 = fmaf(acc[i][4 * gq + 1], csc[gq].y, csh[gq].y);
                    float o2 = fmaf(acc[i][4 * gq + 2], csc[gq].z, csh[gq].z), o3 = fmaf(acc[i][4 * gq + 3], csc[gq].w, csh[gq].w);
                    if (act) {
                        o0 = relu_nan(o0); o1 = relu_nan(o1); o2 = relu_nan(o2); o3 = relu_nan(o3);
                    }
                    acc[i][4 * gq] = o0; acc[i][4 * gq + 1] = o1; acc[i][4 * gq + 2] = o2; acc[i][4 * gq + 3] = o3;
                }
        }
        if (!a.addend) {
            // epilogue through LDS: the tile's RT whole image rows are one contiguous NHWC
            // block, assembled in LDS (16-B chunks XOR-swizzled by pixel) and written with
            // 16-B stores instead of 8 B per lane at a 128-B stride
            char* ot = lds + WB + 2 * r.hbytes;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = wm * 64 + i * 32 + fr;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int chunk = (wn * 4 + gq) ^ (m & 7);
                    *reinterpret_cast<uint2*>(ot + m * 128 + chunk * 16 + 8 * fh) =
                        make_uint2(pack_bf2(acc[i][4 * gq], acc[i][4 * gq + 1]),
                                   pack_bf2(acc[i][4 * gq + 2], acc[i][4 * gq + 3]));
                }
            }
            __syncthreads();
            uint4 vv[4];  // the four reads together, then the stores (then the statistics)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = t + 256 * u;  // 16-B chunk e of the tile: pixel e / 8, chunk e % 8
                const int m = e >> 3, j = e & 7;
                vv[u] = *reinterpret_cast<const uint4*>(ot + (m < valid ? m : 0) * 128 + ((j ^ (m & 7)) << 4));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = t + 256 * u;
                __builtin_amdgcn_raw_buffer_store_b128(
                    __builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, vv[u]), orsrc,
                    (e >> 3) < valid ? tbase + (unsigned)e * 16u : 0xfffffff0u, 0, 0);
            }
            if (a.stats && a.bnx) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = ((t + 256 * u) >> 3) < valid;
                    const unsigned w4[4] = {ok ? vv[u].x : 0u, ok ? vv[u].y : 0u, ok ? vv[u].z : 0u,
                                            ok ? vv[u].w : 0u};
                    const unsigned x4[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
                    bn_acc_bwd(w4, x4, bq, bs1, bs2);
                }
            } else if (a.stats) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = ((t + 256 * u) >> 3) < valid;
                    const unsigned w4[4] = {ok ? vv[u].x : 0u, ok ? vv[u].y : 0u, ok ? vv[u].z : 0u,
                                            ok ? vv[u].w : 0u};
                    bn_acc_fwd(w4, bs1, bs2);
                }
            }
            // the next tile's halo (issued before these stores) has landed; the stores may
            // still be in flight.  Then every wave is done with buffer bb and the LDS tile.
            __builtin_amdgcn_s_waitcnt(kWaitStores4);
            lds_barrier();
            bb ^= 1;
            continue;
        }
        // epilogue with the fused gradient join: rows p0 + prow, columns pcol; 4 consecutive
        // output channels per store, the addend loaded for the whole tile first (its loads in
        // flight together), added in fp32 before the one rounding to bf16
        size_t off[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ho = (p0 + prow[i]) * cl.oS + cl.oH, wo = pcol[i] * cl.oS + cl.oW;
            off[i] = ((size_t)(b * a.Ho + ho) * a.Wo + wo) * a.Nout + wn * 32 + 4 * fh;
        }
        uint2 av[2][4];
        if (a.addend) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
                    av[i][gq] = *(const uint2*)(gadd + off[i] + 8 * gq);  // rows past RT*W read row 0
            if (a.amask) {  // element e's bit: byte e / 8, nibble (e / 4) & 1
                const uint8_t* const gm = a.amask + g * a.gs_out / 8;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        const size_t e = off[i] + 8 * gq;
                        const unsigned b = (unsigned)gm[e >> 3] >> (e & 4);
                        av[i][gq].x = mask_bf2(av[i][gq].x, b);
                        av[i][gq].y = mask_bf2(av[i][gq].y, b >> 2);
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                float o0 = acc[i][4 * gq], o1 = acc[i][4 * gq + 1];
                float o2 = acc[i][4 * gq + 2], o3 = acc[i][4 * gq + 3];
                if (a.addend) {
                    o0 += bf_lo(av[i][gq].x); o1 += bf_hi(av[i][gq].x);
                    o2 += bf_lo(av[i][gq].y); o3 += bf_hi(av[i][gq].y);
                }
                if constexpr (Form == 1) {
                    if (a.relu) {
                        o0 = relu_nan(o0); o1 = relu_nan(o1); o2 = relu_nan(o2); o3 = relu_nan(o3);
                    }
                }
                typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                const u32x2 v = {pack_bf2(o0, o1), pack_bf2(o2, o3)};
                // every wave issues exactly kStores stores (padding rows get an offset past
                // the buffer's range, which the hardware drops), so the wait below can count them
                __builtin_amdgcn_raw_buffer_store_b64(v, orsrc, pok[i] ? (unsigned)((off[i] + 8 * gq) * 2) : 0xfffffff0u,
                                                      0, 0);
            }
        }
        // the next tile's halo (issued before these stores) has landed; the stores may
        // still be in flight.  Then every wave is done with buffer bb.
        __builtin_amdgcn_s_waitcnt(kWaitStores);
        lds_barrier();
        bb ^= 1;
    }
    if (a.stats) {  // the partial row: [32 thread rows][64 channels][2] combined in the free LDS tile
        float* red = reinterpret_cast<float*>(lds + WB + 2 * r.hbytes);  // 16 KB
        const int r0 = t >> 3, cg = t & 7;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            red[r0 * 128 + (cg * 8 + 2 * k) * 2] = bs1[k].x;
            red[r0 * 128 + (cg * 8 + 2 * k) * 2 + 1] = bs2[k].x;
            red[r0 * 128 + (cg * 8 + 2 * k + 1) * 2] = bs1[k].y;
            red[r0 * 128 + (cg * 8 + 2 * k + 1) * 2 + 1] = bs2[k].y;
        }
        __syncthreads();
        if (t < 128) {
            float s = 0.f;
            for (int i = 0; i < 32; ++i) s += red[i * 128 + t];
            a.stats[((size_t)g * (a.stats_rows + 1) + wg) * 128 + t] = s;
        }
    }
}

}  // namespace gm
