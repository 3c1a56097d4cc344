// conv_igemm.hip: the pixel-pair stem kernel (k_conv_stem).
#pragma once
#include "conv_args.h"

namespace gm {

// ---------------------------------------------------------------------------------
// The ResNet stem on its pixel-pair view (conv.py: a 7 x 4 filter over 8-channel pairs,
// strides (2, 1), K = 224, 64 output channels, no padding).  A workgroup walks a
// contiguous run of output rows of one image, TWO rows per iteration:
//  * the weights live in VGPRs (each lane its 2 x 14 B fragments, 112 VGPRs), so the
//    LDS feeds only the pixel operand;
//  * input rows stream through an LDS ring of "units" of two input rows (unit u = rows
//    2u, 2u + 1, slot u % 8), fetched once per workgroup by register-staged global loads
//    two iterations ahead (no LDS-DMA: every LDS access is compiler-visible, so its waits
//    are exact);
//  * output rows p, p + 1 share input rows (row p + 1's tap row r is row p's r + 2): one
//    pixel fragment of input row j feeds row p's MFMAs (tap row j) and row p + 1's (tap
//    row j - 2) - 18 fragment reads for 56 MFMAs per wave, where the row-at-a-time form
//    with weights in LDS read 84;
//  * wave w owns output columns 32 w .. 32 w + 31 and all 64 channels; its 8 KB output
//    tile is private (no barrier between the MFMAs and the stores), leaving as whole
//    128-B pixel rows.
// One barrier per iteration (the ring).  The row-at-a-time kernel this replaces spent
// 121 us per step: per-k-step address math and an LDS round trip + barrier per row.
constexpr int kStemRing = 8;
struct StemArgs {
    int N, P;      // images, output rows per image
    int cpi, L;    // chunks (workgroups) per image, output rows per chunk (even)
    int uchunks;   // 16-B chunks per unit (2 * Wi)
    int upitch;    // LDS bytes per ring slot (uchunks * 16)
    int ichunks;   // 16-B chunks per image (Hi * Wi)
    float* stats;  // optional: per-workgroup BatchNorm partial rows of the stored output
                   // ([G][stats_rows][64 x (sum, sum of squares)] + 128 floats per group)
    int stats_rows;  // workgroups per group (N * cpi: the rows of each group's partials)
};

template <int R, int S>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_conv_stem(ConvArgs a, StemArgs r) {
    static_assert(S % 2 == 0 && R >= 2, "k_conv_stem: even pair-tap count per row");
    constexpr int KS = R * S / 2;  // k-steps (two taps of 8 channels each)
    constexpr int H2 = S / 2;      // k-steps per tap row
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    char* lds = reinterpret_cast<char*>(smem);  // [ring 8 x upitch][4 wave tiles x 8 KB]
    const ConvCls& cl = a.cls[0];
    const int Wi = a.Wi, Q = cl.Q;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int fr = lane & 31, fh = lane >> 5;
    const int per = r.stats_rows;
    const int g = blockIdx.x / per, wg = blockIdx.x - g * per;
    if (g >= a.G) return;
    const int b = wg / r.cpi, c = wg - b * r.cpi;
    const int p0 = c * r.L, p1 = min(cl.P, p0 + r.L);
    const uint4* const img = reinterpret_cast<const uint4*>(a.in + g * a.gs_in) + (size_t)b * r.ichunks;
    char* const tile = lds + kStemRing * r.upitch + wave * 8192;

    // weights -> VGPRs: fragment (k-step ks, channel block cb) = channel 32 cb + fr, tap 2 ks + fh
    bf16x8 wf[KS][2];
    {
        const uint4* wsrc = reinterpret_cast<const uint4*>(a.wt + g * a.gs_wt);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
                wf[ks][cb] = __builtin_bit_cast(bf16x8, wsrc[(cb * 32 + fr) * (2 * KS) + 2 * ks + fh]);
    }
    // two units (u, u + 1: 2 * uchunks 16-B chunks, contiguous in the image) per iteration:
    // thread t holds chunks t and t + 256 (2 * uchunks <= 512); zeros past the image
    auto fetch = [&](int u, uint4 (&v)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int cc = t + 256 * h;
            const int gi = u * r.uchunks + cc;
            v[h] = (cc < 2 * r.uchunks && gi < r.ichunks) ? img[gi] : make_uint4(0, 0, 0, 0);
        }
    };
    auto stash = [&](int u, const uint4 (&v)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int cc = t + 256 * h;
            if (cc < 2 * r.uchunks) {
                const int hi = cc >= r.uchunks;
                const int uu = u + hi;
                *reinterpret_cast<uint4*>(lds + (uu & (kStemRing - 1)) * r.upitch + (cc - hi * r.uchunks) * 16) = v[h];
            }
        }
    };
    // prologue: units p0 .. p0 + 4 into the ring (iteration 0's window), units of
    // iterations 1 and 2 into the register stages
    {
        uint4 v0[2], v1[2], v2[2];
        fetch(p0, v0);
        fetch(p0 + 2, v1);
        fetch(p0 + 4, v2);
        stash(p0, v0);
        stash(p0 + 2, v1);
        stash(p0 + 4, v2);  // (unit p0 + 5 too: part of iteration 1's window, rewritten there)
    }
    uint4 sa[2], sb[2];  // register stages: units for iterations i + 1 (written at i) and i + 2
    fetch(p0 + 5, sa);
    fetch(p0 + 7, sb);

    float bs1[8], bs2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bs1[j] = bs2[j] = 0.f;
    const int q = wave * 32 + fr;
    const int qc = q < Q ? q : 0;
    const size_t out_bytes = (size_t)a.N * a.Ho * a.Wo * a.Nout * 2;
    const __amdgpu_buffer_rsrc_t orsrc =
        __builtin_amdgcn_make_buffer_rsrc(cl.out + g * a.gs_out, 0, (int)(out_bytes < 0x7fffffffu ? out_bytes : 0x7fffffffu),
                                          0x00020000);

    auto iteration = [&](int p, uint4 (&cur)[2]) __attribute__((always_inline)) {
        __syncthreads();  // units p .. p + 4 are in the ring; iteration p - 2's reads are done
        stash(p + 5, cur);  // iteration p + 2's new units into the slots of units p - 3, p - 2
        fetch(p + 9, cur);  // ... and the iteration after next's into the registers

        floatx16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][cb][e] = 0.f;
        unsigned sl[5];  // ring slot bases of units p .. p + 4
#pragma unroll
        for (int d = 0; d < 5; ++d) sl[d] = (unsigned)(((p + d) & (kStemRing - 1)) * r.upitch);
        // pixel fragment (input row j, tap pair h): lane (q, fh) <- pixel pair q + 2 h + fh
#pragma unroll
        for (int j = 0; j < R + 2; ++j) {
#pragma unroll
            for (int h = 0; h < H2; ++h) {
                const bf16x8 af = *reinterpret_cast<const bf16x8*>(lds + sl[j >> 1] +
                                                                   (((j & 1) * Wi + qc + 2 * h + fh) << 4));
                if (j < R) {
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb)
                        acc[0][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j * H2 + h][cb], af, acc[0][cb], 0, 0, 0);
                }
                if (j >= 2) {
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb)
                        acc[1][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[(j - 2) * H2 + h][cb], af, acc[1][cb],
                                                                            0, 0, 0);
                }
            }
        }
        // the wave's tile: [row i][pixel fr][64 channels] bf16, 16-B chunks XOR-swizzled by pixel
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int chunk = (cb * 4 + gq) ^ (fr & 7);
                    *reinterpret_cast<uint2*>(tile + (i * 32 + fr) * 128 + chunk * 16 + 8 * fh) =
                        make_uint2(pack_bf2(acc[i][cb][4 * gq], acc[i][cb][4 * gq + 1]),
                                   pack_bf2(acc[i][cb][4 * gq + 2], acc[i][cb][4 * gq + 3]));
                }
        // 8 KB = 64 pixel rows of 128 B: store u covers pixel rows 8 u .. 8 u + 7, lane ->
        // (pixel row 8 u + lane / 8, chunk lane % 8): the channel group is lane % 8
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int pr = 8 * u + (lane >> 3), j = lane & 7;
            const int i = pr >> 5, px = pr & 31;
            const int qq = wave * 32 + px;
            const bool ok = qq < Q && p + i < p1;
            const uint4 v = *reinterpret_cast<const uint4*>(tile + pr * 128 + ((j ^ (px & 7)) << 4));
            const unsigned off = (unsigned)((((size_t)(b * a.Ho + p + i) * a.Wo + qq) * 64 + j * 8) * 2);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v),
                                                   orsrc, ok ? off : 0xfffffff0u, 0, 0);
            if (r.stats) {
                const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const float f = ok ? __uint_as_float((jj & 1) ? (w4[jj >> 1] & 0xffff0000u) : (w4[jj >> 1] << 16))
                                       : 0.f;
                    bs1[jj] += f;
                    bs2[jj] = fmaf(f, f, bs2[jj]);
                }
            }
        }
    };
    // iterations alternate the two register stages (stage a: units written at even iterations)
    for (int p = p0; p < p1; p += 4) {
        iteration(p, sa);
        if (p + 2 < p1) iteration(p + 2, sb);
    }
    if (r.stats) {  // the workgroup's partial row: [32 thread rows][64 channels][2] combined in LDS
        __syncthreads();
        float* red = reinterpret_cast<float*>(lds);  // the ring (>= 16 KB)
        const int r0 = t >> 3, cg = t & 7;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            red[r0 * 128 + (cg * 8 + jj) * 2] = bs1[jj];
            red[r0 * 128 + (cg * 8 + jj) * 2 + 1] = bs2[jj];
        }
        __syncthreads();
        if (t < 128) {
            float acc = 0.f;
            for (int i = 0; i < 32; ++i) acc += red[i * 128 + t];
            r.stats[((size_t)g * (r.stats_rows + 1) + wg) * 128 + t] = acc;
        }
    }
}

}  // namespace gm
