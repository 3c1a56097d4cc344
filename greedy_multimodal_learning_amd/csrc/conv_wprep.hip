// Weight preparation for the bf16 convolutions (conv_igemm.hip, conv_wgrad.hip): the fp32 master
// weights cast, channel-padded and transposed into the layouts the kernels read.
#include <cstdint>

#include "gm_common.h"

namespace gm {

// W[Co][T][Ci] -> Wt[Ci][T][Co] (bf16), for the input-gradient convolution
__global__ void k_transpose_w(const uint16_t* w, uint16_t* wt, int Co, int T, int Ci) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = Co * T * Ci;
    if (i >= n) return;
    const int c = i % Ci, tk = (i / Ci) % T, k = i / (Ci * T);
    wt[((size_t)c * T + tk) * Co + k] = w[i];
}

}  // namespace gm

using namespace gm;

extern "C" int gm_conv_weight_transpose_bf16(const void* w, void* wt, int Co, int T, int Ci, void* stream) {
    GM_REQUIRE(w && wt && Co > 0 && T > 0 && Ci > 0, "weight transpose: bad args");
    const int n = Co * T * Ci;
    k_transpose_w<<<(n + 255) / 256, 256, 0, as_stream(stream)>>>((const uint16_t*)w, (uint16_t*)wt, Co, T, Ci);
    return check_launch("k_transpose_w");
}

// fp32 master weight [K][RS][C] (KRSC) -> bf16 [K][RS][Cp] (channels zero-padded to Cp)
// and, optionally, the channel-transposed bf16 copy [Cp][RS][K] used by dgrad: one pass
// instead of a cast + a transpose per convolution.
__global__ void k_weight_prep(const float* __restrict__ w, int K, int RS, int C, int Cp,
                              uint16_t* __restrict__ wb, uint16_t* __restrict__ wt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = K * RS * Cp;
    if (i >= n) return;
    const int c = i % Cp, t = (i / Cp) % RS, k = i / (Cp * RS);
    const float v = c < C ? w[((size_t)k * RS + t) * C + c] : 0.f;
    const uint16_t h = gm::Elem<uint16_t>::f2bf(v);
    wb[i] = h;
    if (wt) wt[((size_t)c * RS + t) * K + k] = h;
}

extern "C" int gm_conv_weight_prep_bf16(const float* w, int K, int RS, int C, int Cp, void* wb, void* wt,
                                        void* stream) {
    GM_REQUIRE(w && wb && K > 0 && RS > 0 && C > 0 && Cp >= C, "weight prep: bad args");
    const int n = K * RS * Cp;
    k_weight_prep<<<(n + 255) / 256, 256, 0, gm::as_stream(stream)>>>(w, K, RS, C, Cp, (uint16_t*)wb,
                                                                       (uint16_t*)wt);
    return gm::check_launch("k_weight_prep");
}

// Multi-tensor weight prep: every trunk convolution of a step in ONE launch.  One
// workgroup per 64(k) x 64(c) tile of one tap of one weight: fp32 loads coalesced
// along c, the bf16 KRSC copy written along c, the tile transposed through LDS so the
// [C][RS][K] dgrad copy is also written along k.
__global__ __launch_bounds__(256) void k_wprep_multi(const gm_wprep* __restrict__ tab, int n) {
    __shared__ uint16_t tile[64][66];  // 132-B rows: the transposed column reads are conflict-free
    const int blk = blockIdx.x;
    int lo = 0, hi = n - 1;  // last entry whose tile_start <= blk (uniform: scalar loads)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].tile_start <= blk) lo = mid;
        else hi = mid - 1;
    }
    const float* w = tab[lo].w;
    uint16_t* wb = static_cast<uint16_t*>(tab[lo].wb);
    uint16_t* wt = static_cast<uint16_t*>(tab[lo].wt);
    const int K = tab[lo].K, RS = tab[lo].RS, C = tab[lo].C, Cp = tab[lo].Cp;
    int r = blk - tab[lo].tile_start;
    const int tc = (Cp + 63) >> 6;
    const int ci = r % tc;
    r /= tc;
    const int tap = r % RS, k0 = (r / RS) * 64, c0 = ci * 64;
    // 8 consecutive elements per thread and step: two float4 loads along c, one 16-B bf16 store
    // (vector forms where the whole run is in range and aligned, element-wise otherwise)
    const bool vc = (C & 3) == 0 && (Cp & 7) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)wb & 15) == 0;
    for (int i = threadIdx.x; i < 64 * 8; i += 256) {
        const int kk = i >> 3, cq = (i & 7) * 8;
        const int k = k0 + kk, c = c0 + cq;
        uint16_t h[8];
        const float* src = w + ((size_t)k * RS + tap) * C + c;
        if (vc && k < K && c + 8 <= C) {
            const float4 u0 = reinterpret_cast<const float4*>(src)[0], u1 = reinterpret_cast<const float4*>(src)[1];
            const float f[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = gm::Elem<uint16_t>::f2bf(f[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = gm::Elem<uint16_t>::f2bf((k < K && c + j < C) ? src[j] : 0.f);
        }
        if (k < K) {
            uint16_t* dst = wb + ((size_t)k * RS + tap) * Cp + c;
            if (vc && c + 8 <= Cp) {
                *reinterpret_cast<uint4*>(dst) =
                    make_uint4(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16, h[4] | (uint32_t)h[5] << 16,
                               h[6] | (uint32_t)h[7] << 16);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (c + j < Cp) dst[j] = h[j];
            }
        }
        uint32_t* row = reinterpret_cast<uint32_t*>(&tile[kk][cq]);
#pragma unroll
        for (int j = 0; j < 4; ++j) row[j] = h[2 * j] | (uint32_t)h[2 * j + 1] << 16;
    }
    if (!wt) return;
    __syncthreads();
    // the [C][RS][K] copy: 8 consecutive k of one c per thread and step, one 16-B store
    const bool vk = (K & 7) == 0 && ((uintptr_t)wt & 15) == 0;
    for (int i = threadIdx.x; i < 64 * 8; i += 256) {
        const int cc = i >> 3, kq = (i & 7) * 8;
        const int k = k0 + kq, c = c0 + cc;
        if (c >= Cp) continue;
        uint16_t h[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = tile[kq + j][cc];
        uint16_t* dst = wt + ((size_t)c * RS + tap) * K + k;
        if (vk && k + 8 <= K) {
            *reinterpret_cast<uint4*>(dst) =
                make_uint4(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16, h[4] | (uint32_t)h[5] << 16,
                           h[6] | (uint32_t)h[7] << 16);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k + j < K) dst[j] = h[j];
        }
    }
}

extern "C" int gm_wprep_tiles(int K, int RS, int Cp) {
    if (K <= 0 || RS <= 0 || Cp <= 0) return 0;
    return ((K + 63) / 64) * RS * ((Cp + 63) / 64);
}

extern "C" int gm_conv_weight_prep_multi_bf16(const gm_wprep* table, int n, int total_tiles, void* stream) {
    GM_REQUIRE(table && n > 0 && total_tiles > 0, "weight prep multi: bad args");
    k_wprep_multi<<<total_tiles, 256, 0, gm::as_stream(stream)>>>(table, n);
    return gm::check_launch("k_wprep_multi");
}
