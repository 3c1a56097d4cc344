// bf16 convolution weight gradient on MFMA (gfx950), NHWC activations.
//
//   dw[k, t, c] = sum_{b,p,q} dy[b,p,q,k] * x[b, p*st + r_t - pad, q*st + s_t - pad, c]
//
// GEMM view: rows = output channels k, columns = (tap, c), reduction over the B*P*Q output
// pixels.  Both operands arrive pixel-major (channels contiguous), so every kernel stages
// [pixel][channel] rows in LDS and reads its v_mfma_f32_32x32x16_bf16 fragments with the gfx950
// transposed load ds_read_b64_tr_b16 (conv_kern_wfrag.h).  Four kernel families:
//   k_wgrad_stem, k_wgrad_stem_bn (conv_kern_wstem.h): the pixel-pair stem (7 x 4 filter over
//     8-channel pairs, strides (2, 1), 64 output channels);
//   k_wgrad_halo64 (conv_kern_whalo.h): 3x3 / s1 / p1, 64-channel multiples, W <= 62 (layers 1, 2);
//   k_wgrad_ring (conv_kern_wring.h): the other 3x3 shapes with K % 128 == 0 and C a power of two
//     >= 32 (layers 3, 4 and the strided first convolutions);
//   k_conv_wgrad4 (conv_kern_wgrad4.h): everything else (1x1, small shapes, cropped gradients).
// Each splits the pixels over workgroups into fp32 partial slabs that k_wgrad_sum (or, cropping
// padded input channels, k_wgrad_reduce) adds in a fixed order: deterministic, no atomics.
// This file: the two reductions, launch_wgrad() and the entry points.  The choice of kernel,
// splits and grid is plan_wgrad() in conv_wgrad_plan.h - one translation unit.
#include <cstring>

#include "conv_wgrad_plan.h"

namespace gm {

// dw[i] (+)= sum over splits of part[s][i] in ONE launch, for the uncropped case (Cp == Cr,
// every layer but the RGB stem).  A wave covers 64/R float4 columns with R split lanes per
// column (lane r sums splits r, r+R, ..., eight loads in flight), and the R lane sums are
// combined inside the wave by a fixed xor tree (DPP row rotate, swizzle, bpermute) - a fixed
// summation order for a given shape (deterministic) and NO LDS: these sums run on the weight-
// gradient stream beside LDS-heavy kernels (k_wgrad_halo64, k_wgrad_stem hold most of a CU's
// LDS), where the former LDS combine could not place its workgroups (the stem's sum: 6.3 us
// alone, 34 us in the step).  R is picked on the host so that small slabs still spread over
// hundreds of waves.
template <int C>
__device__ __forceinline__ float wsum_dpp(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), C, 0xf, 0xf, false));
}
__device__ __forceinline__ float wsum_x16(float v) {
    return v + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401f));
}
template <int R>
__global__ __launch_bounds__(256) void k_wgrad_sum(const float* __restrict__ part, int splits, size_t slab,
                                                   int accumulate, float* __restrict__ dw, long long gs_dw) {
    static_assert(R == 1 || R == 2 || R == 4 || R == 8, "k_wgrad_sum: 1, 2, 4 or 8 split lanes");
    constexpr int CPW = 64 / R, CPB = 4 * CPW;
    part += (size_t)blockIdx.y * splits * slab;  // view group blockIdx.y
    dw += blockIdx.y * gs_dw;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane / CPW, cw = lane - r * CPW;
    const size_t i4 = ((size_t)blockIdx.x * CPB + wave * CPW + cw) * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i4 < slab) {
        const float* p = part + i4;
        int s = r;
        for (; s + 7 * R < splits; s += 8 * R) {
            float4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = *(const float4*)(p + (size_t)(s + j * R) * slab);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc.x += v[j].x; acc.y += v[j].y; acc.z += v[j].z; acc.w += v[j].w;
            }
        }
        for (; s < splits; s += R) {
            const float4 v = *(const float4*)(p + (size_t)s * slab);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    // the split lanes of a column are lanes cw + CPW q: xor 8 (row rotate 8), 16, 32
    if constexpr (R >= 8) {
        acc.x = wsum_dpp<0x128>(acc.x); acc.y = wsum_dpp<0x128>(acc.y);
        acc.z = wsum_dpp<0x128>(acc.z); acc.w = wsum_dpp<0x128>(acc.w);
    }
    if constexpr (R >= 4) {
        acc.x = wsum_x16(acc.x); acc.y = wsum_x16(acc.y); acc.z = wsum_x16(acc.z); acc.w = wsum_x16(acc.w);
    }
    if constexpr (R >= 2) {
        acc.x += __shfl_xor(acc.x, 32); acc.y += __shfl_xor(acc.y, 32);
        acc.z += __shfl_xor(acc.z, 32); acc.w += __shfl_xor(acc.w, 32);
    }
    if (r != 0 || i4 >= slab) return;
    float4* o = (float4*)(dw + i4);
    if (accumulate) {
        const float4 v = *o;
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *o = acc;
}

// dw = sum over splits (fixed order); also the [K][T][Cpad] -> [K][T][Creal] crop
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* part, int splits, int Kc, int T, int Cp,
                                                      int Cr, int accumulate, float* dw, long long gs_dw) {
    const size_t n = (size_t)Kc * T * Cr;
    const size_t slab = (size_t)Kc * T * Cp;
    part += (size_t)blockIdx.y * splits * slab;  // view group blockIdx.y
    dw += blockIdx.y * gs_dw;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t c = i % Cr, kt = i / Cr;
        const size_t src = kt * Cp + c;
        float v = 0.f;
        for (int s = 0; s < splits; ++s) v += part[s * slab + src];
        dw[i] = accumulate ? dw[i] + v : v;
    }
}
}  // namespace gm

using namespace gm;

static WgradKnobs g_knobs;  // gm_conv_set_wgrad_*; read by plan_wgrad alone

static gm_conv_desc_hw to_hw(const gm_conv_desc* d) {
    return gm_conv_desc_hw{d->N, d->H, d->W, d->C, d->K, d->R, d->S, d->stride, d->stride, d->pad, d->pad};
}

template <auto Kern, class Args>
static int launch_form(const char* name, const WgradPlan& p, const Args& a, hipStream_t st) {
    if (int rc = grant_lds<Kern>(name, p.lds)) return rc;
    Kern<<<p.grid, p.wg, p.lds, st>>>(a);
    return check_launch(name);
}

// one 64-pixel step in (b, p, q): 64 = adv_b*P*Q + adv_p*Q + adv_q
template <class Args>
static void set_pixel_walk(Args& a, int P, int Q) {
    a.fd_pq = FastDiv((uint32_t)(P * Q));
    a.fd_q = FastDiv((uint32_t)Q);
    a.adv_b = 64 / (P * Q);
    a.adv_p = (64 % (P * Q)) / Q;
    a.adv_q = (64 % (P * Q)) % Q;
}

static int launch_stem(const WgradPlan& p, const void* dy, const void* x, const gm_stem_bn_src* src, float* part,
                       hipStream_t st) {
    const gm_conv_desc_hw* d = &p.d;
    WStemArgs s{};
    s.dy = (const uint16_t*)dy; s.x = (const uint16_t*)x; s.part = part;
    s.P = p.P; s.Q = p.Q; s.Wi = d->W;
    s.cpi = p.cpi; s.L = p.per; s.splits = p.splits;
    s.uchunks = 2 * d->W;
    s.upitch = s.uchunks * 16;
    s.ichunks = d->H * d->W;
    s.gs_dy = (long long)d->N * p.P * p.Q * 64;
    s.gs_x = (long long)d->N * d->H * d->W * 8;
    if (!p.bn) return launch_form<k_wgrad_stem<7, 4>>("k_wgrad_stem", p, s, st);
    s.dy = (const uint16_t*)src->y;
    s.gp = static_cast<const uint4*>(src->dy_pool);
    s.pidx = static_cast<const uint2*>(src->idx);
    s.fcoef = src->fcoef; s.fcoef_gs = src->fcoef_gs;
    s.bcoef = src->bcoef; s.bcoef_gs = src->bcoef_gs;
    s.Pp = (p.P + 1) / 2; s.Qp = (p.Q + 1) / 2;
    s.gs_pool = (long long)d->N * s.Pp * s.Qp * 8;
    return launch_form<k_wgrad_stem_bn<7, 4>>("k_wgrad_stem_bn", p, s, st);
}

static int launch_halo64(const WgradPlan& p, const void* dy, const void* x, float* part, hipStream_t st) {
    const gm_conv_desc_hw* d = &p.d;
    WHaloArgs h;
    h.dy = (const uint16_t*)dy; h.x = (const uint16_t*)x; h.part = part;
    h.N = d->N; h.H = d->H; h.W = d->W;
    h.rows = d->N * d->H;
    h.srows = (h.rows + 64 / p.pp - 1) / (64 / p.pp);
    h.splits = p.splits; h.rpw = p.per;
    h.K = d->K; h.C = d->C; h.kt = p.tiles_k; h.ct = p.tiles_n;
    h.gs_dy = (long long)d->N * d->H * d->W * d->K;
    h.gs_x = (long long)d->N * d->H * d->W * d->C;
    switch (p.pp) {  // 3 super-rows of LDS-DMA in flight
    case 16: return launch_form<k_wgrad_halo64<3, 16>>("k_wgrad_halo64", p, h, st);
    case 32: return launch_form<k_wgrad_halo64<3, 32>>("k_wgrad_halo64", p, h, st);
    default: return launch_form<k_wgrad_halo64<3, 64>>("k_wgrad_halo64", p, h, st);
    }
}

static int launch_ring(const WgradPlan& p, const void* dy, const void* x, float* part, long long gs_part,
                       int accumulate, hipStream_t st) {
    const gm_conv_desc_hw* d = &p.d;
    WRingArgs r;
    memset(&r, 0, sizeof(r));
    r.dy = (const uint16_t*)dy; r.x = (const uint16_t*)x; r.part = part;
    r.N = d->N; r.H = d->H; r.W = d->W; r.C = d->C; r.logC = log2_exact(d->C); r.K = d->K;
    r.P = p.P; r.Q = p.Q; r.sth = d->stride_h; r.stw = d->stride_w; r.padh = d->pad_h; r.padw = d->pad_w;
    r.M = d->N * p.P * p.Q;
    r.tiles_k = p.tiles_k; r.tiles_n = p.tiles_n; r.splits = p.splits; r.sps = p.per;
    set_pixel_walk(r, p.P, p.Q);
    r.gs_dy = (long long)r.M * d->K;
    r.gs_x = (long long)d->N * d->H * d->W * d->C;
    r.gs_part = gs_part; r.accumulate = accumulate;
    return launch_form<k_wgrad_ring>("k_wgrad_ring", p, r, st);
}

static int launch_wgrad4(const WgradPlan& p, const void* dy, const void* x, float* part, long long gs_part,
                         int accumulate, hipStream_t st) {
    const gm_conv_desc_hw* d = &p.d;
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.dy = (const uint16_t*)dy; a.x = (const uint16_t*)x; a.part = part;
    a.N = d->N; a.H = d->H; a.W = d->W; a.C = d->C; a.logC = log2_exact(d->C);
    a.Kc = d->K; a.T = d->R * d->S; a.P = p.P; a.Q = p.Q; a.sth = d->stride_h; a.stw = d->stride_w;
    a.tiles_k = p.tiles_k; a.tiles_n = p.tiles_n; a.splits = p.splits; a.steps_per_split = p.per;
    set_pixel_walk(a, p.P, p.Q);
    a.S = d->S; a.padh = d->pad_h; a.padw = d->pad_w;
    a.gs_dy = (long long)d->N * p.P * p.Q * d->K;
    a.gs_x = (long long)d->N * d->H * d->W * d->C;
    a.gs_part = gs_part; a.accumulate = accumulate;
    switch (p.mt << 8 | p.nt << 4 | p.wr) {
    case 0x220: return launch_form<k_conv_wgrad4<2, 2, 0>>("k_conv_wgrad4", p, a, st);
    case 0x221: return launch_form<k_conv_wgrad4<2, 2, 1>>("k_conv_wgrad4", p, a, st);
    case 0x210: return launch_form<k_conv_wgrad4<2, 1, 0>>("k_conv_wgrad4", p, a, st);
    case 0x211: return launch_form<k_conv_wgrad4<2, 1, 1>>("k_conv_wgrad4", p, a, st);
    case 0x120: return launch_form<k_conv_wgrad4<1, 2, 0>>("k_conv_wgrad4", p, a, st);
    case 0x121: return launch_form<k_conv_wgrad4<1, 2, 1>>("k_conv_wgrad4", p, a, st);
    case 0x110: return launch_form<k_conv_wgrad4<1, 1, 0>>("k_conv_wgrad4", p, a, st);
    default: return launch_form<k_conv_wgrad4<1, 1, 1>>("k_conv_wgrad4", p, a, st);
    }
}

// the split sum of every split weight-gradient kernel: k_wgrad_sum with R split lanes per
// column (at most 8, inside one wave), enough waves for small slabs
static int launch_wgrad_sum(const float* part, int splits, size_t slab, int accumulate, float* dw, long long gs,
                            int G, hipStream_t st) {
    const size_t ncol = slab / 4;
    int R = 1;
    while (R < 8 && R * 2 <= splits && (ncol * R + 255) / 256 < 512) R *= 2;
    const dim3 gg((unsigned)((ncol + 256 / R - 1) / (256 / R)), (unsigned)G);
    switch (R) {
        case 1: k_wgrad_sum<1><<<gg, 256, 0, st>>>(part, splits, slab, accumulate, dw, gs); break;
        case 2: k_wgrad_sum<2><<<gg, 256, 0, st>>>(part, splits, slab, accumulate, dw, gs); break;
        case 4: k_wgrad_sum<4><<<gg, 256, 0, st>>>(part, splits, slab, accumulate, dw, gs); break;
        default: k_wgrad_sum<8><<<gg, 256, 0, st>>>(part, splits, slab, accumulate, dw, gs); break;
    }
    return check_launch("k_wgrad_sum");
}

// Carries plan p out: the kernel's arguments and launch, then the reduction the plan names.  A
// direct kernel writes group g's gradient at dw + g*dw_stride itself; the others write their
// slabs to scratch (p.scratch bytes).  src: the stem BatchNorm's tensors (p.bn only).
static int launch_wgrad(const WgradPlan& p, const void* dy, const void* x, const gm_stem_bn_src* src, float* dw,
                        long long dw_stride, int accumulate, void* scratch, hipStream_t st) {
    float* part = p.direct ? dw : (float*)scratch;
    const long long gs_part = p.direct ? dw_stride : (long long)p.splits * (long long)p.slab;
    const int acc = p.direct ? accumulate : 0;
    int rc = GM_OK;
    switch (p.kernel) {
    case WgradKernel::stem: rc = launch_stem(p, dy, x, src, part, st); break;
    case WgradKernel::halo64: rc = launch_halo64(p, dy, x, part, st); break;
    case WgradKernel::ring: rc = launch_ring(p, dy, x, part, gs_part, acc, st); break;
    case WgradKernel::wgrad4: rc = launch_wgrad4(p, dy, x, part, gs_part, acc, st); break;
    }
    if (rc || p.reduce == WgradReduce::none) return rc;
    if (p.reduce == WgradReduce::sum)  // (slab is a multiple of 4: K % 8 == 0)
        return launch_wgrad_sum(part, p.splits, p.slab, accumulate, dw, dw_stride, p.G, st);
    const int T = p.d.R * p.d.S;
    const size_t n = (size_t)p.d.K * T * p.c_real;
    int g = (int)((n + 255) / 256);
    if (g > 4096) g = 4096;
    k_wgrad_reduce<<<dim3(g, p.G), 256, 0, st>>>(part, p.splits, p.d.K, T, p.d.C, p.c_real, accumulate, dw, dw_stride);
    return check_launch("k_wgrad_reduce");
}

// The scratch a caller provides before it knows c_real: a cropped gradient (c_real < C) drops
// every dedicated kernel back to k_conv_wgrad4 without its direct form, so the size is the larger
// of the whole-gradient plan's and that plan's.
extern "C" size_t gm_conv2d_wgrad_grouped_scratch(const gm_conv_desc_hw* d, int G) {
    if (!d || d->stride_h < 1 || d->stride_w < 1 || G < 1) return 0;
    return std::max(plan_wgrad(d, G, d->C, g_knobs).scratch, plan_wgrad(d, G, 0, g_knobs).scratch);
}

extern "C" size_t gm_conv2d_wgrad_hw_scratch(const gm_conv_desc_hw* d) {
    return gm_conv2d_wgrad_grouped_scratch(d, 1);
}

extern "C" size_t gm_conv2d_wgrad_scratch(const gm_conv_desc* d) {
    if (!d) return 0;
    const gm_conv_desc_hw h = to_hw(d);
    return gm_conv2d_wgrad_hw_scratch(&h);
}

// G view groups in one launch: group g reads dy + g*N*P*Q*K and x + g*N*H*W*C (the views
// stacked along the batch) and writes its weight gradient to dw + g*dw_stride (floats)
extern "C" int gm_conv2d_wgrad_grouped_bf16(const gm_conv_desc_hw* d, int G, const void* dy, const void* x,
                                            float* dw, long long dw_stride, int c_real, int accumulate,
                                            void* scratch, size_t scratch_bytes, void* stream) {
    GM_REQUIRE(d && dy && x && dw, "conv wgrad: null pointer");
    GM_REQUIRE(G >= 1 && G <= 64, "conv wgrad: view groups must be 1..64 (got %d)", G);
    GM_REQUIRE(d->stride_h >= 1 && d->stride_w >= 1 && d->pad_h >= 0 && d->pad_w >= 0, "conv wgrad: bad stride/pad");
    GM_REQUIRE(d->R * d->S <= kWTap, "conv wgrad: at most %d taps", kWTap);
    GM_REQUIRE(log2_exact(d->C) >= 3, "conv wgrad: C must be a power of two >= 8");
    GM_REQUIRE(d->K % 8 == 0, "conv wgrad: K must be a multiple of 8");
    GM_REQUIRE(c_real >= 1 && c_real <= d->C, "conv wgrad: bad c_real");
    const size_t slab_c = (size_t)d->K * d->R * d->S * (size_t)c_real;
    GM_REQUIRE(G == 1 || (dw_stride >= (long long)slab_c || dw_stride <= -(long long)slab_c),
               "conv wgrad: group gradient stride %lld overlaps one gradient", dw_stride);
    const WgradPlan p = plan_wgrad(d, G, c_real, g_knobs);
    GM_REQUIRE(scratch && scratch_bytes >= p.scratch, "conv wgrad: scratch %zu < %zu", scratch_bytes, p.scratch);
    return launch_wgrad(p, dy, x, nullptr, dw, dw_stride, accumulate, scratch, as_stream(stream));
}

extern "C" int gm_conv2d_wgrad_hw_bf16(const gm_conv_desc_hw* d, const void* dy, const void* x, float* dw,
                                       int c_real, int accumulate, void* scratch, size_t scratch_bytes,
                                       void* stream) {
    return gm_conv2d_wgrad_grouped_bf16(d, 1, dy, x, dw, 0, c_real, accumulate, scratch, scratch_bytes, stream);
}

extern "C" int gm_conv2d_wgrad_bf16(const gm_conv_desc* d, const void* dy, const void* x, float* dw, int c_real,
                                    int accumulate, void* scratch, size_t scratch_bytes, void* stream) {
    GM_REQUIRE(d, "conv wgrad: null pointer");
    const gm_conv_desc_hw h = to_hw(d);
    return gm_conv2d_wgrad_hw_bf16(&h, dy, x, dw, c_real, accumulate, scratch, scratch_bytes, stream);
}

// The stem's weight gradient with dy formed in the loader (greedymml.h: the stem BatchNorm +
// ReLU + max-pool backward, never written): k_wgrad_stem_bn on the k_wgrad_stem plan
extern "C" int gm_conv2d_wgrad_stem_bn_ok(const gm_conv_desc_hw* d, int G) {
    return plan_wgrad_stem_bn(d, G, g_knobs).rc == GM_OK ? 1 : 0;
}

extern "C" int gm_conv2d_wgrad_stem_bn_grouped_bf16(const gm_conv_desc_hw* d, int G, const gm_stem_bn_src* src,
                                                    const void* x, float* dw, long long dw_stride, int accumulate,
                                                    void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "gm_conv2d_wgrad_stem_bn_grouped_bf16";
    GM_REQUIRE(d && src && src->y && src->dy_pool && src->idx && src->fcoef && src->bcoef && x && dw,
               "%s: null pointer", fn);
    GM_REQUIRE(G >= 1 && G <= 64, "%s: view groups must be 1..64 (got %d)", fn, G);
    const WgradPlan p = plan_wgrad_stem_bn(d, G, g_knobs);
    if (p.rc != GM_OK) {
        set_error("%s", p.err);
        return p.rc;
    }
    GM_REQUIRE(G == 1 || dw_stride >= 64 * 224 || dw_stride <= -64 * 224, "%s: group gradient stride overlaps", fn);
    GM_REQUIRE(scratch && scratch_bytes >= p.scratch, "%s: scratch %zu < %zu", fn, scratch_bytes, p.scratch);
    return launch_wgrad(p, nullptr, x, src, dw, dw_stride, accumulate, scratch, as_stream(stream));
}

extern "C" int gm_conv_set_wgrad_staging(int wr) {
    GM_REQUIRE(wr >= 0 && wr <= 2,
               "gm_conv_set_wgrad_staging: 0 (LDS-DMA), 1 (register-staged), 2 (register-staged for 1x1 filters)");
    g_knobs.staging = wr;
    return GM_OK;
}

extern "C" int gm_conv_set_wgrad_loop(int mode) {
    GM_REQUIRE(mode >= 0 && mode <= 31 && !(mode & 1),
               "gm_conv_set_wgrad_loop: bit 1 halo kernel for 64 channels, bit 2 up to 128, bit 3 up to 512, "
               "bit 4 the ring kernel for 3x3 shapes with K % 128 == 0, C a power of two >= 32");
    g_knobs.loop = mode;
    return GM_OK;
}

extern "C" int gm_conv_set_wgrad_stem(int on) {
    g_knobs.stem = on ? 1 : 0;
    return GM_OK;
}

extern "C" int gm_stem_dw_crop(const float* dwp, int G, int K, int R, int S, int C0, int Sp, float* const* dst,
                               int accumulate, void* stream) {
    GM_REQUIRE(dwp && dst && G >= 1 && G <= kCropG && K > 0 && R > 0 && S > 0 && C0 >= 1 && C0 <= 4 &&
                   Sp == (S + 1) / 2,
               "gm_stem_dw_crop: bad arguments");
    StemCropArgs a{};
    a.dwp = dwp;
    for (int g = 0; g < G; ++g) {
        GM_REQUIRE(dst[g], "gm_stem_dw_crop: null destination %d", g);
        a.dst[g] = dst[g];
    }
    a.K = K; a.R = R; a.S = S; a.C0 = C0; a.Sp = Sp; a.accumulate = accumulate ? 1 : 0;
    const int n = K * R * S * C0;
    k_stem_dw_crop<<<dim3((unsigned)((n + 255) / 256), (unsigned)G), 256, 0, as_stream(stream)>>>(a);
    return check_launch("k_stem_dw_crop");
}
