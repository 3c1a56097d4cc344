// What the two reference-precision convolution kernels share (conv_f32.hip: exact-f32
// MFMA; conv_f32_split.hip: split-bf16 MFMA): the kernel arguments, the im2col-on-the-fly
// operand gathers, the fixed-order split-reduction sum and the planner.  Everything sits
// in an unnamed namespace: each translation unit owns its copy.
#pragma once
#include <cstring>

#include "gm_common.h"

namespace gm {
namespace {

constexpr int kBK = 16;  // the planner's k-tile (fp32 elements)
typedef float floatx16 __attribute__((ext_vector_type(16)));

enum { FWD = 0, DGRAD = 1, WGRAD = 2 };

struct F32Args {
    int M, N, Kr;                  // GEMM shape (Kr = reduction length)
    int Nb, H, W, C, K, R, S, st, pad, P, Q;
    const float* x;
    const float* w;
    const float* dy;
    float* out;
    const float* addend;           // dgrad: added to the result (gradient join), may be null
    int accumulate;                // out += result
    int ktiles, kt_per_split;      // k-tiles in total / per split (blockIdx.z)
    float* part;                   // splits > 1: [splits][M][N] fp32 slabs
    FastDiv fd_C, fd_S, fd_K, fd_Q, fd_P, fd_W, fd_H, fd_st;
    // the forward-only affine epilogue (gm_conv2d_f32_affine; read by the AFF forms alone)
    const float* coef;             // [2][N]: sc then sh (gm_bn_infer_coef's layout)
    const float* residual;         // out's layout, may be null, may be out itself
    int relu;
};

// ---- operand element access --------------------------------------------------
// Row decode of an output / input pixel index.
struct Pix {
    int n, a, b;  // (n, p, q) or (n, h, w)
};
__device__ __forceinline__ Pix dec_pix(unsigned m, const FastDiv& fq, const FastDiv& fp, int Q, int P) {
    const unsigned t = fq.div(m);
    const unsigned n = fp.div(t);
    return Pix{(int)n, (int)(t - n * P), (int)(m - t * Q)};
}

// x[n, h, w, c..c+V) with zero outside the image
template <int V>
__device__ __forceinline__ void ld_x(const F32Args& a, int n, int h, int w, int c, float* o) {
    if ((unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W) {
        const float* p = a.x + (((long long)n * a.H + h) * a.W + w) * a.C + c;
        if (V == 4) {
            const float4 v = *reinterpret_cast<const float4*>(p);
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        } else {
            o[0] = *p;
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = 0.f;
    }
}

// A(m, kk..kk+V) for FWD (x gather) and DGRAD (dy gather); pixel row pre-decoded.
template <int MODE, int V>
__device__ __forceinline__ void ld_a(const F32Args& a, const Pix& px, bool mok, int kk, float* o) {
    if (!mok || kk >= a.Kr) {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = 0.f;
        return;
    }
    if (MODE == FWD) {
        const unsigned rs = a.fd_C.div((unsigned)kk);
        const int c = kk - (int)rs * a.C;
        const unsigned r = a.fd_S.div(rs);
        const int s = (int)(rs - r * a.S);
        ld_x<V>(a, px.n, px.a * a.st - a.pad + (int)r, px.b * a.st - a.pad + s, c, o);
    } else {  // DGRAD: kk = (r, s, k), k fastest
        const unsigned rs = a.fd_K.div((unsigned)kk);
        const int k = kk - (int)rs * a.K;
        const unsigned r = a.fd_S.div(rs);
        const int s = (int)(rs - r * a.S);
        const int hp = px.a + a.pad - (int)r, wp = px.b + a.pad - s;
        const unsigned p = a.fd_st.div((unsigned)(hp < 0 ? 0 : hp)), q = a.fd_st.div((unsigned)(wp < 0 ? 0 : wp));
        const bool ok = hp >= 0 && wp >= 0 && (int)p * a.st == hp && (int)q * a.st == wp && (int)p < a.P &&
                        (int)q < a.Q;
        if (ok) {
            const float* src = a.dy + (((long long)px.n * a.P + p) * a.Q + q) * a.K + k;
            if (V == 4) {
                const float4 v = *reinterpret_cast<const float4*>(src);
                o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
            } else {
                o[0] = *src;
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = 0.f;
        }
    }
}

// splits > 1: out[i] = sum_s part[s][i] (+ addend) (+ out), fixed order
__global__ __launch_bounds__(256) void k_conv_f32_splitk_sum(const float* __restrict__ part, int splits, long long n,
                                                            const float* __restrict__ addend, int accumulate,
                                                            float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float v = 0.f;
        for (int s = 0; s < splits; ++s) v += part[(size_t)s * n + i];
        if (addend) v += addend[i];
        if (accumulate) v += out[i];
        out[i] = v;
    }
}

// The eval-mode BatchNorm (+ residual, + ReLU) on an fp32 accumulator: k_bn_apply's fp32
// arithmetic term for term (batchnorm.hip), so a convolution that ends in it equals the
// convolution followed by gm_bn_fwd_infer_f32 bit for bit.  The fma is explicit: no
// contraction setting can change it.  The residual may be the output buffer: element o
// is read and then written by this thread alone.
__device__ __forceinline__ float affine_epilogue(float v, float sc, float sh, const float* residual, size_t o,
                                                 int relu) {
    v = fmaf(v, sc, sh);
    if (residual) v += residual[o];
    return relu ? relu_nan(v) : v;
}

// splits > 1, affine form: out[i] = epilogue(sum_s part[s][i]) with column n = i mod N; the
// sum is k_conv_f32_splitk_sum's, term for term.  residual and out may alias (no __restrict__).
__global__ __launch_bounds__(256) void k_conv_f32_splitk_sum_affine(const float* __restrict__ part, int splits,
                                                                   long long n, int N,
                                                                   const float* __restrict__ coef,
                                                                   const float* residual, int relu, float* out) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long stride = (long long)gridDim.x * 256;
    unsigned c = (unsigned)(i % N);       // the one division; the column then steps with the index
    const unsigned cstep = (unsigned)(stride % N);
    for (; i < n; i += stride) {
        float v = 0.f;
        for (int s = 0; s < splits; ++s) v += part[(size_t)s * n + i];
        out[i] = affine_epilogue(v, coef[c], coef[N + c], residual, (size_t)i, relu);
        c += cstep;
        if (c >= (unsigned)N) c -= (unsigned)N;
    }
}

struct Plan {
    F32Args a;
    int TM, TN, splits;
    bool vec;
    dim3 grid;
    size_t scratch;
};

inline int cus() {
    static const int n = [] {
        int dev = 0, c = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return 256;
        return c;
    }();
    return n;
}

inline int make_plan(const gm_conv_f32* p, Plan& pl, const char* fn) {
    if (!p) {
        set_error("%s: null descriptor", fn);
        return GM_E_ARG;
    }
    const gm_conv_desc& d = p->d;
    if (p->mode < 0 || p->mode > 2 || d.N < 1 || d.H < 1 || d.W < 1 || d.C < 1 || d.K < 1 || d.R < 1 || d.S < 1 ||
        d.stride < 1 || d.pad < 0) {
        set_error("%s: bad descriptor (mode=%d N=%d H=%d W=%d C=%d K=%d R=%d S=%d stride=%d pad=%d)", fn, p->mode, d.N,
                  d.H, d.W, d.C, d.K, d.R, d.S, d.stride, d.pad);
        return GM_E_ARG;
    }
    const int P = (d.H + 2 * d.pad - d.R) / d.stride + 1, Q = (d.W + 2 * d.pad - d.S) / d.stride + 1;
    if (P < 1 || Q < 1) {
        set_error("%s: empty output", fn);
        return GM_E_ARG;
    }
    F32Args& a = pl.a;
    memset(&a, 0, sizeof(a));
    a.Nb = d.N; a.H = d.H; a.W = d.W; a.C = d.C; a.K = d.K; a.R = d.R; a.S = d.S;
    a.st = d.stride; a.pad = d.pad; a.P = P; a.Q = Q;
    const long long npix = (long long)d.N * P * Q, nin = (long long)d.N * d.H * d.W;
    const long long rsc = (long long)d.R * d.S * d.C, rsk = (long long)d.R * d.S * d.K;
    long long M, N, Kr;
    if (p->mode == FWD) { M = npix; N = d.K; Kr = rsc; }
    else if (p->mode == DGRAD) { M = nin; N = d.C; Kr = rsk; }
    else { M = d.K; N = rsc; Kr = npix; }
    if (M >= (1ll << 31) || N >= (1ll << 31) || Kr >= (1ll << 31) || M * N >= (1ll << 40) ||
        npix * d.K >= (1ll << 40) || nin * d.C >= (1ll << 40)) {
        set_error("%s: problem too large", fn);
        return GM_E_ARG;
    }
    a.M = (int)M; a.N = (int)N; a.Kr = (int)Kr;
    a.fd_C = FastDiv((uint32_t)d.C); a.fd_S = FastDiv((uint32_t)d.S); a.fd_K = FastDiv((uint32_t)d.K);
    a.fd_Q = FastDiv((uint32_t)Q); a.fd_P = FastDiv((uint32_t)P); a.fd_W = FastDiv((uint32_t)d.W);
    a.fd_H = FastDiv((uint32_t)d.H); a.fd_st = FastDiv((uint32_t)d.stride);
    pl.vec = (d.C % 4 == 0) && (d.K % 4 == 0);
    const long long big = (M + 127) / 128 * ((N + 127) / 128);
    pl.TM = pl.TN = (big >= cus()) ? 2 : 1;
    const int BM = 64 * pl.TM, BN = 64 * pl.TN;
    const long long tiles = (M + BM - 1) / BM * ((N + BN - 1) / BN);
    a.ktiles = (int)((Kr + kBK - 1) / kBK);
    // split the reduction when the tiles alone leave the chip idle; >= 8 k-tiles per split
    int splits = 1;
    const long long target = 2ll * cus();
    if (tiles < target && a.ktiles >= 16) {
        long long s = (target + tiles - 1) / tiles;
        long long maxs = a.ktiles / 8;
        if (s > maxs) s = maxs;
        if (s > 64) s = 64;
        splits = (int)(s < 1 ? 1 : s);
    }
    a.kt_per_split = (a.ktiles + splits - 1) / splits;
    splits = (a.ktiles + a.kt_per_split - 1) / a.kt_per_split;
    pl.splits = splits;
    pl.grid = dim3((unsigned)((M + BM - 1) / BM), (unsigned)((N + BN - 1) / BN), (unsigned)splits);
    pl.scratch = splits > 1 ? (size_t)splits * M * N * sizeof(float) : 0;
    return GM_OK;
}

// gm_conv2d_f32_affine after its plan: the scratch check and the kernel arguments (the
// descriptor's mode / accumulate / addend and the pointers were checked by the entry, abi.hip)
inline int affine_args(Plan& pl, const gm_conv_f32* p, const float* coef, const float* residual, int relu,
                       void* scratch, size_t scratch_bytes) {
    if (pl.scratch && (!scratch || scratch_bytes < pl.scratch)) {
        set_error("gm_conv2d_f32_affine: scratch %zu bytes < required %zu", scratch_bytes, pl.scratch);
        return GM_E_SCRATCH;
    }
    pl.a.x = p->x; pl.a.w = p->w; pl.a.dy = nullptr; pl.a.out = p->out; pl.a.addend = nullptr;
    pl.a.accumulate = 0;
    pl.a.part = static_cast<float*>(scratch);
    pl.a.coef = coef; pl.a.residual = residual; pl.a.relu = relu != 0;
    return GM_OK;
}

// the split reduction's end of an affine launch (nothing to do for an unsplit plan)
inline int affine_sum(const Plan& pl, hipStream_t st) {
    if (pl.splits <= 1) return GM_OK;
    const long long n = (long long)pl.a.M * pl.a.N;
    long long g = (n + 1023) / 1024;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(k_conv_f32_splitk_sum_affine, dim3((unsigned)(g < 1 ? 1 : g)), dim3(256), 0, st, pl.a.part,
                       pl.splits, n, pl.a.N, pl.a.coef, pl.a.residual, pl.a.relu, pl.a.out);
    return check_launch("k_conv_f32_splitk_sum_affine");
}

}  // namespace
}  // namespace gm
