// Small fp32 GEMMs of the MMTM joint FC on MFMA (gfx950 v_mfma_f32_16x16x4_f32).
//
// The MMTM layers are [B, 2C] x [2C, C'] and [B, C'] x [C', C] with B <= 256 and
// C <= 512 (plus their weight/input gradients): a few MFLOP, L2-resident, so the
// kernel is latency/parallelism-bound, not HBM- or MFMA-bound.  Design:
//   * each wave computes one 16x16 output tile over a K range with the exact-f32
//     MFMA (an fmaf chain: same numerics as the fp32 reference's FMA GEMMs);
//   * a 1024-thread workgroup holds TM x TN tiles x KS K-splits (TM*TN*KS = 16 waves),
//     KS up to 16 so a wave's dependent chain is at most ~64 k (two rounds of loads in
//     flight) - the MMTM GEMMs are L2-latency chains, not MFMA work; split-K partial
//     tiles are summed through LDS in fixed order (deterministic);
//   * operands are generic strided views (ld0 = 0 broadcasts a row, ptr = NULL
//     means an all-ones operand) so transposes, concatenated inputs and bias
//     gradients need no copies; up to 6 problems run in one launch;
//   * fused epilogue: bias, relu / sigmoid, relu-backward mask, accumulate.
#include <cstring>

#include "gemm_tile.h"

namespace gm {

struct GemmArgs {
    gm_gemm p[kMaxGemm];
    int tile_start[kMaxGemm + 1];
    int tiles_n[kMaxGemm];  // workgroup tiles along N
    int cfg[kMaxGemm];      // TM | TN<<5 | KS<<10
    int nprob;
    int vec;  // 1: the float4 K-segment form where the operands allow it (A/B knob)
};

// GEMM forms (gm_gemm_set_form A/B knob, kForms in gemm_tile.h)
static GemmKnobs g_knobs = {1, 1, 1};
const GemmKnobs& gemm_knobs() { return g_knobs; }

// The MMTM GEMMs are dependent-latency chains (kernel arguments -> operand loads ->
// MFMAs -> epilogue loads -> store), not MFMA work: every round trip costs ~1-2 us.  So
// the problem index is the grid's y (no tile-table lookup before the argument loads),
// the epilogue's operands (bias, relu mask, accumulated C) are loaded together with the
// first operand round, and a wave's K range is at most two load rounds.  The tile's
// arithmetic is gemm_tile (gemm_tile.h), shared with k_gemm_chain.
template <int NW, int U>
__global__ __launch_bounds__(NW * 64) void k_gemm_f32(GemmArgs a) {
    __shared__ floatx4 red[NW][64];
    const int pi = blockIdx.y;
    const int wg = blockIdx.x;
    if (wg >= a.tile_start[pi + 1] - a.tile_start[pi]) return;
    gemm_tile<NW, U>(a.p[pi], a.cfg[pi], a.tiles_n[pi], wg, a.vec, red, false);
}

// ---------------------------------------------------------------------------------
// Outer-product shapes: K <= 128 with a large M x N output - the MMTM weight gradients at C5
// (fc_squeeze: dW[2048][24576] = dz^T[2048][32] . sq[32][24576], 201 MB of fp32 output written,
// and read back when accumulating).  k_gemm_f32 gives each wave one 16 x 16 tile and its
// epilogue stores 64-B row segments: 0.5 TB/s on that shape (407 us).  Here a 256-thread
// workgroup owns a 64 x 256 output tile; every thread keeps 8 rows x 8 columns (two float4
// column chunks 128 floats apart, so a wave's stores are whole 512-B row segments) in registers
// and runs an in-order fmaf chain over k, its operands loaded straight from global memory as
// float4s (A: the 8 rows of the thread's row group - the same address across the 32 lanes of
// the group; B: the thread's 8 columns), 4 k-steps in flight.  No LDS: the kernel runs beside
// the weight-gradient stream's one-workgroup-per-CU 156 KB ring kernels, which an LDS-staged
// form (40 KB per workgroup) kept off the CUs - C5 +0.5 ms/step in an A/B although its own
// launches were faster.  Bound: the output write (+ read when accumulating).
constexpr int kOM = 64, kON = 256, kOU = 4;

struct OuterArgs {
    gm_gemm p[kMaxGemm];
    int tiles_m[kMaxGemm];
    int tile_start[kMaxGemm + 1];
};

__global__ __launch_bounds__(256) void k_gemm_outer(OuterArgs a) {
    const int pi = blockIdx.y;
    const gm_gemm& p = a.p[pi];
    const int wg = blockIdx.x;
    if (wg >= a.tile_start[pi + 1] - a.tile_start[pi]) return;
    const int tm = wg % a.tiles_m[pi], tn = wg / a.tiles_m[pi];  // tm fastest: neighbours share B
    const int t = threadIdx.x, cg = t & 31, rg = t >> 5;
    const int m0 = tm * kOM + 8 * rg, n0 = tn * kON + 4 * cg;
    const int K = p.K[0];
    // A[m][k] = A.ptr[m + k * ld1] (ld0 == 1), B[k][n] = B.ptr[k * ld0 + n] (ld1 == 1); rows / columns
    // past M / N read a clamped in-range float4 and are never stored
    const float* pa = p.A[0].ptr + min(m0, p.M - 8);
    const long sa = p.A[0].ld1;
    const float* pb0 = p.B[0].ptr + min(n0, p.N - 4);
    const float* pb1 = p.B[0].ptr + min(n0 + 128, p.N - 4);
    const long sb = p.B[0].ld0;
    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    auto fma8 = [&](const float4& a0, const float4& a1, const float4& b0, const float4& b1) __attribute__((always_inline)) {
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    };
    int k = 0;
    for (; k + kOU <= K; k += kOU) {  // kOU k-steps' loads in flight, then their FMAs in k order
        float4 a0[kOU], a1[kOU], b0[kOU], b1[kOU];
#pragma unroll
        for (int u = 0; u < kOU; ++u) {
            const long ka = (long)(k + u) * sa, kb = (long)(k + u) * sb;
            a0[u] = *reinterpret_cast<const float4*>(pa + ka);
            a1[u] = *reinterpret_cast<const float4*>(pa + ka + 4);
            b0[u] = *reinterpret_cast<const float4*>(pb0 + kb);
            b1[u] = *reinterpret_cast<const float4*>(pb1 + kb);
        }
#pragma unroll
        for (int u = 0; u < kOU; ++u) fma8(a0[u], a1[u], b0[u], b1[u]);
    }
    for (; k < K; ++k) {
        const float4 a0 = *reinterpret_cast<const float4*>(pa + (long)k * sa);
        const float4 a1 = *reinterpret_cast<const float4*>(pa + (long)k * sa + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(pb0 + (long)k * sb);
        const float4 b1 = *reinterpret_cast<const float4*>(pb1 + (long)k * sb);
        fma8(a0, a1, b0, b1);
    }
    // the clamped rows / columns: the thread's registers hold rows min(m0, M - 8) + i and columns
    // min(n0, N - 4) + j; store only the thread's own in-range outputs
    const int mb = min(m0, p.M - 8), nb0 = min(n0, p.N - 4), nb1 = min(n0 + 128, p.N - 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = mb + i;
        if (m < m0 || m >= m0 + 8) continue;  // (a clamped row group: rows another group owns)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int nb = h ? nb1 : nb0, n = n0 + 128 * h;
            if (n >= p.N) continue;
            float* c = p.C + (size_t)m * p.ld_c + nb;
            float4 v = make_float4(acc[i][4 * h], acc[i][4 * h + 1], acc[i][4 * h + 2], acc[i][4 * h + 3]);
            if (nb == n) {  // a whole float4 chunk of this thread
                if (p.accumulate) {
                    const float4 o = *reinterpret_cast<const float4*>(c);
                    v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                }
                *reinterpret_cast<float4*>(c) = v;
            } else {  // the last, clamped chunk: columns nb + q >= n are this thread's
                const float vv[4] = {v.x, v.y, v.z, v.w};
                for (int q = n - nb; q < 4; ++q) c[q] = (p.accumulate ? c[q] : 0.f) + vv[q];
            }
        }
    }
}

// a problem the outer-product kernel takes: one K segment of at most 128, a large output, no
// bias / activation / mask, row-contiguous operands (A[m][k] = A[m + k ld1], B[k][n] = B[k ld0 + n]),
// M >= 8 and N >= 4, float4-aligned operand rows and C rows
static bool outer_ok(const gm_gemm& p) {
    const gm_operand& A = p.A[0];
    const gm_operand& B = p.B[0];
    return p.K[1] == 0 && p.K[0] >= 1 && p.K[0] <= 128 && (long long)p.M * p.N >= (1ll << 20) && p.M >= 8 &&
           p.N >= 4 && !p.bias && !p.mask && p.act == 0 && A.ptr && A.ld0 == 1 && (A.ld1 & 3) == 0 &&
           ((uintptr_t)A.ptr & 15) == 0 && B.ld1 == 1 && (B.ld0 & 3) == 0 && ((uintptr_t)B.ptr & 15) == 0 &&
           (p.ld_c & 3) == 0 && ((uintptr_t)p.C & 15) == 0;
}

bool gemm_takes_outer(const gm_gemm& p) {
    return g_knobs.outer && p.M >= 1 && p.N >= 1 && p.C && p.ld_c >= p.N && p.A[0].ptr && p.B[0].ptr && outer_ok(p);
}

int gemm_check(const gm_gemm& p, int i) {
    GM_REQUIRE(p.M >= 1 && p.N >= 1 && p.K[0] >= 0 && p.K[1] >= 0 && p.K[0] + p.K[1] >= 1,
               "gemm_f32[%d]: bad shape M=%d N=%d K=%d+%d", i, p.M, p.N, p.K[0], p.K[1]);
    GM_REQUIRE(p.C && p.ld_c >= p.N, "gemm_f32[%d]: bad C / ld_c", i);
    GM_REQUIRE(p.act >= 0 && p.act <= 2, "gemm_f32[%d]: bad act %d", i, p.act);
    GM_REQUIRE(!p.mask || p.ld_mask >= p.N, "gemm_f32[%d]: bad ld_mask", i);
    for (int s = 0; s < 2; ++s)
        if (p.K[s] > 0)
            GM_REQUIRE(p.B[s].ptr, "gemm_f32[%d]: segment %d has no B operand", i, s);
    return GM_OK;
}

}  // namespace gm

using namespace gm;

static int launch_gemm_f32(const gm_gemm* in, int nprob, hipStream_t st);

extern "C" int gm_gemm_f32(const gm_gemm* in, int nprob, void* stream) {
    GM_REQUIRE(in && nprob >= 1 && nprob <= kMaxGemm, "gemm_f32: nprob must be 1..%d", kMaxGemm);
    hipStream_t st = as_stream(stream);
    // the outer-product problems (k_gemm_outer) and the rest (k_gemm_f32): independent problems,
    // two launches on one stream
    gm_gemm rest[kMaxGemm];
    int nrest = 0;
    OuterArgs o;
    memset(&o, 0, sizeof(o));
    int nout = 0, maxt = 0;
    for (int i = 0; i < nprob; ++i) {
        const gm_gemm& p = in[i];
        if (gemm_takes_outer(p)) {
            o.p[nout] = p;
            o.tiles_m[nout] = (p.M + kOM - 1) / kOM;
            const int t = o.tiles_m[nout] * ((p.N + kON - 1) / kON);
            o.tile_start[nout + 1] = o.tile_start[nout] + t;
            maxt = t > maxt ? t : maxt;
            ++nout;
        } else {
            rest[nrest++] = p;
        }
    }
    if (nrest) {
        const int rc = launch_gemm_f32(rest, nrest, st);
        if (rc) return rc;
    }
    if (nout) {
        k_gemm_outer<<<dim3(maxt, nout), 256, 0, st>>>(o);
        return check_launch("k_gemm_outer");
    }
    return GM_OK;
}

static int launch_gemm_f32(const gm_gemm* in, int nprob, hipStream_t st) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.nprob = nprob;
    int tiles = 0, maxt = 0;
    for (int i = 0; i < nprob; ++i) {
        const gm_gemm& p = in[i];
        const int rc = gemm_check(p, i);
        if (rc) return rc;
        a.p[i] = p;
        const TilePlan t = plan_tiles(p, kForms[g_knobs.form]);
        a.cfg[i] = t.cfg;
        a.tiles_n[i] = t.tiles_n;
        a.tile_start[i] = tiles;
        tiles += t.tiles;
        if (t.tiles > maxt) maxt = t.tiles;
    }
    a.tile_start[nprob] = tiles;
    a.vec = g_knobs.vec;
    const dim3 grid(maxt, nprob);
    switch (g_knobs.form) {
        case 0: k_gemm_f32<4, 8><<<grid, 256, 0, st>>>(a); break;
        case 1: k_gemm_f32<4, 16><<<grid, 256, 0, st>>>(a); break;
        case 2: k_gemm_f32<8, 16><<<grid, 512, 0, st>>>(a); break;
        default: k_gemm_f32<16, 8><<<grid, 1024, 0, st>>>(a); break;
    }
    return check_launch("k_gemm_f32");
}

extern "C" int gm_gemm_set_form(int form) {
    g_knobs.vec = !(form & 256);    // bit 8: scalar k-steps only
    g_knobs.outer = !(form & 512);  // bit 9: no outer-product kernel (every problem on k_gemm_f32)
    form &= 255;
    GM_REQUIRE(form >= 0 && form < (int)(sizeof(kForms) / sizeof(kForms[0])), "gemm form must be 0..3 (got %d)",
               form);
    g_knobs.form = form;
    return GM_OK;
}
