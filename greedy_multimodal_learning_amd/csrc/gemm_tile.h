// The per-tile body of the small fp32 MFMA GEMM (gemm_f32.hip has the design notes), shared by
// k_gemm_f32 (one workgroup per tile) and k_gemm_chain (gemm_chain.hip: a persistent grid that
// walks the tiles of two dependent rounds), plus the host-side tile plan both launchers use, so
// every output element sees the same fmaf / MFMA order whichever kernel computed it.
#pragma once
#include "gm_common.h"

namespace gm {

constexpr int kMaxGemm = 6;
typedef float floatx4 __attribute__((ext_vector_type(4)));

// One K-segment of a wave's 16x16 tile: k in [k0, k1) (segment-local), stepping 4.
// Lane (li, lk) reads A[m0+li][k+lk] and B[k+lk][n0+li]; pointers advance by
// 4*ld1 / 4*ld0 per step.  8 steps (32 k) per iteration with the next
// iteration's 16 loads issued before this iteration's 8 MFMAs (register
// double-buffer), so L2 latency hides behind MFMA issue.  Every load is
// unconditional from a clamped, in-range address and the validity select comes
// after it: a "load or constant" select on a per-lane condition makes hipcc branch
// around each load with a vmcnt(0) inside (cdna_hip_programming.md §5 trap 4c),
// i.e. one dependent L2 round trip per k-step.
template <int U>
__device__ __forceinline__ void seg_mma(floatx4& acc, const gm_operand& A, const gm_operand& B,
                                        int m, int n, bool mrow, bool ncol, int lk, int k0, int k1) {
    if (k1 <= k0) return;
    const bool aone = A.ptr == nullptr;
    // an all-ones A operand loads (and ignores) B's in-range elements
    const float* pa = aone ? B.ptr : A.ptr + (long)m * A.ld0 + (long)(k0 + lk) * A.ld1;
    const float* pb = B.ptr + (long)(k0 + lk) * B.ld0 + (long)n * B.ld1;
    const long sa = aone ? 0 : 4l * A.ld1, sb = 4l * B.ld0;
    const bool va = mrow && !aone, vb = ncol;
    const float one = mrow ? 1.0f : 0.0f;
    int k = k0;
    if (k + 4 * U <= k1) {
        float ac[U], bc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ac[u] = pa[u * sa];
            bc[u] = pb[u * sb];
        }
        for (; k + 8 * U <= k1; k += 4 * U) {
            float an[U], bn[U];
            const float* qa = pa + U * sa;
            const float* qb = pb + U * sb;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                an[u] = qa[u * sa];
                bn[u] = qb[u * sb];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(va ? ac[u] : one, vb ? bc[u] : 0.f, acc, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < U; ++u) { ac[u] = an[u]; bc[u] = bn[u]; }
            pa = qa;
            pb = qb;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(va ? ac[u] : one, vb ? bc[u] : 0.f, acc, 0, 0, 0);
        k += 4 * U;
        pa += U * sa;
        pb += U * sb;
    }
    // tail (< 4U k): lanes past k1 re-read the segment's last k and contribute zero
    for (; k < k1; k += 4) {
        const bool in = (k + lk) < k1;
        const long back = in ? 0 : (long)(k + lk - (k1 - 1));
        const float al = pa[-back * (aone ? 0 : A.ld1)];
        const float bl = pb[-back * B.ld0];
        const float av = in ? (va ? al : (aone ? one : 0.f)) : 0.f;
        const float bv = (in && vb) ? bl : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        pa += sa;
        pb += sb;
    }
}

// The same K-segment on 16-k groups with 16-byte loads along k where an operand is
// k-contiguous (A.ld1 == 1 / B.ld0 == 1, 16-B aligned rows): the four MFMAs of a group
// take k = kg + 4*lk + q in MFMA q (any k -> (lane, instruction) assignment is valid
// when A and B agree), so lane lk's float4 at kg + 4*lk feeds all four; a k-strided
// operand loads its four scalars at those same k.  A strided fp32 load touches one
// cache line per lane row for 4 B of it: the float4 form asks the TA for 4x fewer lines.
// UG groups (16*UG k) per load round, the next round in flight under this one's MFMAs.
template <bool VA, bool VB, int UG>
__device__ __forceinline__ void seg_mma_v(floatx4& acc, const gm_operand& A, const gm_operand& B, int m, int n,
                                          bool mrow, bool ncol, int lk, int k0, int k1) {
    const bool aone = A.ptr == nullptr;
    const bool va = mrow && !aone, vb = ncol;
    const float one = mrow ? 1.0f : 0.0f;
    const float* pa = aone ? B.ptr : A.ptr + (long)m * A.ld0;
    const float* pb = B.ptr + (long)n * B.ld1;
    const long sa = aone ? 0 : A.ld1, sb = B.ld0;
    auto load = [&](int kg, float (&a)[4], float (&b)[4]) {
        const int k = kg + 4 * lk;
        if constexpr (VA) {
            const float4 t = *reinterpret_cast<const float4*>(pa + k);
            a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = pa[(long)(k + q) * sa];
        }
        if constexpr (VB) {
            const float4 t = *reinterpret_cast<const float4*>(pb + k);
            b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = pb[(long)(k + q) * sb];
        }
    };
    auto mma = [&](const float (&a)[4], const float (&b)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(va ? a[q] : one, vb ? b[q] : 0.f, acc, 0, 0, 0);
    };
    int kg = k0;
    if (kg + 16 * UG <= k1) {
        float ac[UG][4], bc[UG][4];
#pragma unroll
        for (int g = 0; g < UG; ++g) load(kg + 16 * g, ac[g], bc[g]);
        for (; kg + 32 * UG <= k1; kg += 16 * UG) {
            float an[UG][4], bn[UG][4];
#pragma unroll
            for (int g = 0; g < UG; ++g) load(kg + 16 * (UG + g), an[g], bn[g]);
#pragma unroll
            for (int g = 0; g < UG; ++g) mma(ac[g], bc[g]);
#pragma unroll
            for (int g = 0; g < UG; ++g)
#pragma unroll
                for (int q = 0; q < 4; ++q) { ac[g][q] = an[g][q]; bc[g][q] = bn[g][q]; }
        }
#pragma unroll
        for (int g = 0; g < UG; ++g) mma(ac[g], bc[g]);
        kg += 16 * UG;
    }
    for (; kg + 16 <= k1; kg += 16) {
        float a[4], b[4];
        load(kg, a, b);
        mma(a, b);
    }
    if (kg < k1) seg_mma<4>(acc, A, B, m, n, mrow, ncol, lk, kg, k1);  // < 16 k left
}

// one K-segment: the float4 form where the operands allow it (uniform per problem)
template <int U>
__device__ __forceinline__ void seg_any(int vec, floatx4& acc, const gm_operand& A, const gm_operand& B, int m,
                                        int n, bool mrow, bool ncol, int lk, int k0, int k1) {
    if (k1 <= k0) return;
    const bool va4 = A.ptr != nullptr && A.ld1 == 1 && (A.ld0 & 3) == 0 && ((uintptr_t)A.ptr & 15) == 0;
    const bool vb4 = B.ld0 == 1 && (B.ld1 & 3) == 0 && ((uintptr_t)B.ptr & 15) == 0;
    if (vec == 0 || (!va4 && !vb4)) seg_mma<U>(acc, A, B, m, n, mrow, ncol, lk, k0, k1);
    else if (va4 && vb4) seg_mma_v<true, true, U / 4>(acc, A, B, m, n, mrow, ncol, lk, k0, k1);
    else if (va4) seg_mma_v<true, false, U / 4>(acc, A, B, m, n, mrow, ncol, lk, k0, k1);
    else seg_mma_v<false, true, U / 4>(acc, A, B, m, n, mrow, ncol, lk, k0, k1);
}

// Workgroup tile `wg` of problem p (cfg = TM | TN<<5 | KS<<10, tiles_n workgroup tiles along
// N): the operand rounds, the K-split reduce through `red` and the epilogue.  Called by all
// NW waves of the workgroup; a caller that calls it again must put a workgroup barrier
// between the calls (`red` is still being read by the ks == 0 waves when the others leave).
// poison: every output of the tile is written as NaN (a chain whose hand-off timed out).
template <int NW, int U>
__device__ __forceinline__ void gemm_tile(const gm_gemm& p, int cfg, int tiles_n, int wg, int vec,
                                          floatx4 (*red)[64], bool poison) {
    const int TM = cfg & 31, TN = (cfg >> 5) & 31, KS = (cfg >> 10) & 31;
    const int wm = wg / tiles_n, wn = wg - wm * tiles_n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = wave / KS, ks = wave - tile * KS;
    const int tm = tile / TN, tn = tile - tm * TN;
    const int m0 = (wm * TM + tm) * 16, n0 = (wn * TN + tn) * 16;
    const int li = lane & 15, lk = lane >> 4;
    const int K0 = p.K[0], Ktot = p.K[0] + p.K[1];
    // K range of this split (global k, a multiple of 16 per split)
    const int k16 = (Ktot + 15) >> 4;
    const int per = (k16 + KS - 1) / KS;
    const int kb = min(Ktot, ks * per * 16), ke = min(Ktot, (ks + 1) * per * 16);
    const bool mrow = (m0 + li) < p.M, ncol = (n0 + li) < p.N;
    const int mm = mrow ? m0 + li : 0, nn = ncol ? n0 + li : 0;
    // epilogue operands, in flight with the first operand round (clamped addresses)
    float bias = 0.f, mk[4] = {1.f, 1.f, 1.f, 1.f}, co[4] = {0.f, 0.f, 0.f, 0.f};
    if (ks == 0) {
        if (p.bias) bias = p.bias[nn];
        if (p.mask) {
#pragma unroll
            for (int r = 0; r < 4; ++r) mk[r] = p.mask[(size_t)min(m0 + lk * 4 + r, p.M - 1) * p.ld_mask + nn];
        }
        if (p.accumulate) {
#pragma unroll
            for (int r = 0; r < 4; ++r) co[r] = p.C[(size_t)min(m0 + lk * 4 + r, p.M - 1) * p.ld_c + nn];
        }
    }
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    seg_any<U>(vec, acc, p.A[0], p.B[0], mm, nn, mrow, ncol, lk, kb, min(ke, K0));
    if (p.K[1] > 0)
        seg_any<U>(vec, acc, p.A[1], p.B[1], mm, nn, mrow, ncol, lk, max(kb, K0) - K0, ke - K0);
    if (KS > 1) {
        red[wave][lane] = acc;
        __syncthreads();
        if (ks != 0) return;
        for (int s = 1; s < KS; ++s) {
            const floatx4 o = red[wave + s][lane];
            acc[0] += o[0]; acc[1] += o[1]; acc[2] += o[2]; acc[3] += o[3];
        }
    }
    // C/D map of 16x16x4: col = lane&15, row = (lane>>4)*4 + r
    const int n = n0 + li;
    if (n >= p.N) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + lk * 4 + r;
        float v = acc[r] + bias;
        if (p.act == 1) v = relu_nan(v);
        else if (p.act == 2) v = 1.0f / (1.0f + expf(-v));
        v = mk[r] > 0.f ? v : 0.f;
        if (poison) v = __builtin_nanf("");
        if (m < p.M) p.C[(size_t)m * p.ld_c + n] = co[r] + v;
    }
}

// ---- host side: what gm_gemm_f32 and the chain entry points share -----------------------
// GEMM forms (gm_gemm_set_form A/B knob): waves per workgroup x k-steps per load round
struct GemmForm { int nw, u; };
constexpr GemmForm kForms[] = {{4, 8}, {4, 16}, {8, 16}, {16, 8}};
struct GemmKnobs { int form, vec, outer; };
const GemmKnobs& gemm_knobs();                    // gemm_f32.hip (gm_gemm_set_form)
bool gemm_takes_outer(const gm_gemm& p);          // gm_gemm_f32 would run p on k_gemm_outer
int gemm_check(const gm_gemm& p, int i);          // launch_gemm_f32's argument checks (GM_E_ARG + text)

struct TilePlan { int cfg, tiles_n, tiles; };
// K splits: about two load rounds (8U k) per wave, at most the workgroup's waves; the rest of
// the workgroup's waves spread over 16x16 tiles along N, then M
inline TilePlan plan_tiles(const gm_gemm& p, const GemmForm& f) {
    const int Kt = p.K[0] + p.K[1];
    const int NW = f.nw;
    int KS = 1;
    while (KS < NW && KS * 8 * f.u < Kt) KS *= 2;
    const int mt16 = (p.M + 15) / 16, nt16 = (p.N + 15) / 16;
    int TM = 1, TN = 1;
    while (TM * TN * KS < NW) {
        if (TN < nt16 && (TN <= TM || TM >= mt16)) TN *= 2;
        else if (TM < mt16) TM *= 2;
        else TN *= 2;
    }
    const int tm = (p.M + 16 * TM - 1) / (16 * TM), tn = (p.N + 16 * TN - 1) / (16 * TN);
    return {TM | (TN << 5) | (KS << 10), tn, tm * tn};
}

unsigned chain_faults_read(bool clear);           // gemm_chain.hip

}  // namespace gm
