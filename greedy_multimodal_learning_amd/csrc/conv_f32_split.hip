// Reference-precision trunk convolutions on the bf16 MFMA: split-bf16 contraction
// (bf16x3 / bf16x6).  Same contract as k_conv_f32 (conv_f32.hip): fp32 NHWC activations
// and KRSC weights in, fp32 out, any C >= 1 (element loads for the RGB stem and for
// C % 4 != 0), the dgrad addend, accumulate, and reductions split into fp32 slabs summed
// in a fixed order (k_conv_f32_splitk_sum).  Same inputs, same bits.
//
// Every fp32 operand x is written as bf16 parts, rounded to nearest even:
//   h = bf16(x),  m = bf16(x - h),  l = bf16(x - h - m)        (the subtractions are exact)
// Products of bf16 values are exact in fp32 and v_mfma_f32_32x32x16_bf16 accumulates in
// fp32, so
//   TERMS = 3 (bf16x3): a*b ~ ah*bm + am*bh + ah*bh                    dropped ~ 2^-16
//   TERMS = 6 (bf16x6):     + am*bm + ah*bl + al*bh                    dropped ~ 2^-24
// Term order: ONE accumulator per output tile; within each 16-deep k-step the small
// terms are issued first and ah*bh last (mm, hl, lh, hm, mh, hh).  That order keeps the
// bf16x6 result at the exact-f32 kernel's error against fp64 on every tested shape (the
// figures are in INTEGRATION.md), so the second accumulator for the correction terms (64
// more registers per wave) was not built.
//
// Operands are gathered as fp32 with conv_f32.hip's im2col-on-the-fly addressing
// (conv_f32_common.h), split ONCE per element per tile in registers and stored to LDS as
// separate bf16 planes, all laid out [row][k] (k = reduction index) so that every MFMA
// fragment (lane l: row l&31, k = 8(l>>5)..+7) is one 16-byte ds_read:
//   * FWD A and B, DGRAD A: contiguous along k in global memory; a 16-byte load gives 4 k
//     of one row -> one 8-byte LDS store per plane.
//   * DGRAD B (w[k][r][s][c]), WGRAD A (dy[pix][k]) and B (x patch): contiguous along the
//     non-reduction index; a thread loads the same 4 rows at 2*T consecutive k and
//     transposes in registers -> per row one 4- or 8-byte LDS store per plane; the lanes
//     that share 4 rows sit next to each other so these stores spread over the banks.
// k-tile = 32 fp32 elements, one LDS buffer (<= 60 KB with three planes, so two
// workgroups share a CU and cover each other's barriers) plus a register prefetch of the
// next k-tile.  Row stride = 40 bf16 = 80 B = five 16-byte slots: an ODD number of slots,
// so the 16 rows that one ds_read_b128 lane group covers (any 16 rows that are distinct
// mod 16) land on 16 different slots of the 256-byte bank row - conflict-free.
//
// Non-finite values: a non-finite input gives a non-finite output, but x - bf16(x) is
// NaN for x = +-inf, so the result may be NaN where exact fp32 gives +-inf.  |x| within
// one bf16 ulp of FLT_MAX rounds to bf16 infinity and is out of range the same way.
#include "conv_f32_common.h"

namespace gm {
namespace {

constexpr int kSK = 32;        // k-tile (fp32 elements) = two MFMA k-steps
constexpr int kRow = kSK + 8;  // bf16 per LDS row: 5 (odd) 16-byte slots
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// x -> NP bf16 parts (RNE via the compiler's conversion, v_cvt_pk_bf16_f32)
template <int NP>
__device__ __forceinline__ void split_parts(float v, uint16_t* p) {
    const __bf16 h = (__bf16)v;
    p[0] = __builtin_bit_cast(uint16_t, h);
    const float r1 = v - (float)h;
    const __bf16 m = (__bf16)r1;
    p[1] = __builtin_bit_cast(uint16_t, m);
    if (NP == 3) {
        const float r2 = r1 - (float)m;
        const __bf16 l = (__bf16)r2;
        p[2] = __builtin_bit_cast(uint16_t, l);
    }
}
// two values at once: each part comes out as the packed pair that goes to LDS
template <int NP>
__device__ __forceinline__ void split_pair(float v0, float v1, uint32_t* p) {
    const f32x2 v = {v0, v1};
    const bf16x2 h = __builtin_convertvector(v, bf16x2);
    p[0] = __builtin_bit_cast(uint32_t, h);
    const f32x2 r1 = v - __builtin_convertvector(h, f32x2);
    const bf16x2 m = __builtin_convertvector(r1, bf16x2);
    p[1] = __builtin_bit_cast(uint32_t, m);
    if (NP == 3) {
        const f32x2 r2 = r1 - __builtin_convertvector(m, f32x2);
        const bf16x2 l = __builtin_convertvector(r2, bf16x2);
        p[2] = __builtin_bit_cast(uint32_t, l);
    }
}

// NV consecutive-k values of one row -> each plane's [row][k..k+NV)  (NV = 1, 2 or 4)
template <int NP, int NV>
__device__ __forceinline__ void st_parts(uint16_t* tile, int plane_stride, int row, int k, const float* v) {
    uint16_t* dst = tile + row * kRow + k;
    if (NV == 1) {
        uint16_t q[3];
        split_parts<NP>(v[0], q);
#pragma unroll
        for (int p = 0; p < NP; ++p) dst[p * plane_stride] = q[p];
    } else {
        constexpr int NQ = NV >= 2 ? NV / 2 : 1;
        uint32_t q[NQ][3];
#pragma unroll
        for (int j = 0; j < NV / 2; ++j) split_pair<NP>(v[2 * j], v[2 * j + 1], q[j]);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (NV == 4) *reinterpret_cast<uint2*>(dst + p * plane_stride) = make_uint2(q[0][p], q[NQ - 1][p]);
            else *reinterpret_cast<uint32_t*>(dst + p * plane_stride) = q[0][p];
        }
    }
}

// ---- the kernel ------------------------------------------------------------------
// TERMS: 3 or 6.  VEC: 16-byte operand loads (C % 4 == 0 and K % 4 == 0), else element loads.
// AFF (FWD only): the affine epilogue of gm_conv2d_f32_affine (affine_epilogue, conv_f32_common.h).
template <int MODE, int TERMS, bool VEC, int TM, int TN, bool AFF = false>
__global__ __launch_bounds__(256) void k_conv_f32s(F32Args a) {
    static_assert(!AFF || MODE == FWD, "the affine epilogue is a forward form");
    constexpr int NP = TERMS == 3 ? 2 : 3;
    constexpr int BM = 64 * TM, BN = 64 * TN;
    constexpr int V = VEC ? 4 : 1;
    constexpr int PSA = BM * kRow, PSB = BN * kRow;  // plane strides (bf16 elements)
    __shared__ __attribute__((aligned(16))) uint16_t As[NP * PSA];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[NP * PSB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    // the planner counts k-tiles of kBK; this block reduces [kbeg, kend)
    const int kbeg = blockIdx.z * a.kt_per_split * kBK;
    int kend = kbeg + a.kt_per_split * kBK;
    if (kend > a.Kr) kend = a.Kr;

    // Chunks per thread and k-tile.  Operands contiguous along k (FWD A/B, DGRAD A):
    //   VEC: chunk e = t + 256 i -> row e>>3, 4 k at 4*(e&7);  element: e -> row e>>5, k e&31.
    // Operands contiguous along the row index (WGRAD A/B, DGRAD B), BX rows, NX chunks:
    //   VEC: k = NX*(t % (32/NX)) + i, rows 4*(t / (32/NX))..+3: the lanes that share 4 rows write one
    //   contiguous 64 bytes of each (lanes varying in the row instead would all fall on two bank
    //   groups, 4 rows = 320 B = 64 mod 128), and each load still covers whole 128-byte lines;
    //   element: row t % BX, k t/BX + i*(256/BX).
    constexpr int NA = VEC ? 2 * TM : 8 * TM;
    constexpr int NB = VEC ? 2 * TN : 8 * TN;
    Pix apx[(MODE != WGRAD) ? NA : 1];
    bool aok[(MODE != WGRAD) ? NA : 1];
    if (MODE != WGRAD) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = t + i * 256;
            const int m = m0 + (VEC ? (e >> 3) : (e >> 5));
            aok[i] = m < a.M;
            apx[i] = MODE == FWD ? dec_pix(aok[i] ? m : 0, a.fd_Q, a.fd_P, a.Q, a.P)
                                 : dec_pix(aok[i] ? m : 0, a.fd_W, a.fd_H, a.W, a.H);
        }
    }
    // row-index-contiguous operands: this thread's row(s) and first k within the tile
    const int am = VEC ? 4 * (t / (kSK / NA)) : t % BM;
    const int ak = VEC ? NA * (t % (kSK / NA)) : t / BM;
    const int bn = VEC ? 4 * (t / (kSK / NB)) : t % BN;
    const int bk = VEC ? NB * (t % (kSK / NB)) : t / BN;
    constexpr int AKS = VEC ? 1 : 256 / BM, BKS = VEC ? 1 : 256 / BN;  // k step between chunks
    // B-operand column decode for WGRAD (cols are (r, s, c)), fixed per thread
    int bh = 0, bw = 0, bc = 0;
    bool bok = false;
    if (MODE == WGRAD) {
        const int n = n0 + bn;
        bok = n < a.N;
        const unsigned rs = a.fd_C.div((unsigned)(bok ? n : 0));
        bc = (bok ? n : 0) - (int)rs * a.C;
        const unsigned r = a.fd_S.div(rs);
        bh = (int)r - a.pad;
        bw = (int)(rs - r * a.S) - a.pad;
    }

    float ra[NA][V], rb[NB][V];
    auto ld4 = [](const float* p, bool ok, float* o) {
        if (VEC) {
            const float4 v = ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        } else {
            o[0] = ok ? *p : 0.f;
        }
    };
    auto load = [&](int kb) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if (MODE != WGRAD) {
                const int e = t + i * 256;
                const int kk = kb + (VEC ? 4 * (e & 7) : (e & 31));
                ld_a<MODE, V>(a, apx[i], aok[i] && kk < kend, kk, ra[i]);
            } else {  // A(m = k, kk = pix) = dy[pix][k]
                const int kk = kb + ak + i * AKS;
                const int m = m0 + am;
                const bool ok = kk < kend && m < a.M;
                ld4(a.dy + (long long)(ok ? kk : 0) * a.K + (ok ? m : 0), ok, ra[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (MODE == FWD) {  // B(kk, n) = w[n][kk]: along kk
                const int e = t + i * 256;
                const int n = n0 + (VEC ? (e >> 3) : (e >> 5));
                const int kk = kb + (VEC ? 4 * (e & 7) : (e & 31));
                const bool ok = n < a.N && kk < kend;
                ld4(a.w + (long long)(ok ? n : 0) * a.Kr + (ok ? kk : 0), ok, rb[i]);
            } else if (MODE == DGRAD) {  // B(kk = (r,s,k), n = c) = w[k][r][s][c]: along n
                const int kk = kb + bk + i * BKS;
                const int n = n0 + bn;
                const bool ok = n < a.N && kk < kend;
                const unsigned rs = a.fd_K.div((unsigned)(ok ? kk : 0));
                const int k = (ok ? kk : 0) - (int)rs * a.K;
                ld4(a.w + ((long long)k * a.R * a.S + rs) * a.C + (ok ? n : 0), ok, rb[i]);
            } else {  // WGRAD: B(kk = pix, n = (r,s,c)) = x patch: along n
                const int kk = kb + bk + i * BKS;
                if (kk < kend && bok) {
                    const Pix px = dec_pix((unsigned)kk, a.fd_Q, a.fd_P, a.Q, a.P);
                    ld_x<V>(a, px.n, px.a * a.st + bh, px.b * a.st + bw, bc, rb[i]);
                } else {
#pragma unroll
                    for (int j = 0; j < V; ++j) rb[i][j] = 0.f;
                }
            }
        }
    };
    auto store = [&]() {
        if (MODE != WGRAD) {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int e = t + i * 256;
                if (VEC) st_parts<NP, 4>(As, PSA, e >> 3, 4 * (e & 7), ra[i]);
                else st_parts<NP, 1>(As, PSA, e >> 5, e & 31, ra[i]);
            }
        } else if (VEC) {  // transpose: row am + j gets its NA consecutive k
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v[NA];
#pragma unroll
                for (int i = 0; i < NA; ++i) v[i] = ra[i][j];
                st_parts<NP, NA>(As, PSA, am + j, ak, v);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NA; ++i) st_parts<NP, 1>(As, PSA, am, ak + i * AKS, ra[i]);
        }
        if (MODE == FWD) {
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int e = t + i * 256;
                if (VEC) st_parts<NP, 4>(Bs, PSB, e >> 3, 4 * (e & 7), rb[i]);
                else st_parts<NP, 1>(Bs, PSB, e >> 5, e & 31, rb[i]);
            }
        } else if (VEC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v[NB];
#pragma unroll
                for (int i = 0; i < NB; ++i) v[i] = rb[i][j];
                st_parts<NP, NB>(Bs, PSB, bn + j, bk, v);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NB; ++i) st_parts<NP, 1>(Bs, PSB, bn, bk + i * BKS, rb[i]);
        }
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int li = lane & 31, lk = lane >> 5;
    if (kbeg < kend) {
        load(kbeg);
        store();
        __syncthreads();
        for (int kb = kbeg; kb < kend; kb += kSK) {
            const bool more = kb + kSK < kend;
            if (more) load(kb + kSK);
#pragma unroll
            for (int ks = 0; ks < kSK; ks += 16) {
                bf16x8 fa[TM][NP], fb[TN][NP];
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int p = 0; p < NP; ++p)
                        fa[i][p] = *reinterpret_cast<const bf16x8*>(
                            &As[p * PSA + (wm * 32 * TM + i * 32 + li) * kRow + ks + 8 * lk]);
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int p = 0; p < NP; ++p)
                        fb[j][p] = *reinterpret_cast<const bf16x8*>(
                            &Bs[p * PSB + (wn * 32 * TN + j * 32 + li) * kRow + ks + 8 * lk]);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        floatx16 c = acc[i][j];
                        if (NP == 3) {  // planes 0 = h, 1 = m, 2 = l; smallest terms first
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[j][1], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][NP - 1], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][NP - 1], fb[j][0], c, 0, 0, 0);
                        }
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][1], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[j][0], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][0], c, 0, 0, 0);
                        acc[i][j] = c;
                    }
            }
            __syncthreads();  // every wave is done reading this k-tile
            if (more) {
                store();
                __syncthreads();
            }
        }
    }

    // C/D map of 32x32: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const bool split = gridDim.z > 1;
    float* dst = split ? a.part + (size_t)blockIdx.z * a.M * a.N : a.out;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * 32 * TN + j * 32 + li;
            if (n >= a.N) continue;
            float sc = 0.f, sh = 0.f;  // AFF: the lane's column coefficients, once per 32-column block
            if (AFF && !split) {
                sc = a.coef[n];
                sh = a.coef[a.N + n];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m >= a.M) continue;
                const size_t o = (size_t)m * a.N + n;
                float v = acc[i][j][r];
                if (AFF) {  // (split: the sum kernel applies it)
                    if (!split) v = affine_epilogue(v, sc, sh, a.residual, o, a.relu);
                } else if (!split) {
                    if (a.addend) v += a.addend[o];
                    if (a.accumulate) v += dst[o];
                }
                dst[o] = v;
            }
        }
}

// The planner is make_plan (conv_f32_common.h): same tile sizes (but for narrow N, below),
// same splits and so the same scratch as the exact kernel.  Its splits are counted in k-tiles of kBK = 16; where
// an odd count per split can be made even without changing the number of splits it is,
// so that no split ends on half a 32-deep tile.
int make_plan_split(const gm_conv_f32* p, int terms, Plan& pl, const char* fn) {
    if (terms != 3 && terms != 6) {
        set_error("%s: terms must be 3 (bf16x3) or 6 (bf16x6), got %d", fn, terms);
        return GM_E_ARG;
    }
    if (!p) {
        set_error("%s: null descriptor (terms=%d)", fn, terms);
        return GM_E_ARG;
    }
    const int rc = make_plan(p, pl, fn);
    if (rc) return rc;
    F32Args& a = pl.a;
    // N <= 64 (the 64-channel layers): a 128-wide tile would be half padding.  The 128 x 64
    // form keeps the tile count, so make_plan's splits and scratch stand; the grid is
    // recomputed here from the tile sizes in force, not taken on trust.
    if (pl.TN == 2 && a.N <= 64) pl.TN = 1;
    // splits are counted in k-tiles of kBK = 16: make an odd count per split even where
    // that leaves the number of splits (and so the scratch) as planned
    if (pl.splits > 1 && (a.kt_per_split & 1)) {
        const int even = a.kt_per_split + 1;
        if ((a.ktiles + even - 1) / even == pl.splits) a.kt_per_split = even;
    }
    const unsigned gx = (unsigned)((a.M + 64 * pl.TM - 1) / (64 * pl.TM));
    const unsigned gy = (unsigned)((a.N + 64 * pl.TN - 1) / (64 * pl.TN));
    const unsigned gz = (unsigned)((a.ktiles + a.kt_per_split - 1) / a.kt_per_split);
    if (gx != pl.grid.x || gy != pl.grid.y || gz != (unsigned)pl.splits) {
        set_error("%s: split plan (%u x %u tiles, %u splits) left the shared plan (%u x %u, %d)", fn, gx, gy, gz,
                  pl.grid.x, pl.grid.y, pl.splits);
        return GM_E_UNSUP;
    }
    pl.grid = dim3(gx, gy, gz);
    return GM_OK;
}

template <int MODE, int TERMS>
void launch(const Plan& pl, hipStream_t st) {
#define GM_F32S_L(V, TM, TN) \
    hipLaunchKernelGGL((k_conv_f32s<MODE, TERMS, V, TM, TN>), pl.grid, dim3(256), 0, st, pl.a)
    if (pl.vec) {
        if (pl.TM == 2 && pl.TN == 2) GM_F32S_L(true, 2, 2);
        else if (pl.TM == 2) GM_F32S_L(true, 2, 1);
        else GM_F32S_L(true, 1, 1);
    } else {
        if (pl.TM == 2 && pl.TN == 2) GM_F32S_L(false, 2, 2);
        else if (pl.TM == 2) GM_F32S_L(false, 2, 1);
        else GM_F32S_L(false, 1, 1);
    }
#undef GM_F32S_L
}

template <int TERMS>
void launch_affine(const Plan& pl, hipStream_t st) {
#define GM_F32S_L(V, TM, TN) \
    hipLaunchKernelGGL((k_conv_f32s<FWD, TERMS, V, TM, TN, true>), pl.grid, dim3(256), 0, st, pl.a)
    if (pl.vec) {
        if (pl.TM == 2 && pl.TN == 2) GM_F32S_L(true, 2, 2);
        else if (pl.TM == 2) GM_F32S_L(true, 2, 1);
        else GM_F32S_L(true, 1, 1);
    } else {
        if (pl.TM == 2 && pl.TN == 2) GM_F32S_L(false, 2, 2);
        else if (pl.TM == 2) GM_F32S_L(false, 2, 1);
        else GM_F32S_L(false, 1, 1);
    }
#undef GM_F32S_L
}

template <int TERMS>
void launch_mode(int mode, const Plan& pl, hipStream_t st) {
    if (mode == FWD) launch<FWD, TERMS>(pl, st);
    else if (mode == DGRAD) launch<DGRAD, TERMS>(pl, st);
    else launch<WGRAD, TERMS>(pl, st);
}

}  // namespace

// gm_conv2d_f32_affine, terms = 3 / 6 (the entry and its argument checks: abi.hip)
int conv_f32_affine_split(const gm_conv_f32* p, int terms, const float* coef, const float* residual, int relu,
                          void* scratch, size_t scratch_bytes, void* stream) {
    Plan pl;
    int rc = make_plan_split(p, terms, pl, "gm_conv2d_f32_affine");
    if (rc) return rc;
    if ((rc = affine_args(pl, p, coef, residual, relu, scratch, scratch_bytes))) return rc;
    hipStream_t st = as_stream(stream);
    if (terms == 3) launch_affine<3>(pl, st);
    else launch_affine<6>(pl, st);
    if ((rc = check_launch("k_conv_f32s<affine>"))) return rc;
    return affine_sum(pl, st);
}

}  // namespace gm

using namespace gm;

extern "C" size_t gm_conv2d_f32_split_scratch(const gm_conv_f32* p, int terms) {
    Plan pl;
    if (make_plan_split(p, terms, pl, "gm_conv2d_f32_split_scratch")) return 0;
    return pl.scratch;
}

extern "C" int gm_conv2d_f32_split(const gm_conv_f32* p, int terms, void* scratch, size_t scratch_bytes,
                                   void* stream) {
    Plan pl;
    int rc = make_plan_split(p, terms, pl, "gm_conv2d_f32_split");
    if (rc) return rc;
    GM_REQUIRE(p->out, "gm_conv2d_f32_split: null output");
    GM_REQUIRE(p->mode == WGRAD ? (p->x && p->dy) : p->mode == FWD ? (p->x && p->w) : (p->dy && p->w),
               "gm_conv2d_f32_split: null operand for mode %d", p->mode);
    GM_REQUIRE(!p->addend || p->mode == DGRAD, "gm_conv2d_f32_split: addend is a dgrad option");
    if (pl.scratch) {
        if (!scratch || scratch_bytes < pl.scratch) {
            set_error("gm_conv2d_f32_split: scratch %zu bytes < required %zu", scratch_bytes, pl.scratch);
            return GM_E_SCRATCH;
        }
    }
    pl.a.x = p->x; pl.a.w = p->w; pl.a.dy = p->dy; pl.a.out = p->out; pl.a.addend = p->addend;
    pl.a.accumulate = p->accumulate;
    pl.a.part = static_cast<float*>(scratch);
    hipStream_t st = as_stream(stream);
    if (terms == 3) launch_mode<3>(p->mode, pl, st);
    else launch_mode<6>(p->mode, pl, st);
    if ((rc = check_launch("k_conv_f32s"))) return rc;
    if (pl.splits > 1) {
        const long long n = (long long)pl.a.M * pl.a.N;
        long long g = (n + 1023) / 1024;
        if (g > 8192) g = 8192;
        hipLaunchKernelGGL(k_conv_f32_splitk_sum, dim3((unsigned)(g < 1 ? 1 : g)), dim3(256), 0, st, pl.a.part,
                           pl.splits, n, p->addend, p->accumulate, p->out);
        return check_launch("k_conv_f32_splitk_sum");
    }
    return GM_OK;
}
