// conv_igemm.hip: the kernel choice as a value.  plan_conv() decides which kernel serves a
// ConvArgs and everything that follows from the choice (template form, splits, grid, LDS,
// statistics rows, split-K workspace); launch_conv() carries a plan out and decides nothing.  The
// size queries of conv_igemm.hip read the same plan.
#pragma once
#include "conv_kern_halo.h"
#include "conv_kern_igemm.h"
#include "conv_kern_rw.h"
#include "conv_kern_stem.h"

namespace gm {

// zero the output pixels no dgrad class covers (e.g. odd pixels of a 1x1/s2 dgrad), or
// copy the addend there when the dgrad is fused with a gradient join
__global__ void k_zero_bf16(uint16_t* p, size_t n, const uint16_t* src, const uint8_t* msk = nullptr) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i * 8 < n; i += (size_t)gridDim.x * blockDim.x) {
        uint4 v = src ? *(const uint4*)(src + i * 8) : make_uint4(0, 0, 0, 0);
        if (msk) {  // the masked addend: byte i covers these 8 elements
            const unsigned b = msk[i];
            v.x = mask_bf2(v.x, b); v.y = mask_bf2(v.y, b >> 2); v.z = mask_bf2(v.z, b >> 4); v.w = mask_bf2(v.w, b >> 6);
        }
        *(uint4*)(p + i * 8) = v;
    }
}

}  // namespace gm

using namespace gm;

// dx[0, n) = 0, the addend, or the addend where its mask bit is set (k_zero_bf16)
static int fill_uncovered(void* dx, size_t n, const void* addend, const uint8_t* amask, hipStream_t st) {
    k_zero_bf16<<<(int)((n / 8 + 255) / 256 < 4096 ? (n / 8 + 255) / 256 : 4096), 256, 0, st>>>(
        (uint16_t*)dx, n, (const uint16_t*)addend, addend ? amask : nullptr);
    return check_launch("k_zero_bf16");
}

static bool grid_ok(const ConvCls& c, int S);

// the run-time switches of the choice (gm_conv_set_*; A/B runs and tests)
struct ConvKnobs {
    int halo = 1;             // 0: no halo kernels; 2: the 256-pixel form where it is eligible
    int h9 = 1;               // 0: the halo shapes take k_conv_halo; BN << 8 | NB: that form when it fits
    int rw = 1;               // 0: layer-1 shapes take the im2col kernel
    int stem = 1;             // 0: the pixel-pair stem takes the im2col kernel
    int splitk_target = 384;  // workgroups wanted from split-K; 0 disables it
};

constexpr int kTileBias = 1024;  // workgroups wanted before a larger tile is taken
constexpr int kSplitkMinK = 16;  // minimum k-tiles per split
// k_conv_rw is persistent: one workgroup per CU of the MI355X, whatever device plans the launch
// (the statistics bounds of conv_igemm.hip count the same rows)
constexpr int kRwWorkgroups = 256;

enum class ConvKernel { halo256, rw, stem, h9, halo, lean, igemm };

struct ConvPlan {
    ConvKernel kernel = ConvKernel::igemm;
    int BM = 0, BN = 0, NB = 0;      // the kernel's template form (NB: weight-ring stages of h9 / halo)
    int splits = 1;
    int grid = 0, wg = 256;          // workgroups (0: nothing to launch), threads of each
    size_t lds = 0;                  // dynamic LDS bytes
    int tiles_g = 0, tiles_total = 0;
    int tiles_m[kMaxCls] = {}, tile_start[kMaxCls] = {};
    int stats_rows = 0;              // partial rows per 64-channel slice the kernel writes (0: none)
    size_t ws_need = 0;              // split-K workspace that keeps every split the planner wants
    size_t ws_used = 0;              // ... and what this plan uses of the workspace it was given
    bool demask = false;             // the masked addend is materialised over dx first
    bool affine = false;             // the *_affine form of the kernel (a.coef: the evaluation epilogue)
    int rc = GM_OK;                  // not GM_OK: no kernel serves the arguments (err says why)
    const char* err = nullptr;
    HaloArgs halo;
    RwArgs rw;
    StemArgs stem;
};

// partial statistics rows of M output pixels in BM-pixel tiles: one row per tile
static int tile_rows(long long M, int BM) { return (int)((M + BM - 1) / BM); }

enum { T128x128 = 0, T128x64 = 1, T64x64 = 2 };
struct TilePick {
    int tile, splits, tiles;
};

static bool lean_ok(const ConvArgs& a) {
    bool grid = a.C >= 64;
    for (int i = 0; i < a.ncls; ++i) grid = grid && grid_ok(a.cls[i], a.Sw);
    return grid;
}

static long conv_pixels(const ConvArgs& a) {
    long M = 0;
    for (int i = 0; i < a.ncls; ++i) M += (long)a.N * a.cls[i].P * a.cls[i].Q * a.G;
    return M;
}

// the unsplit choice below 128x128
static TilePick small_tile(const ConvArgs& a) {
    return {conv_pixels(a) / 128 * ((a.Nout + 63) / 64) >= kTileBias * 3 / 4 ? T128x64 : T64x64, 1, 0};
}

// enough workgroups to fill 256 CUs with the largest tile that does (128x128: 4
// independent accumulators per wave, so one workgroup per CU keeps the MFMA pipe fed);
// when 128x128 tiles alone are too few (layers 3/4: small M, long K), split K over
// 2-4 workgroups per tile (turnstile hand-off, lean kernel only) instead of shrinking
// the tile, which halves the staged bytes per FLOP against 64x64.
static TilePick pick_tile(const ConvArgs& a, const ConvKnobs& k) {
    int t128 = 0, nkmin = 1 << 30;
    for (int i = 0; i < a.ncls; ++i) {
        const long Mi = (long)a.N * a.cls[i].P * a.cls[i].Q;
        t128 += a.G * (int)((Mi + 127) / 128) * ((a.Nout + 127) / 128);
        const int nk = a.cls[i].ntap * a.C / 64;
        nkmin = nk < nkmin ? nk : nkmin;
    }
    if (a.Nout >= 128 && conv_pixels(a) / 128 * (a.Nout / 128) >= kTileBias / 4) return {T128x128, 1, t128};
    const int want = k.splitk_target;
    if (want > 0 && a.Nout >= 128 && a.C >= 64 && t128 > 0 && lean_ok(a)) {
        int S = (want + t128 - 1) / t128;
        if (S > 4) S = 4;
        while (S > 1 && nkmin / S < kSplitkMinK) --S;  // long enough splits to amortize the hand-off
        // deadlock freedom of the turnstile: a waiting split holds its CU slot while the
        // split it waits on may still be queued behind OTHER launches' waiting splits (the
        // other trunk's stream; another process when ranks share the device) or behind
        // kernels that never yield (RCCL collectives overlapping backward).  Keep the
        // waiting workgroups of one launch (tiles x (S-1)) within two slots per usable CU
        // (CUs minus the reserved ones) divided by the launches that can wait at once -
        // the residency plan's streams x sharers (gm_set_residency; S = 4 at layer 4 timed
        // out with two ranks sharing one GPU before the plan counted them)
        const Residency& rs = residency();
        while (S > 1 && (long)t128 * (S - 1) > (long)usable_cus(conv_cus()) * 2 / (rs.streams * rs.sharers)) --S;
        if (S >= 2) return {T128x128, S, t128};
    }
    return small_tile(a);
}

// turnstile words live in a FIXED region at the start of the workspace (never overlapped
// by any call's slabs, whatever its tile count), so they stay zero between calls that
// share the workspace
constexpr int kMaxSplitTiles = 16384;
constexpr size_t kSplitkFlagBytes = (size_t)kMaxSplitTiles * 4;

static size_t splitk_bytes(const TilePick& p) {
    if (p.splits <= 1) return 0;
    return kSplitkFlagBytes + (size_t)p.tiles * 16 * 256 * 16;  // 128x128: 16 float4 per lane
}

// the halo kernel serves one-class, 3x3 tap grids with offsets in [-1, 1] at stride 1
// and same-size output (forward 3x3/s1/p1 and its input gradient), C a multiple of 64;
// returns the halo LDS bytes (0 = not eligible)
static int halo_bytes(const ConvArgs& a, const ConvKnobs& k, int BM = 128) {
    // C >= 128 (two or more chunks): with one chunk (ResNet layer 1) the whole halo must
    // land before the first k-tile and the im2col kernel measured faster (tools/conv_ab.py)
    if (!k.halo || a.ncls != 1 || a.C < 128 || (a.C & 63) || a.sAh != 1 || a.sAw != 1) return 0;
    const ConvCls& c = a.cls[0];
    if (c.ntap != 9 || c.Rc != 3 || c.Sc != 3 || c.oS != 1 || c.P != a.Hi || c.Q != a.Wi || a.Ho != a.Hi ||
        a.Wo != a.Wi || !grid_ok(c, a.Sw))
        return 0;
    for (int i = 0; i < 3; ++i)
        if (c.cdh[i] < -1 || c.cdh[i] > 1 || c.cdw[i] < -1 || c.cdw[i] > 1) return 0;
    const int H1 = a.Hi + 1, W2 = a.Wi + 2, PQ = c.P * c.Q, M = a.N * PQ;
    int maxpix = 0;
    for (int m0 = 0; m0 < M; m0 += BM) {
        const int m1 = (m0 + BM < M ? m0 + BM : M) - 1;
        const int b0 = m0 / PQ, p0 = (m0 - b0 * PQ) / c.Q;
        const int b1 = m1 / PQ, p1 = (m1 - b1 * PQ) / c.Q;
        const int npix = (b1 * H1 + p1 + 2 - (b0 * H1 + p0) + 1) * W2;
        maxpix = npix > maxpix ? npix : maxpix;
    }
    return (maxpix + 7) / 8 * 1024;
}

// k_conv_stem serves the pixel-pair stem: one-class forward convolutions over 8-channel
// elements with 64 output channels, no padding, strides (2, 1), a 7 x 4 filter and output
// columns <= 128; returns its LDS bytes (0 = not eligible)
static size_t stem_plan(const ConvArgs& a, const ConvKnobs& k, StemArgs& r) {
    if (!k.stem || a.ncls != 1 || a.C != 8 || a.Nout != 64 || a.sAw != 1 || a.sAh != 2) return 0;
    const ConvCls& c = a.cls[0];
    if (c.oS != 1 || c.oH != 0 || c.oW != 0 || c.Q > 128 || c.ntap != a.T || a.Sw != 4 || a.T != 28) return 0;
    for (int tp = 0; tp < c.ntap; ++tp) {  // forward taps without padding: (r, s) = (dh, dw), weight tap tp
        const int rr = tp / a.Sw, ss = tp - rr * a.Sw;
        if (c.tw[tp] != tp || c.dh[tp] != rr || c.dw[tp] != ss) return 0;
    }
    const int R = a.T / a.Sw;
    if ((c.P - 1) * a.sAh + R > a.Hi || c.Q - 1 + a.Sw > a.Wi) return 0;
    if ((size_t)a.N * a.Ho * a.Wo * a.Nout * 2 >= 0x7ffff000u) return 0;
    if ((long long)a.Hi * a.Wi >= (1ll << 27)) return 0;
    r.N = a.N;
    r.P = c.P;
    r.uchunks = 2 * a.Wi;
    if (r.uchunks > 256) return 0;  // two units per iteration over 256 threads x 2 chunks
    r.upitch = r.uchunks * 16;
    r.ichunks = a.Hi * a.Wi;
    // chunks of an even number of rows: about two workgroups per CU over all view groups
    const int target = a.G > 0 ? 512 / a.G : 512;
    const int cpi0 = std::max(1, std::min((c.P + 1) / 2, target / std::max(1, a.N)));
    r.L = (c.P + cpi0 - 1) / cpi0;
    r.L += r.L & 1;
    r.cpi = (c.P + r.L - 1) / r.L;  // no empty chunk
    r.stats_rows = a.N * r.cpi;
    r.stats = nullptr;
    const size_t lds = (size_t)kStemRing * r.upitch + 4 * 8192;
    return lds <= 80 * 1024 ? lds : 0;  // two workgroups per CU
}

// the resident-weight kernel serves one-class 3x3 / stride-1 / same-size convolutions with
// C = Nout = 64 and tap offsets in [-1, 1]; returns its LDS bytes (0 = not eligible)
static size_t rw_plan(const ConvArgs& a, const ConvKnobs& k, RwArgs& r) {
    if (!k.rw || a.ncls != 1 || a.C != 64 || a.Nout != 64 || a.T != 9 || a.sAh != 1 || a.sAw != 1) return 0;
    const ConvCls& c = a.cls[0];
    if (c.ntap != 9 || c.Rc != 3 || c.Sc != 3 || c.oS != 1 || c.P != a.Hi || c.Q != a.Wi || a.Ho != a.Hi ||
        a.Wo != a.Wi || !grid_ok(c, a.Sw) || a.Wi > 128)
        return 0;
    if ((size_t)a.N * a.Ho * a.Wo * a.Nout * 2 >= 0x7ffff000u) return 0;  // 32-bit buffer offsets
    for (int i = 0; i < 3; ++i)
        if (c.cdh[i] < -1 || c.cdh[i] > 1 || c.cdw[i] < -1 || c.cdw[i] > 1) return 0;
    int RT = 128 / a.Wi;
    if (RT > a.Hi) RT = a.Hi;
    while (RT > 1 && a.Hi % RT) --RT;
    r.RT = RT;
    r.tpi = a.Hi / RT;
    r.tiles = a.N * r.tpi;
    r.npix = (RT + 2) * (a.Wi + 2);
    r.nI = (r.npix + 7) / 8;
    if (r.nI > 48) return 0;  // k_conv_rw decodes at most 12 halo instructions per wave
    r.hbytes = r.nI * 1024;
    r.fd_w2 = FastDiv((uint32_t)(a.Wi + 2));
    r.fd_tpi = FastDiv((uint32_t)r.tpi);
    const size_t lds = (size_t)kRwWeightBytes + 2 * (size_t)r.hbytes + 128 * 128;
    return lds <= 160 * 1024 ? lds : 0;
}

// persistent: one workgroup per CU, split evenly over the view groups (workgroups per group)
static int rw_per(const ConvArgs& a, const RwArgs& r) {
    const int per = kRwWorkgroups / a.G;
    return r.tiles < per ? r.tiles : (per > 0 ? per : 1);
}

// (BN, NB) of k_conv_h9 for a shape, as BN << 8 | NB: gm_conv_set_h9(1) = automatic - the
// deepest weight ring (<= 3 stages) of 128-channel tiles that keeps two workgroups per CU; a
// forced form (A/B runs) when it fits.  0 when k_conv_h9 does not take the shape: Nout a
// multiple of BN, at most 48 halo DMA instructions, the halo + the weight stages within half
// the CU's LDS (two workgroups per CU), splits over whole channel chunks.
static int h9_form(const ConvArgs& a, const ConvKnobs& k, int hb, int BNmax, int splits) {
    if (splits > (a.C >> 6)) return 0;
    if (!k.h9 || hb / 1024 > 4 * kH9MaxQ || a.N * a.cls[0].P * a.cls[0].Q >= (1 << 30) / 8) return 0;
    const int budget = 80 * 1024 - 256;
    auto fits = [&](int bn, int nb) { return bn <= BNmax && a.Nout % bn == 0 && hb + nb * bn * 128 <= budget; };
    int f = 0;
    if (k.h9 > 1) {
        f = fits(k.h9 >> 8, k.h9 & 255) ? k.h9 : 0;
    } else {
        for (int nb = 3; nb >= 2 && !f; --nb)
            if (fits(128, nb)) f = 128 << 8 | nb;
        if (!f && fits(64, 4)) f = 64 << 8 | 4;
    }
    switch (f) {  // the forms that are compiled
    case 128 << 8 | 2: case 128 << 8 | 3: case 64 << 8 | 3: case 64 << 8 | 4: case 64 << 8 | 5: return f;
    default: return 0;
    }
}

// 256-pixel halo tiles (one workgroup per CU, BN = 128): eligible when the double
// halo plus a 3-stage weight ring fits the CU's LDS.  Tiles too few to fill the chip
// split K (2-4 ways, >= 16 k-tiles each) through the turnstile when the workspace holds
// the 256x128 slabs.
struct Halo256Plan {
    int hb = 0;        // one halo buffer's LDS bytes (0: not taken)
    int tiles = 0, splits = 1;
    size_t ws = 0;     // split-K workspace bytes (turnstile words + 256x128 fp32 slabs)
};

// the 256-pixel form (gm_conv_set_halo(2)): shapes with fewer 256x128 tiles keep the 128-pixel form;
// K is split when the tiles do not fill the chip
static const int g_h256_mintiles = 192;
static const int g_h256_split = 1;

static Halo256Plan halo256_plan(const ConvArgs& a, const ConvKnobs& k) {
    Halo256Plan p;
    if (k.halo != 2 || a.G != 1 || a.Nout % 128) return p;
    const int hb = halo_bytes(a, k, 256);
    if (hb <= 0 || 2 * hb + 3 * 128 * 128 > 160 * 1024) return p;
    const int M = a.N * a.cls[0].P * a.cls[0].Q;
    p.tiles = (M + 255) / 256 * (a.Nout / 128);
    if (p.tiles < g_h256_mintiles) return p;
    p.hb = hb;
    const int nk = 9 * (a.C >> 6);
    int S = (p.tiles >= 192 || !g_h256_split) ? 1 : 256 / p.tiles;
    S = S > 4 ? 4 : S;
    while (S > 1 && nk / S < 16) --S;
    // waiters within the device's slots (one workgroup per CU here) per concurrent launch: see pick_tile
    const Residency& rs = residency();
    while (S > 1 && (long)p.tiles * (S - 1) > (long)usable_cus(conv_cus()) / (rs.streams * rs.sharers)) --S;
    if (p.tiles > kMaxSplitTiles) S = 1;
    p.splits = S;
    if (S > 1) p.ws = kSplitkFlagBytes + (size_t)p.tiles * 32 * 256 * 16;
    return p;
}

// one class of BM x BN tiles over the halo kernels' single class
static void plan_halo_tiles(const ConvArgs& a, ConvPlan& p, int hb, bool groups) {
    const int M = a.N * a.cls[0].P * a.cls[0].Q;
    p.tiles_m[0] = (M + p.BM - 1) / p.BM;
    p.tile_start[0] = 0;
    p.tiles_g = p.tiles_m[0] * ((a.Nout + p.BN - 1) / p.BN);
    p.tiles_total = p.tiles_g * (groups ? a.G : 1);
    p.grid = p.tiles_total * p.splits;
    p.halo.halo_bytes = hb;
    p.halo.fd_w2 = FastDiv((uint32_t)(a.Wi + 2));
    p.halo.fd_h1 = FastDiv((uint32_t)(a.Hi + 1));
}

// The kernel for a: a pure function of a, the workspace bytes on offer (0 without a workspace),
// the switches, the residency plan and the CU count.
static ConvPlan plan_kernel(const ConvArgs& a, size_t ws_bytes, const ConvKnobs& k) {
    ConvPlan p;
    TilePick t = pick_tile(a, k);
    const Halo256Plan h256 = halo256_plan(a, k);
    p.ws_need = std::max(splitk_bytes(t), h256.ws);
    if (h256.hb > 0) {
        p.kernel = ConvKernel::halo256;
        p.BM = 256; p.BN = 128; p.NB = 3;
        p.splits = h256.splits > 1 && ws_bytes < h256.ws ? 1 : h256.splits;
        p.ws_used = p.splits > 1 ? h256.ws : 0;
        p.wg = 512;
        p.lds = 2 * (size_t)h256.hb + 3 * 128 * 128;
        p.demask = a.amask != nullptr;
        plan_halo_tiles(a, p, h256.hb, false);
        return p;
    }
    if ((p.lds = rw_plan(a, k, p.rw)) > 0) {
        p.kernel = ConvKernel::rw;
        p.stats_rows = rw_per(a, p.rw);  // (a.stats: one partial row per workgroup)
        p.grid = p.stats_rows * a.G;
        return p;
    }
    if ((p.lds = stem_plan(a, k, p.stem)) > 0) {
        p.kernel = ConvKernel::stem;
        // N * cpi workgroups per view group (about two per CU in all), one partial row each
        // (gm_conv2d_fwd_grouped_stats_bf16; no statistics without it: p.stem.stats null)
        p.stats_rows = p.stem.stats_rows;
        p.grid = p.stats_rows * a.G;
        return p;
    }
    if (t.splits > 1 && (ws_bytes < splitk_bytes(t) || t.tiles > kMaxSplitTiles)) t = small_tile(a);
    p.splits = t.splits;  // (split-K is only chosen with 128x128 tiles)
    p.ws_used = splitk_bytes(t);
    const long long Mg = (long long)a.N * a.cls[0].P * a.cls[0].Q;
    const int hb = halo_bytes(a, k);
    if (hb > 0 && hb + 2 * 128 * 128 <= 160 * 1024) {
        // k_conv_h9 when it takes the shape; else k_conv_halo, which has no view groups - those fall
        // to the lean kernel below
        p.BM = 128;
        p.stats_rows = tile_rows(Mg, 128);  // (a.stats: one partial row per 128-pixel tile)
        const int BN = (t.tile == T128x128 || a.Nout >= 128) ? 128 : 64;
        if (const int f = h9_form(a, k, hb, BN, p.splits)) {
            p.kernel = ConvKernel::h9;
            p.BN = f >> 8; p.NB = f & 255;
            p.lds = (size_t)hb + p.NB * (size_t)p.BN * 128;
            plan_halo_tiles(a, p, hb, true);
            return p;
        }
        if (a.G == 1) {
            p.kernel = ConvKernel::halo;
            p.BN = BN;
            // a third weight stage when two workgroups per CU still fit
            p.NB = hb + 3 * BN * 128 <= 80 * 1024 - 256 ? 3 : 2;
            p.lds = (size_t)hb + p.NB * (size_t)BN * 128;
            p.demask = a.amask != nullptr;
            plan_halo_tiles(a, p, hb, false);
            return p;
        }
    }
    p.BM = t.tile == T64x64 ? 64 : 128;
    p.BN = t.tile == T128x128 ? 128 : 64;
    p.stats_rows = tile_rows(Mg, p.BM);  // (a.stats: one partial row per tile of the one class)
    p.demask = a.amask != nullptr;
    for (int i = 0; i < a.ncls; ++i) {
        p.tiles_m[i] = tile_rows((long long)a.N * a.cls[i].P * a.cls[i].Q, p.BM);
        p.tile_start[i] = p.tiles_g;
        p.tiles_g += p.tiles_m[i] * ((a.Nout + p.BN - 1) / p.BN);
    }
    p.tiles_total = p.tiles_g * a.G;  // view groups: G x the tiles of one group
    p.grid = p.tiles_total * p.splits;
    p.lds = (size_t)2 * (p.BM + p.BN) * 128;
    if (lean_ok(a)) {
        p.kernel = ConvKernel::lean;
    } else if (a.G > 1) {
        p.rc = GM_E_UNSUP;
        p.err = "conv: view groups need the lean, halo or resident-weight kernels (C >= 64)";
    } else {
        p.kernel = ConvKernel::igemm;  // (its statistics: none - the entry points refuse G == 1)
        p.lds += kMaxTap * 4 + 12;
    }
    return p;
}

// The evaluation epilogue (a.coef) on the planned kernel: the kernels with an *_affine form keep
// their plan - the LDS-staged ones with room for the fp32 tile, which their epilogue then takes
// without a fallback - and the others decline (gm_conv2d_fwd_affine_ok).
static void plan_epilogue(const ConvArgs& a, ConvPlan& p) {
    if (p.rc != GM_OK) return;
    p.affine = true;
    if ((size_t)a.N * a.Ho * a.Wo * a.Nout * 2 >= 0x7ffff000u) {
        p.rc = GM_E_UNSUP;
        p.err = "conv affine: a group's output past 32-bit offsets";
        return;
    }
    switch (p.kernel) {
    case ConvKernel::rw: return;
    case ConvKernel::h9:
    case ConvKernel::lean: p.lds = std::max(p.lds, (size_t)p.BM * p.BN * 4); return;
    default:
        p.rc = GM_E_UNSUP;
        p.err = "conv affine: the planned kernel (k_conv_halo, k_conv_igemm or k_conv_stem) has no affine "
                "epilogue - run the plain forward and a coefficient-only BatchNorm apply";
    }
}

static ConvPlan plan_conv(const ConvArgs& a, size_t ws_bytes, const ConvKnobs& k) {
    ConvPlan p = plan_kernel(a, ws_bytes, k);
    if (a.coef) plan_epilogue(a, p);
    return p;
}

// one kernel instantiation: grow its dynamic LDS limit when this launch needs more, launch
template <auto Kern, class... Extra>
static int launch_form(const char* name, ConvArgs& a, const ConvPlan& p, hipStream_t st, const Extra&... extra) {
    if (int rc = grant_lds<Kern>(name, p.lds)) return rc;
    Kern<<<p.grid, p.wg, p.lds, st>>>(a, extra...);
    return check_launch(name);
}

// Carries plan p (of plan_conv(a, ws ? ws_bytes : 0, ...)) out: the tile fields of a, the masked
// addend, the launch.  ws: the split-K workspace the plan was made for.
static int launch_conv(ConvArgs& a, const ConvPlan& p, void* ws, hipStream_t st) {
    if (p.rc != GM_OK) {
        set_error("%s", p.err);
        return p.rc;
    }
    if (p.demask && a.amask) {
        // the masked addend materialised over dx (k_zero_bf16's masked copy; every group, contiguous),
        // which then is the addend in place - for the kernels whose epilogue reads no mask
        uint16_t* dx = a.cls[0].out;
        if (int rc = fill_uncovered(dx, (size_t)a.G * a.N * a.Ho * a.Wo * a.Nout, a.addend, a.amask, st)) return rc;
        a.addend = dx;
        a.amask = nullptr;
    }
    if (p.grid == 0) return GM_OK;
    for (int i = 0; i < a.ncls; ++i) {
        a.cls[i].tiles_m = p.tiles_m[i];
        a.cls[i].tile_start = p.tile_start[i];
    }
    a.tiles_g = p.tiles_g;
    a.tiles_total = p.tiles_total;
    a.stats_rows = p.stats_rows;
    a.splits = p.splits;
    if (p.splits > 1) {
        a.spin_limit = spin_limit();
        a.flags = static_cast<unsigned*>(ws);
        a.ws = reinterpret_cast<float*>(static_cast<char*>(ws) + kSplitkFlagBytes);
    }
    const int form = p.BM << 16 | p.BN << 8 | p.NB;
    if (p.affine) {
        switch (p.kernel) {
        case ConvKernel::rw: return launch_form<k_conv_rw<1>>("k_conv_rw_affine", a, p, st, p.rw);
        case ConvKernel::h9:
            switch (form) {
            case 128 << 16 | 128 << 8 | 2: return launch_form<k_conv_h9_affine<128, 2>>("k_conv_h9_affine", a, p, st, p.halo);
            case 128 << 16 | 128 << 8 | 3: return launch_form<k_conv_h9_affine<128, 3>>("k_conv_h9_affine", a, p, st, p.halo);
            case 128 << 16 | 64 << 8 | 3: return launch_form<k_conv_h9_affine<64, 3>>("k_conv_h9_affine", a, p, st, p.halo);
            case 128 << 16 | 64 << 8 | 4: return launch_form<k_conv_h9_affine<64, 4>>("k_conv_h9_affine", a, p, st, p.halo);
            case 128 << 16 | 64 << 8 | 5: return launch_form<k_conv_h9_affine<64, 5>>("k_conv_h9_affine", a, p, st, p.halo);
            }
            break;
        case ConvKernel::lean:
            switch (form) {
            case 128 << 16 | 128 << 8: return launch_form<k_conv_igemm_ut_affine<128, 128>>("k_conv_igemm_affine", a, p, st);
            case 128 << 16 | 64 << 8: return launch_form<k_conv_igemm_ut_affine<128, 64>>("k_conv_igemm_affine", a, p, st);
            case 64 << 16 | 64 << 8: return launch_form<k_conv_igemm_ut_affine<64, 64>>("k_conv_igemm_affine", a, p, st);
            }
            break;
        default: break;
        }
        set_error("conv affine: no compiled kernel for plan form %d x %d x %d", p.BM, p.BN, p.NB);
        return GM_E_UNSUP;
    }
    switch (p.kernel) {
    case ConvKernel::halo256: return launch_form<k_conv_halo<256, 128, 3>>("k_conv_halo", a, p, st, p.halo);
    case ConvKernel::rw: return launch_form<k_conv_rw<0>>("k_conv_rw", a, p, st, p.rw);
    case ConvKernel::stem: return launch_form<k_conv_stem<7, 4>>("k_conv_stem", a, p, st, p.stem);
    case ConvKernel::h9:
        switch (form) {
        case 128 << 16 | 128 << 8 | 2: return launch_form<k_conv_h9<128, 2>>("k_conv_h9", a, p, st, p.halo);
        case 128 << 16 | 128 << 8 | 3: return launch_form<k_conv_h9<128, 3>>("k_conv_h9", a, p, st, p.halo);
        case 128 << 16 | 64 << 8 | 3: return launch_form<k_conv_h9<64, 3>>("k_conv_h9", a, p, st, p.halo);
        case 128 << 16 | 64 << 8 | 4: return launch_form<k_conv_h9<64, 4>>("k_conv_h9", a, p, st, p.halo);
        case 128 << 16 | 64 << 8 | 5: return launch_form<k_conv_h9<64, 5>>("k_conv_h9", a, p, st, p.halo);
        }
        break;
    case ConvKernel::halo:
        switch (form) {
        case 128 << 16 | 128 << 8 | 2: return launch_form<k_conv_halo<128, 128, 2>>("k_conv_halo", a, p, st, p.halo);
        case 128 << 16 | 128 << 8 | 3: return launch_form<k_conv_halo<128, 128, 3>>("k_conv_halo", a, p, st, p.halo);
        case 128 << 16 | 64 << 8 | 2: return launch_form<k_conv_halo<128, 64, 2>>("k_conv_halo", a, p, st, p.halo);
        case 128 << 16 | 64 << 8 | 3: return launch_form<k_conv_halo<128, 64, 3>>("k_conv_halo", a, p, st, p.halo);
        }
        break;
    case ConvKernel::lean:
        switch (form) {
        case 128 << 16 | 128 << 8: return launch_form<k_conv_igemm_ut<128, 128>>("k_conv_igemm", a, p, st);
        case 128 << 16 | 64 << 8: return launch_form<k_conv_igemm_ut<128, 64>>("k_conv_igemm", a, p, st);
        case 64 << 16 | 64 << 8: return launch_form<k_conv_igemm_ut<64, 64>>("k_conv_igemm", a, p, st);
        }
        break;
    case ConvKernel::igemm:
        switch (form | (a.C >= 64)) {  // bit 0: a 64-wide k-tile lies inside one tap
        case 128 << 16 | 128 << 8 | 1: return launch_form<k_conv_igemm<128, 128, true>>("k_conv_igemm", a, p, st);
        case 128 << 16 | 128 << 8: return launch_form<k_conv_igemm<128, 128, false>>("k_conv_igemm", a, p, st);
        case 128 << 16 | 64 << 8 | 1: return launch_form<k_conv_igemm<128, 64, true>>("k_conv_igemm", a, p, st);
        case 128 << 16 | 64 << 8: return launch_form<k_conv_igemm<128, 64, false>>("k_conv_igemm", a, p, st);
        case 64 << 16 | 64 << 8 | 1: return launch_form<k_conv_igemm<64, 64, true>>("k_conv_igemm", a, p, st);
        case 64 << 16 | 64 << 8: return launch_form<k_conv_igemm<64, 64, false>>("k_conv_igemm", a, p, st);
        }
        break;
    }
    set_error("conv: no compiled kernel for plan form %d x %d x %d", p.BM, p.BN, p.NB);
    return GM_E_UNSUP;
}
