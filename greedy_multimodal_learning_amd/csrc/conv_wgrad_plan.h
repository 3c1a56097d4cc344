// conv_wgrad.hip: the weight gradient's kernel choice as a value.  plan_wgrad() decides which
// kernel serves a descriptor and everything that follows from the choice (template form, splits,
// grid, LDS, the reduction, scratch bytes); launch_wgrad() in conv_wgrad.hip carries a plan out
// and decides nothing.  The scratch queries read the same plan.  Host code only.
#pragma once
#include <algorithm>

#include "conv_kern_wgrad4.h"
#include "conv_kern_whalo.h"
#include "conv_kern_wring.h"
#include "conv_kern_wstem.h"

namespace gm {

// the run-time switches of the choice (gm_conv_set_wgrad_*; A/B runs and tests)
struct WgradKnobs {
    // operand staging of k_conv_wgrad4 (its WR argument): 0 LDS-DMA, 1 register-staged, 2
    // register-staged for 1x1 filters only.  Isolated (tools/trunk_table.py) the register-staged
    // form is faster on the 1x1/s2 downsample gradients (16.6-18.7 vs 18.0-19.6 us) and slower on
    // every 3x3 shape (layer 4 64.6 -> 73.6 us, conv family 0.195 -> 0.191); in the step, where the
    // weight gradients run beside the input-gradient chain, the all-register form measured 0.4 %
    // faster on average over nine interleaved pairs, within the box-to-box noise.
    int staging = 2;
    // the dedicated 3x3 kernels: bit 1 = k_wgrad_halo64 for 3x3 / s1 / p1 shapes with W <= 62 and
    // 64 channels (layer 1), bit 2 = also for 128 channels (layer 2), bit 3 = up to 512; bit 4 =
    // k_wgrad_ring for the other 3x3 shapes with K % 128 == 0 and C a power of two >= 32 (layers
    // 3 / 4 and the strided first convolutions); otherwise k_conv_wgrad4.  Default 22 = bits 1, 2
    // and 4 (r04, B = 64 two-view step: layer 1 61.9 -> 44.9 us and layer 2 54.6 -> 46.6 us per
    // launch with the sum; step 3.98 -> 3.91 ms against bit 1 alone).
    int loop = 22;
    int stem = 1;  // 0: the pixel-pair stem's weight gradient takes k_conv_wgrad4
};

enum class WgradKernel { stem, halo64, ring, wgrad4 };
enum class WgradReduce { none, sum, crop };  // after the kernel: nothing, k_wgrad_sum, k_wgrad_reduce

constexpr int kWTap = 49;  // taps the entry points accept

struct WgradPlan {
    WgradKernel kernel = WgradKernel::wgrad4;
    gm_conv_desc_hw d{};             // what was planned: the descriptor, the view groups and the
    int G = 1, c_real = 0;           // input channels of the gradient (< C: cropped by the reduction)
    int P = 0, Q = 0;                // output rows and columns
    int tiles_k = 0, tiles_n = 0;    // tiles over output channels and (tap, channel) columns
    int splits = 1, per = 0;         // partial slabs, and per split: 64-pixel steps (wgrad4, ring),
                                     // super-rows (halo64) or output rows (stem: L)
    int mt = 1, nt = 1, wr = 0;      // wgrad4: k_conv_wgrad4<mt, nt, wr>
    int pp = 0;                      // halo64: k_wgrad_halo64<3, pp>
    int cpi = 0;                     // stem: chunks of L output rows per image
    bool bn = false;                 // stem: k_wgrad_stem_bn, dy formed in the loader
    int grid = 0, wg = 256;          // workgroups, threads of each
    size_t lds = 0;                  // dynamic LDS bytes
    size_t slab = 0;                 // floats of one partial slab (one group's padded gradient)
    bool direct = false;             // the kernel writes (or accumulates into) dw itself
    WgradReduce reduce = WgradReduce::sum;
    size_t scratch = 0;              // scratch bytes this plan uses: G x splits x slab floats, 0 if direct
    int rc = GM_OK;                  // not GM_OK: no kernel serves the arguments (err says why)
    const char* err = nullptr;
};

// workgroups k_conv_wgrad4's splits aim at: two per CU of the MI355X
constexpr int kWgrad4TargetWgs = 512;
// k_wgrad_halo64's workgroups per launch, all view groups and channel tiles together: 128 - half the
// CUs: the launch runs on the weight-gradient stream beside the input-gradient chain, and one
// workgroup per CU (512 threads, 81 KB of LDS) left no room on any CU for that chain's BN
// finalize / apply launches (C2, in the step: 64 / 96 / 128 / 160 / 256 workgroups = 3.80 /
// 3.67 / 3.63 / 3.63 / 3.70 ms; as k_wgrad_ring's half-CU grid)
constexpr int kHalo64Wgs = 128;

// what follows from a plan's tiles and splits once its kernel's launch form is known
static void plan_launch(WgradPlan& p, WgradKernel kernel, int wg, size_t lds, size_t slab, bool direct) {
    p.kernel = kernel; p.wg = wg; p.lds = lds; p.slab = slab; p.direct = direct;
    p.grid = p.tiles_k * p.tiles_n * p.splits * p.G;
    p.reduce = p.direct ? WgradReduce::none : (p.c_real == p.d.C ? WgradReduce::sum : WgradReduce::crop);
    p.scratch = p.direct ? 0 : (size_t)p.G * p.splits * p.slab * sizeof(float);
}

// k_conv_wgrad4 serves every shape the entry points accept
static void plan_wgrad4(WgradPlan& w, const WgradKnobs& k) {
    const gm_conv_desc_hw* d = &w.d;
    w.P = (d->H + 2 * d->pad_h - d->R) / d->stride_h + 1;
    w.Q = (d->W + 2 * d->pad_w - d->S) / d->stride_w + 1;
    const int M = d->N * w.P * w.Q;
    const int steps = (M + 63) / 64;
    const int TC = d->R * d->S * d->C;
    // 128 x 128 tiles where the shape allows (256-row / 256-column tiles at one workgroup per
    // CU measured 1.2-1.6x slower in round 2 and were dropped)
    w.mt = d->K >= 128 ? 2 : 1;
    w.nt = TC >= 128 ? 2 : 1;
    w.wr = k.staging == 1 || (k.staging == 2 && d->R * d->S == 1);
    w.tiles_k = (d->K + 64 * w.mt - 1) / (64 * w.mt);
    w.tiles_n = (TC + 64 * w.nt - 1) / (64 * w.nt);
    const int tiles = w.tiles_k * w.tiles_n * w.G;  // the groups' tiles share the chip
    const int min_steps = 8;
    int want = kWgrad4TargetWgs > tiles ? kWgrad4TargetWgs / tiles : 1;
    if (tiles >= 256) want = 1;  // the chip is full: no partial slabs
    if (want > steps / min_steps) want = steps / min_steps > 0 ? steps / min_steps : 1;
    if (want < 1) want = 1;
    w.per = (steps + want - 1) / want;
    w.splits = (steps + w.per - 1) / w.per;
    plan_launch(w, WgradKernel::wgrad4, 256, (size_t)2 * 64 * 2 * (64 * w.mt + 64 * w.nt), (size_t)d->K * TC,
                w.splits == 1 && w.c_real == d->C);
}

// k_wgrad_stem serves the pixel-pair stem: 8-channel pairs, 64 output channels, a 7 x 4
// filter, strides (2, 1), no padding, output rows of a multiple of 16 and <= 128 pixels
static bool plan_stem(WgradPlan& w, const WgradKnobs& k) {
    const gm_conv_desc_hw* d = &w.d;
    if (!k.stem || d->C != 8 || d->K != 64 || d->R != 7 || d->S != 4 || d->stride_h != 2 || d->stride_w != 1 ||
        d->pad_h != 0 || d->pad_w != 0 || d->N < 1 || d->H < 7 || d->W < 4)
        return false;
    const int P = (d->H - 7) / 2 + 1, Q = d->W - 3;
    if (Q % 16 != 0 || Q > 128 || 2 * d->W > 448 || (long long)d->H * d->W >= (1ll << 27)) return false;
    if ((long long)d->N * P * Q * 64 >= (1ll << 31)) return false;
    w.P = P; w.Q = Q;
    w.tiles_k = w.tiles_n = 1;
    const int target = 512 / w.G > 0 ? 512 / w.G : 1;
    const int cpi0 = std::max(1, std::min(P, target / d->N));
    w.per = (P + cpi0 - 1) / cpi0;
    w.per += w.per & 1;  // even: the BN form's pooled-row schedule starts on an even row
    w.cpi = (P + w.per - 1) / w.per;
    w.splits = d->N * w.cpi;
    // one wave per tap row; LDS: two dy tiles and a ring of 8 two-row units
    plan_launch(w, WgradKernel::stem, 448, (size_t)2 * Q * 128 + (size_t)8 * 2 * d->W * 16, (size_t)64 * 224, false);
    return true;
}

// k_wgrad_halo64 serves 3x3 / s1 / p1 shapes with W <= 62: image rows of PP = 16, 32 or 64
// positions (PP >= W + 2), 64 / PP of them per super-row
static bool plan_halo64(WgradPlan& w, const WgradKnobs& k) {
    const gm_conv_desc_hw* d = &w.d;
    // bit 1: 64 channels (layer 1), bit 2: up to 128 (layer 2), bit 3: up to 512 (layers 3, 4)
    const int maxc = (k.loop & 8) ? 512 : ((k.loop & 4) ? 128 : 64);
    const int pp = d->W + 2 <= 16 ? 16 : (d->W + 2 <= 32 ? 32 : 64);
    if (!((k.loop & 2) && d->R == 3 && d->S == 3 && d->stride_h == 1 && d->stride_w == 1 && d->pad_h == 1 &&
          d->pad_w == 1 && d->C % 64 == 0 && d->K % 64 == 0 && d->C <= maxc && d->K <= maxc && d->W <= 62 &&
          d->W >= 1 && d->H >= 64 / pp && d->N >= 1 &&
          (long long)d->N * d->H * d->W * (d->C > d->K ? d->C : d->K) < (1ll << 31)))
        return false;
    w.P = d->H; w.Q = d->W; w.pp = pp;
    w.tiles_k = d->K / 64;
    w.tiles_n = d->C / 64;
    const int srows = (d->N * d->H + 64 / pp - 1) / (64 / pp);
    const int sp = std::max(1, kHalo64Wgs / (w.tiles_k * w.tiles_n * w.G));
    w.splits = std::min(sp, srows);
    w.per = (srows + w.splits - 1) / w.splits;
    constexpr int D = 3;  // super-rows of LDS-DMA in flight
    plan_launch(w, WgradKernel::halo64, 512, (size_t)(D + 3) * 8192 + (size_t)(D + 1) * (8192 + 256),
                (size_t)d->K * 9 * d->C, false);
    return true;
}

// k_wgrad_ring serves 3x3 shapes (any stride / padding) with K % 128 == 0 and C a power of two
// >= 32.  Its grid: tiles x splits sized to HALF the CUs.  The ring runs on the weight-gradient
// stream beside the main chain's input-gradient convolutions and BatchNorms, and a workgroup holds
// its CU's LDS (156 KB): one per CU starved the main chain (C2 step 3.94 ms against 3.85 without
// the ring), half the CUs left the other half to it (3.75 ms; 64 / 96 / 160 / 192 / 224 workgroups:
// 3.77 / 3.77 / 3.80 / 3.80 / 3.80 ms, r05 interleaved A/B).  Alone a launch then takes longer (conv
// family 0.218 vs 0.228 isolated).  Measured and dropped (r05): 6 slots of 32 pixels (+0.06-0.24
// ms/step), 2 slots.
static bool plan_ring(WgradPlan& w, const WgradKnobs& k) {
    const gm_conv_desc_hw* d = &w.d;
    if (!(k.loop & 16) || d->R != 3 || d->S != 3 || d->K < 128 || d->K % 128 != 0 || log2_exact(d->C) < 5) return false;
    const int P = (d->H + 2 * d->pad_h - 3) / d->stride_h + 1;
    const int Q = (d->W + 2 * d->pad_w - 3) / d->stride_w + 1;
    if (P < 1 || Q < 1 || d->N < 1) return false;
    const long long M = (long long)d->N * P * Q;
    if (M * d->K >= (1ll << 31) || (long long)d->N * d->H * d->W * d->C >= (1ll << 31)) return false;
    w.P = P; w.Q = Q;
    w.tiles_k = d->K / 128;
    w.tiles_n = d->C / 32;  // 9 C / 288
    constexpr int bk = ring::BK;
    const int steps = ((int)M + bk - 1) / bk;
    int want = (conv_cus() / 2) / (w.tiles_k * w.tiles_n * w.G);
    if (want > steps / (512 / bk)) want = steps / (512 / bk);  // >= 512 pixels per split
    if (want < 1) want = 1;
    w.per = (steps + want - 1) / want;
    w.splits = (steps + w.per - 1) / w.per;
    plan_launch(w, WgradKernel::ring, 512, ring::LDS, (size_t)d->K * 9 * d->C, w.splits == 1);
    return true;
}

// The kernel for (d, G, c_real): a pure function of them, the switches and the CU count - the only
// place that tests eligibility.  The dedicated kernels write whole gradients, so a cropped one
// (c_real < C: the RGB stem's padded channels) takes k_conv_wgrad4 and ends in k_wgrad_reduce.
static WgradPlan plan_wgrad(const gm_conv_desc_hw* d, int G, int c_real, const WgradKnobs& k) {
    WgradPlan p;
    p.d = *d; p.G = G; p.c_real = c_real;
    if (c_real == d->C && (plan_stem(p, k) || plan_halo64(p, k) || plan_ring(p, k))) return p;
    plan_wgrad4(p, k);
    return p;
}

// The stem plan for k_wgrad_stem_bn (gm_conv2d_wgrad_stem_bn_*): four waves with two (column pair,
// chunk) items, two pooled vectors and a unit chunk per thread, the pooled rows and the
// coefficients in LDS beside the stem's tiles
static WgradPlan plan_wgrad_stem_bn(const gm_conv_desc_hw* d, int G, const WgradKnobs& k) {
    WgradPlan p;
    if (d && G >= 1 && G <= 64) p = plan_wgrad(d, G, d->C, k);
    if (p.kernel != WgradKernel::stem || p.Q * 4 > 2 * 256 || ((p.Q + 1) / 2) * 8 > 2 * 256 || 2 * d->W > 256 ||
        (p.per & 1)) {
        p.rc = GM_E_UNSUP;
        p.err = "gm_conv2d_wgrad_stem_bn_grouped_bf16: not the pixel-pair stem shape of k_wgrad_stem with Q <= 112";
        return p;
    }
    p.bn = true;
    p.wg = 256;
    p.lds += (size_t)2 * ((p.Q + 1) / 2) * 192 + 5 * 64 * sizeof(float);
    return p;
}

}  // namespace gm
