// bf16 implicit-GEMM convolution on MFMA (gfx950), NHWC activations, KRSC weights.
//
// One kernel serves the ResNet trunk's forward convolutions and their input
// gradients (the trunk of reference src/model.py:53-106, torchvision ResNet):
//
//   out[b, p*oS+oH, q*oS+oW, n] = sum_{t < ntap} sum_c in[b, p*sA+dh_t, q*sA+dw_t, c] * wt[n, tap_t, c]
//
//   forward  : one class, taps (r,s) with dh = r - pad, dw = s - pad, sA = stride, oS = 1;
//   dgrad    : input = dY, weights = transpose(W) [Ci][R][S][Co], sA = 1; the output
//              pixels split into stride^2 parity classes (ph, pw), each with only the
//              taps r where (ph + pad - r) % stride == 0 and dh = (ph + pad - r)/stride,
//              so a strided convolution's input gradient wastes no MFMA work.
//
// GEMM view: M = B*P*Q output pixels, N = output channels, K = ntap*C (c fastest).
// Tiles BM x BN x 64; 256 threads = 2x2 waves, each wave (BM/2)x(BN/2) built from
// v_mfma_f32_32x32x16_bf16 tiles; operands staged global -> LDS by LDS-DMA
// (global_load_lds_dwordx4; double-buffered, next tile's DMA under this tile's MFMAs),
// LDS rows of 128 B XOR-swizzled by ((row>>1)&7) (applied on the DMA source address)
// so the ds_read_b128 fragment reads are conflict-free; fp32 accumulation; weights are
// the MFMA A operand so each lane holds 4 consecutive output channels of one pixel and
// the epilogue writes 8-B NHWC chunks directly.  Out-of-range taps read zeros.
//
// This file: the setup of the kernel arguments (tap classes and grids) and the entry points.
// The kernels are in conv_kern_*.h over conv_args.h, their choice and launch in conv_plan.h -
// one translation unit (g_conv_fault is its device symbol).
#include "conv_plan.h"

static void pack_grid(ConvCls& c, int S);

// the class's taps as a grid: rows r (stride-compatible with the class parity ph) and
// columns s (with pw); fwd is the st = 1 case with every (r, s) - same order as tw/dh/dw
static void set_grid(ConvCls& c, const gm_conv_desc* d, int st, int ph, int pw) {
    c.Rc = c.Sc = 0;
    for (int r = 0; r < d->R && c.Rc < 8; ++r) {
        if (((ph + d->pad - r) % st + st) % st) continue;
        c.cdh[c.Rc] = (signed char)((ph + d->pad - r) / st);
        c.crs[c.Rc++] = (unsigned char)(r * d->S);
    }
    for (int s = 0; s < d->S && c.Sc < 8; ++s) {
        if (((pw + d->pad - s) % st + st) % st) continue;
        c.cdw[c.Sc] = (signed char)((pw + d->pad - s) / st);
        c.cs[c.Sc++] = (unsigned char)s;
    }
    c.smag = c.Sc > 0 ? (256 + c.Sc - 1) / c.Sc : 0;
    c.fd_pq = FastDiv((uint32_t)(c.P * c.Q > 0 ? c.P * c.Q : 1));
    c.fd_q = FastDiv((uint32_t)(c.Q > 0 ? c.Q : 1));
    pack_grid(c, d->S);
}

// forward taps read dh = r - pad, i.e. the dgrad formula with st = 1 and a sign flip
static void set_grid_fwd(ConvCls& c, const gm_conv_desc_hw* d) {
    c.Rc = d->R < 8 ? d->R : 8;
    c.Sc = d->S < 8 ? d->S : 8;
    for (int r = 0; r < c.Rc; ++r) {
        c.cdh[r] = (signed char)(r - d->pad_h);
        c.crs[r] = (unsigned char)(r * d->S);
    }
    for (int s = 0; s < c.Sc; ++s) {
        c.cdw[s] = (signed char)(s - d->pad_w);
        c.cs[s] = (unsigned char)s;
    }
    c.smag = (256 + c.Sc - 1) / c.Sc;
    c.fd_pq = FastDiv((uint32_t)(c.P * c.Q));
    c.fd_q = FastDiv((uint32_t)c.Q);
    pack_grid(c, d->S);
}

static void pack_grid(ConvCls& c, int S) {
    c.dh0 = c.cdh[0];
    c.sh = c.Rc > 1 ? c.cdh[1] - c.cdh[0] : 1;
    c.dw0 = c.cdw[0];
    c.sw = c.Sc > 1 ? c.cdw[1] - c.cdw[0] : 1;
    c.pk_dh = c.pk_dw = c.pk_r = c.pk_s = 0;
    for (int i = 0; i < c.Rc; ++i) {
        c.pk_dh |= (unsigned)((c.cdh[i] + 8) & 15) << (4 * i);
        c.pk_r |= (unsigned)((c.crs[i] / S) & 15) << (4 * i);
    }
    for (int j = 0; j < c.Sc; ++j) {
        c.pk_dw |= (unsigned)((c.cdw[j] + 8) & 15) << (4 * j);
        c.pk_s |= (unsigned)(c.cs[j] & 15) << (4 * j);
    }
}

// the lean kernel's tap grid must reproduce the tap list exactly (order, offsets, weights)
static bool grid_ok(const ConvCls& c, int S) {
    if (c.Rc * c.Sc != c.ntap || c.Rc > 8 || c.Sc > 8) return false;
    if ((c.sh != 1 && c.sh != -1) || (c.sw != 1 && c.sw != -1)) return false;
    for (int i = 0; i < c.Rc; ++i)
        if (c.cdh[i] != c.dh0 + c.sh * i) return false;
    for (int j = 0; j < c.Sc; ++j)
        if (c.cdw[j] != c.dw0 + c.sw * j) return false;
    for (int t = 0; t < c.ntap; ++t) {
        const int i = (t * c.smag) >> 8, j = t - i * c.Sc;
        if (i != t / c.Sc) return false;
        const int dh = (int)((c.pk_dh >> (4 * i)) & 15u) - 8, dw = (int)((c.pk_dw >> (4 * j)) & 15u) - 8;
        const int tw = (int)((c.pk_r >> (4 * i)) & 15u) * S + (int)((c.pk_s >> (4 * j)) & 15u);
        if (dh != c.dh[t] || dw != c.dw[t] || tw != c.tw[t]) return false;
    }
    return true;
}

static int check_desc(const gm_conv_desc* d) {
    GM_REQUIRE(d && d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->K > 0 && d->R > 0 && d->S > 0,
               "conv: empty shape");
    GM_REQUIRE(d->stride >= 1 && d->pad >= 0, "conv: bad stride/pad");
    GM_REQUIRE(d->R * d->S <= kMaxTap, "conv: at most %d taps", kMaxTap);
    GM_REQUIRE(log2_exact(d->C) >= 3, "conv: C must be a power of two >= 8 (got %d)", d->C);
    GM_REQUIRE(d->K % 8 == 0, "conv: K must be a multiple of 8 (got %d)", d->K);
    return GM_OK;
}

static int check_desc_hw(const gm_conv_desc_hw* d) {
    GM_REQUIRE(d && d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->K > 0 && d->R > 0 && d->S > 0,
               "conv: empty shape");
    GM_REQUIRE(d->stride_h >= 1 && d->stride_w >= 1 && d->pad_h >= 0 && d->pad_w >= 0, "conv: bad stride/pad");
    GM_REQUIRE(d->R * d->S <= kMaxTap, "conv: at most %d taps", kMaxTap);
    GM_REQUIRE(log2_exact(d->C) >= 3, "conv: C must be a power of two >= 8 (got %d)", d->C);
    GM_REQUIRE(d->K % 8 == 0, "conv: K must be a multiple of 8 (got %d)", d->K);
    GM_REQUIRE(d->H + 2 * d->pad_h >= d->R && d->W + 2 * d->pad_w >= d->S, "conv: filter larger than input");
    return GM_OK;
}

static void fwd_setup(const gm_conv_desc_hw* d, const void* x, const void* w, void* y, ConvArgs& a) {
    const int P = (d->H + 2 * d->pad_h - d->R) / d->stride_h + 1;
    const int Q = (d->W + 2 * d->pad_w - d->S) / d->stride_w + 1;
    memset(&a, 0, sizeof(a));
    a.in = (const uint16_t*)x;
    a.wt = (const uint16_t*)w;
    a.N = d->N; a.Hi = d->H; a.Wi = d->W; a.C = d->C; a.logC = log2_exact(d->C);
    a.Nout = d->K; a.T = d->R * d->S; a.Sw = d->S;
    a.Ho = P; a.Wo = Q; a.sAh = d->stride_h; a.sAw = d->stride_w;
    a.ncls = 1;
    a.G = 1;
    ConvCls& c = a.cls[0];
    c.out = (uint16_t*)y;
    c.P = P; c.Q = Q; c.oS = 1; c.oH = 0; c.oW = 0;
    c.ntap = d->R * d->S;
    for (int r = 0; r < d->R; ++r)
        for (int s = 0; s < d->S; ++s) {
            const int i = r * d->S + s;
            c.tw[i] = (short)i;
            c.dh[i] = (signed char)(r - d->pad_h);
            c.dw[i] = (signed char)(s - d->pad_w);
        }
    set_grid_fwd(c, d);
}

// returns false when some output pixels belong to no parity class (they must be zeroed)
static bool dgrad_setup(const gm_conv_desc* d, const void* dy, const void* wt, void* dx, ConvArgs& a) {
    const int st = d->stride;
    const int P = (d->H + 2 * d->pad - d->R) / st + 1;
    const int Q = (d->W + 2 * d->pad - d->S) / st + 1;
    memset(&a, 0, sizeof(a));
    a.in = (const uint16_t*)dy;
    a.wt = (const uint16_t*)wt;
    a.N = d->N; a.Hi = P; a.Wi = Q; a.C = d->K; a.logC = log2_exact(d->K);
    a.Nout = d->C; a.T = d->R * d->S; a.Sw = d->S;
    a.Ho = d->H; a.Wo = d->W; a.sAh = a.sAw = 1;
    a.G = 1;
    bool full = true;
    for (int ph = 0; ph < st; ++ph)
        for (int pw = 0; pw < st; ++pw) {
            ConvCls& c = a.cls[a.ncls];
            c.out = (uint16_t*)dx;
            c.P = (d->H - ph + st - 1) / st;
            c.Q = (d->W - pw + st - 1) / st;
            c.oS = st; c.oH = ph; c.oW = pw;
            int n = 0;
            for (int r = 0; r < d->R; ++r) {
                if (((ph + d->pad - r) % st + st) % st) continue;
                for (int sx = 0; sx < d->S; ++sx) {
                    if (((pw + d->pad - sx) % st + st) % st) continue;
                    c.tw[n] = (short)(r * d->S + sx);
                    c.dh[n] = (signed char)((ph + d->pad - r) / st);
                    c.dw[n] = (signed char)((pw + d->pad - sx) / st);
                    ++n;
                }
            }
            c.ntap = n;
            if (n == 0 || c.P <= 0 || c.Q <= 0) { full = false; continue; }
            set_grid(c, d, st, ph, pw);
            ++a.ncls;
        }
    return full;
}

static int check_dgrad(const gm_conv_desc* d) {
    int rc = check_desc(d);
    if (rc) return rc;
    GM_REQUIRE(log2_exact(d->K) >= 3, "conv dgrad: K must be a power of two >= 8 (got %d)", d->K);
    GM_REQUIRE(d->stride * d->stride <= kMaxCls, "conv dgrad: stride %d unsupported", d->stride);
    return GM_OK;
}

static gm_conv_desc_hw to_hw(const gm_conv_desc* d) {
    return gm_conv_desc_hw{d->N, d->H, d->W, d->C, d->K, d->R, d->S, d->stride, d->stride, d->pad, d->pad};
}

namespace gm {
unsigned conv_faults_read(bool clear) {
    unsigned v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_conv_fault), sizeof(v), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return ~0u;
    if (clear && v) {
        const unsigned z = 0;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_conv_fault), &z, sizeof(z), 0, hipMemcpyHostToDevice);
    }
    return v;
}
}  // namespace gm

static ConvKnobs g_knobs;

extern "C" int gm_conv_set_splitk(int target) {
    GM_REQUIRE(target >= 0, "gm_conv_set_splitk: target must be >= 0");
    g_knobs.splitk_target = target;
    return GM_OK;
}

extern "C" int gm_conv_set_h9(int on) {
    g_knobs.h9 = on;
    return GM_OK;
}

extern "C" int gm_conv_set_halo(int on) {
    g_knobs.halo = on < 0 ? 0 : on > 2 ? 2 : on;
    return GM_OK;
}

extern "C" int gm_conv_set_stem(int on) {
    g_knobs.stem = on ? 1 : 0;
    return GM_OK;
}

extern "C" int gm_conv_set_rw(int on) {
    g_knobs.rw = on ? 1 : 0;  // 0: the layer-1 shapes take the im2col kernel
    return GM_OK;
}

static int pick_and_launch(ConvArgs& a, hipStream_t st, void* ws, size_t ws_bytes) {
    return launch_conv(a, plan_conv(a, ws ? ws_bytes : 0, g_knobs), ws, st);
}

// view groups in one launch: group g's weight sits w_stride elements after group 0's
static int check_groups(const char* fn, int G, long long w_stride, long long weight_elems) {
    GM_REQUIRE(G >= 1 && G <= 64, "%s: view groups must be 1..64 (got %d)", fn, G);
    GM_REQUIRE(G == 1 || w_stride >= weight_elems || -w_stride >= weight_elems,
               "%s: group weight stride %lld shorter than one weight", fn, w_stride);
    return GM_OK;
}
static long long weight_elems(const gm_conv_desc_hw* d) { return (long long)d->K * d->R * d->S * d->C; }
static long long weight_elems(const gm_conv_desc* d) { return (long long)d->K * d->R * d->S * d->C; }

// the views stacked along the batch: group g's input, weight and output after group 0's
static void set_groups(ConvArgs& a, int G, long long w_stride) {
    a.G = G;
    a.gs_in = (long long)a.N * a.Hi * a.Wi * a.C;
    a.gs_wt = w_stride;
    a.gs_out = (long long)a.N * a.Ho * a.Wo * a.Nout;
}

// 1x1 / s1 / p0 convolutions as plain GEMMs (conv1x1.hip, k_gemm_ring)
namespace gm {
bool conv1x1_ok(int R, int S, int sh, int sw, int ph, int pw, long long M, int Kr, int N);
bool conv1x1s_ok(int R, int S, int sh, int sw, int ph, int pw, long long M, int Kr, int N);
int conv1x1_gemm(long long M, int Kr, int N, int G, const void* A, long long gsA, const void* B, long long gsB,
                 void* out, long long gsO, const void* addend, hipStream_t st, const char* fn,
                 float* stats = nullptr, const uint16_t* bnx = nullptr, const float* bncoef = nullptr,
                 const float* bnmean = nullptr, const uint8_t* amask = nullptr, const int* sgeo = nullptr);
}  // namespace gm

constexpr int kNotTaken = 1;  // (no GM_* code)
struct Gemm1x1 {
    bool dgrad = false;       // input gradient: in = dy, w = the transposed weight, out = dx
    bool s2 = false;          // also route the stride-2 downsample (the view-grouped entry points)
    int G = 1;
    long long w_stride = 0;
    const void* addend = nullptr;  // dgrad: out = conv + addend (where amask's bit is set)
    const uint8_t* amask = nullptr;
    float* stats = nullptr;   // BatchNorm statistics from the epilogue, *rows_out partial rows
    int* rows_out = nullptr;
    const uint16_t* bnx = nullptr;
    const float* bncoef = nullptr;
    const float* bnmean = nullptr;
};

// Routes a 1x1 convolution to conv1x1_gemm - stride 1 as a plain GEMM; with o.s2 the stride-2
// downsample, its A rows gathered (forward) or its output rows scattered (input gradient) - or
// returns kNotTaken, with nothing launched, when the kernels of this file serve the shape.
static int route_1x1(const gm_conv_desc_hw* d, const void* in, const void* w, void* out, const Gemm1x1& o,
                     hipStream_t st) {
    const long long M = (long long)d->N * d->H * d->W;                     // pixels of x / dx
    const int Kr = o.dgrad ? d->K : d->C, Nn = o.dgrad ? d->C : d->K;      // channels reduced / written
    if (gm::conv1x1_ok(d->R, d->S, d->stride_h, d->stride_w, d->pad_h, d->pad_w, M, Kr, Nn)) {
        if (o.rows_out) *o.rows_out = tile_rows(M, 64);
        return gm::conv1x1_gemm(M, Kr, Nn, o.G, in, M * Kr, w, o.w_stride, out, M * Nn, o.addend, st,
                                o.dgrad ? "conv1x1 dgrad" : "conv1x1 fwd", o.stats, o.bnx, o.bncoef, o.bnmean,
                                o.amask);
    }
    const int P = (d->H - 1) / 2 + 1, Q = (d->W - 1) / 2 + 1;
    const long long Mo = (long long)d->N * P * Q;                          // pixels of y / dy
    if (!o.s2 || !gm::conv1x1s_ok(d->R, d->S, d->stride_h, d->stride_w, d->pad_h, d->pad_w, Mo, Kr, Nn) ||
        M * d->C >= (1ll << 30))
        return kNotTaken;
    const int geo[6] = {2, d->H, d->W, P, Q, o.dgrad ? 1 : 0};
    if (o.rows_out) *o.rows_out = tile_rows(Mo, 64);
    if (!o.dgrad)  // the downsample: A rows gathered at stride 2
        return gm::conv1x1_gemm(Mo, Kr, Nn, o.G, in, M * Kr, w, o.w_stride, out, Mo * Nn, nullptr, st,
                                "conv1x1/s2 fwd", o.stats, nullptr, nullptr, nullptr, nullptr, geo);
    // the downsample's input gradient: dy rows dense, out rows scattered to the even pixels; the
    // others hold the (masked) addend or zero - one pass over dx unless the addend is dx itself
    if (o.addend != out)
        if (int rc = fill_uncovered(out, (size_t)o.G * M * Nn, o.addend, o.amask, st)) return rc;
    return gm::conv1x1_gemm(Mo, Kr, Nn, o.G, in, Mo * Kr, w, o.w_stride, out, M * Nn, o.addend ? out : nullptr, st,
                            "conv1x1/s2 dgrad", nullptr, nullptr, nullptr, nullptr, nullptr, geo);
}

// the forward convolution of a checked descriptor over G view groups; s2: the stride-2 downsample
// goes to k_gemm_ring too (the view-grouped entry point's routing)
static int conv_fwd(const gm_conv_desc_hw* d, int G, bool s2, const void* x, const void* w, long long w_stride,
                    void* y, void* ws, size_t ws_bytes, void* stream) {
    GM_REQUIRE(x && w && y, "conv fwd: null pointer");
    int rc = check_groups("conv fwd", G, w_stride, weight_elems(d));
    if (rc) return rc;
    Gemm1x1 o;
    o.s2 = s2; o.G = G; o.w_stride = w_stride;
    if ((rc = route_1x1(d, x, w, y, o, as_stream(stream))) != kNotTaken) return rc;
    ConvArgs a;
    fwd_setup(d, x, w, y, a);
    set_groups(a, G, w_stride);
    return pick_and_launch(a, as_stream(stream), ws, ws_bytes);
}

extern "C" int gm_conv2d_fwd_hw_bf16(const gm_conv_desc_hw* d, const void* x, const void* w, void* y,
                                     void* stream) {
    if (int rc = check_desc_hw(d)) return rc;
    return conv_fwd(d, 1, false, x, w, 0, y, nullptr, 0, stream);
}

extern "C" int gm_conv2d_fwd_ex_bf16(const gm_conv_desc* d, const void* x, const void* w, void* y, void* ws,
                                     size_t ws_bytes, void* stream) {
    if (int rc = check_desc(d)) return rc;
    const gm_conv_desc_hw h = to_hw(d);
    return conv_fwd(&h, 1, false, x, w, 0, y, ws, ws_bytes, stream);
}

extern "C" int gm_conv2d_fwd_bf16(const gm_conv_desc* d, const void* x, const void* w, void* y, void* stream) {
    return gm_conv2d_fwd_ex_bf16(d, x, w, y, nullptr, 0, stream);
}

// G view groups in one launch: group g reads x + g*N*H*W*C with the weight w + g*w_stride
// and writes y + g*N*P*Q*K (the views stacked along the batch, one weight per view)
extern "C" int gm_conv2d_fwd_grouped_bf16(const gm_conv_desc_hw* d, int G, const void* x, const void* w,
                                          long long w_stride, void* y, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_desc_hw(d)) return rc;
    return conv_fwd(d, G, true, x, w, w_stride, y, ws, ws_bytes, stream);
}

static void query_setup(const gm_conv_desc_hw* d, int G, ConvArgs& a);

// does route_1x1 (with the stride-2 downsample, as the view-grouped forward routes) take d?
static bool takes_1x1_fwd(const gm_conv_desc_hw* d) {
    const long long M = (long long)d->N * d->H * d->W;
    if (gm::conv1x1_ok(d->R, d->S, d->stride_h, d->stride_w, d->pad_h, d->pad_w, M, d->C, d->K)) return true;
    const long long Mo = (long long)d->N * ((d->H - 1) / 2 + 1) * ((d->W - 1) / 2 + 1);
    return gm::conv1x1s_ok(d->R, d->S, d->stride_h, d->stride_w, d->pad_h, d->pad_w, Mo, d->C, d->K) &&
           M * d->C < (1ll << 30);
}

static const char* const kAffine1x1 =
    "conv fwd affine: 1x1 shapes go to k_gemm_ring, which has no affine epilogue - run "
    "gm_conv2d_fwd_grouped_bf16 and a coefficient-only gm_bn_fwd_apply_grouped_bf16";

// The evaluation forward (include/greedymml.h): the view-grouped forward of
// gm_conv2d_fwd_grouped_bf16 - the same plan under the same switches - with
// y = act(acc sc[n] + sh[n] (+ residual)) as its epilogue.  1: the call below takes the shape.
extern "C" int gm_conv2d_fwd_affine_ok(const gm_conv_desc_hw* d, int G) {
    if (!d || check_desc_hw(d) || G < 1 || G > 64) return 0;
    if (takes_1x1_fwd(d)) {
        set_error("%s", kAffine1x1);
        return 0;
    }
    ConvArgs a;
    query_setup(d, G, a);
    a.coef = reinterpret_cast<const float*>(16);
    const ConvPlan p = plan_conv(a, 0, g_knobs);
    if (p.rc != GM_OK) set_error("%s", p.err);
    return p.rc == GM_OK;
}

extern "C" int gm_conv2d_fwd_grouped_affine_bf16(const gm_conv_desc_hw* d, int G, const void* x, const void* w,
                                                 long long w_stride, void* y, const float* coef,
                                                 long long coef_stride, const void* residual, int relu, void* ws,
                                                 size_t ws_bytes, void* stream) {
    const char* fn = "gm_conv2d_fwd_grouped_affine_bf16";
    GM_REQUIRE(d, "%s: null descriptor d", fn);
    int rc = check_desc_hw(d);
    if (rc) return rc;
    GM_REQUIRE(x && w && y, "%s: null x, w or y", fn);
    GM_REQUIRE(coef && (reinterpret_cast<uintptr_t>(coef) & 15) == 0, "%s: coef null or not 16-byte aligned", fn);
    GM_REQUIRE(coef_stride % 4 == 0 && (G == 1 || coef_stride >= 2ll * d->K || -coef_stride >= 2ll * d->K),
               "%s: coef_stride %lld: a multiple of 4, at least 2 K floats apart", fn, coef_stride);
    GM_REQUIRE((reinterpret_cast<uintptr_t>(y) & 15) == 0 && (reinterpret_cast<uintptr_t>(residual) & 15) == 0,
               "%s: y and residual must be 16-byte aligned", fn);
    if ((rc = check_groups(fn, G, w_stride, weight_elems(d)))) return rc;
    if (takes_1x1_fwd(d)) {
        set_error("%s", kAffine1x1);
        return GM_E_UNSUP;
    }
    ConvArgs a;
    fwd_setup(d, x, w, y, a);
    set_groups(a, G, w_stride);
    a.coef = coef;
    a.gs_coef = coef_stride;
    a.addend = static_cast<const uint16_t*>(residual);
    a.relu = relu ? 1 : 0;
    return pick_and_launch(a, as_stream(stream), ws, ws_bytes);
}

// an upper bound of the partial statistics rows any kernel takes for M output pixels, whatever the
// switches say at the launch: 64-pixel tiles (k_gemm_ring, the lean kernel's smallest), k_conv_rw's
// one row per workgroup
static long long stats_rows_bound(long long M) { return std::max<long long>(tile_rows(M, 64), kRwWorkgroups); }

// the arguments of a size query: the plan reads no data pointer
static void query_setup(const gm_conv_desc_hw* d, int G, ConvArgs& a) {
    fwd_setup(d, reinterpret_cast<const void*>(16), reinterpret_cast<const void*>(16), reinterpret_cast<void*>(16), a);
    a.G = G;
}

// Forward convolution + the BatchNorm statistics of its stored output from the epilogue
// (include/greedymml.h).  The statistics buffer: an upper bound of the partial rows either
// statistics kernel takes for the shape.
extern "C" size_t gm_conv2d_fwd_bn_stats_floats(const gm_conv_desc_hw* d, int G) {
    if (check_desc_hw(d) || G < 1 || G > 64) return 0;
    ConvArgs a;
    query_setup(d, G, a);
    const long long rows = std::max<long long>(stats_rows_bound((long long)d->N * a.Ho * a.Wo),
                                               gm_conv_stem_stats_rows(d, G));  // k_conv_stem: one per workgroup
    return (size_t)G * 2 * d->K * (size_t)(rows + 1);
}

extern "C" int gm_conv2d_fwd_grouped_bn_stats_bf16(const gm_conv_desc_hw* d, int G, const void* x, const void* w,
                                                   long long w_stride, void* y, float* stats, size_t stats_floats,
                                                   int* rows_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_desc_hw(d);
    if (rc) return rc;
    GM_REQUIRE(x && w && y && stats && rows_out, "conv fwd bn stats: null pointer");
    if ((rc = check_groups("conv fwd bn stats", G, w_stride, weight_elems(d)))) return rc;
    const size_t need = gm_conv2d_fwd_bn_stats_floats(d, G);
    GM_REQUIRE(stats_floats >= need, "conv fwd bn stats: %zu floats < %zu", stats_floats, need);
    ConvArgs a;
    fwd_setup(d, x, w, y, a);
    const long long M = (long long)d->N * a.Ho * a.Wo;
    if (d->K % 64 != 0 || (size_t)M * d->K * 2 >= 0x7ffff000u) {
        set_error("conv fwd bn stats: K %% 64 != 0 or a group's output past 32-bit offsets");
        return GM_E_UNSUP;
    }
    Gemm1x1 o;
    o.s2 = true; o.G = G; o.w_stride = w_stride; o.stats = stats; o.rows_out = rows_out;
    if ((rc = route_1x1(d, x, w, y, o, as_stream(stream))) != kNotTaken) return rc;
    set_groups(a, G, w_stride);
    // every view-grouped forward kernel stages its output tile through LDS (k_conv_rw,
    // store_tile_lds of k_conv_h9 / k_conv_igemm_ut; k_gemm_ring above), where the sums are a
    // few VALU per stored 16-B chunk.  (Summed in the MFMA layout instead - a 32-lane reduction
    // per value, one row per 64-pixel slab - they cost more than the statistics read: r05.)
    if (a.G < 2) {
        set_error("conv fwd bn stats: view groups (G >= 2) only");
        return GM_E_UNSUP;
    }
    const ConvPlan p = plan_conv(a, ws ? ws_bytes : 0, g_knobs);
    if (p.kernel == ConvKernel::stem) {  // the stem's statistics come from gm_conv2d_fwd_grouped_stats_bf16
        set_error("conv fwd bn stats: stem shapes take the stem statistics entry point");
        return GM_E_UNSUP;
    }
    GM_REQUIRE((size_t)G * 2 * d->K * ((size_t)p.stats_rows + 1) <= stats_floats,
               "conv fwd bn stats: %d rows past %zu floats", p.stats_rows, stats_floats);
    a.stats = stats;
    *rows_out = p.stats_rows;
    return launch_conv(a, p, ws, as_stream(stream));
}

extern "C" int gm_conv_stem_stats_rows(const gm_conv_desc_hw* d, int G) {
    if (check_desc_hw(d) || G < 1 || G > 64) return 0;
    ConvArgs a;
    query_setup(d, G, a);
    const ConvPlan p = plan_conv(a, 0, g_knobs);
    return p.kernel == ConvKernel::stem ? p.stats_rows : 0;
}

// The stem convolution (k_conv_stem's shapes) with the BatchNorm statistics of its output
// accumulated in its epilogue: partial rows per workgroup, finalized by
// gm_bn_fwd_stats_finalize_grouped (no statistics pass over the 205 MB output).
extern "C" int gm_conv2d_fwd_grouped_stats_bf16(const gm_conv_desc_hw* d, int G, const void* x, const void* w,
                                                long long w_stride, void* y, float* stats, int stats_rows,
                                                void* stream) {
    int rc = check_desc_hw(d);
    if (rc) return rc;
    GM_REQUIRE(x && w && y && stats, "conv fwd stats: null pointer");
    if ((rc = check_groups("conv fwd stats", G, w_stride, weight_elems(d)))) return rc;
    ConvArgs a;
    fwd_setup(d, x, w, y, a);
    set_groups(a, G, w_stride);
    ConvPlan p = plan_conv(a, 0, g_knobs);
    GM_REQUIRE(p.kernel == ConvKernel::stem, "conv fwd stats: only the stem kernel's shapes (64 output channels)");
    GM_REQUIRE(stats_rows == p.stats_rows, "conv fwd stats: stats_rows %d != gm_conv_stem_stats_rows %d",
               stats_rows, p.stats_rows);
    p.stem.stats = stats;
    return launch_conv(a, p, nullptr, as_stream(stream));
}

// The input gradient with a masked gradient-join addend: dx = dgrad + (addend where the 1-bit mask
// is set) - the identity branch's dz = dy . [y > 0] of a block-output ReLU read from its dy and the
// BatchNorm forward's mask bits (batchnorm.hip) instead of a materialised dres.  dx != addend.
static int dgrad_grouped(const gm_conv_desc* d, int G, bool s2, const void* dy, const void* wt, long long wt_stride,
                         void* dx, const void* addend, const uint8_t* amask, void* ws, size_t ws_bytes, void* stream);

extern "C" int gm_conv2d_dgrad_grouped_masked_bf16(const gm_conv_desc* d, int G, const void* dy, const void* wt,
                                                   long long wt_stride, void* dx, const void* addend,
                                                   const void* addend_mask, void* ws, size_t ws_bytes, void* stream) {
    GM_REQUIRE(addend && addend_mask, "conv dgrad masked: null addend or mask");
    GM_REQUIRE(addend != dx, "conv dgrad masked: the addend must not alias dx");
    GM_REQUIRE(d && d->C % 32 == 0, "conv dgrad masked: C must be a multiple of 32 (one mask dword per 32 channels)");
    return dgrad_grouped(d, G, true, dy, wt, wt_stride, dx, addend, static_cast<const uint8_t*>(addend_mask), ws,
                         ws_bytes, stream);
}

extern "C" int gm_conv2d_dgrad_grouped_bf16(const gm_conv_desc* d, int G, const void* dy, const void* wt,
                                            long long wt_stride, void* dx, const void* addend, void* ws,
                                            size_t ws_bytes, void* stream) {
    return dgrad_grouped(d, G, true, dy, wt, wt_stride, dx, addend, nullptr, ws, ws_bytes, stream);
}

// addend == dx (in place) is allowed: every epilogue loads an output element's addend
// and stores that element from the same thread, and pixels no parity class covers
// then simply keep the addend (no zero / copy pass).  s2: the stride-2 downsample's input gradient goes
// to k_gemm_ring too (the view-grouped entry points' routing)
static int dgrad_grouped(const gm_conv_desc* d, int G, bool s2, const void* dy, const void* wt, long long wt_stride,
                         void* dx, const void* addend, const uint8_t* amask, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_dgrad(d);
    if (rc) return rc;
    GM_REQUIRE(dy && wt && dx, "conv dgrad: null pointer");
    if ((rc = check_groups("conv dgrad", G, wt_stride, weight_elems(d)))) return rc;
    hipStream_t s = as_stream(stream);
    const gm_conv_desc_hw h = to_hw(d);
    Gemm1x1 o;
    o.dgrad = true; o.s2 = s2; o.G = G; o.w_stride = wt_stride; o.addend = addend; o.amask = amask;
    if ((rc = route_1x1(&h, dy, wt, dx, o, s)) != kNotTaken) return rc;
    ConvArgs a;
    const bool full = dgrad_setup(d, dy, wt, dx, a);
    set_groups(a, G, wt_stride);
    a.addend = (const uint16_t*)addend;
    a.amask = addend ? amask : nullptr;
    if (!full && addend != dx) {  // the groups are contiguous: one pass zeroes (or copies) them all
        if ((rc = fill_uncovered(dx, (size_t)G * d->N * d->H * d->W * d->C, addend, amask, s))) return rc;
        if (addend) {  // dx now holds the (masked) addend everywhere: the addend in place
            a.addend = (const uint16_t*)dx;
            a.amask = nullptr;
        }
    }
    return pick_and_launch(a, s, ws, ws_bytes);
}

// Input gradient + the statistics of the BatchNorm backward that consumes it (include/
// greedymml.h): the partial rows of (sum dz, sum dz (x - mean)) from the LDS-staged epilogue
// (k_conv_rw, k_conv_h9, k_conv_igemm_ut), then G x 4C floats for the backward's coefficients
// (gm_bn_bwd_stats_finalize_grouped / gm_bn_bwd_apply_grouped_bf16).
extern "C" size_t gm_conv2d_dgrad_bn_stats_floats(const gm_conv_desc* d, int G) {
    if (check_desc(d) || G < 1 || G > 64) return 0;
    const long long rows = stats_rows_bound((long long)d->N * d->H * d->W);
    return (size_t)G * 2 * d->C * (size_t)(rows + 1) + (size_t)G * 4 * d->C;
}

extern "C" int gm_conv2d_dgrad_grouped_bn_stats_bf16(const gm_conv_desc* d, int G, const void* dy, const void* wt,
                                                     long long wt_stride, void* dx, const void* bn_x,
                                                     const float* bn_coef, const float* bn_mean, float* stats,
                                                     size_t stats_floats, int* rows_out, void* ws, size_t ws_bytes,
                                                     void* stream) {
    int rc = check_dgrad(d);
    if (rc) return rc;
    GM_REQUIRE(dy && wt && dx && bn_x && bn_coef && bn_mean && stats && rows_out, "conv dgrad bn stats: null pointer");
    if ((rc = check_groups("conv dgrad bn stats", G, wt_stride, weight_elems(d)))) return rc;
    const size_t need = gm_conv2d_dgrad_bn_stats_floats(d, G);
    GM_REQUIRE(stats_floats >= need, "conv dgrad bn stats: %zu floats < %zu", stats_floats, need);
    const long long M = (long long)d->N * d->H * d->W;
    // one dense output class (stride 1: the parity classes of a strided input gradient would
    // share tile rows), view groups, 64-channel slices, 32-bit offsets
    if (d->stride != 1 || G < 2 || d->C % 64 != 0 || (size_t)M * d->C * 2 >= 0x7ffff000u) {
        set_error("conv dgrad bn stats: stride 1, G >= 2, C %% 64 == 0, 32-bit offsets only");
        return GM_E_UNSUP;
    }
    const gm_conv_desc_hw h = to_hw(d);
    Gemm1x1 o;  // k_gemm_ring
    o.dgrad = true; o.G = G; o.w_stride = wt_stride; o.stats = stats; o.rows_out = rows_out;
    o.bnx = static_cast<const uint16_t*>(bn_x); o.bncoef = bn_coef; o.bnmean = bn_mean;
    if ((rc = route_1x1(&h, dy, wt, dx, o, as_stream(stream))) != kNotTaken) return rc;
    ConvArgs a;
    const bool full = dgrad_setup(d, dy, wt, dx, a);
    set_groups(a, G, wt_stride);
    ConvPlan p;
    if (!full || a.ncls != 1 || (p = plan_conv(a, ws ? ws_bytes : 0, g_knobs)).kernel == ConvKernel::stem) {
        set_error("conv dgrad bn stats: one dense output class only");
        return GM_E_UNSUP;
    }
    GM_REQUIRE((size_t)G * 2 * d->C * ((size_t)p.stats_rows + 1) + (size_t)G * 4 * d->C <= stats_floats,
               "conv dgrad bn stats: %d rows past %zu floats", p.stats_rows, stats_floats);
    a.stats = stats;
    a.bnx = o.bnx;
    a.bncoef = bn_coef;
    a.bnmean = bn_mean;
    *rows_out = p.stats_rows;
    return launch_conv(a, p, ws, as_stream(stream));
}

extern "C" int gm_conv2d_dgrad_add_bf16(const gm_conv_desc* d, const void* dy, const void* wt, void* dx,
                                        const void* addend, void* ws, size_t ws_bytes, void* stream) {
    return dgrad_grouped(d, 1, false, dy, wt, 0, dx, addend, nullptr, ws, ws_bytes, stream);
}

extern "C" int gm_conv2d_dgrad_ex_bf16(const gm_conv_desc* d, const void* dy, const void* wt, void* dx, void* ws,
                                       size_t ws_bytes, void* stream) {
    return gm_conv2d_dgrad_add_bf16(d, dy, wt, dx, nullptr, ws, ws_bytes, stream);
}

extern "C" int gm_conv2d_dgrad_bf16(const gm_conv_desc* d, const void* dy, const void* wt, void* dx,
                                    void* stream) {
    return gm_conv2d_dgrad_ex_bf16(d, dy, wt, dx, nullptr, 0, stream);
}

extern "C" size_t gm_conv2d_splitk_ws_bytes_grouped(const gm_conv_desc* d, int G, int dgrad) {
    ConvArgs a;
    if (G < 1) return 0;
    if (dgrad) {
        if (check_dgrad(d)) return 0;
        dgrad_setup(d, nullptr, nullptr, nullptr, a);
    } else {
        if (check_desc(d)) return 0;
        const gm_conv_desc_hw h = to_hw(d);
        fwd_setup(&h, nullptr, nullptr, nullptr, a);
    }
    a.G = G;
    return plan_conv(a, 0, g_knobs).ws_need;
}

extern "C" size_t gm_conv2d_splitk_ws_bytes(const gm_conv_desc* d, int dgrad) {
    return gm_conv2d_splitk_ws_bytes_grouped(d, 1, dgrad);
}
