// Two dependent rounds of small fp32 GEMMs in ONE launch (the MMTM site's FC chain:
// squeeze FC + ReLU -> excite FCs + sigmoid -> running average; its backward: excite
// gradients + dz -> squeeze gradients + dsq).
//
// gemm_f32.hip prices the separate launches: they are dependent latency chains, ~7 us
// each, not MFMA work.  Here a persistent grid (at most one workgroup per usable CU of
// the residency plan, divided by streams x sharers, so every workgroup is resident while
// the others wait for it) walks the first round's workgroup tiles, meets at a device
// counter, and walks the second round's tiles, which may read any first-round output.
// Every tile is gemm_tile (gemm_tile.h) under launch_gemm_f32's own tile plan, so each
// output element is bit-identical to the separate launches'.
//
// Hand-off (cdna_hip_programming.md Guideline 16, the plain-store form): every wave
// drains its stores (s_waitcnt vmcnt(0)), the workgroup barriers, thread 0 releases at
// agent scope and adds to the arrival counter (relaxed, agent scope); the workgroup
// whose add came last zeroes the counter and advances the generation word, the others
// poll the generation (relaxed, s_sleep between polls, bounded by spin_limit()); then
// thread 0 acquires at agent scope (L1 invalidate), waits for it and the workgroup
// barriers before any wave's plain operand loads.  A spin that runs out sets
// GM_FAULT_CHAIN_SPIN and every later output of that workgroup is NaN.
//
// Sync words (caller-provided, gm_gemm_chain_sync_bytes(), zeroed once): word 0 the
// round-1 arrival counter, word 16 the generation, word 32 the round-2 arrival counter
// (running-average stage), each on a line of its own.  Each counter is zeroed by its
// last arriver and the generation only ever advances, so back-to-back launches and
// graph replays need no host-side reset (launches that share the words are ordered on
// one stream).
//
// Running average (ra_v != NULL): after a second arrival the LAST workgroup to arrive
// (told by the value its add returned - no second spin) acquires and runs
// k_running_avg_dev's arithmetic over fc2[0].C, reads the device step counter and
// advances it once.
#include <cstring>

#include "gemm_tile.h"

namespace gm {

__device__ unsigned g_chain_fault = 0;

constexpr int kSyncCount1 = 0, kSyncGen = 16, kSyncCount2 = 32, kSyncWords = 64;

struct ChainArgs {
    gm_gemm p[2 * kMaxGemm];           // round r's problems at [r * kMaxGemm ...]
    int tile_start[2][kMaxGemm + 1];
    int tiles_n[2 * kMaxGemm];
    int cfg[2 * kMaxGemm];
    int vec;
    unsigned spin_limit;
    unsigned* sync;
    // running-average stage (ra_v != NULL)
    const float* e;
    int ld_e, B, C;
    float* ra_v;
    float* ra_s;
    int* step;
    int increment;
};

#define GM_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// this workgroup's share of round r's tiles
template <int NW, int U>
__device__ __forceinline__ void walk_round(const ChainArgs& a, int r, floatx4 (*red)[64], bool poison) {
    const int* ts = a.tile_start[r];
    const int total = ts[kMaxGemm];
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        int pi = 0;
        while (pi + 1 < kMaxGemm && t >= ts[pi + 1]) ++pi;
        const int q = r * kMaxGemm + pi;
        gemm_tile<NW, U>(a.p[q], a.cfg[q], a.tiles_n[q], t - ts[pi], a.vec, red, poison);
        __syncthreads();  // `red` is free again
    }
}

// producer side of an arrival: every wave's stores are in L2, then thread 0 (the caller
// branches on it) releases at agent scope.  Returns the counter's value before the add.
__device__ __forceinline__ void drain_stores() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}
__device__ __forceinline__ unsigned release_and_arrive(unsigned* counter) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return __hip_atomic_fetch_add(counter, 1u, GM_RLX_AGENT);
}
__device__ __forceinline__ void acquire_agent() {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int NW, int U>
__global__ __launch_bounds__(NW * 64) void k_gemm_chain(ChainArgs a) {
    __shared__ floatx4 red[NW][64];
    __shared__ unsigned flag[2];
    const unsigned G = gridDim.x;
    unsigned* sync = a.sync;
    unsigned g0 = 0;
    // the generation before anyone of this launch can have advanced it: the load has
    // returned by the drain below, ahead of this workgroup's own arrival
    if (threadIdx.x == 0) g0 = __hip_atomic_load(sync + kSyncGen, GM_RLX_AGENT);

    walk_round<NW, U>(a, 0, red, false);

    drain_stores();
    if (threadIdx.x == 0) {
        bool ok = true;
        const unsigned before = release_and_arrive(sync + kSyncCount1);
        if (before + 1 == G) {  // last: re-arm the counter, then let everyone through
            __hip_atomic_store(sync + kSyncCount1, 0u, GM_RLX_AGENT);
            __hip_atomic_fetch_add(sync + kSyncGen, 1u, GM_RLX_AGENT);
        } else {
            unsigned it = 0;
            while (__hip_atomic_load(sync + kSyncGen, GM_RLX_AGENT) == g0) {
                if (++it >= a.spin_limit) {
                    ok = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            if (!ok) atomicOr(&g_chain_fault, GM_FAULT_CHAIN_SPIN);
        }
        acquire_agent();
        flag[0] = ok ? 1u : 0u;
    }
    __syncthreads();
    const bool poison = flag[0] == 0u;

    walk_round<NW, U>(a, 1, red, poison);

    if (a.ra_v == nullptr) return;
    drain_stores();
    if (threadIdx.x == 0) {
        const unsigned before = release_and_arrive(sync + kSyncCount2);
        const bool last = before + 1 == G;
        if (last) {
            __hip_atomic_store(sync + kSyncCount2, 0u, GM_RLX_AGENT);
            acquire_agent();
        }
        flag[1] = last ? 1u : 0u;
    }
    __syncthreads();
    if (flag[1] == 0u) return;
    // k_running_avg_dev's arithmetic (mmtm_kernels.hip): one thread per channel, four partial
    // sums over b & 3 combined ((p0 + p1) + p2) + p3
    const int st = *a.step;
    const float k = (float)st, k1 = (float)(st + 1);
    const int B = a.B, C = a.C, ld = a.ld_e;
    const float* e = a.e;
    float* rv = a.ra_v;
    float* rs = a.ra_s;
    for (int c = threadIdx.x; c < C; c += NW * 64) {
        float p[4] = {0.f, 0.f, 0.f, 0.f};
        int b = 0;
        for (; b + 16 <= B; b += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = e[(size_t)(b + u) * ld + c];
#pragma unroll
            for (int u = 0; u < 16; ++u) p[u & 3] += v[u];
        }
        for (; b < B; ++b) p[b & 3] += e[(size_t)b * ld + c];
        float m = ((p[0] + p[1]) + p[2]) + p[3];
        m = m / (float)B;
        if (poison) m = __builtin_nanf("");
        rv[c] = (m + rv[c] * k) / k1;
        if (rs != rv) rs[c] = (m + rs[c] * k) / k1;
    }
    __syncthreads();  // every thread has read *step
    if (threadIdx.x == 0 && a.increment) *a.step = st + 1;
}

static int chain_cus() {
    static const int n = [] {
        int dev = 0, c = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0)
            return 0;
        return c;
    }();
    return n;
}

unsigned chain_faults_read(bool clear) {
    unsigned v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_chain_fault), sizeof(v), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return ~0u;
    if (clear && v) {
        const unsigned z = 0;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_chain_fault), &z, sizeof(z), 0, hipMemcpyHostToDevice);
    }
    return v;
}

struct RunAvg {
    float* ra_v;
    float* ra_s;
    int* step;
    int increment;
};

// argument checks of the three entry points: no HIP call is made before they pass
static int chain_check(const char* what, const gm_gemm* first, int nfirst, const gm_gemm* second, int nsecond,
                       const void* sync) {
    GM_REQUIRE(first && nfirst >= 1 && nfirst <= kMaxGemm, "%s: the first round's problem count must be 1..%d", what,
               kMaxGemm);
    GM_REQUIRE(second && nsecond >= 1 && nsecond <= kMaxGemm, "%s: the second round's problem count must be 1..%d",
               what, kMaxGemm);
    GM_REQUIRE(sync, "%s: null sync words (gm_gemm_chain_sync_bytes() zeroed bytes)", what);
    for (int i = 0; i < nfirst; ++i)
        if (const int rc = gemm_check(first[i], i)) return rc;
    for (int i = 0; i < nsecond; ++i)
        if (const int rc = gemm_check(second[i], i)) return rc;
    return GM_OK;
}

// The single launch.  GM_E_UNSUP (nothing launched) when the residency plan leaves no
// workgroup for it or a problem belongs to the outer-product kernel.
static int launch_chain(const gm_gemm* first, int nfirst, const gm_gemm* second, int nsecond, const RunAvg* ra,
                        void* sync, hipStream_t st) {
    const gm_gemm* in[2] = {first, second};
    const int n[2] = {nfirst, nsecond};
    const GemmKnobs& kn = gemm_knobs();
    ChainArgs a;
    memset(&a, 0, sizeof(a));
    int most = 0;
    for (int r = 0; r < 2; ++r) {
        int tiles = 0;
        for (int i = 0; i < kMaxGemm; ++i) {
            a.tile_start[r][i] = tiles;
            if (i >= n[r]) continue;
            const gm_gemm& p = in[r][i];
            if (gemm_takes_outer(p)) return GM_E_UNSUP;
            const int q = r * kMaxGemm + i;
            a.p[q] = p;
            const TilePlan t = plan_tiles(p, kForms[kn.form]);
            a.cfg[q] = t.cfg;
            a.tiles_n[q] = t.tiles_n;
            tiles += t.tiles;
        }
        a.tile_start[r][kMaxGemm] = tiles;
        if (tiles > most) most = tiles;
    }
    // every workgroup resident while the others wait for it: one per usable CU, shared with
    // the other launches that may wait at the same time (gm_set_residency)
    const Residency& rs = residency();
    const int cus = chain_cus();
    const int cap = cus > 0 ? usable_cus(cus) / (rs.streams * rs.sharers) : 0;
    if (cap < 1) return GM_E_UNSUP;
    const int grid = most < cap ? most : cap;
    a.vec = kn.vec;
    a.spin_limit = spin_limit();
    a.sync = static_cast<unsigned*>(sync);
    if (ra) {
        const gm_gemm& src = second[0];
        a.e = src.C;
        a.ld_e = src.ld_c;
        a.B = src.M;
        a.C = src.N;
        a.ra_v = ra->ra_v;
        a.ra_s = ra->ra_s;
        a.step = ra->step;
        a.increment = ra->increment;
    }
    switch (kn.form) {
        case 0: k_gemm_chain<4, 8><<<grid, 256, 0, st>>>(a); break;
        case 1: k_gemm_chain<4, 16><<<grid, 256, 0, st>>>(a); break;
        case 2: k_gemm_chain<8, 16><<<grid, 512, 0, st>>>(a); break;
        default: k_gemm_chain<16, 8><<<grid, 1024, 0, st>>>(a); break;
    }
    return check_launch("k_gemm_chain");
}

static int run_chain(const gm_gemm* first, int nfirst, const gm_gemm* second, int nsecond, const RunAvg* ra,
                     void* sync, void* stream) {
    int rc = launch_chain(first, nfirst, second, nsecond, ra, sync, as_stream(stream));
    if (rc != GM_E_UNSUP) return rc;
    // the separate launches, in the chain's order
    if ((rc = gm_gemm_f32(first, nfirst, stream)) != GM_OK) return rc;
    if ((rc = gm_gemm_f32(second, nsecond, stream)) != GM_OK) return rc;
    if (ra)
        rc = gm_mmtm_running_avg_dev(second[0].C, second[0].ld_c, second[0].M, second[0].N, ra->ra_v, ra->ra_s,
                                     ra->step, ra->increment, stream);
    return rc;
}

}  // namespace gm

using namespace gm;

extern "C" size_t gm_gemm_chain_sync_bytes(void) { return kSyncWords * sizeof(unsigned); }

extern "C" int gm_gemm_f32_chain(const gm_gemm* first, int nfirst, const gm_gemm* second, int nsecond, void* sync,
                                 void* stream) {
    if (const int rc = chain_check("gemm_f32_chain", first, nfirst, second, nsecond, sync)) return rc;
    return run_chain(first, nfirst, second, nsecond, nullptr, sync, stream);
}

extern "C" int gm_mmtm_excite_fwd(const gm_gemm* fc1, int nfc1, const gm_gemm* fc2, int nfc2, float* ra_v,
                                  float* ra_s, int* step, int increment, void* sync, void* stream) {
    if (const int rc = chain_check("mmtm_excite_fwd", fc1, nfc1, fc2, nfc2, sync)) return rc;
    for (int i = 0; i < nfc1; ++i)
        GM_REQUIRE(fc1[i].act == 1, "mmtm_excite_fwd: fc1[%d] must end in relu (act 1, got %d)", i, fc1[i].act);
    for (int i = 0; i < nfc2; ++i)
        GM_REQUIRE(fc2[i].act == 2, "mmtm_excite_fwd: fc2[%d] must end in sigmoid (act 2, got %d)", i, fc2[i].act);
    GM_REQUIRE(!ra_v || (ra_s && step), "mmtm_excite_fwd: the running average needs ra_s and step");
    const RunAvg ra = {ra_v, ra_s, step, increment};
    return run_chain(fc1, nfc1, fc2, nfc2, ra_v ? &ra : nullptr, sync, stream);
}

extern "C" int gm_mmtm_excite_bwd(const gm_gemm* first, int nfirst, const gm_gemm* second, int nsecond, void* sync,
                                  void* stream) {
    if (const int rc = chain_check("mmtm_excite_bwd", first, nfirst, second, nsecond, sync)) return rc;
    return run_chain(first, nfirst, second, nsecond, nullptr, sync, stream);
}
