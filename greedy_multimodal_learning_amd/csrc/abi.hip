// ABI housekeeping: version and thread-local error text.
#include <cstdlib>
#include <cstring>

#include "gemm_tile.h"

namespace gm {

static thread_local char g_err[512] = {0};

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return GM_OK;
}

static unsigned g_spin_limit = 0;  // 0: default

unsigned spin_limit() { return g_spin_limit ? g_spin_limit : (1u << 24); }

static Residency g_res = {2, 1, 0};  // two trunk streams, one process, nothing reserved

const Residency& residency() { return g_res; }

int usable_cus(int cus) {
    const int u = cus - g_res.reserved_cus;
    return u > cus / 4 ? u : cus / 4;
}

}  // namespace gm

extern "C" int gm_abi_version(void) { return GM_ABI_VERSION; }

extern "C" int gm_device_faults(unsigned* out, int clear) {
    GM_REQUIRE(out, "gm_device_faults: null out");
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        gm::set_error("gm_device_faults: %s", hipGetErrorString(e));
        return (int)e;
    }
    *out = gm::bn_faults_read(clear != 0) | gm::conv_faults_read(clear != 0) | gm::chain_faults_read(clear != 0);
    return GM_OK;
}

// The fp32 forward convolution with the eval-mode BatchNorm in its epilogue: every argument
// is checked here, before a plan is made or anything is launched.
extern "C" int gm_conv2d_f32_affine(const gm_conv_f32* p, int terms, const float* coef, const float* residual,
                                    int relu, void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "gm_conv2d_f32_affine";
    GM_REQUIRE(p, "%s: null descriptor", fn);
    GM_REQUIRE(p->mode == GM_CONV_FWD, "%s: mode must be GM_CONV_FWD (got %d)", fn, p->mode);
    GM_REQUIRE(!p->accumulate, "%s: accumulate must be 0", fn);
    GM_REQUIRE(!p->addend, "%s: addend must be NULL (a dgrad option)", fn);
    GM_REQUIRE(terms == 0 || terms == 3 || terms == 6,
               "%s: terms must be 0 (exact), 3 (bf16x3) or 6 (bf16x6), got %d", fn, terms);
    GM_REQUIRE(coef, "%s: null coef", fn);
    GM_REQUIRE(reinterpret_cast<uintptr_t>(coef) % 4 == 0, "%s: coef must be 4-byte aligned", fn);
    GM_REQUIRE(reinterpret_cast<uintptr_t>(residual) % 4 == 0, "%s: residual must be 4-byte aligned", fn);
    GM_REQUIRE(p->out, "%s: null out", fn);
    GM_REQUIRE(p->x, "%s: null x", fn);
    GM_REQUIRE(p->w, "%s: null w", fn);
    if (terms == 0) return gm::conv_f32_affine_exact(p, coef, residual, relu, scratch, scratch_bytes, stream);
    return gm::conv_f32_affine_split(p, terms, coef, residual, relu, scratch, scratch_bytes, stream);
}

extern "C" int gm_set_spin_limit(unsigned polls) {
    gm::g_spin_limit = polls;
    return GM_OK;
}
extern "C" const char* gm_last_error(void) { return gm::g_err; }

extern "C" int gm_set_residency(int streams, int sharers, int reserved_cus) {
    GM_REQUIRE(streams >= 1 && streams <= 64, "gm_set_residency: streams must be in [1, 64] (got %d)", streams);
    GM_REQUIRE(sharers >= 1 && sharers <= 64, "gm_set_residency: sharers must be in [1, 64] (got %d)", sharers);
    GM_REQUIRE(reserved_cus >= 0 && reserved_cus <= 4096, "gm_set_residency: reserved_cus out of range (%d)",
               reserved_cus);
    gm::g_res = gm::Residency{streams, sharers, reserved_cus};
    return GM_OK;
}

extern "C" int gm_get_residency(int* streams, int* sharers, int* reserved_cus) {
    GM_REQUIRE(streams && sharers && reserved_cus, "gm_get_residency: null output");
    *streams = gm::g_res.streams;
    *sharers = gm::g_res.sharers;
    *reserved_cus = gm::g_res.reserved_cus;
    return GM_OK;
}
