// What the weight-gradient kernels (conv_kern_wgrad4.h, conv_kern_whalo.h, conv_kern_wring.h,
// conv_kern_wstem.h) share: the vector types, the transposed LDS fragment reads, the LDS row
// swizzle and the zero block that padding taps read.
#pragma once
#include <cstdint>
#include <type_traits>

#include "gm_common.h"

namespace gm {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short short4_t __attribute__((ext_vector_type(4)));
typedef short short8_t __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

typedef __attribute__((address_space(3))) short4_t lds_s4;

__device__ __forceinline__ bf16x8 tr_frag(const uint16_t* base_row0, const uint16_t* base_row4) {
    const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)base_row0);
    const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)base_row4);
    const short8_t s = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, s);
}

// ds_read_b64_tr_b16 as inline asm for k_conv_wgrad4: the builtin form makes hipcc wait
// vmcnt(0) for every LDS-DMA in flight before each transposed read (it cannot tell the
// DMA's LDS destination from the read's buffer), which serialised the next step's DMA with
// this step's MFMAs.  The asm reads are invisible to the compiler's lgkmcnt tracking, so
// the caller waits for them explicitly (wait_lgkm0 on the fragments it is about to use).
template <int OFF>
__device__ __forceinline__ short4_t tr_rd(unsigned a) {
    short4_t d;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(a), "i"(OFF));
    return d;
}

__device__ __attribute__((aligned(16))) const uint4 g_wzero16[1] = {{0u, 0u, 0u, 0u}};

// 16-B chunk XOR of an LDS row, applied on the source side of a DMA or store: keeps the tr-read
// half-waves conflict-free (k_conv_wgrad4's comment)
template <int RB>  // row bytes (128 or 256)
__device__ __forceinline__ int wswz(int row) {
    return RB >= 256 ? 4 * (row & 3) : 4 * ((row >> 1) & 1);
}
}  // namespace gm
