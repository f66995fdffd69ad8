// The one-line lane helpers of the MFMA kernels, written once: the 32x32 accumulator's row of a register, the 32-bit-offset
// load, the opaque lane copy, the tagged granule store of the persistent kernels and the 16-bit MFMA, with the vector types
// they need.  Every unit that used to carry its own copy includes this header.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));   // native vector: stays in VGPRs
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(1))) unsigned long long gu64;

// An opaque copy of a lane-dependent value: address arithmetic derived from it cannot be hoisted out of the layer
// loop (hoisted per-lane offsets of the staging / epilogue sections would push the resident tile into scratch).
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// base[idx] with the byte offset formed in 32 bits, so the load takes the (SGPR base + 32-bit VGPR offset) form instead of
// a 64-bit VGPR address per element (64 of those in flight would not fit the register file).  idx < 2^30.
__device__ __forceinline__ float ldg(const float* base, unsigned idx) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + (size_t)(idx * 4u));
}

// Row of accumulator register r within a 32x32 MFMA C tile (the column is lane & 31).
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// One 8-byte {layer tag, value} granule of the persistent kernels' halo exchange: a relaxed agent-scope store, tag and
// value in one instruction, so a neighbour that sees the tag has the value.
__device__ __forceinline__ void store_granule(unsigned long long* g, unsigned tag, float v) {
    __hip_atomic_store((gu64*)g, ((unsigned long long)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// v_mfma_f32_32x32x16_{bf16,f16} on fragments carried as four dwords: MODE 1 = bf16, anything else = fp16.
template <int MODE>
__device__ __forceinline__ f32x16 mma16(const u32x4& a, const u32x4& b, const f32x16& c) {
    if (MODE == 1)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
