// Device helpers shared by the fused residual-block kernel sources (preact_*.hip, tiny_block.hip,
// wgrad_ds.hip).  One definition each: a fix here reaches every kernel that uses it.
#pragma once
#include "common.h"

namespace vq3d {

// circular wrap of an index at most one period outside [0, n)
__device__ __forceinline__ int wrapm(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// ELU on the hardware exp (v_exp_f32 of z log2 e: ~1e-7 relative, far inside the 16-bit rounding
// that follows every use; the libm expf of common.h's elu is ~10 instructions)
__device__ __forceinline__ float elu_fast(float z) { return z > 0.f ? z : __expf(z) - 1.f; }
__device__ __forceinline__ float elu_d_act(float t, float b) {  // elu'(z) from t = elu(z) + b
    const float z1 = t - b;
    return z1 > 0.f ? 1.f : z1 + 1.f;
}

// the block's eight scalar parameters in registers
struct Scal {
    float b1a, b1b, b2a, b2b, b3a, b3b, sc, b4;
};
__device__ __forceinline__ Scal load_scal(const vq3d_preact_params &p) {
    return Scal{*p.bias1a, *p.bias1b, *p.bias2a, *p.bias2b, *p.bias3a, *p.bias3b, *p.scale, *p.bias4};
}

__device__ __forceinline__ f32x4 mfma(hx8 a, hx8 b, f32x4 c) {
    return VQ3D_MFMA_16X16X32(a, b, c, 0, 0, 0);
}

// 8 fp32 values rounded to one MFMA operand fragment
__device__ __forceinline__ hx8 pack8(const float (&v)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = pk2(v[2 * j], v[2 * j + 1]);
    return __builtin_bit_cast(hx8, uint4{w[0], w[1], w[2], w[3]});
}

// 8 consecutive 16-bit elements from LDS at element offset `off` of a 4-byte aligned base (any
// parity): five dwords + v_alignbyte
__device__ __forceinline__ hx8 read8(const h16_t *base, int off) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(base + (off & ~1));
    const uint32_t sh = uint32_t(off & 1) * 2u;
    const uint32_t u0 = q[0], u1 = q[1], u2 = q[2], u3 = q[3], u4 = q[4];
    const uint4 r = {__builtin_amdgcn_alignbyte(u1, u0, sh), __builtin_amdgcn_alignbyte(u2, u1, sh),
                     __builtin_amdgcn_alignbyte(u3, u2, sh), __builtin_amdgcn_alignbyte(u4, u3, sh)};
    return __builtin_bit_cast(hx8, r);
}

}  // namespace vq3d
