// Skinny-M GEMM on the fp8 decode weights (W8A16) for batched decode, 5..64 tokens per step:  C[M <= 64, N] = epilogue( scale[n] * (A[M,K] . q[N,K]^T) ).
//
// gemm_skinny_body (k_skinny.h) behind the fp8 weight policy: the 16-bit kernel's grid, K split, x staging (A operand in LDS, 16-bit elements)
// and MFMA sequence, literally.
// The weights are OCP e4m3fn bytes with one power-of-two scale per output row (k_fp8.h).  Each lane loads 8 bytes of one weight row per 32-deep
// step -- the 8 k of B[k = (lane>>4)*8 + j][n = lane&15] that the 16-bit kernel's 16-byte load carries -- converts them (v_cvt_pk_f32_fp8, then
// the pack to the element type: every e4m3fn value is exact in bf16 and in half) and feeds the result to v_mfma_f32_16x16x32 as the B operand.
// Sixteen loads in flight per lane keep the 16-bit kernel's bytes per wave outstanding.  The row scale is applied to the fp32 sum in the ordered
// reduce (skinny_reduce_kernel<.., true>), before bias / residual / SwiGLU.  Scaling by a power of two is exact, so the output is bit for bit
// gemm_skinny_kernel on the dequantised weights q * 2^e (which bf16 holds exactly), provided the K split is the same -- the launcher
// (vl2_gemm_skinny_fp8) picks it from N and K only, so a row's bits do not depend on the other rows of the batch either.
#pragma once
#include "k_fp8.h"
#include "k_skinny.h"

struct Skinny8Args {
    const bf16_t* A;        // [M, lda]
    const uint8_t* Q;       // [N, ldq] e4m3fn bytes
    float* part;            // [KS][Mp][N] fp32 partial sums (unscaled), Mp = 16 * MT
    int M, N, K, lda, ldq;
    int kslice, kchunk;     // K per workgroup (multiple of kchunk), K per LDS chunk (multiple of 32)
};

// 8 e4m3fn bytes (k .. k+7) -> the 8 elements of an MFMA fragment, in order
__device__ __forceinline__ bf16x8 fp8x8_to_frag(u32x2 w) {
    u32x4 o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const vl2_f32x2_t lo = VL2_CVT_PK_F32_FP8(w[h], false), hi = VL2_CVT_PK_F32_FP8(w[h], true);
        o[2 * h] = pack2bf(lo[0], lo[1]);
        o[2 * h + 1] = pack2bf(hi[0], hi[1]);
    }
    return __builtin_bit_cast(bf16x8, o);
}

// gemm_skinny_body's policy for the fp8 weights: 16 x 8 B in flight per lane (the 16-bit kernel's bytes per wave outstanding)
struct SkinnyWFp8 {
    using Args = Skinny8Args;
    static constexpr int NL = 16;
    using word = u32x2;
    const uint8_t* wrow;
    __device__ __forceinline__ SkinnyWFp8(const Args& p, int n, int k0, int lg) : wrow(p.Q + (size_t)n * p.ldq + k0 + lg * 8) {}
    __device__ __forceinline__ word load(int kc, int s) const { return __builtin_nontemporal_load((const u32x2*)(wrow + kc + s * 32)); }
    static __device__ __forceinline__ bf16x8 frag(word w) { return fp8x8_to_frag(w); }
    static __device__ __forceinline__ void at_expert(Args& p, int e, long long stride, long long) { p.Q += (size_t)e * stride; }
};

template <int MT>
__global__ __launch_bounds__(256) void gemm_skinny_fp8_kernel(Skinny8Args p) { gemm_skinny_body<MT, SkinnyWFp8>(p); }
