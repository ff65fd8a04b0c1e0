// Skinny-M GEMM on the fp8 decode weights (W8A16) for batched decode, 5..64 tokens per step:  C[M <= 64, N] = epilogue( scale[n] * (A[M,K] . q[N,K]^T) ).
//
// The fp8 twin of gemm_skinny_kernel (k_skinny.h): the same grid, K split, x staging (A operand in LDS, 16-bit elements) and MFMA sequence.
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

// grid = (N/64, KS), block 256; dynamic LDS = Mp * (kchunk + 8) * 2 bytes
template <int MT>
__global__ __launch_bounds__(256) void gemm_skinny_fp8_kernel(Skinny8Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vl2_smem[];
    constexpr int Mp = 16 * MT;
    constexpr int NL = 16;                                // 8-byte weight loads in flight per lane (the 16-bit kernel: 8 x 16 B)
    bf16_t* xs = (bf16_t*)vl2_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * 64 + wave * 16;
    const int k0 = blockIdx.y * p.kslice;
    const int pitch = p.kchunk + 8;
    const int l15 = lane & 15, lg = lane >> 4;
    const uint8_t* wrow = p.Q + (size_t)(n0 + l15) * p.ldq + k0 + lg * 8;

    f32x4v acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = f32x4v{0.f, 0.f, 0.f, 0.f};

    const int cvec = p.kchunk >> 3;
    for (int kc = 0; kc < p.kslice; kc += p.kchunk) {
        const int nstep = p.kchunk >> 5;
        u32x2 wv[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i)
            if (i < nstep) wv[i] = __builtin_nontemporal_load((const u32x2*)(wrow + kc + i * 32));
        __syncthreads();
        for (int e = tid; e < Mp * cvec; e += 256) {
            const int r = e / cvec, c = e - r * cvec;
            u32x4 v = u32x4{0u, 0u, 0u, 0u};
            if (r < p.M) v = *(const u32x4*)(p.A + (size_t)r * p.lda + k0 + kc + c * 8);
            *(u32x4*)(xs + (size_t)r * pitch + c * 8) = v;
        }
        __syncthreads();
        for (int s0 = 0; s0 < nstep; s0 += NL) {
            if (s0) {
#pragma unroll
                for (int i = 0; i < NL; ++i)
                    if (s0 + i < nstep) wv[i] = __builtin_nontemporal_load((const u32x2*)(wrow + kc + (s0 + i) * 32));
            }
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                if (s0 + i < nstep) {
                    const bf16x8 bfrag = fp8x8_to_frag(wv[i]);
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        const bf16x8 afrag = *(const bf16x8*)(xs + (size_t)(m * 16 + l15) * pitch + (s0 + i) * 32 + lg * 8);
                        acc[m] = VL2_MFMA16(afrag, bfrag, acc[m]);
                    }
                }
            }
        }
    }
    float* dst = p.part + (size_t)blockIdx.y * Mp * p.N;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(size_t)(m * 16 + lg * 4 + r) * p.N + n0 + l15] = acc[m][r];
}
