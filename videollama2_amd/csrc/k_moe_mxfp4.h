// MXFP4 expert weights for the decode step of the Mixtral sparse MoE block: the expert-indexed forms of k_mxfp4.h.
// The expert stacks wgu [E, 2I, D] and wd [E, D, I] are OCP MXFP4: q [E, N, ldq] bytes of two E2M1 codes (k = 2j in bits 3:0) and s [E, N, lds]
// E8M0 bytes, one per 32 k (the block rule of quant_mxfp4_rows_kernel on the [E * N, K] view); activations stay 16-bit (W4A16), products and
// sums are fp32, and the block scale rides in the conversion as in k_mxfp4.h.  Everything but the expert products -- router, attention,
// wqkv / wo, lm_head, the prefill -- keeps its 16-bit weights.
//
//   moe_gemv_gu_mxfp4_kernel    grid = (workgroups of gemv_mxfp4_body, k, S): pair (t, j) runs k_mxfp4.h gemv_mxfp4_body<SWIGLU, .., NP, 1> on token
//                               t's row with expert ids[t][j]'s bytes and scales into a[t * k + j].  S = 1 is the solo step.  A slot is bit for
//                               bit gemv_mxfp4_kernel (SWIGLU, rms_plain) on that expert's matrix: the same body.
//   moe_gemv_down_mxfp4_kernel  grid = (ceil(N / 4), S): moe_gemv_down_mxfp4_body, the MXFP4 form of k_moe_fp8.h moe_gemv_down_fp8_body: one
//                               output row per wave, the KS experts' rows streamed together against their KS staged SwiGLU rows.
//   moe_skinny_reduce_mxfp4_kernel
//                               the reduce of k_moe_skinny.h moe_skinny_kernel<MT, SkinnyWMx4>: k_skinny.h skinny_reduce_body (unscaled: the
//                               fragments already hold E2M1 * 2^e) on the permuted rows that an expert owns.  The 16-bit grouped call's
//                               skinny_reduce_kernel walks all R rows, owned or not, so it does not serve here.
//
// NOT BUILT: a tiled W4A16 grouped GEMM.  The grouped skinny-M form stops at 64 sequences, and so does a batched step on these weights.
#pragma once
#include "k_mxfp4.h"
#include "k_moe_skinny.h"

// grid = (ceil(N / 2 / (4 NP)), k, S), block 256, dynamic LDS = K * 2.  g = gemv_mxfp4_kernel's arguments for expert 0 and token 0 (SWIGLU,
// rms_plain); q_stride / s_stride = bytes between two experts; y row t * k + j, rows lda elements apart.  An id outside [0, E) writes nothing
// (the whole workgroup leaves before the body's barriers).
template <int NP>
__global__ __launch_bounds__(256) void moe_gemv_gu_mxfp4_kernel(Gemv4Args g, const int* __restrict__ ids, long long q_stride, long long s_stride, int E,
                                                                int lda, int ldx) {
    const int j = blockIdx.y, k = gridDim.y, t = blockIdx.z;
    const int e = __builtin_amdgcn_readfirstlane(ids[t * k + j]);
    if ((unsigned)e >= (unsigned)E) return;
    Gemv4Args p = g;
    p.W = g.W + (size_t)e * q_stride;
    p.scale = g.scale + (size_t)e * s_stride;
    p.x = g.x + (size_t)t * ldx;
    p.y = (void*)((bf16_t*)g.y + ((size_t)t * k + j) * lda);
    gemv_mxfp4_body<true, false, NP, 1>(p);
}

// 16-byte vectors (32 codes, one scale block) in flight per lane and expert in the down body.  8 is gemv_mxfp4_body's own depth per weight row
// at NP = 1, so one pass covers K = 64 * 8 * 32 = 16384 (the down projection's K = I = 14336 is one pass).  At KS = 4 that is 4 x 8 x (4 + 1)
// = 160 registers of weights and scale bytes per lane; the resource report shows no scratch at any KS.
constexpr int MOE_MX4_DOWN_DEPTH = 8;

// One output row n per wave, four per workgroup; dynamic LDS = KS * K * 2 (the KS SwiGLU rows a [KS][K]).  Each expert's dot product walks K
// exactly as gemv_mxfp4_body walks a row -- 16-byte vectors of 32 codes with their one scale byte at lane, lane + 64, ..., dwords 0..3 in
// order, each converted by mx4_cvt8 with mx4_scale, four v_dot2 per dword in order -- so d_j = wave_sum(acc_j) is bit for bit
// gemv_mxfp4_kernel<false, true, ..>[n] on expert e_j and row a_j; no multiply follows the sum.  The epilogue is moe_gemv_down_body's:
// o = fma(w_j, d_j, o) in slot order from 0, y[n] = elem(res[n] + o).  K % 32 == 0, any N.
template <int KS>
__device__ __forceinline__ void moe_gemv_down_mxfp4_body(const uint8_t* __restrict__ Q, long long q_stride, int ldq, const uint8_t* __restrict__ S,
                                                         long long s_stride, int lds, const bf16_t* __restrict__ a, const int* __restrict__ ids,
                                                         const float* __restrict__ wts, const bf16_t* __restrict__ res, bf16_t* __restrict__ y, int N,
                                                         int K, int E, int bid) {
#pragma clang fp reassociate(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char vl2_smem[];
    constexpr int DP = MOE_MX4_DOWN_DEPTH;
    bf16_t* as = (bf16_t*)vl2_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* qp[KS];
    const uint8_t* sp[KS];
    float wj[KS];
    bool ok = true;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int e = __builtin_amdgcn_readfirstlane(ids[s]);
        ok = ok && (unsigned)e < (unsigned)E;
        qp[s] = Q + (size_t)e * q_stride;
        sp[s] = S + (size_t)e * s_stride;
        wj[s] = wts[s];
    }
    if (!ok) return;                                               // (uniform over the workgroup: before the barrier)
    for (int v = tid; v < KS * (K >> 3); v += 256) *(u32x4*)(as + (size_t)v * 8) = *(const u32x4*)(a + (size_t)v * 8);
    __syncthreads();
    const int n = bid * 4 + wave;
    if (n >= N) return;
    const int nvec = K >> 5;                                       // 16-B vectors (32 weights, one scale block) per row
    float acc[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) acc[s] = 0.f;
    for (int v0 = 0; v0 < nvec; v0 += 64 * DP) {
        u32x4 wv[KS][DP];
        uint32_t ws[KS][DP];
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < DP; ++i) {
                const int v = v0 + i * 64 + lane;
                if (v < nvec) {
                    wv[s][i] = __builtin_nontemporal_load((const u32x4*)(qp[s] + (size_t)n * ldq + (size_t)v * 16));
                    ws[s][i] = sp[s][(size_t)n * lds + v];
                }
            }
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < DP; ++i) {
                const int v = v0 + i * 64 + lane;
                if (v < nvec) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const u32x4 el = mx4_cvt8(wv[s][i][q], mx4_scale(ws[s][i]));
                        const u32x4 xq = *(const u32x4*)(as + (size_t)s * K + (size_t)v * 32 + 8 * q);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[s] = dot2_bf16(el[j], xq[j], acc[s]);
                    }
                }
            }
    }
    float o = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) o = __builtin_fmaf(wj[s], wave_sum(acc[s]), o);
    if (lane == 0) {
        if (res) o = bf2f(res[n]) + o;
        y[n] = f2bf(o);
    }
}

// grid = (ceil(N / 4), S), block 256: token t runs the body on its KS SwiGLU rows a[t * KS ..], its ids / weights and its residual row (S = 1:
// the solo step).
template <int KS>
__global__ __launch_bounds__(256) void moe_gemv_down_mxfp4_kernel(const uint8_t* __restrict__ Q, long long q_stride, int ldq, const uint8_t* __restrict__ S,
                                                                  long long s_stride, int lds, const bf16_t* __restrict__ a, const int* __restrict__ ids,
                                                                  const float* __restrict__ wts, const bf16_t* __restrict__ res, int ldres,
                                                                  bf16_t* __restrict__ y, int ldy, int N, int K, int E) {
    const int t = blockIdx.y;
    moe_gemv_down_mxfp4_body<KS>(Q, q_stride, ldq, S, s_stride, lds, a + (size_t)t * KS * K, ids + t * KS, wts + t * KS,
                                 res ? res + (size_t)t * ldres : nullptr, y + (size_t)t * ldy, N, K, E, blockIdx.x);
}

// The grouped skinny-M GEMM on the MXFP4 expert weights is k_moe_skinny.h moe_skinny_kernel<MT, SkinnyWMx4>: its grid, K split, staging, MFMA
// order and partials [KS][R][N] are the 16-bit kernel's, and the B fragment is the dequantised weight exactly.  This reduce sums permuted row
// p's partials in slice order (skinny_reduce_body, unscaled) if an expert owns p -- its rows are offs[e] .. offs[e] + counts[e] - 1 -- and
// leaves the row alone otherwise (its partials were never written).  One thread per 4 output columns of one row; p.M = p.Mp = R.
template <bool SWIGLU>
__global__ __launch_bounds__(256) void moe_skinny_reduce_mxfp4_kernel(SkinnyReduceArgs p, const int* __restrict__ counts, const int* __restrict__ offs,
                                                                      int E) {
    const int ncol = SWIGLU ? p.N / 2 : p.N;
    const int per_row = ncol >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.M * per_row) return;
    const int m = i / per_row, c = (i - m * per_row) * 4;
    int e = 0;
    while (e + 1 < E && offs[e + 1] <= m) ++e;
    const int r = m - offs[e];
    if (r < 0 || r >= counts[e]) return;
    skinny_reduce_body<SWIGLU, false, false>(p, m, c, nullptr);
}
