// fp8 expert weights for the decode step of the Mixtral sparse MoE block: the expert-indexed forms of k_fp8.h and
// k_skinny_fp8.h.  The expert stacks wgu [E, 2I, D] and wd [E, D, I] are OCP e4m3fn bytes q [E, N, K] with one power-of-two fp32 scale per
// expert and output row, scale [E, N] (the row rule of quant_fp8_rows_kernel on the [E * N, K] view); activations stay 16-bit (W8A16),
// products and sums are fp32.  Everything but the expert products -- router, attention, wqkv / wo, lm_head, the prefill -- keeps its 16-bit
// weights.
//
//   moe_gemv_gu_fp8_kernel    grid = (workgroups of gemv_fp8_body, k, S): pair (t, j) runs k_fp8.h gemv_fp8_body<SWIGLU, .., NP, 1> on token t's
//                             row with expert ids[t][j]'s bytes and scales into a[t * k + j].  S = 1 is the solo step.  A slot is bit for bit
//                             gemv_fp8_kernel (SWIGLU, rms_plain) on that expert's matrix: the same body.
//   moe_gemv_down_fp8_kernel  grid = (ceil(N / 4), S): moe_gemv_down_fp8_body, the fp8 form of k_moe.h moe_gemv_down_body: one output row per
//                             wave, the KS experts' rows streamed together against their KS staged SwiGLU rows.
//   moe_skinny_reduce_fp8_kernel
//                             the reduce of k_moe_skinny.h moe_skinny_kernel<MT, SkinnyWFp8>: k_skinny.h skinny_reduce_body on permuted row p with
//                             the scale row of p's expert, found from offs on the device.  Rows no expert owns are not written.
#pragma once
#include "k_fp8.h"
#include "k_moe_skinny.h"
#include "k_skinny_fp8.h"

// grid = (ceil(N / 2 / (4 NP)), k, S), block 256, dynamic LDS = K * 2.  g = gemv_fp8_kernel's arguments for expert 0 and token 0 (SWIGLU,
// rms_plain); q_stride / s_stride = bytes / floats between two experts; y row t * k + j, rows lda elements apart.  An id outside [0, E) writes
// nothing (the whole workgroup leaves before the body's barriers).
template <int NP>
__global__ __launch_bounds__(256) void moe_gemv_gu_fp8_kernel(Gemv8Args g, const int* __restrict__ ids, long long q_stride, long long s_stride, int E,
                                                              int lda, int ldx) {
    const int j = blockIdx.y, k = gridDim.y, t = blockIdx.z;
    const int e = __builtin_amdgcn_readfirstlane(ids[t * k + j]);
    if ((unsigned)e >= (unsigned)E) return;
    Gemv8Args p = g;
    p.W = g.W + (size_t)e * q_stride;
    p.scale = g.scale + (size_t)e * s_stride;
    p.x = g.x + (size_t)t * ldx;
    p.y = (void*)((bf16_t*)g.y + ((size_t)t * k + j) * lda);
    gemv_fp8_body<true, false, NP, 1>(p);
}

// One output row n per wave, four per workgroup; dynamic LDS = KS * K * 2 (the KS SwiGLU rows a [KS][K]).  Each expert's dot product walks K
// exactly as gemv_fp8_body walks a row -- 16-byte vectors of 16 weights at lane, lane + 64, ..., each dword converted by v_cvt_pk_f32_fp8 and
// packed to two element pairs once, the low pair's v_dot2 before the high pair's -- so d_j = scale[e_j][n] * wave_sum(acc_j) is bit for bit
// gemv_fp8_kernel<false, true, ..>[n] on expert e_j and row a_j.  The epilogue is moe_gemv_down_body's: o = fma(w_j, d_j, o) in slot order
// from 0, y[n] = bf16(res[n] + o).  Loads in flight per lane: KS x 8 x 16 B, the 16-bit body's bytes (the stream is bound by them); one trip
// covers K = 8192.  K % 16 == 0.
template <int KS>
__device__ __forceinline__ void moe_gemv_down_fp8_body(const uint8_t* __restrict__ Q, long long q_stride, int ldq, const float* __restrict__ scale,
                                                       long long s_stride, const bf16_t* __restrict__ a, const int* __restrict__ ids,
                                                       const float* __restrict__ wts, const bf16_t* __restrict__ res, bf16_t* __restrict__ y, int N,
                                                       int K, int E, int bid) {
#pragma clang fp reassociate(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char vl2_smem[];
    bf16_t* as = (bf16_t*)vl2_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* qp[KS];
    const float* sp[KS];
    float wj[KS];
    bool ok = true;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int e = __builtin_amdgcn_readfirstlane(ids[s]);
        ok = ok && (unsigned)e < (unsigned)E;
        qp[s] = Q + (size_t)e * q_stride;
        sp[s] = scale + (size_t)e * s_stride;
        wj[s] = wts[s];
    }
    if (!ok) return;                                               // (uniform over the workgroup: before the barrier)
    for (int v = tid; v < KS * (K >> 3); v += 256) *(u32x4*)(as + (size_t)v * 8) = *(const u32x4*)(a + (size_t)v * 8);
    __syncthreads();
    const int n = bid * 4 + wave;
    if (n >= N) return;
    const int nvec = K >> 4;                                       // 16-B vectors (16 weights) per row
    float acc[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) acc[s] = 0.f;
    for (int v0 = 0; v0 < nvec; v0 += 64 * 8) {
        u32x4 wv[KS][8];
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int v = v0 + i * 64 + lane;
                if (v < nvec) wv[s][i] = __builtin_nontemporal_load((const u32x4*)(qp[s] + (size_t)n * ldq + (size_t)v * 16));
            }
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int v = v0 + i * 64 + lane;
                if (v < nvec) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const vl2_f32x2_t wl = VL2_CVT_PK_F32_FP8(wv[s][i][q], false), wh = VL2_CVT_PK_F32_FP8(wv[s][i][q], true);
                        const uint32_t el = pack2bf(wl[0], wl[1]), eh = pack2bf(wh[0], wh[1]);
                        const u32x2 xq = *(const u32x2*)(as + (size_t)s * K + (size_t)v * 16 + 4 * q);
                        acc[s] = dot2_bf16(el, xq[0], acc[s]);
                        acc[s] = dot2_bf16(eh, xq[1], acc[s]);
                    }
                }
            }
    }
    float o = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        float d = wave_sum(acc[s]);
        d *= sp[s][n];
        o = __builtin_fmaf(wj[s], d, o);
    }
    if (lane == 0) {
        if (res) o = bf2f(res[n]) + o;
        y[n] = f2bf(o);
    }
}

// grid = (ceil(N / 4), S), block 256: token t runs the body on its KS SwiGLU rows a[t * KS ..], its ids / weights and its residual row (S = 1:
// the solo step).
template <int KS>
__global__ __launch_bounds__(256) void moe_gemv_down_fp8_kernel(const uint8_t* __restrict__ Q, long long q_stride, int ldq, const float* __restrict__ scale,
                                                                long long s_stride, const bf16_t* __restrict__ a, const int* __restrict__ ids,
                                                                const float* __restrict__ wts, const bf16_t* __restrict__ res, int ldres,
                                                                bf16_t* __restrict__ y, int ldy, int N, int K, int E) {
    const int t = blockIdx.y;
    moe_gemv_down_fp8_body<KS>(Q, q_stride, ldq, scale, s_stride, a + (size_t)t * KS * K, ids + t * KS, wts + t * KS,
                               res ? res + (size_t)t * ldres : nullptr, y + (size_t)t * ldy, N, K, E, blockIdx.x);
}

// The grouped skinny-M GEMM on the fp8 expert weights is k_moe_skinny.h moe_skinny_kernel<MT, SkinnyWFp8>: its grid, K split, staging, MFMA
// order and partials [KS][R][N] are the 16-bit kernel's.  This reduce sums permuted row p's partials in slice order and multiplies GEMM column
// n's sum by scale[e(p)][n] before the SwiGLU or the store (skinny_reduce_body<.., SCALED>), e(p) = the expert whose rows offs[e] .. offs[e] +
// counts[e] - 1 hold p.  One thread per 4 output columns of one row; p.M = p.Mp = R, p.scale = expert 0's scale row.  A row that no expert
// owns (its partials were never written) is left alone.
template <bool SWIGLU>
__global__ __launch_bounds__(256) void moe_skinny_reduce_fp8_kernel(SkinnyReduceArgs p, const int* __restrict__ counts, const int* __restrict__ offs, int E,
                                                                    long long s_stride) {
    const int ncol = SWIGLU ? p.N / 2 : p.N;
    const int per_row = ncol >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.M * per_row) return;
    const int m = i / per_row, c = (i - m * per_row) * 4;
    int e = 0;
    while (e + 1 < E && offs[e + 1] <= m) ++e;
    const int r = m - offs[e];
    if (r < 0 || r >= counts[e]) return;
    skinny_reduce_body<SWIGLU, false, true>(p, m, c, p.scale + (size_t)e * s_stride);
}
